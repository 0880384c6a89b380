"""numpy yardstick of altro_batch_evaluate_grad: the penalty P = 1/2 sum r^2, the gradient of M = J + rho P with respect to the
controls and the initial state from given (X, U), the rounding bounds the tests hold it to, and the distance of every row value
from its kink.  The cases and helpers are those of tests/evaluate_ref.py (ER).  Shared by tests/test_evaluate_grad_api.py (this
yardstick against the CPU oracle) and tests/test_evaluate_grad_gpu.py (the device against this yardstick).

Definitions (include/altro_batch.h): r per row = BOX max(0, z - hi), max(0, lo - z) on finite sides (state columns only at knot
N-1); LINEAR v (equality), max(0, v) (inequality); SOC the vector v - Proj(v).  c_k = sum_rows a_r r_r (BOX: +r_hi - r_lo on the
element).  lambda_{N-1} = Qf e_x + rho c_x; gU_k = dt R e_u + rho c_u + B_k' lambda_{k+1}; lambda_k = dt Q e_x + rho c_x + A_k'
lambda_{k+1}; gx0 = lambda_0.

Bounds (u = 2^-53), all derived, none measured.  E_r is ER's bound 4 of the row (between two computations of the row value from
the same doubles): 2 (nz + 2) u (|a_r||z| + |b_r|) for a LINEAR row, 2 u (|z| + |bound|) for a BOX side, sqrt(p) max E + 16 u |v|_2
for every element of a cone's residual (v -> v - Proj(v) is nonexpansive).  max(0, .) and the identity are 1-Lipschitz, so two
computations of r differ by at most E_r wherever they pick the same side, which the margins below make sure of.
 5. P.  |r1^2 - r2^2| <= E (2 |r| + E), and a sum of T products has relative error (T + 2) u in each computation:
      Pb = sum (|r| E_r + E_r^2 / 2) + 2 (T + 3) u P                                  (between two computations)
 6. gradient.  Each element of lambda is a chain of at most g = n + rows + 4 operations (w e, rho c, `rows` terms of the
    pullback, n terms of the transposed product), so with gamma = g u the reverse recursion run on absolute values bounds one
    computation:
      dL_k <= |A_k|' dL_{k+1} + gamma (|w e_x| + rho |C|'|r| + |A_k|'|lambda_{k+1}|) + rho |C|' E_r
    and the same for gU_k with B_k and e_u.  The tests allow twice that between two computations.
 7. states that are themselves rounded (a rollout: bound 1 of ER, d_{k+1} <= |A| d_k + (nz + 2) u S_k, d_0 = 0) move every row
    value by at most |a_r| d and every e_x by d: with `state_err` = d these enter E_r and the local term, so the same recursion
    bounds the gradient at the exact states; M itself moves by at most sum_k |w e_x + rho c_x|_k . d_k (first order in u).
 8. central differences.  M is quadratic along a line wherever no row changes side, EXCEPT through a cone value on the boundary
    branch: there 1/2 |v - Proj(v)|^2 = (|s| - t)^2 / 4, and |s| is not a polynomial.  Along v + tau dv, with ds = |dv_s| and
    dt = |dv_t|: the second derivative of |s| is at most ds^2 / |s| and the third at most 1.155 ds^3 / |s|^2, so the third
    derivative of the row's term is at most (3 dt ds^2 / |s| + 1.155 |t| ds^3 / |s|^2) / 2.  For |tau| <= hmax / 2 (hmax <=
    |s| / (ds + dt)) |s| stays above half its value at tau = 0 and |t| below |t| + |s| / 2 of that point:
      f3 = 3 dt ds^2 / |s| + 2.31 (|t| + |s| / 2) ds^3 / |s|^2,
    summed over the boundary-branch cone values, bounds it on the segment, and a central difference with step h is off by at
    most rho h^2 f3 / 6.  Every other row contributes nothing.
Margins: per (b, c) the smallest distance of any row value from its kink -- 0 for a BOX side or an inequality row; ||s|| - t,
||s|| + t and ||s|| for a cone -- in units of that row's E_r.
"""
from types import SimpleNamespace as NS

import numpy as np

import evaluate_ref as ER

U_ = ER.U_


def stack_z(cs, X, U):
    B, nc = U.shape[:2]
    Z = np.zeros((B, nc, cs.N, cs.n + cs.m))
    Z[..., :cs.n] = X
    Z[:, :, :-1, cs.n:] = U
    return Z


def tangent(cs, dU, dx0=None):
    """dX (B, nc, N, n): the rollout's derivative along (dU, dx0)"""
    B, nc = dU.shape[:2]
    dX = np.zeros((B, nc, cs.N, cs.n))
    if dx0 is not None:
        dX[:, :, 0] = dx0
    for k in range(cs.N - 1):
        dX[:, :, k + 1] = np.einsum("bij,bcj->bci", cs.A[:, k], dX[:, :, k]) + np.einsum("bij,bcj->bci", cs.Bm[:, k], dU[:, :, k])
    return dX


def rollout_error(cs, X, U):
    """bound 7: d (B, nc, N, n), how far the states of a rounded rollout can be from the exact rollout of the same controls"""
    _, S = ER.step_residual(cs, X, U)
    d = np.zeros(X.shape)
    for k in range(cs.N - 1):
        d[:, :, k + 1] = np.einsum("bij,bcj->bci", np.abs(cs.A[:, k]), d[:, :, k]) + (cs.n + cs.m + 2) * U_ * S[:, :, k]
    return d


def merit_grad(cs, X, U, rho, cons=None, Xref=None, Uref=None, direction=None, state_err=None):
    """P, gU, gx0 of (X, U) (B, nc, ..) with their bounds Pb (5; between two computations), gUb, gx0b (6; one computation),
    margin (B, nc), nact (B, nc) the number of rows with r != 0, branch (B, nc, 3) the cone values inside / polar / boundary,
    Lx (B, nc, N, n) the local term w e_x + rho c_x.  direction = (dX, dU): also hmax (B, nc), the largest step along it for
    which no row value reaches its kink, and f3 (B, nc) of bound 8."""
    cons = cs.cons if cons is None else cons
    Xr = cs.Xref if Xref is None else Xref
    Ur = cs.Uref if Uref is None else Uref
    B, nc = U.shape[:2]
    n, m, N = cs.n, cs.m, cs.N
    nz = n + m
    Z = stack_z(cs, X, U)
    dZs = np.zeros(Z.shape)
    if state_err is not None:
        dZs[..., :n] = state_err
    dirZ = None if direction is None else stack_z(cs, direction[0], direction[1])
    C, Ca, CE = np.zeros(Z.shape), np.zeros(Z.shape), np.zeros(Z.shape)
    P, Perr, terms = np.zeros((B, nc)), np.zeros((B, nc)), 0
    margin, hmax, f3 = np.full((B, nc), np.inf), np.full((B, nc), np.inf), np.zeros((B, nc))
    nact, branch = np.zeros((B, nc), dtype=int), np.zeros((B, nc, 3), dtype=int)
    rows = 2
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in cons:
            rows += 0 if c.kind == "box" else c.A.shape[2]
            for k in range(c.k0, c.k1 + 1):
                z = Z[:, :, k]
                if c.kind == "box":
                    cols = n if k == N - 1 else nz
                    zc = z[..., :cols]
                    for sign, side in ((1.0, c.zmax), (-1.0, c.zmin)):
                        bnd = side[:, None, :cols]
                        fin = np.broadcast_to(np.isfinite(bnd), zc.shape)
                        bf = np.where(fin, bnd, 0.0)
                        d = np.where(fin, sign * (zc - bf), -1.0)
                        r = np.where(fin, np.maximum(d, 0.0), 0.0)
                        E = np.where(fin, 2 * U_ * (np.abs(zc) + np.abs(bf)) + dZs[:, :, k, :cols], 0.0)
                        C[:, :, k, :cols] += sign * r
                        Ca[:, :, k, :cols] += r
                        CE[:, :, k, :cols] += E
                        P += 0.5 * (r * r).sum(axis=-1)
                        Perr += (r * E + 0.5 * E * E).sum(axis=-1)
                        terms += cols
                        margin = np.minimum(margin, np.where(fin, np.abs(d) / E, np.inf).min(axis=-1))
                        nact += (r != 0.0).sum(axis=-1)
                        if dirZ is not None:
                            hmax = np.minimum(hmax, np.where(fin, np.abs(d) / np.abs(dirZ[:, :, k, :cols]), np.inf).min(axis=-1))
                    continue
                Ak, bk = c.A[:, k - c.k0], c.b[:, k - c.k0]
                v = np.einsum("bpj,bcj->bcp", Ak, z) + bk[:, None]
                E = (2 * (nz + 2) * U_ * (np.einsum("bpj,bcj->bcp", np.abs(Ak), np.abs(z)) + np.abs(bk)[:, None])
                     + np.einsum("bpj,bcj->bcp", np.abs(Ak), dZs[:, :, k]))
                dv = None if dirZ is None else np.einsum("bpj,bcj->bcp", Ak, dirZ[:, :, k])
                p = v.shape[-1]
                terms += p
                if c.kind == "lin":
                    r = v if c.eq else np.maximum(v, 0.0)
                    Er = E
                    if not c.eq:
                        margin = np.minimum(margin, (np.abs(v) / E).min(axis=-1))
                        if dv is not None:
                            hmax = np.minimum(hmax, (np.abs(v) / np.abs(dv)).min(axis=-1))
                else:
                    s, t = v[..., :-1], v[..., -1]
                    ns = np.linalg.norm(s, axis=-1)
                    inside = ns <= t
                    polar = ~inside & (ns <= -t)
                    bdry = ~inside & ~polar
                    cc = np.where(ns > 0, 0.5 * (1 + t / ns), 0.0)
                    rb = np.concatenate(((1 - cc)[..., None] * s, (t - cc * ns)[..., None]), axis=-1)
                    r = np.where(inside[..., None], 0.0, np.where(polar[..., None], v, rb))
                    Ec = np.sqrt(p) * E.max(axis=-1) + 16 * U_ * np.linalg.norm(v, axis=-1)
                    Er = np.broadcast_to(Ec[..., None], v.shape)
                    kink = np.minimum(np.minimum(np.abs(ns - t), np.abs(ns + t)), ns)
                    margin = np.minimum(margin, kink / Ec)
                    for i, w in enumerate((inside, polar, bdry)):
                        branch[..., i] += w
                    if dv is not None:
                        ds, dt = np.linalg.norm(dv[..., :-1], axis=-1), np.abs(dv[..., -1])
                        hmax = np.minimum(hmax, kink / (ds + dt))
                        f3 += np.where(bdry, 3 * dt * ds ** 2 / ns + 2.31 * (np.abs(t) + 0.5 * ns) * ds ** 3 / ns ** 2, 0.0)
                C[:, :, k] += np.einsum("bpj,bcp->bcj", Ak, r)
                Ca[:, :, k] += np.einsum("bpj,bcp->bcj", np.abs(Ak), np.abs(r))
                CE[:, :, k] += np.einsum("bpj,bcp->bcj", np.abs(Ak), Er)
                P += 0.5 * (r * r).sum(axis=-1)
                Perr += (np.abs(r) * Er + 0.5 * Er * Er).sum(axis=-1)
                nact += (r != 0.0).sum(axis=-1)
    Pb = Perr + 2 * (terms + 3) * U_ * P
    gam = (n + rows + 4) * U_
    ex, eu = X - Xr[:, None], U - Ur[:, None]
    wx = np.broadcast_to((cs.dt * cs.Q)[:, None, None], ex.shape).copy()
    wx[:, :, -1] = cs.Qf[:, None]
    wu = (cs.dt * cs.R)[:, None, None]
    Lx, Lu = wx * ex + rho * C[..., :n], wu * eu + rho * C[:, :, :-1, n:]
    Lax, Lau = np.abs(wx * ex) + rho * Ca[..., :n], np.abs(wu * eu) + rho * Ca[:, :, :-1, n:]
    Dx, Du = rho * CE[..., :n] + wx * dZs[..., :n], rho * CE[:, :, :-1, n:]
    gU, gUb = np.zeros(U.shape), np.zeros(U.shape)
    lam, dlam = Lx[:, :, -1], gam * Lax[:, :, -1] + Dx[:, :, -1]
    T = lambda M, v: np.einsum("bij,bci->bcj", M, v)
    for k in range(N - 2, -1, -1):
        A, Bm = cs.A[:, k], cs.Bm[:, k]
        gU[:, :, k] = Lu[:, :, k] + T(Bm, lam)
        gUb[:, :, k] = T(np.abs(Bm), dlam) + gam * (Lau[:, :, k] + T(np.abs(Bm), np.abs(lam))) + Du[:, :, k]
        lam, dlam = (Lx[:, :, k] + T(A, lam),
                     T(np.abs(A), dlam) + gam * (Lax[:, :, k] + T(np.abs(A), np.abs(lam))) + Dx[:, :, k])
    return NS(P=P, Pb=Pb, gU=gU, gUb=gUb, gx0=lam, gx0b=dlam, margin=margin, nact=nact, branch=branch, Lx=Lx, hmax=hmax, f3=f3)


def merit(cs, X, U, rho, **kw):
    """(M, Mb) of (X, U): ER.cost's J and bound 3 plus rho times P and bound 5 (between two computations)"""
    J, Jb = ER.cost(cs, X, U, Xref=kw.get("Xref"), Uref=kw.get("Uref"))
    g = merit_grad(cs, X, U, rho, **kw)
    return J + rho * g.P, Jb + rho * g.Pb


def fd_step(g, rho, Mb):
    """the step of a central difference along the direction g = merit_grad(.., direction=..) was given: half the distance to the
    nearest kink, at most 1; with cone values on the boundary branch also at most the step that balances bound 8's truncation
    rho h^2 f3 / 6 against the rounding Mb / h of the two merits (any step below hmax / 2 is valid: the tolerance follows it)"""
    h = np.minimum(0.5 * g.hmax, 1.0)
    with np.errstate(divide="ignore"):
        return np.where(rho * g.f3 > 0, np.minimum(h, np.cbrt(3 * Mb / (rho * g.f3))), h)


def fd_truncation(g, rho, h):
    """bound 8"""
    return rho * h * h * g.f3 / 6


def candidates_with_polar(cs, seed):
    """ER.candidates, and for ER.case_wide_cone a fourth candidate: candidate 2 with knot 1's control set to (0.1, 0.1, -6), which
    puts the cone value of that knot into the polar cone by construction (t = 0.5 * -6 + 2 = -1, ||s|| = 0.141)"""
    U = ER.candidates(cs, seed)
    if (cs.n, cs.m) != (7, 3):
        return U
    extra = U[:, 2:3].copy()
    extra[:, 0, 1] = (0.1, 0.1, -6.0)
    return np.ascontiguousarray(np.concatenate((U, extra), axis=1))
