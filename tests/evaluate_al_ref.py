"""numpy yardstick of altro_batch_evaluate_al: the solver's augmented Lagrangian L_A(U; lambda, mu) from given (X, U), duals and
penalty, its gradient with respect to the controls and the initial state, its partial derivatives with respect to the problem
data, the rounding bounds the tests hold all of it to, and the branch counts the tests assert on.  The cases and helpers are
those of tests/evaluate_ref.py (ER) and tests/evaluate_grad_ref.py (GR).  Shared by tests/test_evaluate_al_api.py (this yardstick
against the CPU oracle) and tests/test_evaluate_al_gpu.py (the device against this yardstick).

Definitions (include/altro_batch.h): per BOX finite side / LINEAR row of value c and dual l: phi = l c + [a] mu c^2 / 2 with
a = equality | c >= 0 | l > 0, g = l + [a] mu c; per cone of values v and duals l: psi = (|y|^2 - |l|^2) / (2 mu) with
y = Proj_K(l - mu v), pulled back as -A'y.  L_A = J + sum phi + sum psi.  c_k = the pullback sum; lam_{N-1} = Qf e_x + c_x;
gU_k = dt R e_u + c_u + B_k' lam_{k+1}; lam_k = dt Q e_x + c_x + A_k' lam_{k+1}; gx0 = lam_0.  gXref = -(w e_x), gUref =
-(dt R e_u); gQ = dt/2 sum_{k<N-1} e_x^2, gR = dt/2 sum e_u^2, gQf = e_{x,N-1}^2 / 2; gzmax = -sum_k g_hi, gzmin = sum_k g_lo.
Duals: one array per constraint of the case, BOX (B, nk, 2, nz) (side 0 the upper side), LINEAR / SOC (B, nk, p).

Bounds (u = 2^-53), all derived, none measured.  E_r is ER's bound 4 of the row value (GR's docstring), between two
computations of it from the same doubles, plus |a_r| d for states that are off by d (GR's bound 7).
 A. g of a linear term.  c -> l + [a] mu c is continuous (at c = 0 the two sides agree: a switches only where l <= 0, and for
    l < 0 an inequality row is inactive below 0 and g = l on both sides of it) and mu-Lipschitz, so two computations differ by
    at most mu E_r wherever they stand relative to the kink -- this is the rounding of mu c near zero -- plus one rounding of
    the fused multiply-add in each: Eg = mu E_r + 2 u |g|.
 B. phi is C^1 with derivative g, so two computations of it differ by at most (|g| + mu E_r) E_r, plus the roundings of
    l * c (one) and 0.5 * (mu * (c * c)) (two) in each: 2 u |l c| + 4 u mu c^2 / 2.
 C. cone.  w = l - mu v is off by mu E + 2 u |w| per element; Proj_K is nonexpansive in the 2-norm and its evaluation adds
    16 u |w|_2 (ER's bound 4): Ey = sqrt(p) (mu max E + 2 u max |w|) + 16 u |w|_2 for every element of y.  psi is C^1 in v with
    gradient -y: two computations differ by at most (|y|_2 + sqrt(p) Ey) sqrt(p) (max E + Eyr / mu), Eyr the part of Ey that
    is rounding alone, plus (p + 6) u (|y|^2 + |l|^2) / (2 mu) in each for the products, the sums and the division.
 D. L_A.  J by ER's bound 3; the T terms of sum phi and the lanes of sum psi are added in some order: 2 (T + 3) u sum |term|.
 E. gradient.  GR's bound 6 with Eg (A) resp. Ey (C) in place of rho E_r: the chain has g = n + rows + 4 operations.
 F. data.  gXref, gUref: one subtraction, one product: 4 u |w e| (+ w d).  gQ, gR: a sum of N - 1 rounded squares times dt / 2:
    2 (N + 4) u gQ (+ dt sum |e| d).  gQf: 4 u gQf (+ |e| d).  gzmax, gzmin: sum_k Eg + 2 (nk + 1) u sum_k |g|.
 G. central differences.  L_A is quadratic along a line wherever no row changes side, except through a cone value on the
    boundary branch, where (|s| + t)^2 / (4 mu) of w = l - mu v takes GR's bound 8 with dw = mu dv and the factor 1 / mu.  The
    kinks a step must not cross: c = 0 for a BOX side or inequality row with l <= 0 (with l > 0 the row is active on both
    sides: no kink), and |s| = t, |s| = -t, |s| = 0 of w for a cone.
"""
from types import SimpleNamespace as NS

import numpy as np

import evaluate_ref as ER
import evaluate_grad_ref as GR

U_ = ER.U_
OUTS = ("LA", "J", "gU", "gx0", "gXref", "gUref", "gQ", "gQf", "gR", "gzmin", "gzmax")


def case_16_soc_eq(B=5, N=9, seed=12):
    """ER.case_16_soc with its LINEAR row an equality"""
    cs = ER.case_16_soc(B, N, seed)
    cs.cons[-1].eq = True
    return cs


def zero_duals(cs):
    return [np.zeros((cs.B, c.k1 - c.k0 + 1, 2, cs.n + cs.m)) if c.kind == "box" else np.zeros((cs.B, c.k1 - c.k0 + 1, c.A.shape[2]))
            for c in cs.cons]


def finite_sides(cs, c):
    """(B, nk, 2, nz) bool: the sides of a BOX that exist (state columns only at knot N-1)"""
    fin = np.stack((np.isfinite(c.zmax), np.isfinite(c.zmin)), axis=1)[:, None]
    fin = np.broadcast_to(fin, (cs.B, c.k1 - c.k0 + 1, 2, cs.n + cs.m)).copy()
    if c.k1 == cs.N - 1:
        fin[:, -1, :, cs.n:] = False
    return fin


def draw_duals(cs, lam, mu, seed):
    """the recipe that reaches every branch: of the duals a solve left keep a third, zero a third and redraw a third -- mu U(0, 1)
    for BOX and inequality rows, either sign for equality rows, 3 mu U(0, 1) (0.3 d, 1) with d a unit vector for cones (whole
    cones at a time).  Zero on infinite box sides."""
    rng = np.random.default_rng(seed)
    out = []
    for c, l in zip(cs.cons, lam):
        l = np.array(l, dtype=np.float64)
        m_ = mu.reshape((-1,) + (1,) * (l.ndim - 1))
        if c.kind == "soc":
            pick = rng.integers(0, 3, l.shape[:-1])[..., None]
            d = rng.standard_normal(l.shape[:-1] + (l.shape[-1] - 1,))
            d /= np.linalg.norm(d, axis=-1, keepdims=True)
            new = 3 * m_ * rng.random(l.shape[:-1] + (1,)) * np.concatenate((0.3 * d, np.ones(l.shape[:-1] + (1,))), axis=-1)
        else:
            pick = rng.integers(0, 3, l.shape)
            new = m_ * rng.random(l.shape)
            if c.kind == "lin" and c.eq:
                new = new * np.where(rng.random(l.shape) < 0.5, -1.0, 1.0)
        l = np.where(pick == 0, l, np.where(pick == 1, 0.0, new))
        if c.kind == "box":
            l = np.where(finite_sides(cs, c), l, 0.0)
        out.append(np.ascontiguousarray(l))
    return out


def al(cs, X, U, lam, mu, cons=None, Xref=None, Uref=None, Q=None, R=None, Qf=None, direction=None, state_err=None):
    """every output of the call for (X, U) (B, nc, ..) with duals lam (list, one per constraint) and penalty mu (B,), each with
    its bound `<name>b` between two computations (gU, gx0: one computation, the tests allow twice that, as GR's); counts: the
    branch counts (dict); Lx the local term (GR's bound 7); with direction = (dX, dU): hmax and f3 of bound G"""
    cons = cs.cons if cons is None else cons
    Xr = cs.Xref if Xref is None else Xref
    Ur = cs.Uref if Uref is None else Uref
    Q, R, Qf = (cs.Q if Q is None else Q), (cs.R if R is None else R), (cs.Qf if Qf is None else Qf)
    B, nc = U.shape[:2]
    n, m, N = cs.n, cs.m, cs.N
    nz = n + m
    Z = GR.stack_z(cs, X, U)
    dZs = np.zeros(Z.shape)
    if state_err is not None:
        dZs[..., :n] = state_err
    dirZ = None if direction is None else GR.stack_z(cs, direction[0], direction[1])
    mu_ = np.asarray(mu, dtype=np.float64)[:, None]                # (B, 1) against (B, nc)
    C, Ca, CE = np.zeros(Z.shape), np.zeros(Z.shape), np.zeros(Z.shape)
    S, Sabs, Serr, terms = np.zeros((B, nc)), np.zeros((B, nc)), np.zeros((B, nc)), 0
    hmax, f3 = np.full((B, nc), np.inf), np.zeros((B, nc))
    gz = {k: np.zeros((B, nc, nz)) for k in ("gzmax", "gzmin", "gzmaxb", "gzminb")}
    counts = dict(lin_pos=0, lin_neg_dual=0, lin_off=0, cone=np.zeros(3, dtype=int), eq_pos=0, eq_neg=0)
    rows = 2

    def linear(c, l, E, eq, dc):
        """(g, Eg) of rows of value c (.., p) with duals l; adds phi and its bounds to S, Sabs, Serr; counts; hmax"""
        nonlocal S, Sabs, Serr, hmax
        mm = mu_[..., None]
        act = np.ones(c.shape, dtype=bool) if eq else (c >= 0) | (l > 0)
        g = l + np.where(act, mm * c, 0.0)
        quad = np.where(act, 0.5 * mm * c * c, 0.0)
        S = S + (l * c + quad).sum(axis=-1)
        Sabs = Sabs + (np.abs(l * c) + quad).sum(axis=-1)
        Serr = Serr + ((np.abs(g) + mm * E) * E + 2 * U_ * np.abs(l * c) + 4 * U_ * quad).sum(axis=-1)
        if eq:
            counts["eq_pos"] += int((l > 0).sum())
            counts["eq_neg"] += int((l < 0).sum())
        else:
            counts["lin_pos"] += int((c >= 0).sum())
            counts["lin_neg_dual"] += int(((c < 0) & (l > 0)).sum())
            counts["lin_off"] += int(((c < 0) & ~(l > 0)).sum())
            if dc is not None:
                with np.errstate(divide="ignore", invalid="ignore"):
                    hmax = np.minimum(hmax, np.where(l > 0, np.inf, np.abs(c) / np.abs(dc)).min(axis=-1))
        return g, mm * E + 2 * U_ * np.abs(g)

    for c, lc in zip(cons, lam):
        rows += 0 if c.kind == "box" else c.A.shape[2]
        for k in range(c.k0, c.k1 + 1):
            z = Z[:, :, k]
            lk = lc[:, k - c.k0]
            if c.kind == "box":
                cols = n if k == N - 1 else nz
                zc = z[..., :cols]
                for side, (sign, bound, name) in enumerate(((1.0, c.zmax, "gzmax"), (-1.0, c.zmin, "gzmin"))):
                    bnd = bound[:, None, :cols]
                    fin = np.broadcast_to(np.isfinite(bnd), zc.shape)
                    bf = np.where(fin, bnd, 0.0)
                    idx = np.nonzero(fin.any(axis=(0, 1)))[0]                   # columns with this side somewhere in the batch
                    if idx.size == 0:
                        continue
                    assert fin[..., idx].all(), "a BOX side is finite for every instance or for none"
                    cv = sign * (zc - bf)[..., idx]
                    E = (2 * U_ * (np.abs(zc) + np.abs(bf)) + dZs[:, :, k, :cols])[..., idx]
                    l = np.broadcast_to(lk[:, None, side, :cols], zc.shape)[..., idx]
                    g, Eg = linear(cv, l, E, False, None if dirZ is None else sign * dirZ[:, :, k, :cols][..., idx])
                    terms += idx.size
                    C[:, :, k, idx] += sign * g
                    Ca[:, :, k, idx] += np.abs(g)
                    CE[:, :, k, idx] += Eg
                    gz[name][..., idx] += -sign * g
                    gz[name + "b"][..., idx] += Eg + 2 * (c.k1 - c.k0 + 2) * U_ * np.abs(g)
                continue
            Ak, bk = c.A[:, k - c.k0], c.b[:, k - c.k0]
            v = np.einsum("bpj,bcj->bcp", Ak, z) + bk[:, None]
            E = (2 * (nz + 2) * U_ * (np.einsum("bpj,bcj->bcp", np.abs(Ak), np.abs(z)) + np.abs(bk)[:, None])
                 + np.einsum("bpj,bcj->bcp", np.abs(Ak), dZs[:, :, k]))
            dv = None if dirZ is None else np.einsum("bpj,bcj->bcp", Ak, dirZ[:, :, k])
            p = v.shape[-1]
            l = np.broadcast_to(lk[:, None], v.shape)
            terms += p
            if c.kind == "lin":
                g, Eg = linear(v, l, E, c.eq, dv)
            else:
                mm = mu_[..., None]
                w = l - mm * v
                s, t = w[..., :-1], w[..., -1]
                ns = np.linalg.norm(s, axis=-1)
                inside = ns <= t
                polar = ~inside & (ns <= -t)
                bdry = ~inside & ~polar
                with np.errstate(divide="ignore", invalid="ignore"):
                    cc = np.where(ns > 0, 0.5 * (1 + t / ns), 0.0)
                yb = np.concatenate((cc[..., None] * s, (cc * ns)[..., None]), axis=-1)
                y = np.where(inside[..., None], w, np.where(polar[..., None], 0.0, yb))
                nw, ny, nl2 = np.linalg.norm(w, axis=-1), np.linalg.norm(y, axis=-1), (l * l).sum(axis=-1)
                Eyr = np.sqrt(p) * 2 * U_ * np.abs(w).max(axis=-1) + 16 * U_ * nw
                Ey = np.sqrt(p) * mu_ * E.max(axis=-1) + Eyr
                psi = ((y * y).sum(axis=-1) - nl2) / (2 * mu_)
                S = S + psi
                Sabs = Sabs + (ny * ny + nl2) / (2 * mu_)
                Serr = Serr + (ny + np.sqrt(p) * Ey) * np.sqrt(p) * (E.max(axis=-1) + Eyr / mu_) + 2 * (p + 6) * U_ * (ny * ny + nl2) / (2 * mu_)
                g, Eg = -y, np.broadcast_to(Ey[..., None], v.shape)
                for i, wh in enumerate((inside, polar, bdry)):
                    counts["cone"][i] += int(wh.sum())
                if dv is not None:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        dws, dwt = mu_ * np.linalg.norm(dv[..., :-1], axis=-1), mu_ * np.abs(dv[..., -1])
                        kink = np.minimum(np.minimum(np.abs(ns - t), np.abs(ns + t)), ns)
                        hmax = np.minimum(hmax, kink / (dws + dwt))
                        f3 += np.where(bdry, (3 * dwt * dws ** 2 / ns + 2.31 * (np.abs(t) + 0.5 * ns) * dws ** 3 / ns ** 2) / mu_, 0.0)
            C[:, :, k] += np.einsum("bpj,bcp->bcj", Ak, g)
            Ca[:, :, k] += np.einsum("bpj,bcp->bcj", np.abs(Ak), np.abs(g))
            CE[:, :, k] += np.einsum("bpj,bcp->bcj", np.abs(Ak), Eg)
    # the cost with the weights given (ER.cost's formula and bound 3)
    ex, eu = X - Xr[:, None], U - Ur[:, None]
    dt = cs.dt
    J = (0.5 * dt * (np.einsum("bi,bcki->bc", Q, ex[:, :, :-1] ** 2) + np.einsum("bi,bcki->bc", R, eu ** 2))
         + 0.5 * np.einsum("bi,bci->bc", Qf, ex[:, :, -1] ** 2))
    Jb = 2 * (N * nz + 8) * U_ * J
    LA = J + S
    LAb = Jb + Serr + 2 * (terms + 3) * U_ * Sabs + 2 * U_ * np.abs(LA)
    gam = (n + rows + 4) * U_
    wx = np.broadcast_to((dt * Q)[:, None, None], ex.shape).copy()
    wx[:, :, -1] = Qf[:, None]
    wu = (dt * R)[:, None, None]
    Lx, Lu = wx * ex + C[..., :n], wu * eu + C[:, :, :-1, n:]
    Lax, Lau = np.abs(wx * ex) + Ca[..., :n], np.abs(wu * eu) + Ca[:, :, :-1, n:]
    Dx, Du = CE[..., :n] + wx * dZs[..., :n], CE[:, :, :-1, n:]
    gU, gUb = np.zeros(U.shape), np.zeros(U.shape)
    lamc, dlam = Lx[:, :, -1], gam * Lax[:, :, -1] + Dx[:, :, -1]
    T = lambda M, v: np.einsum("bij,bci->bcj", M, v)
    for k in range(N - 2, -1, -1):
        A, Bm = cs.A[:, k], cs.Bm[:, k]
        gU[:, :, k] = Lu[:, :, k] + T(Bm, lamc)
        gUb[:, :, k] = T(np.abs(Bm), dlam) + gam * (Lau[:, :, k] + T(np.abs(Bm), np.abs(lamc))) + Du[:, :, k]
        lamc, dlam = (Lx[:, :, k] + T(A, lamc), T(np.abs(A), dlam) + gam * (Lax[:, :, k] + T(np.abs(A), np.abs(lamc))) + Dx[:, :, k])
    d = dZs[..., :n]
    gQ, gR, gQf = 0.5 * dt * (ex[:, :, :-1] ** 2).sum(axis=2), 0.5 * dt * (eu ** 2).sum(axis=2), 0.5 * ex[:, :, -1] ** 2
    return NS(LA=LA, LAb=LAb, J=J, Jb=Jb, gU=gU, gUb=gUb, gx0=lamc, gx0b=dlam,
              gXref=-(wx * ex), gXrefb=4 * U_ * np.abs(wx * ex) + wx * d, gUref=-(wu * eu), gUrefb=4 * U_ * np.abs(wu * eu),
              gQ=gQ, gQb=2 * (N + 4) * U_ * gQ + dt * (np.abs(ex[:, :, :-1]) * d[:, :, :-1]).sum(axis=2),
              gR=gR, gRb=2 * (N + 4) * U_ * gR, gQf=gQf, gQfb=4 * U_ * gQf + np.abs(ex[:, :, -1]) * d[:, :, -1],
              gzmax=gz["gzmax"], gzmaxb=gz["gzmaxb"], gzmin=gz["gzmin"], gzminb=gz["gzminb"],
              counts=counts, Lx=Lx, hmax=hmax, f3=f3)


def bound_of(y, name):
    """the bound the tests hold output `name` to between the device and the yardstick: twice bound E for gU and gx0 (GR's rule),
    the bound as it stands for the others"""
    b = getattr(y, {"LA": "LAb", "J": "Jb"}.get(name, name + "b"))
    return 2 * b if name in ("gU", "gx0") else b


def reaches_every_branch(cs, counts):
    """the issue's condition on the inputs, on the yardstick's own counts"""
    ok = True
    if any(c.kind == "box" or (c.kind == "lin" and not c.eq) for c in cs.cons):
        ok = ok and counts["lin_pos"] > 0 and counts["lin_neg_dual"] > 0 and counts["lin_off"] > 0
    if any(c.kind == "soc" for c in cs.cons):
        ok = ok and bool((counts["cone"] > 0).all())
    if any(c.kind == "lin" and c.eq for c in cs.cons):
        ok = ok and counts["eq_pos"] > 0 and counts["eq_neg"] > 0
    return ok


# ---------------------------------------------------------------------------------------------- the envelope identity
TIGHT = dict(iterations_outer=1, reset_duals=0, reset_penalties=0, cost_tolerance=1e-14, cost_tolerance_intermediate=1e-14,
             gradient_tolerance=1e-12, gradient_tolerance_intermediate=1e-12, iterations_inner=300, iterations=300)


def shape_duals(cs, flat):
    """the oracle's flat dual arrays of one instance as the (1, nk, ..) arrays of this module"""
    return [np.asarray(l).reshape((1, c.k1 - c.k0 + 1) + ((2, cs.n + cs.m) if c.kind == "box" else (-1,))) for c, l in zip(cs.cons, flat)]


def oracle_envelope(O, cs, b, pk, d, h):
    """The envelope identity on the CPU oracle for instance b and direction d: solve (3 outer iterations), then one tight inner
    solve with the duals and the penalty held; gx0 . d of the yardstick at what that left, against central differences of
    cost() after tight fixed-dual re-solves at x0 +- h d.  Returns NS(err = |fd - gx0 . d|, tol = the rounding bound of the two
    values over 2h plus twice bound E of gx0 times |d| plus bound G along the measured (dX, dU) / (2h), got, mu, ulp = one unit in
    the last place of the larger value over 2h)."""
    s = ER.oracle_of(O, cs, b, pk)
    s.set_opts(O.default_opts(iterations_outer=3))
    s.solve()
    lam = [s.duals(i) for i in range(len(cs.cons))]
    mu = np.array([s.penalties(0)[0]])
    put = lambda: [s.set_duals(i, l) for i, l in enumerate(lam)]
    s.set_opts(O.default_opts(**TIGHT))
    s.solve()
    put()
    U0 = s.controls()
    s.set_controls(U0), s.max_violation()
    X0 = s.states()
    sub, shaped = ER.sub_case(cs, b), shape_duals(cs, lam)
    pts = []
    for sgn in (1.0, -1.0):
        s.set_initial_state(cs.x0[b] + sgn * h * d)
        s.set_controls(U0)
        put()
        s.solve()
        put()
        Up = s.controls()
        s.set_controls(Up), s.max_violation()
        Xp = s.states()
        pts.append((s.cost(), Xp, Up, al(sub, Xp[None, None], Up[None, None], shaped, mu).LAb[0, 0]))
    s.set_initial_state(cs.x0[b])
    dX, dU = (pts[0][1] - pts[1][1]) / (2 * h), (pts[0][2] - pts[1][2]) / (2 * h)
    y = al(sub, X0[None, None], U0[None, None], shaped, mu, direction=(dX[None, None], dU[None, None]))
    got = float(y.gx0[0, 0] @ d)
    fd = (pts[0][0] - pts[1][0]) / (2 * h)
    tol = (pts[0][3] + pts[1][3]) / (2 * h) + 2 * float(y.gx0b[0, 0] @ np.abs(d)) + h * h * float(y.f3[0, 0]) / 6
    return NS(err=abs(fd - got), tol=tol, got=got, mu=mu[0], ulp=U_ * max(abs(pts[0][0]), abs(pts[1][0])) / h)


ENVELOPE_LADDER = 1e-3 * 1.5 ** np.arange(16)        # 1e-3 .. 0.44


def envelope_step(O, cs, b, pk, d):
    """The step at which a second computation of the envelope quotient (the device's) can be held to a multiple of the oracle's
    own error, chosen from the oracle alone.  With duals and penalty fixed the optimal cost is piecewise quadratic in x0, so the
    central difference is exact until x0 +- h d crosses a change of the active set at some h0; below h0 the oracle's error is a
    few units in the last place of L_A over 2h, i.e. chance (it can be zero), and a ratio against it says nothing.  Beyond h0
    both computations share the truncation of the same function, which grows continuously from zero, like (h - h0)^2 / h.  The
    step is one at which the oracle's error is between 1e3 and 1e5 such units: rounding and the stopping tolerance then move
    either error by parts in a hundred at most, and the error is still some 1e-11 .. 1e-9 of the gradient.  It is found by the
    first step of the ladder that reaches 1e3 units and bisection (geometric) between it and the step before.  Returns (h, the
    oracle's result at h)."""
    units = lambda e: e.err / e.ulp
    lo = ENVELOPE_LADDER[0] / 8
    for h in ENVELOPE_LADDER:
        e = oracle_envelope(O, cs, b, pk, d, float(h))
        if units(e) >= 1e3:
            break
        lo = h
    else:
        raise AssertionError("no step of the ladder reaches a change of the active set")
    hi = h
    for _ in range(60):
        if units(e) <= 1e5:
            return float(h), e
        h = float(np.sqrt(lo * hi))
        e = oracle_envelope(O, cs, b, pk, d, h)
        if units(e) < 1e3:
            lo = h
            e = NS(err=np.inf, ulp=1.0)
        else:
            hi = h
    raise AssertionError("no step with an oracle error between 1e3 and 1e5 units in the last place")
