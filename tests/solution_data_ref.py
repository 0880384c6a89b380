"""numpy yardstick of altro_batch_solution_vjp_data and altro_batch_get_gain_active_set: the definition restated,
parametric in dtype (np.float64, np.longdouble), on the data of a box-only evaluate_ref.Case, and a DENSE adjoint that shares no
code with the sweeps.  Shared by tests/test_solution_data_api.py (the sweeps against the dense solve, on the CPU) and
tests/test_solution_data_gpu.py (the device against the sweeps and against the dense adjoint).

Inside the active set `codes` (B, N, n+m; bit 0 the upper side, bit 1 the lower side) and the penalty mu_p of the stored pass
the augmented Lagrangian of a box-only problem is
    1/2 sum_k (z_k - zref_k)' diag(w_k) (z_k - zref_k) + sum over the sides in the set of  l c + mu_p c^2 / 2,
c = z - zmax resp. zmin - z, with the diagonal Hessian  hz = w + mu_p [upper] + mu_p [lower].  With z = (X, U) the trajectory
held, e = z - zref, lam its costate, (s_0, xi, nu) = Lin((gX, gU), 0) of solution_ref.lin and dz = (xi, nu):
    dlam_{N-1} = gX_{N-1} + hz xi_{N-1};   dlam_k = gX_k + hz_k xi_k + A_k' dlam_{k+1}
    gQ = dt sum_{k<N-1} xi_k e_k;  gQf = xi_{N-1} e_{N-1};  gR = dt sum_k nu_k e_{u,k}
    gzmax = -mu_p sum_k [upper side in the set] dz_k;  gzmin = -mu_p sum_k [lower side in the set] dz_k
    gA_k = lam_{k+1} xi_k' + dlam_{k+1} x_k';  gB_k = lam_{k+1} nu_k' + dlam_{k+1} u_k';  gf_k = dlam_{k+1}
Every array carries a seed axis: (B, S, ...).  Matrices are indexed [i, j] (row, column)."""
from types import SimpleNamespace as NS

import numpy as np

import solution_ref as SR

OUTS = ("gQ", "gQf", "gR", "gzmin", "gzmax", "gA", "gB", "gf")


def _t(a, dtype):
    return np.asarray(a, dtype=dtype)


def box_of(cs):
    return next((c for c in cs.cons if c.kind == "box"), None)


def theta_of(cs):
    """the data the derivatives are taken with respect to, as one namespace of float64 arrays (copies)"""
    box = box_of(cs)
    nz = cs.n + cs.m
    zmin = box.zmin.copy() if box is not None else np.full((cs.B, nz), -np.inf)
    zmax = box.zmax.copy() if box is not None else np.full((cs.B, nz), np.inf)
    return NS(A=cs.A.copy(), Bm=cs.Bm.copy(), f=cs.f.copy(), Q=cs.Q.copy(), R=cs.R.copy(), Qf=cs.Qf.copy(), zmin=zmin, zmax=zmax)


def weights(th, cs, dtype):
    """(wx (B, N, n), wu (B, m)) of the data th: dt Q before the last knot, Qf at it; dt R"""
    dt = dtype(cs.dt)
    wx = np.repeat((dt * _t(th.Q, dtype))[:, None], cs.N, axis=1)
    wx[:, -1] = _t(th.Qf, dtype)
    return wx, dt * _t(th.R, dtype)


def stack_duals(cs, duals):
    """the BOX duals (B, nk, 2, nz) of the knots k0 .. k1 as (lhi, llo), each (B, N, nz), zero outside the range; None: zeros"""
    box = box_of(cs)
    lhi, llo = np.zeros((cs.B, cs.N, cs.n + cs.m)), np.zeros((cs.B, cs.N, cs.n + cs.m))
    if box is not None and duals is not None:
        lhi[:, box.k0:box.k1 + 1], llo[:, box.k0:box.k1 + 1] = duals[:, :, 0], duals[:, :, 1]
    return lhi, llo


def box_mask(cs):
    """(B, N, nz) bool x 2: the upper / lower sides that exist (finite, inside the knot range, state columns only at knot N-1)"""
    box = box_of(cs)
    nz = cs.n + cs.m
    hi, lo = np.zeros((cs.B, cs.N, nz), dtype=bool), np.zeros((cs.B, cs.N, nz), dtype=bool)
    if box is not None:
        hi[:, box.k0:box.k1 + 1] = np.isfinite(box.zmax)[:, None]
        lo[:, box.k0:box.k1 + 1] = np.isfinite(box.zmin)[:, None]
        hi[:, cs.N - 1, cs.n:] = lo[:, cs.N - 1, cs.n:] = False
    return hi, lo


def stack_z(cs, X, U, dtype=np.float64):
    """(B, N, nz): [x_k, u_k], zero controls at knot N-1"""
    Z = np.zeros((cs.B, cs.N, cs.n + cs.m), dtype=dtype)
    Z[..., :cs.n] = X
    Z[:, :-1, cs.n:] = U
    return Z


def codes_at(cs, X, U, duals):
    """the active set of the trajectory (X, U) under the duals: a side is in it iff it exists and c >= 0 or its dual > 0"""
    box = box_of(cs)
    hi, lo = box_mask(cs)
    lhi, llo = stack_duals(cs, duals)
    Z = stack_z(cs, X, U)
    codes = np.zeros(Z.shape, dtype=np.uint8)
    if box is not None:
        zmax, zmin = np.where(np.isfinite(box.zmax), box.zmax, 0.0)[:, None], np.where(np.isfinite(box.zmin), box.zmin, 0.0)[:, None]
        codes |= (hi & ((Z - zmax >= 0) | (lhi > 0))).astype(np.uint8)
        codes |= (lo & ((zmin - Z >= 0) | (llo > 0))).astype(np.uint8) << 1
    return codes


def hz_of(th, cs, codes, mu_pass, dtype):
    """(hx (B, N, n), hu (B, N-1, m)): w, + mu_p for the upper side in the set, + mu_p for the lower side"""
    wx, wu = weights(th, cs, dtype)
    w = np.concatenate([wx, np.repeat(wu[:, None], cs.N, axis=1)], axis=2)
    mu = _t(mu_pass, dtype)[:, None, None]
    zero = dtype(0)
    h = w + np.where(codes & 1, mu, zero)
    h = h + np.where(codes & 2, mu, zero)
    return h[..., :cs.n], h[:, :-1, cs.n:]


def costate(cs, X, U, duals, mu, dtype=np.float64):
    """lam (B, N, n) of the trajectory (X, U) with the duals and the penalty held (altro_batch_evaluate_al at U == NULL):
    l = w e + g_hi - g_lo, g = dual + [c >= 0 or dual > 0] mu c;  lam_{N-1} = l_x,  lam_k = l_x + A_k' lam_{k+1}"""
    th = theta_of(cs)
    wx, _ = weights(th, cs, dtype)
    hi, lo = box_mask(cs)
    lhi, llo = (_t(a, dtype) for a in stack_duals(cs, duals))
    Xd = _t(X, dtype)
    Z = stack_z(cs, Xd, _t(U, dtype), dtype)
    m_ = _t(mu, dtype)[:, None, None]
    zero = dtype(0)
    zmax, zmin = _t(np.where(np.isfinite(th.zmax), th.zmax, 0.0), dtype)[:, None], _t(np.where(np.isfinite(th.zmin), th.zmin, 0.0), dtype)[:, None]
    chi, clo = Z - zmax, zmin - Z
    ghi = np.where(hi, lhi + np.where((chi >= 0) | (lhi > 0), m_ * chi, zero), zero)
    glo = np.where(lo, llo + np.where((clo >= 0) | (llo > 0), m_ * clo, zero), zero)
    l = wx * (Xd - _t(cs.Xref, dtype)) + (ghi - glo)[..., :cs.n]
    A = _t(cs.A, dtype)
    lam = np.zeros(Xd.shape, dtype=dtype)
    lam[:, -1] = l[:, -1]
    for k in range(cs.N - 2, -1, -1):
        lam[:, k] = l[:, k] + np.einsum("bij,bi->bj", A[:, k], lam[:, k + 1])
    return lam


def _mask(valid, d):
    for a in d.values():
        a[np.asarray(valid) == 0] = np.nan
    return d


def gradients(cs, codes, mu_pass, X, U, lam, xi, nu, dlam, per_knot, dtype):
    """the eight outputs from dz = (xi, nu) (B, S, ..), dlam (B, S, N, n), the trajectory and its costate"""
    n, N = cs.n, cs.N
    dt = dtype(cs.dt)
    X, U, lam = _t(X, dtype), _t(U, dtype), _t(lam, dtype)
    ex, eu = (X - _t(cs.Xref, dtype))[:, None], (U - _t(cs.Uref, dtype))[:, None]
    mu = _t(mu_pass, dtype)[:, None, None]
    dz = np.zeros(xi.shape[:-1] + (n + cs.m,), dtype=dtype)
    dz[..., :n] = xi
    dz[:, :, :-1, n:] = nu
    cd = codes[:, None]
    zero = dtype(0)
    gA = np.einsum("bki,bskj->bskij", lam[:, 1:], xi[:, :, :-1]) + np.einsum("bski,bkj->bskij", dlam[:, :, 1:], X[:, :-1])
    gB = np.einsum("bki,bskj->bskij", lam[:, 1:], nu) + np.einsum("bski,bkj->bskij", dlam[:, :, 1:], U)
    gf = dlam[:, :, 1:].copy()
    if not per_knot:
        gA, gB, gf = gA.sum(axis=2), gB.sum(axis=2), gf.sum(axis=2)
    return dict(gQ=dt * (xi[:, :, :-1] * ex[:, :, :-1]).sum(axis=2), gQf=xi[:, :, -1] * ex[:, :, -1], gR=dt * (nu * eu).sum(axis=2),
                gzmax=-(mu * np.where(cd & 1, dz, zero).sum(axis=2)), gzmin=-(mu * np.where(cd & 2, dz, zero).sum(axis=2)),
                gA=gA, gB=gB, gf=gf)


def sweep(cs, K, F, codes, mu_pass, valid, X, U, lam, gX=None, gU=None, per_knot=False, dtype=np.float64):
    """the three sweeps restated: dict of the eight outputs, plus xi, nu, dlam, s0"""
    S = (gX if gX is not None else gU).shape[1]
    zx, zu, z0 = SR._zeros(cs, S, dtype)
    gx, gu = (zx if gX is None else _t(gX, dtype)), (zu if gU is None else _t(gU, dtype))
    s0, xi, nu = SR.lin(cs, K, F, gx, gu, z0, dtype)
    hx, _ = hz_of(theta_of(cs), cs, codes, mu_pass, dtype)
    A = _t(cs.A, dtype)
    dlam = np.zeros(xi.shape, dtype=dtype)
    dlam[:, :, -1] = gx[:, :, -1] + hx[:, None, -1] * xi[:, :, -1]
    for k in range(cs.N - 2, -1, -1):
        dlam[:, :, k] = gx[:, :, k] + hx[:, None, k] * xi[:, :, k] + np.einsum("bij,bsi->bsj", A[:, k], dlam[:, :, k + 1])
    out = _mask(valid, gradients(cs, codes, mu_pass, X, U, lam, xi, nu, dlam, per_knot, dtype))
    out.update(xi=xi, nu=nu, dlam=dlam, s0=s0)
    return out


def riccati_codes(cs, codes, mu_pass, dtype=np.float64):
    """(K (B, N-1, m, n), Quu (B, N-1, m, m)) of the LQ problem inside the set: the Riccati recursion with the diagonal
    Hessians hz, every operation in `dtype`"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    A, Bm = _t(cs.A, dtype), _t(cs.Bm, dtype)
    hx, hu = hz_of(theta_of(cs), cs, codes, mu_pass, dtype)
    K = np.zeros((B, N - 1, m, n), dtype=dtype)
    Quu_all = np.zeros((B, N - 1, m, m), dtype=dtype)
    eye_n, eye_m = np.eye(n, dtype=dtype), np.eye(m, dtype=dtype)
    P = hx[:, N - 1, :, None] * eye_n
    half = dtype(0.5)
    T = lambda M: np.swapaxes(M, -1, -2)
    for k in range(N - 2, -1, -1):
        PA, PB = P @ A[:, k], P @ Bm[:, k]
        Qxx = hx[:, k, :, None] * eye_n + T(A[:, k]) @ PA
        Quu = hu[:, k, :, None] * eye_m + T(Bm[:, k]) @ PB
        Qux = T(Bm[:, k]) @ PA
        Quu_all[:, k] = Quu
        K[:, k] = T(SR.quu_solve(SR.ldl(Quu), T(Qux)))
        P = Qxx + T(Qux) @ K[:, k]
        P = half * (P + T(P))
    return K, Quu_all


def factors(Quu):
    """F (B, N-1, m, m) of Quu = L D L' knot by knot, in the convention of altro_batch_get_gain_factors"""
    m = Quu.shape[-1]
    return SR.ldl(Quu.reshape(-1, m, m)).reshape(Quu.shape)


def quu_of_factors(F, dtype=np.longdouble):
    """Quu = L D L' (.., m, m) from the stored factors: 1 / D on the diagonal, L below it"""
    F = _t(F, dtype)
    m = F.shape[-1]
    L = np.tril(F, -1) + np.eye(m, dtype=dtype)
    D = dtype(1) / np.einsum("...aa->...a", F)
    return np.einsum("...ac,...c,...bc->...ab", L, D, L)


# ------------------------------------------------------------------ the dense adjoint: one KKT matrix, no sweep
def _layout(cs):
    nxv, nuv = (cs.N - 1) * cs.n, (cs.N - 1) * cs.m
    return nxv, nuv, nxv + nuv, (cs.N - 1) * cs.n


def kkt(th, cs, codes, mu_pass, duals, dtype=np.longdouble):
    """(M, r) of the LQ problem inside the set with the data th: unknowns z = (x_1 .. x_{N-1}, u_0 .. u_{N-2}) and one multiplier
    p_k (= lam_{k+1}) per dynamics row  A_k x_k + B_k u_k + f_k - x_{k+1} = 0:   [H C'; C 0] [z; p] = [h; rhs]"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    nxv, nuv, nzv, nc = _layout(cs)
    A, Bm, f = _t(th.A, dtype), _t(th.Bm, dtype), _t(th.f, dtype)
    hx, hu = hz_of(th, cs, codes, mu_pass, dtype)
    wx, wu = weights(th, cs, dtype)
    lhi, llo = (_t(a, dtype) for a in stack_duals(cs, duals))
    hi, lo = box_mask(cs)
    mu = _t(mu_pass, dtype)[:, None, None]
    zero = dtype(0)
    zmax, zmin = _t(np.where(np.isfinite(th.zmax), th.zmax, 0.0), dtype)[:, None], _t(np.where(np.isfinite(th.zmin), th.zmin, 0.0), dtype)[:, None]
    # the constant part of the gradient of the box terms, moved to the right-hand side
    hb = np.where(hi, np.where(codes & 1, mu * zmax, zero) - lhi, zero) + np.where(lo, np.where(codes & 2, mu * zmin, zero) + llo, zero)
    x0 = _t(cs.x0, dtype)
    M = np.zeros((B, nzv + nc, nzv + nc), dtype=dtype)
    r = np.zeros((B, nzv + nc), dtype=dtype)
    ar = np.arange
    for k in range(1, N):
        o = (k - 1) * n
        M[:, o + ar(n), o + ar(n)] = hx[:, k]
        r[:, o:o + n] = wx[:, k] * _t(cs.Xref, dtype)[:, k] + hb[:, k, :n]
    for k in range(N - 1):
        o = nxv + k * m
        M[:, o + ar(m), o + ar(m)] = hu[:, k]
        r[:, o:o + m] = wu * _t(cs.Uref, dtype)[:, k] + hb[:, k, n:]
    for k in range(N - 1):
        q = nzv + k * n
        M[:, q + ar(n), k * n + ar(n)] = -1
        M[:, q:q + n, nxv + k * m:nxv + (k + 1) * m] = Bm[:, k]
        r[:, q:q + n] = -f[:, k]
        if k > 0:
            M[:, q:q + n, (k - 1) * n:k * n] = A[:, k]
        else:
            r[:, q:q + n] -= np.einsum("bij,bj->bi", A[:, 0], x0)
    M[:, :nzv, nzv:] = np.swapaxes(M[:, nzv:, :nzv], -1, -2)
    return M, r


def _unpack(cs, sol, x_first):
    """columns of a KKT solution (B, nzv + nc, S) -> x (B, S, N, n) with x_first at knot 0, u (B, S, N-1, m), p (B, S, N, n) with
    p at knots 1 .. N-1 (knot 0: zero)"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    nxv, nuv, nzv, nc = _layout(cs)
    S = sol.shape[2]
    s = np.swapaxes(sol, 1, 2)
    x = np.zeros((B, S, N, n), dtype=sol.dtype)
    x[:, :, 0] = x_first
    x[:, :, 1:] = s[:, :, :nxv].reshape(B, S, N - 1, n)
    u = s[:, :, nxv:nzv].reshape(B, S, N - 1, m).copy()
    p = np.zeros((B, S, N, n), dtype=sol.dtype)
    p[:, :, 1:] = s[:, :, nzv:].reshape(B, S, N - 1, n)
    return x, u, p


def dense_solve(th, cs, codes, mu_pass, duals, dtype=np.longdouble):
    """the minimiser of the LQ problem inside the set with the data th: (X (B, N, n), U (B, N-1, m), lam (B, N, n); lam_0 unset)"""
    M, r = kkt(th, cs, codes, mu_pass, duals, dtype)
    x, u, p = _unpack(cs, SR.gauss_solve(M, r[:, :, None]), _t(cs.x0, dtype)[:, None])
    return x[:, 0], u[:, 0], p[:, 0]


def dense_adjoint(cs, codes, mu_pass, valid, X, U, lam, gX=None, gU=None, per_knot=False, dtype=np.longdouble):
    """[dz; dp] = -KKT^-1 [g; 0], then the gradients from dz, dp (= dlam_{k+1}), the trajectory and its costate"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    nxv, nuv, nzv, nc = _layout(cs)
    S = (gX if gX is not None else gU).shape[1]
    g = np.zeros((B, nzv + nc, S), dtype=dtype)
    if gX is not None:
        g[:, :nxv] = np.swapaxes(_t(gX, dtype)[:, :, 1:].reshape(B, S, nxv), 1, 2)
    if gU is not None:
        g[:, nxv:nzv] = np.swapaxes(_t(gU, dtype).reshape(B, S, nuv), 1, 2)
    M, _ = kkt(theta_of(cs), cs, codes, mu_pass, None, dtype)
    xi, nu, dp = _unpack(cs, -SR.gauss_solve(M, g), dtype(0))
    out = _mask(valid, gradients(cs, codes, mu_pass, X, U, lam, xi, nu, dp, per_knot, dtype))
    out.update(xi=xi, nu=nu, dlam=dp)
    return out


def perturbed(th, dth, t):
    """th + t dth on every datum (infinite bounds stay)"""
    out = NS()
    for k, v in vars(th).items():
        d = getattr(dth, k)
        setattr(out, k, np.where(np.isfinite(v), v + t * d, v) if k in ("zmin", "zmax") else v + t * d)
    return out


def dense_forward(th, dth, cs, codes, mu_pass, duals, dtype=np.longdouble):
    """the derivative of the minimiser along dth: d[z; p] = KKT^-1 (dr - dKKT [z; p]) -> (dX (B, N, n), dU (B, N-1, m)).  KKT and
    r are affine in the data, so their derivatives are differences of two assemblies."""
    ld = lambda ns: NS(**{k: _t(v, dtype) for k, v in vars(ns).items()})
    M, r = kkt(ld(th), cs, codes, mu_pass, duals, dtype)
    M1, r1 = kkt(perturbed(ld(th), ld(dth), dtype(1)), cs, codes, mu_pass, duals, dtype)
    y = SR.gauss_solve(M, r[:, :, None])
    rhs = (r1 - r)[:, :, None] - (M1 - M) @ y
    x, u, _ = _unpack(cs, SR.gauss_solve(M, rhs), dtype(0))
    return x[:, 0], u[:, 0]


def pairing(out, dth, per_knot):
    """sum <g_theta, d_theta> per (instance, seed) in the dtype of `out`, and the sum of the absolute terms"""
    tot, ab = 0, 0
    for k, d in (("gQ", dth.Q), ("gQf", dth.Qf), ("gR", dth.R), ("gzmin", dth.zmin), ("gzmax", dth.zmax), ("gA", dth.A), ("gB", dth.Bm), ("gf", dth.f)):
        g = out[k]
        d = np.asarray(d, dtype=g.dtype)
        if k in ("gA", "gB", "gf") and not per_knot:   # a time-invariant datum: one direction for every knot
            assert (d == d[:, :1]).all()
            d = d[:, 0]
        t = g * d[:, None]
        ax = tuple(range(2, t.ndim))
        tot, ab = tot + t.sum(axis=ax), ab + np.abs(t).sum(axis=ax)
    return tot, ab
