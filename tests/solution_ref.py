"""numpy yardstick of altro_batch_solution_vjp / altro_batch_solution_jvp: the definition restated, parametric in dtype
(np.float64, np.longdouble), on the data of an evaluate_ref.Case, the gains altro_batch_get_gains returns and the factors
altro_batch_get_gain_factors_dev returns.  Shared by tests/test_solution_sens_gpu.py (the device against it in extended
precision) and tests/test_solution_sens_api.py (its meaning against the dense solve, on the CPU).

    Lin(g, xi_0) -> (s_0, xi, nu),  g = (gx [N][n], gu [N-1][m]):
      backward  s_{N-1} = gx_{N-1};  k = N-2 .. 0:  q_x = gx_k + A_k' s_{k+1},  q_u = gu_k + B_k' s_{k+1},
                d_k = -Quu_k^-1 q_u  (L y = q_u; z = y * (1/D); L' w = z; d = -w),  s_k = q_x + K_k' q_u
      forward   xi_0 given;  k = 0 .. N-2:  nu_k = K_k xi_k + d_k,  xi_{k+1} = A_k xi_k + B_k nu_k
    VJP  (s_0, xi, nu) = Lin((gX, gU), 0):  gx0 = s_0,  gXref_k = -(w xi)_k (w = dt Q, Qf at N-1),  gUref_k = -(dt R nu)_k
    JVP  (., xi, nu) = Lin((-w vXref, -dt R vUref), vx0):  dX = xi,  dU = nu

Also here, with no solver data at all: the dense KKT Jacobian of the unconstrained tracking problem (the true solution map where
it is unambiguous) and a Riccati recursion that makes (K, F) from (A, B, W) in the dtype asked for.
Every array carries a seed axis: (B, S, ...).  An instance whose flag is 0 gets NaN rows."""
import numpy as np


def _t(a, dtype):
    return np.asarray(a, dtype=dtype)


def weights(cs, dtype):
    """(wx (B, N, n), wu (B, m)): dt Q at the knots before the last, Qf at the last; dt R"""
    dt = dtype(cs.dt)
    wx = np.repeat((dt * _t(cs.Q, dtype))[:, None], cs.N, axis=1)
    wx[:, -1] = _t(cs.Qf, dtype)
    return wx, dt * _t(cs.R, dtype)


def quu_solve(F, q):
    """-Quu^-1 q from the stored factors: F (B, m, m) with 1 / D on the diagonal and L below it; q (B, S, m)"""
    m = F.shape[-1]
    y = q.copy()
    for a in range(m):
        for c in range(a):
            y[..., a] = y[..., a] - F[:, None, a, c] * y[..., c]
    w = y * np.einsum("baa->ba", F)[:, None]
    for a in range(m - 1, -1, -1):
        for c in range(m - 1, a, -1):
            w[..., a] = w[..., a] - F[:, None, c, a] * w[..., c]
    return -w


def lin(cs, K, F, gx, gu, xi0, dtype=np.float64):
    """gx (B, S, N, n), gu (B, S, N-1, m), xi0 (B, S, n) -> (s0 (B, S, n), xi (B, S, N, n), nu (B, S, N-1, m)).  F None: no
    factors (d = 0: only right for seeds that are zero)."""
    N = cs.N
    A, Bm, K = _t(cs.A, dtype), _t(cs.Bm, dtype), _t(K, dtype)
    gx, gu, xi0 = _t(gx, dtype), _t(gu, dtype), _t(xi0, dtype)
    F = None if F is None else _t(F, dtype)
    d = np.zeros(gu.shape, dtype=dtype)
    s = gx[:, :, N - 1]
    for k in range(N - 2, -1, -1):
        qx = gx[:, :, k] + np.einsum("bij,bsi->bsj", A[:, k], s)
        qu = gu[:, :, k] + np.einsum("bia,bsi->bsa", Bm[:, k], s)
        if F is not None:
            d[:, :, k] = quu_solve(F[:, k], qu)
        s = qx + np.einsum("baj,bsa->bsj", K[:, k], qu)
    xi = np.zeros(gx.shape, dtype=dtype)
    nu = np.zeros(gu.shape, dtype=dtype)
    xi[:, :, 0] = xi0
    for k in range(N - 1):
        nu[:, :, k] = np.einsum("baj,bsj->bsa", K[:, k], xi[:, :, k]) + d[:, :, k]
        xi[:, :, k + 1] = np.einsum("bij,bsj->bsi", A[:, k], xi[:, :, k]) + np.einsum("bia,bsa->bsi", Bm[:, k], nu[:, :, k])
    return s, xi, nu


def _mask(valid, *arrs):
    out = []
    for a in arrs:
        a = a.copy()
        a[np.asarray(valid) == 0] = np.nan
        out.append(a)
    return out


def _zeros(cs, S, dtype):
    return (np.zeros((cs.B, S, cs.N, cs.n), dtype=dtype), np.zeros((cs.B, S, cs.N - 1, cs.m), dtype=dtype),
            np.zeros((cs.B, S, cs.n), dtype=dtype))


def vjp(cs, K, F, valid, gX=None, gU=None, dtype=np.float64):
    """-> (gx0, gXref, gUref)"""
    S = (gX if gX is not None else gU).shape[1]
    zx, zu, z0 = _zeros(cs, S, dtype)
    wx, wu = weights(cs, dtype)
    s0, xi, nu = lin(cs, K, F, zx if gX is None else gX, zu if gU is None else gU, z0, dtype)
    return _mask(valid, s0, -(wx[:, None] * xi), -(wu[:, None, None] * nu))


def jvp(cs, K, F, valid, vx0=None, vXref=None, vUref=None, dtype=np.float64):
    """-> (dX, dU)"""
    S = next(a for a in (vx0, vXref, vUref) if a is not None).shape[1]
    zx, zu, z0 = _zeros(cs, S, dtype)
    wx, wu = weights(cs, dtype)
    gx = zx if vXref is None else -(wx[:, None] * _t(vXref, dtype))
    gu = zu if vUref is None else -(wu[:, None, None] * _t(vUref, dtype))
    _, xi, nu = lin(cs, K, F, gx, gu, z0 if vx0 is None else vx0, dtype)
    return _mask(valid, xi, nu)


# ------------------------------------------------------------------ no solver data: Riccati gains and the dense KKT Jacobian
def ldl(M):
    """F (B, m, m) of M = L D L' (B, m, m): 1 / D on the diagonal, L below it, 0 above; in M's dtype"""
    Bn, m = M.shape[0], M.shape[-1]
    a = M.copy()
    F = np.zeros_like(M)
    one = M.dtype.type(1)
    for j in range(m):
        inv = one / a[:, j, j]
        F[:, j, j] = inv
        f = a[:, j + 1:, j] * inv[:, None]
        a[:, j + 1:, j + 1:] = a[:, j + 1:, j + 1:] - a[:, j + 1:, j, None] * f[:, None, :]
        F[:, j + 1:, j] = f
    return F


def riccati(cs, dtype=np.float64):
    """(K (B, N-1, m, n), F (B, N-1, m, m)) of the unconstrained tracking problem of cs, every operation in `dtype`"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    A, Bm = _t(cs.A, dtype), _t(cs.Bm, dtype)
    wx, wu = weights(cs, dtype)
    K = np.zeros((B, N - 1, m, n), dtype=dtype)
    F = np.zeros((B, N - 1, m, m), dtype=dtype)
    eye_n, eye_m = np.eye(n, dtype=dtype), np.eye(m, dtype=dtype)
    P = wx[:, N - 1, :, None] * eye_n
    half = dtype(0.5)
    for k in range(N - 2, -1, -1):
        PA, PB = P @ A[:, k], P @ Bm[:, k]
        At, Bt = np.swapaxes(A[:, k], -1, -2), np.swapaxes(Bm[:, k], -1, -2)
        Qxx = wx[:, k, :, None] * eye_n + At @ PA
        Quu = wu[:, :, None] * eye_m + Bt @ PB
        Qux = Bt @ PA
        F[:, k] = ldl(Quu)
        K[:, k] = np.swapaxes(quu_solve(F[:, k], np.swapaxes(Qux, -1, -2)), -1, -2)
        P = Qxx + np.swapaxes(Qux, -1, -2) @ K[:, k]
        P = half * (P + np.swapaxes(P, -1, -2))
    return K, F


def gauss_solve(M, R):
    """M^-1 R by Gaussian elimination with partial pivoting in the dtype of M (numpy's LAPACK has no long double): M (B, p, p),
    R (B, p, q)"""
    Bn, p = M.shape[0], M.shape[1]
    W = np.concatenate([M, R], axis=2).copy()
    idx = np.arange(Bn)
    for j in range(p):
        piv = j + np.abs(W[:, j:, j]).argmax(axis=1)
        rj, rp = W[idx, j].copy(), W[idx, piv].copy()
        W[idx, j], W[idx, piv] = rp, rj
        W[:, j] = W[:, j] / W[:, j, j, None]
        fac = W[:, :, j].copy()
        fac[:, j] = 0
        W[:, :, j:] = W[:, :, j:] - fac[:, :, None] * W[:, j, None, j:]      # (row j is zero left of its pivot: those columns do not change)
    return W[:, :, p:]


def dense_jacobian(cs, dtype=np.longdouble):
    """The exact Jacobian of the minimiser of the UNCONSTRAINED tracking problem of cs -- affine in (x0, Xref, Uref) -- from one
    dense KKT solve per instance, built from A, B and the weights alone: J (B, N n + (N-1) m, n + N n + (N-1) m), rows (X, U)
    flattened, columns (x0, Xref, Uref) flattened.
      minimise 1/2 sum_k |x_k - xref_k|^2_w + 1/2 sum_k |u_k - uref_k|^2_{dt R}   s.t.  x_{k+1} = A_k x_k + B_k u_k + f_k,  x_0 given
    unknowns z = (x_1 .. x_{N-1}, u_0 .. u_{N-2}) and one multiplier per dynamics row:
      [H C'; C 0] [z; lam] = [w xref, dt R uref; f_0 + A_0 x0, f_1, ..]"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    A, Bm = _t(cs.A, dtype), _t(cs.Bm, dtype)
    wx, wu = weights(cs, dtype)
    nxv, nuv = (N - 1) * n, (N - 1) * m
    nzv, nc = nxv + nuv, (N - 1) * n
    nin = n + N * n + nuv
    M = np.zeros((B, nzv + nc, nzv + nc), dtype=dtype)
    R = np.zeros((B, nzv + nc, nin), dtype=dtype)
    ar = np.arange
    for k in range(1, N):      # x_k: rows / columns (k - 1) n ..
        o = (k - 1) * n
        M[:, o + ar(n), o + ar(n)] = wx[:, k]
        R[:, o + ar(n), n + k * n + ar(n)] = wx[:, k]                    # d rhs / d xref_k
    for k in range(N - 1):
        o = nxv + k * m
        M[:, o + ar(m), o + ar(m)] = wu
        R[:, o + ar(m), n + N * n + k * m + ar(m)] = wu                  # d rhs / d uref_k
    for k in range(N - 1):     # x_{k+1} - A_k x_k - B_k u_k = f_k
        r = nzv + k * n
        M[:, r + ar(n), k * n + ar(n)] = 1
        if k > 0:
            M[:, r:r + n, (k - 1) * n:k * n] = -A[:, k]
        else:
            R[:, r:r + n, 0:n] = A[:, 0]                                 # d rhs / d x0
        M[:, r:r + n, nxv + k * m:nxv + (k + 1) * m] = -Bm[:, k]
    M[:, :nzv, nzv:] = np.swapaxes(M[:, nzv:, :nzv], -1, -2)
    sol = gauss_solve(M, R)
    J = np.zeros((B, N * n + nuv, nin), dtype=dtype)
    J[:, ar(n), ar(n)] = 1                                               # x_0 = x0
    J[:, n:N * n] = sol[:, :nxv]
    J[:, N * n:] = sol[:, nxv:nzv]
    return J


def dense_jvp(J, cs, vx0, vXref, vUref):
    """(dX, dU) (B, S, ..) of the Jacobian J along the tangents (B, S, ..)"""
    S = vx0.shape[1]
    v = np.concatenate([vx0.reshape(cs.B, S, -1), vXref.reshape(cs.B, S, -1), vUref.reshape(cs.B, S, -1)], axis=2).astype(J.dtype)
    o = np.einsum("boi,bsi->bso", J, v)
    return o[:, :, :cs.N * cs.n].reshape(cs.B, S, cs.N, cs.n), o[:, :, cs.N * cs.n:].reshape(cs.B, S, cs.N - 1, cs.m)


def dense_vjp(J, cs, gX, gU):
    """(gx0, gXref, gUref) (B, S, ..) of the Jacobian J against the seeds (B, S, ..)"""
    S = gX.shape[1]
    g = np.concatenate([gX.reshape(cs.B, S, -1), gU.reshape(cs.B, S, -1)], axis=2).astype(J.dtype)
    o = np.einsum("boi,bso->bsi", J, g)
    n, N = cs.n, cs.N
    return (o[:, :, :n], o[:, :, n:n + N * n].reshape(cs.B, S, N, n), o[:, :, n + N * n:].reshape(cs.B, S, N - 1, cs.m))
