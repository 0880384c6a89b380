"""numpy yardstick of altro_batch_evaluate (rollout, plain cost, maximum violation, dynamics defect), the rounding bounds the
tests hold it to, and the small problems they run on.  Shared by tests/test_evaluate_api.py (which compares this yardstick
with the CPU oracle) and tests/test_evaluate_gpu.py (which compares the device with this yardstick).

Bounds (u = 2^-53, nz = n + m, T = N nz), all derived, none measured:
 1. one dynamics row is a chain of nz fused multiply-adds from f_i (the device), or nz products and nz additions (numpy): either
    way the computed value differs from the exact one by at most (nz + 1) u S_i + O(u^2), S_i = (|A||x| + |B||u| + |f|)_i
    (Higham, Accuracy and Stability, (3.5): gamma_{nz+1}).  Two computations of the same row therefore differ by at most
    2 (nz + 1) u S_i; the tests allow 2 (nz + 2) u S_i.
 2. the defect is a maximum of |row - x_{k+1}|: 1-Lipschitz in the row, so bound 1 carries over, plus one rounding of the
    subtraction (<= u |row - x|, covered by the slack between nz + 1 and nz + 2 whenever the defect is below S).
 3. J is a sum of T + n non-negative terms, each with three roundings (e e, w (e e), and dt Q formed once); any order of
    summation has relative error <= (terms - 1 + 3) u: |dJ| <= (T + 8) u J for each computation, 2 (T + 8) u J between two.
 4. a LINEAR row is a dynamics row with b_r in place of f_i: E_r = 2 (nz + 2) u (|A_r||z| + |b_r|); |v| and max(0, v) are
    1-Lipschitz.  A BOX side is one subtraction of two given doubles: both computations round the same exact value, they
    agree to 2 u (|z| + |bound|) (in fact exactly).  v -> v - Proj(v) is the projection onto the polar cone, nonexpansive in
    the 2-norm, so an error of at most E in each of the p rows moves every element of the residual by at most sqrt(p) E; the
    projection itself (a norm of <= 3 squares, a division, two products and a subtraction) adds <= 16 u |v|_2.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

U_ = 2.0 ** -53


@dataclass
class Con:
    kind: str                 # "box" | "lin" | "soc"
    k0: int                   # 0-based inclusive knot range
    k1: int
    zmin: Optional[np.ndarray] = None   # box: (B, nz)
    zmax: Optional[np.ndarray] = None
    A: Optional[np.ndarray] = None      # lin / soc: (B, nk, p, nz)
    b: Optional[np.ndarray] = None      # (B, nk, p)
    eq: bool = False


@dataclass
class Case:
    """per-instance data of a batch, everything expanded to one row per instance"""
    B: int
    n: int
    m: int
    N: int
    dt: float
    A: np.ndarray             # (B, N-1, n, n)
    Bm: np.ndarray            # (B, N-1, n, m)
    f: np.ndarray             # (B, N-1, n)
    Q: np.ndarray             # (B, n)
    R: np.ndarray             # (B, m)
    Qf: np.ndarray            # (B, n)
    Xref: np.ndarray          # (B, N, n)
    Uref: np.ndarray          # (B, N-1, m)
    x0: np.ndarray            # (B, n)
    cons: List[Con] = field(default_factory=list)


def rollout(cs, U, x0=None):
    """X (B, ncand, N, n) of U (B, ncand, N-1, m), plain numpy"""
    B, nc = U.shape[:2]
    X = np.zeros((B, nc, cs.N, cs.n))
    X[:, :, 0] = (cs.x0 if x0 is None else x0)[:, None]
    for k in range(cs.N - 1):
        X[:, :, k + 1] = np.einsum("bij,bcj->bci", cs.A[:, k], X[:, :, k]) + np.einsum("bij,bcj->bci", cs.Bm[:, k], U[:, :, k]) + cs.f[:, None, k]
    return X


def step_residual(cs, X, U):
    """(|x_{k+1} - (A x_k + B u_k + f)|, S) per (b, c, k, i): bound 1 says residual <= 2 (nz + 2) u S for a rollout's own states"""
    pred = np.einsum("bkij,bckj->bcki", cs.A, X[:, :, :-1]) + np.einsum("bkij,bckj->bcki", cs.Bm, U) + cs.f[:, None]
    S = (np.einsum("bkij,bckj->bcki", np.abs(cs.A), np.abs(X[:, :, :-1])) + np.einsum("bkij,bckj->bcki", np.abs(cs.Bm), np.abs(U))
         + np.abs(cs.f)[:, None])
    return np.abs(pred - X[:, :, 1:]), S


def step_bound(cs, S):
    return 2 * (cs.n + cs.m + 2) * U_ * S


def defect(cs, X, U):
    res, S = step_residual(cs, X, U)
    return res.max(axis=(2, 3)), step_bound(cs, S).max(axis=(2, 3))


def cost(cs, X, U, Xref=None, Uref=None):
    """(J, bound 3) per (b, c)"""
    Xr = cs.Xref if Xref is None else Xref
    Ur = cs.Uref if Uref is None else Uref
    ex, eu = X - Xr[:, None], U - Ur[:, None]
    J = (0.5 * cs.dt * (np.einsum("bi,bcki->bc", cs.Q, ex[:, :, :-1] ** 2) + np.einsum("bi,bcki->bc", cs.R, eu ** 2))
         + 0.5 * np.einsum("bi,bci->bc", cs.Qf, ex[:, :, -1] ** 2))
    return J, 2 * (cs.N * (cs.n + cs.m) + 8) * U_ * J


def soc_residual(v):
    """||Proj(v) - v||_inf for one cone value v (p,)"""
    s, t = v[:-1], v[-1]
    ns = np.linalg.norm(s)
    if ns <= t:
        return 0.0
    if ns <= -t:
        return float(np.abs(v).max())
    c = 0.5 * (1 + t / ns)
    return float(np.abs(np.r_[c * s, c * ns] - v).max())


def violation(cs, X, U, cons=None):
    """(c_max, bound 4) per (b, c): the oracle's con_violation on every constraint and every knot of its range"""
    cons = cs.cons if cons is None else cons
    B, nc = U.shape[:2]
    n, m, N = cs.n, cs.m, cs.N
    nz = n + m
    Z = np.zeros((B, nc, N, nz))
    Z[..., :n] = X
    Z[:, :, :-1, n:] = U
    cm, bd = np.zeros((B, nc)), np.zeros((B, nc))
    for c in cons:
        for k in range(c.k0, c.k1 + 1):
            z = Z[:, :, k]
            if c.kind == "box":
                cols = n if k == N - 1 else nz
                for lo, side in ((False, c.zmax), (True, c.zmin)):
                    bnd = side[:, None, :cols]
                    fin = np.isfinite(bnd)
                    v = np.where(fin, (bnd - z[..., :cols]) if lo else (z[..., :cols] - bnd), 0.0)
                    cm = np.maximum(cm, np.maximum(v, 0.0).max(axis=-1))
                    bd = np.maximum(bd, np.where(fin, 2 * U_ * (np.abs(z[..., :cols]) + np.abs(np.where(fin, bnd, 0.0))), 0.0).max(axis=-1))
                continue
            Ak, bk = c.A[:, k - c.k0], c.b[:, k - c.k0]
            v = np.einsum("bpj,bcj->bcp", Ak, z) + bk[:, None]
            E = 2 * (nz + 2) * U_ * (np.einsum("bpj,bcj->bcp", np.abs(Ak), np.abs(z)) + np.abs(bk)[:, None])
            if c.kind == "lin":
                viol = np.abs(v) if c.eq else np.maximum(v, 0.0)
                cm = np.maximum(cm, viol.max(axis=-1))
                bd = np.maximum(bd, E.max(axis=-1))
            else:
                p = v.shape[-1]
                res = np.array([[soc_residual(v[b, q]) for q in range(nc)] for b in range(B)])
                cm = np.maximum(cm, res)
                bd = np.maximum(bd, np.sqrt(p) * E.max(axis=-1) + 16 * U_ * np.linalg.norm(v, axis=-1))
    return cm, bd


# ---------------------------------------------------------------------------------------------- problems
def make_case(B, n, m, N, seed, per_knot_dyn=False, per_instance_dyn=True, per_instance_cost=False, affine=True, dt=0.1):
    rng = np.random.default_rng(seed)
    nb = N - 1 if per_knot_dyn else 1
    lead = (B, nb) if per_instance_dyn else (1, nb)
    A = np.eye(n) + 0.3 * rng.standard_normal(lead + (n, n)) / np.sqrt(n)
    Bm = 0.5 * rng.standard_normal(lead + (n, m))
    f = 0.05 * rng.standard_normal(lead + (n,)) if affine else np.zeros(lead + (n,))
    full = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B, N - 1) + a.shape[2:]))
    cl = (B,) if per_instance_cost else (1,)
    Q, R = 1.0 + 9.0 * rng.random(cl + (n,)), 0.1 + rng.random(cl + (m,))
    Qf = (N - 1) * Q
    bc = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape[1:]))
    return Case(B, n, m, N, dt, full(A), full(Bm), full(f), bc(Q), bc(R), bc(Qf), rng.standard_normal((B, N, n)),
                0.3 * rng.standard_normal((B, N - 1, m)), rng.standard_normal((B, n)))


def add_box(cs, u_bnd, x_bnd=None, k0=0, k1=None):
    """|u| <= u_bnd ((B, m), (m,) or scalar); optionally x_j <= x_bnd on the even states and x_j >= -x_bnd on every third"""
    nz = cs.n + cs.m
    zmin, zmax = np.full((cs.B, nz), -np.inf), np.full((cs.B, nz), np.inf)
    ub = np.broadcast_to(np.asarray(u_bnd, dtype=np.float64), (cs.B, cs.m))
    zmin[:, cs.n:], zmax[:, cs.n:] = -ub, ub
    if x_bnd is not None:
        zmax[:, 0:cs.n:2] = x_bnd
        zmin[:, 0:cs.n:3] = -x_bnd
    cs.cons.append(Con("box", k0, cs.N - 2 if k1 is None else k1, zmin=zmin, zmax=zmax))
    return cs


def add_rows(cs, kind, A, b, k0, k1, eq=False):
    """A (p, nz) | (nk, p, nz) | (B, nk, p, nz): expanded to one block per instance and knot"""
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nk = k1 - k0 + 1
    A4 = np.broadcast_to(A if A.ndim == 4 else A[None] if A.ndim == 3 else A[None, None], (cs.B, nk) + A.shape[-2:])
    b3 = np.broadcast_to(b if b.ndim == 3 else b[None] if b.ndim == 2 else b[None, None], (cs.B, nk) + b.shape[-1:])
    cs.cons.append(Con(kind, k0, k1, A=np.ascontiguousarray(A4), b=np.ascontiguousarray(b3), eq=eq))
    return cs


def candidates(cs, seed, scale_in=0.03, push=3.0):
    """U (B, 3, N-1, m): candidate 0 small (inside every control constraint of the cases below by construction: the control
    bounds, the negative offsets of the inequality rows and the positive offsets of the cones all leave a ball around u = 0
    free), candidate 1 pushed outside the control bounds / rows, candidate 2 random"""
    rng = np.random.default_rng(seed)
    B, N, m = cs.B, cs.N, cs.m
    box = next((c for c in cs.cons if c.kind == "box"), None)
    ub = box.zmax[:, None, cs.n:] if box is not None and np.isfinite(box.zmax[:, cs.n:]).all() else np.full((B, 1, m), 1.0)
    U = np.empty((B, 3, N - 1, m))
    U[:, 0] = np.clip(scale_in * ub * rng.standard_normal((B, N - 1, m)), -0.9 * ub, 0.9 * ub)
    U[:, 1] = U[:, 0]
    U[:, 1, N // 2] = push * ub[:, 0] * np.where(rng.random((B, m)) < 0.5, -1.0, 1.0)
    U[:, 2] = ub * rng.standard_normal((B, N - 1, m))
    return np.ascontiguousarray(U)


def to_problem(altro, cs, per_knot_dyn=False, shared=()):
    """the altro.Problem of a Case; `shared` names what is handed over as ONE block for the batch ("dyn", "cost", "box",
    or the index of a row constraint) -- the Case then holds B equal copies of it"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    pick = lambda a, name: a[0] if name in shared else a
    if per_knot_dyn:
        model = altro.LinearModel(pick(cs.A, "dyn"), pick(cs.Bm, "dyn"), pick(cs.f, "dyn"), dt=cs.dt, per_knot=True)
    else:
        model = altro.LinearModel(pick(cs.A[:, 0], "dyn"), pick(cs.Bm[:, 0], "dyn"), pick(cs.f[:, 0], "dyn"), dt=cs.dt)
    obj = altro.TrackingObjective(pick(cs.Q, "cost"), pick(cs.R, "cost"), pick(cs.Qf, "cost"), cs.Xref, cs.Uref)
    cons = altro.ConstraintList(n, m, N)
    for i, c in enumerate(cs.cons):
        rng_ = (c.k0 + 1, c.k1 + 1)
        if c.kind == "box":
            zmin, zmax = pick(c.zmin, "box"), pick(c.zmax, "box")
            fin = lambda a: None if not np.isfinite(a).any() else a
            cons.add_constraint(altro.BoundConstraint(n, m, x_min=fin(zmin[..., :n]), x_max=fin(zmax[..., :n]), u_min=fin(zmin[..., n:]),
                                                      u_max=fin(zmax[..., n:])), rng_)
            continue
        sh = i in shared
        A, b = (c.A[0], c.b[0]) if sh else (c.A, c.b)
        if sh and (A == A[:1]).all() and (b == b[:1]).all():   # one block for every knot too
            A, b = A[0], b[0]
        con = altro.NormConstraint(A, b, per_instance=not sh) if c.kind == "soc" else altro.LinearConstraint(A, b, equality=c.eq, per_instance=not sh)
        cons.add_constraint(con, rng_)
    return altro.Problem(model, obj, cons, x0=cs.x0.copy(), N=N, U0=cs.Uref.copy())


def sub_case(cs, b):
    """instance b alone, as a batch of one"""
    sl = lambda a: None if a is None else a[b:b + 1]
    return Case(1, cs.n, cs.m, cs.N, cs.dt, sl(cs.A), sl(cs.Bm), sl(cs.f), sl(cs.Q), sl(cs.R), sl(cs.Qf), sl(cs.Xref), sl(cs.Uref), sl(cs.x0),
                [Con(c.kind, c.k0, c.k1, sl(c.zmin), sl(c.zmax), sl(c.A), sl(c.b), c.eq) for c in cs.cons])


def oracle_of(O, cs, b, per_knot_dyn=False):
    """a fresh OracleSolver (zero duals) holding instance b of the case"""
    s = O.OracleSolver(cs.n, cs.m, cs.N, cs.dt)
    if per_knot_dyn:
        s.set_dynamics(cs.A[b], cs.Bm[b], cs.f[b])
    else:
        s.set_dynamics(cs.A[b, 0], cs.Bm[b, 0], cs.f[b, 0])
    s.set_cost(cs.Q[b], cs.R[b], cs.Qf[b])
    s.set_reference(cs.Xref[b], cs.Uref[b])
    s.set_initial_state(cs.x0[b])
    for c in cs.cons:
        if c.kind == "box":
            s.add_box(c.zmin[b], c.zmax[b], c.k0, c.k1)
        else:
            s.add_affine(O.SOC if c.kind == "soc" else O.LINEAR, O.EQ if c.eq else O.INEQ, c.A[b], c.b[b], c.k0, c.k1)
    s.set_opts(O.default_opts())
    return s


def oracle_scores(O, cs, U, per_knot_dyn=False):
    """(X_orc (B, nc, N, n), J_orc, cmax_orc) of every candidate: set_controls, orc_max_violation, orc_states, orc_cost on a fresh
    oracle with zero duals (its cost then carries no AL term wherever c_max == 0 and there is no equality row)"""
    B, nc = U.shape[:2]
    X, J, cm = np.zeros((B, nc, cs.N, cs.n)), np.zeros((B, nc)), np.zeros((B, nc))
    for b in range(B):
        for c in range(nc):
            s = oracle_of(O, cs, b, per_knot_dyn)
            s.set_controls(U[b, c])
            cm[b, c] = s.max_violation()
            X[b, c] = s.states()
            J[b, c] = s.cost()
    return X, J, cm


def controls_only_box(cs):
    """the case has a BOX and it bounds controls only: candidate 0 is then feasible and candidate 1 infeasible by construction"""
    box = [c for c in cs.cons if c.kind == "box"]
    return bool(box) and not np.isfinite(box[0].zmin[:, :cs.n]).any() and not np.isfinite(box[0].zmax[:, :cs.n]).any()


def case_of_batch(pb, windows, x0):
    """the Case a RandomLinearBatch (problems.gen_random_linear_batch) is at when instance b tracks window windows[b]"""
    B, n, m, N = pb.batch, pb.n, pb.m, pb.N
    full = lambda a: np.ascontiguousarray(np.broadcast_to(a[:, None], (B, N - 1) + a.shape[1:]))
    w = lambda v, k: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (B, k)))
    cs = Case(B, n, m, N, pb.dt, full(pb.A), full(pb.Bm), np.zeros((B, N - 1, n)), w(pb.Qk, n), w(pb.Rk, m), w(pb.Qfk, n),
              np.stack([pb.Xtrack[b, k:k + N] for b, k in enumerate(windows)]), np.stack([pb.Utrack[b, k:k + N - 1] for b, k in enumerate(windows)]),
              np.asarray(x0, dtype=np.float64))
    return add_box(cs, pb.u_bnd)


# the cases of the issue's table --------------------------------------------------------------------
def case_16_box(B=5, N=9, seed=11):
    """(12, 4) on the 16-lane kernels: BOX on the controls with per-instance weights and bounds"""
    cs = make_case(B, 12, 4, N, seed, per_instance_cost=True)
    rng = np.random.default_rng(seed + 1)
    return add_box(cs, 0.5 + rng.random((B, 4)))


def case_16_soc(B=5, N=9, seed=12):
    """(6, 3) on the 16-lane kernels: a cone of dimension 3 on the controls, ||(a0'u, a1'u)|| <= a2'u + t0 with t0 > 0, and one
    inequality row a'u - c <= 0, c > 0; per-knot per-instance tables on knots 0 .. N-2"""
    cs = make_case(B, 6, 3, N, seed)
    rng = np.random.default_rng(seed + 1)
    nk, nz = N - 1, 9
    A = np.zeros((B, nk, 3, nz))
    A[..., 6:] = rng.standard_normal((B, nk, 3, 3))
    b = np.zeros((B, nk, 3))
    b[..., 2] = 1.0 + rng.random((B, nk))
    add_rows(cs, "soc", A, b, 0, N - 2)
    Al = np.zeros((B, nk, 1, nz))
    Al[..., 6:] = rng.standard_normal((B, nk, 1, 3))
    Al[..., :6] = 0.05 * rng.standard_normal((B, nk, 1, 6))
    return add_rows(cs, "lin", Al, -3.0 - rng.random((B, nk, 1)), 0, N - 2)


def case_wide_rows(B=5, N=9, seed=13):
    """(20, 5) on the one-wave-per-instance kernels: BOX plus 40 LINEAR rows (more than 32 lanes of rows): 24 inequality rows on
    knots 0 .. N-2 and 16 on knots 2 .. N-1 (the terminal knot: state columns only), one shared block each"""
    cs = make_case(B, 20, 5, N, seed, per_instance_dyn=False)
    rng = np.random.default_rng(seed + 1)
    add_box(cs, 1.0)
    A1 = np.zeros((24, 25))
    A1[:, 20:] = rng.standard_normal((24, 5))
    add_rows(cs, "lin", A1, -4.0 - rng.random(24), 0, N - 2)
    A2 = 0.02 * rng.standard_normal((16, 25))
    return add_rows(cs, "lin", A2, -3.0 - rng.random(16), 2, N - 1)


def case_wide_ltv(B=5, N=9, seed=14):
    """(12, 12) with per-knot dynamics (the handle moves to the one-wave-per-instance kernels), BOX on the controls"""
    cs = make_case(B, 12, 12, N, seed, per_knot_dyn=True)
    return add_box(cs, 0.8)


def case_wide_cone(B=5, N=9, seed=17):
    """(7, 3): the problem of test_constraint_dev_gpu.py::wide_problem restated -- the box of a random-linear problem, two
    per-knot per-instance inequality rows on the controls, a one-block cone of dimension 3"""
    n, m = 7, 3
    cs = make_case(B, n, m, N, seed, affine=False)
    rng = np.random.default_rng(seed + 1)
    add_box(cs, 1.5)
    A = np.zeros((B, N - 1, 2, n + m))
    A[..., n:] = rng.standard_normal((B, N - 1, 2, m))
    add_rows(cs, "lin", A, -0.5 - rng.random((B, N - 1, 2)), 0, N - 2)
    Ac = np.zeros((3, n + m))
    Ac[0, n], Ac[1, n + 1], Ac[2, n + 2] = 1.0, 1.0, 0.5
    return add_rows(cs, "soc", Ac, np.array([0.0, 0.0, 2.0]), 0, N - 2)


def case_wide_box(B=5, N=9, seed=15):
    """(30, 25): BOX on the controls and on some states, up to the terminal knot (where the largest states are: some instances
    violate a state bound there whatever their controls)"""
    cs = make_case(B, 30, 25, N, seed, per_instance_dyn=False)
    return add_box(cs, 1.0, x_bnd=6.0, k0=0, k1=N - 1)


def case_wide_limits(B=2, N=4, seed=16):
    """(64, 32): the size limits of the library"""
    cs = make_case(B, 64, 32, N, seed)
    return add_box(cs, 1.0)
