"""The projected-Newton polish as a table of cases: the smallest problems that reach each path of csrc/pn_core.h which the
oracle-parity tests leave out.  Shared by tests/test_polish_ref.py (the oracle against the dense yardstick
tests/polish_ref.py, on the CPU) and tests/test_polish_gpu.py (the device against both).

Every problem is an LQ tracking problem with H = dt Q, dt R, Qf between 0.5 and 2 (cond(S) stays small: the default rho_chol = 1e-2
refinement converges), a stable A (0.95 x an orthogonal matrix), a reference that ramps from 0 to a per-instance goal, and
bounds taken from the UNCONSTRAINED optimum of the same instance so that they bind where the case says.  Seeds and fractions
were tuned on the oracle until tests/test_polish_ref.py holds; nothing here depends on the device."""
import functools
from dataclasses import dataclass, field, replace

import numpy as np

import polish_ref
from helpers import REF_OPTS

B = 3
AL_OPTS = dict(REF_OPTS, penalty_initial=10.0, penalty_scaling=10.0, iterations_outer=40)
POLISH = dict(constraint_tolerance=1e-8, projected_newton=1)       # projected_newton_tolerance, active_set_tolerance_pn: 1e-3
BMAX = 56    # csrc/pn_polish.h


@dataclass
class Case:
    id: str
    backend: str              # "lane16" | "wide"
    n: int
    m: int
    N: int
    dt: float
    A: np.ndarray
    Bm: np.ndarray
    f: np.ndarray
    Q: np.ndarray
    R: np.ndarray
    Qf: np.ndarray
    Xref: np.ndarray          # (B, N, n)
    Uref: np.ndarray
    x0: np.ndarray            # (B, n)
    zmin: np.ndarray = None
    zmax: np.ndarray = None
    box_k0: int = 0
    box_k1: int = -1
    rows: list = field(default_factory=list)     # polish_ref.Rows
    opts: dict = field(default_factory=lambda: dict(AL_OPTS, **POLISH))
    reaches: tuple = ()       # the paths this case is listed for (test_polish_ref.test_cases_reach_their_paths)

    @property
    def ltv(self):
        return np.ndim(self.A) == 3

    @property
    def batch(self):
        return self.x0.shape[0]

    def with_opts(self, suffix, **kw):
        return replace(self, id=self.id + suffix, opts=dict(self.opts, **kw))


def _orth(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _free_optimum(c, b):
    """The unconstrained optimum of instance b, dense: min 1/2 (z - zref)' H (z - zref) s.t. initial condition and dynamics."""
    ref = polish_ref.PolishRef(instance(replace(c, zmin=None, zmax=None, rows=[]), b))
    z = ref.zref.copy()
    act = ref.active_rows(z, 0.0)
    return ref.unpack(ref.project(z, act))


def _lq(id, backend, n, m, N, seed, ltv=False, dt=0.1, goal=2.0, x0s=0.5, bscale=1.0, nb=B):
    rng = np.random.default_rng([seed, n, m, N])
    A = 0.95 * _orth(rng, n)
    Bm = bscale * rng.standard_normal((n, m)) / np.sqrt(m)
    f = np.zeros(n)
    if ltv:
        A = A[None] * (1.0 + 0.05 * rng.standard_normal((N - 1, 1, 1)))
        Bm = Bm[None] * (1.0 + 0.05 * rng.standard_normal((N - 1, 1, 1)))
        f = 0.05 * rng.standard_normal((N - 1, n))
    xf = goal * np.sign(rng.standard_normal(n)) * (0.5 + np.abs(rng.standard_normal((nb, n))))   # one sign per coordinate
    ramp = (np.arange(N) / (N - 1.0))[None, :, None]
    x0 = x0s * rng.standard_normal((nb, n))
    # H between 0.5 and 2, a different value in every coordinate: a weight read at the wrong index shows
    Q, R, Qf = (0.5 + 1.5 * rng.random(n)) / dt, (0.5 + 1.5 * rng.random(m)) / dt, 0.5 + 1.5 * rng.random(n)
    return Case(id, backend, n, m, N, dt, A, Bm, f, Q, R, Qf, ramp * xf[:, None, :], np.zeros((nb, N - 1, m)), x0)


def _free(c):
    sols = [_free_optimum(c, b) for b in range(c.batch)]
    return np.array([s[0] for s in sols]), np.array([s[1] for s in sols])


def _control_box(c, frac, Uf):
    ub = frac * np.abs(Uf).max(axis=(1, 2)).min()      # of the smallest peak over the batch: it binds in every instance
    zmax = np.r_[np.full(c.n, np.inf), np.full(c.m, ub)]
    return replace(c, zmin=-zmax, zmax=zmax, box_k0=0, box_k1=c.N - 2)


def _state_box(c, Xf, Uf, ufrac, wide, tight, tfrac, k0=1):
    """Bounds on EVERY coordinate, knots k0..N-1: controls at ufrac of the free peak, states at `wide` times their free peak
    (slack), except the `tight` coordinates: there the side on which the free terminal state lies comes to tfrac of the
    smallest free terminal |x_j| over the batch, which the ramp makes the peak of the trajectory -- it binds at the terminal
    knot, from above where the goal is positive and from below where it is negative."""
    xpk = np.abs(Xf[:, k0:]).max(axis=(0, 1))
    zmax = np.r_[wide * xpk, np.full(c.m, ufrac * np.abs(Uf).max(axis=(1, 2)).min())]
    zmin = -zmax.copy()
    for j in tight:
        t = Xf[:, -1, j]
        assert np.all(t > 0) or np.all(t < 0), ("tight coordinate changes sign over the batch", j, t)
        if t[0] > 0:
            zmax[j] = tfrac * t.min()
        else:
            zmin[j] = tfrac * t.max()
    return replace(c, zmin=zmin, zmax=zmax, box_k0=k0, box_k1=c.N - 1)


def _same_sign_states(Xf, count):
    """`count` state coordinates whose free terminal value has one sign over the batch: first a negative one, then positive."""
    t = Xf[:, -1, :]
    neg = [j for j in range(t.shape[1]) if np.all(t[:, j] < -0.3)]
    pos = [j for j in range(t.shape[1]) if np.all(t[:, j] > 0.3)]
    assert neg and pos, "no coordinate with a common sign: another seed"
    return (neg[:1] + pos)[:count]


@functools.lru_cache(maxsize=None)
def case(id):
    return {c.id: c for c in _table()}[id]


@functools.lru_cache(maxsize=None)
def _table():
    out = []
    # ---- a. 16-lane
    c = _lq("l16-bmax", "lane16", 12, 4, 9, seed=1)
    Xf, Uf = _free(c)
    c = _state_box(c, Xf, Uf, 0.6, 1.5, _same_sign_states(Xf, 2), 0.9)
    out.append(replace(c, reaches=("bm==BMAX", "box_k0>0", "state bound", "terminal row", "lower side")))
    c = _lq("l16-long", "lane16", 6, 3, 70, seed=2, goal=4.0)
    Xf, Uf = _free(c)
    out.append(replace(_control_box(c, 0.6, Uf), reaches=("N>64", "lower side")))
    c = _lq("l16-rows", "lane16", 8, 4, 9, seed=3)
    Xf, Uf = _free(c)
    c = _control_box(c, 0.7, Uf)
    out.append(replace(c, rows=_linear_rows(c, Xf, Uf, seed=3), reaches=("linear rows", "terminal equality")))
    # ---- b. wide
    c = _lq("w-long", "wide", 5, 2, 70, seed=4, goal=4.0)
    Xf, Uf = _free(c)
    out.append(replace(_control_box(c, 0.6, Uf), reaches=("N>64", "lower side")))
    c = _lq("w-40x6", "wide", 40, 6, 8, seed=5)
    Xf, Uf = _free(c)
    c = _state_box(c, Xf, Uf, 0.6, 1.5, _same_sign_states(Xf, 3), 0.9)
    out.append(replace(c, reaches=("rows>64", "n+m>32", "state bound", "terminal row", "lower side", "box_k0>0")))
    c = _lq("w-64x16", "wide", 64, 16, 8, seed=6)
    Xf, Uf = _free(c)
    out.append(replace(_control_box(c, 0.6, Uf), reaches=("rows>64", "n+m>32", "lower side")))
    c = _lq("w-48x32", "wide", 48, 32, 6, seed=7)
    Xf, Uf = _free(c)
    out.append(replace(_control_box(c, 0.6, Uf), reaches=("rows>64", "n+m>32", "lower side")))
    c = _lq("w-ltv", "wide", 30, 6, 8, seed=8, ltv=True)
    Xf, Uf = _free(c)
    out.append(replace(_control_box(c, 0.6, Uf), reaches=("per-knot dynamics", "n+m>32", "lower side")))
    out.append(_from_wide_matrix("40x6-r10"))
    # ---- c. rho_chol = 1e-8: the refinement converges at once
    by = {c.id: c for c in out}
    out.append(by["l16-bmax"].with_opts("-rho1e-8", rho_chol=1e-8))
    out.append(by["w-40x6"].with_opts("-rho1e-8", rho_chol=1e-8))
    # ---- e / f. a control with lo == hi: both sides active.  dt R = 1 and rho_primal = 0 make 1 / (h + rho_primal) exactly 1,
    # so with rho_chol = 0 the second pivot is exactly 1 - 1 = 0 (failed = 1); with the default rho_chol the polish succeeds
    for id, backend, n, m, N, seed in (("l16-dup", "lane16", 6, 3, 9, 10), ("w-dup", "wide", 5, 2, 9, 11)):
        c = _lq(id, backend, n, m, N, seed=seed, dt=0.5)
        Xf, Uf = _free(c)
        c = _control_box(c, 0.7, Uf)
        c.zmin[n] = c.zmax[n] = 0.25 * c.zmax[n]
        c.R[0] = 1.0 / c.dt
        c = replace(c, opts=dict(c.opts, rho_primal=0.0), reaches=("duplicated row",))
        out.append(c)
        out.append(replace(c.with_opts("-fail", rho_chol=0.0), reaches=("failed=1",)))
    return tuple(out)


def _from_wide_matrix(wid):
    """A rows problem of tests/wide_matrix.py (Q = 10, R = 0.1: H = 1 and 0.01) with its cone taken out: mixing inequality
    rows, a terminal equality, a box on some controls and a bound on the last state as a linear row on knots 1..N-1."""
    import wide_matrix as WM
    from altro_mpc_icra2021_amd import problems as P
    pr = WM.rows_problem(WM.CASE_BY_ID[wid])
    rp, nb = pr.rp, len(pr.x0)
    box = [s for s in rp.constraints if s.kind == P.BOX][0]
    rows = [polish_ref.Rows(s.sense == P.EQ, s.A, s.b, s.k_first, s.k_last) for s in rp.constraints if s.kind == P.LINEAR]
    return Case("w-rows40", "wide", rp.n, rp.m, rp.N, rp.dt, rp.A, rp.Bm, rp.f, rp.Q, rp.R, rp.Qf, np.tile(rp.xf, (nb, rp.N, 1)),
                np.zeros((nb, rp.N - 1, rp.m)), pr.x0.copy(), box.zmin, box.zmax, box.k_first, box.k_last, rows,
                dict(pr.opts, **POLISH), ("rows>64", "n+m>32", "linear rows", "terminal equality"))


def _linear_rows(c, Xf, Uf, seed):
    """Two inequality rows mixing states and controls on knots 2..N-3 at 0.7 of their free peak, one equality row on the
    controls at knots 1..3, and a terminal equality on half of the states (ncol = n) at 0.8 of the free terminal state of
    instance 0."""
    rng = np.random.default_rng([seed, 77])
    n, m, N, nz = c.n, c.m, c.N, c.n + c.m
    Zf = np.concatenate([Xf[:, :N - 1], Uf], axis=-1)
    Ai = np.zeros((2, nz))
    Ai[:, :n] = 0.3 * rng.standard_normal((2, n)) / np.sqrt(n)
    Ai[:, n:] = rng.standard_normal((2, m))
    vals = Zf[:, 2:N - 2] @ Ai.T
    hi, lo = vals.max(axis=(0, 1)), vals.min(axis=(0, 1))
    flip = -lo > hi
    Ai[flip] *= -1.0
    peak = np.where(flip, -lo, hi)
    Ae = np.zeros((1, nz)); Ae[0, n:] = rng.standard_normal(m)
    ne = n // 2
    Ag = np.zeros((ne, nz)); Ag[:, :ne] = np.eye(ne)
    return [polish_ref.Rows(False, Ai, -0.7 * peak, 2, N - 3),
            polish_ref.Rows(True, Ae, np.zeros(1), 1, 3),
            polish_ref.Rows(True, Ag, -0.8 * Xf[0, -1, :ne], N - 1, N - 1)]


CASE_IDS = ("l16-bmax", "l16-long", "l16-rows", "w-long", "w-40x6", "w-64x16", "w-48x32", "w-ltv", "w-rows40",
            "l16-bmax-rho1e-8", "w-40x6-rho1e-8", "l16-dup", "w-dup")
FAIL_IDS = ("l16-dup-fail", "w-dup-fail")


def refusal_case():
    """d. (12, 4) with all 16 coordinates bounded (bm = 56 = BMAX) plus one linear row: 72 rows, more than pn_polish.h holds."""
    c = case("l16-bmax")
    Ar = np.zeros((1, c.n + c.m)); Ar[0, c.n] = 1.0
    return replace(c, id="l16-refusal", rows=[polish_ref.Rows(False, Ar, np.array([-10.0]), 0, c.N - 2)])


# ---------------------------------------------------------------------------------------------------------------------
# the same problem for the yardstick, the oracle and the library
def instance(c, b, opts=None):
    o = c.opts if opts is None else opts
    return polish_ref.Instance(c.n, c.m, c.N, c.dt, c.A, c.Bm, c.f, c.Q, c.R, c.Qf, o.get("rho_primal", 1e-8), c.Xref[b], c.Uref[b],
                               c.x0[b], c.zmin, c.zmax, c.box_k0, c.box_k1, c.rows)


def make_oracle(O, c, b, **over):
    s = O.OracleSolver(c.n, c.m, c.N, c.dt)
    s.set_dynamics(c.A, c.Bm, c.f)
    s.set_cost(c.Q, c.R, c.Qf)
    s.set_reference(c.Xref[b], c.Uref[b])
    s.set_initial_state(c.x0[b])
    s.set_controls(np.zeros((c.N - 1, c.m)))
    s.con_ids = []
    if c.zmax is not None:
        s.con_ids.append(s.add_box(c.zmin, c.zmax, c.box_k0, c.box_k1))
    for r in c.rows:
        s.con_ids.append(s.add_affine(O.LINEAR, O.EQ if r.equality else O.INEQ, r.A, r.b, r.k0, r.k1))
    s.set_opts(O.default_opts(**dict(c.opts, **over)))
    return s


def twin_opts(c):
    """The AL stage alone: what both backends and the oracle hand their solve with the polish on."""
    return dict(projected_newton=0, constraint_tolerance=c.opts.get("projected_newton_tolerance", 1e-3))


@dataclass
class OracleRun:
    X: np.ndarray
    U: np.ndarray
    status: int
    iterations: int
    cost: float
    c_max: float
    pn_ran: int
    pn_failed: int
    pn_residual: float
    pn_dual_failed: int
    r0: float
    r1: float
    box_duals: np.ndarray
    row_duals: list


def oracle_run(O, c, b, **over):
    s = make_oracle(O, c, b, **over)
    so = s.solve()
    ids = list(s.con_ids)
    box = None
    if c.zmax is not None:
        box = s.duals(ids.pop(0)).reshape(c.box_k1 - c.box_k0 + 1, 2, c.n + c.m)
    rows = [s.duals(i).reshape(r.k1 - r.k0 + 1, r.A.shape[0]) for i, r in zip(ids, c.rows)]
    return OracleRun(s.states(), s.controls(), so.status, so.iterations, so.cost, so.c_max, so.pn_ran, so.pn_failed, so.pn_residual,
                     so.pn_dual_failed, so.pn_dual_residual0, so.pn_dual_residual, box, rows)


@functools.lru_cache(maxsize=None)
def oracle_pair(id, b):
    """(AL-stage twin, polished run) of instance b on the oracle, computed once per session."""
    import oracle_py as O
    O.build()
    c = case(id) if id != "l16-refusal" else refusal_case()
    return oracle_run(O, c, b, **twin_opts(c)), oracle_run(O, c, b)


def gpu_problem(altro, c):
    """The same batch for the library."""
    model = altro.LinearModel(c.A, c.Bm, c.f, dt=c.dt, per_knot=True) if c.ltv else altro.LinearModel(c.A, c.Bm, c.f, dt=c.dt)
    obj = altro.TrackingObjective(c.Q, c.R, c.Qf, c.Xref.copy(), c.Uref.copy())
    cons = altro.ConstraintList(c.n, c.m, c.N)
    if c.zmax is not None:
        def side(v, fill):
            return None if np.all(v == fill) else v
        cons.add_constraint(altro.BoundConstraint(c.n, c.m, x_min=side(c.zmin[:c.n], -np.inf), x_max=side(c.zmax[:c.n], np.inf),
                                                  u_min=side(c.zmin[c.n:], -np.inf), u_max=side(c.zmax[c.n:], np.inf)),
                            (c.box_k0 + 1, c.box_k1 + 1))
    for r in c.rows:
        cons.add_constraint(altro.LinearConstraint(r.A, r.b, equality=r.equality), (r.k0 + 1, r.k1 + 1))
    return altro.Problem(model, obj, cons, x0=c.x0.copy(), N=c.N, U0=np.zeros((c.batch, c.N - 1, c.m)))


# ---------------------------------------------------------------------------------------------------------------------
# what the yardstick says about one polished trajectory (the oracle's on the CPU, the device's on the GPU)
@dataclass
class Verdict:
    admissible: bool
    why: str
    ratios: dict          # check -> error / bound


def admissibility(c, b):
    """The closed form applies only where the yardstick, the oracle and the device cannot disagree on the active set, and
    the oracle's polish converged: decided on the CPU, from the oracle alone."""
    tw, po = oracle_pair(c.id, b)
    ref = polish_ref.PolishRef(instance(c, b))
    tol = c.opts.get("active_set_tolerance_pn", 1e-3)
    a0 = ref.active_rows(ref.pack(tw.X, tw.U), tol)
    a1 = ref.active_rows(ref.pack(po.X, po.U), tol)
    if not po.pn_ran:
        return False, "the polish did not run"
    if po.pn_failed:
        return False, "the polish failed"
    if not po.pn_residual < c.opts["constraint_tolerance"]:
        return False, "the oracle's polish ended at %.3g" % po.pn_residual
    if a0.labels != a1.labels:
        return False, "the active set differs between the AL-stage and the polished trajectory"
    if min(a0.margin, a1.margin) < 1e-6:
        return False, "an inequality row lies within 1e-6 of the active-set threshold"
    return True, ""


def judge(c, b, z0XU, z1XU, box_duals, row_duals, r0, r1, admissible):
    """Range, closed form and both dual residuals of one polished trajectory against the yardstick: error / bound each."""
    ref = polish_ref.PolishRef(instance(c, b))
    tol, ctol = c.opts.get("active_set_tolerance_pn", 1e-3), c.opts["constraint_tolerance"]
    z0, z1 = ref.pack(*z0XU), ref.pack(*z1XU)
    a0, a1 = ref.active_rows(z0, tol), ref.active_rows(z1, tol)
    Du = ref.union(a0, a1)
    ratios = {"range": ref.out_of_range(z1 - z0, Du) / ref.range_bound(z0, z1, a0, Du)}
    lam0 = ref.lam0(a1, box_duals, row_duals)
    y0, yls = ref.dual_residuals(z1, a1, lam0)
    ratios["r0"] = abs(r0 - y0) / (ref.r0_bound(z1, a1, lam0) + ref.len * polish_ref.U_ROUND * y0)
    if admissible:
        zs = ref.project(z0, a0)
        ratios["closed form"] = float(np.abs(z1 - zs).max()) / ref.closed_form_bound(z0, z1, a0, ctol)
        slack = ref.r1_slack(a1) + ref.r0_bound(z1, a1, lam0) + ref.len * polish_ref.U_ROUND * y0
        ratios["r1 above r_ls"] = max(0.0, yls - r1) / slack
        ratios["r1 below r0"] = max(0.0, r1 - r0) / slack
        ratios["r1 near r_ls"] = max(0.0, r1 - yls) / slack
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# the device
@dataclass
class DeviceRun:
    X: np.ndarray
    U: np.ndarray
    status: np.ndarray
    iterations: np.ndarray
    cost: np.ndarray
    c_max: np.ndarray
    ran: np.ndarray
    failed: np.ndarray
    residual: np.ndarray
    r0: np.ndarray
    r1: np.ndarray
    dual_failed: np.ndarray
    duals: list              # per constraint, as altro.get_duals returns them: box (B, nk, 2, nz) first, then the row blocks
    wide: bool


def device_solve(altro, c, **over):
    """One solve of the batch on a fresh handle."""
    sv = altro.ALTROSolver(gpu_problem(altro, c), altro.SolverOptions(**dict(c.opts, **over)))
    try:
        altro.solve(sv)
        return read_device(altro, sv)
    finally:
        sv.close()


def read_device(altro, sv):
    st = altro.stats(sv)
    ran, failed, res = altro.polish_stats(sv)
    d0, d1, dfail = altro.polish_dual_residuals(sv)
    duals = [altro.get_duals(sv, i) for i in range(len(sv.prob.constraints.items))]
    return DeviceRun(altro.states(sv), altro.controls(sv), st.status.copy(), st.iterations.copy(), st.cost.copy(), st.c_max.copy(),
                     ran, failed, res, d0, d1, dfail, duals, altro.wave_cycles(sv).size == 0)


def device_pair(altro, c):
    """(AL-stage twin, polished run) on the device: the twin is handed exactly the options the solve kernel of the polished
    handle gets (projected_newton = 0, constraint_tolerance = projected_newton_tolerance)."""
    return device_solve(altro, c, **twin_opts(c)), device_solve(altro, c)


def judge_device(c, b, tw, po):
    """judge() on instance b of a device pair; the closed form where the ORACLE says it applies."""
    ok, why = admissibility(c, b)
    box = po.duals[0][b] if c.zmax is not None else None
    rows = [d[b] for d in po.duals[(1 if c.zmax is not None else 0):]]
    return judge(c, b, (tw.X[b], tw.U[b]), (po.X[b], po.U[b]), box, rows, po.r0[b], po.r1[b], ok), ok, why
