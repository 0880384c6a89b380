"""The horizon axis of the one-wave-per-instance backend as a table: every horizon-periodic loop of solve_wide.h with its period
and lookahead, the horizons that reach each loop's group, remainder and end-of-horizon edges, and the recipes of the problems
run at them -- one smallest shape per code path (tests/wide_matrix.py has the instantiations, all at N = 12).  Shared by
tests/test_wide_horizons.py (periods against the source, edge coverage, the dispatch restated, and the conditions on the
INPUTS, on the CPU oracle alone) and tests/test_wide_horizons_gpu.py (the device).  Mirrors tests/lane16_horizons.py, whose Loop,
edges(), Tune, _box_batch, guards and search it imports.

 - LOOPS: the loops as data.  S = N - 1 stage knots; a loop walks count(N) knots (or rows of a table) in groups of `period`
   and asks for operands `lookahead` knots ahead of the one it works on.
 - box classes: lane16_horizons._box_batch (gen_random_linear_batch, B = 6, steps = 3) with u_bnd = frac * max |Utrack|; the
   per-knot class draws A_k, B_k, d_k over the whole track as test_wide_kernel_shortest_horizons draws them for one window.
 - constrained classes: lane16_matrix.TrackProblem over the same batch without its box: four LINEAR rows mixing states and
   controls, a control box, a state bound on knots 1..N-1 (row-linrows); the same with a cone on (u0, u1) and the box on the
   other controls (generic).
Seeds and fractions were tuned on the ORACLE until the guards hold (seed 5, 6, ... x frac 0.6, 0.4, 0.8, the first hit in that
order); nothing here depends on the device."""
import functools
from dataclasses import dataclass, replace
from types import SimpleNamespace as NS

import numpy as np

import lane16_horizons as lh
import lane16_matrix as lm
import wide_matrix as wm
from altro_mpc_icra2021_amd import problems as P
from helpers import REF_OPTS, make_oracle, mpc_update
from lane16_horizons import ABI_MIN_N, STEPS, Loop, Tune, edges, last_word_knots, sensitivity_ok, stage   # noqa: F401
from lane16_matrix import ULP_BOUND, X0_ULP_BOUND, _flip_to_positive_peak   # noqa: F401
from wide_matrix import at_penalty_cap

B = lh.B           # the batch of _box_batch: every instance is a block of its own on this backend
XSCALE = 0.3       # size of the state coefficients of the mixing rows (wide_matrix.Tune.xscale)
# Options of the constrained classes: the penalty schedule of the generic-rows tests (wide_matrix.ROWS_OPTS: penalty 10, x 10 an
# outer iteration).  With REF_OPTS (1000, x 100) a row that holds a state, or the state bound, is enforced at a penalty of 1e5
# and more within a knot or two of x0, and the oracle's own u_0 -- hence the x0 of the next step -- moves by 1e-10 under one ulp of
# the dynamics: seeds 5..24 x the three fractions leave no case at N = 3..7 that holds X0_ULP_BOUND.
TRACK_OPTS = wm.ROWS_OPTS
TRIP_KNOTS = 16    # sets_differ: 64 lanes x 16 bytes a trip, 64 bytes a knot (solve_wide.h:505 aset_plane)

HORIZONS = [3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 32, 33]
"""3..11: every residue of S and of N mod 4 below, at and above one and two groups of four, a third group, and the rows 7..10 of the
tables shift_column moves in chunks of 8; 16: one full trip of sets_differ (and 15 rows of X: the largest remainder of a chunk);
17: a second trip that holds the terminal knot alone, two chunks of X; 18: one stage knot more, two chunks of U; 32, 33: the same
at two trips."""


# ---------------------------------------------------------------------------------------------------------------------
# the loops
@dataclass(frozen=True)
class WideLoop(Loop):
    line: int = 0              # solve_wide.h line of the loop statement
    lookahead: int = 0         # deepest request ahead of the knot at work (clamped at the end of the horizon)
    text: tuple = ()           # source lines that carry the period and the lookahead: (text, times it occurs in solve_wide.h)
    sweep: bool = False        # a grouped sweep: its edge horizons make SWEEP_HORIZONS
    more_counts: tuple = ()    # further tables the same loop walks (shift_column)
    trips: bool = False        # sets_differ: the edges of a 16-knot trip instead of a remainder


def knots(N):
    return N


LOOPS = [
    # rollout_row<CLOSED, LTV, ROWS>: `for (int k = 0; k < N - 1; ++k)` at :1335; ld(0..2) before the loop (:1333) and ld(k + 3)
    # in it (:1336); k_request(k + 2) (:1337) and dyn_req two knots ahead, parked in kpark[k & 1] / park[k & 1]
    WideLoop("rollout_row", "", 2, stage, line=1335, lookahead=3,
             text=(("const Ld d3 = ld(k + 3);", 1), ("kq1 = k_request(k + 2);", 1), ("const lds_d* st = kpark[k & 1];", 1))),
    # rollout_simple<CLOSED>: one knot ahead, K in kbuf[k & 1]
    WideLoop("rollout_simple", "", 2, stage, line=1112, lookahead=1,
             text=(("const lds_d* st = kbuf[k & 1];", 1), ("k_put(kn, kbuf[(k + 1) & 1]);", 1))),
    # rollout_generic: load_knot(k + 1) at :1888, dyn_request(last ? k : k + 1) at :1889, park[k & 1] at :1917
    WideLoop("rollout_generic", "", 2, stage, line=1886, lookahead=1,
             text=(("if (ahead) dq = dyn_request(last ? k : k + 1);", 1), ("xn = ahead ? next_state_parked(park[k & 1]) : next_state(k);", 1))),
    # grad_pass<ROWS>: groups of four knots forward over ALL N knots, ldq(k + 3); knots k >= N store to the trash line
    WideLoop("grad_pass", "", 4, knots, line=1517, lookahead=3, sweep=True,
             text=(("for (int k = 0; k < N; k += 4) {", 1), ("qs[(U + 3) & 3] = ldq(k + 3);", 1))),
    # adjoint_row<LTV, FULL>: groups of four backward from kt = N - 2, ldq(k - 3), fac_req(k - 2), dyn_req(k - 2); dead knots k < 0
    WideLoop("adjoint_row", "", 4, stage, line=1690, lookahead=3, sweep=True,
             text=(("for (int k = kt; k >= 0; k -= 4) {", 1), ("qs[(U + 3) & 3] = ldq(k - 3);", 1), ("fq[U & 1] = fac_req(k - 2);", 1),
                   ("dq[U & 1] = dyn_req(k - 2);", 1))),
    # adjoint_lds(full): pairs backward, register slots and fpark[U] alternate
    WideLoop("adjoint_lds", "", 2, stage, line=1820, lookahead=1, sweep=True, text=(("for (int k = N - 2; k >= 0; k -= 2) {", 1),)),
    # backward: one knot a trip, operands (and with dyn_ahead the dynamics) of knot k - 1 requested, clamped at 0
    WideLoop("backward", "", 1, stage, line=2347, lookahead=1,
             text=(("const KnotLd kdn = load_knot(k > 0 ? k - 1 : 0, false, 2, Xp(cur), Up(cur));", 1), ("if (ahead) dq = dyn_request(k > 0 ? k - 1 : 0);", 1))),
    # sets_differ: 16 knots a trip of the wave; no remainder code, every lane is bounded by c < N * 4 alone
    WideLoop("sets_differ", "", TRIP_KNOTS, knots, line=511, trips=True, text=(("for (int c = T; c < N * 4; c += 64) {", 1),)),
    # shift_column: chunks of 8 rows, (k0, k1] -> [k0, k1): X moves N - 1 rows; U N - 2, and so do the duals of a box or of rows on
    # knots 0..N-2 and of rows on knots 1..N-1
    WideLoop("shift_column", "", 8, stage, line=2887, sweep=True, more_counts=(lambda N: N - 2,),
             text=(("for (int k = k0; k < k1; k += 8) {", 1), ("v[u] = col[(size_t)(k + 1 + u < k1 ? k + 1 + u : k1) * stride];", 1),
                   ("if (T < n) shift_column(Xp(cur) + T, n, 0, N - 1);", 1), ("if (T < m) shift_column(Up(cur) + T, m, 0, N - 2);", 1))),
]
LOOP = {lp.name: lp for lp in LOOPS}


def counts(loop):
    return (loop.count,) + loop.more_counts


def edge_witnesses(loop, horizons):
    """{edge: the horizons of `horizons` that reach it}, over every table the loop walks.  The four edges of
    lane16_horizons.edges() (largest_remainder: the first above one group), two full groups, a third group, the first horizon whose
    deepest request at the first knot is not clamped (N - 1 > lookahead at the terminal-clamped loads: N = lookahead + 2) with one
    where it is; for a trip loop, instead of a remainder: one full trip, a trip that holds the terminal knot alone, one stage
    knot more, and the same at two trips."""
    p, w = loop.period, {}
    for ci, cnt in enumerate(counts(loop)):
        t = "" if ci == 0 else "_table%d" % ci
        c = {N: cnt(N) for N in horizons}
        w["below" + t] = [N for N in horizons if c[N] < p]
        w["equal" + t] = [N for N in horizons if c[N] == p]
        w["one_above" + t] = [N for N in horizons if c[N] == p + 1]
        if loop.trips:
            w["terminal_alone_in_second_trip"] = w.pop("one_above")
            w["one_stage_knot_in_second_trip"] = [N for N in horizons if c[N] == p + 2]
            w["two_full_trips"] = [N for N in horizons if c[N] == 2 * p]
            w["terminal_alone_in_third_trip"] = [N for N in horizons if c[N] == 2 * p + 1]
            continue
        w["largest_remainder" + t] = [N for N in horizons if c[N] == 2 * p - 1]
        w["two_groups" + t] = [N for N in horizons if c[N] == 2 * p]
        if ci == 0:      # (a further table is the same function called with another k1: its third chunk is the first table's)
            w["third_group"] = [N for N in horizons if c[N] == 2 * p + 1]
    if loop.lookahead > 1:
        w["request_clamped"] = [N for N in horizons if N < loop.lookahead + 2]
        w["request_not_clamped"] = [N for N in horizons if N == loop.lookahead + 2]
    return w


def unreachable(loop, edge):
    """edges no horizon >= ABI_MIN_N reaches (lane16_horizons.edges reports them True): fewer knots than the shortest horizon has,
    at a period of 1 or 2"""
    least, p = counts(loop)[int(edge[-1]) if "_table" in edge else 0](ABI_MIN_N), loop.period
    return (edge.startswith("below") and least >= p) or (edge.startswith("equal") and least > p) or (edge.startswith("largest_remainder") and least > 2 * p - 1)


def wide_edges(loop, horizons):
    """every edge of edge_witnesses as a boolean (tests/test_wide_horizons.py holds the ones lane16_horizons.edges() knows to it)"""
    return {k: bool(v) or unreachable(loop, k) for k, v in edge_witnesses(loop, horizons).items()}


SWEEP_HORIZONS = sorted({N for lp in LOOPS if lp.sweep for ws in edge_witnesses(lp, HORIZONS).values() for N in ws})
"""the horizons at which grad_pass, adjoint_row, adjoint_lds or shift_column has an edge"""
TRIP_HORIZONS = [17, 18, 33]   # sets_differ beyond its first trip: a pair of solves whose sets differ at knots >= 16 only


# ---------------------------------------------------------------------------------------------------------------------
# the classes: one smallest shape per code path
@dataclass(frozen=True)
class Class:
    name: str
    shape: tuple
    kinds: tuple = ()          # constraint blocks of a TrackProblem (() for the box classes)
    ltv: bool = False
    counter: str = ""          # the sweep counter that must advance at SWEEP_HORIZONS ("" where no sweep can run)
    path: tuple = ()           # (rollout, sweeps) the class is there for: held to dispatch() by tests/test_wide_horizons.py

    @property
    def n(self):
        return self.shape[0]

    @property
    def m(self):
        return self.shape[1]

    @property
    def rows(self):
        return sum({"soc": 3, "lin": 4, "xub": 1}.get(k, 0) for k in self.kinds)

    @property
    def cones(self):
        return sum(k == "soc" for k in self.kinds)


CLASSES = [
    Class("row-reuse", (16, 4), counter="reuse", path=("rollout_row<., false, false>", "grad_pass<false> + adjoint_row<false, true>")),
    Class("row-confirm", (12, 7), counter="confirm", path=("rollout_row<., false, false>", "grad_pass<false> + adjoint_row<false, false>")),
    Class("row-ltv", (12, 7), ltv=True, counter="confirm", path=("rollout_row<., true, false>", "grad_pass<false> + adjoint_row<true, false>")),
    Class("row-linrows", (12, 7), kinds=("lin", "box", "xub"), counter="confirm",
          path=("rollout_row<., false, true>", "grad_pass<true> + adjoint_row<false, false>")),
    Class("simple-4", (20, 4), counter="reuse", path=("rollout_simple", "adjoint_lds(true)")),
    Class("simple-8", (24, 7), counter="reuse", path=("rollout_simple", "adjoint_lds(true)")),
    Class("generic", (12, 7), kinds=("soc", "lin", "box", "xub"), path=("rollout_generic", "")),
]
CLASS = {c.name: c for c in CLASSES}
TRIP_CLASSES = ["row-reuse", "simple-4"]


def dispatch(n, m, rows, cones, ltv, strict=False):
    """(rollout, sweeps) of Solver::rollout() and Solver::ilqr() (solve_wide.h) for a problem whose constraint tables are the same at
    every knot (con_static & 1): row_rollouts (:1847), the dispatch of rollout() (:1850), kReuseRow (:574), kReuse and reuse_class
    (:2684), can_sweep and the `tryg` condition (:2716).  sweeps: what an iteration without a backward pass runs, "" where none
    can."""
    mc, sm, _, _ = wm.instantiation(n, m, rows)
    row_rollouts = sm and cones == 0 and rows <= 16
    if sm and row_rollouts:
        rollout = "rollout_row<., %s, %s>" % ("true" if ltv else "false", "true" if rows > 0 else "false")
    elif not sm and rows == 0 and not ltv:
        rollout = "rollout_simple"
    else:
        rollout = "rollout_generic"
    reuse_row = sm and mc == 4
    reuse = (mc > 0 and not sm) or reuse_row
    reuse_class = reuse and not strict and rows == 0 and not ltv and (not sm or row_rollouts)
    can_sweep = mc > 0 and (row_rollouts if sm else (rows == 0 and not ltv))
    if reuse_class:
        sweeps = "grad_pass<false> + adjoint_row<false, true>" if sm else "adjoint_lds(true)"
    elif can_sweep and not strict:
        # (!sm would be adjoint_lds(false): the CPU test holds that no combination gets here -- can_sweep and !strict make
        # reuse_class true when !sm and mc > 0)
        sweeps = "grad_pass<%s> + adjoint_row<%s, false>" % ("true" if rows > 0 else "false", "true" if ltv else "false") if sm else "adjoint_lds(false)"
    else:
        sweeps = ""
    return rollout, sweeps


# ---------------------------------------------------------------------------------------------------------------------
# the tables.  Tune(seed, frac): the first of the search order at which every guard of test_wide_horizons.py holds.
SEEDS, FRACS = range(5, 25), (0.6, 0.4, 0.8)
# (class name, N) -> Tune where it is not Tune().  Box classes: 62 of the 70 cases hold every guard at seed 5, frac 0.6; the eight
# below miss one there (most often: the warm re-solve of a sweep case, which the guards count as a solve of the loop, at the penalty cap) and hold all at seed 5, 0.4.  One-ulp sensitivity, duals included: at most 8.9e-12 ((12, 7) at N = 3); the
# x0 of a step moves by 1.5e-14 at most.  Constrained classes: what made an earlier choice miss is a block whose dual is nonzero
# in fewer than two instances (most often the state bound), a solve at the penalty cap, or a sensitivity above ULP_BOUND;
# at most 7.4e-10 (generic, N = 7), the x0 of a step 4.5e-14 (row-linrows, N = 4).
TUNES = {("row-reuse", 5): Tune(frac=0.4), ("row-confirm", 18): Tune(frac=0.4), ("row-ltv", 4): Tune(frac=0.4), ("row-ltv", 7): Tune(frac=0.4),
         ("simple-4", 3): Tune(frac=0.4), ("simple-4", 11): Tune(frac=0.4), ("simple-4", 16): Tune(frac=0.4), ("simple-4", 18): Tune(frac=0.4),
         ("row-linrows", 4): Tune(frac=0.4), ("row-linrows", 5): Tune(frac=0.4), ("row-linrows", 6): Tune(seed=6, frac=0.4),
         ("row-linrows", 8): Tune(frac=0.4), ("row-linrows", 10): Tune(frac=0.4), ("row-linrows", 32): Tune(frac=0.4), ("row-linrows", 33): Tune(frac=0.4),
         ("generic", 4): Tune(frac=0.4), ("generic", 5): Tune(seed=8), ("generic", 6): Tune(frac=0.4), ("generic", 8): Tune(seed=8, frac=0.4),
         ("generic", 9): Tune(frac=0.4), ("generic", 10): Tune(seed=6, frac=0.4), ("generic", 11): Tune(seed=9, frac=0.4),
         ("generic", 18): Tune(seed=9, frac=0.4), ("generic", 32): Tune(seed=7, frac=0.4), ("generic", 33): Tune(seed=10, frac=0.4)}
LEFT_OUT = {}    # (class name, N) -> reason; box classes: none; row-ltv, row-linrows, generic: at most two horizons each
CASES = [(c.name, N) for c in CLASSES for N in HORIZONS if (c.name, N) not in LEFT_OUT]


def case_id(case):
    return "%s-N%d" % case


def tune_of(case):
    return TUNES.get(case, Tune())


def is_box(cls):
    return not cls.kinds


# ---------------------------------------------------------------------------------------------------------------------
# problems
@functools.lru_cache(maxsize=None)
def _dyn_track(shape, N, seed):
    """per-knot A_k, B_k, d_k for every knot of the track the loop reaches (block (i + 1) + k at step i, knot k), drawn as
    test_wide_kernel_shortest_horizons draws its window"""
    pb = lh._box_batch(shape, N, seed, 0.6)
    rng = np.random.default_rng([seed, N, 50])
    nb = STEPS + N
    A = pb.A[:, None] * (1.0 + 0.1 * rng.standard_normal((nb, 1, 1)))[None]
    Bm = pb.Bm[:, None] * (1.0 + 0.1 * rng.standard_normal((nb, 1, 1)))[None]
    d = 0.05 * rng.standard_normal((B, nb, shape[0]))
    return A, Bm, d


@functools.lru_cache(maxsize=None)
def _track_problem(shape, N, seed, frac, kinds):
    """lane16_matrix.TrackProblem over _box_batch without the generator's box:
      soc  ||(u0, u1)|| <= frac * (peak over Utrack), knots 0..N-2                         (generic only)
      lin  four rows mixing states (0.3 x unit normals) and controls (unit normals) at frac * (peak over the track), knots 0..N-2
      box  on the controls (with the cone: on u2..) at frac * max |Utrack|
      xub  bound on x_{n-1} at frac * (peak over Xtrack), knots 1..N-1: a row range that starts at knot 1"""
    n, m = shape
    nz = n + m
    pb = lh._box_batch(shape, N, seed, 0.6)
    rng = np.random.default_rng([seed, n, m, N, 4])
    cons = []
    lo = 2 if "soc" in kinds else 0
    for kind in kinds:
        if kind == "soc":
            As = np.zeros((3, nz)); As[0, n] = 1.0; As[1, n + 1] = 1.0
            rad = frac * np.linalg.norm(pb.Utrack[:, :, :2], axis=-1).max()
            cons.append(P.ConstraintSpec(P.SOC, P.INEQ, 0, N - 2, A=As, b=np.array([0.0, 0.0, rad])))
        elif kind == "lin":
            Al = np.zeros((4, nz))
            Al[:, :n] = XSCALE * rng.standard_normal((4, n))
            Al[:, n:] = rng.standard_normal((4, m))
            Z = np.concatenate([pb.Xtrack[:, :pb.Utrack.shape[1]], pb.Utrack], axis=-1)
            cons.append(P.ConstraintSpec(P.LINEAR, P.INEQ, 0, N - 2, A=Al, b=-frac * _flip_to_positive_peak(Al, Z @ Al.T)))
        elif kind == "box":
            zmax = np.r_[np.full(n + lo, np.inf), np.full(m - lo, frac * np.abs(pb.Utrack[:, :, lo:]).max())]
            cons.append(P.ConstraintSpec(P.BOX, P.INEQ, 0, N - 2, zmin=-zmax, zmax=zmax))
        elif kind == "xub":
            Ax = np.zeros((1, nz)); Ax[0, n - 1] = 1.0
            cons.append(P.ConstraintSpec(P.LINEAR, P.INEQ, 1, N - 1, A=Ax, b=-frac * _flip_to_positive_peak(Ax, pb.Xtrack[:, :, n - 1:n] * Ax[0, n - 1])))
    return lm.TrackProblem(pb, cons, list(kinds), dict(TRACK_OPTS))


def problem(case, tune=None):
    """NS(cls, N, pb, tp, dyn, resolve): pb the RandomLinearBatch (with its box for the box classes), tp the TrackProblem of a constrained
    class, dyn = (A, Bm, d) over the track for the per-knot class"""
    cls, N = CLASS[case[0]], case[1]
    t = tune or tune_of(case)
    resolve = bool(cls.counter) and N in SWEEP_HORIZONS     # the warm re-solve of the sweep tests belongs to the loop there
    if is_box(cls):
        return NS(cls=cls, N=N, pb=lh._box_batch(cls.shape, N, t.seed, t.frac), tp=None, dyn=_dyn_track(cls.shape, N, t.seed) if cls.ltv else None, resolve=resolve)
    tp = _track_problem(cls.shape, N, t.seed, t.frac, cls.kinds)
    return NS(cls=cls, N=N, pb=tp.pb, tp=tp, dyn=None, resolve=resolve)


def oracles(oracle, pr):
    N = pr.N
    if pr.tp is not None:
        return lh.conic_oracles(oracle, pr.tp)
    orcs = [make_oracle(oracle, pr.pb, b) for b in range(B)]
    for b, o in enumerate(orcs):
        o.con_ids = [0]
        if pr.dyn is not None:
            A, Bm, d = pr.dyn
            o.set_dynamics(A[b, :N - 1], Bm[b, :N - 1], d[b, :N - 1])
    return orcs


def oracle_step(o, pr, b, i):
    """helpers.mpc_update, and for the per-knot class the window of the dynamics track moved on (the plant step runs on the model
    of the step that just ended: test_quadruped_ltv_mpc_runs_device_resident)"""
    x0 = mpc_update(o, pr.pb, b, i)
    if pr.dyn is not None:
        A, Bm, d = pr.dyn
        o.set_dynamics(A[b, i + 1:i + pr.N], Bm[b, i + 1:i + pr.N], d[b, i + 1:i + pr.N])
    return x0


def kinds_of(pr):
    return list(pr.cls.kinds) or ["box"]


def box_bound(pr):
    """(columns of U, bound) of the class's control box"""
    if pr.tp is None:
        return slice(0, pr.cls.m), pr.pb.u_bnd
    c = pr.tp.cons[pr.tp.kinds.index("box")]
    lo = int(np.isinf(c.zmax[pr.cls.n:]).sum())
    return slice(lo, pr.cls.m), float(c.zmax[-1])


def resolve_move(N, shape):
    """the move of x0 before the warm re-solve (test_lane16_horizons_gpu.box_run)"""
    return 0.02 * np.random.default_rng([N, 82]).standard_normal(shape)


def run_loop(oracle, pr, answers=False):
    """The loop on the oracle: initial solve and STEPS steps, and where pr.resolve the warm re-solve after them.  dict(status (1 + STEPS [+ 1], B), capped, on_bound (B, N - 1): controls of
    the LAST solve on the box, nonzero {kind: instances with a nonzero dual after the last solve}); with answers: X, U and every
    dual block after every solve, and the x0 of every step."""
    orcs = oracles(oracle, pr)
    kinds = kinds_of(pr)
    status, capped, out, x0s = [], False, [], []
    for i in range(-1, STEPS + int(pr.resolve)):
        if i >= STEPS:
            x1 = np.array([x[0] for x in x0s[-B:]]) + resolve_move(pr.N, (B, pr.cls.n))
            for b, o in enumerate(orcs):
                o.set_initial_state(x1[b])
        elif i >= 0:
            for b, o in enumerate(orcs):
                x0s.append([oracle_step(o, pr, b, i)])
        sos = [o.solve() for o in orcs]
        status.append([so.status for so in sos])
        capped = capped or any(at_penalty_cap(so) for so in sos)
        if answers:
            out += lm._answers(orcs, kinds)
    cols, ub = box_bound(pr)
    on = np.array([(np.abs(o.controls()[:, cols]) >= ub * (1.0 - 1e-6)).any(axis=-1) for o in orcs])
    nonzero = {kind: sum(bool(np.any(o.duals(o.con_ids[ci]) != 0.0)) for o in orcs) for ci, kind in enumerate(kinds)}
    return dict(status=np.array(status), capped=capped, on_bound=on, nonzero=nonzero, answers=out, x0s=x0s)


def _moved(pr, trial):
    """every element of the dynamics moved by at most one unit in the last place (lane16_horizons._moved)"""
    pb = lh._moved(pr.pb, trial)
    out = NS(**vars(pr))
    out.pb = pb
    if pr.tp is not None:
        out.tp = replace(pr.tp, pb=pb)
    if pr.dyn is not None:
        rng = np.random.default_rng([trial, 7, 1])
        out.dyn = tuple(x * (1.0 + np.finfo(float).eps * rng.choice([-1.0, 0.0, 1.0], x.shape)) for x in pr.dyn)
    return out


def ulp_sensitivity(oracle, pr, trials=6):
    """lane16_horizons.box_ulp_sensitivity for every class: (largest change of X, U or a dual block after any solve of the loop,
    largest change of the x0 of a step) of the oracle against itself with its dynamics moved in the last place"""
    base = run_loop(oracle, pr, answers=True)
    runs = [run_loop(oracle, _moved(pr, t), answers=True) for t in range(trials)]
    return max(lm._largest_change(base["answers"], r["answers"]) for r in runs), max(lm._largest_change(base["x0s"], r["x0s"]) for r in runs)


def guard(oracle, pr):
    """(ok, figures): every guard of a case but the sensitivity -- every solve SOLVE_SUCCEEDED below the penalty cap, two instances
    end with a control on its bound, one of them at a stage knot of the last 16-knot trip that holds one, and in the constrained
    classes every inequality block has a nonzero dual in two instances"""
    g = run_loop(oracle, pr)
    g["instances_on_bound"] = int(g["on_bound"].any(axis=1).sum())
    g["instances_on_bound_in_last_trip"] = int(g["on_bound"][:, list(last_word_knots(pr.N))].any(axis=1).sum())
    ok = bool(np.all(g["status"] == 1)) and not g["capped"] and g["instances_on_bound"] >= 2 and g["instances_on_bound_in_last_trip"] >= 1
    if pr.tp is not None:
        ok = ok and all(v >= 2 for v in g["nonzero"].values())
    return ok, g


def search(oracle, case):
    """the first Tune of the search order that holds every guard"""
    for seed in SEEDS:
        for frac in FRACS:
            t = Tune(seed, frac)
            pr = problem(case, t)
            if guard(oracle, pr)[0] and sensitivity_ok(ulp_sensitivity(oracle, pr)):
                return t
    return None


# ---------------------------------------------------------------------------------------------------------------------
# sets_differ beyond the first trip (test d).  The planes sets_differ compares hold the solver's codes (active_codes) of the
# trajectory at hand and of the trajectory the last backward pass expanded.  A pair of solves whose SOLUTIONS differ late says
# little about them: 1200 moves of x0 after the loop (400 streams x 0.02, 0.005, 0.002 standard normal) give no pair whose sets
# differ at knots >= 16 only by a side that enters -- feedback absorbs a move of x0 within a few knots -- and a side that leaves keeps
# its multiplier and stays in the set.  So the pair is made at the START of the second solve: after the loop one control at a knot
# >= 16, inactive in the solution, is put 5 % beyond its bound (set_initial_trajectory does not drop the stored gains), and a twin
# solves again with nothing changed.  Where the twin ran that solve on the stored gains throughout, the stored pass was usable
# and its set is the solution's: the changed start differs from it at that one late knot, and the FIRST iteration must be a
# backward pass.  Held where both solves take one outer iteration: a pass after a penalty change runs whatever sets_differ says.
# N = 17: the second trip holds the terminal knot alone, which carries no control -- under a box on the controls its 64 bytes are
# zero in every plane, and no start can differ there.  That edge is reached by parity at N = 17 alone: open.
TRIP_BEYOND = 1.05
TRIP_LEFT_OUT = {(c, 17): "the terminal knot, alone in the second trip, carries no control: its bytes are zero under a control box" for c in TRIP_CLASSES}
TRIP_CASES = [(c, N) for c in TRIP_CLASSES for N in TRIP_HORIZONS if (c, N) not in TRIP_LEFT_OUT]


def active_codes(orcs, pr):
    """(B, N - 1, m) the sides of the control box the SOLVER counts as active (solve_wide.h box_code: value at or beyond the bound, or
    a positive multiplier), bit 0 upper, bit 1 lower, at the oracles' controls and multipliers"""
    cols, ub = box_bound(pr)
    n, nz = pr.cls.n, pr.cls.n + pr.cls.m
    U = np.array([o.controls()[:, cols] for o in orcs])
    lam = np.array([o.duals(o.con_ids[kinds_of(pr).index("box")]).reshape(pr.N - 1, 2, nz)[:, :, n:][:, :, cols] for o in orcs])
    return np.where((U >= ub) | (lam[:, :, 0] > 0.0), 1, 0) + np.where((U <= -ub) | (lam[:, :, 1] > 0.0), 2, 0)


def _after_loop(oracle, pr):
    orcs = oracles(oracle, pr)
    for i in range(-1, STEPS):
        if i >= 0:
            for b, o in enumerate(orcs):
                oracle_step(o, pr, b, i)
        for o in orcs:
            o.solve()
    return orcs


def trip_start(oracle, case):
    """NS(pr, pick (B, 3): knot, control and value of the entry of U that changes -- per instance the inactive control at a knot >= 16
    that is closest to its bound, put TRIP_BEYOND x the bound --, same / moved: oracles and their statistics after the second solve
    with nothing changed / from the changed start, one_outer (B,): both second solves took one outer iteration,
    ok: every second solve succeeded below the cap and one_outer holds somewhere)"""
    pr = problem(case)
    same, moved = _after_loop(oracle, pr), _after_loop(oracle, pr)
    codes = active_codes(moved, pr)
    _, ub = box_bound(pr)
    pick = np.zeros((B, 3))
    for b, o in enumerate(moved):
        U = o.controls().copy()
        room = np.where(codes[b, TRIP_KNOTS:] == 0, np.abs(U[TRIP_KNOTS:]), -1.0)
        k, j = np.unravel_index(np.argmax(room), room.shape)
        assert room[k, j] >= 0.0
        pick[b] = k + TRIP_KNOTS, j, np.copysign(TRIP_BEYOND * ub, U[k + TRIP_KNOTS, j])
        U[int(pick[b, 0]), j] = pick[b, 2]
        o.set_controls(U)
    so_same, so_moved = [o.solve() for o in same], [o.solve() for o in moved]
    one = np.array([a.iterations_outer == 1 and c.iterations_outer == 1 for a, c in zip(so_same, so_moved)])
    ok = bool(one.any()) and all(so.status == 1 and not at_penalty_cap(so) for so in so_same + so_moved)
    return NS(pr=pr, pick=pick, same=same, so_same=so_same, moved=moved, so_moved=so_moved, one_outer=one, ok=ok)
