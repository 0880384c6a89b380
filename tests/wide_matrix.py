"""The one-wave-per-instance backend as a table: one problem per instantiation of wide_kernel<MC, SM, NPC, PRC> (solve_wide.h
ALTRO_WIDE_KERNELS), with constraints that are active.  Shared by tests/test_wide_matrix.py (dispatch coverage, and the
conditions on the INPUTS, checked on the CPU oracle alone) and tests/test_wide_matrix_gpu.py (the device against the oracle).

 - instantiation() restates wide_kernel_for, lds_bytes() restates lds_layout + wide_compact + the default block-size rule.
 - CASES / BOX_CASES: the table.  B = 3 instances, N = 12 knots (8 where n = 64: the oracle's time goes with n^3).
 - rows_problem(): the recipe of test_wide_kernel_generic_rows_on_large_states with every constraint SCALED FROM THE
   UNCONSTRAINED SOLUTION of the same instances, so that each kind of row binds whatever the size:
     block 0  LINEAR INEQ, 4 rows mixing states and controls, knots 0..N-2, b = -frac * (peak of the row over Z_free)
     block 1  LINEAR EQ, `neq` rows on x at the terminal knot
     block 2  SOC on (u_0, u_1), radius frac * max |(u_0, u_1)_free|
     block 3  BOX on u_2..u_{m-1} at +- frac * max |u_free|
     block 4  LINEAR INEQ, 1 row: upper bound on x_{n-1} (the row next to the state padding), knots 1..N-1 (`xub`)
     block 5  the rows that take the count to 16 (bound at 0.9 of their peak) or to 64 (slack: bound at ten peaks)
   4 + 2 + 3 + 1 = 10 rows: not a multiple of 4, so pad4 of the row count matters.
 - box_problem(): gen_random_linear_batch with u_bnd tightened until controls saturate at every MPC step.
 - guards: what the inputs must satisfy for a comparison on them to mean anything (rows_guard, box_guard).
Seeds, fractions and bounds below were tuned on the ORACLE until the guards hold; nothing here depends on the device."""
import functools
from dataclasses import dataclass, field, replace

import numpy as np

from altro_mpc_icra2021_amd import problems as P
from helpers import REF_OPTS, make_oracle, mpc_update, rocket_oracle

B = 3
DT = 0.1
ROWS_OPTS = dict(REF_OPTS, penalty_initial=10.0, penalty_scaling=10.0, iterations_outer=40)   # (the generic-rows test's)
PENALTY_MAX = 1e8          # altro_default_opts / orc_default_opts
LDS_LIMIT = 160 * 1024     # wide_backend.h prepare_launch
MAX_ROWS = 64              # solve_wide.h kMaxP


# ---------------------------------------------------------------------------------------------------------------------
# mirror of the dispatch and of the LDS carve-up
def _pad16(v):
    return (v + 15) & ~15


def _pad4(v):
    return (v + 3) & ~3


def instantiation(n, m, nrows):
    """(MC, SM, NPC, PRC) of the kernel wide_kernel_for(n, m, nrows) returns (solve_wide.h)."""
    sm = n <= 16 and m <= 16
    plain = nrows == 0
    np_ = _pad16(n)
    mc = 4 if m <= 4 else 8 if m <= 8 else 12 if m <= 12 else 16 if m <= 16 else 0
    if mc == 4:
        if sm:
            return (4, True, 0, 0 if plain else -1)
        return (4, False, np_, 0 if plain else -1)
    if mc == 0:
        return (0, False, 0, -1)
    if sm:
        return (mc, True, 0, 16 if (mc == 12 and nrows == 16) else -1)
    return (mc, False, 32 if np_ == 32 else 0, -1)


def lds_doubles(n, m, nrows, compact):
    """lds_layout(n, m, Pn, compact).total (solve_wide.h)."""
    np_, mp, pp = _pad16(n), _pad16(m), _pad4(nrows)
    nzp = np_ + mp
    ldg, lds, ldh, ldu = nzp + 1, np_ + 1, np_ + 17, mp + 1
    o = np_ * ldg + np_ * lds + np_ * ldg     # G, S, W
    if not compact:
        o += 2 * mp * ldh                     # Hux, Kl (compact: inside W)
    o += mp * ldu                             # Huu
    o += 2 * pp * ldg                         # Ac, DA
    o += 6 * nzp + 2 * np_ + 8 * (pp + 4)     # vec
    o += 32                                   # cmd
    return o


def lds_bytes(n, m, nrows, ltv=False, compact_np_max=48):
    """WideBackend::lds_bytes() with the default switches: the compact carve-up where wide_compact allows it AND the block is
    one wave (at most 80 KB with the compact layout: wide_block_threads)."""
    np_, mp = _pad16(n), _pad16(m)
    compact = (not (n <= 16 and m <= 16)) and not ltv and mp == 16 and 32 <= np_ <= min(compact_np_max, 48)
    if compact and 8 * lds_doubles(n, m, nrows, True) > 80 * 1024:
        compact = False
    return 8 * lds_doubles(n, m, nrows, compact)


# ---------------------------------------------------------------------------------------------------------------------
# the table
@dataclass(frozen=True)
class Tune:
    seed: int = 0
    frac: float = 0.75
    neq: int = 2        # rows of the terminal equality
    xub: bool = True    # the bound on the last state component
    xscale: float = 0.3  # size of the state coefficients of the mixing rows (the control coefficients are unit normals)


@dataclass(frozen=True)
class Case:
    n: int
    m: int
    rows: int                 # 10: the recipe as it stands (10 - (2 - neq) - (not xub) rows); any other: filled up to exactly that
    ti: Tune = Tune()         # time-invariant variant
    ltv: Tune = Tune()        # per-knot variant

    @property
    def N(self):
        return 8 if self.n == 64 else 12

    @property
    def id(self):
        return "%dx%d-r%d" % (self.n, self.m, self.rows)

    def tune(self, ltv):
        return self.ltv if ltv else self.ti

    def nrows(self, ltv=False):
        t = self.tune(ltv)
        base = 4 + t.neq + 3 + (1 if t.xub else 0)
        return base if self.rows == 10 else self.rows

    def inst(self, ltv=False):
        return instantiation(self.n, self.m, self.nrows(ltv))


# Tuning, all of it on the oracle (tests/test_wide_matrix.py holds the result): the first of seed 0, 1, ... x frac 0.75, 0.8, 0.7
# at which every guard holds.  What made a default miss: one instance infeasible (status 3 at the 40th outer iteration, or the
# cost limit) where the terminal equality meets tight controls; a box or a cone that stays slack; no cold solve of three outer
# iterations.  Two departures from the plain recipe:
#  - xscale 0.1 at m = 4 with n >= 48 and at 64 rows: with the generic-rows test's 0.3 the state part of a mixing row outweighs
#    its four control coefficients, the row peaks at knot 0 -- where x is given -- and no seed is feasible for all three
#    instances (seeds 0..39 tried at (64, 4), 0..7 at the others);
#  - no bound on the last state in (40, 6) per-knot and (16, 4) time-invariant (9 rows: pad4 still pads): with it, seeds 0..7
#    leave an instance infeasible.
CASES = [
    Case(12, 7, 10, ltv=Tune(seed=1)),                                   # <8, true>
    Case(14, 11, 10, ti=Tune(frac=0.7)),                                 # <12, true>
    Case(14, 11, 16, ti=Tune(seed=2)),                                   # <12, true, 0, 16>: one cone + 13 linear rows (not the quadruped's sixteen)
    Case(9, 14, 10),                                                     # <16, true>
    Case(24, 7, 10, ti=Tune(seed=1, frac=0.8), ltv=Tune(seed=1, frac=0.8)),   # <8, false, 32>
    Case(40, 6, 10, ti=Tune(seed=3), ltv=Tune(seed=5, frac=0.8, xub=False)),  # <8, false>
    Case(30, 10, 10, ti=Tune(frac=0.8)),                                 # <12, false, 32>
    Case(50, 11, 10, ti=Tune(seed=2, frac=0.8), ltv=Tune(seed=2, frac=0.8)),  # <12, false>
    Case(17, 16, 10, ti=Tune(seed=12), ltv=Tune(seed=1)),                # <16, false, 32>
    Case(48, 13, 10),                                                    # <16, false>
    Case(64, 4, 10, ti=Tune(frac=0.8, xscale=0.1), ltv=Tune(seed=8, frac=0.8, xscale=0.1)),   # <4, false, 64>
    Case(33, 17, 10),                                                    # <0, false>
    Case(30, 25, 10, ti=Tune(seed=2)),                                   # <0, false>
    Case(48, 32, 10),                                                    # <0, false>: the largest m > 16 shape that fits the LDS
    # <0, false> at np = 16 < mp = 32: the gains tests/stored_policy_matrix.py reads at that shape class (its LDS carve-up of the
    # covariance is sized by mp there)
    Case(12, 20, 10, ti=Tune(frac=0.7)),
    Case(24, 7, 64, ti=Tune(xscale=0.1)),                                # <8, false, 32> at kMaxP rows
    # the m <= 4 kernels that take rows: reached before by the rocket / grasp / satellite tests and the generic-rows test,
    # here so that every entry of ALTRO_WIDE_KERNELS has its line in one table
    Case(16, 4, 10, ti=Tune(seed=4, xub=False), ltv=Tune(seed=7)),       # <4, true>
    Case(20, 4, 10, ti=Tune(seed=6, frac=0.8), ltv=Tune(seed=2, frac=0.8)),   # <4, false, 32>
    Case(48, 4, 10, ti=Tune(seed=2, frac=0.8, xscale=0.1), ltv=Tune(seed=1, xscale=0.1)),     # <4, false, 48>
]
CASE_BY_ID = {c.id: c for c in CASES}

# the two sides of the 160 KB limit at the largest padded state: (64, 16) holds 12 rows (160 832 B) and not 13; m = 17 pads
# to 32 and does not fit even without rows
LDS_FITS = Case(64, 16, 12, ti=Tune(frac=0.8))
LDS_OVER = Case(64, 16, 13, ti=Tune(frac=0.8))
LDS_OVER_BOX = (64, 17)


@dataclass(frozen=True)
class BoxCase:
    n: int
    m: int
    u_bnd: float = 1.0
    seed: int = 21

    @property
    def N(self):
        return 8 if self.n == 64 else 12

    @property
    def id(self):
        return "%dx%d" % (self.n, self.m)

    def inst(self):
        return instantiation(self.n, self.m, 0)


# every (n, m) of the table once, box only.  u_bnd = 1 (the polish tests' value) unless the cold solves then end in two outer
# iterations ((12, 7), (14, 11): 0.8) or a step runs to the penalty cap ((9, 14): seed 24; both m >= 14 shapes: 0.5).  (12, 20):
# of seeds 21..26 x u_bnd 1, 0.8, 0.5, 1.5, 2 only seed 22 at 0.5 holds every guard (the others: a step at the cap, or cold solves
# of two outer iterations)
BOX_TUNE = {(12, 7): dict(u_bnd=0.8), (14, 11): dict(u_bnd=0.8), (9, 14): dict(u_bnd=0.5, seed=24), (17, 16): dict(u_bnd=0.5),
            (12, 20): dict(u_bnd=0.5, seed=22)}
BOX_CASES = [BoxCase(n, m, **BOX_TUNE.get((n, m), {})) for n, m in dict.fromkeys((c.n, c.m) for c in CASES)]
BOX_BY_ID = {c.id: c for c in BOX_CASES}
BOX_STEPS = 3


# ---------------------------------------------------------------------------------------------------------------------
# problems
@dataclass
class RowsProblem:
    case: Case
    ltv: bool
    rp: object                 # P.RocketProblemData (A, Bm, f: per knot when ltv)
    x0: np.ndarray             # (B, n)
    x0_warm: np.ndarray        # x0 moved by 2 % (time-invariant variant: the warm solve)
    opts: dict
    kinds: list = field(default_factory=list)    # name of every constraint block, in order
    cons_b: list = None        # [instance][block]: constraint data of each instance's own (tests/lane16_matrix.py); None: rp.constraints


def _flip_to_positive_peak(A, vals):
    """vals (..., p): values of the rows over Z_free.  Flip the rows whose largest |value| is negative; returns the peaks."""
    hi, lo = vals.reshape(-1, vals.shape[-1]).max(axis=0), vals.reshape(-1, vals.shape[-1]).min(axis=0)
    flip = -lo > hi
    A[flip] *= -1.0
    return np.where(flip, -lo, hi)


def _free_solution(oracle, rp, x0, opts):
    Xf, Uf = [], []
    for b in range(x0.shape[0]):
        o = rocket_oracle(oracle, rp, x0[b], opts, constraints=[])
        so = o.solve()
        assert so.status == 1
        Xf.append(o.states()); Uf.append(o.controls())
    return np.array(Xf), np.array(Uf)


@functools.lru_cache(maxsize=None)
def _rows_problem(case, ltv, nb):
    import oracle_py as oracle
    oracle.build()
    t = case.tune(ltv)
    n, m, N = case.n, case.m, case.N
    nz = n + m
    pbr = P.gen_random_linear_batch(1, n=n, m=m, N=N, steps=1, seed=61)
    rng = np.random.default_rng([t.seed, n, m, case.rows, int(ltv)])
    A, Bm, f = pbr.A[0], pbr.Bm[0], np.zeros(n)
    if ltv:   # per-knot A_k, B_k and affine d_k, as test_wide_kernel_shortest_horizons draws them
        A = A[None] * (1.0 + 0.1 * rng.standard_normal((N - 1, 1, 1)))
        Bm = Bm[None] * (1.0 + 0.1 * rng.standard_normal((N - 1, 1, 1)))
        f = 0.05 * rng.standard_normal((N - 1, n))
    x0 = rng.standard_normal((nb, n))
    x0_warm = x0 + 0.02 * np.abs(x0).max() * rng.standard_normal((nb, n))
    rp = P.RocketProblemData(n=n, m=m, N=N, dt=DT, A=A, Bm=Bm, f=f, Q=np.full(n, 10.0), R=np.full(m, 0.1), Qf=np.full(n, 10.0),
                             xf=np.zeros(n), x0=np.zeros(n), U0=np.zeros((N - 1, m)), constraints=[])
    Xf, Uf = _free_solution(oracle, rp, x0, ROWS_OPTS)
    Zf = np.concatenate([Xf[:, :N - 1], Uf], axis=-1)          # (B, N-1, nz): knots 0..N-2
    cons, kinds = [], []

    def mixing_rows(p, frac):
        Al = np.zeros((p, nz))
        Al[:, :n] = t.xscale * rng.standard_normal((p, n))
        Al[:, n:] = rng.standard_normal((p, m))
        peak = _flip_to_positive_peak(Al, Zf @ Al.T)
        return P.ConstraintSpec(P.LINEAR, P.INEQ, 0, N - 2, A=Al, b=-frac * peak)     # A z <= frac * peak

    cons.append(mixing_rows(4, t.frac)); kinds.append("lin")
    Ae = np.zeros((t.neq, nz)); Ae[:, :n] = rng.standard_normal((t.neq, n))
    cons.append(P.ConstraintSpec(P.LINEAR, P.EQ, N - 1, N - 1, A=Ae, b=np.zeros(t.neq))); kinds.append("eq")
    As = np.zeros((3, nz)); As[0, n] = 1.0; As[1, n + 1] = 1.0
    rad = t.frac * np.linalg.norm(Uf[:, :, :2], axis=-1).max()
    cons.append(P.ConstraintSpec(P.SOC, P.INEQ, 0, N - 2, A=As, b=np.array([0.0, 0.0, rad]))); kinds.append("soc")   # |u_0, u_1| <= rad
    ub = t.frac * np.abs(Uf[:, :, 2:]).max()
    zmax = np.r_[np.full(n + 2, np.inf), np.full(m - 2, ub)]
    cons.append(P.ConstraintSpec(P.BOX, P.INEQ, 0, N - 2, zmin=-zmax, zmax=zmax)); kinds.append("box")
    if t.xub:
        Ax = np.zeros((1, nz)); Ax[0, n - 1] = 1.0
        peak = _flip_to_positive_peak(Ax, Xf[:, 1:, n - 1:n] * Ax[0, n - 1])
        cons.append(P.ConstraintSpec(P.LINEAR, P.INEQ, 1, N - 1, A=Ax, b=-t.frac * peak)); kinds.append("xub")
    have = sum(c.A.shape[0] for c in cons if c.A is not None)
    if case.rows != 10:
        cons.append(mixing_rows(case.rows - have, 0.9 if case.rows == 16 else 10.0)); kinds.append("fill")
        have = case.rows
    assert have == case.nrows(ltv)
    rp.constraints = cons
    return RowsProblem(case, ltv, rp, x0, x0_warm, dict(ROWS_OPTS), kinds)


def rows_problem(case, ltv=False, nb=B):
    """nb: instances (the table of this file: B)."""
    return _rows_problem(case, bool(ltv), nb)


def rows_oracles(oracle, pr):
    return [rocket_oracle(oracle, pr.rp, pr.x0[b], pr.opts, constraints=pr.cons_b[b] if pr.cons_b else None) for b in range(len(pr.x0))]


def rows_gpu_problem(altro, pr):
    """The same problem for the library: altro.mpc.constrained_problem, with the per-knot model put in where there is one."""
    rp = pr.rp
    if not pr.ltv:
        return altro.mpc.constrained_problem(rp, pr.x0.copy())
    ti = replace(rp, A=rp.A[0], Bm=rp.Bm[0], f=rp.f[0])
    prob = altro.mpc.constrained_problem(ti, pr.x0.copy())
    prob.model = altro.LinearModel(rp.A, rp.Bm, rp.f, dt=rp.dt, per_knot=True)
    return prob


def box_problem(bc):
    pb = P.gen_random_linear_batch(B, n=bc.n, m=bc.m, N=bc.N, steps=BOX_STEPS, seed=bc.seed)
    pb.u_bnd = bc.u_bnd        # the track was drawn with |u| <= 3: the reference's own bound never binds
    return pb


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the inputs
def at_penalty_cap(so):
    """The solve reached penalty_max: its inner iteration counts may differ by one or two between two correct implementations
    (test_option_fuzz_matches_oracle), so it is no parity case."""
    return max(so.penalty_max_outer[:min(so.iterations_outer, 64)]) >= PENALTY_MAX


def rows_guard(oracle, pr):
    """Solve on the oracle (cold; warm too for the time-invariant variant) and return what the guards look at:
    dict(status (nsolves, B), outer (nsolves, B), capped, nonzero {kind: instances with a nonzero dual after the cold solve},
    nonzero_rows {kind: the same count for every row of an affine block})."""
    orcs = rows_oracles(oracle, pr)
    status, outer, capped, nonzero, nonzero_rows = [], [], False, {}, {}
    for rep in range(1 if pr.ltv else 2):
        if rep:
            for b, o in enumerate(orcs):
                o.set_initial_state(pr.x0_warm[b])
        sos = [o.solve() for o in orcs]
        status.append([so.status for so in sos]); outer.append([so.iterations_outer for so in sos])
        capped = capped or any(at_penalty_cap(so) for so in sos)
        if rep == 0:
            for ci, kind in enumerate(pr.kinds):
                nonzero[kind] = sum(bool(np.any(o.duals(o.con_ids[ci]) != 0.0)) for o in orcs)
                c = (pr.cons_b[0] if pr.cons_b else pr.rp.constraints)[ci]
                if c.A is not None:
                    p = c.A.shape[-2]
                    nonzero_rows[kind] = sum(np.any(o.duals(o.con_ids[ci]).reshape(-1, p) != 0.0, axis=0).astype(int) for o in orcs).tolist()
    return dict(status=np.array(status), outer=np.array(outer), capped=capped, nonzero=nonzero, nonzero_rows=nonzero_rows)


def box_guard(oracle, bc):
    """The box-only MPC loop on the oracle: dict(status, outer (1 + steps, B), capped, box (1 + steps,): instances with a
    nonzero box dual after every solve)."""
    pb = box_problem(bc)
    orcs = [make_oracle(oracle, pb, b) for b in range(B)]
    status, outer, box, capped = [], [], [], False
    for i in range(-1, BOX_STEPS):
        if i >= 0:
            for b, o in enumerate(orcs):
                mpc_update(o, pb, b, i)
        sos = [o.solve() for o in orcs]
        status.append([so.status for so in sos]); outer.append([so.iterations_outer for so in sos])
        capped = capped or any(at_penalty_cap(so) for so in sos)
        box.append(sum(bool(np.any(o.duals(0) != 0.0)) for o in orcs))
    return dict(status=np.array(status), outer=np.array(outer), capped=capped, box=np.array(box))
