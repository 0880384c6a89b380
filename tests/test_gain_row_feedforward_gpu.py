"""Feedforward terms in the free control lanes of the gain rows (solve_dpp16.h kd_drow / kd_dcol, Solver::d_ofs).

The box-only 16-lane kernels keep d[a] of a knot on control lanes of the knot's gain rows that the factors of Quu leave
free: the backward passes write it with the rows they store, the first-order sweep overwrites only those lanes (one store
per knot, every other lane to the trash block), the closed-loop rollouts and the accessor read it from there.  What can go
wrong is a store that clobbers a neighbouring lane (K or a factor), a reader that looks in the wrong lane, and the lone
rollout, which loads d for four knots at once.

Random-linear (12, 4) and (6, 3) -- the shortest built shape, NZ = 9 -- at N = 50, two waves, six fused MPC steps; with
u_bnd = 3 and seed 44 the tracked controls of some instances of each wave leave the box and those of others never come near
it, so backward passes and first-order sweeps both occur in one wave.  Each configuration runs once and is shared."""
import os

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from helpers import make_oracle, mpc_update
from test_gpu_parity import RTOL, check_against_oracle, rel_err   # the headline parity test's constants

pytestmark = pytest.mark.gpu

B, S, N, SEED = 8, 6, 50, 44
SHAPES = [(12, 4), (6, 3)]
_runs = {}


def problem(n, m):
    return altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=SEED)


def run(n, m, switch=None):
    """the fused S-step run under one ALTRO_* switch (read when the solver is created); results as host arrays"""
    key = (n, m, switch)
    if key not in _runs:
        old = os.environ.get(switch) if switch else None
        if switch:
            os.environ[switch] = "1"
        try:
            mp = altro.mpc.BatchMPC(problem(n, m))
            mp.initial_solve()
            altro.timing_reset(mp.solver)
            mp.run_async(S, first=0)
            mp.synchronize()
            st = altro.stats(mp.solver)
            K, d = altro.gains(mp.solver)
            _runs[key] = dict(X=altro.states(mp.solver), U=altro.controls(mp.solver), lam=altro.get_duals(mp.solver), x0=mp.x0(),
                              K=K, d=d, F=altro.gain_factors(mp.solver), lone=int(altro.wave_cycles(mp.solver)[:, 7].sum()),
                              alpha=altro.alpha_trace(mp.solver), st=st, reuse=altro.reuse_counter(mp.solver),
                              passes=altro.work_counters(mp.solver)[0], iters=altro.solve_counters(mp.solver)[1])
        finally:
            if switch:
                if old is None:
                    del os.environ[switch]
                else:
                    os.environ[switch] = old
    return _runs[key]


@pytest.mark.parametrize("n,m", SHAPES)
def test_first_order_sweep_changes_only_the_feedforward_lanes(n, m):
    """After a run in which first-order sweeps wrote d into the gain rows, K and the factors of Quu = L D L' read back from
    those rows (gains, gain_factors: the control lanes b <= a, the neighbours of the slots d is written to) are those of a
    run without gain reuse, where every iteration's backward pass recomputes them: bit for bit (inside a fixed active set
    neither depends on the trajectory).  d itself comes from other arithmetic there (the pass instead of the sweep): equal
    to the parity tolerance."""
    a, b = run(n, m), run(n, m, "ALTRO_NO_REUSE")
    pb = problem(n, m)
    hit = np.abs(a["U"]).max(axis=(1, 2)) >= pb.u_bnd * (1 - 1e-6)
    print("(%d, %d): sweeps %s, passes %s, instances at a bound %s" % (n, m, a["reuse"], a["passes"], hit))
    assert hit.any() and not hit.all(), "the case needs instances with and without an active control bound"
    assert int(a["reuse"].sum()) > 0 and int(a["passes"].sum()) > 0 and int(b["reuse"].sum()) == 0
    assert np.array_equal(a["st"].status, b["st"].status) and np.array_equal(a["iters"], b["iters"])
    assert np.array_equal(a["K"], b["K"])
    low = np.tril(np.ones((m, m), dtype=bool))
    assert np.all(a["F"][..., np.arange(m), np.arange(m)] > 0.0)          # 1 / D: the lanes hold factors, not zeros
    assert np.array_equal(a["F"][..., low], b["F"][..., low])
    assert np.abs(a["d"] - b["d"]).max() <= RTOL * max(1.0, np.abs(b["d"]).max())


@pytest.mark.parametrize("n,m", SHAPES)
def test_lone_phases_leave_and_read_the_same_gain_rows(n, m):
    """ALTRO_NO_LONE keeps the four-row forms of every phase (the lone backward pass, which stores the gain rows through
    store_gains, and the lone rollouts, which read d from them): states, controls, duals, gains, factors, d, statistics,
    iteration counts and the accepted steps are the same bit for bit.  The one lone phase the kernel counts is the backward
    pass (wave_cycles column 7; built for n = 12 only, as in test_lone_row_backward_pass_is_bit_identical_to_the_four_row_pass):
    it must have run.  Lone rollouts have no counter."""
    a, b = run(n, m), run(n, m, "ALTRO_NO_LONE")
    print("(%d, %d): lone backward passes %d / %d" % (n, m, a["lone"], b["lone"]))
    assert b["lone"] == 0 and (a["lone"] > 0 or n < 12)
    assert np.array_equal(a["F"], b["F"])
    for k in ("X", "U", "lam", "x0", "K", "d", "alpha", "reuse", "passes", "iters"):
        assert np.array_equal(a[k], b[k]), k
    sa, sb = a["st"], b["st"]
    for k in ("iterations", "iterations_outer", "status", "cost", "c_max", "cost_trace", "cmax_trace"):
        assert np.array_equal(getattr(sa, k), getattr(sb, k)), k


@pytest.mark.parametrize("n,m", SHAPES)
def test_run_and_gains_match_the_oracle(oracle, n, m):
    """The same run against the CPU oracle stepped through the reference's MPC update order: last solve, gains and
    feedforward terms within the tolerance of test_gpu_parity.test_mpc_loop_matches_oracle (RTOL)."""
    a = run(n, m)
    pb = problem(n, m)
    for b in range(B):
        o = make_oracle(oracle, pb, b)
        so = o.solve()
        for i in range(S):
            mpc_update(o, pb, b, i)
            so = o.solve()
        check_against_oracle(a["st"], a["X"], a["U"], b, o, so)
        Ko, do = o.gains()
        assert rel_err(a["K"][b], Ko) <= RTOL
        assert np.abs(a["d"][b] - do).max() <= RTOL * max(1.0, np.abs(do).max())
