"""Clone rows and the wave-uniform variants of the knot loops (solve_dpp16.h: clone_flag, uniform_phase, rollout<.., UNI>,
fosweep<UNI>).  A row that sits a phase out runs it as an exact clone of a row that takes part -- same loads, same
arithmetic, same stores to the same addresses -- and where every row of the wave is a participant or a clone and the
participants agree on `shift`, the phase runs a variant whose knot index lives on the scalar unit.  Neither changes a value:
every case runs the default, `no_shadow` (rows keep their own instance and flags; no clone, no uniform variant) and
`no_lone` (a phase only one row needs runs in the four-row form too, with three clones) and compares every output bit
for bit.  Every comparison first asserts, from the form counters in altro_batch_get_wave_passes, that the default run
took the uniform variants and the `no_shadow` run did not: an equality with no uniform phase proves nothing.

All shapes are n = 12, m = 4 random-linear MPC, the smallest horizons at which these loops take every path: N = 5 has
fewer stage knots (4) than one prefetch group of either rollout, so only the remainder code runs; N = 10 is one group of
eight plus one remainder knot in the open-loop rollout; N = 13 has groups with a clamped prefetch tail in both rollouts.
Batch 6 is two waves, the second padded."""
import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import problems as P
from altro_mpc_icra2021_amd.mpc import REF_OPTS
from helpers import make_oracle, mpc_update
from test_gpu_parity import check_against_oracle

pytestmark = pytest.mark.gpu

n, m = 12, 4
SWITCHES = (None, "no_shadow", "no_lone")
_runs = {}
_problems = {}


def problem(N, B, S, seed, u_bnd, spread):
    key = (N, B, S, seed, u_bnd, spread)
    if key not in _problems:
        pb = P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=seed, u_bnd=u_bnd)
        if spread:   # rows of a wave start at different distances from their track: they need different numbers of iterations
            for b in range(B):
                pb.Xtrack[b, 0] *= 1.0 + 0.75 * (b % 4)
        _problems[key] = pb
    return _problems[key]


def forms(sv):
    """(waves, 3, 2): open-loop rollouts, closed-loop rollouts, first-order sweeps of the last launch that ran in the
    four-row form -- [.., 0] as the wave-uniform variant, [.., 1] in the generic form"""
    w = altro.wave_passes(sv)[:, 1:4]
    return np.stack([w & 0xFFFF, w >> 16], axis=-1)


def snapshot(mp, log):
    sv = mp.solver
    st = altro.stats(sv)
    K, d = altro.gains(sv)
    out = dict(X=altro.states(sv), U=altro.controls(sv), lam=altro.get_duals(sv), x0=mp.x0(), K=K, d=d, F=altro.gain_factors(sv),
               alpha=altro.alpha_trace(sv), reuse=altro.reuse_counter(sv), confirm=altro.confirm_counter(sv))
    for k in ("iterations", "iterations_outer", "status", "cost", "c_max", "cost_trace", "cmax_trace"):
        out[k] = np.asarray(getattr(st, k)).copy()
    for i, a in enumerate(altro.work_counters(sv)):     # backward passes, rollouts, trials
        out["work%d" % i] = a
    for i, a in enumerate(altro.solve_counters(sv)):    # solves, iterations, successes
        out["solves%d" % i] = a
    if log:
        for k, v in vars(mp.log()).items():
            if isinstance(v, np.ndarray):
                out["log_" + k] = v.copy()
    return out


def run(monkeypatch, switch, N=10, B=6, S=4, seed=5, u_bnd=3.0, spread=False, active=None, separate=False, log=False, **opts):
    """the closed loop of S steps (one fused launch, or S single-step launches) under one scheduling switch;
    returns (outputs, form counters summed over the launches)"""
    key = (switch, N, B, S, seed, u_bnd, spread, None if active is None else tuple(active), separate, log, tuple(sorted(opts.items())))
    if key in _runs:
        return _runs[key]
    with monkeypatch.context() as mk:
        mk.setenv("ALTRO_NO_GROUP", "1")   # wave w holds the instances 4w..4w+3
        pb = problem(N, B, S, seed, u_bnd, spread)
        mp = altro.mpc.BatchMPC(pb, opts=altro.SolverOptions(**dict(REF_OPTS, **opts)))
        if switch is not None:
            altro._lib.debug_set(switch, 1, mp.solver.h)
        if active is not None:
            mp.set_active(np.asarray(active, dtype=np.int32))
        mp.initial_solve()
        if log:
            mp.enable_log(S)
        count = 0
        if separate:
            for i in range(S):
                mp.run_async(1, first=i)
                mp.synchronize()
                count = count + forms(mp.solver)
        else:
            mp.run_async(S, first=0)
            mp.synchronize()
            count = forms(mp.solver)
        out = snapshot(mp, log)
    _runs[key] = (out, count)
    return _runs[key]


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def all_switches(monkeypatch, **kw):
    (a, fa), (b, fb), (c, fc) = (run(monkeypatch, sw, **kw) for sw in SWITCHES)
    print("four-row phases [open, closed, first-order] x [uniform, generic], summed over the waves: default %s, no_shadow %s, no_lone %s"
          % (fa.sum(0).tolist(), fb.sum(0).tolist(), fc.sum(0).tolist()))
    assert fa[..., 0].sum() > 0 and fc[..., 0].sum() > 0, "the default and no_lone runs must take the wave-uniform variants"
    assert fb[..., 0].sum() == 0 and fb[..., 1].sum() > 0, "without shadow rows every four-row phase is the generic one"
    assert_same(a, b, "no_shadow")
    assert_same(a, c, "no_lone")
    return a, fa, fc


@pytest.mark.parametrize("N", [5, 10, 13])
def test_horizons(monkeypatch, N):
    """remainder code only / one group and a remainder knot / groups with a clamped prefetch tail; the second wave padded"""
    _, fa, _ = all_switches(monkeypatch, N=N)
    assert (fa[:, 0, 0] > 0).all() and (fa[:, 1, 0] > 0).all(), "both waves: uniform open- and closed-loop rollouts"


def test_subsets_of_a_wave(monkeypatch):
    """One, two and three rows of a wave take part (the active mask parks the others, which then only ever clone), and the
    rows that do start at different distances from their tracks, so that they fall out of step with each other."""
    active = [0, 0, 1, 0,  1, 0, 0, 1,  1, 1, 0, 1]
    a, fa, fc = all_switches(monkeypatch, B=12, S=5, spread=True, active=active)
    assert (fc[:, 0].sum(-1) > 0).all(), "no_lone: every wave runs four-row open-loop rollouts, the one-row wave included"
    assert (a["solves0"] > 0).tolist() == [bool(x) for x in active]


def test_fused_launch_equals_single_step_launches(monkeypatch):
    (a, fa), (b, fb) = run(monkeypatch, None, S=12), run(monkeypatch, None, S=12, separate=True)
    assert fa[..., 0].sum() > 0 and fb[..., 0].sum() > 0
    assert_same(a, b, "12 launches")   # (the traces: those of the last solve in both)
    all_switches(monkeypatch, S=12)


def test_generic_fallback_in_the_same_launch(monkeypatch):
    """Tight bounds and a constraint tolerance the first AL iteration does not reach: rows begin later outer iterations
    (no shift) while wave-mates begin a step (shift), the rows of a phase disagree and the generic form runs -- with the
    idle rows as clones -- next to uniform phases in one launch."""
    a, fa, _ = all_switches(monkeypatch, S=6, u_bnd=1.0, spread=True, constraint_tolerance=1e-9, iterations_outer=6)
    assert a["iterations_outer"].max() > 1
    assert fa[:, 0, 1].sum() > 0 and fa[:, 0, 0].sum() > 0, "open-loop rollouts of both forms"


def test_strict_mode(monkeypatch):
    all_switches(monkeypatch, strict=1)


def test_per_step_log(monkeypatch):
    a, _, _ = all_switches(monkeypatch, log=True)
    assert a["log_iterations"].shape == (4, 6) and (a["log_status"] == altro.SOLVE_SUCCEEDED).all()


def test_every_instance_matches_the_oracle(monkeypatch, oracle):
    """N = 10, batch 6, stepped through the reference's MPC update order: the tolerance of test_gpu_parity (1e-6)"""
    a, fa = run(monkeypatch, None)
    assert fa[..., 0].sum() > 0
    pb = problem(10, 6, 4, 5, 3.0, False)
    st = type("St", (), {k: a[k] for k in ("iterations", "iterations_outer", "status", "cost", "c_max", "cost_trace", "cmax_trace")})
    for b in range(6):
        o = make_oracle(oracle, pb, b)
        so = o.solve()
        for i in range(4):
            mpc_update(o, pb, b, i)
            so = o.solve()
        check_against_oracle(st, a["X"], a["U"], b, o, so)
