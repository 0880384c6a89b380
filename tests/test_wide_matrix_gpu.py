"""Every instantiation of the one-wave-per-instance kernel (solve_wide.h ALTRO_WIDE_KERNELS) against the CPU oracle, with
constraints that bind: the table of tests/wide_matrix.py (tests/test_wide_matrix.py holds the inputs to that, on the oracle
alone).  Every tolerance is the project's RTOL = 1e-6, exact integer equality or byte equality."""
import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
import wide_matrix as wm
from helpers import REF_OPTS, make_oracle, mpc_update
from test_gpu_parity import RTOL, check_against_oracle, rel_err   # the headline parity test's constants

pytestmark = pytest.mark.gpu

SWITCH_CASES = ["24x7-r10", "48x13-r10", "64x4-r10"]


def check_duals_and_gains(sv, pr, orcs, gains=True, tag=""):
    """Duals of every constraint block as test_conic_option_fuzz_matches_oracle compares them, gains as the sizes test does."""
    Kg, dg = altro.gains(sv)
    for b, o in enumerate(orcs):
        for ci, kind in enumerate(pr.kinds):
            lam_o = o.duals(o.con_ids[ci])
            lam_g = altro.get_duals(sv, ci)[b].reshape(-1)
            err = np.abs(lam_g - lam_o).max() / max(1.0, np.abs(lam_o).max())
            print("%s instance %d duals of %s: %.2e (largest %.3g)" % (tag, b, kind, err, np.abs(lam_o).max()))
            assert err <= RTOL, (tag, b, kind, err)
        if gains:
            Ko, do = o.gains()
            print("%s instance %d gains: K %.2e, d %.2e" % (tag, b, rel_err(Kg[b], Ko), rel_err(dg[b], do)))
            assert rel_err(Kg[b], Ko) <= RTOL and rel_err(dg[b], do) <= RTOL, (tag, b)


def solve_rows(oracle, pr, warm):
    sv = altro.ALTROSolver(wm.rows_gpu_problem(altro, pr), altro.SolverOptions(**pr.opts))
    assert altro.wave_cycles(sv).size == 0        # the wide path
    orcs = wm.rows_oracles(oracle, pr)
    for rep in range(2 if warm else 1):
        if rep:
            altro.set_initial_state(sv, pr.x0_warm)
            for b, o in enumerate(orcs):
                o.set_initial_state(pr.x0_warm[b])
        altro.solve(sv)
        st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
        sos = [o.solve() for o in orcs]
        print("%s solve: status %s, iterations %s, outer %s" % ("warm" if rep else "cold", st.status.tolist(), st.iterations.tolist(), st.iterations_outer.tolist()))
        for b, o in enumerate(orcs):
            check_against_oracle(st, X, U, b, o, sos[b])
        check_duals_and_gains(sv, pr, orcs, tag="warm" if rep else "cold")
    return sv


@pytest.mark.parametrize("cid", [c.id for c in wm.CASES])
def test_rows_time_invariant_match_oracle(oracle, cid):
    """LINEAR inequality and equality rows, a second-order cone, a control box and a state bound, all binding (scaled from the
    unconstrained solution), on the instantiation the case reaches: a cold solve and a warm solve from x0 moved by 2 %.
    Status, both iteration counts, cost, c_max, both traces, X, U, the duals of every block and the gains, at RTOL."""
    solve_rows(oracle, wm.rows_problem(wm.CASE_BY_ID[cid], False), warm=True)


@pytest.mark.parametrize("cid", [c.id for c in wm.CASES])
def test_rows_per_knot_dynamics_match_oracle(oracle, cid):
    """The same rows over per-knot A_k, B_k and affine d_k (the `ltv` paths of the kernel: dynamics blocks streamed two knots
    ahead, no compact carve-up): a cold solve with the same checks."""
    solve_rows(oracle, wm.rows_problem(wm.CASE_BY_ID[cid], True), warm=False)


@pytest.mark.parametrize("bid", [bc.id for bc in wm.BOX_CASES])
def test_box_only_mpc_matches_oracle_and_fused_equals_single_steps(oracle, bid):
    """Box-only MPC with a bound that controls sit on at every step (test_mpc_loop_wide_kernel_sizes_match_oracle keeps the
    generator's |u| <= 3, which at most sizes never binds): initial solve and three steps against the oracle as
    test_mpc_loop_matches_oracle compares them, plus the box duals; then the same three steps as one fused launch, byte for byte."""
    bc = wm.BOX_BY_ID[bid]
    pb = wm.box_problem(bc)
    S, N, nz = wm.BOX_STEPS, bc.N, bc.n + bc.m
    mp = altro.mpc.BatchMPC(pb)
    assert altro.wave_cycles(mp.solver).size == 0
    mp.initial_solve()
    orcs = [make_oracle(oracle, pb, b) for b in range(wm.B)]
    sos = [o.solve() for o in orcs]
    st, X, U, L = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), altro.get_duals(mp.solver)
    Kg, dg = altro.gains(mp.solver)
    for b, o in enumerate(orcs):
        check_against_oracle(st, X, U, b, o, sos[b])
        Ko, do = o.gains()
        assert rel_err(Kg[b], Ko) <= RTOL and rel_err(dg[b], do) <= RTOL
    for i in range(S):
        mp.step(i)
        st, X, U, L = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), altro.get_duals(mp.solver)
        x0g = mp.x0()
        for b, o in enumerate(orcs):
            x0 = mpc_update(o, pb, b, i)
            assert np.abs(x0 - x0g[b]).max() <= 1e-12 * max(1.0, np.abs(x0).max())
            check_against_oracle(st, X, U, b, o, o.solve())
            assert np.array_equal(X[b, 0], x0g[b])
            lo = o.duals(0).reshape(N - 1, 2, nz)
            assert np.abs(L[b][:N - 1] - lo).max() <= RTOL * max(1.0, np.abs(lo).max()), (i, b)
    mf = altro.mpc.BatchMPC(pb)
    mf.initial_solve()
    mf.run_async(S, first=0)
    mf.synchronize()
    sf = altro.stats(mf.solver)
    assert np.array_equal(altro.states(mf.solver), X) and np.array_equal(altro.controls(mf.solver), U)
    assert np.array_equal(altro.get_duals(mf.solver), L) and np.array_equal(mf.x0(), x0g)
    assert np.array_equal(sf.iterations, st.iterations) and np.array_equal(sf.iterations_outer, st.iterations_outer)
    assert np.array_equal(sf.status, st.status) and np.array_equal(sf.cost, st.cost) and np.array_equal(sf.c_max, st.c_max)


def _everything(sv, pr):
    st = altro.stats(sv)
    K, d = altro.gains(sv)
    out = dict(X=altro.states(sv), U=altro.controls(sv), K=K, d=d, iterations=st.iterations, outer=st.iterations_outer, status=st.status,
               cost=st.cost, c_max=st.c_max, cost_trace=st.cost_trace, cmax_trace=st.cmax_trace)
    for ci, kind in enumerate(pr.kinds):
        out["duals_" + kind] = altro.get_duals(sv, ci)
    return out


def _run_with(monkeypatch, pr, var, value):
    """Cold and warm solve of the case on a solver created with the switch set (the switches are read at create time)."""
    if var:
        monkeypatch.setenv(var, value)
    sv = altro.ALTROSolver(wm.rows_gpu_problem(altro, pr), altro.SolverOptions(**pr.opts))
    if var:
        monkeypatch.delenv(var)
    altro.solve(sv)
    cold = _everything(sv, pr)
    altro.set_initial_state(sv, pr.x0_warm)
    altro.solve(sv)
    return cold, _everything(sv, pr)


def _assert_same_bytes(a, b, what):
    for ra, rb in zip(a, b):
        assert np.all(ra["status"] == altro.SOLVE_SUCCEEDED)
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), (what, k)


@pytest.mark.parametrize("cid", SWITCH_CASES)
def test_static_mask_switch_does_not_change_results(monkeypatch, cid):
    """wide_static_mask selects which uses of time-invariant constraint tables (rollouts, row values of expansion and dual
    update, expansion tables) read the copy kept in LDS instead of the tables in HBM: the same operands from another place.
    ALTRO_WIDE_STATIC_MASK=0 (everything from HBM) against the default (7), cold and warm solve: states, controls, duals of
    every block, statistics with both traces, and gains, byte for byte."""
    pr = wm.rows_problem(wm.CASE_BY_ID[cid], False)
    _assert_same_bytes(_run_with(monkeypatch, pr, None, None), _run_with(monkeypatch, pr, "ALTRO_WIDE_STATIC_MASK", "0"), "static mask")


@pytest.mark.parametrize("cid", SWITCH_CASES)
def test_cooperative_blocks_do_not_change_results(monkeypatch, cid):
    """wide_coop = 1 launches four waves per instance and the helper waves take 16-row strips of the backward pass's products
    (coop_exec); wide_coop = 0 is one wave.  BYTE EQUALITY, from reading the products: a strip is computed by the same
    gemm_rows call in both forms -- same tiles, same k order, same MFMA chain -- and only the wave that runs it differs;
    products that accumulate into the same matrix (S += Qux'K, then -rho K'K; the three A_c' D A_c products) keep their
    order because a strip of one matrix always goes to the same wave, and different matrices do not overlap; the
    symmetrisation averages a + b and b + a.  The switch also moves (24, 7) off the compact carve-up (a cooperative block
    never uses it), which test_wide_kernel_compact_lds_layout_does_not_change_results pins as bit-neutral.  By default
    (24, 7) is one wave and (48, 13), (64, 4) are cooperative, so each side is also the default of some case, which
    test_rows_time_invariant_match_oracle holds to the oracle."""
    pr = wm.rows_problem(wm.CASE_BY_ID[cid], False)
    _assert_same_bytes(_run_with(monkeypatch, pr, "ALTRO_WIDE_COOP", "0"), _run_with(monkeypatch, pr, "ALTRO_WIDE_COOP", "1"), "coop")


def test_lds_limit_both_sides(oracle):
    """prepare_launch refuses a carve-up above 160 KB.  (64, 16) with 12 generic rows is the last that fits (160 832 B): it
    solves and matches the oracle; with 13 rows, and (64, 17) without any (m pads to 32), the solve returns ERR_UNSUPPORTED.
    wide_matrix.lds_bytes puts each of the three on the same side."""
    assert wm.lds_bytes(wm.LDS_FITS.n, wm.LDS_FITS.m, wm.LDS_FITS.rows) <= wm.LDS_LIMIT
    assert wm.lds_bytes(wm.LDS_OVER.n, wm.LDS_OVER.m, wm.LDS_OVER.rows) > wm.LDS_LIMIT
    assert wm.lds_bytes(*wm.LDS_OVER_BOX, 0) > wm.LDS_LIMIT
    solve_rows(oracle, wm.rows_problem(wm.LDS_FITS, False), warm=False)
    pr = wm.rows_problem(wm.LDS_OVER, False)
    sv = altro.ALTROSolver(wm.rows_gpu_problem(altro, pr), altro.SolverOptions(**pr.opts))
    with pytest.raises(altro.AltroError) as e:
        altro.solve(sv)
    assert e.value.code == altro._lib.ERR_UNSUPPORTED
    n, m = wm.LDS_OVER_BOX
    mp = altro.mpc.BatchMPC(altro.problems.gen_random_linear_batch(wm.B, n=n, m=m, N=8, steps=1, seed=21))
    with pytest.raises(altro.AltroError) as e:
        mp.initial_solve()
    assert e.value.code == altro._lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("u_bnd", [1.0, 3.0])
def test_fused_launch_right_after_a_setter_equals_single_steps(u_bnd):
    """With projected_newton = 1 a fused launch is S pairs of (one-step solve kernel, polish kernel), each with its own kernel
    arguments.  A setter drops the stored gains; the FIRST step of the launch must see that, the later ones must not -- as in S
    single steps, where the second step may already reuse the pass the first one stored.  (The arguments used to carry
    "dropped" for every step of the launch.)  altro_batch_set_options immediately before run_async(S) against S single steps
    on a twin: states, controls and duals byte for byte, and the same backward passes, rollouts, trials and reused passes.
    u_bnd = 1: controls saturate, every solve ends at a penalty above the initial one, and the next step's first iteration
    cannot take the stored pass whatever the arguments say (reuse asks for the same penalty) -- the two agreed before the
    change too.  u_bnd = 3 (the generator's own): most solves end in one outer iteration and the next step starts from the
    stored pass; this is the case the arguments decide."""
    B, S = 5, 6
    n, m, N = 20, 4, 21
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=87)
    pb.u_bnd = u_bnd
    opts = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)
    a = altro.mpc.BatchMPC(pb, altro.SolverOptions(**opts))
    b = altro.mpc.BatchMPC(pb, altro.SolverOptions(**opts))
    assert altro.wave_cycles(a.solver).size == 0
    for mp in (a, b):
        mp.initial_solve()
        altro.timing_reset(mp.solver)
        altro.set_options(mp.solver, cost_tolerance=opts["cost_tolerance"])     # same options: the setter alone
    a.run_async(S, first=0)
    a.synchronize()
    for i in range(S):
        b.step(i)
    wa, wb = altro.work_counters(a.solver), altro.work_counters(b.solver)
    ra, rb = altro.reuse_counter(a.solver), altro.reuse_counter(b.solver)
    print("fused: backward %s rollouts %s trials %s reused %s" % (wa[0].tolist(), wa[1].tolist(), wa[2].tolist(), ra.tolist()))
    print("single: backward %s rollouts %s trials %s reused %s" % (wb[0].tolist(), wb[1].tolist(), wb[2].tolist(), rb.tolist()))
    assert np.array_equal(altro.states(a.solver), altro.states(b.solver))
    assert np.array_equal(altro.controls(a.solver), altro.controls(b.solver))
    assert np.array_equal(altro.get_duals(a.solver), altro.get_duals(b.solver))
    assert np.array_equal(a.x0(), b.x0())
    for ca, cb in zip(wa, wb):
        assert np.array_equal(ca, cb)
    assert np.array_equal(ra, rb)
    assert rb.sum() > 0       # passes were reused across steps: the comparison is about something
