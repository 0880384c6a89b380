"""Every instantiation of the 16-lane kernel (altro_batch.hip launch_solve: solve_kernel<NX, NU, CONES> at five shapes) against the
CPU oracle with LINEAR / SOC rows that bind, and every edge of the lane packing: the table of tests/lane16_matrix.py
(tests/test_lane16_matrix.py holds the inputs and the packing to that, without a GPU).  Every tolerance is the project's
RTOL = 1e-6, exact integer equality or byte equality; the polish case uses those of test_projected_newton_polish_matches_oracle (a)."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
import lane16_matrix as lm
import wide_matrix as wm
from helpers import mpc_update
from test_gpu_parity import RTOL, check_against_oracle, rel_err
from test_wide_matrix_gpu import _assert_same_bytes, _everything, check_duals_and_gains

pytestmark = pytest.mark.gpu

B, N = lm.B, lm.N
ALL = [lm.shape_id(s) for s in lm.SHAPES]
QUADS = [lm.shape_id(s) for s in lm.QUAD_SHAPES]


def new_solver(pr, on_16_lanes=True):
    sv = altro.ALTROSolver(lm.gpu_problem(altro, pr), altro.SolverOptions(**pr.opts))
    assert (altro.wave_cycles(sv).size > 0) == on_16_lanes
    return sv


def solve_rows(oracle, pr, warm, on_16_lanes=True):
    """Cold (and warm, from x0_warm) solve against one oracle per instance: status, both iteration counts, cost, c_max, both
    traces, X, U, the duals of every block and the gains K, d (the conic kernels keep d in Dff, not in the gain rows)."""
    sv = new_solver(pr, on_16_lanes)
    orcs = wm.rows_oracles(oracle, pr)
    assert len(orcs) == B
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
            assert not wm.at_penalty_cap(sos[b])
            check_against_oracle(st, X, U, b, o, sos[b])
        check_duals_and_gains(sv, pr, orcs, tag="warm" if rep else "cold")
    return sv


@pytest.mark.parametrize("sid", ALL)
def test_rows10_time_invariant_match_oracle(oracle, sid):
    """<n, m, true> at every shape: four mixing inequality rows (the first in the spare lane of the cone's quad), a terminal
    equality on the cone's lanes, a cone, a box, a state bound -- all binding; cold and warm solve, every instance."""
    solve_rows(oracle, lm.rows_problem(lm.SHAPE_BY_ID[sid], "ti"), warm=True)


@pytest.mark.parametrize("sid", ALL)
def test_rows10_per_instance_constraint_data_match_oracle(oracle, sid):
    """The same rows with the mixing rows, the cone and the state bound as per_instance blocks (con_istride != 0; the padded
    rows of the second wave read the last instance's tables), the equality and the box shared: cold solve."""
    pr = lm.rows_problem(lm.SHAPE_BY_ID[sid], "pi")
    assert sorted(lm.per_instance_blocks(pr)) == [0, 2, 4]
    solve_rows(oracle, pr, warm=False)


def test_rows10_per_knot_dynamics_move_to_the_wide_kernel_and_match_oracle(oracle):
    """Per-knot dynamics on a 16-lane size move the handle to the one-wave-per-instance backend by design
    (test_per_knot_dynamics_on_a_16_lane_size_move_to_the_wide_kernel); with rows on it that is the kernel of wide_matrix's
    16x4 case, so ONE shape is kept here, (12, 4): that the move happens with constraints present, and the oracle's answer."""
    pr = lm.rows_problem((12, 4), "ltv")
    solve_rows(oracle, pr, warm=False, on_16_lanes=False)


@pytest.mark.parametrize("sid", QUADS)
def test_quads_all_16_lanes_match_oracle(oracle, sid):
    """All 16 lanes at knots 6..N-2, cones of dimension 4, 2, 3 and a quad that holds a p = 2 cone on knots 0..5 and a p = 3
    cone after, linear rows in the spare lanes 6, 7, 11, 15 and in lane 14 before the cone takes it: cold and warm."""
    solve_rows(oracle, lm.quads_problem(lm.SHAPE_BY_ID[sid]), warm=True)


@pytest.mark.parametrize("sid", ["12x4", "6x6"])
def test_quads_projected_newton_polish_matches_oracle(oracle, sid):
    """The 16-lane polish view (pn_polish.h row_kind / cone_size) reading linear rows out of cone quads' spare lanes: the
    quads case with projected_newton = 1, constraint_tolerance = 1e-8, tolerances of test_projected_newton_polish_matches_oracle (a)."""
    pr = lm.quads_problem(lm.SHAPE_BY_ID[sid])
    pr = replace(pr, opts=dict(pr.opts, constraint_tolerance=1e-8, projected_newton=1))
    sv = new_solver(pr)
    altro.solve(sv)
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    ran, failed, res = altro.polish_stats(sv)
    d0, d1, dfail = altro.polish_dual_residuals(sv)
    print("polish ran %s, failed %s, c_max %s, dual residual %s -> %s" % (ran.tolist(), failed.tolist(), st.c_max.tolist(), d0.tolist(), d1.tolist()))
    assert ran.sum() >= 1 and not failed.any()
    for b, o in enumerate(wm.rows_oracles(oracle, pr)):
        so = o.solve()
        assert int(st.status[b]) == so.status == 1 and int(st.iterations[b]) == so.iterations and int(ran[b]) == so.pn_ran
        assert abs(st.cost[b] - so.cost) <= RTOL * max(1.0, abs(so.cost)) and st.c_max[b] < 1e-8
        assert abs(st.c_max[b] - so.c_max) <= RTOL * max(1.0, abs(so.c_max))
        assert rel_err(X[b], o.states()) <= RTOL and rel_err(U[b], o.controls()) <= RTOL
        assert int(dfail[b]) == so.pn_dual_failed == 0
        assert abs(d0[b] - so.pn_dual_residual0) <= 1e-6 * max(1.0, so.pn_dual_residual0) and abs(d1[b] - so.pn_dual_residual) <= 1e-6 * max(1.0, so.pn_dual_residual0)


# ---------------------------------------------------------------------------------------------------------------------
# the tracking loop
def _track_everything(mp, tp):
    out = _everything(mp.solver, tp)
    out["x0"] = mp.x0()
    return out


def _track_single_steps(tp, check=None):
    mp = lm.track_mpc(altro, tp)
    assert altro.wave_cycles(mp.solver).size > 0
    mp.initial_solve()
    if check:
        check(mp, -1)
    for i in range(lm.TRACK_STEPS):
        mp.step(i)
        if check:
            check(mp, i)
    return mp


def _track_fused(tp):
    mf = lm.track_mpc(altro, tp)
    mf.initial_solve()
    mf.run_async(lm.TRACK_STEPS, first=0)
    mf.synchronize()
    return mf


@pytest.mark.parametrize("sid", ALL)
def test_track_mpc_loop_matches_oracle_and_fused_equals_single_steps(oracle, sid):
    """Tracking MPC with a cone, two linear rows (one in the cone quad's spare lane), a box and a state bound whose lane's
    canonical knot is 1 (con_inv = 1: the sweeps load each lane's row once): initial solve and three steps against one oracle
    per instance in mpc_update's order (x0 to 1e-12), the duals of every block after every step; then the three steps as one
    fused launch on a twin, byte for byte."""
    tp = lm.track_problem(lm.SHAPE_BY_ID[sid])
    pk = lm.pack(tp.cons, N)
    assert pk.con_inv == 1 and pk.ckn[5] == 1
    orcs = lm.track_oracles(oracle, tp)

    def check(mp, i):
        sv = mp.solver
        st, X, U, x0g = altro.stats(sv), altro.states(sv), altro.controls(sv), mp.x0()
        for b, o in enumerate(orcs):
            if i >= 0:
                x0 = mpc_update(o, tp.pb, b, i)
                assert np.abs(x0 - x0g[b]).max() <= 1e-12 * max(1.0, np.abs(x0).max())
                assert np.array_equal(X[b, 0], x0g[b])
            so = o.solve()
            assert not wm.at_penalty_cap(so)
            check_against_oracle(st, X, U, b, o, so)
        check_duals_and_gains(sv, tp, orcs, tag="step %d" % i)

    mp = _track_single_steps(tp, check)
    _assert_same_bytes([_track_everything(mp, tp)], [_track_everything(_track_fused(tp), tp)], "fused")


# ---------------------------------------------------------------------------------------------------------------------
# switches
def _rows_cold_warm(pr):
    sv = new_solver(pr)
    altro.solve(sv)
    cold = _everything(sv, pr)
    altro.set_initial_state(sv, pr.x0_warm)
    altro.solve(sv)
    return cold, _everything(sv, pr)


@pytest.mark.parametrize("switches", [("ALTRO_NO_SHADOW", "ALTRO_NO_MATE_RANK"), ("ALTRO_NO_REUSE",)], ids=["shadow+mate", "reuse"])
def test_scheduling_switches_do_not_change_the_conic_kernels_results(monkeypatch, switches):
    """Idle rows shadowing a busy one, issue priority by the work a SIMD's wave has left, and gain reuse (which the conic kernels
    never take: kvalid is computed in the box-only kernels alone) decide when and in which wave a row works, never what it
    computes: the quads case at (12, 4), cold and warm, and the track loop at (8, 4), single steps and fused, with the
    switches set at create time against the defaults -- states, controls, gains, duals of every block and statistics with both
    traces, byte for byte."""
    pr, tp = lm.quads_problem((12, 4)), lm.track_problem((8, 4))
    base = _rows_cold_warm(pr)
    base_t = [_track_everything(_track_single_steps(tp), tp), _track_everything(_track_fused(tp), tp)]
    for var in switches:
        monkeypatch.setenv(var, "1")
    _assert_same_bytes(base, _rows_cold_warm(pr), switches)
    _assert_same_bytes(base_t, [_track_everything(_track_single_steps(tp), tp), _track_everything(_track_fused(tp), tp)], switches)


# ---------------------------------------------------------------------------------------------------------------------
# limits
def _add_block(sv, c):
    """altro_batch_add_constraint on a handle that exists: the return code; an accepted block joins the solver's lists."""
    api, L = altro.api, altro._lib
    soc = c.kind == lm.P.SOC
    con = altro.NormConstraint(c.A, c.b) if soc else altro.LinearConstraint(c.A, c.b, equality=(c.sense == lm.P.EQ))
    cid = C.c_int32(-1)
    rc = sv._L.altro_batch_add_constraint(sv.h, L.CON_SOC if soc else L.CON_LINEAR, L.SENSE_EQ if (not soc and c.sense == lm.P.EQ) else L.SENSE_INEQ,
                                          c.k_first, c.k_last, c.A.shape[0], api._p(api._c(c.A)), api._p(api._c(c.b)), None, None, 0, C.byref(cid))
    if rc == 0:
        sv.prob.constraints.items.append((con, c.k_first + 1, c.k_last + 1))
        sv.con_ids.append(cid.value)
    return rc


def test_row_and_cone_limits_refuse_and_leave_the_handle_as_it_was(oracle):
    """(12, 4), the quads problem: every lane is taken at knots 1..N-2 and four cones stand at knots 1..5.  A 17th row at a full
    knot and a 5th cone over knots 3..4 return ERR_UNSUPPORTED; altro_batch_add_constraint then pops the block and packs again,
    and the handle solves (cold and warm) to the bytes of a twin that never attempted the add.  The 5th cone of the problem
    itself (soc3m, on knots disjoint from soc2m's) is taken when it is added to a handle that holds the other eight blocks,
    and the solve matches the oracle."""
    pr = lm.quads_problem((12, 4))
    nz = pr.rp.n + pr.rp.m
    twin = _rows_cold_warm(pr)
    row = lm.P.ConstraintSpec(lm.P.LINEAR, lm.P.INEQ, 8, 8, A=np.ones((1, nz)), b=np.array([-1e3]))
    cone = lm.P.ConstraintSpec(lm.P.SOC, lm.P.INEQ, 3, 4, A=np.eye(2, nz), b=np.array([0.0, 1e3]))
    for extra in (row, cone):
        with pytest.raises(lm.Unsupported):
            lm.pack(pr.rp.constraints + [extra], N)
        sv = new_solver(pr)
        assert _add_block(sv, extra) == altro._lib.ERR_UNSUPPORTED
        altro.solve(sv)
        cold = _everything(sv, pr)
        altro.set_initial_state(sv, pr.x0_warm)
        altro.solve(sv)
        _assert_same_bytes(twin, (cold, _everything(sv, pr)), "after a refused block")
    # soc3m last: the same lanes as in the table's order (cones are packed first, in the order they were added)
    ci = pr.kinds.index("soc3m")
    order = [i for i in range(len(pr.kinds)) if i != ci] + [ci]
    late = replace(pr, rp=replace(pr.rp, constraints=[pr.rp.constraints[i] for i in order]), kinds=[pr.kinds[i] for i in order])
    assert lm.packed(late).lanes[len(order) - 1] == [12, 13, 14] and np.array_equal(lm.packed(late).meta, lm.packed(pr).meta)
    prob = lm.gpu_problem(altro, late)
    prob.constraints.items.pop()
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**late.opts))
    assert altro.wave_cycles(sv).size > 0
    assert _add_block(sv, late.rp.constraints[-1]) == 0 and len(sv.con_ids) == len(order)
    altro.solve(sv)
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    orcs = wm.rows_oracles(oracle, late)
    for b, o in enumerate(orcs):
        check_against_oracle(st, X, U, b, o, o.solve())
    check_duals_and_gains(sv, late, orcs, tag="late cone")
