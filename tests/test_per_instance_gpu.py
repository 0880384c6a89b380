"""Per-instance tracking-cost weights and box bounds (altro_batch_set_tracking_cost_per_instance, altro_batch_set_bounds)
on the GPU: instance i of a batch whose problems differ gives, bit for bit, what a handle whose shared setters were given
instance i's values gives -- on the 16-lane kernels (lone and shadowed phases included), on the one-wave-per-instance
kernel, in the fused MPC loop and in the projected-Newton polish -- and matches the CPU oracle given its own values."""
import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import problems as P
from helpers import REF_OPTS, ROCKET_COLD_OPTS, mpc_update, rocket_gpu_problem

pytestmark = pytest.mark.gpu

RTOL = 1e-6


def rel_err(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def snapshot(sv):
    """every per-instance output of a handle, instance-major"""
    st = altro.stats(sv)
    K, d = altro.gains(sv)
    out = dict(X=altro.states(sv), U=altro.controls(sv), it=st.iterations, ito=st.iterations_outer, status=st.status,
               cost=st.cost, cmax=st.c_max, Jt=st.cost_trace, ct=st.cmax_trace, alpha=altro.alpha_trace(sv), K=K, d=d,
               reuse=altro.reuse_counter(sv), confirm=altro.confirm_counter(sv))
    for i, a in enumerate(altro.work_counters(sv)):
        out["work%d" % i] = a
    for i, a in enumerate(altro.solve_counters(sv)):
        out["solves%d" % i] = a
    for c in range(len(sv.con_ids)):
        out["dual%d" % c] = altro.get_duals(sv, c)
    return out


def assert_same(a, b, rows=None, what=""):
    for k in a:
        x, y = a[k], b[k]
        if rows is not None:
            x, y = x[rows], y[rows]
        assert np.array_equal(x, y), (what, k)


def classes(pb, B, ncls=4, seed=5):
    """four classes of (Q, R, Qf, u_bnd), given to the instances at random"""
    rng = np.random.default_rng(seed)
    n, m, N = pb.n, pb.m, pb.N
    Q = 10.0 * rng.random((ncls, n))
    R = 0.05 + 0.2 * rng.random((ncls, m))
    Qf = (N - 1) * Q
    ub = rng.uniform(1.5, 4.0, ncls)
    cls = rng.integers(0, ncls, B)
    cls[:ncls] = np.arange(ncls)
    return cls, Q, R, Qf, ub


def with_values(pb, Q, R, Qf, ub):
    q = P.RandomLinearBatch(**{k: getattr(pb, k) for k in ("n", "m", "N", "dt", "A", "Bm", "Xtrack", "Utrack", "noise")})
    q.Qk, q.Rk, q.Qfk, q.u_bnd = Q, R, Qf, ub
    return q


def run_mpc(pb, S, opts=None):
    mp = altro.mpc.BatchMPC(pb, opts=altro.SolverOptions(**(opts or REF_OPTS)))
    mp.initial_solve()
    altro.timing_reset(mp.solver)
    mp.run_async(S, first=0)
    mp.synchronize()
    return mp


BOX16 = [(12, 4, 50), (6, 6, 31), (8, 4, 21)]
WIDE = [(16, 4, 30), (24, 4, 21), (30, 15, 21)]


@pytest.mark.parametrize("n,m,N", BOX16 + WIDE)
def test_uniform_per_instance_tables_equal_the_shared_setters(n, m, N):
    """Every row the same: the per-instance calls give the shared setters' results bit for bit, gain reuse included."""
    B, S = 18, 8
    pb = P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=21)
    a = run_mpc(pb, S)
    q = with_values(pb, np.full((B, n), pb.Qk), np.full((B, m), pb.Rk), np.full((B, n), pb.Qfk), np.full(B, pb.u_bnd))
    b = run_mpc(q, S)
    assert_same(snapshot(a.solver), snapshot(b.solver), what=(n, m))
    assert np.array_equal(a.x0(), b.x0())
    if (n, m) in ((12, 4), (16, 4), (24, 4)):
        assert int(altro.reuse_counter(b.solver).sum()) > 0


def test_uniform_per_instance_tables_on_the_conic_kernel(oracle):
    """(6, 3) with a second-order cone (rocket): per-instance weights equal to the shared ones give the same solve."""
    rp = P.gen_rocket_problem(N=41, tf=4.0)
    B = 6
    x0 = np.tile(rp.x0, (B, 1)) + 0.1 * np.random.default_rng(2).standard_normal((B, rp.n))
    opts = altro.SolverOptions(**ROCKET_COLD_OPTS)
    prob = rocket_gpu_problem(altro, rp, x0)
    a = altro.ALTROSolver(prob, opts)
    altro.solve(a)
    prob.obj.Q, prob.obj.R, prob.obj.Qf = (np.tile(np.asarray(v, dtype=float), (B, 1)) for v in (rp.Q, rp.R, rp.Qf))
    b = altro.ALTROSolver(prob, opts)
    altro.solve(b)
    assert_same(snapshot(a), snapshot(b))


@pytest.mark.parametrize("n,m,N,switch", [(n, m, N, sw) for (n, m, N) in BOX16 for sw in (None, "ALTRO_NO_LONE", "ALTRO_NO_SHADOW", "ALTRO_NO_GROUP")]
                         + [(n, m, N, None) for (n, m, N) in WIDE])
def test_heterogeneous_batch_equals_its_homogeneous_sub_batches(monkeypatch, n, m, N, switch):
    """Four classes of weights and bounds spread over the batch: instance i equals instance i of a handle built with its
    class's values through the shared setters -- with the default scheduling and with each of the 16-lane kernels'
    scheduling features off.  A lane that read its own instance's row in a lone or shadowed phase (where it works for
    another instance) would break this."""
    if switch is not None:
        monkeypatch.setenv(switch, "1")
    B, S = 43, 10
    pb = P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=23)
    cls, Q, R, Qf, ub = classes(pb, B)
    het = run_mpc(with_values(pb, Q[cls], R[cls], Qf[cls], ub[cls]), S)
    hs = snapshot(het.solver)
    for c in range(len(ub)):
        hom = run_mpc(with_values(pb, Q[c], R[c], Qf[c], float(ub[c])), S)
        rows = np.nonzero(cls == c)[0]
        assert_same(snapshot(hom.solver), hs, rows=rows, what=(switch, c))
        assert np.array_equal(hom.x0()[rows], het.x0()[rows])


def make_oracle_pi(O, pb, b, opts=None):
    n, m, N = pb.n, pb.m, pb.N
    s = O.OracleSolver(n, m, N, pb.dt)
    s.set_dynamics(pb.A[b], pb.Bm[b])
    s.set_cost(pb.Qk[b], np.full(m, pb.Rk), pb.Qfk[b])
    zmin = np.r_[np.full(n, -np.inf), np.full(m, -pb.u_bnd[b])]
    s.add_box(zmin, -zmin, 0, N - 2)
    s.set_opts(O.default_opts(**(opts or REF_OPTS)))
    Xr, Ur = pb.window(0)
    s.set_reference(Xr[b], Ur[b])
    s.set_initial_state(Xr[b, 0])
    s.set_controls(Ur[b])
    return s


def check_against_oracle(st, X, U, b, orc, so):
    assert int(st.status[b]) == so.status
    assert int(st.iterations[b]) == so.iterations
    assert int(st.iterations_outer[b]) == so.iterations_outer
    assert abs(st.cost[b] - so.cost) <= RTOL * max(1.0, abs(so.cost))
    assert abs(st.c_max[b] - so.c_max) <= RTOL * max(1.0, abs(so.c_max))
    assert rel_err(X[b], orc.states()) <= RTOL
    assert rel_err(U[b], orc.controls()) <= RTOL


@pytest.mark.parametrize("n,m,N,force_wide", [(12, 4, 50, 0), (12, 4, 50, 1), (6, 3, 21, 0), (16, 4, 30, 0)])
def test_heterogeneous_mpc_loop_matches_oracle(oracle, monkeypatch, n, m, N, force_wide):
    """gen_random_linear's own per-problem draws (Q = 10 rand(n), Qf = (N-1) Q) and u_bnd in [1.5, 4], step by step
    against one oracle per instance given its own values."""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    B, S = 10, 6
    pb = P.gen_random_linear_hetero_batch(B, n=n, m=m, N=N, steps=S, seed=11)
    mp = altro.mpc.BatchMPC(pb)
    mp.initial_solve()
    orcs = [make_oracle_pi(oracle, pb, b) for b in range(B)]
    sos = [o.solve() for o in orcs]
    st, X, U = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver)
    for b in range(B):
        check_against_oracle(st, X, U, b, orcs[b], sos[b])
    assert np.all(np.abs(U) <= pb.u_bnd[:, None, None] + 1e-3)
    for i in range(S):
        mp.step(i)
        st, X, U = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver)
        for b in range(B):
            mpc_update(orcs[b], pb, b, i)
            check_against_oracle(st, X, U, b, orcs[b], orcs[b].solve())


@pytest.mark.parametrize("force_wide", [0, 1])
def test_projected_newton_polish_with_per_instance_bounds(oracle, monkeypatch, force_wide):
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    B = 6
    pb = P.gen_random_linear_hetero_batch(B, steps=1, seed=81)
    prob = altro.mpc.gen_tracking_problem(pb)
    rng = np.random.default_rng(3)
    prob.x0 = prob.x0 + np.array([25.0, 25.0, 0.1, 12.0, 25.0, 20.0])[:, None] + rng.standard_normal(prob.x0.shape)
    opts = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**opts))
    altro.solve(sv)
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    ran, failed, res = altro.polish_stats(sv)
    assert ran.sum() >= 2 and not failed.any()
    for b in range(B):
        o = make_oracle_pi(oracle, pb, b, opts=opts)
        o.set_initial_state(prob.x0[b])
        so = o.solve()
        assert int(st.status[b]) == so.status and int(st.iterations[b]) == so.iterations and int(ran[b]) == so.pn_ran
        assert abs(st.cost[b] - so.cost) <= RTOL * max(1.0, abs(so.cost))
        assert rel_err(X[b], o.states()) <= RTOL and rel_err(U[b], o.controls()) <= RTOL
        assert np.abs(U[b]).max() <= pb.u_bnd[b] + 1e-8


@pytest.mark.parametrize("n,m,N", [(12, 4, 50), (16, 4, 30)])
def test_set_bounds_between_solves(oracle, n, m, N):
    """New bounds for some instances, in place: the next solve equals a fresh handle built with them (bit for bit) and a
    fresh oracle.  With stale gains it would not."""
    B = 11
    pb = P.gen_random_linear_hetero_batch(B, n=n, m=m, N=N, steps=1, seed=41)
    opts = dict(REF_OPTS, reset_duals=1, reset_penalties=1)
    prob = altro.mpc.gen_tracking_problem(pb)
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**opts))
    altro.solve(sv)
    ub = pb.u_bnd.copy()
    ub[[0, 3, 7]] = [1.2, 0.9, 1.6]
    lo = np.c_[np.full((B, n), -np.inf), -np.repeat(ub[:, None], m, axis=1)]
    altro.set_bounds(sv, 0, lo, -lo)
    altro.initial_controls(sv, prob.U0)
    altro.solve(sv)
    pb2 = with_values(pb, pb.Qk, pb.Rk, pb.Qfk, ub)
    prob2 = altro.mpc.gen_tracking_problem(pb2)
    fresh = altro.ALTROSolver(prob2, altro.SolverOptions(**opts))
    altro.solve(fresh)
    a, b = snapshot(sv), snapshot(fresh)
    for k in ("work0", "work1", "work2", "solves0", "solves1", "solves2", "reuse", "confirm"):
        a.pop(k), b.pop(k)   # the first handle has solved twice
    assert_same(a, b)
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    for i in (0, 3, 5, 7):
        o = make_oracle_pi(oracle, pb2, i, opts=opts)
        check_against_oracle(st, X, U, i, o, o.solve())
    # back to one shared row for the batch
    altro.set_bounds(sv, 0, lo[0], -lo[0])
    altro.initial_controls(sv, prob.U0)
    altro.solve(sv)
    assert np.abs(altro.controls(sv)).max() <= ub[0] + 1e-3


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (16, 4, 21)])
def test_per_instance_error_paths(n, m, N):
    B = 10
    pb = P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=3)
    prob = altro.mpc.gen_tracking_problem(pb)
    L = altro._lib.lib()
    # a handle without a BOX: set_bounds has nothing to set
    bare = altro.api.Problem(prob.model, prob.obj, altro.ConstraintList(n, m, N), x0=prob.x0, N=N, U0=prob.U0)
    s0 = altro.ALTROSolver(bare)
    z = np.zeros(n + m)
    with pytest.raises(altro.AltroError) as e:
        s0._chk(L.altro_batch_set_bounds(s0.h, 0, altro.api._p(z), altro.api._p(z), 0))
    assert e.value.code == altro._lib.ERR_INVALID_ARG
    sv = altro.ALTROSolver(prob)
    lo = np.tile(np.r_[np.full(n, -np.inf), np.full(m, -3.0)], (B, 1))
    bad = []
    x = lo.copy(); x[4, n] = -np.inf; bad.append(x)               # pattern differs in one instance
    x = lo.copy(); x[2, n + 1] = np.nan; bad.append(x)             # NaN
    for x in bad:
        with pytest.raises(altro.AltroError) as e:
            altro.set_bounds(sv, 0, x, -lo)
        assert e.value.code == altro._lib.ERR_INVALID_ARG
    hi = -lo.copy(); hi[5, n] = -4.0                               # zmin > zmax
    with pytest.raises(altro.AltroError) as e:
        altro.set_bounds(sv, 0, lo, hi)
    assert e.value.code == altro._lib.ERR_INVALID_ARG
    with pytest.raises(altro.AltroError) as e:                     # wrong batch length
        altro.set_bounds(sv, 0, lo[:-1], -lo[:-1])
    assert e.value.code == altro._lib.ERR_INVALID_ARG
    with pytest.raises(altro.AltroError) as e:
        altro.set_tracking_cost(sv, np.ones((B - 1, n)), np.ones(m), np.ones(n))
    assert e.value.code == altro._lib.ERR_INVALID_ARG
    # a LINEAR constraint is not a BOX
    cons = altro.ConstraintList(n, m, N)
    cons.add_constraint(altro.LinearConstraint(np.ones((1, n + m)), np.array([-100.0])), (1, N - 1))
    s2 = altro.ALTROSolver(altro.api.Problem(prob.model, prob.obj, cons, x0=prob.x0, N=N, U0=prob.U0))
    with pytest.raises(altro.AltroError) as e:
        altro.set_bounds(s2, 0, lo, -lo)
    assert e.value.code == altro._lib.ERR_INVALID_ARG
    # the refused calls changed nothing: the handle still solves as before
    ref = altro.ALTROSolver(prob)
    altro.solve(sv)
    altro.solve(ref)
    assert np.array_equal(altro.states(sv), altro.states(ref))
