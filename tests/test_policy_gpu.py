"""Feedback policy on the device (altro_batch_eval_policy_dev / _eval_policy / _get_gains_dev) on both backends: the value
against the host getters within the dot-product rounding bound, the exact fixed point, the clamp, the host twin, the life
cycle of `fb`, out-of-range knots, refusals, the gains getter, stream order and a two-rate closed loop.  Small shapes (N = 9;
batch 5 on the 16-lane backend, a partial wave; batch 3 on the other).  Memory is allocated through torch."""
import ctypes as C

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc, problems

pytestmark = pytest.mark.gpu
N = 9
INV = altro._lib.ERR_INVALID_ARG


def dev():
    return torch.device("cuda", 0)


def T(a):
    """numpy -> GPU tensor, same bytes"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def random_linear(B, n, m, seed, per_knot=False, cone=False, strict=0, steps=2):
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=steps, seed=seed)
    prob = mpc.gen_tracking_problem(pb)
    rng = np.random.default_rng(seed + 1)
    prob.x0 = prob.x0 + 0.3 * rng.standard_normal(prob.x0.shape)      # the solve has work to do and meets the bounds
    if per_knot:
        sc = 1.0 + 0.01 * rng.standard_normal((B, N - 1, 1, 1))
        prob.model = altro.LinearModel(pb.A[:, None] * sc, pb.Bm[:, None] * sc, 1e-3 * rng.standard_normal((B, N - 1, n)), dt=pb.dt,
                                       per_knot=True)
    if cone:   # one cone on the controls: ||u[0:m-1]|| <= u[m-1] + 5
        A = np.zeros((m, n + m))
        A[:, n:] = np.eye(m)
        b = np.zeros(m)
        b[-1] = 5.0
        prob.constraints.add_constraint(altro.NormConstraint(A, b), (1, N - 1))
    return prob, altro.SolverOptions(strict=strict, **mpc.REF_OPTS), pb


CASES = {
    "box_12x4": lambda: random_linear(5, 12, 4, 51),                       # headline kernel: d rides in KD
    "cone_6x3": lambda: random_linear(5, 6, 3, 52, cone=True),             # conic kernel: d in Dff
    "reuse_20x5": lambda: random_linear(3, 20, 5, 53),                     # wide kernel, gain-reuse class
    "ltv_12x12": lambda: random_linear(3, 12, 12, 54, per_knot=True),      # wide kernel, SM instantiation
    "wide_30x25": lambda: random_linear(3, 30, 25, 55),                    # m > 16
    "box_12x4_strict": lambda: random_linear(5, 12, 4, 51, strict=1),
}
BOTH_BACKENDS = ["box_12x4", "reuse_20x5"]


def raw_gains(sv):
    """(K, d) exactly as altro_batch_get_gains writes them: K (B, N-1, n, m) in memory (column-major m x n blocks)"""
    K, d = np.empty((sv.B, sv.N - 1, sv.n, sv.m)), np.empty((sv.B, sv.N - 1, sv.m))
    sv._chk(sv._L.altro_batch_get_gains(sv.h, api._p(K), api._p(d)))
    return K, d


class Solved:
    """one solved handle per case and what the host getters of the parent commit say about it; shared, never modified"""

    def __init__(self, case):
        self.prob, self.opts, self.pb = CASES[case]()
        self.sv = altro.ALTROSolver(self.prob, self.opts)
        altro.solve(self.sv)
        self.X, self.U = altro.states(self.sv), altro.controls(self.sv)
        self.K = altro.gains(self.sv)[0]                                    # (B, N-1, m, n)
        sv = self.sv
        rng = np.random.default_rng(7)
        self.knot = np.array([0, 1, N - 2, 1, 0][:sv.B], dtype=np.int32)
        self.Xk = self.X[np.arange(sv.B), self.knot]
        self.x = self.Xk + 1e-2 * (1.0 + np.abs(self.Xk)) * rng.standard_normal(self.Xk.shape)


_solved = {}


@pytest.fixture(scope="module")
def solved():
    def get(case):
        if case not in _solved:
            _solved[case] = Solved(case)
        return _solved[case]
    yield get
    for s in _solved.values():
        s.sv.close()
    _solved.clear()


def policy(sv, x, knot=None, clamp=False):
    """device form; returns (u, fb) as numpy"""
    fb = torch.full((sv.B,), -9, dtype=torch.int32, device=dev())
    u = altro.eval_policy(sv, T(x), None if knot is None else T(np.asarray(knot, dtype=np.int32)), clamp=clamp, fb=fb)
    return u.cpu().numpy(), fb.cpu().numpy()


@pytest.mark.parametrize("case", list(CASES))
def test_value_against_the_host_getters(case, solved):
    """u = U[b,k] + K[b,k] (x - X[b,k]) with X, U, K from the host getters, within the rounding bound of two dot products
    evaluated in different orders: |delta_a| <= 2 (n + 2) 2^-53 (|u_a| + sum_j |K_aj| |dx_j|), with or without FMA."""
    s = solved(case)
    sv = s.sv
    u, fb = policy(sv, s.x, s.knot)
    b = np.arange(sv.B)
    Uk, Kk = s.U[b, s.knot], s.K[b, s.knot]
    dx = s.x - s.Xk
    ref = Uk + np.einsum("baj,bj->ba", Kk, dx)
    bound = 2 * (sv.n + 2) * 2.0 ** -53 * (np.abs(Uk) + np.einsum("baj,bj->ba", np.abs(Kk), np.abs(dx)))
    err = np.abs(u - ref)
    print(case, "max err / bound:", float((err / bound).max()), "max |K dx|:", float(np.abs(ref - Uk).max()))
    assert (fb == 1).all(), fb
    assert np.abs(ref - Uk).max() > 1e-6            # the feedback term is really there
    assert (err <= bound).all(), (float(err.max()), float((err / bound).max()))


@pytest.mark.parametrize("case", list(CASES))
def test_exact_fixed_point(case, solved):
    """x on the trajectory returns the nominal control byte for byte, at every knot (clamp off: an AL solution may sit a
    tolerance outside its bounds)"""
    s = solved(case)
    sv = s.sv
    for k in range(N - 1):
        u, fb = policy(sv, s.X[:, k], np.full(sv.B, k))
        assert (fb == 1).all()
        assert u.tobytes() == np.ascontiguousarray(s.U[:, k]).tobytes(), (k, float(np.abs(u - s.U[:, k]).max()))
    u, fb = policy(sv, s.X[:, 0], None)                                      # knot = NULL: knot 0
    assert (fb == 1).all() and u.tobytes() == np.ascontiguousarray(s.U[:, 0]).tobytes()


@pytest.mark.parametrize("case", list(CASES))
def test_host_twin_writes_the_same_bytes(case, solved):
    s = solved(case)
    sv = s.sv
    for clamp in (False, True):
        for knot in (s.knot, None):
            x = s.x if knot is not None else s.X[:, 0] + (s.x - s.Xk)
            ud, fbd = policy(sv, x, knot, clamp)
            fbh = np.full(sv.B, -9, dtype=np.int32)
            uh = altro.eval_policy(sv, x, knot, clamp=clamp, fb=fbh)
            assert uh.tobytes() == ud.tobytes() and fbh.tobytes() == fbd.tobytes(), (clamp, knot is None)
    uh = altro.eval_policy(sv, s.x, s.knot)                                  # fb = NULL on the host twin
    assert uh.tobytes() == policy(sv, s.x, s.knot, True)[0].tobytes()


@pytest.mark.parametrize("case", BOTH_BACKENDS)
def test_clamp(case):
    """Per-instance rows of the BOX (altro_batch_set_bounds), tight enough that the perturbed policy leaves them for some
    controls and not for others: clamp = 1 is np.clip of clamp = 0 with the instance's row, byte for byte; and a row written
    through altro_batch_set_bounds_dev just before the call is the one that clamps."""
    prob, opts, _ = CASES[case]()
    sv = altro.ALTROSolver(prob, opts)
    try:
        B, n, m = sv.B, sv.n, sv.m
        rng = np.random.default_rng(9)
        ub = rng.uniform(0.4, 1.2, (B, m))
        zmin = np.concatenate([np.full((B, n), -np.inf), -ub], axis=1)
        zmax = np.concatenate([np.full((B, n), np.inf), 0.8 * ub], axis=1)
        altro.set_bounds(sv, 0, zmin, zmax)
        altro.solve(sv)
        X = altro.states(sv)
        outside = inside = 0
        for k in (0, 1, N - 2):
            x = X[:, k] + 5e-2 * (1.0 + np.abs(X[:, k])) * rng.standard_normal((B, n))
            u0, fb = policy(sv, x, np.full(B, k), clamp=False)
            u1, _ = policy(sv, x, np.full(B, k), clamp=True)
            assert (fb == 1).all()
            want = np.clip(u0, zmin[:, n:], zmax[:, n:])
            assert u1.tobytes() == want.tobytes(), k
            outside += int((want != u0).sum())
            inside += int((want == u0).sum())
        print(case, "controls clamped:", outside, "left alone:", inside)
        assert outside > 0 and inside > 0
        # a new row for instance 1 through the device setter, the call right behind it
        zmin2, zmax2 = zmin.copy(), zmax.copy()
        zmin2[1, n:], zmax2[1, n:] = -0.05, 0.04
        altro.set_bounds(sv, 0, T(zmin2), T(zmax2))
        u1, fb1 = policy(sv, X[:, 1], np.full(B, 1), clamp=True)
        u0, _ = policy(sv, X[:, 1], np.full(B, 1), clamp=False)
        assert altro.dev_refusals(sv) == 0
        assert (fb1 == 0).all()                                              # the setter dropped the gains: u0 is the nominal control
        assert u0.tobytes() == np.ascontiguousarray(altro.controls(sv)[:, 1]).tobytes()
        assert u1.tobytes() == np.clip(u0, zmin2[:, n:], zmax2[:, n:]).tobytes()
        assert (u1[1] != u0[1]).any() and (np.abs(u1[1]) <= 0.05).all()
    finally:
        sv.close()


@pytest.mark.parametrize("case", BOTH_BACKENDS)
def test_fb_life_cycle(case):
    prob, opts, _ = CASES[case]()
    sv = altro.ALTROSolver(prob, opts)
    try:
        B = sv.B
        rng = np.random.default_rng(11)
        knot = np.array([0, 1, N - 2, 1, 0][:B], dtype=np.int32)
        bi = np.arange(B)

        def look():
            X, U = altro.states(sv), altro.controls(sv)
            x = X[bi, knot] + 1e-2 * (1.0 + np.abs(X[bi, knot])) * rng.standard_normal((B, sv.n))
            u, fb = policy(sv, x, knot)
            return u, fb, U[bi, knot]

        u, fb, Uk = look()                                                   # before the first solve
        assert (fb == 0).all() and u.tobytes() == np.ascontiguousarray(Uk).tobytes()
        altro.solve(sv)
        u, fb, Uk = look()
        assert (fb == 1).all() and (u != Uk).any()
        altro.set_tracking_cost(sv, prob.obj.Q, prob.obj.R, prob.obj.Qf)     # the same weights: still drops the gains
        u, fb, Uk = look()
        assert (fb == 0).all() and u.tobytes() == np.ascontiguousarray(Uk).tobytes()
        altro.solve(sv)
        assert (look()[1] == 1).all()
        which = np.array([1, 0, 1, 0, 0][:B], dtype=np.int32)                # a strict subset
        api.restart_instances(sv, which, np.asarray(prob.U0))
        u, fb, Uk = look()
        assert np.array_equal(fb, 1 - which)
        assert u[which == 1].tobytes() == np.ascontiguousarray(Uk[which == 1]).tobytes()
        altro.solve(sv)
        assert (look()[1] == 1).all()
        active = np.ones(B, dtype=np.int32)                                  # a mask that leaves instance 0 out
        active[0] = 0
        api.set_active(sv, active)
        altro.set_tracking_cost(sv, prob.obj.Q, prob.obj.R, prob.obj.Qf)
        altro.solve(sv)
        u, fb, Uk = look()
        assert np.array_equal(fb, active)
        assert u[0].tobytes() == np.ascontiguousarray(Uk[0]).tobytes()
    finally:
        sv.close()


@pytest.mark.parametrize("case", BOTH_BACKENDS)
def test_out_of_range_knot(case, solved):
    s = solved(case)
    sv = s.sv
    B = sv.B
    knot = np.array([-1, 0, N - 1, 1, N - 2][:B], dtype=np.int32)
    okay = (knot >= 0) & (knot <= N - 2)
    valid = np.where(okay, knot, 0).astype(np.int32)
    x = s.X[np.arange(B), valid] + (s.x - s.Xk)
    want, _ = policy(sv, x, valid)
    u = torch.full((B, sv.m), 777.0, dtype=torch.float64, device=dev())
    fb = torch.full((B,), -9, dtype=torch.int32, device=dev())
    altro.eval_policy(sv, T(x), T(knot), clamp=False, out=u, fb=fb)
    u, fb = u.cpu().numpy(), fb.cpu().numpy()
    assert np.array_equal(fb, np.where(okay, 1, -1))
    assert (u[~okay] == 777.0).all()
    assert u[okay].tobytes() == want[okay].tobytes()
    assert altro.dev_refusals(sv) == 0
    with pytest.raises(altro.AltroError) as e:                               # the host twin checks on the host
        altro.eval_policy(sv, x, knot, clamp=False)
    assert e.value.code == INV
    assert altro.eval_policy(sv, x, valid, clamp=False).tobytes() == want.tobytes()


@pytest.mark.parametrize("case", BOTH_BACKENDS)
def test_refusals_launch_nothing(case, solved):
    """a host pointer, a u one element short, a NULL x: error 1 with a message, decided from the pointer's attributes before
    anything is enqueued; the next valid call writes what it wrote before"""
    s = solved(case)
    sv = s.sv
    L, B, n, m = sv._L, sv.B, sv.n, sv.m
    before, fb_before = policy(sv, s.x, s.knot)
    gp = lambda t: C.c_void_p(t.data_ptr())
    xt, kt = T(s.x), T(s.knot)
    ut = torch.zeros((B, m), dtype=torch.float64, device=dev())
    Kt = torch.zeros((B, N - 1, n, m), dtype=torch.float64, device=dev())
    host = np.zeros((B, max(n, m)))
    hp = C.c_void_p(host.ctypes.data)
    paths = altro._lib.hip_runtimes()
    assert len(paths) == 1, paths
    rt = C.CDLL(paths[0])
    rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    base, size = C.c_void_p(), C.c_size_t()
    assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), gp(ut)) == 0
    need = B * m * 8
    short = C.c_void_p(base.value + size.value - (need - 8))                 # the last B*m - 1 doubles of ut's allocation
    msgs = []
    for call in (lambda: L.altro_batch_eval_policy_dev(sv.h, hp, gp(kt), 0, gp(ut), None),
                 lambda: L.altro_batch_eval_policy_dev(sv.h, gp(xt), gp(kt), 0, hp, None),
                 lambda: L.altro_batch_eval_policy_dev(sv.h, gp(xt), gp(kt), 0, short, None),
                 lambda: L.altro_batch_eval_policy_dev(sv.h, None, gp(kt), 0, gp(ut), None),
                 lambda: L.altro_batch_eval_policy_dev(sv.h, gp(xt), hp, 0, gp(ut), None),
                 lambda: L.altro_batch_get_gains_dev(sv.h, hp, None),
                 lambda: L.altro_batch_get_gains_dev(sv.h, None, None)):
        rc = call()
        msg = (L.altro_last_error(sv.h) or b"").decode()
        assert rc == INV and msg, (rc, msg)
        msgs.append(msg)
    assert "shorter" in msgs[2]
    assert L.altro_batch_eval_policy_dev(None, gp(xt), None, 0, gp(ut), None) == INV and (L.altro_last_error(None) or b"").decode()
    assert L.altro_batch_eval_policy(sv.h, None, None, 0, None, None) == INV
    assert L.altro_batch_get_gains_dev(sv.h, gp(Kt), None) == 0              # d = NULL alone is fine
    after, fb_after = policy(sv, s.x, s.knot)
    assert after.tobytes() == before.tobytes() and fb_after.tobytes() == fb_before.tobytes()


def assert_gains_twins(sv, what):
    K, d = raw_gains(sv)
    Kt, dt = altro.get_gains_dev(sv)
    assert Kt.shape == (sv.B, sv.N - 1, sv.m, sv.n)
    assert Kt.transpose(-1, -2).contiguous().cpu().numpy().tobytes() == K.tobytes(), what
    assert dt.cpu().numpy().tobytes() == d.tobytes(), what
    only_d = torch.full_like(dt, np.nan)
    altro.get_gains_dev(sv, d=only_d)                                        # K = NULL
    assert only_d.cpu().numpy().tobytes() == d.tobytes(), what
    return K, d


@pytest.mark.parametrize("case", list(CASES))
def test_get_gains_dev_equals_get_gains(case, solved):
    s = solved(case)
    K, d = assert_gains_twins(s.sv, case)
    assert np.abs(K).max() > 0 and np.isfinite(K).all() and np.isfinite(d).all()


def test_get_gains_dev_after_a_confirmed_mpc_step():
    """(12, 4), default mode: MPC steps until some instance's solve ends with a costate-sweep confirmation (the confirm
    counter of that solve is nonzero: a confirmation is always a solve's last iteration), so the d = 0 branch is taken"""
    prob, opts, pb = random_linear(5, 12, 4, 56, steps=6)
    sv = altro.ALTROSolver(prob, opts)
    try:
        altro.solve(sv)
        assert_gains_twins(sv, "initial solve")
        found = False
        for i in range(6):
            x1 = altro.states(sv)[:, 1]
            altro.set_initial_state(sv, x1 + 0.01 * pb.noise[i] * np.abs(x1).max(axis=1, keepdims=True))
            altro.update_trajectory(sv, pb.Xtrack[:, i + 1:i + 1 + N], pb.Utrack[:, i + 1:i + N])
            altro.shift_fill(sv, True, True)
            altro.timing_reset(sv)
            altro.solve(sv)
            conf = altro.confirm_counter(sv)
            K, d = assert_gains_twins(sv, "step %d" % i)
            if (conf > 0).any():
                found = True
                assert (d[conf > 0] == 0.0).all()
                break
        assert found, "no solve of six MPC steps ended with a costate-sweep confirmation"
    finally:
        sv.close()


def test_stream_order_tick_then_policy():
    """ExternalMPC.tick followed at once by policy, nothing synchronised in between, gives the bytes of the same pair with a
    synchronise in between"""
    prob, opts, pb = random_linear(5, 12, 4, 57)
    a, b = altro.ALTROSolver(prob, opts), altro.ALTROSolver(prob, opts)
    try:
        altro.solve(a), altro.solve(b)
        rng = np.random.default_rng(13)
        x0 = T(prob.x0 + 0.05 * rng.standard_normal(prob.x0.shape))
        xm = T(prob.x0 + 0.1 * rng.standard_normal(prob.x0.shape))
        Xr, Ur = T(pb.Xtrack[:, 1:1 + N]), T(pb.Utrack[:, 1:N])
        la, lb = altro.ExternalMPC(a), altro.ExternalMPC(b)
        la.tick(x0, Xr, Ur)
        ua = la.policy(xm)
        lb.tick(x0, Xr, Ur)
        torch.cuda.synchronize()
        altro.synchronize(b)
        ub = lb.policy(xm)
        torch.cuda.synchronize()
        assert ua.cpu().numpy().tobytes() == ub.cpu().numpy().tobytes()
        assert ua.cpu().numpy().tobytes() != altro.controls(a)[:, 0].tobytes()    # (feedback was applied)
    finally:
        a.close(), b.close()


def test_two_rate_closed_loop_device_equals_host():
    """Five ticks of ExternalMPC on (12, 4), batch 5, with S = 4 policy substeps per tick against a torch plant
    x <- A_s x + B_s u (a fine-step model: A_s = I + (A - I) / S, B_s = B / S), once through the device calls and once through
    the host twins: identical final states, and every fb is 1."""
    B, n, m, S, ticks = 5, 12, 4, 4, 5
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=ticks + 1, seed=58)
    As = T(np.eye(n) + (pb.A - np.eye(n)) / S)
    Bs = T(pb.Bm / S)
    Xt, Ut = T(pb.Xtrack), T(pb.Utrack)

    def plant(x, u):
        return torch.bmm(As, x.unsqueeze(-1)).squeeze(-1) + torch.bmm(Bs, u.unsqueeze(-1)).squeeze(-1)

    hs, ds = (altro.ALTROSolver(mpc.gen_tracking_problem(pb), altro.SolverOptions(**mpc.REF_OPTS)) for _ in range(2))
    try:
        altro.solve(hs), altro.solve(ds)
        loop = altro.ExternalMPC(ds)
        rng = np.random.default_rng(14)
        xh = xd = T(pb.Xtrack[:, 0] + 0.05 * rng.standard_normal((B, n)))
        fbs = []
        for i in range(ticks):
            Xr, Ur = Xt[:, i + 1:i + 1 + N].contiguous(), Ut[:, i + 1:i + N].contiguous()
            loop.tick(xd, Xr, Ur)                                            # device: nothing below waits for the GPU
            fbd = torch.zeros((S, B), dtype=torch.int32, device=dev())
            for s in range(S):
                ud = altro.eval_policy(ds, xd, fb=fbd[s])
                xd = plant(xd, ud)
            fbs.append(fbd)
            altro.set_initial_state(hs, xh.cpu().numpy())                    # host twins
            altro.update_trajectory(hs, Xr.cpu().numpy(), Ur.cpu().numpy())
            altro.shift_fill(hs, True, True)
            altro.solve(hs)
            for s in range(S):
                fbh = np.zeros(B, dtype=np.int32)
                uh = altro.eval_policy(hs, xh.cpu().numpy(), fb=fbh)
                assert (fbh == 1).all(), (i, s)
                xh = plant(xh, T(uh))
        assert xd.cpu().numpy().tobytes() == xh.cpu().numpy().tobytes()
        assert all((f.cpu().numpy() == 1).all() for f in fbs)
        assert np.isfinite(xd.cpu().numpy()).all()
    finally:
        hs.close(), ds.close()
