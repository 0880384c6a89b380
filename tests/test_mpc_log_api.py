"""CPU tests of the per-step MPC log (altro_mpc_set_log / altro_mpc_get_log): the exports and their refusals without a
handle, the record object and the X_traj helper on synthetic arrays, and the benchmark functions' result assembly from a
log against the per-step assembly of the same numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import benchmarks as Bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    altro._lib.build()
    return altro._lib.lib()


def test_log_exports_are_declared_bound_and_refuse_a_null_handle(lib):
    txt = open(os.path.join(ROOT, "include", "altro_batch.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("altro_mpc_set_log", "altro_mpc_get_log"):
        assert name in altro._lib.EXPORTS
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name)
    assert lib.altro_mpc_set_log(None, 8) == altro._lib.ERR_INVALID_ARG
    assert lib.altro_mpc_set_log(None, -1) == altro._lib.ERR_INVALID_ARG
    x = np.zeros(4)
    i = np.zeros(4, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    assert lib.altro_mpc_get_log(None, 0, 1, altro.api._p(x), altro.api._p(x), i.ctypes.data_as(ip), i.ctypes.data_as(ip),
                                 i.ctypes.data_as(ip), altro.api._p(x), altro.api._p(x)) == altro._lib.ERR_INVALID_ARG
    assert lib.altro_mpc_get_log(None, 0, 1, None, None, None, None, None, None, None) == altro._lib.ERR_INVALID_ARG


def synthetic_log(S=5, B=3, n=4, m=2, first=2, seed=0):
    rng = np.random.default_rng(seed)
    it = rng.integers(1, 9, (S, B)).astype(np.int32)
    st = np.where(rng.random((S, B)) < 0.8, altro.SOLVE_SUCCEEDED, 3).astype(np.int32)
    return altro.MPCLog(first, rng.standard_normal((S, B, n)), rng.standard_normal((S, B, m)), it,
                        np.ones((S, B), dtype=np.int32), st, rng.random((S, B)), rng.random((S, B)))


def test_record_object_and_x_traj_helper():
    S, B, n, m = 5, 3, 4, 2
    lg = synthetic_log(S, B, n, m)
    assert lg.steps == S and lg.first == 2
    assert lg.x0.shape == (S, B, n) and lg.u0.shape == (S, B, m)
    for a in (lg.iterations, lg.iterations_outer, lg.status):
        assert a.shape == (S, B) and a.dtype == np.int32
    for a in (lg.x0, lg.u0, lg.cost, lg.c_max):
        assert a.dtype == np.float64
    assert lg.solve_succeeded.dtype == bool and np.array_equal(lg.solve_succeeded, lg.status == 1)
    xs = np.arange(B * n, dtype=np.float64).reshape(B, n)
    X = lg.x_traj(xs)
    assert X.shape == (S + 1, B, n) and X.dtype == np.float64
    assert np.array_equal(X[0], xs)
    for s in range(S):                                  # step-major: row s + 1 is x0 of step first + s
        assert np.array_equal(X[s + 1], lg.x0[s])
    assert np.array_equal(altro.x_traj(xs, lg), X)
    with pytest.raises(ValueError):
        lg.x_traj(np.zeros((B, n + 1)))
    with pytest.raises(ValueError):
        lg.x_traj(np.zeros((B + 1, n)))


@pytest.mark.parametrize("S,K", [(12, 4), (10, 4), (7, 7), (5, 8)])
def test_benchmark_result_from_a_log_equals_the_per_step_assembly(S, K):
    B = 6
    lg = synthetic_log(S, B, first=0, seed=S)
    # the per-step path: one stats read per step (benchmarks.run_random_linear with launch_steps = 1)
    t1, it, ok = [], [], []
    for s in range(S):
        t1.append(0.5 + s); it.append(lg.iterations[s].copy()); ok.append(lg.status[s] == altro.SOLVE_SUCCEEDED)
    per_step = Bm._result(t1, it, ok, B)
    nl = (S + K - 1) // K
    tl = [2.0 + l for l in range(nl)]
    fused = Bm._result_from_log(tl, lg, B, K)
    assert np.array_equal(fused["iter"], per_step["iter"]) and fused["iter"].shape == (S, B)
    assert np.array_equal(fused["solve_succeeded"], per_step["solve_succeeded"])
    assert fused["batch"] == per_step["batch"] == B
    assert fused["launch_steps"] == K and "launch_steps" not in per_step
    assert fused["time"].shape == (nl,) and np.array_equal(fused["time"], np.asarray(tl))      # one entry per launch
    in_launch = np.array([min(K, S - f) for f in range(0, S, K)])
    assert in_launch.sum() == S
    assert np.allclose(fused["time_us_per_solve"], 1e3 * np.asarray(tl) / (B * in_launch), rtol=1e-15)
    a, b = Bm.summarise(fused), Bm.summarise(per_step)
    for k in ("batch", "steps", "iterations_median", "iterations_mean", "iterations_max", "solve_succeeded_frac"):
        assert a[k] == b[k], k
    assert a["launch_steps"] == K and "launch_steps" not in b
    assert a["ms_per_step_median"] == pytest.approx(np.median(np.asarray(tl) / in_launch), rel=1e-12)
