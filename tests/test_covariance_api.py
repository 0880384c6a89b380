"""Closed-loop covariance of the stored policy (altro_batch_propagate_covariance / _dev), the part that needs no GPU: the two
entry points are declared in the header, exported by the built library with 14 arguments, bound by the ctypes layer and named in
INTEGRATION.md's Julia shim; the Python wrappers send GPU tensors to the device form and numpy to the host twin and refuse what
they would have to convert; and the numpy yardstick (tests/covariance_ref.py) means what it says: with the oracle's gains on an
unconstrained LQ problem its matrices are the outer products of the deviations simulate_ref's unclamped closed loop produces,
and its dJ is the mean cost excess of a sampled simulate_ref study."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

import covariance_ref as CR
import evaluate_ref as ER
import simulate_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["altro_batch_propagate_covariance_dev", "altro_batch_propagate_covariance"]
U_ = 2.0 ** -53


def test_header_declares_both_functions():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "altro_batch.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(\s*altro_handle\s*\*\s*h\s*,\s*const\s+double\s*\*\s*Sigma0\s*,\s*const\s+double\s*\*\s*W\s*,"
                         r"\s*int32_t\s+per_instance\s*,\s*int32_t\s+con_id\s*,\s*double\s+kappa\b" % s, hdr), s


def test_header_comment_cites_the_reference_noise_models():
    hdr = open(os.path.join(ROOT, "include", "altro_batch.h")).read()
    blk = hdr[hdr.index("closed-loop covariance of the stored policy"):hdr.index("altro_batch_propagate_covariance(altro_handle")]
    for cite in ("random_linear_problem.jl:129", "simple_rocket.jl:65-71", "flexible_sat_mpc.jl:266"):
        assert cite in blk, cite


def test_built_library_exports_them():
    altro._lib.build()
    L = altro._lib.lib()
    for s in NEW:
        assert hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == 14 and getattr(L, s).restype is not None, s


def test_lib_exports_lists_them():
    for s in NEW:
        assert s in altro._lib.EXPORTS, s


def test_integration_doc_names_them():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert (":" + s) in doc, s


def test_package_exposes_the_wrappers():
    assert callable(altro.propagate_covariance) and altro.propagate_covariance is api.propagate_covariance
    assert callable(altro.ExternalMPC.covariance)


# ---------------------------------------------------------------------------------------------- wrapper validation
def fake(shape, dtype="torch.float64", strides=None, dev=("cuda", 0)):
    """stand-in with the four things the validation looks at"""
    st = api._dense_strides(shape) if strides is None else tuple(strides)
    return NS(shape=tuple(shape), dtype=dtype, stride=lambda: st, device=NS(type=dev[0], index=dev[1]), data_ptr=lambda: 4096)


def stand_in_solver(calls, B=3, n=2, m=1, N=4):
    """B 3, n 2, m 1, N 4; constraint 0 a BOX on knots 1 .. 3, constraint 1 two LINEAR rows on knots 2 .. 4 (library ids 7, 9)"""
    rec = lambda name: (lambda *a: calls.append((name,) + a) or 0)
    L = NS(**{k: rec(k) for k in NEW})
    items = [(altro.BoundConstraint(n, m, u_min=-np.ones(m), u_max=np.ones(m)), 1, 3),
             (altro.LinearConstraint(np.ones((2, n + m)), np.zeros(2)), 2, 4)]
    return NS(B=B, n=n, m=m, N=N, h=None, device=0, _L=L, _chk=lambda rc: None, prob=NS(constraints=NS(items=items)), con_ids=[7, 9])


def test_device_form_validates_every_tensor_before_the_library_sees_it():
    calls = []
    sv = stand_in_solver(calls)
    i32 = "torch.int32"
    S0, W = fake((3, 2, 2)), fake((3, 2, 2))
    out = dict(sx=fake((3, 4, 2)), su=fake((3, 3, 1)), sc=fake((3, 3, 2)), dJ=fake((3,)), fb=fake((3,), dtype=i32), zmin_t=fake((3, 3)),
               zmax_t=fake((3, 3)), Sout=fake((3, 4, 2, 2)))
    good = dict(Sigma0=S0, W=W, con_id=1, kappa=2.0, out=out)
    sub = lambda **kw: dict(out, **kw)
    less = lambda *names: {k: v for k, v in out.items() if k not in names}
    bad = [dict(Sigma0=None, W=None), dict(Sigma0=fake((2, 2))), dict(Sigma0=fake((3, 2, 3))), dict(W=fake((2, 2, 2))),
           dict(Sigma0=fake((3, 2, 2), dtype="torch.float32")), dict(W=fake((3, 2, 2), strides=(4, 1, 2))), dict(W=fake((3, 2, 2), dev=("cuda", 1))),
           dict(Sigma0=fake((3, 2, 2), dev=("cpu", None))),
           dict(con_id=0), dict(con_id=2), dict(con_id=-1), dict(con_id=0.5), dict(con_id=None), dict(kappa=-1.0), dict(kappa=float("nan")),
           dict(kappa=float("inf")), dict(kappa=None),
           dict(out={}), dict(out=(out["sx"],)), dict(out=sub(sx=None)), dict(out=sub(J=fake((3,)))), dict(out=less("zmin_t")),
           dict(out=less("zmax_t")), dict(out=less("sc")),
           dict(out=sub(sx=fake((3, 3, 2)))), dict(out=sub(su=fake((3, 3, 2)))), dict(out=sub(sc=fake((3, 2, 2)))), dict(out=sub(sc=fake((3, 3, 1)))),
           dict(out=sub(dJ=fake((3, 1)))), dict(out=sub(dJ=fake((3,), dtype=i32))), dict(out=sub(fb=fake((3,)))), dict(out=sub(fb=fake((4,), dtype=i32))),
           dict(out=sub(zmin_t=fake((3, 2)))), dict(out=sub(zmax_t=fake((3,)))), dict(out=sub(Sout=fake((3, 4, 2, 2), strides=(16, 4, 1, 2)))),
           dict(out=sub(Sout=fake((3, 3, 2, 2)))), dict(out=sub(sx=fake((3, 4, 2), dev=("cuda", 1)))), dict(out=sub(su=fake((3, 3, 1), dtype="torch.float32")))]
    for b in bad:
        args = dict(good)
        args.update(b)
        with pytest.raises(ValueError):
            api._propagate_covariance_dev(sv, **args)
    assert calls == []
    assert api._propagate_covariance_dev(sv, **good) is out
    only = dict(dJ=out["dJ"])
    assert api._propagate_covariance_dev(sv, None, fake((2, 2)), out=only) is only           # one shared W, no Sigma0, dJ alone
    assert api._propagate_covariance_dev(sv, fake((2, 2)), None, kappa=0.0, out=less("sc")) is not None
    assert [c[0] for c in calls] == [NEW[0]] * 3
    assert [c[4:7] for c in calls] == [(1, 9, 2.0), (0, -1, 0.0), (0, -1, 0.0)]            # per_instance, library id, kappa
    assert all(a is not None for a in calls[0][2:4] + calls[0][7:15]) and len(calls[0]) == 15
    assert calls[1][2] is None and calls[1][3] is not None and [a is not None for a in calls[1][7:15]] == [False] * 3 + [True] + [False] * 4
    assert calls[2][3] is None and calls[2][9] is None and calls[2][12] is not None and calls[2][13] is not None


def test_numpy_takes_the_host_twin():
    calls = []
    sv = stand_in_solver(calls)
    r = api.propagate_covariance(sv, Sigma0=np.eye(2))
    assert sorted(r) == ["dJ", "fb", "su", "sx"] and r["sx"].shape == (3, 4, 2) and r["fb"].dtype == np.int32 and r["dJ"].dtype == np.float64
    r = altro.ExternalMPC(sv).covariance(W=np.zeros((3, 2, 2)), con_id=1, kappa=3.0)
    assert sorted(r) == ["dJ", "fb", "sc", "su", "sx", "zmax_t", "zmin_t"] and r["sc"].shape == (3, 3, 2) and r["zmin_t"].shape == (3, 3)
    So = np.zeros((3, 4, 2, 2))
    assert api.propagate_covariance(sv, np.eye(2), np.eye(2), out=dict(Sout=So))["Sout"] is So
    assert [c[0] for c in calls] == [NEW[1]] * 3 and [c[4:7] for c in calls] == [(0, -1, 0.0), (1, 9, 3.0), (0, -1, 0.0)]
    assert calls[0][3] is None and calls[1][2] is None and calls[2][14] is not None and all(a is None for a in calls[2][7:14])
    for kw in (dict(), dict(Sigma0=np.eye(3)), dict(Sigma0=np.eye(2), W=np.zeros((3, 2, 2))), dict(Sigma0=np.eye(2, dtype=np.float32)),
               dict(Sigma0=np.zeros((2, 4))[:, ::2]), dict(Sigma0=[[1.0, 0.0], [0.0, 1.0]]), dict(Sigma0=np.eye(2), con_id=0),
               dict(Sigma0=np.eye(2), kappa=-0.5), dict(Sigma0=np.eye(2), out=dict(sx=np.zeros((3, 4, 2), dtype=np.float32))),
               dict(Sigma0=np.eye(2), out=dict(fb=np.zeros(3))), dict(Sigma0=np.eye(2), out=dict(sc=np.zeros((3, 3, 2)))),
               dict(Sigma0=np.eye(2), out=dict(zmin_t=np.zeros((3, 3)), zmax_t=np.zeros((3, 3)))),
               dict(Sigma0=np.eye(2), out=dict(Sout=np.zeros((3, 4, 2, 2))[..., ::-1])), dict(Sigma0=np.eye(2), out=dict(sx=fake((3, 4, 2))))):
        with pytest.raises(ValueError):
            api.propagate_covariance(sv, **kw)
    assert len(calls) == 3


# ---------------------------------------------------------------------------------------------- the yardstick
def lq_with_oracle_gains(oracle):
    """the unconstrained random-linear problem of test_simulate_api.py (n = 4, m = 2, N = 9) solved by the oracle:
    (case, K (1, N-1, m, n), Xbar (1, N, n), Ubar (1, N-1, m))"""
    cs = ER.make_case(1, 4, 2, 9, seed=41)
    s = ER.oracle_of(oracle, cs, 0)
    s.solve()
    K, _ = s.gains()
    return cs, np.asarray(K)[None], s.states()[None], s.controls()[None]


def test_yardstick_rank_one_is_the_simulated_deviation(oracle):
    """Sigma0 = v v', W = 0: S_k is the outer product of d_k = x_k - xbar_k of simulate_ref's unclamped closed loop started at
    xbar_0 + v.  Both sides are float64.  Bound: one step of either recursion is sums of at most n + m products, relative error
    <= (n + m + 2) u of the absolute sums, and errors made earlier are carried through at most N - 1 steps, each multiplying them
    by at most g_k = max(1, |M_k|_1 |M_k|_inf); the deviation is a difference of states of size |x|, so it carries u |x| too:
    |S_k - d_k d_k'| <= 4 N (n + m + 2) u G (max |S_k| + 2 max |x_k| max |d_k|),  G = prod_k g_k"""
    cs, K, Xbar, Ubar = lq_with_oracle_gains(oracle)
    n, m, N = cs.n, cs.m, cs.N
    v = 0.5 * np.random.default_rng(7).standard_normal(n)
    X, _ = SR.closed_loop(cs, K, Xbar, Ubar, (Xbar[:, 0] + v)[:, None])
    D = X[:, 0] - Xbar
    r = CR.propagate(cs, K, Sigma0=np.outer(v, v))
    G = 1.0
    worst = 0.0
    for k in range(N):
        outer = np.einsum("bi,bj->bij", D[:, k], D[:, k])
        bound = 4 * N * (n + m + 2) * U_ * G * (np.abs(r.S[:, k]).max() + 2 * np.abs(X[:, 0, k]).max() * np.abs(D[:, k]).max())
        err = np.abs(r.S[:, k] - outer).max()
        worst = max(worst, err / bound)
        assert err <= bound, (k, err, bound)
        assert np.abs(r.sx[:, k] - np.abs(D[:, k])).max() <= np.sqrt(bound) if k else np.array_equal(r.sx[:, 0], np.abs(v)[None])
        if k < N - 1:
            Mk = cs.A[0, k] + cs.Bm[0, k] @ K[0, k]
            G *= max(1.0, np.abs(Mk).sum(axis=0).max() * np.abs(Mk).sum(axis=1).max())
    print("rank one: worst error / bound", worst, "growth", G)
    assert np.abs(D[:, -1]).max() > 1e-3          # (the deviation has not died out: the comparison says something to the end)


SAMPLES = 20000


def test_yardstick_dJ_is_the_mean_cost_excess_of_a_sampled_study(oracle):
    """SAMPLES = 20000 draws x_0 ~ N(xbar_0, Sigma0), w_k ~ N(0, W) through simulate_ref (unclamped): the mean of
    J(sample) - J(nominal) equals dJ within the study's own standard error (sample standard deviation / sqrt(SAMPLES)); one
    fixed seed, so the comparison is deterministic"""
    cs, K, Xbar, Ubar = lq_with_oracle_gains(oracle)
    n, N = cs.n, cs.N
    rng = np.random.default_rng(20260)
    L0, Lw = 0.3 * rng.standard_normal((n, n)), 0.05 * rng.standard_normal((n, n))
    S0, W = L0 @ L0.T, Lw @ Lw.T
    x0 = Xbar[:, 0][:, None] + rng.standard_normal((1, SAMPLES, n)) @ L0.T
    w = rng.standard_normal((1, SAMPLES, N - 1, n)) @ Lw.T
    J = SR.simulate(cs, K, Xbar, Ubar, x0, w)[0][0]
    J0 = ER.cost(cs, Xbar[:, None], Ubar[:, None])[0][0, 0]
    excess = J - J0
    se = excess.std(ddof=1) / np.sqrt(SAMPLES)
    dJ = CR.propagate(cs, K, Sigma0=S0, W=W).dJ[0]
    print("dJ", dJ, "study mean", excess.mean(), "standard error", se, "distance / se", abs(excess.mean() - dJ) / se)
    assert dJ > 0 and abs(excess.mean() - dJ) <= se
