"""The quadratic cost-to-go of the stored policy (altro_batch_cost_to_go / _dev), the part that needs no GPU: the
numpy yardstick (tests/cost_to_go_ref.py) means what it says -- with the gains of a dense Riccati recursion its P_k are the
Riccati matrices and its p_k the costates, its quadratic model is the cost of simulate_ref's unclamped closed loop, and its
matrices give covariance_ref's dJ by the trace formula -- the two entry points are declared, exported, bound and named in the Julia
shim, and the Python wrappers send GPU tensors to the device form and numpy to the host twin and refuse what they would have to
convert.

The rule of the first three tests (both sides numpy): per instance, max |a - ref| / max |ref| of the float64 computation `a` of
one side against the long-double computation `ref` of the OTHER side is at most 16 x max(the error of the float64 computation of
that other side against the same ref, 2^-52)."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

import cost_to_go_ref as CT
import covariance_ref as CR
import evaluate_ref as ER
import simulate_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["altro_batch_cost_to_go_dev", "altro_batch_cost_to_go"]
LD = np.longdouble
EPS = 2.0 ** -52


def held(a, ref, y64, what):
    err, e64 = CR.rel_err(a, ref), CR.rel_err(y64, ref)
    bound = 16 * np.maximum(e64, EPS)
    print("%-22s err %.2e  float64 yardstick %.2e  err/bound %.3f" % (what, err.max(), e64.max(), (err / bound).max()))
    assert (err <= bound).all(), (what, err, bound)


# ---------------------------------------------------------------------------------------------- the yardstick
def riccati(cs, dtype):
    """the dense Riccati recursion of the unconstrained tracking problem in absolute coordinates, V_k(x) = x'S_k x / 2 + s_k'x + c:
    (K (B, N-1, m, n), d (B, N-1, m), S (B, N, n, n), s (B, N, n))"""
    t = lambda a: np.asarray(a, dtype=dtype)
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    A, Bm, f = t(cs.A), t(cs.Bm), t(cs.f)
    dt = dtype(cs.dt)
    Wx, Wu, Wf = dt * t(cs.Q), dt * t(cs.R), t(cs.Qf)
    Xr, Ur = t(cs.Xref), t(cs.Uref)
    K, d = np.zeros((B, N - 1, m, n), dtype=dtype), np.zeros((B, N - 1, m), dtype=dtype)
    S, s = np.zeros((B, N, n, n), dtype=dtype), np.zeros((B, N, n), dtype=dtype)
    for b in range(B):
        S[b, -1], s[b, -1] = np.diag(Wf[b]), -Wf[b] * Xr[b, -1]
        for k in range(N - 2, -1, -1):
            a, bm = A[b, k], Bm[b, k]
            g = S[b, k + 1] @ f[b, k] + s[b, k + 1]
            Qxx, Quu, Qux = np.diag(Wx[b]) + a.T @ S[b, k + 1] @ a, np.diag(Wu[b]) + bm.T @ S[b, k + 1] @ bm, bm.T @ S[b, k + 1] @ a
            qx, qu = -Wx[b] * Xr[b, k] + a.T @ g, -Wu[b] * Ur[b, k] + bm.T @ g
            L = np.linalg.cholesky(Quu.astype(np.float64)).astype(dtype)      # (a start; two refinements in `dtype` below)
            sol = lambda r: np.linalg.solve(L.T.astype(np.float64), np.linalg.solve(L.astype(np.float64), r.astype(np.float64))).astype(dtype)
            KK, dd = -sol(Qux), -sol(qu)
            for _ in range(3):
                KK, dd = KK - sol(Quu @ KK + Qux), dd - sol(Quu @ dd + qu)
            K[b, k], d[b, k] = KK, dd
            S[b, k] = Qxx + Qux.T @ KK
            s[b, k] = qx + Qux.T @ dd
    return K, d, S, s


def optimal_loop(cs, K, d, dtype):
    t = lambda a: np.asarray(a, dtype=dtype)
    A, Bm, f = t(cs.A), t(cs.Bm), t(cs.f)
    X, U = np.zeros((cs.B, cs.N, cs.n), dtype=dtype), np.zeros((cs.B, cs.N - 1, cs.m), dtype=dtype)
    X[:, 0] = t(cs.x0)
    for k in range(cs.N - 1):
        U[:, k] = np.einsum("baj,bj->ba", K[:, k], X[:, k]) + d[:, k]
        X[:, k + 1] = np.einsum("bij,bj->bi", A[:, k], X[:, k]) + np.einsum("bij,bj->bi", Bm[:, k], U[:, k]) + f[:, k]
    return X, U


def test_with_riccati_gains_the_yardstick_is_the_riccati_recursion():
    """1: P_k = S_k and p_k = S_k xbar_k + s_k, the gradient of the optimal cost-to-go at the optimal trajectory"""
    cs = ER.make_case(3, 5, 2, 8, seed=61, per_knot_dyn=True, per_instance_cost=True)
    Kl, dl, Sl, sl = riccati(cs, LD)
    Xl, Ul = optimal_loop(cs, Kl, dl, LD)
    K, X, U = Kl.astype(np.float64), Xl.astype(np.float64), Ul.astype(np.float64)
    _, _, S64, s64 = riccati(cs, np.float64)
    got, gl = CT.cost_to_go(cs, K, X, U), CT.cost_to_go(cs, K, X, U, dtype=LD)
    grad = lambda S, s, Xb: np.einsum("bkij,bkj->bki", S, np.asarray(Xb, dtype=S.dtype)) + s
    held(got.P, Sl, S64, "P against Riccati")
    held(got.p, grad(Sl, sl, Xl), grad(S64, s64, X), "p against costate")
    # and the matrices the other way round: the Riccati recursion in float64 against the yardstick in long double.  (Not the
    # costates: S_k xbar_k + s_k in absolute coordinates is a cancelling sum, the local recursion of p_k is not, so the Riccati
    # side is the less accurate one and is the `other side` of the rule only.)
    held(S64, gl.P, got.P, "Riccati against P")
    assert (np.abs(got.p).max(axis=(1, 2)) > 1e-2).all()


def loop_case(seed):
    """a case, gains that are nobody's optimum and a trajectory that is a rollout: the identities hold for every policy"""
    cs = ER.make_case(3, 6, 3, 7, seed=seed, per_knot_dyn=True, per_instance_cost=True)
    rng = np.random.default_rng(seed + 1)
    K = -0.3 * rng.standard_normal((cs.B, cs.N - 1, cs.m, cs.n))
    U = 0.3 * rng.standard_normal((cs.B, cs.N - 1, cs.m))
    X = ER.rollout(cs, U[:, None])[:, 0]
    return cs, K, X, U


def test_quadratic_model_is_the_cost_of_the_simulated_loop():
    """2: J of simulate_ref's unclamped closed loop from xbar_0 + d, |d| ~ 0.3, equals v_0 + p_0'd + d'P_0 d / 2; v_0 is J of the
    held trajectory"""
    cs, K, X, U = loop_case(63)
    d = 0.3 * np.random.default_rng(65).standard_normal((cs.B, cs.n))
    J = SR.simulate(cs, K, X, U, x0=(X[:, 0] + d)[:, None])[0][:, 0]
    J0 = ER.cost(cs, X[:, None], U[:, None])[0][:, 0]
    c64, cl = CT.cost_to_go(cs, K, X, U), CT.cost_to_go(cs, K, X, U, dtype=LD)
    held(J, CT.quadratic(cl, d, LD), CT.quadratic(c64, d), "J against the model")
    held(J0, cl.v[:, 0], c64.v[:, 0], "J of the trajectory held")
    assert (np.abs(J - J0) > 1e-3 * J0).all()


def test_trace_formula_is_covariance_refs_dJ():
    """3: dJ of covariance_ref equals <P_0, Sigma0> / 2 + sum_{k=1..N-1} <P_k, W> / 2, per instance and shared matrices"""
    cs, K, X, U = loop_case(67)
    rng = np.random.default_rng(69)
    for lead in ((), (cs.B,)):
        L0, Lw = 0.2 * rng.standard_normal(lead + (cs.n, cs.n)), 0.05 * rng.standard_normal(lead + (cs.n, cs.n))
        S0, W = L0 @ np.swapaxes(L0, -1, -2), Lw @ np.swapaxes(Lw, -1, -2)
        for a, w in ((S0, W), (S0, None), (None, W)):
            c64, cl = CT.cost_to_go(cs, K, X, U), CT.cost_to_go(cs, K, X, U, dtype=LD)
            dJ = CR.propagate(cs, K, a, w).dJ
            held(dJ, CT.trace_formula(cl.P, a, w, LD), CT.trace_formula(c64.P, a, w), "dJ against the traces")
            held(CT.trace_formula(c64.P, a, w), CR.propagate(cs, K, a, w, dtype=LD).dJ, dJ, "traces against dJ")


def test_mode_1_with_an_empty_set_and_zero_duals_is_mode_0():
    cs, K, X, U = loop_case(71)
    ER.add_box(cs, 50.0)
    codes = np.zeros((cs.B, cs.N, cs.n + cs.m), dtype=np.uint8)
    duals = np.zeros((cs.B, cs.N - 1, 2, cs.n + cs.m))
    a = CT.cost_to_go(cs, K, X, U)
    b = CT.cost_to_go(cs, K, X, U, 1, codes, np.full(cs.B, 10.0), duals, np.full(cs.B, 10.0))
    for k in ("P", "p", "v"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    codes[:, 2, cs.n] = 1
    c = CT.cost_to_go(cs, K, X, U, 1, codes, np.full(cs.B, 10.0), duals, np.full(cs.B, 10.0))
    assert np.array_equal(c.P[:, 3:], a.P[:, 3:]) and not np.array_equal(c.P[:, 2], a.P[:, 2]) and np.array_equal(c.v, a.v)


# ---------------------------------------------------------------------------------------------- declarations
def test_header_declares_both_functions_and_the_struct():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "altro_batch.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(\s*altro_handle\s*\*\s*h\s*,\s*int32_t\s+mode\s*,\s*const\s+altro_ctg_out\s*\*\s*out\s*,"
                         r"\s*int32_t\s*\*\s*fb\s*\)\s*;" % s, hdr), s
    body = hdr[hdr.index("typedef struct altro_ctg_out {"):hdr.index("} altro_ctg_out;")]
    assert re.findall(r"\*(\w+)", body) == list(altro._lib.CTG_OUT_FIELDS) == [f for f, _ in altro._lib.CtgOut._fields_]


def test_built_library_exports_them():
    altro._lib.build()
    L = altro._lib.lib()
    for s in NEW:
        assert s in altro._lib.EXPORTS and hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == 4, s
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert (":" + s) in doc, s
    assert L.altro_batch_cost_to_go(None, 0, None, None) == altro._lib.ERR_INVALID_ARG
    assert L.altro_batch_cost_to_go_dev(None, 0, None, None) == altro._lib.ERR_INVALID_ARG
    assert (L.altro_last_error(None) or b"").decode()


def test_package_exposes_the_wrappers():
    assert callable(altro.cost_to_go) and altro.cost_to_go is api.cost_to_go
    assert callable(altro.ExternalMPC.cost_to_go)


# ---------------------------------------------------------------------------------------------- wrapper validation
def fake(shape, dtype="torch.float64", strides=None, dev=("cuda", 0)):
    """stand-in with the four things the validation looks at"""
    st = api._dense_strides(shape) if strides is None else tuple(strides)
    return NS(shape=tuple(shape), dtype=dtype, stride=lambda: st, device=NS(type=dev[0], index=dev[1]), data_ptr=lambda: 4096)


def stand_in_solver(calls, B=3, n=2, m=1, N=4):
    def rec(name):
        def f(h, mode, st, fb):
            o = st._obj
            calls.append((name, mode, {k: getattr(o, k) for k in altro._lib.CTG_OUT_FIELDS}, fb))
            return 0
        return f
    return NS(B=B, n=n, m=m, N=N, h=None, device=0, _L=NS(**{k: rec(k) for k in NEW}), _chk=lambda rc: None)


def test_device_form_validates_every_tensor_before_the_library_sees_it():
    calls = []
    sv = stand_in_solver(calls)
    i32 = "torch.int32"
    out = dict(P0=fake((3, 2, 2)), p0=fake((3, 2)), v0=fake((3,)), P=fake((3, 4, 2, 2)), p=fake((3, 4, 2)), v=fake((3, 4)), fb=fake((3,), dtype=i32))
    sub = lambda **kw: dict(out, **kw)
    bad = [dict(), dict(fb=out["fb"]), dict(J=fake((3,))), sub(S=fake((3,))), "P0", (1, 2), sub(P0=fake((3, 2, 3))), sub(P0=fake((2, 2))),
           sub(P0=fake((3, 2, 2), strides=(4, 1, 2))), sub(p0=fake((3, 2), dtype="torch.float32")), sub(v0=fake((3, 1))), sub(v0=fake((3,), dtype=i32)),
           sub(P=fake((3, 3, 2, 2))), sub(P=fake((3, 4, 2, 2), strides=(16, 4, 1, 2))), sub(p=fake((3, 4, 2), dev=("cuda", 1))),
           sub(v=fake((3, 4), dev=("cpu", None))), sub(v=fake((4, 3))), sub(fb=fake((3,))), sub(fb=fake((4,), dtype=i32))]
    for b in bad:
        with pytest.raises(ValueError):
            api._cost_to_go_dev(sv, False, b)
    assert calls == []
    assert api._cost_to_go_dev(sv, True, out) == out
    only = dict(v=out["v"])
    assert api._cost_to_go_dev(sv, False, only) == only
    assert [(c[0], c[1]) for c in calls] == [(NEW[0], 1), (NEW[0], 0)]
    assert all(calls[0][2][k] == 4096 for k in altro._lib.CTG_OUT_FIELDS) and calls[0][3] is not None
    assert [calls[1][2][k] for k in altro._lib.CTG_OUT_FIELDS] == [None] * 5 + [4096] and calls[1][3] is None


def test_numpy_takes_the_host_twin_and_a_mix_is_refused():
    calls = []
    sv = stand_in_solver(calls)
    r = api.cost_to_go(sv)
    assert list(r) == ["P0", "p0", "v0", "fb"] and r["P0"].shape == (3, 2, 2) and r["p0"].shape == (3, 2) and r["v0"].shape == (3,)
    assert r["fb"].dtype == np.int32 and r["P0"].dtype == np.float64
    r = altro.ExternalMPC(sv).cost_to_go(penalty=True, out=("P", "v"))
    assert list(r) == ["P", "v"] and r["P"].shape == (3, 4, 2, 2) and r["v"].shape == (3, 4)
    Pn, fb = np.zeros((3, 4, 2, 2)), np.zeros(3, dtype=np.int32)
    r = api.cost_to_go(sv, out=dict(P=Pn, fb=fb, p0=None))
    assert r["P"] is Pn and r["fb"] is fb and r["p0"].shape == (3, 2)
    assert [(c[0], c[1]) for c in calls] == [(NEW[1], 0), (NEW[1], 1), (NEW[1], 0)]
    assert [k for k, a in calls[0][2].items() if a] == ["P0", "p0", "v0"] and calls[0][3] is not None
    assert [k for k, a in calls[1][2].items() if a] == ["P", "v"] and calls[1][3] is None
    assert calls[2][2]["P"] == Pn.ctypes.data and [k for k, a in calls[2][2].items() if a] == ["p0", "P"]
    meta = lambda *s: torch.empty(s, dtype=torch.float64, device="meta")      # (a tensor that is not in host memory)
    for o in (dict(P0=np.zeros((3, 2, 2)), p0=meta(3, 2)), dict(P0=meta(3, 2, 2), fb=fb), dict(P0=np.zeros((3, 2, 2), dtype=np.float32)),
              dict(P0=np.zeros((3, 2, 3))), dict(P=np.zeros((3, 4, 2, 2))[..., ::-1]), dict(p0=[[0.0, 0.0]] * 3), dict(fb=np.zeros(3)),
              dict(fb=np.zeros(3, dtype=np.int32)), dict(P0=torch.zeros((3, 2, 2), dtype=torch.float64)), dict(P0=fake((3, 2, 2))), ("P0", "S"), "v0", ()):
        with pytest.raises(ValueError):
            api.cost_to_go(sv, out=o)
    assert len(calls) == 3
