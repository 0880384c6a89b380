"""Trajectories scored on the device (altro_batch_evaluate / _dev), the part that needs no GPU: the two entry points are declared
in the header, exported by the built library, bound by the ctypes layer and named in INTEGRATION.md's Julia shim; the Python
wrappers send GPU tensors to the device form and numpy to the host twin and refuse what they would have to convert; and the
numpy yardstick the GPU tests hold the device to (tests/evaluate_ref.py) is itself compared with the CPU oracle."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

import evaluate_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["altro_batch_evaluate_dev", "altro_batch_evaluate"]


def test_header_declares_both_functions():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "altro_batch.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(\s*altro_handle\s*\*\s*h\s*,\s*int32_t\s+ncand\b" % s, hdr), s


def test_built_library_exports_them():
    altro._lib.build()
    L = altro._lib.lib()
    for s in NEW:
        assert hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == 9 and getattr(L, s).restype is not None, s


def test_lib_exports_lists_them():
    for s in NEW:
        assert s in altro._lib.EXPORTS, s


def test_integration_doc_names_them():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert (":" + s) in doc, s


def fake(shape, dtype="torch.float64", strides=None, dev=("cuda", 0)):
    """stand-in with the four things the validation looks at"""
    st = api._dense_strides(shape) if strides is None else tuple(strides)
    return NS(shape=tuple(shape), dtype=dtype, stride=lambda: st, device=NS(type=dev[0], index=dev[1]), data_ptr=lambda: 4096)


def stand_in_solver(calls, B=3, n=2, m=1, N=4):
    rec = lambda name: (lambda *a: calls.append((name,) + a) or 0)
    L = NS(**{k: rec(k) for k in NEW})
    return NS(B=B, n=n, m=m, N=N, h=None, device=0, _L=L, _chk=lambda rc: None)


def test_device_form_validates_every_tensor_before_the_library_sees_it():
    calls = []
    sv = stand_in_solver(calls)          # B 3, n 2, m 1, N 4
    U, X, x0, Xout = fake((3, 5, 3, 1)), fake((3, 5, 4, 2)), fake((3, 2)), fake((3, 5, 4, 2))
    out = (fake((3, 5)), fake((3, 5)), fake((3, 5)))
    good = dict(U=U, X=None, x0=x0, out=out, Xout=Xout)
    bad = [dict(U=fake((3, 5, 4, 1))), dict(U=fake((2, 5, 3, 1))), dict(U=fake((3, 5, 3, 1), dtype="torch.float32")),
           dict(U=fake((3, 5, 3, 1), strides=(30, 6, 2, 1))), dict(U=fake((3, 5, 3, 1), dev=("cuda", 1))), dict(U=fake((3, 1))),
           dict(x0=fake((3, 3))), dict(x0=fake((3, 2), dtype="torch.float32")), dict(Xout=fake((3, 5, 3, 2))), dict(Xout=fake((3, 4, 2))),
           dict(out=(fake((3, 4)), None, None)), dict(out=(None, fake((3, 5), dtype="torch.int32"), None)), dict(out=(None, None, None)),
           dict(out=(fake((3, 5)), fake((3, 5)))), dict(out=(fake((3, 5), dev=("cuda", 1)), None, None)),
           dict(X=X), dict(X=X, x0=None), dict(X=fake((3, 5, 4, 3)), x0=None, Xout=None), dict(U=None), dict(U=None, x0=None)]
    for b in bad:
        args = dict(good)
        args.update(b)
        with pytest.raises(ValueError):
            api._evaluate_dev(sv, **args)
    assert calls == []
    assert api._evaluate_dev(sv, **good) == out
    assert api._evaluate_dev(sv, U, X, None, (None, out[1], None), None) == (None, out[1], None)
    one = (fake((3,)), fake((3,)), fake((3,)))
    assert api._evaluate_dev(sv, fake((3, 3, 1)), None, None, one, fake((3, 4, 2))) == one          # (B, N-1, m): one candidate
    assert api._evaluate_dev(sv, None, None, None, one, None) == one                               # the solver's own trajectory
    assert [c[0] for c in calls] == ["altro_batch_evaluate_dev"] * 4
    assert [c[2] for c in calls] == [5, 5, 1, 1]                                                     # ncand
    assert calls[0][4] is None and calls[1][5] is None and calls[1][9] is None                      # X / x0, Xout = NULL
    assert calls[3][3] is None and calls[3][4] is None


def test_numpy_takes_the_host_twin():
    calls = []
    sv = stand_in_solver(calls)
    U = np.zeros((3, 2, 3, 1))
    J, c, d = api.evaluate(sv, U)
    assert J.shape == c.shape == d.shape == (3, 2) and J.dtype == np.float64
    Xo = np.zeros((3, 2, 4, 2))
    assert api.rollout(sv, U, x0=np.zeros((3, 2)), out=Xo) is Xo
    assert api.rollout(sv, np.zeros((3, 3, 1))).shape == (3, 4, 2)
    Jo = np.zeros(3)
    assert api.evaluate(sv, out=(Jo, None, None))[0] is Jo
    assert [c_[0] for c_ in calls] == ["altro_batch_evaluate"] * 4 and [c_[2] for c_ in calls] == [2, 2, 1, 1]
    assert calls[1][6] is None and calls[1][8] is None and calls[1][9] is not None               # rollout: c_max and Xout only
    for kw in (dict(U=np.zeros((3, 2, 4, 1))), dict(U=U, X=np.zeros((3, 2, 4, 3))), dict(U=U, x0=np.zeros((2, 2))),
               dict(U=U, X=np.zeros((3, 2, 4, 2)), x0=np.zeros((3, 2))), dict(U=U, X=np.zeros((3, 2, 4, 2)), Xout=Xo),
               dict(U=U, out=(np.zeros((3, 2), dtype=np.float32), None, None)), dict(U=U, out=(None, None, None)), dict(U=None, x0=np.zeros((3, 2))),
               dict(U=U, Xout=np.zeros((3, 2, 4, 2))[:, :, :, ::-1])):
        with pytest.raises(ValueError):
            api.evaluate(sv, **kw)
    assert len(calls) == 4


def test_package_exposes_evaluate_and_rollout():
    assert callable(altro.evaluate) and callable(altro.rollout) and callable(altro.ExternalMPC.evaluate)
    assert altro.evaluate is api.evaluate and altro.rollout is api.rollout


@pytest.mark.parametrize("make", [ER.case_16_soc, ER.case_16_box, ER.case_wide_cone, ER.case_wide_rows])
def test_numpy_yardstick_agrees_with_the_oracle(oracle, make):
    """The protocol of the GPU tests' oracle check with numpy in place of the device: for every (instance, candidate) a fresh
    OracleSolver with zero duals takes the controls, reports orc_max_violation and orc_states, and the yardstick scores
    (X_orc, U).  c_max agrees within bound 4 (both sides computed in double: evaluate_ref's docstring); for the candidates the
    oracle finds feasible (c_max == 0; none of these problems has an equality row) orc_cost carries no AL term and J agrees
    within bound 3.  The yardstick's own rollout satisfies bound 1 against the oracle's states knot by knot, and its defect on the
    oracle's states stays inside bound 2.  (6, 3) with a cone is the case the issue names; the others ride along."""
    cs = make()
    U = ER.candidates(cs, 5)
    Xo, Jo, co = ER.oracle_scores(oracle, cs, U)
    cm, cb = ER.violation(cs, Xo, U)
    assert (np.abs(cm - co) <= cb).all(), np.abs(cm - co).max()
    feas = co == 0.0
    assert feas.any() and (~feas).any()
    assert feas[:, 0].all()                                # inside by construction
    if ER.controls_only_box(cs):
        assert not feas[:, 1].any()                        # pushed outside the control bounds
    J, Jb = ER.cost(cs, Xo, U)
    assert (np.abs(J - Jo)[feas] <= Jb[feas]).all(), (np.abs(J - Jo)[feas] / Jb[feas]).max()
    res, S = ER.step_residual(cs, Xo, U)
    assert (res <= ER.step_bound(cs, S)).all()
    assert (Xo[:, :, 0] == cs.x0[:, None]).all()
    dfc, db = ER.defect(cs, Xo, U)
    assert (dfc <= db).all()
    Xp = Xo.copy()
    Xp[:, :, 3, 1] += 1e-3
    assert (ER.defect(cs, Xp, U)[0] > 1e-4).all()


def test_yardstick_cone_residual_cases():
    """inside, polar and boundary branches of ||Proj(v) - v||_inf"""
    assert ER.soc_residual(np.array([0.3, 0.4, 0.5])) == 0.0
    assert ER.soc_residual(np.array([0.3, 0.4, -0.5])) == 0.5
    v = np.array([3.0, 4.0, 1.0])
    c = 0.5 * (1 + 1.0 / 5.0)
    assert abs(ER.soc_residual(v) - max(abs(c * 3 - 3), abs(c * 4 - 4), abs(c * 5 - 1))) < 1e-15
