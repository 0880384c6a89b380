"""Warm start from the best of several candidates (altro_batch_warm_start / _dev), the part that needs no GPU: the two entry
points are declared in the header, exported by the built library, bound by the ctypes layer and named in INTEGRATION.md's Julia
shim; the Python wrappers send GPU tensors to the device form and numpy to the host twin and refuse what they would have to
convert; the selection rule in plain Python (tests/warm_start_ref.py) on hand-made arrays; and the inputs of the GPU tests are
decidable by the numpy yardstick and exercise the choice."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

import evaluate_ref as ER
import warm_start_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["altro_batch_warm_start_dev", "altro_batch_warm_start"]
NAN, INF = float("nan"), float("inf")


def test_header_declares_both_functions():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "altro_batch.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(\s*altro_handle\s*\*\s*h\s*,\s*int32_t\s+ncand\s*,\s*const\s+double\s*\*\s*U\s*,\s*double\s+rho\s*,"
                         r"\s*int32_t\s+include_current\s*,\s*int32_t\s*\*\s*chosen\s*,\s*double\s*\*\s*J\s*,\s*double\s*\*\s*c_max\s*\)" % s, hdr), s


def test_built_library_exports_them():
    altro._lib.build()
    L = altro._lib.lib()
    for s in NEW:
        assert hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == 8 and getattr(L, s).restype is not None, s


def test_lib_exports_lists_them():
    for s in NEW:
        assert s in altro._lib.EXPORTS, s


def test_integration_doc_names_them():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert (":" + s) in doc, s


def test_package_exposes_warm_start():
    assert callable(altro.warm_start) and altro.warm_start is api.warm_start and callable(altro.ExternalMPC.warm_start)


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
    U = fake((3, 5, 3, 1))
    out = (fake((3,), dtype="torch.int32"), fake((3, 6)), fake((3, 6)))
    good = dict(U=U, rho=2.0, include_current=True, out=out)
    bad = [dict(U=fake((3, 5, 4, 1))), dict(U=fake((2, 5, 3, 1))), dict(U=fake((3, 5, 3, 1), dtype="torch.float32")),
           dict(U=fake((3, 5, 3, 1), strides=(30, 6, 2, 1))), dict(U=fake((3, 5, 3, 1), dev=("cuda", 1))), dict(U=fake((3, 1))),
           dict(U=fake((3, 0, 3, 1))), dict(U=None), dict(U=fake((3, 5, 3, 1), dev=("cpu", None))),
           dict(rho=-1.0), dict(rho=-1e-300), dict(rho=NAN), dict(rho=INF),
           dict(out=(fake((3,)), None, None)), dict(out=(fake((4,), dtype="torch.int32"), None, None)),
           dict(out=(None, fake((3, 5)), None)), dict(out=(None, None, fake((3, 6), dtype="torch.float32"))),
           dict(out=(None, fake((3, 6), strides=(1, 3)), None)), dict(out=(None, fake((3, 6), dev=("cuda", 1)), None)),
           dict(out=(None, None)), dict(include_current=False)]            # (without the incumbent J is (3, 5))
    for b in bad:
        args = dict(good)
        args.update(b)
        with pytest.raises(ValueError):
            api._warm_start_dev(sv, **args)
    assert calls == []
    assert api._warm_start_dev(sv, **good) == out
    assert api._warm_start_dev(sv, U, 0.0, False, (None, fake((3, 5)), None))[0] is None
    assert api._warm_start_dev(sv, fake((3, 3, 1)), 0.0, True, (out[0], fake((3, 2)), None))[0] is out[0]      # (B, N-1, m): one candidate
    assert api._warm_start_dev(sv, U, out=(None, None, None)) == (None, None, None)
    assert [c[0] for c in calls] == ["altro_batch_warm_start_dev"] * 4
    assert [c[2] for c in calls] == [5, 5, 1, 5]                                                     # ncand
    assert [c[4] for c in calls] == [2.0, 0.0, 0.0, 0.0] and [c[5] for c in calls] == [1, 0, 1, 1]  # rho, include_current
    assert calls[1][6] is None and calls[1][8] is None and calls[2][8] is None                      # NULLs as given
    assert calls[3][6] is None and calls[3][7] is None and calls[3][8] is None


def test_numpy_takes_the_host_twin():
    calls = []
    sv = stand_in_solver(calls)
    U = np.zeros((3, 2, 3, 1))
    ch, J, c = api.warm_start(sv, U)
    assert ch.shape == (3,) and ch.dtype == np.int32 and J.shape == c.shape == (3, 3) and J.dtype == np.float64
    ch, J, c = api.warm_start(sv, np.zeros((3, 3, 1)), rho=5.0, include_current=False)
    assert J.shape == (3, 1)
    Jo = np.zeros((3, 3))
    assert api.warm_start(sv, U, out=(None, Jo, None)) == (None, Jo, None)
    assert altro.ExternalMPC(sv).warm_start(U, rho=1.0)[1].shape == (3, 3)
    assert [c_[0] for c_ in calls] == ["altro_batch_warm_start"] * 4 and [c_[2] for c_ in calls] == [2, 1, 2, 2]
    assert [c_[4] for c_ in calls] == [0.0, 5.0, 0.0, 1.0] and [c_[5] for c_ in calls] == [1, 0, 1, 1]
    assert calls[2][6] is None and calls[2][7] is not None and calls[2][8] is None
    for kw in (dict(U=np.zeros((3, 2, 4, 1))), dict(U=np.zeros((2, 2, 3, 1))), dict(U=U, rho=-0.5), dict(U=U, rho=NAN), dict(U=U, rho=INF),
               dict(U=None), dict(U=U, out=(np.zeros(3), None, None)), dict(U=U, out=(None, np.zeros((3, 2)), None)),
               dict(U=U, out=(None, np.zeros((3, 3), dtype=np.float32), None)), dict(U=U, out=(None, np.zeros((3, 6))[:, ::2], None)),
               dict(U=U, out=(None, None))):
        with pytest.raises(ValueError):
            api.warm_start(sv, **kw)
    assert len(calls) == 4


# ---------------------------------------------------------------------------------------------- the rule
def test_fma_is_rounded_once():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30           # a b = 1 - 2^-60 exactly: the product rounds to 1.0
    assert a * b - 1.0 == 0.0 and WR.fma(a, b, -1.0) == -2.0 ** -60
    assert WR.fma(0.0, 7.0, 3.5) == 3.5 and np.isnan(WR.fma(0.0, INF, 1.0)) and WR.fma(2.0, INF, 1.0) == INF
    assert WR.fma(1e308, 10.0, 0.0) == INF


def test_select_ties_among_candidates_go_to_the_lowest_index():
    J = np.array([[3.0, 1.0, 1.0, 2.0], [5.0, 5.0, 5.0, 5.0]])
    assert list(WR.select(J, np.zeros_like(J), 0.0, False)) == [1, 0]
    c = np.array([[0.0, 2.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    assert list(WR.select(J, c, 1.0, False)) == [2, 0]                  # merits (3, 3, 2, 2), (5, 5, 5, 5)


def test_select_incumbent_wins_ties_and_is_the_last_column():
    J = np.array([[2.0, 1.0, 1.0], [2.0, 0.5, 1.0], [2.0, 3.0, 9.0]])
    assert list(WR.select(J, np.zeros_like(J), 0.0, True)) == [2, 1, 0]
    assert list(WR.select(J, np.zeros_like(J), 0.0, False)) == [1, 1, 0]


def test_select_nan_and_inf_never_win_and_all_invalid_gives_minus_one():
    J = np.array([[NAN, 4.0, 1.0], [INF, NAN, INF], [1.0, 2.0, NAN], [NAN, NAN, -INF]])
    c = np.zeros_like(J)
    assert list(WR.select(J, c, 0.0, True)) == [2, -1, 0, 2]
    assert list(WR.select(J, c, 0.0, False)) == [2, -1, 0, 2]
    c = np.array([[0.0, 0.0, INF], [0.0, 0.0, 0.0], [NAN, 0.0, 0.0], [0.0, 0.0, 0.0]])
    assert list(WR.select(J, c, 0.0, True)) == [1, -1, 1, 2]            # 0 * Inf is a NaN: the column cannot win
    assert list(WR.select(J, c, 1.0, True)) == [1, -1, 1, 2]


def test_select_mask_gives_minus_two():
    J = np.array([[2.0, 1.0], [2.0, 1.0], [NAN, NAN]])
    assert list(WR.select(J, np.zeros_like(J), 0.0, True, active=[1, 0, 0])) == [1, -2, -2]
    assert list(WR.select(J, np.zeros_like(J), 0.0, True, active=[1, 1, 1])) == [1, 1, -1]


# ---------------------------------------------------------------------------------------------- the inputs of the GPU tests
@pytest.mark.parametrize("name", list(WR.CASES))
def test_gpu_cases_are_decidable(name):
    """for every case and rho the gap between the best and the second-best merit (numpy yardstick; ER.candidates(cs, 5) and the
    reference controls as the incumbent) exceeds twice the summed rounding bounds 3 and 4 -- by a factor above 1e7, so the
    device's winner among distinct candidates is the yardstick's whatever its summation order"""
    cs = WR.CASES[name][0]()
    U = ER.candidates(cs, 5)
    for rho in WR.RHOS:
        win, gap, bound = WR.decided(cs, U, cs.Uref, rho)
        print(name, rho, list(win), (gap / bound).min())
        assert (gap > 1e7 * bound).all(), (name, rho)


def test_gpu_inputs_exercise_the_choice():
    """winners differ between instances (16-box, rho 0) and change with rho (16-soc, wide-cone): a constant answer fails"""
    def winners(name, rho):
        cs = WR.CASES[name][0]()
        return list(WR.decided(cs, ER.candidates(cs, 5), cs.Uref, rho)[0])
    assert set(winners("16-box(12,4)", 0.0)) == {0, 1, 3}
    assert winners("16-soc(6,3)", 0.0) == [0, 1, 0, 0, 3] and winners("16-soc(6,3)", 1e3) == [0, 3, 0, 0, 3]
    assert winners("wide-cone(7,3)", 0.0) != winners("wide-cone(7,3)", 1e3) != winners("wide-cone(7,3)", 1e6)
    cs = WR.CASES["16-box(12,4)"][0]()
    U6 = WR.six_candidates(cs, cs.Uref)
    assert U6.shape == (5, 6, 8, 4) and np.isnan(U6[:, 5]).any() and not np.isnan(U6[:, :5]).any()
    assert list(WR.expected_of_six(np.array([0, 3, 2]))) == [0, 6, 2]
