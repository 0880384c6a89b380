"""Feedback policy on the device, the part that needs no GPU: the three entry points are declared in the header, exported by
the built library, bound by the ctypes layer and named in INTEGRATION.md's Julia shim; the Python wrappers send GPU tensors to
the device form and numpy to the host twin, and refuse what they would have to convert."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["altro_batch_eval_policy_dev", "altro_batch_eval_policy", "altro_batch_get_gains_dev"]


def test_header_declares_the_three_functions():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "altro_batch.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(\s*altro_handle\s*\*" % s, hdr), s


def test_built_library_exports_them():
    altro._lib.build()
    L = altro._lib.lib()
    for s in NEW:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None and getattr(L, s).restype is not None, s


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
    sv = stand_in_solver(calls)
    x, knot, out, fb = fake((3, 2)), fake((3,), dtype="torch.int32"), fake((3, 1)), fake((3,), dtype="torch.int32")
    bad = [dict(x=fake((3, 3))), dict(x=fake((3, 2), dtype="torch.float32")), dict(knot=fake((3,), dtype="torch.int64")),
           dict(out=fake((3, 2))), dict(fb=fake((3,))), dict(x=fake((3, 2), dev=("cuda", 1))), dict(out=fake((3, 1), strides=(2, 2)))]
    for b in bad:
        args = dict(x=x, knot=knot, out=out, fb=fb)
        args.update(b)
        with pytest.raises(ValueError):
            api._eval_policy_dev(sv, args["x"], args["knot"], True, args["out"], args["fb"])
    assert calls == []
    assert api._eval_policy_dev(sv, x, knot, True, out, fb) is out
    assert api._eval_policy_dev(sv, x, None, False, out, None) is out
    assert [c[0] for c in calls] == ["altro_batch_eval_policy_dev"] * 2
    assert calls[0][4] == 1 and calls[1][4] == 0                       # clamp
    assert calls[1][3] is None and calls[1][6] is None                 # knot = NULL, fb = NULL


def test_numpy_takes_the_host_twin():
    calls = []
    sv = stand_in_solver(calls)
    fb = np.zeros(3, dtype=np.int32)
    u = api.eval_policy(sv, np.zeros((3, 2)), knot=[0, 1, 2], clamp=False, fb=fb)
    assert u.shape == (3, 1) and u.dtype == np.float64
    assert [c[0] for c in calls] == ["altro_batch_eval_policy"] and calls[0][4] == 0
    assert np.array_equal(np.ctypeslib.as_array(calls[0][3], shape=(3,)), [0, 1, 2])
    with pytest.raises(ValueError):
        api.eval_policy(sv, np.zeros((3, 2)), fb=np.zeros(3, dtype=np.int64))
    with pytest.raises(TypeError):
        api.eval_policy(sv, np.zeros((3, 2)), knot=np.array([0.0, 1.0, 2.0]))
    assert len(calls) == 1


def test_package_exposes_the_policy_calls():
    assert callable(altro.eval_policy) and callable(altro.get_gains_dev) and callable(altro.ExternalMPC.policy)
    assert "policy" in altro.ExternalMPC.__doc__
