"""Constraint data and box bounds from device pointers, the part that needs no GPU: the three exports are declared, bound,
exported and documented; GPU tensors for A, b, zmin, zmax go through check_device_tensor, which refuses what it would have to
convert; numpy and CPU tensors keep taking the host entry points."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["altro_batch_update_constraint_data_dev", "altro_batch_set_bounds_dev", "altro_batch_get_dev_refusals"]


def test_new_exports_are_declared_bound_exported_and_documented():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "altro_batch.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    altro._lib.build()
    L = altro._lib.lib()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in altro._lib.EXPORTS, s
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None and getattr(L, s).restype is not None, s
        assert (":" + s) in doc, s


def fake(shape, dtype="torch.float64", strides=None, dev=("cuda", 0)):
    """stand-in with the four things the validation looks at"""
    st = api._dense_strides(shape) if strides is None else tuple(strides)
    return NS(shape=tuple(shape), dtype=dtype, stride=lambda: st, device=NS(type=dev[0], index=dev[1]), data_ptr=lambda: 4096)


def stand_in_solver(calls, B=3, n=2, m=1, N=4, p=2):
    """a solver whose library records which entry point was taken; constraint 0 is a BOX, constraint 1 a per-knot LINEAR
    constraint of p rows on knots 1..N-1"""
    rec = lambda name: (lambda *a: calls.append((name,) + a) or 0)
    L = NS(**{k: rec(k) for k in ("altro_batch_update_constraint_data", "altro_batch_update_constraint_data_dev",
                                  "altro_batch_set_bounds", "altro_batch_set_bounds_dev")})
    cons = api.ConstraintList(n, m, N)
    cons.add_constraint(api.BoundConstraint(n, m, u_min=-1.0, u_max=1.0), (1, N - 1))
    cons.add_constraint(api.LinearConstraint(np.zeros((N - 1, p, n + m)), np.zeros((N - 1, p))), (1, N - 1))
    return NS(B=B, n=n, m=m, N=N, h=None, device=0, _L=L, _chk=lambda rc: None, con_ids=[0, 1], prob=NS(constraints=cons))


@pytest.mark.parametrize("what", ["A", "b", "zmin", "zmax"])
def test_tensors_with_a_wrong_dtype_strides_device_or_shape_are_refused(what):
    calls = []
    sv = stand_in_solver(calls)
    nz, nk, p = 3, 3, 2
    good = {"A": (nk, p, nz), "b": (nk, p), "zmin": (sv.B, nz), "zmax": (sv.B, nz)}
    shape = good[what]
    bad = [(fake(shape, dtype="torch.float32"), "dtype"),
           (fake(shape, strides=tuple(2 * s for s in api._dense_strides(shape))), "strides"),
           (fake(shape, dev=("cuda", 1)), "cuda:0"),
           (fake(shape[:-1] + (shape[-1] + 1,)), "shape")]
    for t, msg in bad:
        args = {k: fake(v) for k, v in good.items()}
        args[what] = t
        with pytest.raises(ValueError, match=msg):
            if what in ("A", "b"):
                api._update_constraint_data_dev(sv, 1, args["A"], args["b"])
            else:
                api._set_bounds_dev(sv, 0, args["zmin"], args["zmax"])
    assert calls == []                                        # nothing reached the library
    # the good ones do, on the device entry points; a shared row of bounds is (n+m,)
    api._update_constraint_data_dev(sv, 1, fake(good["A"]), None)
    api._update_constraint_data_dev(sv, 1, None, fake(good["b"]))
    api._set_bounds_dev(sv, 0, fake(good["zmin"]), fake(good["zmax"]))
    api._set_bounds_dev(sv, 0, fake((nz,)), fake((nz,)))
    assert [c[0] for c in calls] == ["altro_batch_update_constraint_data_dev"] * 2 + ["altro_batch_set_bounds_dev"] * 2
    assert calls[2][-1] == 1 and calls[3][-1] == 0            # per_instance
    with pytest.raises(altro.AltroError):                     # a BOX has no A, b
        api._update_constraint_data_dev(sv, 0, fake(good["A"]), None)


def test_cpu_tensors_and_numpy_still_take_the_host_entry_points():
    import torch
    calls = []
    sv = stand_in_solver(calls)
    A, b = np.arange(18.0).reshape(3, 2, 3), np.arange(6.0).reshape(3, 2)
    api.update_constraint_data(sv, 1, A, b)
    api.update_constraint_data(sv, 1, torch.from_numpy(A).to(torch.float32), None)   # cast by the numpy path, as ever
    api.set_bounds(sv, 0, np.full(3, -2.0), np.full(3, 2.0))
    api.set_bounds(sv, 0, torch.full((3, 3), -2.0), torch.full((3, 3), 2.0))
    assert [c[0] for c in calls] == ["altro_batch_update_constraint_data"] * 2 + ["altro_batch_set_bounds"] * 2
    got = np.ctypeslib.as_array(calls[1][3], shape=(3, 2, 3))
    assert got.dtype == np.float64 and np.array_equal(got, A) and calls[1][4] is None
    assert calls[2][-1] == 0 and calls[3][-1] == 1


def test_dev_refusals_is_exported_by_the_package():
    assert callable(api.dev_refusals) and "constraint_data" in altro.ExternalMPC.tick.__code__.co_varnames
