"""Per-instance episode clock: the parts that need no GPU -- the three symbols are declared by the header, listed in
_lib.EXPORTS, bound with argument types and exported by the built library; each refuses a NULL handle; INTEGRATION.md's
shim names them; api.set_clock refuses arrays of the wrong length or dtype before it calls the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc

NAMES = ["altro_mpc_set_clock", "altro_mpc_set_clock_dev", "altro_mpc_get_clock"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree():
    L = altro._lib.lib()
    with open(os.path.join(ROOT, "include", "altro_batch.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name in altro._lib.EXPORTS, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
        assert getattr(L, name).restype is C.c_int32, name
    assert "int32_t altro_mpc_set_clock(altro_handle* h, const int32_t* start, const int32_t* length);" in header
    assert "int32_t altro_mpc_set_clock_dev(altro_handle* h, const int32_t* start, const int32_t* length);" in header
    assert "int32_t altro_mpc_get_clock(altro_handle* h, int32_t* start, int32_t* length, int32_t* window);" in header
    # one ctypes argument per parameter of the declaration
    for name in NAMES:
        decl = re.search(r"^int32_t %s\(([^)]*)\);" % name, header, re.M).group(1)
        assert len(getattr(L, name).argtypes) == len(decl.split(",")), name


def test_each_refuses_a_null_handle():
    L = altro._lib.lib()
    INV = altro._lib.ERR_INVALID_ARG
    a = np.zeros(4, dtype=np.int32)
    ip = a.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.altro_mpc_set_clock(None, ip, ip) == INV
    assert L.altro_mpc_set_clock(None, None, None) == INV
    assert L.altro_mpc_set_clock_dev(None, None, None) == INV
    assert L.altro_mpc_get_clock(None, ip, ip, ip) == INV
    assert (L.altro_last_error(None) or b"").decode()


def test_integration_shim_names_them():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in NAMES:
        assert ":" + name in doc, name


class _NoLibrary:
    """a solver whose library must not be reached"""
    B, device, h = 6, 0, None

    @property
    def _L(self):
        raise AssertionError("the library was called")

    def _chk(self, rc):
        raise AssertionError("the library was called")


def test_set_clock_checks_its_arrays_first():
    s = _NoLibrary()
    with pytest.raises(ValueError):
        api.set_clock(s, np.zeros(5, dtype=np.int32))                       # wrong length
    with pytest.raises(ValueError):
        api.set_clock(s, np.zeros(6, dtype=np.int32), np.zeros(7, dtype=np.int32))
    with pytest.raises(ValueError):
        api.set_clock(s, np.zeros((6, 1), dtype=np.int32))
    with pytest.raises(TypeError):
        api.set_clock(s, np.zeros(6, dtype=np.float64))                     # wrong dtype
    with pytest.raises(TypeError):
        api.set_clock(s, np.zeros(6, dtype=np.int32), np.ones(6, dtype=np.float32))
    with pytest.raises(ValueError):
        api.set_clock(s, np.full(6, 2 ** 40, dtype=np.int64))               # does not fit int32
    with pytest.raises(ValueError):
        api.set_clock(s, None, np.zeros(6, dtype=np.int32))                 # a length without a start


def test_python_layer_exposes_the_calls():
    assert callable(api.set_clock) and callable(api.get_clock)
    for cls in (mpc.BatchMPC, mpc.TrackMPC):
        assert callable(cls.set_clock) and callable(cls.respawn)
