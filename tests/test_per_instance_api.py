"""Per-instance cost weights and box bounds: the parts that need no GPU -- the two exports refuse a NULL handle, and the
Python layer picks the shared or the per-instance call from the shapes it is given (and refuses a wrong batch length
instead of passing a pointer to too little data through)."""
import ctypes as C

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api


def test_new_exports_refuse_a_null_handle():
    L = altro._lib.lib()
    q = np.ones(4)
    dp = q.ctypes.data_as(C.POINTER(C.c_double))
    assert L.altro_batch_set_tracking_cost_per_instance(None, dp, dp, dp, 0.1) == altro._lib.ERR_INVALID_ARG
    assert L.altro_batch_set_bounds(None, 0, dp, dp, 1) == altro._lib.ERR_INVALID_ARG
    assert L.altro_batch_set_bounds(None, 0, dp, dp, 0) == altro._lib.ERR_INVALID_ARG


def test_one_dimensional_weights_take_the_shared_call():
    pi, q, r, qf = api.cost_rows(np.full(12, 10.0), np.full(4, 0.1), np.full(12, 10.0), 7)
    assert not pi and q.shape == (12,) and r.shape == (4,) and qf.shape == (12,)


def test_two_dimensional_weights_take_the_per_instance_call():
    B = 7
    Q = np.arange(B * 12, dtype=float).reshape(B, 12)
    pi, q, r, qf = api.cost_rows(Q, np.full(4, 0.1), 49 * Q, B)
    assert pi and q.shape == (B, 12) and r.shape == (B, 4) and qf.shape == (B, 12)
    assert np.array_equal(q, Q) and np.array_equal(qf, 49 * Q)
    assert np.all(r == 0.1)                 # the shared one is broadcast to every instance
    assert q.flags.c_contiguous and r.flags.c_contiguous


def test_wrong_leading_dimension_raises():
    with pytest.raises(altro.AltroError) as e:
        api.cost_rows(np.ones((6, 12)), np.ones(4), np.ones(12), 7)
    assert e.value.code == altro._lib.ERR_INVALID_ARG
    with pytest.raises(altro.AltroError):
        api.cost_rows(np.ones((7, 2, 12)), np.ones(4), np.ones(12), 7)


def test_bound_constraint_rows():
    n, m, B = 3, 2, 5
    ub = np.linspace(1.5, 4.0, B)[:, None] * np.ones(m)
    c = api.BoundConstraint(n, m, u_min=-ub, u_max=ub)
    assert c.per_instance()
    zmin, zmax = c.zbounds(B)
    assert zmin.shape == (B, n + m) and zmax.shape == (B, n + m)
    assert np.all(np.isneginf(zmin[:, :n])) and np.all(np.isposinf(zmax[:, :n]))
    assert np.array_equal(zmax[:, n:], ub) and np.array_equal(zmin[:, n:], -ub)
    with pytest.raises(altro.AltroError) as e:
        c.zbounds(B + 1)
    assert e.value.code == altro._lib.ERR_INVALID_ARG
    # the shared form is unchanged
    s = api.BoundConstraint(n, m, u_min=-3.0, u_max=3.0)
    assert not s.per_instance()
    lo, hi = s.zbounds()
    assert lo.shape == (n + m,) and np.array_equal(hi[n:], np.full(m, 3.0))


def test_heterogeneous_generator_keeps_the_shared_batch():
    a = altro.problems.gen_random_linear_batch(6, steps=3, seed=4)
    h = altro.problems.gen_random_linear_hetero_batch(6, steps=3, seed=4)
    assert np.array_equal(a.A, h.A) and np.array_equal(a.Xtrack, h.Xtrack) and np.array_equal(a.noise, h.noise)
    assert h.Qk.shape == (6, 12) and np.array_equal(h.Qfk, (h.N - 1) * h.Qk)
    assert h.u_bnd.shape == (6,) and np.all((h.u_bnd >= 1.5) & (h.u_bnd <= 4.0))
    assert a.Qk == 10.0 and a.u_bnd == 3.0
    prob = altro.mpc.gen_tracking_problem(h)
    assert prob.obj.Q.shape == (6, 12) and prob.obj.R.shape == (4,)
    zmin, zmax = prob.constraints.items[0][0].zbounds(6)
    assert np.array_equal(zmax[:, 12:], np.repeat(h.u_bnd[:, None], 4, axis=1))
