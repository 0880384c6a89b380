"""Gradient of a candidate's merit (altro_batch_evaluate_grad / _dev), the part that needs no GPU: the two entry points are
declared, exported, bound and named in INTEGRATION.md; the Python wrappers validate before the library is called; and the numpy
yardstick the GPU tests hold the device to (tests/evaluate_grad_ref.py) is itself pinned by the CPU oracle: a fresh oracle with
zero duals carries penalty 1 per row, so its cost() is M = J + P at rho = 1, and its central differences are the gradient (M is
piecewise quadratic: exact in exact arithmetic for any step that crosses no kink).

Tolerances are the derived bounds of evaluate_grad_ref's docstring, none measured.  Measured figures are printed before each
assertion."""
import dataclasses
import functools
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

import evaluate_ref as ER
import evaluate_grad_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["altro_batch_evaluate_grad_dev", "altro_batch_evaluate_grad"]
CASES = {
    "16-box(12,4)": (ER.case_16_box, False),
    "16-soc(6,3)": (ER.case_16_soc, False),
    "wide-rows(20,5)": (ER.case_wide_rows, False),
    "wide-ltv(12,12)": (ER.case_wide_ltv, True),
    "wide-cone(7,3)": (ER.case_wide_cone, False),
    "wide-box(30,25)": (ER.case_wide_box, False),
    "wide-limits(64,32)": (ER.case_wide_limits, False),
}
ORACLE_CASES = [k for k in CASES if k != "wide-limits(64,32)"]


# ---------------------------------------------------------------------------------------------- the interface
def test_header_declares_both_functions():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "altro_batch.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(\s*altro_handle\s*\*\s*h\s*,\s*int32_t\s+ncand\s*,\s*const\s+double\s*\*\s*U\s*,"
                         r"\s*const\s+double\s*\*\s*x0\s*,\s*double\s+rho\b" % s, hdr), s


def test_built_library_exports_them():
    altro._lib.build()
    L = altro._lib.lib()
    for s in NEW:
        assert hasattr(L, s) and s in altro._lib.EXPORTS, s
        assert len(getattr(L, s).argtypes) == 10 and getattr(L, s).restype is not None, s


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
    return NS(B=B, n=n, m=m, N=N, h=None, device=0, _L=NS(**{k: rec(k) for k in NEW}), _chk=lambda rc: None)


def test_device_form_validates_every_tensor_before_the_library_sees_it():
    calls = []
    sv = stand_in_solver(calls)          # B 3, n 2, m 1, N 4
    U, x0, Xout = fake((3, 5, 3, 1)), fake((3, 2)), fake((3, 5, 4, 2))
    out = (fake((3, 5)), fake((3, 5)), fake((3, 5, 3, 1)), fake((3, 5, 2)))
    good = dict(U=U, x0=x0, rho=2.0, out=out, Xout=Xout)
    bad = [dict(U=None), dict(U=fake((3, 5, 4, 1))), dict(U=fake((3, 5, 3, 1), dtype="torch.float32")), dict(U=fake((3, 5, 3, 1), strides=(30, 6, 2, 1))),
           dict(U=fake((3, 5, 3, 1), dev=("cuda", 1))), dict(x0=fake((3, 3))), dict(Xout=fake((3, 5, 3, 2))),
           dict(rho=-1.0), dict(rho=float("nan")), dict(rho=float("inf")),
           dict(out=(None, None, None, None)), dict(out=out[:3]), dict(out=(fake((3, 4)), None, None, None)),
           dict(out=(None, None, fake((3, 5, 3, 2)), None)), dict(out=(None, None, None, fake((3, 2)))),
           dict(out=(None, fake((3, 5), dtype="torch.int32"), None, None))]
    for b in bad:
        args = dict(good)
        args.update(b)
        with pytest.raises(ValueError):
            api._evaluate_grad_dev(sv, **args)
    assert calls == []
    assert api._evaluate_grad_dev(sv, **good) == out
    one = (None, None, fake((3, 3, 1)), fake((3, 2)))
    assert api._evaluate_grad_dev(sv, fake((3, 3, 1)), None, 0.0, one, None) == one               # (B, N-1, m): one candidate
    assert [c[0] for c in calls] == ["altro_batch_evaluate_grad_dev"] * 2 and [c[2] for c in calls] == [5, 1]
    assert calls[0][5] == 2.0 and calls[1][4] is None and calls[1][5] == 0.0 and calls[1][6] is None and calls[1][10] is None


def test_numpy_takes_the_host_twin():
    calls = []
    sv = stand_in_solver(calls)
    U = np.zeros((3, 2, 3, 1))
    J, P, gU, gx0 = api.evaluate_grad(sv, U, rho=1.0)
    assert J.shape == P.shape == (3, 2) and gU.shape == U.shape and gx0.shape == (3, 2, 2)
    g1 = np.zeros((3, 3, 1))
    assert api.evaluate_grad(sv, np.zeros((3, 3, 1)), x0=np.zeros((3, 2)), out=(None, None, g1, None))[2] is g1
    assert [c[0] for c in calls] == ["altro_batch_evaluate_grad"] * 2 and [c[2] for c in calls] == [2, 1]
    for kw in (dict(U=None), dict(U=np.zeros((3, 2, 4, 1))), dict(U=U, x0=np.zeros((2, 2))), dict(U=U, rho=-0.5),
               dict(U=U, out=(None,) * 4), dict(U=U, out=(np.zeros((3, 2), dtype=np.float32), None, None, None)),
               dict(U=U, Xout=np.zeros((3, 2, 4, 2))[:, :, :, ::-1])):
        with pytest.raises(ValueError):
            api.evaluate_grad(sv, **kw)
    assert len(calls) == 2


def test_package_exposes_the_calls():
    assert altro.evaluate_grad is api.evaluate_grad and altro.merit is api.merit and callable(altro.ExternalMPC.merit)
    with pytest.raises(ValueError):
        altro.merit(stand_in_solver([]), np.zeros((3, 3, 1)))       # numpy has no grad_fn to give


# ---------------------------------------------------------------------------------------------- the yardstick
@functools.lru_cache(maxsize=None)
def setup(name):
    make, pk = CASES[name]
    cs = make()
    U = GR.candidates_with_polar(cs, 101)
    return NS(cs=cs, pk=pk, U=U, X=ER.rollout(cs, U))


def oracle_merit(O, cs, U, pk, x0=None):
    """(X_orc, M_orc): set_controls on a fresh oracle with zero duals per (instance, candidate); x0 (B, nc, n) replaces the
    case's initial state.  Its cost() is J + P (penalty 1 on every row)."""
    B, nc = U.shape[:2]
    X, M = np.zeros((B, nc, cs.N, cs.n)), np.zeros((B, nc))
    for b in range(B):
        for c in range(nc):
            cb = cs if x0 is None else dataclasses.replace(cs, x0=np.broadcast_to(x0[b, c], cs.x0.shape))
            s = ER.oracle_of(O, cb, b, pk)
            s.set_controls(U[b, c])
            s.max_violation()                                 # (ER.oracle_scores' order: the oracle rolls out here)
            X[b, c], M[b, c] = s.states(), s.cost()
    return X, M


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_are_clear_of_kinks(name):
    """1: every row value of every candidate is at least 1e6 of its own bounds from its kink, so no two computations of it pick
    different sides; candidates 1 and 2 have active rows; (6, 3) reaches all three cone branches, (7, 3) the polar cone only
    through the candidate built for it"""
    s = setup(name)
    g = GR.merit_grad(s.cs, s.X, s.U, 1.0)
    print(name, "min margin", g.margin.min(), "active rows", g.nact.sum(axis=0), "cone branches", g.branch.sum(axis=0).tolist())
    assert (g.margin >= 1e6).all(), g.margin.min()
    assert (g.nact[:, 1:3].sum(axis=0) > 0).all()
    if name == "16-soc(6,3)":
        assert (g.branch.sum(axis=(0, 1)) > 0).all()
    if name == "wide-cone(7,3)":
        assert s.U.shape[1] == 4 and (g.branch[:, :3, 1] == 0).all() and (g.branch[:, 3, 1] >= 1).all()
        v = np.array([0.1, 0.1, 0.5 * -6.0 + 2.0])
        assert v[2] == -1.0 and np.hypot(v[0], v[1]) <= -v[2]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_merit_at_rho_one_is_the_oracles_cost(name, oracle):
    """2: J + P of the yardstick on the oracle's own states == the fresh oracle's cost() within bound 3 plus bound 5"""
    s = setup(name)
    Xo, Mo = oracle_merit(oracle, s.cs, s.U, s.pk)
    M, Mb = GR.merit(s.cs, Xo, s.U, 1.0)
    print(name, "max |dM| / bound", (np.abs(M - Mo) / Mb).max(), "relative", (np.abs(M - Mo) / np.abs(Mo)).max())
    assert (np.abs(M - Mo) <= Mb).all()
    assert (GR.merit_grad(s.cs, Xo, s.U, 1.0).P[:, 1:3] > 0).any(axis=0).all()


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_gradient_against_the_oracles_central_differences(name, oracle):
    """3: along a random direction D (and, for gx0, d0) with the step chosen from the margins so that no row changes side
    between the two points -- nothing is excluded -- the oracle's (M(+h) - M(-h)) / 2h equals <g, D>.  Tolerance: the bounds of
    M at both points (3 + 5, and bound 7 for the oracle's rounded states) over 2h, plus twice the gradient bound (6, with 7)
    times |D|, plus bound 8 where a cone value sits on the boundary branch (M is not quadratic there, so the difference is not
    exact; the step is then chosen to balance truncation against rounding)."""
    s = setup(name)
    cs, U = s.cs, s.U
    rng = np.random.default_rng(7)
    Xo, _ = oracle_merit(oracle, cs, U, s.pk)
    x0c = np.broadcast_to(cs.x0[:, None], U.shape[:2] + (cs.n,))
    for what in ("U", "x0"):
        D = rng.standard_normal(U.shape) if what == "U" else np.zeros(U.shape)
        d0 = None if what == "U" else rng.standard_normal(x0c.shape)
        g = GR.merit_grad(cs, Xo, U, 1.0, direction=(GR.tangent(cs, D, d0), D), state_err=GR.rollout_error(cs, Xo, U))
        h = GR.fd_step(g, 1.0, GR.merit(cs, Xo, U, 1.0)[1])
        assert (h > 0).all() and np.isfinite(h).all()
        pts, err = [], 0.0
        for sgn in (1.0, -1.0):
            Up = U + sgn * h[..., None, None] * D
            Xp, Mp = oracle_merit(oracle, cs, Up, s.pk, None if d0 is None else x0c + sgn * h[..., None] * d0)
            gp = GR.merit_grad(cs, Xp, Up, 1.0)
            assert (gp.margin >= 1e6).all()
            err = err + GR.merit(cs, Xp, Up, 1.0)[1] + (np.abs(gp.Lx) * GR.rollout_error(cs, Xp, Up)).sum(axis=(2, 3))
            pts.append(Mp)
        fd = (pts[0] - pts[1]) / (2 * h)
        if what == "U":
            want, gb = (g.gU * D).sum(axis=(2, 3)), 2 * (g.gUb * np.abs(D)).sum(axis=(2, 3))
        else:
            want, gb = (g.gx0 * d0).sum(axis=-1), 2 * (g.gx0b * np.abs(d0)).sum(axis=-1)
        tol = err / (2 * h) + gb + GR.fd_truncation(g, 1.0, h)
        print(name, what, "h", h.min(), h.max(), "max |fd - <g, D>| / tol", (np.abs(fd - want) / tol).max(),
              "relative", (np.abs(fd - want) / np.abs(want)).max())
        assert (np.abs(fd - want) <= tol).all()
        assert (tol <= 1e-6 * np.abs(want)).all()          # (the check has teeth: the tolerance is far below the gradient)


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_is_affine_in_rho(name):
    """4: g(10) - g(0) == 10 (g(1) - g(0)) within bound 6 of each of the four evaluations"""
    s = setup(name)
    g0, g1, g10 = (GR.merit_grad(s.cs, s.X, s.U, rho) for rho in (0.0, 1.0, 10.0))
    for a, b in (("gU", "gUb"), ("gx0", "gx0b")):
        lhs, rhs = getattr(g10, a) - getattr(g0, a), 10 * (getattr(g1, a) - getattr(g0, a))
        tol = getattr(g10, b) + getattr(g0, b) + 10 * (getattr(g1, b) + getattr(g0, b))
        assert (np.abs(lhs - rhs) <= tol).all(), (name, a)
        assert a != "gU" or (np.abs(lhs) > 1e3 * tol).any()         # (the constraint term is there)
    assert np.array_equal(g0.P, g10.P)
