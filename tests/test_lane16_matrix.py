"""The table of tests/lane16_matrix.py, checked without a GPU: (a) supported_dims and the ALTRO_LAUNCH list of altro_batch.hip name
exactly the table's shapes, and the table reaches each with generic rows and without; (b) the Python restatement of
pack_constraints puts the cases where the table says they are -- all 16 lanes, linear rows in the spare lanes of cone quads, a
quad whose cone changes dimension, a canonical knot that is not 0, the refusals; (c) the inputs of every case are worth comparing
on -- feasible, below the penalty cap, several outer iterations, every kind of constraint binding, and answers that do not hinge
on the last bit of the inputs -- on the CPU oracle alone.
Each case prints its statuses, outer-iteration counts, which dual blocks are nonzero and the oracle's one-ulp sensitivity."""
import os
import re

import numpy as np
import pytest

import lane16_matrix as lm
from altro_mpc_icra2021_amd import problems as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "altro-mpc-icra2021_amd", "csrc")
N = lm.N
ROW_CASES = [(lm.shape_id(s), v) for s in lm.SHAPES for v in ("ti", "ltv", "pi")]


def built_shapes():
    """((n, m) of supported_dims, (n, m) of the ALTRO_LAUNCH dispatch) in altro_batch.hip; every ALTRO_LAUNCH builds
    solve_kernel<n, m, true> and <n, m, false>."""
    src = open(os.path.join(CSRC, "altro_batch.hip")).read()
    body = re.search(r"static bool supported_dims\(int n, int m\) \{(.*?)\n\}", src, re.S).group(1)
    dims = [(int(a), int(b)) for a, b in re.findall(r"n == (\d+) && m == (\d+)", body)]
    macro = re.search(r"#define ALTRO_LAUNCH\(NX_, NU_\)((?:.*\\\n)*.*\n)", src).group(1)
    assert "solve_kernel<NX_, NU_, true>" in macro and "solve_kernel<NX_, NU_, false>" in macro
    launch = [(int(a), int(b)) for a, b in re.findall(r"n == (\d+) && m == (\d+)\) ALTRO_LAUNCH\((?:\d+), (?:\d+)\)", src)]
    assert [(int(a), int(b)) for a, b in re.findall(r"ALTRO_LAUNCH\((\d+), (\d+)\);", src)] == launch
    return dims, launch


def test_table_names_exactly_the_built_kernels_with_rows_and_without():
    dims, launch = built_shapes()
    assert dims == launch == lm.SHAPES
    with_rows = {s for s in lm.SHAPES if lm.packed(lm.rows_problem(s, "ti")).meta[:, :, 0].any()}
    assert with_rows == set(lm.SHAPES) == set(lm.ROWS10) == set(lm.TRACK)
    # without rows: test_option_fuzz_matches_oracle runs every shape box-only (its parameter list, read from the source)
    parity = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_parity.py")).read()
    fuzz = re.search(r'parametrize\("n,m", \[(.*?)\]\)\ndef test_option_fuzz_matches_oracle', parity).group(1)
    assert set(lm.SHAPES) <= {(int(a), int(b)) for a, b in re.findall(r"\((\d+), (\d+)\)", fuzz)}
    assert {(12, 4), (8, 4), (6, 6)} <= set(lm.QUAD_SHAPES)


# ---------------------------------------------------------------------------------------------------------------------
# the packing
def _row(k0, k1, p=1, sense=P.INEQ):
    return P.ConstraintSpec(P.LINEAR, sense, k0, k1, A=np.ones((p, 4)), b=np.zeros(p))


def _cone(k0, k1, p):
    return P.ConstraintSpec(P.SOC, P.INEQ, k0, k1, A=np.ones((p, 4)), b=np.zeros(p))


@pytest.mark.parametrize("sid", [lm.shape_id(s) for s in lm.QUAD_SHAPES])
def test_quads_layout(sid):
    pr = lm.quads_problem(lm.SHAPE_BY_ID[sid])
    pk = lm.packed(pr)
    lanes = {kind: pk.lanes.get(ci) for ci, kind in enumerate(pr.kinds)}
    assert lanes == dict(soc4=[0, 1, 2, 3], soc2=[4, 5], soc3x=[8, 9, 10], soc2m=[12, 13], soc3m=[12, 13, 14], lin=[6, 7, 11, 15],
                         eq=[0, 1], xub=[14], box=None)
    typ, dim = pk.meta[:, :, 0], pk.meta[:, :, 3]
    assert np.all(typ[6:N - 1] != 0)                                      # knots 6..N-2: all 16 lanes hold a row
    assert np.all(typ[:N - 1, [6, 7, 11, 15]] == 2)                       # linear rows ...
    assert np.all(dim[:N - 1, [6, 7]] == 2) and np.all(dim[1:N - 1, 11] == 3) and np.all(dim[6:N - 1, 15] == 3)   # ... inside cone quads
    assert np.all(dim[:6, 12:16] == 2) and np.all(dim[6:N - 1, 12:16] == 3)   # quad 3: dimension 2, then 3
    assert np.all(typ[1:6, 14] == 2) and np.all(typ[6:N - 1, 14] == 3)    # lane 14: the state bound, then the third row of soc3m
    assert np.all(typ[N - 1, :2] == 1) and np.all(typ[N - 1, 8:11] == 3) and typ[N - 1].astype(bool).sum() == 5
    assert dim[0, 11] == 0                                                # soc3x starts at knot 1: at knot 0 lane 11 is a plain row
    assert pk.con_inv == 0


@pytest.mark.parametrize("sid", [lm.shape_id(s) for s in lm.SHAPES])
def test_track_and_rows10_layout(sid):
    shape = lm.SHAPE_BY_ID[sid]
    tp = lm.track_problem(shape)
    pk = lm.pack(tp.cons, N)
    assert pk.lanes == {0: [0, 1, 2], 1: [3, 4], 3: [5]}
    assert pk.con_inv == 1 and pk.ckn == [0] * 5 + [1] + [0] * 10          # the state bound starts at knot 1
    assert np.all(pk.meta[:N - 1, 3, 0] == 2) and np.all(pk.meta[:N - 1, 3, 3] == 3)     # lane 3: a linear row in the cone's spare lane
    for variant in ("ti", "ltv", "pi"):
        pr = lm.rows_problem(shape, variant)
        pk = lm.packed(pr)
        lanes = {kind: pk.lanes.get(ci) for ci, kind in enumerate(pr.kinds)}
        assert lanes == dict(soc=[0, 1, 2], lin=[3, 4, 5, 6], eq=[0, 1], xub=[7], box=None), variant
        assert pk.con_inv == 0        # the equality shares lanes 0 and 1 with the cone
        assert np.all(pk.meta[:N - 1, 0, 0] == 3) and pk.meta[N - 1, 0, 0] == 1
        assert sorted(lm.per_instance_blocks(pr)) == ([0, 2, 4] if variant == "pi" else [])
    # without the equality every lane of rows10 holds one block, but per-instance data alone rules con_inv out
    pr = lm.rows_problem(shape, "pi")
    free = [c for c, kind in zip(pr.cons_b[0], pr.kinds) if kind != "eq"]
    assert lm.pack(free, N).con_inv == 1 and lm.pack(free, N, per_instance=True).con_inv == 0


def test_pack_refusals():
    """The 17th row at a full knot, the 5th cone over a knot that holds four; a 5th cone on a disjoint range is taken."""
    full = [_cone(0, N - 2, 4), _cone(0, 5, 2), _cone(6, N - 2, 3), _row(0, N - 2, 9)]
    pk = lm.pack(full, N)
    assert pk.lanes == {0: [0, 1, 2, 3], 1: [4, 5], 2: [4, 5, 6], 3: [7, 8, 9, 10, 11, 12, 13, 14, 15]}
    assert np.all(pk.meta[6:N - 1, :, 0] != 0) and np.all(pk.meta[:6, 6, 0] == 0)
    lm.pack(full + [_row(0, 5)], N)                       # lane 6 is free on knots 0..5
    lm.pack(full + [_row(N - 1, N - 1, 16, P.EQ)], N)     # and the whole terminal knot
    for extra in (_row(6, 6), _row(0, N - 2), _row(N - 1, N - 1, 17)):
        with pytest.raises(lm.Unsupported):
            lm.pack(full + [extra], N)
    four = [_cone(0, N - 2, 3), _cone(0, N - 2, 2), _cone(0, N - 2, 4), _cone(0, 5, 2)]
    with pytest.raises(lm.Unsupported):
        lm.pack(four + [_cone(5, 8, 2)], N)               # knot 5 holds four cones
    pk = lm.pack(four + [_cone(6, 8, 3)], N)
    assert pk.lanes[4] == [12, 13, 14] and np.all(pk.meta[6:9, 12:16, 3] == 3) and np.all(pk.meta[:6, 12:16, 3] == 2)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs, on the oracle
def _rows_figures(oracle, capsys, name, pr):
    """rows_guard and rows_ulp_sensitivity of the case, printed; the conditions every rows case shares."""
    g, ulp = lm.rows_guard(oracle, pr), lm.rows_ulp_sensitivity(oracle, pr)
    with capsys.disabled():    # (part of what the test is for: the figures show in a -q run too)
        print("\n%s: status %s, outer %s, nonzero duals %s, per row %s, one-ulp sensitivity %.1e" % (
            name, g["status"].tolist(), g["outer"].tolist(), g["nonzero"], g["nonzero_rows"], ulp))
    assert np.all(g["status"] == 1) and not g["capped"]
    assert g["outer"][0].max() >= 3
    assert ulp <= lm.ULP_BOUND      # the oracle agrees with itself far below the tolerance the device is held to
    return g


@pytest.mark.parametrize("sid,variant", ROW_CASES)
def test_rows10_case_is_not_vacuous(oracle, capsys, sid, variant):
    """Conditions on the INPUTS (seed and fraction per case are tuned until they hold, lane16_matrix.ROWS10; never relaxed):
    every solve succeeds below the penalty cap, the cold solve of some instance takes >= 3 outer iterations, the final
    duals of the LINEAR-INEQ block, of the cone and of the box are nonzero in at least one instance each, and the oracle's own
    answers move by less than ULP_BOUND when x0 moves by one unit in the last place (lane16_matrix.rows_ulp_sensitivity)."""
    pr = lm.rows_problem(lm.SHAPE_BY_ID[sid], variant)
    assert pr.x0.shape[0] == lm.B and pr.rp.N == N
    g = _rows_figures(oracle, capsys, "rows10 %s %s" % (sid, variant), pr)
    for kind in ("lin", "soc", "box"):
        assert g["nonzero"][kind] >= 1, kind


@pytest.mark.parametrize("sid", [lm.shape_id(s) for s in lm.QUAD_SHAPES])
def test_quads_case_is_not_vacuous(oracle, capsys, sid):
    """The same conditions with every one of the five cones binding in some instance, and every one of the four linear rows in
    a spare lane of a cone quad ending with a nonzero dual in some instance (per ROW, not per block)."""
    pr = lm.quads_problem(lm.SHAPE_BY_ID[sid])
    g = _rows_figures(oracle, capsys, "quads %s" % sid, pr)
    for kind in ("soc4", "soc2", "soc3x", "soc2m", "soc3m", "lin", "box", "xub"):    # (xub: lane 14, a linear row before the cone takes it)
        assert g["nonzero"][kind] >= 1, kind
    assert min(g["nonzero_rows"]["lin"]) >= 1


@pytest.mark.parametrize("sid", [lm.shape_id(s) for s in lm.SHAPES])
def test_track_case_is_not_vacuous(oracle, capsys, sid):
    """The tracking loop: every solve succeeds below the penalty cap; the cone, the linear block and the box hold a nonzero dual
    after EVERY solve of the loop, the state bound after at least one."""
    tp = lm.track_problem(lm.SHAPE_BY_ID[sid])
    g, (ulp, ulp_x0) = lm.track_guard(oracle, tp), lm.track_ulp_sensitivity(oracle, tp)
    with capsys.disabled():
        print("\ntrack %s: status %s, outer %s, instances with nonzero duals per solve %s, one-ulp sensitivity %.1e (x0 of a step %.1e)" % (
            sid, g["status"].tolist(), g["outer"].tolist(), {k: v.tolist() for k, v in g["nonzero"].items()}, ulp, ulp_x0))
    assert ulp <= lm.ULP_BOUND and ulp_x0 <= lm.X0_ULP_BOUND
    assert g["status"].shape == (1 + lm.TRACK_STEPS, lm.B) and np.all(g["status"] == 1) and not g["capped"]
    for kind in ("soc", "lin", "box"):
        assert np.all(g["nonzero"][kind] >= 1), kind
    assert g["nonzero"]["xub"].max() >= 1
