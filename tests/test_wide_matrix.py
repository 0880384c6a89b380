"""The table of tests/wide_matrix.py, checked without a GPU: (a) the Python restatement of wide_kernel_for only returns
instantiations that ALTRO_WIDE_KERNELS builds, and the table reaches every one of them; (b) the inputs of every case are
worth comparing on -- feasible, several outer iterations, every kind of constraint binding -- on the CPU oracle alone.
Each case prints its statuses, outer-iteration counts and which dual blocks are nonzero."""
import os
import re

import numpy as np
import pytest

import wide_matrix as wm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "altro-mpc-icra2021_amd", "csrc")


def built_instantiations():
    """The X(tu, MC, SM, NPC, PRC) tuples of ALTRO_WIDE_KERNELS in solve_wide.h."""
    src = open(os.path.join(CSRC, "solve_wide.h")).read()
    body = re.search(r"#define ALTRO_WIDE_KERNELS\(X\)((?:.*\\\n)*.*\n)", src).group(1)
    out = [(int(mc), sm == "true", int(npc), int(prc))
           for mc, sm, npc, prc in re.findall(r"X\(\s*\d+\s*,\s*(\d+)\s*,\s*(true|false)\s*,\s*(\d+)\s*,\s*(-?\d+)\s*\)", body)]
    assert len(out) == len(set(out)) >= 10
    return out


def test_dispatch_mirror_stays_inside_the_build_list_and_the_table_reaches_all_of_it():
    built = set(built_instantiations())
    reachable, reachable_plain = set(), set()
    for n in range(1, 65):
        for m in range(1, 33):
            for nrows in (0, 1, 16, 64):
                inst = wm.instantiation(n, m, nrows)
                assert inst in built, (n, m, nrows, inst)
                reachable.add(inst)
                if nrows == 0:
                    reachable_plain.add(inst)
    assert (4, False, 0, -1) not in reachable       # m <= 4, n > 16: the padded n is 32, 48 or 64, each with a kernel of its own
    assert reachable == built                        # nothing is built that the dispatch cannot return
    with_rows = {c.inst(ltv) for c in wm.CASES for ltv in (False, True)}
    box_only = {bc.inst() for bc in wm.BOX_CASES}
    for inst in sorted(built):
        if inst[3] == 0:                             # the "no rows" kernels of the m <= 4 class
            assert inst in box_only, inst
            continue
        assert inst in with_rows, inst
        if inst in reachable_plain:                  # (<12, true, 0, 16> and the m <= 4 kernels with rows never run box-only)
            assert inst in box_only, inst


def test_lds_mirror_at_the_documented_sizes():
    """Numbers solve_wide.h states for lds_layout: 51.6 -> 39.0 KB (of 1000 bytes) at n = 17..32, m <= 16 with the compact
    carve-up, and the 160 KB (of 1024) boundary of wide_backend.h prepare_launch."""
    assert 8 * wm.lds_doubles(32, 4, 0, False) == 51584 and wm.lds_bytes(32, 4, 0) == 39040
    assert wm.lds_bytes(64, 16, 12) == 160832 <= wm.LDS_LIMIT < wm.lds_bytes(64, 16, 13)
    assert wm.lds_bytes(64, 17, 0) > wm.LDS_LIMIT and wm.lds_bytes(64, 32, 0) > wm.LDS_LIMIT
    assert wm.lds_bytes(48, 32, 10) <= wm.LDS_LIMIT
    for c in wm.CASES:
        assert wm.lds_bytes(c.n, c.m, c.nrows(True), True) <= wm.LDS_LIMIT and wm.lds_bytes(c.n, c.m, c.nrows(False)) <= wm.LDS_LIMIT, c.id
    # (48, 32) is the largest m > 16 shape that fits: neither a larger padded n nor more rows than a few do
    assert wm.lds_bytes(49, 17, 0) > wm.LDS_LIMIT


@pytest.mark.parametrize("ltv", [False, True], ids=["ti", "ltv"])
@pytest.mark.parametrize("cid", [c.id for c in wm.CASES])
def test_rows_case_is_not_vacuous(oracle, capsys, cid, ltv):
    """Conditions on the INPUTS (seed and fraction per case are tuned until they hold, wide_matrix.CASES; never relaxed):
    every solve succeeds below the penalty cap, the cold solve of some instance takes >= 3 outer iterations, and the final
    duals of the LINEAR-INEQ block, of the cone and of the box are nonzero in at least one instance each."""
    case = wm.CASE_BY_ID[cid]
    pr = wm.rows_problem(case, ltv)
    g = wm.rows_guard(oracle, pr)
    with capsys.disabled():    # (part of what the test is for: the figures show in a -q run too)
        print("\n%s %s <%s>: rows %d, status %s, outer %s, nonzero duals %s" % (
            cid, "per-knot" if ltv else "time-invariant", ", ".join(str(v).lower() for v in case.inst(ltv)), case.nrows(ltv),
            g["status"].tolist(), g["outer"].tolist(), g["nonzero"]))
    assert sum(c.A.shape[0] for c in pr.rp.constraints if c.A is not None) == case.nrows(ltv) <= wm.MAX_ROWS
    assert np.all(g["status"] == 1) and not g["capped"]
    assert g["outer"][0].max() >= 3
    for kind in ("lin", "soc", "box"):
        assert g["nonzero"][kind] >= 1, kind
    if case.rows == wm.MAX_ROWS:
        assert g["nonzero"]["fill"] == 0     # slack by construction: the case is about the row COUNT


def test_lds_boundary_case_is_not_vacuous(oracle, capsys):
    """(64, 16) with 12 rows, the last problem that fits the LDS: the same conditions (its two fill rows are slack)."""
    g = wm.rows_guard(oracle, wm.rows_problem(wm.LDS_FITS, False))
    with capsys.disabled():
        print("\n%s: status %s, outer %s, nonzero duals %s" % (wm.LDS_FITS.id, g["status"].tolist(), g["outer"].tolist(), g["nonzero"]))
    assert np.all(g["status"] == 1) and not g["capped"] and g["outer"][0].max() >= 3
    assert all(g["nonzero"][kind] >= 1 for kind in ("lin", "soc", "box"))


@pytest.mark.parametrize("bid", [bc.id for bc in wm.BOX_CASES])
def test_box_case_is_not_vacuous(oracle, capsys, bid):
    """The box-only MPC loop: every solve succeeds below the penalty cap, the cold solve of some instance takes >= 3 outer
    iterations, and after every solve of the loop some instance holds a nonzero box dual (a control sits on its bound)."""
    bc = wm.BOX_BY_ID[bid]
    g = wm.box_guard(oracle, bc)
    with capsys.disabled():
        print("\n%s box-only <%s>: u_bnd %g, status %s, outer %s, instances with box duals %s" % (
            bid, ", ".join(str(v).lower() for v in bc.inst()), bc.u_bnd, g["status"].tolist(), g["outer"].tolist(), g["box"].tolist()))
    assert np.all(g["status"] == 1) and not g["capped"]
    assert g["outer"][0].max() >= 3
    assert np.all(g["box"] >= 1)
