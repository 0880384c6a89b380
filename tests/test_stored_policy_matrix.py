"""The table of tests/stored_policy_matrix.py, checked without a GPU: (a) its restatement of the LDS carve-ups of k_cov_wide and
k_ctg_wide against the source and at the sizes each case is in the table for; (b) the solve kernel every case runs on, whose gains
the calls read, has its line in tests/wide_matrix.py; (c) the inputs of every case are worth comparing on -- solved, below the
penalty cap, a control on its bound with a positive dual in every instance, a nonzero dual on the LINEAR rows -- on the CPU
oracle alone.  Each case prints its statuses, iteration counts and what binds."""
import os
import re

import numpy as np
import pytest

import stored_policy_matrix as sp
import wide_matrix as wm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "altro-mpc-icra2021_amd", "csrc")


def source_formula(header, name):
    """the return expression of `name` in `header`, with its declarations of np, mp, mq checked to be the padded sizes"""
    src = open(os.path.join(CSRC, header)).read()
    body = re.search(r"inline size_t %s\(int n, int m\) \{(.*?)\n\}" % name, src, re.S).group(1)
    assert "np = (size_t)altro_wide::pad16(n)" in body and "mq = (size_t)((m + 3) & ~3)" in body, body
    return re.search(r"return (.*?);", body).group(1)


def test_lds_mirror_against_the_source_and_at_the_sizes_of_the_table():
    """the two formulas as the headers state them, evaluated in Python on every (n, m) the library takes, equal the restatement;
    the table's byte counts; which side of the 64 KB a kernel gets unasked each case is on; Tt sized by mp only at (12, 20)"""
    cov, ctg = source_formula("covariance.h", "covw_lds_doubles"), source_formula("cost_to_go.h", "ctgw_lds_doubles")
    assert cov == "2 * np * np + (np > mp ? np : mp) * np + 2 * mq * np + np * mp" and ctg == "2 * np * np + np * (np + 1) + 2 * mq * np"
    for n in range(1, 65):
        for m in range(1, 33):
            np_, mp, mq = wm._pad16(n), wm._pad16(m), (m + 3) & ~3
            assert sp.covw_lds_doubles(n, m) == 2 * np_ * np_ + (np_ if np_ > mp else mp) * np_ + 2 * mq * np_ + np_ * mp
            assert sp.ctgw_lds_doubles(n, m) == 2 * np_ * np_ + np_ * (np_ + 1) + 2 * mq * np_
    for (n, m), (bc, bg) in sp.LDS.items():
        assert (8 * sp.covw_lds_doubles(n, m), 8 * sp.ctgw_lds_doubles(n, m)) == (bc, bg), (n, m)
    assert set(sp.LDS) == {sp.shape(s) for s in sp.CASES} | {(64, 16)}
    assert sp.LDS[40, 6][1] < sp.LDS_UNASKED < sp.LDS[40, 6][0]                      # cost-to-go just under, covariance just over
    assert sp.LDS_UNASKED < sp.LDS[48, 13][1] < sp.LDS[48, 32][1] < sp.LDS[64, 16][1] and sp.LDS[48, 32][0] < sp.LDS[64, 16][0]
    assert [s for s in sp.CASES if wm._pad16(sp.shape(s)[1]) > wm._pad16(sp.shape(s)[0])] == ["wide(12,20)"]
    assert [wm._pad16(sp.shape(s)[0]) for s in sp.CASES] == [48, 48, 16, 48]
    # the sweeps of wide(48,13) read the dynamics from memory: four waves' copies of [A | B] do not fit (evaluate.h evalw_lds_fits)
    assert 4 * 8 * (48 | 1) * (48 + 13) > sp.LDS_UNASKED >= 4 * 8 * (12 | 1) * (12 + 20)


def test_every_case_has_its_solve_in_the_wide_matrix():
    """the gains the calls read come from a solve kernel that tests/wide_matrix.py checks against the oracle at that (n, m), with
    rows and box-only; (12, 20) runs wide_kernel<0, false> at np = 16"""
    for s in sp.CASES:
        n, m = sp.shape(s)
        assert "%dx%d-r10" % (n, m) in wm.CASE_BY_ID and "%dx%d" % (n, m) in wm.BOX_BY_ID, s
        for name in (s,) + ((s + sp.BOXONLY,) if s in sp.ROWS_CASES else ()):
            cs, _, con, _ = sp.build(name, True)
            nrows = sum(c.A.shape[2] for c in cs.cons if c.kind != "box")
            assert (nrows > 0) == (con is not None) and (cs.B, cs.N) == (sp.B, sp.N) == (3, 5)
            assert wm.instantiation(n, m, nrows) in (wm.CASE_BY_ID["%dx%d-r10" % (n, m)].inst(), wm.BOX_BY_ID["%dx%d" % (n, m)].inst())
            assert wm.lds_bytes(n, m, nrows) <= wm.LDS_LIMIT
    c = wm.CASE_BY_ID["12x20-r10"]
    assert c.inst(False) == c.inst(True) == wm.BOX_BY_ID["12x20"].inst() == (0, False, 0, -1) and wm._pad16(c.n) == 16 < wm._pad16(c.m) == 32


ALL_RUNS = sp.RUNS + [q for q in sp.BOX_RUNS if q not in sp.RUNS]
ALL_IDS = [s + ("-pi" if pi else "-shared") for s, pi in ALL_RUNS]


@pytest.mark.parametrize("name,pi", ALL_RUNS, ids=ALL_IDS)
def test_case_is_not_vacuous(capsys, name, pi):
    """Conditions on the INPUTS (seed and bounds per case are tuned until they hold, stored_policy_matrix.TUNE; never relaxed):
    every instance solves with status 1 below the penalty cap and ends with a control on its bound and a positive dual there; the
    rows case has a nonzero dual on its LINEAR block in every instance; the cases with state bounds have a state side with a positive
    dual in some instance."""
    g = sp.guard(name, pi)
    with capsys.disabled():    # (part of what the test is for: the figures show in a -q run too)
        print("\n%s %s: status %s, iterations %s, control on its bound %s, state sides with a dual %s, LINEAR duals %s" % (
            name, "pi" if pi else "shared", g["status"].tolist(), g["iterations"].tolist(), g["on_bound"].tolist(), g["state_sides"].tolist(),
            None if g["lin"] is None else g["lin"].tolist()))
    assert np.all(g["status"] == 1) and not g["capped"]
    assert g["iterations"].max() <= 50        # (of the 60 the handles allow)
    assert g["on_bound"].all()
    assert (g["lin"] is not None) == (name in sp.ROWS_CASES) and (g["lin"] is None or g["lin"].all())
    base = name[:-len(sp.BOXONLY)] if name.endswith(sp.BOXONLY) else name
    if sp.TUNE[base]["xb"] is not None:
        assert g["state_sides"].max() >= 1
