"""The oracle's projected-Newton polish (oracle/altro_oracle.c projected_newton, multiplier_projection) against the dense
yardstick tests/polish_ref.py, on every case of tests/polish_cases.py: CPU only.  The device tests (tests/test_polish_gpu.py)
compare csrc/pn_core.h with the same yardstick and with this oracle; what is decided here -- which case reaches which path,
which case the closed form applies to -- is decided from the oracle alone.

The cases with n + m > 32 end in "stack smashing detected" on the oracle as it was before this file: pn_row evaluated a BOX
(2 (n + m) rows) into double cv[64]."""
import numpy as np
import pytest

import polish_cases as PC
import polish_ref


def _print_ratios(tag, ratios):
    print("%-22s %s" % (tag, "  ".join("%s %.3g" % kv for kv in ratios.items())))


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick itself
def test_yardstick_projection_is_a_projection():
    """project() lands on {D z = c}, moves nothing that is already there, and its displacement has no part outside
    range(H^-1 D'); out_of_range() returns the whole norm of a vector H-orthogonal to that range."""
    c = PC.case("l16-rows")
    ref = polish_ref.PolishRef(PC.instance(c, 0))
    rng = np.random.default_rng(0)
    z = ref.zref + rng.standard_normal(ref.len)
    act = ref.active_rows(z, 1e-3)
    zs = ref.project(z, act)
    scale = np.abs(act.D).sum(axis=1).max() * np.abs(z).max()
    assert np.abs(act.D @ zs - act.c).max() <= 64 * polish_ref.U_ROUND * scale
    act_s = polish_ref.Active(act.D, act.c, act.D @ zs - act.c, act.labels, act.block_rows, act.margin)
    assert np.abs(ref.project(zs, act_s) - zs).max() <= 64 * polish_ref.U_ROUND * scale
    disp = np.linalg.norm(np.sqrt(ref.H) * (zs - z))
    assert ref.out_of_range(zs - z, act.D) <= 64 * polish_ref.U_ROUND * disp
    # a vector in the null space of D, scaled by H^-1/2: H-orthogonal to range(H^-1 D')
    W = act.D / np.sqrt(ref.H)
    v = rng.standard_normal(ref.len)
    v -= np.linalg.pinv(W) @ (W @ v)
    out = ref.out_of_range(v / np.sqrt(ref.H), act.D)
    assert abs(out - np.linalg.norm(v)) <= 1e-12 * np.linalg.norm(v)


def test_yardstick_handles_duplicated_rows():
    """lo == hi puts the same row into D twice with opposite signs: S is singular, the pseudo-inverse projection is the
    projection onto the same set, and the gain stays finite."""
    c = PC.case("l16-dup")
    ref = polish_ref.PolishRef(PC.instance(c, 0))
    tw, _ = PC.oracle_pair(c.id, 0)
    z0 = ref.pack(tw.X, tw.U)
    act = ref.active_rows(z0, 1e-3)
    assert np.linalg.matrix_rank(act.D) < act.D.shape[0]
    zs = ref.project(z0, act)
    assert np.abs(act.D @ zs - act.c).max() <= 1e-13
    keep = [i for i, lab in enumerate(act.labels) if not (lab[0] == "lo" and ("hi", lab[1], lab[2]) in act.labels)]
    sub = polish_ref.Active(act.D[keep], act.c[keep], act.d[keep], [act.labels[i] for i in keep], act.block_rows, act.margin)
    assert np.abs(ref.project(z0, sub) - zs).max() <= 1e-13
    assert np.isfinite(ref.gain(act.D)) and ref.gain(act.D) < 1e3


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against it
@pytest.mark.parametrize("cid", PC.CASE_IDS)
def test_oracle_polish_against_the_yardstick(cid):
    """Range, closed form (where admissible) and both dual residuals of the oracle's polish: error / bound, each at most 1."""
    c = PC.case(cid)
    for b in range(c.batch):
        tw, po = PC.oracle_pair(cid, b)
        assert tw.status == 1 and po.pn_ran == 1 and po.pn_failed == 0 and po.pn_dual_failed == 0, (cid, b)
        assert (tw.iterations, tw.box_duals.tobytes()) == (po.iterations, po.box_duals.tobytes())     # the AL stage is the twin's
        ok, why = PC.admissibility(c, b)
        ratios = PC.judge(c, b, (tw.X, tw.U), (po.X, po.U), po.box_duals, po.row_duals, po.r0, po.r1, ok)
        _print_ratios("%s[%d]%s" % (cid, b, "" if ok else " (closed form n/a: %s)" % why), ratios)
        assert all(v <= 1.0 for v in ratios.values()), (cid, b, ratios)
        if "rho1e-8" in cid:    # the refinement converges at once: the closed form must apply
            assert ok and po.status == 1, (cid, b, why)


def test_at_most_one_inadmissible_case_per_backend():
    bad = {"lane16": [], "wide": []}
    for cid in PC.CASE_IDS:
        c = PC.case(cid)
        why = [PC.admissibility(c, b)[1] for b in range(c.batch)]
        if any(why):
            bad[c.backend].append((cid, why))
    print("inadmissible for the closed form:", bad)
    assert len(bad["lane16"]) <= 1 and len(bad["wide"]) <= 1, bad


def _reached(c):
    """The paths of pn_core.h the case reaches, from the yardstick's active set at the oracle's AL-stage trajectory."""
    got = set()
    if c.N > 64:
        got.add("N>64")
    if c.n + c.m > 32:
        got.add("n+m>32")
    if c.box_k0 > 0:
        got.add("box_k0>0")
    if c.ltv:
        got.add("per-knot dynamics")
    if c.backend == "lane16" and c.zmax is not None:
        bounded = int(np.sum(np.isfinite(c.zmax) | np.isfinite(c.zmin)))
        if 2 * c.n + 2 * bounded + (16 if c.rows else 0) == PC.BMAX:
            got.add("bm==BMAX")
    for b in range(c.batch):
        tw, po = PC.oracle_pair(c.id, b)
        ref = polish_ref.PolishRef(PC.instance(c, b))
        act = ref.active_rows(ref.pack(tw.X, tw.U), c.opts.get("active_set_tolerance_pn", 1e-3))
        labels = set(act.labels)
        stage0 = sum(1 for kind, k, _ in act.labels if k == 0 and kind in ("hi", "lo", "row"))
        if 2 * c.n + stage0 > 64:
            assert act.block_rows[0] == 2 * c.n + stage0
            got.add("rows>64")
        for kind, k, j in act.labels:
            if kind == "lo":
                got.add("lower side")
            if kind in ("hi", "lo") and j < c.n:
                got.add("state bound")
            if kind in ("hi", "lo") and k == c.N - 1:
                got.add("terminal row")
            if kind == "lo" and ("hi", k, j) in labels:
                got.add("duplicated row")
            if kind == "row":
                blk = c.rows[j[0]]
                if blk.equality and k == c.N - 1:
                    got.add("terminal equality")
                if not blk.equality:
                    got.add("linear rows")
        if po.pn_failed:
            got.add("failed=1")
    return got


@pytest.mark.parametrize("cid", PC.CASE_IDS + PC.FAIL_IDS)
def test_cases_reach_their_paths(cid):
    c = PC.case(cid)
    got = _reached(c)
    print(cid, "(%s, (%d, %d), N = %d) reaches:" % (c.backend, c.n, c.m, c.N), sorted(got))
    assert c.reaches and set(c.reaches) <= got, (cid, set(c.reaches) - got)


def test_every_listed_path_has_a_case_on_its_backend():
    have = {(PC.case(cid).backend, r) for cid in PC.CASE_IDS + PC.FAIL_IDS for r in PC.case(cid).reaches}
    for backend in ("lane16", "wide"):
        for path in ("N>64", "lower side", "linear rows", "terminal equality", "duplicated row", "failed=1", "state bound", "terminal row", "box_k0>0"):
            assert (backend, path) in have, (backend, path)
    for path in ("rows>64", "n+m>32", "per-knot dynamics"):
        assert ("wide", path) in have
    assert ("lane16", "bm==BMAX") in have
    # the refusal: one linear row more than the (12, 4) case at BMAX
    r = PC.refusal_case()
    bounded = int(np.sum(np.isfinite(r.zmax) | np.isfinite(r.zmin)))
    assert 2 * r.n + 2 * bounded + 16 > PC.BMAX and 2 * r.n + 2 * bounded == PC.BMAX


@pytest.mark.parametrize("cid", PC.FAIL_IDS)
def test_oracle_reports_a_failed_factorisation(cid):
    """lo == hi on a control, dt R = 1, rho_primal = rho_chol = 0: the two sides give the pivots 1 and 1 - 1 = 0.  The polish
    reports failed = 1, leaves the AL-stage trajectory as it is and the status below SOLVE_SUCCEEDED."""
    c = PC.case(cid)
    assert c.dt * c.R[0] == 1.0 and c.opts["rho_primal"] == 0.0 and c.opts["rho_chol"] == 0.0
    for b in range(c.batch):
        tw, po = PC.oracle_pair(cid, b)
        assert po.pn_ran == 1 and po.pn_failed == 1
        assert po.X.tobytes() == tw.X.tobytes() and po.U.tobytes() == tw.U.tobytes()
        assert po.c_max > c.opts["constraint_tolerance"] and po.status == 0 and po.pn_residual > c.opts["constraint_tolerance"]
        assert po.pn_dual_failed == 1 and po.r0 == 0.0 and po.r1 == 0.0
