"""The table of tests/scoring_matrix.py, checked without a GPU: (1) its restatement of the LDS rule of the scoring core against the
text of evaluate.h and wide_backend.h, at the sizes each case is in the table for; (2) the backend every case runs on and the
lane / row every block lands on, against tests/lane16_matrix.pack; (3) the guards (a) .. (h): the inputs of every case reach the
path the case is in the table for -- on numpy and the CPU oracle alone.  Each case prints what decides c_max where."""
import os
import re

import numpy as np
import pytest

import evaluate_al_ref as AR
import evaluate_grad_ref as GR
import evaluate_ref as ER
import lane16_matrix as lm
import scoring_matrix as sm
import wide_matrix as wm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "altro-mpc-icra2021_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def body_of(src, head):
    """the text of the member function that starts with `head`, up to the closing brace at its indentation"""
    i = src.index(head)
    return src[i:src.index("\n  }\n", i)]


# ---------------------------------------------------------------------------------------------- 1: the LDS rule
def test_lds_rule_against_the_source_and_at_the_sizes_of_the_table():
    """evalw_ld, evalw_lds_doubles, evalw_lds_bytes, evalw_lds_fits as evaluate.h states them; the slice offset of EvalWDynT; the
    table's bytes and which slice fits; (32, 32) asks for exactly the allowance, (40, 12) is the first shape past (40, 11)"""
    ev = source("evaluate.h")
    for line in ("inline int evalw_ld(int n, bool pad) { return pad ? n | 1 : n; }",
                 "inline size_t evalw_lds_doubles(int ld, int n, int m) { return (size_t)ld * (n + m); }",
                 "inline size_t evalw_lds_bytes(int ld, int n, int m) { return 4 * evalw_lds_doubles(ld, n, m) * sizeof(double); }",
                 "inline bool evalw_lds_fits(int ld, int n, int m, int ltv) { return !ltv && evalw_lds_bytes(ld, n, m) <= 65536; }",
                 "double* slice = eval_lds + (threadIdx.x >> 6) * evalw_lds_doubles(ld, P.n, P.m);",
                 "ld = evalw_ld(P.n, PAD);"):
        assert line in ev, line
    assert sm.LDS_UNASKED == 65536
    for name, t in sm.TABLE.items():
        n, m, ltv = t["n"], t["m"], t["ltv"]
        plain, padded = sm.evalw_lds_bytes(sm.evalw_ld(n, False), n, m), sm.evalw_lds_bytes(sm.evalw_ld(n, True), n, m)
        assert (plain, padded) == t["bytes"], name
        assert (sm.evalw_lds_fits(n, n, m, ltv), sm.evalw_lds_fits(n | 1, n, m, ltv)) == t["fits"], name
        assert sm.eval_lds(n, m, ltv) == (plain if t["fits"][0] else 0) and sm.eval_grad_lds(n, m, ltv) == (padded if t["fits"][1] else 0)
    T = sm.TABLE
    assert T["wide(32,32)"]["bytes"] == (65536, 67584) and T["wide(32,32)"]["fits"] == (True, False)          # exactly the allowance; split
    assert T["wide(32,30)"]["bytes"][1] == 65472 and T["wide(32,30)"]["fits"] == (True, True) and sm.evalw_ld(32, True) == 33
    assert T["wide(33,29)"]["bytes"] == (65472, 65472) and sm.evalw_ld(33, True) == 33                         # the pad is a no-op
    assert T["wide(40,12)"]["bytes"][0] == 66560 and sm.evalw_lds_fits(40, 40, 11, False) and not sm.evalw_lds_fits(40, 40, 12, False)
    assert sm.eval_lds(40, 12, False) == 0 and sm.eval_grad_lds(40, 12, False) == 0                            # the launches ask for 0 B
    assert sm.evalw_lds_fits(32, 32, 31, False) and not sm.evalw_lds_fits(33, 32, 31, False)                  # (32, 31) is split too
    assert not sm.evalw_lds_fits(33, 32, 32, False) and not sm.evalw_lds_fits(41, 40, 11, False)
    # the largest padded slice that fits at n = 32 is m = 30
    assert max(m for m in range(1, 33) if sm.evalw_lds_fits(33, 32, m, False)) == 30
    # evalw_dot: counts that are multiples of 8, tails of one and of five, m = 1
    assert (32 % 8, 32 % 8) == (0, 0) and (33 % 8, 29 % 8) == (1, 5) and (17 % 8, T["wide(17,1)"]["m"]) == (1, 1) and 64 % 8 == 0


def test_which_kernel_asks_for_which_slice():
    """wide_backend.h: lds_dyn is the plain rule; eval_lds is the plain slice where lds_dyn says so; eval_grad_lds is the padded
    slice under its own rule; evaluate, warm_start and simulate_policy launch with the first, evaluate_grad and evaluate_al with
    the second and tell their kernel whether there is a slice"""
    wb = source("wide_backend.h")
    assert "p.lds_dyn = altro::evalw_lds_fits(d.n, d.n, d.m, ltv) ? 1 : 0;" in wb
    assert "static size_t eval_lds(const altro::EvalW& p) { return p.lds_dyn ? altro::evalw_lds_bytes(p.n, p.n, p.m) : 0; }" in wb
    g = body_of(wb, "  static size_t eval_grad_lds(")
    assert "const int ld = altro::evalw_ld(p.n, true);" in g
    assert "return altro::evalw_lds_fits(ld, p.n, p.m, p.ltv) ? altro::evalw_lds_bytes(ld, p.n, p.m) : 0;" in g
    for fn, rule in (("evaluate_dev", "eval_lds"), ("warm_start_dev", "eval_lds"), ("simulate_policy_dev", "eval_lds"),
                     ("evaluate_grad_dev", "eval_grad_lds"), ("evaluate_al_dev", "eval_grad_lds")):
        b = body_of(wb, "  int %s(" % fn)
        assert "const size_t lds = %s(p);" % rule in b, fn
        assert ("eval_grad_lds" in b) == (rule == "eval_grad_lds") and b.count("dim3(256)") + b.count("block(256)") >= 1, fn
        if rule == "eval_grad_lds":
            assert "lds, stream, io, p, ncand, R, lds ? 1 : 0);" in b, fn


# ---------------------------------------------------------------------------------------------- 2: backends, lanes and rows
def test_backend_of_every_case():
    """the 16-lane shapes are those of supported_dims (altro_batch.hip); every other shape of the table runs one wave per instance"""
    src = source("altro_batch.hip")
    body = re.search(r"static bool supported_dims\(int n, int m\) \{(.*?)\n\}", src, re.S).group(1)
    assert sorted((int(a), int(b)) for a, b in re.findall(r"n == (\d+) && m == (\d+)", body)) == sorted(sm.LANE16_SHAPES)
    for name, t in sm.TABLE.items():
        assert (((t["n"], t["m"]) in sm.LANE16_SHAPES) == (t["backend"] == "16")), name
        assert t["N"] >= 3 and (t["backend"] == "16" or wm.MAX_ROWS == sm.MAX_ROWS)
    assert [sm.TABLE[s]["N"] for s in ("16-quads(6,6)", "wide(17,1)")] == [3, 3]        # the minimum horizon on both backends


@pytest.mark.parametrize("name", sm.QUADS)
def test_lane_placement_of_the_quads_cases(name):
    """lane16_matrix.pack on instance 0's blocks: every block on the lanes the table says; all 16 lanes own a row; lanes 0, 1 hold
    a cone row on knots 0 .. N-2 and an equality row at N-1; the spare lanes of cone quads hold inequality rows; (12, 4): n + m =
    16, the quad whose cone goes from dimension 2 to 3, 35 rows = two blocks of 16 and one of three live rows and a padded one;
    (6, 6): lanes 12 .. 15 own rows and hold no element"""
    cs, names, _ = sm.build(name)
    t = sm.TABLE[name]
    N = cs.N
    pk = lm.pack(sm.specs_of(cs), N, per_instance=True)
    assert {names[i]: l for i, l in pk.lanes.items()} == {k: v for k, v in sm.QUAD_LANES.items() if k in names}
    assert pk.con_inv == 0
    typ = pk.meta[:, :, 0]
    assert (typ != 0).any(axis=0).all()                                               # every lane owns a row at some knot
    assert (typ[:N - 1, :4] == 3).all() and (typ[N - 1, :2] == 1).all() and typ[N - 1, 2] == 2
    for lane in sm.QUAD_LANES["lin"]:
        assert (typ[:N - 1, lane] == 2).all() and (pk.meta[1:N - 1, lane, 3] > 0).all()   # a LINEAR row in the quad of a cone (lane 11: from knot 1)
    assert (typ[1:, 8:11] == 3).all() and (pk.meta[N - 1, 8:12, 3] == 3).all()          # the cone on the states reaches the terminal knot
    assert sorted({c.A.shape[2] for c in cs.cons if c.kind == "soc"}) == [2, 3, 4]
    eq = cs.cons[names.index("eq")]
    assert eq.eq and (eq.k0, eq.k1) == (N - 1, N - 1) and (np.abs(eq.b) > 1e-3).all()
    if name == "16-quads(12,4)":
        assert cs.n + cs.m == 16 and list(pk.meta[:, 12, 3]) == [2, 2, 2, 3, 3, 0] and list(typ[:, 14]) == [0, 0, 0, 3, 3, 0]
        rows = cs.B * t["ncand"]
        assert rows == 35 and -(-rows * 16 // 256) == 3 and rows - 32 == 3 and (-rows) % 4 == 1
    else:
        assert cs.n + cs.m == 12 and "soc2m" not in names and N == 3
        assert (typ[:, 12:] != 0).any(axis=0).all()
    assert all((c.A[0] != c.A[1]).any() for c in cs.cons if c.kind != "box")            # per-instance constraint data


def test_rows_of_wide_rows64():
    """Pn = 64, rows in order of addition, the p = 4 cone LAST at c0 = 60; per-knot dynamics; the equality rows on knots 1 .. N-2 with
    nonzero offsets, per instance and per knot; the second inequality block reaches the terminal knot"""
    cs, names, kw = sm.build("wide-rows64(20,5)")
    assert names == ["box", "lin24", "eq", "soc2", "lin26", "soc4"] and kw["per_knot_dyn"]
    assert sm.wide_rows(cs) == ([(0, 24), (24, 8), (32, 2), (34, 26), (60, 4)], 64) and sm.MAX_ROWS == 64
    assert (cs.A[:, 0] != cs.A[:, 1]).any() and (cs.A[0] != cs.A[1]).any()
    eq, l24, l26 = cs.cons[2], cs.cons[1], cs.cons[4]
    assert eq.eq and (eq.k0, eq.k1) == (1, cs.N - 2) and (np.abs(eq.b) > 1e-6).all() and (eq.A[0] != eq.A[1]).any() and (eq.A[:, 0] != eq.A[:, 1]).any()
    assert (l24.k0, l24.k1) == (0, cs.N - 2) and (l26.k0, l26.k1) == (2, cs.N - 1)
    for c in (l24, l26):                                                              # one block for the batch and the horizon
        assert (c.A == c.A[:1, :1]).all() and (c.b == c.b[:1, :1]).all()


# ---------------------------------------------------------------------------------------------- 3: the guards
def named(g, w):
    return [[g.names[i] if i >= 0 else "-" for i in row] for row in w]


@pytest.mark.parametrize("name", sm.CASES)
def test_inputs_reach_the_path(capsys, name):
    """Guards (a) .. (g) (seeds, margins and the factors of scoring_matrix.SCALE are tuned until they hold; never relaxed)"""
    g = sm.guards(name)
    cs, names = g.cs, g.names
    with capsys.disabled():
        print("\n%s: c_max decided by %s" % (name, named(g, g.winner)))
        for nm, c in g.cones.items():
            print("   %s inside / polar / boundary %s, decides c_max %d times" % (nm, c.branch.tolist(), c.decides))
    # a candidate well inside, one pushed out, one random
    assert (g.cmax[:, 0] <= g.cb[:, 0]).all() and (g.cmax[:, 1] > 1e-3).all()
    # (a) every cone: each branch somewhere, the arg-max row of c_max somewhere
    for nm, c in g.cones.items():
        assert (c.branch > 0).all() and c.decides > 0, nm
    assert (len(g.cones) > 0) == (name in sm.ORACLE_CASES)
    # (b) every equality block: a row with v < 0 decides c_max, and without the fabs that c_max moves by more than its bound
    for nm, e in g.eqs.items():
        assert (e.decides_neg & (g.cmax - e.drop > g.cb)).any(), nm
    assert (len(g.eqs) > 0) == (name in sm.ORACLE_CASES)
    if name in sm.QUADS:
        # (c) a LINEAR row in a spare lane of a cone quad decides c_max; both dimensions of the changing quad are violated
        assert (g.winner == names.index("lin")).any()
        if "soc2m" in names:
            assert g.cones["soc2m"].violated_knots.any() and g.cones["soc3m"].violated_knots.any()
        # (e) rows on the terminal knot are violated: the equality rows, the inequality row, the cone on the states
        assert g.terminal["eq"] > 1e-3 and g.terminal["xub"] > 1e-3 and g.terminal["soc3x"] > 1e-3
    if name == "wide-rows64(20,5)":
        # (d) the cone in rows 60 .. 63 is violated for a candidate of every instance, and row 63 alone moves P
        assert g.cones["soc4"].violated_instances.all()
        d, Pb = sm.row63_moves_P()
        assert (d > Pb).any(axis=1).all()
        assert g.terminal["lin26"] > 1e-3                                             # (e)
    if name == "wide(32,32)":
        box = cs.cons[0]                                                              # (e) a terminal state bound
        over = np.maximum(g.X[:, :, -1] - box.zmax[:, None, :cs.n], box.zmin[:, None, :cs.n] - g.X[:, :, -1])
        assert (box.k0, box.k1) == (0, cs.N - 1) and np.isfinite(box.zmax[:, :cs.n]).any() and over.max() > 1e-3
    if name == "wide(17,1)":
        assert (g.winner == names.index("lin")).any() and cs.cons[1].A.shape[2] == 2
    # (f) every row value is clear of its kink for every candidate (in units of the row's own rounding bound)
    assert (g.grad.margin >= 1e6).all()
    # (g) per-instance dynamics differ between the instances that share a block of four waves
    if name in sm.LDS_CASES:
        assert cs.B * sm.TABLE[name]["ncand"] == 9                                  # rows 0 .. 8: block 0 holds instances 0 and 1
        gap, bound = sm.swapped_rollout_gap(name)
        assert gap > 1e6 * bound


@pytest.mark.parametrize("name", sm.SOLVED_CASES)
def test_the_solves_behind_the_calls_end_regularly(capsys, name):
    """Guard (h) on the oracle: the short solve behind evaluate_al ends at its three outer iterations and the solve behind
    simulate_policy with status 1, both below the penalty cap, every instance with a nonzero dual of every constraint kind; the
    duals drawn from the short solve's reach every branch of the augmented Lagrangian"""
    cs, names, _ = sm.build(name)
    for short in (True, False):
        g = sm.solve_guard(name, short)
        with capsys.disabled():
            print("\n%s %s: status %s, outer %s, nonzero duals %s" % (name, "short" if short else "gains", g["status"].tolist(), g["outer"].tolist(),
                                                                      {k: v.astype(int).tolist() for k, v in g["nonzero"].items()}))
        assert not g["capped"]
        assert (g["status"] == (3 if short else 1)).all() and (not short or (g["outer"] == 3).all())
        assert all(v.all() for v in g["nonzero"].values()), g["nonzero"]
    lam0, mu, lam = sm.al_inputs(name)
    U = sm.candidates(name)
    y = AR.al(cs, ER.rollout(cs, U), U, lam, mu)
    assert AR.reaches_every_branch(cs, y.counts), y.counts
    # guard (f), the kink list of evaluate_al_ref (G): along the direction of the device test's central difference no candidate
    # sits on a kink of the augmented Lagrangian under the drawn duals
    D = np.random.default_rng(8).standard_normal(U.shape)
    X = ER.rollout(cs, U)
    yk = AR.al(cs, X, U, lam, mu, direction=(GR.tangent(cs, D, None), D))
    assert (yk.hmax > 0).all() and np.isfinite(yk.f3).all()


def test_what_runs_where():
    assert sm.SOLVED_CASES == sm.CASES
    assert set(sm.SPLIT) <= set(sm.SOLVED_CASES) and set(sm.ORACLE_CASES) == set(sm.QUADS) | {"wide-rows64(20,5)"}
