"""The pair blocks of gen_dpp_blocks.py (SGP, GTWP, CTGP0), checked without a GPU: the emitted instruction lists are run
as index tables.  Every element of S, W, Qxx and [Qux Quu] must be owned by exactly one DPP row of a pair, and the chain
of FMAs that forms an element must be the four-row block's, term for term and in the same order."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_dpp_blocks", os.path.join(ROOT, "altro-mpc-icra2021_amd", "csrc", "gen_dpp_blocks.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

NX, NU = 12, 4
FMAC = re.compile(r"v_fmac_f64_dpp %\[(\w+)\], %\[(\w+)\], %\[(\w+)\] row_newbcast:(\d+)")


def blocks():
    txt = gen.gen(NX, NU)
    out = {}
    for name, body in re.findall(r"void (\w+)\(.*?asm volatile\((.*?)\n      :", txt, flags=re.S):
        out[name] = [(a, b, c, int(k)) for a, b, c, k in FMAC.findall(body)]
    rl = int(re.search(r"RLP = (\d+)", txt).group(1))
    rq = int(re.search(r"RQP = (\d+)", txt).group(1))
    return out, rl, rq


def idx(s):
    return int(re.sub(r"\D", "", s))


def chains(ops):
    """accumulator -> list of (dpp operand, plain operand, broadcast lane) in program order"""
    ch = {}
    for acc, sd, sp, k in ops:
        ch.setdefault(idx(acc), []).append((idx(sd), idx(sp), k))
    return ch


def test_pair_rows_own_every_element_once():
    """Ownership as the emitted blocks have it.  GTWP's accumulator t takes its broadcast from lane t of the permuted
    operand gp, and the kernel puts column r*RLP + t (t < RLP) or NX + r*RQP + (t - RLP) of G on that lane in row r of a
    pair (backward_pair: pc); so the rows of H = [Qxx; Qux Quu] the two rows of a pair produce are read off the
    block's accumulators and broadcast lanes.  They must tile 0..NX+NU-1 exactly once; the same for W through SGP's
    accumulators (slot RLP: the vector s, row 0 only) and for S through CTGP0's."""
    B, RL, RQ = blocks()
    assert (RL, RQ) == (6, 2)
    slots = sorted(chains(B["GTWP"]))                       # accumulators the block writes
    assert slots == list(range(RL + RQ))
    assert all(k == t for t, ch in chains(B["GTWP"]).items() for (_, _, k) in ch)      # slot t <- lane t of gp
    col = lambda r, t: r * RL + t if t < RL else NX + r * RQ + (t - RL)                # backward_pair's pc
    rows_h = [col(r, t) for r in range(2) for t in slots]
    assert sorted(rows_h) == list(range(NX + NU))           # every row of H once
    w_slots = sorted(chains(B["SGP"]))
    assert w_slots == list(range(RL + 1))
    rows_w = [r * RL + t for r in range(2) for t in w_slots if t < RL] + [NX]          # slot RL: s, owned by row 0
    assert sorted(rows_w) == list(range(NX + 1))
    s_slots = sorted(chains(B["CTGP0"]))
    assert s_slots == list(range(RL))                       # CTGP0 updates the Qxx slots only
    assert sorted(r * RL + t for r in range(2) for t in s_slots) == list(range(NX))
    # every product of a chain reads the slot it accumulates into (SGP) or the whole gathered W (GTWP): no slot is
    # fed from another row's operand
    assert all(sd == t for t, ch in chains(B["SGP"]).items() for (sd, _, _) in ch)
    assert all(sorted(set(g for (g, _, _) in ch)) == list(range(NX)) for ch in chains(B["GTWP"]).values())


def test_pair_blocks_run_the_four_row_chains_in_order():
    B, RL, RQ = blocks()
    sg, sgp = chains(B["SG"]), chains(B["SGP"])
    gtw, gtwp = chains(B["GtW"]), chains(B["GTWP"])
    ctg, ctgp = chains(B["CTG0"]), chains(B["CTGP0"])
    for r in range(2):
        # W row i = r*RL + t: SG's w[i] += bcast_k(Sx[i]) g[k]; the pair block's slot t holds that row, slot RL the vector s
        for t in range(RL + 1):
            i = NX if t == RL else r * RL + t
            if t == RL and r != 0:
                continue      # only row 0 of the pair owns s; the other row's slot carries zeros
            assert [(k, g) for (_, g, k) in sgp[t]] == [(k, g) for (_, g, k) in sg[i]], ("SG", r, t)
            assert all(sd == t for (sd, _, _) in sgp[t]) and all(sd == i for (sd, _, _) in sg[i])
        # H row i: GtW's h[i] += bcast_i(g[k]) w[k]; the pair block broadcasts from lane t of the permuted gp (column i there)
        for t in range(RL + RQ):
            i = r * RL + t if t < RL else NX + r * RQ + (t - RL)
            assert [(g, w) for (g, w, _) in gtwp[t]] == [(g, w) for (g, w, _) in gtw[i]], ("GtW", r, t)
            assert all(k == t for (_, _, k) in gtwp[t]) and all(k == i for (_, _, k) in gtw[i])
        # S row i: CTG0's h[i] += bcast_i(r[a]) kd[a]
        for t in range(RL):
            i = r * RL + t
            assert [(a, b) for (a, b, _) in ctgp[t]] == [(a, b) for (a, b, _) in ctg[i]], ("CTG0", r, t)
            assert all(k == t for (_, _, k) in ctgp[t]) and all(k == i for (_, _, k) in ctg[i])
