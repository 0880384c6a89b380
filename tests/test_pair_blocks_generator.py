"""The split blocks of gen_dpp_blocks.py (Split4 / Split2: SG, GTW, CTG0), checked without a GPU: the emitted instruction
lists are run as index tables.  Every element of S, W, Qxx and [Qux Quu] must be owned by exactly one of the R DPP rows
that share an instance, and the chain of FMAs that forms an element must be the four-row block's, term for term and in the
same order -- for R = 4 (the lone form) and R = 2 (the pair form), at every size the generator emits."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_dpp_blocks", os.path.join(ROOT, "altro-mpc-icra2021_amd", "csrc", "gen_dpp_blocks.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

FMAC = re.compile(r"v_fmac_f64_dpp %\[(\w+)\], %\[(\w+)\], %\[(\w+)\] row_newbcast:(\d+)")
BLOCK = re.compile(r"void (\w+)\(.*?asm volatile\((.*?)\n      :", flags=re.S)
CASES = [(nx, nu, R) for (nx, nu) in gen.SIZES for R in (2, 4)]


def parse(txt):
    return {name: [(a, b, c, int(k)) for a, b, c, k in FMAC.findall(body)] for name, body in BLOCK.findall(txt)}


def blocks(NX, NU, R):
    """the four-row blocks of Blk<NX,NU>, the blocks of its nested struct Split<R>, and that struct's RL, RQ"""
    txt = gen.gen(NX, NU)
    m = re.search(r"struct Split%d \{\n\s*static constexpr int RL = (\d+), RQ = (\d+);(.*?)\n  \};\n" % R, txt, flags=re.S)
    return parse(txt[:txt.index("struct Split")]), parse(m.group(3)), int(m.group(1)), int(m.group(2))


def idx(s):
    return int(re.sub(r"\D", "", s))


def chains(ops):
    """accumulator -> list of (dpp operand, plain operand, broadcast lane) in program order"""
    ch = {}
    for acc, sd, sp, k in ops:
        ch.setdefault(idx(acc), []).append((idx(sd), idx(sp), k))
    return ch


def owned(NX, NU, R, RL, RQ, r, t):
    """Row of H = [Qxx; Qux Quu] that slot t of DPP row r holds (backward_split's pc), or None where the kernel masks the
    slot off (its pv: R*RL > NX or R*RQ > NU leaves the last rows' spare slots empty)."""
    if t < RL:
        return r * RL + t if r * RL + t < NX else None
    return NX + r * RQ + (t - RL) if r * RQ + (t - RL) < NU else None


def test_pair_rows_own_every_element_once():
    """Ownership as the emitted blocks have it.  GTW's accumulator t takes its broadcast from lane t of the permuted
    operand gp, and the kernel puts column r*RL + t (t < RL) or NX + r*RQ + (t - RL) of G on that lane in row r of the R
    (backward_split: pc); so the rows of H = [Qxx; Qux Quu] the R rows produce are read off the block's accumulators and
    broadcast lanes.  They must tile 0..NX+NU-1 exactly once; the same for W through SG's accumulators (slot RL: the
    vector s, row 0 only) and for S through CTG0's.  Checked for R = 2 and R = 4 at every size of the generator."""
    for NX, NU, R in CASES:
        check_ownership(NX, NU, R)


def check_ownership(NX, NU, R):
    _, S, RL, RQ = blocks(NX, NU, R)
    assert (RL, RQ) == (-(-NX // R), -(-NU // R))
    if (NX, NU) == (12, 4):
        assert (RL, RQ) == {2: (6, 2), 4: (3, 1)}[R]
    slots = sorted(chains(S["GTW"]))                        # accumulators the block writes
    assert slots == list(range(RL + RQ))
    assert all(k == t for t, ch in chains(S["GTW"]).items() for (_, _, k) in ch)       # slot t <- lane t of gp
    rows_h = [owned(NX, NU, R, RL, RQ, r, t) for r in range(R) for t in slots]
    assert sorted(i for i in rows_h if i is not None) == list(range(NX + NU))           # every row of H once
    w_slots = sorted(chains(S["SG"]))
    assert w_slots == list(range(RL + 1))
    rows_w = [r * RL + t for r in range(R) for t in w_slots if t < RL and r * RL + t < NX] + [NX]   # slot RL: s, owned by row 0
    assert sorted(rows_w) == list(range(NX + 1))
    s_slots = sorted(chains(S["CTG0"]))
    assert s_slots == list(range(RL))                       # CTG0 updates the Qxx slots only
    assert sorted(r * RL + t for r in range(R) for t in s_slots if r * RL + t < NX) == list(range(NX))
    # every product of a chain reads the slot it accumulates into (SG) or the whole gathered W (GTW): no slot is
    # fed from another row's operand
    assert all(sd == t for t, ch in chains(S["SG"]).items() for (sd, _, _) in ch)
    assert all(sorted(set(g for (g, _, _) in ch)) == list(range(NX)) for ch in chains(S["GTW"]).values())


def test_pair_blocks_run_the_four_row_chains_in_order():
    for NX, NU, R in CASES:
        check_chains(NX, NU, R)


def check_chains(NX, NU, R):
    B, S, RL, RQ = blocks(NX, NU, R)
    sg, sgs = chains(B["SG"]), chains(S["SG"])
    gtw, gtws = chains(B["GtW"]), chains(S["GTW"])
    ctg, ctgs = chains(B["CTG0"]), chains(S["CTG0"])
    for r in range(R):
        # W row i = r*RL + t: SG's w[i] += bcast_k(Sx[i]) g[k]; the split block's slot t holds that row, slot RL the vector s
        for t in range(RL + 1):
            i = NX if t == RL else r * RL + t
            if (t == RL and r != 0) or (t < RL and i >= NX):
                continue      # only row 0 of the R owns s, and a slot past row NX-1 owns nothing: those carry zeros
            assert [(k, g) for (_, g, k) in sgs[t]] == [(k, g) for (_, g, k) in sg[i]], ("SG", NX, NU, R, r, t)
            assert all(sd == t for (sd, _, _) in sgs[t]) and all(sd == i for (sd, _, _) in sg[i])
        # H row i: GtW's h[i] += bcast_i(g[k]) w[k]; the split block broadcasts from lane t of the permuted gp (column i there)
        for t in range(RL + RQ):
            i = owned(NX, NU, R, RL, RQ, r, t)
            if i is None:
                continue
            assert [(g, w) for (g, w, _) in gtws[t]] == [(g, w) for (g, w, _) in gtw[i]], ("GtW", NX, NU, R, r, t)
            assert all(k == t for (_, _, k) in gtws[t]) and all(k == i for (_, _, k) in gtw[i])
        # S row i: CTG0's h[i] += bcast_i(r[a]) kd[a]
        for t in range(RL):
            i = r * RL + t
            if i >= NX:
                continue
            assert [(a, b) for (a, b, _) in ctgs[t]] == [(a, b) for (a, b, _) in ctg[i]], ("CTG0", NX, NU, R, r, t)
            assert all(k == t for (_, _, k) in ctgs[t]) and all(k == i for (_, _, k) in ctg[i])
