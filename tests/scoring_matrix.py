"""The calls built on the scoring core (csrc/evaluate.h, DESIGN.md 7l / 7q: evaluate, evaluate_grad, evaluate_al, warm_start,
simulate_policy) as a table: the row tables, LDS sizes and shapes at which their kernels take a path the seven cases of
tests/evaluate_ref.py do not reach.  Shared by tests/test_scoring_matrix.py (the LDS rule against the source, the lane placement
against tests/lane16_matrix.pack, and the conditions on the INPUTS, on numpy and the CPU oracle alone) and
tests/test_scoring_matrix_gpu.py (the device against the numpy yardsticks of the five sibling test files).

 - evalw_ld / evalw_lds_bytes / evalw_lds_fits restate evaluate.h; TABLE holds the bytes each case is in the table for.
 - the builders return an evaluate_ref.Case.  Every inequality row, cone and equality row gets its offset from a BASE trajectory
   (the rollout of small controls): the base is strictly inside every inequality and on every equality, so each problem is
   feasible by construction whatever the seed, and the offsets of the equality rows are nonzero.
 - SCALE: per (case, instance) factors on whole constraint blocks.  Scaling a block's (A, b) by s > 0 multiplies its violation
   by s and leaves the branch of every cone value where it is, so the factors only decide which block is the arg-max row of
   c_max where; they were chosen on the numpy yardstick until the guards of tests/test_scoring_matrix.py hold.
Nothing here depends on the device."""
import functools
from types import SimpleNamespace as NS

import numpy as np

import evaluate_ref as ER
import evaluate_grad_ref as GR
from wide_matrix import PENALTY_MAX
from altro_mpc_icra2021_amd import problems as P

LDS_UNASKED = 65536                       # the dynamic LDS a kernel gets without asking for more
MAX_ROWS = 64                             # solve_wide.h kMaxP
LANE16_SHAPES = [(12, 4), (6, 3), (6, 6), (8, 4), (12, 3)]      # altro_batch.hip supported_dims: every other (n, m) runs wide


# ---------------------------------------------------------------------------------------------- evaluate.h restated
def evalw_ld(n, pad):
    return n | 1 if pad else n


def evalw_lds_doubles(ld, n, m):
    return ld * (n + m)


def evalw_lds_bytes(ld, n, m):
    return 4 * evalw_lds_doubles(ld, n, m) * 8


def evalw_lds_fits(ld, n, m, ltv):
    return (not ltv) and evalw_lds_bytes(ld, n, m) <= LDS_UNASKED


def eval_lds(n, m, ltv):
    """wide_backend.h eval_lds: what k_eval_rollout_wide, k_eval_score_wide (given form with a defect), k_ws_*_wide and k_sim_wide ask for"""
    return evalw_lds_bytes(n, n, m) if evalw_lds_fits(n, n, m, ltv) else 0


def eval_grad_lds(n, m, ltv):
    """wide_backend.h eval_grad_lds: what k_eval_grad_wide and k_eval_al_wide ask for (the padded slice)"""
    ld = evalw_ld(n, True)
    return evalw_lds_bytes(ld, n, m) if evalw_lds_fits(ld, n, m, ltv) else 0


# ---------------------------------------------------------------------------------------------- the table
# name -> backend, shape, batch, candidates, per-knot dynamics, (bytes of the plain slice x 4, of the padded slice x 4),
# (the plain one is kept in LDS, the padded one is)
TABLE = {
    "16-quads(12,4)": dict(backend="16", n=12, m=4, N=6, B=5, ncand=7, ltv=False, bytes=(6144, 6656), fits=(True, True)),
    "16-quads(6,6)": dict(backend="16", n=6, m=6, N=3, B=3, ncand=7, ltv=False, bytes=(2304, 2688), fits=(True, True)),
    "wide(32,32)": dict(backend="wide", n=32, m=32, N=4, B=3, ncand=3, ltv=False, bytes=(65536, 67584), fits=(True, False)),
    "wide(32,30)": dict(backend="wide", n=32, m=30, N=4, B=3, ncand=3, ltv=False, bytes=(63488, 65472), fits=(True, True)),
    "wide(33,29)": dict(backend="wide", n=33, m=29, N=4, B=3, ncand=3, ltv=False, bytes=(65472, 65472), fits=(True, True)),
    "wide(40,12)": dict(backend="wide", n=40, m=12, N=4, B=3, ncand=3, ltv=False, bytes=(66560, 68224), fits=(False, False)),
    "wide(17,1)": dict(backend="wide", n=17, m=1, N=3, B=3, ncand=3, ltv=False, bytes=(9792, 9792), fits=(True, True)),
    "wide-rows64(20,5)": dict(backend="wide", n=20, m=5, N=5, B=3, ncand=5, ltv=True, bytes=(16000, 16800), fits=(False, False)),
}
CASES = list(TABLE)
QUADS = [s for s in CASES if s.startswith("16-quads")]
SPLIT = ["wide(32,32)", "wide(32,30)"]          # the handles that go through all five calls interleaved
LDS_CASES = ["wide(32,32)", "wide(32,30)", "wide(33,29)"]       # per-instance [A | B] in four different slices of one block
ORACLE_CASES = QUADS + ["wide-rows64(20,5)"]
SOLVED_CASES = list(CASES)          # the cases on which the calls that need a solve run (evaluate_al: duals and penalty; simulate_policy: gains)
# Tuning, all of it on numpy and the oracle (tests/test_scoring_matrix.py holds the result).  seed: of evaluate_ref.make_case and of
# every draw below; margin: how far inside every inequality the base trajectory is, relative to 1 + the size of the row's value
# (cone_margin: times that for the cones); ubox: the control bounds of a case with row blocks are the largest |u_j| of the
# instance's base controls + ubox; pw: the power the factors of SCALE are raised to.
def _tune(seed, margin=0.05, cone_margin=1.0, ubox=0.05, pw=1.0, theta=None, tbox=1.0, tlin=1.0):
    return dict(seed=seed, margin=margin, cone_margin=cone_margin, ubox=ubox, pw=pw, theta=theta, tbox=tbox, tlin=tlin)


TUNE = {"16-quads(12,4)": _tune(271, margin=0.3, pw=0.25), "16-quads(6,6)": _tune(212, margin=0.02, ubox=0.02, pw=0.5, theta=0.5), "wide(32,32)": _tune(203), "wide(32,30)": _tune(204),
        "wide(33,29)": _tune(205), "wide(40,12)": _tune(206), "wide(17,1)": _tune(467, margin=0.2, ubox=0.02), "wide-rows64(20,5)": _tune(208, margin=0.3, pw=0.25)}
CAND_SEED = 301
X_BND = 6.0            # the state bound of wide(32,32), knots 0 .. N-1 (evaluate_ref.case_wide_box's)
TSCALE = 2.0           # the size of a cone's last row against its other rows: the polar cone is then within reach of the controls
POLAR = 8.0            # the length of the control step that puts a cone value into the polar cone (polar_step)

# per (case, instance) factors on blocks, by block name; anything not named is 1.  See the module docstring.
SCALE = {
    "16-quads(12,4)": [dict(soc4=8.0, eq=0.05), dict(soc2=16.0, eq=0.05, soc3x=0.25), dict(soc3x=8.0, eq=0.05), dict(soc2m=32.0, soc3m=32.0, eq=0.02),
                       dict(lin=16.0, eq=24.0)],
    "16-quads(6,6)": [dict(soc4=8.0, soc2=24.0, eq=0.05), dict(soc3x=8.0, soc3m=24.0, eq=0.05), dict(lin=16.0, eq=128.0)],
    "wide-rows64(20,5)": [dict(soc2=16.0, eq=0.02), dict(soc4=16.0, eq=0.02), dict(eq=4.0, soc4=4.0)],
}


def base_of(cs, seed):
    """the base trajectory Z (B, N, nz) of small controls (0 in the control columns of the terminal knot)"""
    rng = np.random.default_rng(seed + 7)
    Ub = np.clip(0.1 * rng.standard_normal((cs.B, cs.N - 1, cs.m)), -0.3, 0.3)
    Xb = ER.rollout(cs, Ub[:, None])[:, 0]
    return GR.stack_z(cs, Xb[:, None], Ub[:, None])[:, 0]


def free_optimum(cs):
    """Z (B, N, nz) of the controls that minimise the tracking cost with no constraint at all: the cost is a sum of squares of
    affine functions of U, solved as a least-squares problem per instance"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    nu = (N - 1) * m
    E = np.zeros((1 + nu, N - 1, m))
    E[1:] = np.eye(nu).reshape(nu, N - 1, m)
    Ua = np.ascontiguousarray(np.broadcast_to(E, (B,) + E.shape))
    Z = GR.stack_z(cs, ER.rollout(cs, Ua), Ua)                             # (B, 1 + nu, N, nz): the origin and the unit controls
    w = np.concatenate([np.broadcast_to(np.concatenate([cs.dt * cs.Q, cs.dt * cs.R], axis=1)[:, None], (B, N - 1, n + m)),
                        np.concatenate([cs.Qf, np.zeros((B, m))], axis=1)[:, None]], axis=1)
    ref = np.concatenate([cs.Xref, np.concatenate([cs.Uref, np.zeros((B, 1, m))], axis=1)], axis=-1)
    out = np.zeros((B, N, n + m))
    for b in range(B):
        sw = np.sqrt(w[b]).reshape(-1)
        M = ((Z[b, 1:] - Z[b, :1]).reshape(nu, -1) * sw).T
        u = np.linalg.lstsq(M, ((ref[b] - Z[b, 0]).reshape(-1) * sw), rcond=None)[0]
        out[b] = Z[b, 0] + np.tensordot(u, Z[b, 1:] - Z[b, :1], axes=1)
    return out


def base_box(cs, name):
    """control bounds (B, m) that leave the base inside: the largest |u_j| of the instance's base controls + ubox (theta: + theta
    times what the largest |u_j| of the free optimum has more)"""
    t = TUNE[name]
    ub = np.abs(base_of(cs, t["seed"])[:, :-1, cs.n:]).max(axis=1)
    more = 0.0 if t["theta"] is None else t["tbox"] * t["theta"] * np.maximum(np.abs(free_optimum(cs)[:, :-1, cs.n:]).max(axis=1) - ub, 0.0)
    return ub + more + t["ubox"]


class Blocks:
    """adds row blocks to a Case with offsets from the base trajectory; names[i] names cs.cons[i]"""

    def __init__(self, cs, name, seed):
        self.cs, self.rng, self.Z, self.t = cs, np.random.default_rng(seed + 1), base_of(cs, seed), TUNE[name]
        self.names = ["box" for _ in cs.cons]
        self.scale = SCALE.get(name, [{}] * cs.B)
        self.Zs = None if self.t["theta"] is None else free_optimum(cs)

    def _margin(self, fun, A, k0, k1, size, factor=1.0, tf=1.0):
        """how far inside the base is: margin (1 + size); theta: + theta times what fun has more at the free optimum than at the base,
        so that the row cuts the way from the base to the free optimum at that fraction and wants to be active"""
        mg = factor * self.t["margin"] * (1.0 + size)
        if self.Zs is None:
            return mg
        Zb, self.Z = self.Z, self.Zs
        vs = fun(self._values(A, k0, k1)[1])
        self.Z = Zb
        return mg + tf * self.t["theta"] * np.maximum(vs - fun(self._values(A, k0, k1)[1]), 0.0)

    def draw(self, p, xs, us, shared=False, per_knot=1):
        """rows (B, per_knot, p, nz): normal coefficients of size xs on the states and us on the controls"""
        cs = self.cs
        A = np.concatenate([xs * self.rng.standard_normal((1 if shared else cs.B, per_knot, p, cs.n)),
                            us * self.rng.standard_normal((1 if shared else cs.B, per_knot, p, cs.m))], axis=-1)
        return np.broadcast_to(A, (cs.B,) + A.shape[1:]).copy()

    def _put(self, kind, name, A, b, k0, k1, eq=False):
        s = np.array([self.scale[i].get(name, 1.0) ** self.t["pw"] for i in range(self.cs.B)])
        ER.add_rows(self.cs, kind, A * s[:, None, None, None], b * s[:, None, None], k0, k1, eq=eq)
        self.names.append(name)

    def _values(self, A, k0, k1):
        nk = k1 - k0 + 1
        A = np.broadcast_to(A, (self.cs.B, nk) + A.shape[2:])
        return A, np.einsum("bkpj,bkj->bkp", A, self.Z[:, k0:k1 + 1])

    def ineq(self, name, A, k0, k1, shared=False):
        """A z + b <= 0 with the base at -margin (1 + |A z_base|) (shared: one offset per row for the batch and the horizon)"""
        A, v = self._values(A, k0, k1)
        b = -v - self._margin(lambda x: x, A, k0, k1, np.abs(v), tf=self.t["tlin"])
        if shared:
            b = np.broadcast_to(b.min(axis=(0, 1)), b.shape)
        self._put("lin", name, A, b, k0, k1)

    def eq(self, name, A, k0, k1):
        """A z + b = 0 on the base: b = -A z_base, nonzero"""
        A, v = self._values(A, k0, k1)
        self._put("lin", name, A, -v, k0, k1, eq=True)

    def cone(self, name, A, k0, k1):
        """||(A z)_{0..p-2}|| <= (A z)_{p-1} + rad, rad per instance and knot so that the base is inside by cone_margin margin (1 + ||s||)"""
        A = A.copy()
        A[..., -1, :] *= TSCALE
        A, v = self._values(A, k0, k1)
        ns = np.linalg.norm(v[..., :-1], axis=-1)
        b = np.zeros(v.shape)
        b[..., -1] = ns - v[..., -1] + self._margin(lambda x: np.linalg.norm(x[..., :-1], axis=-1) - x[..., -1], A, k0, k1, ns, self.t["cone_margin"])
        self._put("soc", name, A, b, k0, k1)


def quads_case(name):
    """Every lane of the 16-lane row table, every cone dimension (the layout of lane16_matrix.quads_problem), per-instance data:
      soc4   p = 4 on mixing rows of the controls, knots 0..N-2                  quad 0, lanes 0-3
      soc2   p = 2 on mixing rows, knots 0..N-2                                  quad 1, lanes 4, 5
      soc3x  p = 3 on the states, knots 1..N-1 (the terminal knot)               quad 2, lanes 8-10
      soc2m  p = 2 on mixing rows, knots 0..2       } (12, 4): the quad whose    quad 3, lanes 12, 13
      soc3m  p = 3 on mixing rows, knots 3..N-2     } cone changes dimension     quad 3, lanes 12-14    ((6, 6): soc3m alone, 0..N-2)
      lin    4 mixing inequality rows, knots 0..N-2                              the spare lanes 6, 7, 11, 15
      eq     2 equality rows on the states at the terminal knot, b != 0          lanes 0, 1
      xub    1 inequality row on the states at the terminal knot                 lane 2
      box    on the controls, per instance"""
    t = TABLE[name]
    n, m, N, seed = t["n"], t["m"], t["N"], TUNE[name]["seed"]
    cs = ER.make_case(t["B"], n, m, N, seed, per_instance_cost=True)
    ER.add_box(cs, base_box(cs, name))
    bl = Blocks(cs, name, seed)
    bl.cone("soc4", bl.draw(4, 0.0, 1.0), 0, N - 2)
    bl.cone("soc2", bl.draw(2, 0.1, 1.0), 0, N - 2)
    bl.cone("soc3x", bl.draw(3, 0.5, 0.0), 1, N - 1)
    if N >= 6:
        bl.cone("soc2m", bl.draw(2, 0.1, 1.0), 0, 2)
        bl.cone("soc3m", bl.draw(3, 0.1, 1.0), 3, N - 2)
    else:
        bl.cone("soc3m", bl.draw(3, 0.1, 1.0), 0, N - 2)
    bl.ineq("lin", bl.draw(4, 0.1, 1.0), 0, N - 2)
    bl.eq("eq", bl.draw(2, 0.5, 0.0), N - 1, N - 1)
    bl.ineq("xub", bl.draw(1, 0.5, 0.0), N - 1, N - 1)
    return cs, bl.names, {}


QUAD_LANES = {"soc4": [0, 1, 2, 3], "soc2": [4, 5], "soc3x": [8, 9, 10], "soc2m": [12, 13], "soc3m": [12, 13, 14], "lin": [6, 7, 11, 15],
              "eq": [0, 1], "xub": [2]}


def wide_case(name):
    """per-instance time-invariant dynamics, a per-instance box on the controls; wide(32,32): also the state bound X_BND on knots
    0 .. N-1; wide(17,1): also two per-instance inequality rows on knots 0 .. N-2"""
    t = TABLE[name]
    n, m, N, seed = t["n"], t["m"], t["N"], TUNE[name]["seed"]
    cs = ER.make_case(t["B"], n, m, N, seed, per_instance_cost=True)
    ub = base_box(cs, name) if name == "wide(17,1)" else 0.5 + np.random.default_rng(seed + 2).random((t["B"], m))
    if name == "wide(32,32)":
        ER.add_box(cs, ub, x_bnd=X_BND, k0=0, k1=N - 1)
    else:
        ER.add_box(cs, ub)
    bl = Blocks(cs, name, seed)
    if name == "wide(17,1)":
        bl.ineq("lin", bl.draw(2, 0.1, 1.0), 0, N - 2)
    return cs, bl.names, {}


def rows64_case(name):
    """Pn = 64 with per-knot per-instance dynamics, in order of addition:
      lin24  24 inequality rows on the controls, knots 0..N-2, one block for the batch and the horizon     rows 0-23
      eq     8 equality rows, knots 1..N-2, per instance and per knot, b != 0.  The 8 rows of a knot span two directions
             (8 x 2 times 2 x nz): 24 independent equalities would leave the 20 controls of the horizon no freedom      rows 24-31
      soc2   p = 2 on mixing rows, knots 0..N-2                                                            rows 32, 33
      lin26  26 inequality rows, knots 2..N-1 (the terminal knot: state columns only), one block           rows 34-59
      soc4   p = 4 on mixing rows, knots 0..N-2, LAST: c0 = 60                                             rows 60-63
      box    on the controls"""
    t = TABLE[name]
    n, m, N, seed = t["n"], t["m"], t["N"], TUNE[name]["seed"]
    cs = ER.make_case(t["B"], n, m, N, seed, per_knot_dyn=True)
    ER.add_box(cs, base_box(cs, name))
    bl = Blocks(cs, name, seed)
    bl.ineq("lin24", bl.draw(24, 0.0, 1.0, shared=True), 0, N - 2, shared=True)
    W, R = bl.rng.standard_normal((cs.B, N - 2, 8, 2)), bl.draw(2, 0.3, 1.0, per_knot=N - 2)
    bl.eq("eq", W @ R, 1, N - 2)
    bl.cone("soc2", bl.draw(2, 0.1, 1.0), 0, N - 2)
    bl.ineq("lin26", bl.draw(26, 0.02, 0.02, shared=True), 2, N - 1, shared=True)
    bl.cone("soc4", bl.draw(4, 0.1, 1.0), 0, N - 2)
    return cs, bl.names, dict(per_knot_dyn=True, shared=(1, 4))


@functools.lru_cache(maxsize=None)
def build(name):
    """(Case, name of every constraint of the case, keywords of evaluate_ref.to_problem).  The Case is shared: do not write to it."""
    make = quads_case if name in QUADS else rows64_case if name.startswith("wide-rows64") else wide_case
    cs, names, kw = make(name)
    t = TABLE[name]
    assert (cs.B, cs.n, cs.m, cs.N) == (t["B"], t["n"], t["m"], t["N"])
    return cs, names, kw


# extra candidates per case: "big" 2.5 x the bounds random, "neg" the random one negated, or {knot: cone} -- the base controls with
# the control of that knot stepped so that the named cone's value (a state cone: at the NEXT knot) lies in the polar cone
EXTRA = {
    "16-quads(12,4)": ["big", "neg", {0: "soc4", 1: "soc2", 2: "soc2m", 4: "soc3m"}, {0: "soc3x"}],
    "16-quads(6,6)": ["big", {0: "soc4", 1: "soc2"}, {0: "soc3m"}, {0: "soc3x"}],
    "wide-rows64(20,5)": ["big", {0: "soc4", 1: "soc2"}],
}


def polar_step(cs, c, b, k):
    """the unit control step w at knot k that lowers the cone's last value fastest per unit of ||s||: with S the rows of s and a
    the last row as functions of u_k (through B_k for a cone on the states of knot k + 1), w = -(S'S)^-1 a, regularised"""
    n = cs.n
    if np.abs(c.A[b, :, :, n:]).max() > 0:
        M = c.A[b, k - c.k0][:, n:]
    else:
        M = c.A[b, k + 1 - c.k0][:, :n] @ cs.Bm[b, k]
    S, a = M[:-1], M[-1]
    G = S.T @ S
    w = -np.linalg.solve(G + 1e-9 * np.trace(G) * np.eye(cs.m), a)
    return w / np.linalg.norm(w)


@functools.lru_cache(maxsize=None)
def candidates(name):
    """ER.candidates (inside, pushed, random) and the EXTRA ones of the case.  In a case with row blocks candidate 0 is the base
    trajectory's controls (inside every inequality by its margin, on every equality) and candidate 1 the same with ER's push"""
    cs, names, _ = build(name)
    U = ER.candidates(cs, CAND_SEED)
    if len(names) > 1:
        push = U[:, 1, cs.N // 2].copy()
        U[:, 0] = U[:, 1] = base_of(cs, TUNE[name]["seed"])[:, :-1, cs.n:]
        U[:, 1, cs.N // 2] = push
    rng = np.random.default_rng(CAND_SEED + 1)
    ub = cs.cons[0].zmax[:, None, cs.n:]
    more = []
    for e in EXTRA.get(name, []):
        if e == "big":
            more.append(2.5 * ub * rng.standard_normal(U[:, 0].shape))
        elif e == "neg":
            more.append(-U[:, 2])
        else:
            V = U[:, 0].copy()
            for k, cone in e.items():
                c = cs.cons[names.index(cone)]
                for b in range(cs.B):
                    V[b, k] += POLAR * polar_step(cs, c, b, k)
            more.append(V)
    if more:
        U = np.concatenate([U, np.stack(more, axis=1)], axis=1)
    assert U.shape[1] == TABLE[name]["ncand"]
    return np.ascontiguousarray(U)


# ---------------------------------------------------------------------------------------------- the lane placement
def specs_of(cs):
    """instance 0's row blocks as lane16_matrix.pack takes them (a BOX takes no lane)"""
    return [NS(kind=P.SOC if c.kind == "soc" else P.LINEAR if c.kind == "lin" else P.BOX, sense=P.EQ if c.eq else P.INEQ, k_first=c.k0, k_last=c.k1,
               A=None if c.kind == "box" else c.A[0], b=None if c.kind == "box" else c.b[0]) for c in cs.cons]


def wide_rows(cs):
    """(first row, dimension) of every row block on the one-wave-per-instance backend: rows in order of addition"""
    out, r = [], 0
    for c in cs.cons:
        if c.kind != "box":
            out.append((r, c.A.shape[2]))
            r += c.A.shape[2]
    return out, r


# ---------------------------------------------------------------------------------------------- what the inputs reach
def per_block(cs, X, U):
    """[(violation (B, nc, nk) of the block per knot, value v (B, nc, nk, p) or None for the box)] per constraint of the case:
    ER.violation's terms one block at a time"""
    out = []
    for c in cs.cons:
        one = [ER.violation(cs, X, U, cons=[ER.Con(c.kind, k, k, c.zmin, c.zmax, None if c.A is None else c.A[:, k - c.k0:k - c.k0 + 1],
                                                  None if c.b is None else c.b[:, k - c.k0:k - c.k0 + 1], c.eq)])[0] for k in range(c.k0, c.k1 + 1)]
        v = None
        if c.kind != "box":
            Z = GR.stack_z(cs, X, U)[:, :, c.k0:c.k1 + 1]
            v = np.einsum("bkpj,bckj->bckp", c.A, Z) + c.b[:, None]
        out.append((np.stack(one, axis=-1), v))
    return out


def branches(v):
    """(inside, polar, boundary) of cone values v (.., p), bool arrays"""
    ns, t = np.linalg.norm(v[..., :-1], axis=-1), v[..., -1]
    inside = ns <= t
    polar = ~inside & (ns <= -t)
    return inside, polar, ~inside & ~polar


def deciders(cs, X, U):
    """(winner (B, nc): index of the constraint whose violation is c_max, -1 where c_max == 0; cmax (B, nc); blocks)"""
    blocks = per_block(cs, X, U)
    V = np.stack([b[0].max(axis=-1) for b in blocks], axis=0)
    cmax = V.max(axis=0)
    return np.where(cmax > 0, V.argmax(axis=0), -1), cmax, blocks


def guards(name):
    """what tests/test_scoring_matrix.py asserts on, all of it on numpy: NS(cs, names, U, X, winner, cmax, cb, blocks, cones {name:
    NS(branch (3,), decides, violated_knots (nk,))}, eqs {name: NS(decides_neg: (b, c) where a row with v < 0 is the arg-max row,
    drop: c_max without the fabs)}, terminal {name: largest violation at knot N-1}, grad: GR.merit_grad at rho = 10)"""
    cs, names, kw = build(name)
    U = candidates(name)
    X = ER.rollout(cs, U)
    winner, cmax, blocks = deciders(cs, X, U)
    _, cb = ER.violation(cs, X, U)
    g = NS(cs=cs, names=names, U=U, X=X, winner=winner, cmax=cmax, cb=cb, blocks=blocks, cones={}, eqs={}, terminal={})
    for i, (c, nm, (V, v)) in enumerate(zip(cs.cons, names, blocks)):
        if c.k1 == cs.N - 1:
            g.terminal[nm] = float(V[..., -1].max())
        if c.kind == "soc":
            g.cones[nm] = NS(branch=np.array([int(w.sum()) for w in branches(v)]), decides=int((winner == i).sum()),
                             violated_knots=(V > 0).any(axis=(0, 1)), violated_instances=(V > 0).any(axis=(1, 2)))
        elif c.eq:
            others = np.stack([bl[0].max(axis=-1) for j, bl in enumerate(blocks) if j != i], axis=0).max(axis=0)
            kk = V.argmax(axis=-1)                                        # the knot of the block's largest |v| per (b, c)
            vk = np.take_along_axis(v, kk[..., None, None], axis=2)[:, :, 0]
            row = np.abs(vk).argmax(axis=-1)
            neg = np.take_along_axis(vk, row[..., None], axis=-1)[..., 0] < 0
            drop = np.maximum(others, np.maximum(v, 0.0).max(axis=(2, 3)))
            g.eqs[nm] = NS(decides_neg=(winner == i) & neg, drop=drop)
    g.grad = GR.merit_grad(cs, X, U, 10.0)
    return g


def swapped_rollout_gap(name):
    """guard (g): (largest difference between instance 1's true rollout and its rollout under instance 0's [A | B | f], largest
    bound 1 of instance 1's own rollout)"""
    cs, _, _ = build(name)
    U = candidates(name)
    one, other = ER.sub_case(cs, 1), ER.sub_case(cs, 1)
    other.A, other.Bm, other.f = cs.A[0:1], cs.Bm[0:1], cs.f[0:1]
    X1, X0 = ER.rollout(one, U[1:2]), ER.rollout(other, U[1:2])
    _, S = ER.step_residual(one, X1, U[1:2])
    return float(np.abs(X1 - X0).max()), float(ER.step_bound(one, S).max())


def row63_moves_P(name="wide-rows64(20,5)", delta=1e-3):
    """guard (d): (|P - P'| (B, nc), bound 5) with the value of the last row of the last cone moved by delta alone"""
    g = guards(name)
    cs = g.cs
    last = cs.cons[-1]
    assert last.kind == "soc" and wide_rows(cs) == ([(0, 24), (24, 8), (32, 2), (34, 26), (60, 4)], MAX_ROWS)
    b2 = last.b.copy()
    b2[..., -1] += delta
    moved = cs.cons[:-1] + [ER.Con("soc", last.k0, last.k1, A=last.A, b=b2)]
    y2 = GR.merit_grad(cs, g.X, g.U, 10.0, cons=moved)
    return np.abs(g.grad.P - y2.P), g.grad.Pb


# ---------------------------------------------------------------------------------------------- the solves behind the calls
SIM_OPTS = dict(cost_tolerance=1e-4, cost_tolerance_intermediate=1e-4, constraint_tolerance=1e-4, penalty_initial=1000.0, penalty_scaling=100.0,
                reset_duals=0, iterations=60)       # test_simulate_gpu.OPTS: the solve that provides the gains
AL_OPTS = dict(iterations_outer=3)                  # test_evaluate_al_gpu.SOLVE: the short solve that provides duals and penalty
QUADS_SIM_OPTS = dict(SIM_OPTS, penalty_initial=10.0, penalty_scaling=10.0, iterations_outer=40, iterations=300)    # wide_matrix.ROWS_OPTS


def sim_opts(name):
    return QUADS_SIM_OPTS if name in QUADS else SIM_OPTS


@functools.lru_cache(maxsize=None)
def solve_guard(name, short):
    """guard (h): the case on the oracle, solved from the reference controls with AL_OPTS (short) or SIM_OPTS: dict(status (B,),
    outer (B,), capped, nonzero {kind: (B,) bool: a nonzero dual on a constraint of that kind})"""
    import oracle_py as oracle
    oracle.build()
    cs, names, kw = build(name)
    out = dict(status=[], outer=[], capped=False, nonzero={})
    for b in range(cs.B):
        o = ER.oracle_of(oracle, cs, b, bool(kw.get("per_knot_dyn")))
        o.set_opts(oracle.default_opts(**(AL_OPTS if short else sim_opts(name))))
        o.set_controls(cs.Uref[b])
        so = o.solve()
        out["status"].append(so.status); out["outer"].append(so.iterations_outer)
        out["capped"] = out["capped"] or max(so.penalty_max_outer[:min(so.iterations_outer, 64)]) >= PENALTY_MAX
        for i, c in enumerate(cs.cons):
            kind = "eq" if c.eq else c.kind
            out["nonzero"].setdefault(kind, [False] * cs.B)
            out["nonzero"][kind][b] = out["nonzero"][kind][b] or bool(np.any(o.duals(i) != 0.0))
    return dict(status=np.array(out["status"]), outer=np.array(out["outer"]), capped=out["capped"],
                nonzero={k: np.array(v) for k, v in out["nonzero"].items()})


@functools.lru_cache(maxsize=None)
def al_inputs(name):
    """(duals the short solve left on the oracle, penalty (B,), the duals drawn from them by evaluate_al_ref.draw_duals)"""
    import oracle_py as oracle
    import evaluate_al_ref as AR
    oracle.build()
    cs, names, kw = build(name)
    lam, mu = [[] for _ in cs.cons], []
    for b in range(cs.B):
        o = ER.oracle_of(oracle, cs, b, bool(kw.get("per_knot_dyn")))
        o.set_opts(oracle.default_opts(**AL_OPTS))
        o.set_controls(cs.Uref[b])
        o.solve()
        for i, l in enumerate(AR.shape_duals(cs, [o.duals(i) for i in range(len(cs.cons))])):
            lam[i].append(l[0])
        mu.append(o.penalties(0)[0])
    lam, mu = [np.array(l) for l in lam], np.array(mu)
    return lam, mu, AR.draw_duals(cs, lam, mu, 77)
