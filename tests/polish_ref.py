"""Dense yardstick of the projected-Newton polish (csrc/pn_core.h; restated in oracle/altro_oracle.c projected_newton).

Plain numpy, long double where it is cheap.  It shares nothing with the code under test but the definition of the rows: no
block structure, no Cholesky, no regularisation, no refinement loop, no line search.

The polish moves the AL-stage trajectory z0 = (x_0, u_0, ..., x_{N-1}) by accepted steps -alpha H^-1 D' lam, where D holds the
rows in force -- initial condition, active box sides, active linear rows, dynamics defects -- and H = diag(cost Hessian) +
rho_primal.  All rows handled here are LINEAR in z (cones are out of scope: their fixed point depends on the path), so D is
constant while the active set holds and two things follow whatever the factorisation, the refinement or the line search did:

 RANGE        z1 - z0 lies in range(H^-1 D').  out_of_range() measures the part of sqrt(H) (z1 - z0) outside range(H^-1/2 D').
 CLOSED FORM  if the polish ends with ||d(z1)||_inf < ctol, then with z* = project(z0) = z0 - H^-1 D' S^+ d(z0), S = D H^-1 D':
              z1 - z* is in the same range and D (z1 - z*) = d(z1), hence z1 - z* = H^-1 D' S^+ d(z1) and
                  ||z1 - z*||_inf <= K ctol,      K = gain(D, H) = || H^-1 D' S^+ ||_inf.

Bounds (derived here, never from what the code under test returns; u = 2^-53):

 range_bound()   An accepted step is z <- fl(z - alpha t), t = fl(hinv (E' v - v_prev)), alpha a power of two.
                 (i) storing the sum rounds every component: <= u |z_new| + u |alpha t| per step; over at most 112 steps
                 (11 linearisations x 10 refinements, and the plane copies, which are exact) and with every iterate within
                 twice the hull of z0 and z1:                           112 * 2 u * || sqrt(H) max(|z0|, |z1|) ||_2
                 (ii) t itself: a column of D has at most c nonzeros (the rows of its knot's block and one defect row of the
                 knot before), so the dot product and the scaling carry gamma_(c+2) against hinv |D|' |v|.  chi is the
                 cancellation in D' lam measured on the YARDSTICK's multipliers lam* = S^+ d(z0), and the steps of a descent
                 on ||d|| add up to at most twice the displacement:   2 (c + 3) u chi || sqrt(H) (z1 - z0) ||_2
                 (iii) the yardstick's own projector (orthonormal basis from an SVD, applied twice in long double):
                                                                        64 u || sqrt(H) (z1 - z0) ||_2
 closed_form_bound()  K ctol + range_bound / sqrt(min H)   (the rounding term carried into the max norm)
 r0_bound()      r0 = || g + D' lam0 ||_2 is one matrix-vector product: gamma_(c+3) (|| g ||_2 + || |D|' |lam0| ||_2).
 r1_slack()      reg_solve stops at a residual of 1e-8 in the max norm of (D D') cor = rhs; the multipliers are then off by
                 (D D')^+ res and the stationarity residual by D' (D D')^+ res:  sqrt(len z) K2 1e-8, K2 = gain(D, I).
"""
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
U_ROUND = 2.0 ** -53
N_UPDATES = 112
REG_SOLVE_STOP = 1e-8


@dataclass
class Rows:
    """One LINEAR constraint block: value = A z_k + b on knots k0..k1 (terminal knot: state columns only)."""
    equality: bool
    A: np.ndarray        # (p, n + m)
    b: np.ndarray        # (p,)
    k0: int
    k1: int


@dataclass
class Instance:
    n: int
    m: int
    N: int
    dt: float
    A: np.ndarray        # (n, n) or (N - 1, n, n)
    Bm: np.ndarray       # (n, m) or (N - 1, n, m)
    f: np.ndarray        # (n,) or (N - 1, n)
    Q: np.ndarray        # (n,) diagonal; the stage Hessian is dt Q, dt R, the terminal one Qf
    R: np.ndarray
    Qf: np.ndarray
    rho_primal: float
    Xref: np.ndarray     # (N, n)
    Uref: np.ndarray     # (N - 1, m)
    x0: np.ndarray
    zmin: np.ndarray = None   # (n + m,), +-inf where absent
    zmax: np.ndarray = None
    box_k0: int = 0
    box_k1: int = -1
    rows: list = field(default_factory=list)


@dataclass
class Active:
    D: np.ndarray        # (rows, len z)
    c: np.ndarray        # d(z) = D z - c
    d: np.ndarray        # values at the trajectory given
    labels: list         # per row: ("ic", 0, i) | ("hi", k, j) | ("lo", k, j) | ("row", k, (block, r)) | ("dyn", k, i)
    block_rows: np.ndarray   # (N,) rows of block k of S
    margin: float        # smallest distance of an inequality row from the test c >= -tol (inf if none)


class PolishRef:
    def __init__(self, inst):
        self.p = p = inst
        self.nz = p.n + p.m
        self.len = (p.N - 1) * self.nz + p.n
        h = np.empty(self.len)
        for k in range(p.N - 1):
            h[k * self.nz:(k + 1) * self.nz] = np.r_[p.dt * p.Q, p.dt * p.R]
        h[(p.N - 1) * self.nz:] = p.Qf
        self.hcost = h                       # the cost Hessian (g = hcost (z - zref))
        self.H = h + p.rho_primal            # the polish's metric
        self.zref = self.pack(p.Xref, p.Uref)

    # ---- layout
    def pack(self, X, U):
        p = self.p
        z = np.empty(self.len)
        for k in range(p.N - 1):
            z[k * self.nz:(k + 1) * self.nz] = np.r_[X[k], U[k]]
        z[(p.N - 1) * self.nz:] = X[p.N - 1]
        return z

    def unpack(self, z):
        p = self.p
        body = np.asarray(z[:(p.N - 1) * self.nz]).reshape(p.N - 1, self.nz)
        X = np.vstack([body[:, :p.n], z[(p.N - 1) * self.nz:][None]])
        return X, body[:, p.n:].copy()

    def _dyn(self, k):
        p = self.p
        per = np.ndim(p.A) == 3
        return (p.A[k] if per else p.A), (p.Bm[k] if per else p.Bm), (p.f[k] if np.ndim(p.f) == 2 else p.f)

    # ---- rows
    def active_rows(self, z, tol):
        """Dense D, right-hand side and values in the polish's row order: initial condition; per knot upper box sides, lower
        box sides, generic rows (inequalities join with c >= -tol; the terminal knot sees states only); then the defect."""
        p, nz = self.p, self.nz
        Dr, cr, labels, blocks = [], [], [], np.zeros(p.N, dtype=int)
        margin = np.inf

        def add(k, cols, vals, c, label):
            row = np.zeros(self.len)
            row[cols] = vals
            Dr.append(row); cr.append(c); labels.append(label); blocks[k] += 1

        for i in range(p.n):
            add(0, [i], [1.0], p.x0[i], ("ic", 0, i))
        for k in range(p.N):
            base, lim = k * nz, (p.n if k == p.N - 1 else nz)
            zk = z[base:base + lim]
            if p.zmax is not None and p.box_k0 <= k <= p.box_k1:
                for j in range(lim):
                    if np.isfinite(p.zmax[j]):
                        v = zk[j] - p.zmax[j]
                        margin = min(margin, abs(v + tol))
                        if v >= -tol:
                            add(k, [base + j], [1.0], p.zmax[j], ("hi", k, j))
                for j in range(lim):
                    if np.isfinite(p.zmin[j]):
                        v = p.zmin[j] - zk[j]
                        margin = min(margin, abs(v + tol))
                        if v >= -tol:
                            add(k, [base + j], [-1.0], -p.zmin[j], ("lo", k, j))
            for bi, blk in enumerate(p.rows):
                if not blk.k0 <= k <= blk.k1:
                    continue
                for r in range(blk.A.shape[0]):
                    v = blk.b[r] + blk.A[r, :lim] @ zk
                    if not blk.equality:
                        margin = min(margin, abs(v + tol))
                        if not v >= -tol:
                            continue
                    add(k, np.arange(base, base + lim), blk.A[r, :lim], -blk.b[r], ("row", k, (bi, r)))
            if k < p.N - 1:
                Ak, Bk, fk = self._dyn(k)
                for i in range(p.n):
                    row = np.zeros(self.len)
                    row[base:base + nz] = np.r_[Ak[i], Bk[i]]
                    row[base + nz + i] -= 1.0
                    Dr.append(row); cr.append(-fk[i]); labels.append(("dyn", k, i)); blocks[k] += 1
        D, c = np.array(Dr), np.array(cr)
        d = np.asarray(D.astype(LD) @ z.astype(LD) - c.astype(LD), dtype=np.float64)
        return Active(D, c, d, labels, blocks, margin)

    def union(self, a, b):
        """The rows active in a or in b (a's order first): what a displacement may use if the set changed on the way."""
        have = set(a.labels)
        extra = [i for i, lab in enumerate(b.labels) if lab not in have]
        if not extra:
            return a.D
        return np.vstack([a.D, b.D[extra]])

    # ---- dense algebra
    def _W(self, D, H):
        return D / np.sqrt(H)[None, :]

    def _pinv_refined(self, W, rhs):
        """Minimum-norm least-squares solution of W y = rhs: pseudo-inverse (duplicated rows are fine), refined in long double."""
        Wp = np.linalg.pinv(W, rcond=1e-12)
        Wl = W.astype(LD)
        y = (Wp @ rhs).astype(LD)
        for _ in range(3):
            res = rhs.astype(LD) - Wl @ y
            y = y + (Wp @ np.asarray(res, dtype=np.float64)).astype(LD)
        return y

    def project(self, z0, act):
        """z0 - H^-1 D' S^+ d(z0), S = D H^-1 D': the H-orthogonal projection of z0 onto {D z = c}."""
        H = self.H
        y = self._pinv_refined(self._W(act.D, H), act.d)          # y = H^-1/2 D' S^+ d
        return np.asarray(z0.astype(LD) - y / np.sqrt(H).astype(LD), dtype=np.float64)

    def multipliers(self, act):
        """lam* = S^+ d(z0) (minimum norm), for the cancellation factor of range_bound."""
        W = self._W(act.D, self.H)
        return np.linalg.pinv(W @ W.T, rcond=1e-12) @ act.d

    def _basis(self, W):
        _, s, Vt = np.linalg.svd(W, full_matrices=False)
        return Vt[s > 1e-12 * s.max()].T

    def out_of_range(self, dz, D, H=None):
        """|| part of sqrt(H) dz outside range(H^-1/2 D') ||_2"""
        H = self.H if H is None else H
        V = self._basis(self._W(D, H)).astype(LD)
        v = np.sqrt(H).astype(LD) * dz.astype(LD)
        for _ in range(2):
            v = v - V @ (V.T @ v)
        return float(np.sqrt(np.sum(v * v)))

    def gain(self, D, H=None):
        """K = || H^-1 D' S^+ ||_inf = || H^-1/2 pinv(D H^-1/2) ||_inf (largest absolute row sum)"""
        H = self.H if H is None else H
        M = np.linalg.pinv(self._W(D, H), rcond=1e-12) / np.sqrt(H)[:, None]
        return float(np.abs(M).sum(axis=1).max())

    def dual_residuals(self, z1, act, lam0):
        """(r0, r_ls): || g + D' lam0 ||_2 with g = hcost (z1 - zref) (no rho_primal: as the kernel forms it), and
        min_lam || g + D' lam ||_2."""
        g = self.hcost.astype(LD) * (z1.astype(LD) - self.zref.astype(LD))
        r = g + act.D.T.astype(LD) @ lam0.astype(LD)
        r0 = float(np.sqrt(np.sum(r * r)))
        V = self._basis(act.D).astype(LD)
        v = g
        for _ in range(2):
            v = v - V @ (V.T @ v)
        return r0, float(np.sqrt(np.sum(v * v)))

    def lam0(self, act, box_duals, row_duals):
        """The AL duals of the active rows: box_duals (nk, 2, nz) from knot box_k0 on (or None), row_duals[block] (nk, p) from
        the block's k0 on; zero for the initial condition and the dynamics."""
        p = self.p
        out = np.zeros(len(act.labels))
        for i, (kind, k, j) in enumerate(act.labels):
            if kind == "hi":
                out[i] = box_duals[k - p.box_k0, 0, j]
            elif kind == "lo":
                out[i] = box_duals[k - p.box_k0, 1, j]
            elif kind == "row":
                out[i] = row_duals[j[0]][k - p.rows[j[0]].k0, j[1]]
        return out

    # ---- bounds
    def _colnnz(self, D):
        return int((D != 0.0).sum(axis=0).max())

    def range_bound(self, z0, z1, act0, D):
        sH = np.sqrt(self.H)
        disp = float(np.linalg.norm(sH * (z1 - z0)))
        store = N_UPDATES * 2.0 * U_ROUND * float(np.linalg.norm(sH * np.maximum(np.abs(z0), np.abs(z1))))
        lam = self.multipliers(act0)
        num = np.linalg.norm((np.abs(act0.D).T @ np.abs(lam)) / sH)
        den = np.linalg.norm((act0.D.T @ lam) / sH)
        chi = float(num / den) if den > 0 else 1.0
        step = 2.0 * (self._colnnz(D) + 3) * U_ROUND * chi * disp
        return store + step + 64.0 * U_ROUND * disp

    def closed_form_bound(self, z0, z1, act0, ctol):
        return self.gain(act0.D) * ctol + self.range_bound(z0, z1, act0, act0.D) / float(np.sqrt(self.H.min()))

    def r0_bound(self, z1, act, lam0):
        g = self.hcost * (z1 - self.zref)
        return (self._colnnz(act.D) + 3) * U_ROUND * float(np.linalg.norm(g) + np.linalg.norm(np.abs(act.D).T @ np.abs(lam0))) * 1.01

    def r1_slack(self, act):
        return float(np.sqrt(self.len)) * self.gain(act.D, np.ones(self.len)) * REG_SOLVE_STOP
