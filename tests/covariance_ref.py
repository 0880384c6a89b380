"""numpy yardstick of altro_batch_propagate_covariance: the definition restated, parametric in dtype (np.float32, np.float64,
np.longdouble), on the data of an evaluate_ref.Case and the gains altro_batch_get_gains returns.  Shared by
tests/test_covariance_api.py (its meaning against simulate_ref and the CPU oracle) and tests/test_covariance_gpu.py (the device
against it in extended precision).

    M_k = A_k + B_k K_k;   S_0 = Sigma0;   S_{k+1} = M_k S_k M_k' + W,  k = 0 .. N-2
    sx[k, i] = sqrt(max(S_k[i, i], 0));   su[k, a] = sqrt(max((K_k S_k K_k')[a, a], 0))
    sc[k - k0, r] = sqrt(max(g' S_k g, 0)),  g = a_x + K_k' a_u  (knot N-1: g = a_x)
    dJ = 1/2 sum_{k<N-1} dt (Q . diag S_k + R . diag K_k S_k K_k') + 1/2 Qf . diag S_{N-1}
    s_e = max over the knots of the BOX's range of element e's deviation (controls up to knot N-2)
    two finite sides: lo' = min(lo + kappa s_e, mid), hi' = max(hi - kappa s_e, mid), mid = (lo + hi) / 2;
    a lone finite side lo + kappa s_e or hi - kappa s_e; infinite sides stay

Every sum is numpy's matmul / dot in the dtype asked for; Sigma0 / W None means zero."""
from types import SimpleNamespace as NS

import numpy as np


def _pos(a):
    return np.where(a > 0, a, np.where(np.isnan(a), a, 0))


def propagate(cs, K, Sigma0=None, W=None, rows=None, box=None, kappa=0.0, dtype=np.float64):
    """cs: evaluate_ref.Case (A (B, N-1, n, n), Bm (B, N-1, n, m), Q, R, Qf (B, .), dt); K (B, N-1, m, n), zeros for the open
    loop; Sigma0, W (n, n) or (B, n, n) or None; rows: a Con of kind "lin" / "soc" (A (B, nk, p, nz), k0, k1) or None; box: a Con
    of kind "box" (zmin, zmax (B, nz), k0, k1) or None.
    -> NS(S (B, N, n, n), sx (B, N, n), su (B, N-1, m), dJ (B,), sc (B, nk, p) or None, zmin_t, zmax_t (B, nz) or None), all of
    `dtype`"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    t = lambda a: np.asarray(a, dtype=dtype)
    full = lambda a: np.zeros((B, n, n), dtype=dtype) if a is None else np.broadcast_to(t(a), (B, n, n))
    A, Bm, K = t(cs.A), t(cs.Bm), t(K)
    S0, Wf = full(Sigma0), full(W)
    Q, R, Qf, dt = t(cs.Q), t(cs.R), t(cs.Qf), dtype(cs.dt)
    S = np.zeros((B, N, n, n), dtype=dtype)
    KSK = np.zeros((B, N - 1, m), dtype=dtype)
    S[:, 0] = S0
    for k in range(N - 1):
        M = A[:, k] + Bm[:, k] @ K[:, k]
        KSK[:, k] = np.einsum("baj,bja->ba", K[:, k] @ S[:, k], np.swapaxes(K[:, k], -1, -2))
        S[:, k + 1] = (M @ S[:, k]) @ np.swapaxes(M, -1, -2)
        if W is not None:
            S[:, k + 1] = S[:, k + 1] + Wf
    dg = np.einsum("bkii->bki", S)
    half = dtype(0.5)
    dJ = (half * ((dt * Q)[:, None] * dg[:, :-1]).sum(axis=(1, 2)) + half * ((dt * R)[:, None] * KSK).sum(axis=(1, 2))
          + half * (Qf * dg[:, -1]).sum(axis=1))
    out = NS(S=S, sx=np.sqrt(_pos(dg)), su=np.sqrt(_pos(KSK)), dJ=dJ, sc=None, zmin_t=None, zmax_t=None)
    if rows is not None:
        nk, p = rows.A.shape[1:3]
        Ar = t(rows.A)
        sc = np.zeros((B, nk, p), dtype=dtype)
        for kk in range(nk):
            k = rows.k0 + kk
            g = Ar[:, kk, :, :n]
            if k < N - 1:
                g = g + Ar[:, kk, :, n:] @ K[:, k]
            sc[:, kk] = np.einsum("bpi,bpi->bp", g @ S[:, k], g)
        out.sc = np.sqrt(_pos(sc))
    if box is not None:
        kap = dtype(kappa)
        s = np.zeros((B, n + m), dtype=dtype)
        s[:, :n] = out.sx[:, box.k0:box.k1 + 1].max(axis=1)
        ku = min(box.k1, N - 2)
        if ku >= box.k0:
            s[:, n:] = out.su[:, box.k0:ku + 1].max(axis=1)
        lo, hi = t(box.zmin), t(box.zmax)
        fl, fh = np.isfinite(lo), np.isfinite(hi)
        with np.errstate(invalid="ignore"):
            mid = half * (lo + hi)
            lo_t = np.where(fl & fh, np.minimum(lo + kap * s, mid), np.where(fl, lo + kap * s, lo))
            hi_t = np.where(fl & fh, np.maximum(hi - kap * s, mid), np.where(fh, hi - kap * s, hi))
        out.zmin_t, out.zmax_t = lo_t, hi_t
    return out


def rel_err(a, ref):
    """max |a - ref| / max |ref| over everything but the leading (instance) axis, in extended precision; 0 where ref is
    identically zero and a is too (inf where it is not)"""
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    ax = tuple(range(1, ref.ndim))
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        diff = np.where(fin, a - ref, 0)
    num = np.abs(diff).max(axis=ax) if ax else np.abs(diff)
    den = np.abs(np.where(fin, ref, 0)).max(axis=ax) if ax else np.abs(np.where(fin, ref, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0)).astype(np.float64)
