"""numpy yardstick of altro_batch_cost_to_go: the definition restated, parametric in dtype (np.float64,
np.longdouble), on the data of an evaluate_ref.Case, the gains altro_batch_get_gains returns and the trajectory the handle holds;
for mode 1 also the codes and mu_pass of altro_batch_get_gain_active_set, the BOX duals and the penalty held.  Shared by
tests/test_cost_to_go_api.py (its meaning against a dense Riccati recursion, simulate_ref and covariance_ref, on the CPU) and
tests/test_cost_to_go_gpu.py (the device against it in extended precision).

    V_k(x) = v_k + p_k'(x - xbar_k) + 1/2 (x - xbar_k)' P_k (x - xbar_k),   M_k = A_k + B_k K_k,   e = z - zref
    P_{N-1} = Hx_{N-1}                 P_k = Hx_k + K_k' Hu_k K_k + M_k' P_{k+1} M_k
    p_{N-1} = lx_{N-1}                 p_k = lx_k + K_k' lu_k + M_k' p_{k+1}
    v_{N-1} = value of knot N-1        v_k = value of knot k + v_{k+1}
    mode 0:  H = w (dt Q, dt R; Qf at knot N-1),  l = w e,  value of a knot = 1/2 sum w e^2
    mode 1:  H = w + mu_p [upper side in the set] + mu_p [lower side],  l = w e + g_hi - g_lo,  g = dual + [c >= 0 or dual > 0] mu c,
             value of a knot = 1/2 sum w e^2 + sum over the sides that exist of  dual c + [c >= 0 or dual > 0] mu c^2 / 2

Every product is numpy's matmul / einsum in the dtype asked for."""
from types import SimpleNamespace as NS

import numpy as np

import solution_data_ref as SD


def local_terms(cs, X, U, mode=0, codes=None, mu_pass=None, duals=None, mu=None, dtype=np.float64):
    """(H (B, N, nz), l (B, N, nz), value (B, N)) of every knot; the control columns of knot N-1 are zero"""
    t = lambda a: np.asarray(a, dtype=dtype)
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    th = SD.theta_of(cs)
    wx, wu = SD.weights(th, cs, dtype)
    w = np.concatenate([wx, np.repeat(wu[:, None], N, axis=1)], axis=2)
    w[:, -1, n:] = 0
    Z = SD.stack_z(cs, t(X), t(U), dtype)
    Zr = SD.stack_z(cs, t(cs.Xref), t(cs.Uref), dtype)
    e = Z - Zr
    half = dtype(0.5)
    val = half * (w * e * e).sum(axis=2)
    if not mode:
        return w, w * e, val
    hx, hu = SD.hz_of(th, cs, codes, mu_pass, dtype)
    H = np.zeros((B, N, n + m), dtype=dtype)
    H[..., :n], H[:, :-1, n:] = hx, hu
    hi, lo = SD.box_mask(cs)
    lhi, llo = (t(a) for a in SD.stack_duals(cs, duals))
    m_ = t(mu)[:, None, None]
    zero = dtype(0)
    zmax, zmin = t(np.where(np.isfinite(th.zmax), th.zmax, 0.0))[:, None], t(np.where(np.isfinite(th.zmin), th.zmin, 0.0))[:, None]
    chi, clo = Z - zmax, zmin - Z
    ahi, alo = (chi >= 0) | (lhi > 0), (clo >= 0) | (llo > 0)
    ghi = np.where(hi, lhi + np.where(ahi, m_ * chi, zero), zero)
    glo = np.where(lo, llo + np.where(alo, m_ * clo, zero), zero)
    pen = (np.where(hi, lhi * chi + np.where(ahi, half * m_ * chi * chi, zero), zero)
           + np.where(lo, llo * clo + np.where(alo, half * m_ * clo * clo, zero), zero))
    return H, w * e + (ghi - glo), val + pen.sum(axis=2)


def cost_to_go(cs, K, X, U, mode=0, codes=None, mu_pass=None, duals=None, mu=None, dtype=np.float64):
    """cs: evaluate_ref.Case; K (B, N-1, m, n), zeros for the open loop; (X, U) the trajectory held
    -> NS(P (B, N, n, n), p (B, N, n), v (B, N)), all of `dtype`"""
    t = lambda a: np.asarray(a, dtype=dtype)
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    A, Bm, K = t(cs.A), t(cs.Bm), t(K)
    H, l, val = local_terms(cs, X, U, mode, codes, mu_pass, duals, mu, dtype)
    P, p, v = np.zeros((B, N, n, n), dtype=dtype), np.zeros((B, N, n), dtype=dtype), np.zeros((B, N), dtype=dtype)
    idx = np.arange(n)
    P[:, -1, idx, idx] = H[:, -1, :n]
    p[:, -1] = l[:, -1, :n]
    v[:, -1] = val[:, -1]
    for k in range(N - 2, -1, -1):
        M = A[:, k] + Bm[:, k] @ K[:, k]
        Mt, Kt = np.swapaxes(M, -1, -2), np.swapaxes(K[:, k], -1, -2)
        Pk = Mt @ (P[:, k + 1] @ M) + Kt @ (H[:, k, n:, None] * K[:, k])
        Pk[:, idx, idx] = Pk[:, idx, idx] + H[:, k, :n]
        P[:, k] = Pk
        p[:, k] = (l[:, k, :n] + np.einsum("baj,ba->bj", K[:, k], l[:, k, n:])) + np.einsum("bij,bi->bj", M, p[:, k + 1])
        v[:, k] = val[:, k] + v[:, k + 1]
    return NS(P=P, p=p, v=v)


def quadratic(ctg, d, dtype=np.float64):
    """v_0 + p_0'd + 1/2 d'P_0 d per instance; d (B, n)"""
    d = np.asarray(d, dtype=dtype)
    return ctg.v[:, 0] + np.einsum("bi,bi->b", ctg.p[:, 0], d) + dtype(0.5) * np.einsum("bi,bij,bj->b", d, ctg.P[:, 0], d)


def trace_formula(P, Sigma0, W, dtype=np.float64):
    """1/2 <P_0, Sigma0> + 1/2 sum_{k=1..N-1} <P_k, W> per instance; Sigma0, W (n, n) or (B, n, n) or None"""
    P = np.asarray(P, dtype=dtype)
    B, N, n = P.shape[:3]
    full = lambda a: np.zeros((B, n, n), dtype=dtype) if a is None else np.broadcast_to(np.asarray(a, dtype=dtype), (B, n, n))
    half = dtype(0.5)
    return half * np.einsum("bij,bij->b", P[:, 0], full(Sigma0)) + half * np.einsum("bkij,bij->b", P[:, 1:], full(W))
