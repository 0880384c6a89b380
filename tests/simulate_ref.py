"""numpy yardstick of altro_batch_simulate_policy: the stored policy u_k = ubar_k + K_k (x_k - xbar_k) run in closed loop on the
model of an evaluate_ref.Case, sample by sample, with given gains K, nominal trajectory (Xbar, Ubar), start states and additive
disturbances.  Shared by tests/test_simulate_api.py (its meaning against the CPU oracle) and tests/test_simulate_gpu.py (the
inputs of the device tests).

    x_0 = x0[b, s];  u_k = clamp(ubar_k + K_k (x_k - xbar_k));  x_{k+1} = A_k x_k + B_k u_k + f_k (+ w[b, s, k])
    J, c_max = evaluate_ref.cost / violation of the simulated pair;  dx_max = max_{k, i} |x_k[i] - xbar_k[i]|

clamp saturates the controls at the case's BOX on the knots of its range; feedback False is the open loop u_k = ubar_k."""
import numpy as np

import evaluate_ref as ER


def closed_loop(cs, K, Xbar, Ubar, x0=None, w=None, clamp=False, feedback=True):
    """K (B, N-1, m, n), Xbar (B, N, n), Ubar (B, N-1, m), x0 (B, S, n) (None: cs.x0, one sample), w (B, S, N-1, n) or None
    -> X (B, S, N, n), U (B, S, N-1, m)"""
    B, n, m, N = cs.B, cs.n, cs.m, cs.N
    if x0 is None:
        x0 = cs.x0[:, None] if w is None else np.broadcast_to(cs.x0[:, None], (B, w.shape[1], n))
    S = x0.shape[1]
    box = next((c for c in cs.cons if c.kind == "box"), None) if clamp else None
    X, U = np.zeros((B, S, N, n)), np.zeros((B, S, N - 1, m))
    X[:, :, 0] = x0
    for k in range(N - 1):
        u = np.broadcast_to(Ubar[:, None, k], (B, S, m)).copy()
        if feedback:
            u = u + np.einsum("baj,bsj->bsa", K[:, k], X[:, :, k] - Xbar[:, None, k])
        if box is not None and box.k0 <= k <= box.k1:
            u = np.minimum(np.maximum(u, box.zmin[:, None, n:]), box.zmax[:, None, n:])
        U[:, :, k] = u
        X[:, :, k + 1] = np.einsum("bij,bsj->bsi", cs.A[:, k], X[:, :, k]) + np.einsum("bij,bsj->bsi", cs.Bm[:, k], u) + cs.f[:, None, k]
        if w is not None:
            X[:, :, k + 1] += w[:, :, k]
    return X, U


def simulate(cs, K, Xbar, Ubar, x0=None, w=None, clamp=False, feedback=True):
    """(J, c_max, dx_max (B, S), X, U) of the closed loop above"""
    X, U = closed_loop(cs, K, Xbar, Ubar, x0, w, clamp, feedback)
    J = ER.cost(cs, X, U)[0]
    c = ER.violation(cs, X, U)[0]
    return J, c, np.abs(X - Xbar[:, None]).max(axis=(2, 3)), X, U


def disturbed_starts(xbar0, S, seed, rel=1e-2):
    """x0 (B, S, n) = xbar_0 + rel (1 + |xbar_0|) randn"""
    rng = np.random.default_rng(seed)
    B, n = xbar0.shape
    return np.ascontiguousarray(xbar0[:, None] + rel * (1.0 + np.abs(xbar0))[:, None] * rng.standard_normal((B, S, n)))


def disturbances(Xbar, S, seed, rel=1e-2):
    """w (B, S, N-1, n) of the same relative size, scaled by the nominal state each one is added to"""
    rng = np.random.default_rng(seed)
    B, N, n = Xbar.shape
    return np.ascontiguousarray(rel * (1.0 + np.abs(Xbar[:, None, 1:])) * rng.standard_normal((B, S, N - 1, n)))
