// simulate.h -- the stored feedback policy run in closed loop on the model, under disturbances, on the device
// (altro_batch_simulate_policy(_dev); include/altro_batch.h).  One fused kernel per backend, shaped like the
// scoring kernels of warm_start.h: one 16-lane row (16-lane backend) or one wave (one-wave-per-instance backend) per
// (instance, sample), row r = b * nsamp + s, so the rows of one instance are neighbours and share its gain rows, reference rows
// and constraint rows in cache.  The state stays in registers: per knot the policy forms u_k from x_k, the pair is consumed for
// the cost, the box and the constraint rows, and advanced to x_{k+1} (+ w_k) -- no state reaches memory unless the caller asks
// for Xout / Uout, and no workspace grows with nsamp * N * n.
// The arithmetic is that of the calls a caller would compose, because the same device functions compute it:
//   u_k      the bytes k_eval_policy / k_eval_policy_wide write for x = x_k, knot = k (policy.h: policy16_control, resp. the
//            fma chain over j; policy_add last; policy_clamp in the box range)
//   x_{k+1}  eval16_step / evalw_advance of evaluate.h; with w one more rounded addition, performed last
//   J, c_max the scoring core of evaluate.h (score16_knot / scorew_knot, score_reduce)
//   dx_max   max over k = 0 .. N-1 and i of |x_k[i] - xbar_k[i]| (eval_max: a NaN stays)
// fb[b]: 1 the stored gains are valid (kmu[b] >= 0, resp. reuse_ok and word 128 of the instance's reuse state), 0 they are not
// and the loop is open: u_k = ubar_k, clamped if asked.  Nothing the library owns is written.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "evaluate.h"
#include "policy.h"

namespace altro {

// The caller's arrays of one call, [R = batch * nsamp] rows each; any output may be null.
struct SimIO {
  const double* x0;   // [R][n], or null: the initial state the handle holds
  const double* w;    // [R][N-1][n], or null: no disturbance, no addition
  double *J, *cmax, *dxmax;   // [R]
  int* fb;            // [batch]
  double* Xout;       // [R][N][n]
  double* Uout;       // [R][N-1][m]
};

// ------------------------------------------------------------------ 16-lane backend
// Lane layout of evaluate.h and policy.h: lane j < n holds x_j, lane n + a holds u_a (0 at the terminal knot), lanes >= n + m
// hold 0.  Zp: [Bp] blocks of (2 N + 1) knots x 16 lanes, plane cur[b] (`plane` = N * 16): lane j of knot k holds xbar_k[j],
// lane n + a holds ubar_k[a].  KD [b][k (N)][a][16]: state lane j of gain row a holds K[a][j].  hx0 [Bp][16].
// rows = R padded to whole waves; rows >= R compute on row 0 and store nothing, so EXEC is all ones at every DPP move.
// What a knot needs from memory and does not depend on the state -- its gain rows, nominal row, reference row and
// disturbance -- is loaded one knot ahead, before the dependent chain of the current knot (m butterflies, then 16 FMAs).
// 165 VGPRs (two sets of gain rows, the dynamics column, a constraint row): the launch bound lets the compiler have them.
// (Measured and not kept: the gain rows loaded by every lane under a wave-uniform condition instead of by the state lanes of
//  rows with valid gains -- fewer branches, a third more data, 754 us against 650 us at the headline shape.)
__global__ void __launch_bounds__(256)
k_sim16(SimIO io, const double* __restrict__ Zp, const int* __restrict__ cur, size_t plane, const double* __restrict__ KD,
        const double* __restrict__ kmu, const double* __restrict__ hx0, Eval16 P, int nsamp, int clamp, size_t R, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const auto [r, b, lane, live, in, isx, isu] = eval16_row(R, rows, (size_t)nsamp, n, m);
  if (!in) return;   // (whole waves only)
  const bool valid = !(kmu[b] < 0.0);
  const Ctx16 c(P, b, lane);
  double g[16], fv;
  eval16_dyn(P, b, lane, g, fv);
  const double* Zn = Zp + b * (2 * (size_t)N + 1) * 16 + (size_t)cur[b] * plane + lane;
  const double* kdp = KD + b * (size_t)N * m * 16 + lane;
  const double* wr = io.w != nullptr ? io.w + r * (size_t)(N - 1) * n + (isx ? lane : 0) : nullptr;
  double* Xr = io.Xout != nullptr ? io.Xout + r * (size_t)N * n + (isx ? lane : 0) : nullptr;
  double* Ur = io.Uout != nullptr ? io.Uout + r * (size_t)(N - 1) * m + (isu ? lane - n : 0) : nullptr;
  Score s;
  double dxm = 0.0;
  double x = isx ? (io.x0 != nullptr ? io.x0[r * (size_t)n + lane] : hx0[b * 16 + lane]) : 0.0;
  // knot 0's loads
  double kd_n[16], zl_n = Zn[0], zr_n = c.Zr[0], w_n = (wr != nullptr && isx) ? wr[0] : 0.0;
#pragma unroll
  for (int a = 0; a < 16; ++a) kd_n[a] = (a < m && valid && isx) ? kdp[(size_t)a * 16] : 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const bool on = isx || (isu && !term);
    double kd[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) kd[a] = kd_n[a];
    const double zl = zl_n, zr = zr_n, wk = w_n;
    if (!term) {   // the next knot's loads go out ahead of this knot's chain (knot N - 1 has a gain block too: KD holds N)
      const size_t k1 = (size_t)k + 1;
      zl_n = Zn[k1 * 16];
      zr_n = c.Zr[k1 * 16];
      w_n = (wr != nullptr && isx && k1 < (size_t)(N - 1)) ? wr[k1 * n] : 0.0;
#pragma unroll
      for (int a = 0; a < 16; ++a) kd_n[a] = (a < m && valid && isx) ? kdp[(k1 * m + a) * 16] : 0.0;
    }
    // the policy (k_eval_policy): dx on the state lanes, one butterfly per control, the nominal control added last
    const double dx = isx ? x - zl : 0.0;
    if (isx) dxm = eval_max(dxm, fabs(dx));
    double out = zl;
    if (!term) {
#pragma unroll
      for (int a = 0; a < 16; ++a)
        if (a < m) out = policy16_control(out, kd[a], dx, valid && isx, lane == n + a, zl);   // (uniform: EXEC stays all ones at the shuffles)
      if (clamp && isu && k >= P.box_k0 && k <= P.box_k1) out = policy_clamp(out, c.zlo, c.zhi);
    }
    const double z = isx ? x : (on ? out : 0.0);
    if (live && isx && Xr != nullptr) Xr[(size_t)k * n] = x;
    if (live && on && !isx && Ur != nullptr) Ur[(size_t)k * m] = z;
    score16_knot(s, P, c, k, z, zr);
    if (!term) {   // z is consumed: advance it in registers
      x = eval16_step(g, fv, z, isx);
      if (wr != nullptr) x = x + wk;   // (wk is 0 off the state lanes)
    }
  }
  double Jr, cr;
  score_reduce<16>(s, Jr, cr);
  dxm = lanes_max<16>(dxm);
  if (!live || lane != 0) return;
  if (io.J != nullptr) io.J[r] = Jr;
  if (io.cmax != nullptr) io.cmax[r] = cr;
  if (io.dxmax != nullptr) io.dxmax[r] = dxm;
  if (io.fb != nullptr && r == b * (size_t)nsamp) io.fb[b] = valid ? 1 : 0;
}

// ------------------------------------------------------------------ one-wave-per-instance backend
// Lane layout of evaluate.h: lane T < n owns x_T, lane T < m owns u_T, lane T < Pn owns constraint row T.  Xp [B][2][N][n],
// Up [B][2][N-1][m]: the planes the handle holds, plane cur[b].  Kg [B][N-1] blocks, column-major m x n (element a + m j).
// Lane T < m forms its control with the chain s = fma(K[T][j], dx_j, s), j = 0 .. n-1 from +0 (k_eval_policy_wide), dx_j
// read from lane j (evalw_dot: the chain of evaluate.h, its loads eight at a time).
__global__ void __launch_bounds__(256)
k_sim_wide(SimIO io, const double* __restrict__ Xp, const double* __restrict__ Up, const int* __restrict__ cur, const double* __restrict__ Kg,
           const unsigned* __restrict__ bwst, int reuse_ok, const double* __restrict__ hx0, EvalW P, int nsamp, int clamp, size_t R) {
#pragma clang fp contract(off)
  const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int T = (int)(threadIdx.x & 63);
  if (r >= R) return;   // (whole waves)
  const size_t b = r / (size_t)nsamp;
  const int n = P.n, m = P.m, N = P.N;
  const bool valid = reuse_ok != 0 && bwst[b * 136 + 128] != 0u;
  const CtxW c(P, b, T, true);
  const bool isx = c.isx, isu = c.isu;
  const size_t pl = b * 2 + (size_t)cur[b];
  const double* Xn = Xp + pl * (size_t)N * n + c.Tn;
  const double* Un = Up + pl * (size_t)(N - 1) * m + c.Tm;
  const double* kg = Kg + b * (size_t)(N - 1) * n * m + c.Tm;
  const double* wr = io.w != nullptr ? io.w + r * (size_t)(N - 1) * n + c.Tn : nullptr;
  double* Xr = io.Xout != nullptr ? io.Xout + r * (size_t)N * n + c.Tn : nullptr;
  double* Ur = io.Uout != nullptr ? io.Uout + r * (size_t)(N - 1) * m + c.Tm : nullptr;
  Score s;
  double dxm = 0.0;
  double x = isx ? (io.x0 != nullptr ? io.x0[r * (size_t)n + T] : hx0[b * (size_t)n + T]) : 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const bool uon = isu && !term;
    const double wk = (wr != nullptr && !term) ? wr[(size_t)k * n] : 0.0;   // (does not depend on the state: issued first)
    const double dx = isx ? x - Xn[(size_t)k * n] : 0.0;
    if (isx) dxm = eval_max(dxm, fabs(dx));
    double u = 0.0;
    if (!term) {   // the policy (k_eval_policy_wide); every lane of the wave walks the chain, lanes >= m on row m - 1
      double sum = 0.0;
      if (valid) sum = evalw_dot(kg + (size_t)k * n * m, (size_t)m, dx, n, 0.0, true);
      double out = policy_add(Un[(size_t)k * m], sum);
      if (clamp && k >= P.box_k0 && k <= P.box_k1) out = policy_clamp(out, c.ulo, c.uhi);
      u = isu ? out : 0.0;
    }
    if (isx && Xr != nullptr) Xr[(size_t)k * n] = x;
    if (uon && Ur != nullptr) Ur[(size_t)k * m] = u;
    scorew_knot(s, P, c, k, x, u);
    if (!term) {   // x, u are consumed: advance in registers
      x = evalw_advance(c.dyn, k, x, u, isx);
      if (wr != nullptr && isx) x = x + wk;
    }
  }
  double Jr, cr;
  score_reduce<64>(s, Jr, cr);
  dxm = lanes_max<64>(dxm);
  if (T != 0) return;
  if (io.J != nullptr) io.J[r] = Jr;
  if (io.cmax != nullptr) io.cmax[r] = cr;
  if (io.dxmax != nullptr) io.dxmax[r] = dxm;
  if (io.fb != nullptr && r == b * (size_t)nsamp) io.fb[b] = valid ? 1 : 0;
}

}  // namespace altro
