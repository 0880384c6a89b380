// simulate.h -- the stored feedback policy run in closed loop on the model, under disturbances, on the device
// (altro_batch_simulate_policy(_dev); include/altro_batch.h).  One fused kernel per backend, shaped like the
// scoring kernels of warm_start.h: one 16-lane row (16-lane backend) or one wave (one-wave-per-instance backend) per
// (instance, sample), row r = b * nsamp + s, so the rows of one instance are neighbours and share its gain rows, reference rows
// and constraint rows in cache.  The state stays in registers: per knot the policy forms u_k from x_k, the pair is consumed for
// the cost, the box and the constraint rows, and advanced to x_{k+1} (+ w_k) -- no state reaches memory unless the caller asks
// for Xout / Uout, and no workspace grows with nsamp * N * n.
// The arithmetic is that of the calls a caller would compose, through their device functions, contraction off and every fused
// multiply-add written out:
//   u_k      the bytes k_eval_policy / k_eval_policy_wide write for x = x_k, knot = k (policy.h: the products on their state
//            lanes and the xor butterfly 8, 4, 2, 1, resp. the fma chain over j; policy_add last; policy_clamp in the box range)
//   x_{k+1}  row_affine / EvalWDyn::step of evaluate.h; with w one more rounded addition, performed last
//   J, c_max the per-knot terms, their order, the butterfly and the final * 0.5 of k_eval_score16 / k_eval_score_wide
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
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t row = t / 16;
  const int lane = (int)(t % 16);
  if (row >= rows) return;   // (whole waves only)
  const bool live = row < R;
  const size_t r = live ? row : 0, b = r / (size_t)nsamp;
  const int n = P.n, m = P.m, N = P.N;
  const bool isx = lane < n, isu = lane >= n && lane < n + m;
  const bool valid = !(kmu[b] < 0.0);
  const int kref = eval_window(P.window, P.kref, b, N, P.Nt);
  const unsigned e = ((unsigned)b * 16u + (unsigned)lane) & P.imask;
  const double wd = P.wd[e], wf = P.wf[e], zlo = P.zmin[e], zhi = P.zmax[e];
  const bool has_hi = zhi < 1e300, has_lo = zlo > -1e300;   // (the solve kernels' test for a finite side)
  double g[16], fv;
  eval16_dyn(P, b, lane, g, fv);
  const double* Zn = Zp + b * (2 * (size_t)N + 1) * 16 + (size_t)cur[b] * plane + lane;
  const double* kdp = KD + b * (size_t)N * m * 16 + lane;
  const double* Zr = P.Zref + (b * (size_t)P.Nt + (size_t)kref) * 16 + lane;
  const double* Ac = P.Acon + b * P.con_istride + (size_t)lane * 16;
  const double* bc = P.bcon + b * (P.con_istride / 16) + lane;
  const double* wr = io.w != nullptr ? io.w + r * (size_t)(N - 1) * n + (isx ? lane : 0) : nullptr;
  double* Xr = io.Xout != nullptr ? io.Xout + r * (size_t)N * n + (isx ? lane : 0) : nullptr;
  double* Ur = io.Uout != nullptr ? io.Uout + r * (size_t)(N - 1) * m + (isu ? lane - n : 0) : nullptr;
  const int pos = lane & 3;
  double cost = 0.0, viol = 0.0, dxm = 0.0;
  double x = isx ? (io.x0 != nullptr ? io.x0[r * (size_t)n + lane] : hx0[b * 16 + lane]) : 0.0;
  // knot 0's loads
  double kd_n[16], zl_n = Zn[0], zr_n = Zr[0], w_n = (wr != nullptr && isx) ? wr[0] : 0.0;
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
      zr_n = Zr[k1 * 16];
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
      for (int a = 0; a < 16; ++a) {
        if (a < m) {   // (uniform: EXEC stays all ones at the shuffles)
          double p = (valid && isx) ? kd[a] * dx : 0.0;
          for (int s = 8; s > 0; s >>= 1) p += __shfl_xor(p, s, 16);
          if (lane == n + a) out = policy_add(zl, p);
        }
      }
      if (clamp && isu && k >= P.box_k0 && k <= P.box_k1) out = policy_clamp(out, zlo, zhi);
    }
    const double z = isx ? x : (on ? out : 0.0);
    if (live && isx && Xr != nullptr) Xr[(size_t)k * n] = x;
    if (live && on && !isx && Ur != nullptr) Ur[(size_t)k * m] = z;
    // the score (k_eval_score16)
    {
      const double d = z - zr;
      double q = d * d;
      q = (term ? wf : wd) * q;
      cost = on ? cost + q : cost;
    }
    if (on && k >= P.box_k0 && k <= P.box_k1) {
      if (has_hi) viol = eval_max(viol, z - zhi);
      if (has_lo) viol = eval_max(viol, zlo - z);
    }
    if (P.ncrows > 0) {   // lane r owns constraint row r of the knot's table
      const int* cm = P.cmeta + ((size_t)k * 16 + lane) * 4;
      const int type = cm[0], p = cm[3];
      const bool act = type != CT_NONE && k >= cm[1] && k <= cm[2];
      double a[16], v = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) a[q] = 0.0;
      if (act) {
        const double* ar = Ac + (size_t)k * 256;
#pragma unroll
        for (int q = 0; q < 16; ++q) a[q] = q < n + m ? ar[q] : 0.0;
        v = bc[(size_t)k * 16];
      }
      v = row_affine(a, v, z);
      const bool is_soc = type == CT_SOC;
      const bool row_on = act && (!is_soc || pos < p);
      const double vv = (row_on && is_soc) ? v : 0.0;
      double vq[4];
      vq[0] = quad_bcast<0>(vv); vq[1] = quad_bcast<1>(vv); vq[2] = quad_bcast<2>(vv); vq[3] = quad_bcast<3>(vv);
      const double cv = is_soc ? soc_row_violation(vq, p, pos) : (type == CT_EQ ? fabs(v) : v);
      if (row_on) viol = eval_max(viol, cv);
    }
    if (!term) {   // z is consumed: advance it in registers
      double nx = row_affine(g, fv, z);
      if (wr != nullptr) nx = nx + wk;
      x = isx ? nx : 0.0;
    }
  }
  for (int s = 8; s > 0; s >>= 1) {
    cost += __shfl_xor(cost, s, 16);
    viol = eval_max(viol, __shfl_xor(viol, s, 16));
    dxm = eval_max(dxm, __shfl_xor(dxm, s, 16));
  }
  if (!live || lane != 0) return;
  if (io.J != nullptr) io.J[r] = 0.5 * cost;
  if (io.cmax != nullptr) io.cmax[r] = viol;
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
  const int n = P.n, m = P.m, N = P.N, nz = P.n + P.m, Pn = P.Pn;
  const bool isx = T < n, isu = T < m, isr = T < Pn;
  const int Tn = isx ? T : n - 1, Tm = isu ? T : m - 1;
  const bool valid = reuse_ok != 0 && bwst[b * 136 + 128] != 0u;
  const int kref = eval_window(P.window, P.kref, b, N, P.Nt);
  const double* wdi = P.wd + b * (size_t)P.w_pi * nz;
  const double* wfi = P.wf + b * (size_t)P.w_pi * n;
  const double* zlo = P.zmin + b * (size_t)P.b_pi * nz;
  const double* zhi = P.zmax + b * (size_t)P.b_pi * nz;
  const double wx = wdi[Tn], wfx = wfi[Tn], wu = wdi[n + Tm];
  const double xlo = zlo[Tn], xhi = zhi[Tn], ulo = zlo[n + Tm], uhi = zhi[n + Tm];
  const size_t pl = b * 2 + (size_t)cur[b];
  const double* Xn = Xp + pl * (size_t)N * n + Tn;
  const double* Un = Up + pl * (size_t)(N - 1) * m + Tm;
  const double* kg = Kg + b * (size_t)(N - 1) * n * m + Tm;
  const double* Xf = P.Xref + (b * (size_t)P.Nt + (size_t)kref) * n;
  const double* Uf = P.Uref + (b * (size_t)(P.Nt - 1) + (size_t)kref) * m;
  const double* At = P.AconT + b * P.con_istride + (isr ? T : 0);
  const double* bc = P.bcon + b * P.bcon_istride + (isr ? T : 0);
  const int c0 = isr ? P.rowc0[T] : 0, cp = isr ? P.rowcp[T] : 0;
  const double* wr = io.w != nullptr ? io.w + r * (size_t)(N - 1) * n + Tn : nullptr;
  double* Xr = io.Xout != nullptr ? io.Xout + r * (size_t)N * n + Tn : nullptr;
  double* Ur = io.Uout != nullptr ? io.Uout + r * (size_t)(N - 1) * m + Tm : nullptr;
  extern __shared__ double eval_lds[];
  const EvalWDyn dyn(P, b, kref, T, Tn, eval_lds + (threadIdx.x >> 6) * evalw_lds_doubles(n, m), true);
  double cost = 0.0, viol = 0.0, dxm = 0.0;
  double x = isx ? (io.x0 != nullptr ? io.x0[r * (size_t)n + T] : hx0[b * (size_t)n + T]) : 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const bool uon = isu && !term;
    const double wk = (wr != nullptr && !term) ? wr[(size_t)k * n] : 0.0;   // (does not depend on the state: issued first)
    const double dx = isx ? x - Xn[(size_t)k * n] : 0.0;
    if (isx) dxm = eval_max(dxm, fabs(dx));
    double u = 0.0;
    if (!term) {   // the policy (k_eval_policy_wide); every lane of the wave walks the chain, lanes >= m on row m - 1
      double s = 0.0;
      if (valid) s = evalw_dot(kg + (size_t)k * n * m, (size_t)m, dx, n, 0.0, true);
      double out = policy_add(Un[(size_t)k * m], s);
      if (clamp && k >= P.box_k0 && k <= P.box_k1) out = policy_clamp(out, ulo, uhi);
      u = isu ? out : 0.0;
    }
    if (isx && Xr != nullptr) Xr[(size_t)k * n] = x;
    if (uon && Ur != nullptr) Ur[(size_t)k * m] = u;
    // the score (k_eval_score_wide)
    if (isx) {
      const double d = x - Xf[(size_t)k * n + T];
      double q = d * d;
      q = (term ? wfx : wx) * q;
      cost += q;
    }
    if (uon) {
      const double d = u - Uf[(size_t)k * m + T];
      double q = d * d;
      q = wu * q;
      cost += q;
    }
    if (k >= P.box_k0 && k <= P.box_k1) {
      if (isx && xhi < 1e300) viol = eval_max(viol, x - xhi);
      if (isx && xlo > -1e300) viol = eval_max(viol, xlo - x);
      if (uon && uhi < 1e300) viol = eval_max(viol, u - uhi);
      if (uon && ulo > -1e300) viol = eval_max(viol, ulo - u);
    }
    if (Pn > 0) {
      const int ct = isr ? P.ctype[(size_t)k * Pn + T] : 0;
      const bool on = ct != 0;
      const double* Ak = At + (size_t)k * nz * Pn;
      double v = on ? bc[(size_t)k * Pn] : 0.0;
      v = evalw_dot(Ak, (size_t)Pn, x, n, v, on);
      if (!term) v = evalw_dot(Ak + (size_t)n * Pn, (size_t)Pn, u, m, v, on);
      double vq[4];   // (every lane of the wave is here: the shuffles read live lanes)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double s = __shfl(v, (c0 + q) & 63, 64);
        vq[q] = q < cp ? s : 0.0;
      }
      const double cv = ct == 3 ? soc_row_violation(vq, cp, T - c0) : (ct == 1 ? fabs(v) : v);
      if (on) viol = eval_max(viol, cv);
    }
    if (!term) {   // x, u are consumed: advance in registers
      double nx = dyn.step(k, x, u);
      if (wr != nullptr) nx = nx + wk;
      x = isx ? nx : 0.0;
    }
  }
  for (int s = 32; s > 0; s >>= 1) {
    cost += __shfl_xor(cost, s, 64);
    viol = eval_max(viol, __shfl_xor(viol, s, 64));
    dxm = eval_max(dxm, __shfl_xor(dxm, s, 64));
  }
  if (T != 0) return;
  if (io.J != nullptr) io.J[r] = 0.5 * cost;
  if (io.cmax != nullptr) io.cmax[r] = viol;
  if (io.dxmax != nullptr) io.dxmax[r] = dxm;
  if (io.fb != nullptr && r == b * (size_t)nsamp) io.fb[b] = valid ? 1 : 0;
}

}  // namespace altro
