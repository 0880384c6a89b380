// warm_start.h -- the best of several candidate control sequences chosen and installed on the device
// (altro_batch_warm_start(_dev); include/altro_batch.h).  Two kernels per backend.
// The SCORING kernel is a fused rollout-and-score: one 16-lane row (16-lane backend) or one wave (one-wave-per-instance
// backend) per (instance, candidate) keeps the state in registers -- a knot's z = [x; u] is consumed for the cost, the box and
// the constraint rows and then advanced to x_{k+1} -- so no candidate state reaches memory and no workspace grows with
// ncand * N * n.  With include_current the trajectory the handle holds is one more row per instance (the incumbent, column
// ncand), its controls read from plane cur[b].  The SELECT-AND-INSTALL kernel takes one row / wave per instance: it walks the
// instance's merits in the stated order, writes `chosen`, tests the active mask and rolls the winner out once more, straight
// into plane cur[b] -- one extra rollout per instance instead of ncand state planes.
// The arithmetic is the scoring core's (evaluate.h: Ctx16 / CtxW, score16_knot / scorew_knot, score_reduce, eval16_step /
// evalw_advance): the states are those k_eval_rollout16 / k_eval_rollout_wide write, and J, c_max are the bytes
// k_eval_score16 / k_eval_score_wide give for them, because the same functions compute them.
//   merit = fma(rho, c_max, J) (one rounding); best = +Inf, chosen = -1; the incumbent first, then c = 0 .. ncand-1; a
//   candidate takes over only if merit < best -- ties stay with the earlier visit, a NaN or +Inf merit never wins.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "evaluate.h"

namespace altro {

constexpr int WS_NONE = -1;       // chosen[b]: nothing had a finite merit, instance b is left as it was
constexpr int WS_INACTIVE = -2;   // chosen[b]: the active mask leaves instance b out

// The choice among the nc1 = ncand + inc merits of one instance (J, c: its rows).  Serial on purpose: every lane of the row /
// wave walks the same few values, and the stated order is the result.
__device__ __forceinline__ int ws_select(const double* J, const double* c, int ncand, int inc, double rho) {
#pragma clang fp contract(off)
  double best = INFINITY;
  int w = WS_NONE;
  if (inc) {
    const double merit = __builtin_fma(rho, c[ncand], J[ncand]);
    if (merit < best) { best = merit; w = ncand; }
  }
  for (int q = 0; q < ncand; ++q) {
    const double merit = __builtin_fma(rho, c[q], J[q]);
    if (merit < best) { best = merit; w = q; }
  }
  return w;
}

// ------------------------------------------------------------------ 16-lane backend
// Lane layout of evaluate.h: lane j < n holds x_j, lane n + a holds u_a (0 at the terminal knot), lanes >= n + m hold 0 --
// which is a row of Z as k_pack_traj writes it.  Zp: [Bp] blocks of (2 N + 1) knots x 16 lanes, `plane` = N * 16.

// lane's control of knot 0 of column c of instance b and the stride between knots: a caller's candidate (c < ncand) or the
// plane the handle holds (the incumbent); only lanes n .. n + m - 1 read through it
__device__ __forceinline__ const double* ws16_controls(const double* U, const double* Zp, const int* cur, size_t plane, size_t b, int c, int ncand,
                                                       int N, int n, int m, int lane, bool isu, size_t& stride) {
  if (c < ncand) {
    stride = (size_t)m;
    return U + (b * (size_t)ncand + (size_t)c) * (size_t)(N - 1) * m + (isu ? lane - n : 0);
  }
  stride = 16;
  return Zp + b * (2 * (size_t)N + 1) * 16 + (size_t)cur[b] * plane + lane;
}

// J, cmax [R] <- column c = r % nc1 of instance b = r / nc1, R = batch * nc1, nc1 = ncand + inc.  rows = R padded to whole
// waves; rows >= R compute on row 0 and store nothing, so EXEC is all ones at every DPP move.
__global__ void k_ws_score16(double* __restrict__ J, double* __restrict__ cmax, const double* __restrict__ U, const double* __restrict__ Zp,
                             const int* __restrict__ cur, size_t plane, const double* __restrict__ x0, Eval16 P, int ncand, int inc, size_t R,
                             size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const size_t nc1 = (size_t)(ncand + inc);
  const auto [r, b, lane, live, in, isx, isu] = eval16_row(R, rows, nc1, n, m);
  if (!in) return;   // (whole waves only)
  const int c = (int)(r - b * nc1);
  const Ctx16 cx(P, b, lane);
  double g[16], fv;
  eval16_dyn(P, b, lane, g, fv);
  size_t us;
  const double* up = ws16_controls(U, Zp, cur, plane, b, c, ncand, N, n, m, lane, isu, us);
  Score s;
  double x = isx ? x0[b * 16 + lane] : 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const bool on = isx || (isu && !term);
    const double z = isx ? x : (on ? up[(size_t)k * us] : 0.0);
    score16_knot(s, P, cx, k, z, cx.Zr[(size_t)k * 16]);
    if (!term) x = eval16_step(g, fv, z, isx);   // z is consumed: advance it in registers
  }
  double Jr, cr;
  score_reduce<16>(s, Jr, cr);
  if (!live || lane != 0) return;
  J[r] = Jr;
  cmax[r] = cr;
}

// One row per instance slot (Bp of them, padded to whole waves; a padded slot mirrors instance B - 1, as k_pack_traj has it).
// chosen [B] may be null; active: the mask (null: none; padded slots hold 0).  A slot that installs nothing rolls candidate 0
// and stores nothing, so EXEC stays all ones.  The plane receives every lane of every knot: x, u (0 at the terminal knot), 0.
__global__ void k_ws_install16(int* __restrict__ chosen, const double* __restrict__ J, const double* __restrict__ cmax,
                               const double* __restrict__ U, double* Zp, const int* __restrict__ cur, size_t plane,
                               const double* __restrict__ x0, const int* __restrict__ active, Eval16 P, int ncand, int inc, double rho, int B,
                               int Bp, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const auto [inst, b0, lane, slot, in, isx, isu] = eval16_row((size_t)Bp, rows, 1, n, m);
  if (!in) return;   // (whole waves only)
  const size_t b = b0 < (size_t)B ? b0 : (size_t)B - 1;
  const size_t nc1 = (size_t)(ncand + inc);
  const bool masked = active != nullptr && active[inst] == 0;
  int w = ws_select(J + b * nc1, cmax + b * nc1, ncand, inc, rho);
  if (slot && inst < (size_t)B && lane == 0 && chosen != nullptr) chosen[inst] = masked ? WS_INACTIVE : w;
  const bool store = slot && !masked && w >= 0 && w <= ncand && (w < ncand || inc != 0);   // (the winner is range-checked before it addresses anything)
  if (!store) w = 0;
  double g[16], fv;
  eval16_dyn(P, b, lane, g, fv);
  size_t us;
  // (an incumbent's controls go back where they came from, unchanged; a padded slot takes those of instance B - 1, whose own
  //  row rewrites the same values meanwhile)
  const double* up = ws16_controls(U, Zp, cur, plane, b, w, ncand, N, n, m, lane, isu, us);
  double* dst = Zp + inst * (2 * (size_t)N + 1) * 16 + (size_t)cur[inst] * plane + lane;
  double x = isx ? x0[b * 16 + lane] : 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const bool on = isx || (isu && !term);
    const double z = isx ? x : (on ? up[(size_t)k * us] : 0.0);
    if (store) dst[(size_t)k * 16] = z;
    if (!term) x = eval16_step(g, fv, z, isx);
  }
}

// ------------------------------------------------------------------ one-wave-per-instance backend
// Lane layout of evaluate.h: lane T < n owns x_T, lane T < m owns u_T, lane T < Pn owns constraint row T.  Xp [B][2][N][n],
// Up [B][2][N-1][m]: the planes the handle holds.

__device__ __forceinline__ const double* wsw_controls(const double* U, const double* Up, const int* cur, size_t b, int c, int ncand, int N, int m) {
  const size_t lu = (size_t)(N - 1) * m;
  return c < ncand ? U + (b * (size_t)ncand + (size_t)c) * lu : Up + (b * 2 + (size_t)cur[b]) * lu;
}

__global__ void k_ws_score_wide(double* __restrict__ J, double* __restrict__ cmax, const double* __restrict__ U, const double* __restrict__ Up,
                                const int* __restrict__ cur, const double* __restrict__ x0, EvalW P, int ncand, int inc, size_t R) {
#pragma clang fp contract(off)
  const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int T = (int)(threadIdx.x & 63);
  if (r >= R) return;   // (whole waves)
  const size_t nc1 = (size_t)(ncand + inc), b = r / nc1;
  const int c = (int)(r - b * nc1);
  const int n = P.n, m = P.m, N = P.N;
  const CtxW cx(P, b, T, true);
  const bool isx = cx.isx;
  const double* Ur = wsw_controls(U, Up, cur, b, c, ncand, N, m);
  Score s;
  double x = isx ? x0[b * (size_t)n + T] : 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const double u = (cx.isu && !term) ? Ur[(size_t)k * m + T] : 0.0;
    scorew_knot(s, P, cx, k, x, u);
    if (!term) x = evalw_advance(cx.dyn, k, x, u, isx);   // x, u are consumed: advance in registers
  }
  double Jr, cr;
  score_reduce<64>(s, Jr, cr);
  if (T != 0) return;
  J[r] = Jr;
  cmax[r] = cr;
}

// One wave per instance; a wave that installs nothing leaves as a whole.
__global__ void k_ws_install_wide(int* __restrict__ chosen, const double* __restrict__ J, const double* __restrict__ cmax,
                                  const double* __restrict__ U, double* Xp, double* Up, const int* __restrict__ cur,
                                  const double* __restrict__ x0, const int* __restrict__ active, EvalW P, int ncand, int inc, double rho, size_t B) {
#pragma clang fp contract(off)
  const size_t b = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int T = (int)(threadIdx.x & 63);
  if (b >= B) return;   // (whole waves)
  const size_t nc1 = (size_t)(ncand + inc);
  const bool masked = active != nullptr && active[b] == 0;
  const int w = ws_select(J + b * nc1, cmax + b * nc1, ncand, inc, rho);
  if (T == 0 && chosen != nullptr) chosen[b] = masked ? WS_INACTIVE : w;
  if (masked || w < 0 || w > ncand || (w == ncand && inc == 0)) return;   // (the winner is range-checked before it addresses anything)
  const int n = P.n, m = P.m, N = P.N;
  const bool isx = T < n, isu = T < m;
  const double* Ur = wsw_controls(U, Up, cur, b, w, ncand, N, m);
  const size_t pl = b * 2 + (size_t)cur[b];
  double* Xd = Xp + pl * (size_t)N * n;
  double* Ud = Up + pl * (size_t)(N - 1) * m;
  const EvalWDyn dyn(P, b, eval_window(P.window, P.kref, b, N, P.Nt), T, P.lds_dyn != 0);
  double x = isx ? x0[b * (size_t)n + T] : 0.0;
  for (int k = 0;; ++k) {
    if (isx) Xd[(size_t)k * n + T] = x;
    if (k == N - 1) break;
    const double u = isu ? Ur[(size_t)k * m + T] : 0.0;
    if (isu) Ud[(size_t)k * m + T] = u;
    x = evalw_advance(dyn, k, x, u, isx);
  }
}

}  // namespace altro
