// sensitivity.h -- the sensitivity of the SOLUTION of the last solve, through the stored gains, on the device
// (altro_batch_solution_vjp(_dev), altro_batch_solution_jvp(_dev), altro_batch_get_gain_factors_dev; include/altro_batch.h,
// DESIGN.md 7t).  Inside the active set and penalty of the stored backward pass the problem the solve minimised is an LQ
// problem and the stored gains are its exact Riccati solution, so the derivative of its minimiser is two sweeps with what the
// solve left in memory.  For every row (instance b, seed s) and g = (gx [N][n], gu [N-1][m]),  Lin(g, xi_0) -> (s_0, xi, nu):
//   BACKWARD  s_{N-1} = gx_{N-1};  k = N-2 .. 0:  q_x = gx_k + A_k' s_{k+1},  q_u = gu_k + B_k' s_{k+1},
//             d_k = -Quu_k^-1 q_u  (Quu_k = L D L', the stored factors),  s_k = q_x + K_k' q_u
//   FORWARD   xi_0 given;  k = 0 .. N-2:  nu_k = K_k xi_k + d_k,  xi_{k+1} = A_k xi_k + B_k nu_k      (tangents: no affine term)
//   VJP  (s_0, xi, nu) = Lin((gX, gU), 0):          gx0 = s_0,  gXref_k = -(w xi_k)  (w = wd, wf at k = N-1),  gUref_k = -(wd nu_k)
//   JVP  (., xi, nu) = Lin((-(w vXref), -(wd vUref)), vx0):   dX = xi,  dU = nu
// ONE kernel per backend serves both operations (SensIO::jvp says on which side the weights are applied) and runs only the
// sweeps the call needs: the backward sweep when there is a seed, the forward sweep when xi or nu is asked for, the
// triangular solves when both run.  d_k goes from the backward to the forward sweep through a workspace in memory
// ([rows][N-1][m]); the lane that stored an element reads it back, so no fence and no second launch is needed.
// The kernels read the tables evaluate.h reads through the same structs (Eval16 / EvalW, Ctx16 / CtxW), the gains and their
// validity as policy.h addresses them and the factors of Quu; they write the caller's outputs and the workspace, nothing the
// library owns.  valid = the gains are valid AND the stored pass ran without regularisation (16-lane backend: kmu[b] >= 0;
// one-wave-per-instance backend: reuse_ok and words 128 and 129 of the instance's reuse state): without it every output of the
// instance is a quiet NaN.  No masking, no clamp; a NaN stays a NaN.
// Contraction is off and every fused multiply-add is written out.  SUMMATION ORDERS (both backends unless said)
//   seed               JVP: g = -(w * v), the product rounded; VJP: g = the caller's element; a NULL array: +0, no product
//   transposed product q = g; q = fma([A B][i][element], s_i, q) for i = 0, 1, .., n - 1 in turn   (evaluate_grad.h's)
//   L y = q_u          y_a = q_a; y_a = fma(-L[a][c], y_c, y_a) for c = 0, 1, .., a - 1 in turn
//   z = D^-1 y         z_a = y_a * (1 / D_a), the stored reciprocal: one product
//   L' w = z           w_a = z_a; w_a = fma(-L[c][a], w_c, w_a) for c = m - 1, m - 2, .., a + 1 in turn;   d_a = 0 - w_a
//   s = q_x + K' q_u   16-lane: acc = q_x; acc = fma(K[C - n][j], q_u[C - n], acc) over the lanes C = 0 .. 15 of the row in turn,
//                      the terms of the lanes that hold no control being fma(0, 0, acc);
//                      one-wave-per-instance: acc = q_x; acc = fma(K[a][j], q_u[a], acc) for a = 0, 1, .., m - 1 in turn
//   nu = K xi + d      16-lane: p_j = K[a][j] * xi_j rounded, added over the row by the xor butterfly of policy16_control
//                      (strides 8, 4, 2, 1), then d_a + sum (d_a alone when the sum is zero);
//                      one-wave-per-instance: acc = d_a; acc = fma(K[a][j], xi_j, acc) for j = 0, 1, .., n - 1 in turn
//   xi' = A xi + B nu  the dynamics sum of evaluate.h from acc = +0:  acc = fma(coefficient_j, z_j, acc), j = 0 .. n + m - 1 in turn
//   outputs            VJP: -(w * xi), -(wd * nu), the product rounded; JVP: xi, nu
#pragma once
#include "evaluate.h"
#include "policy.h"
#include "solve_wide.h"

namespace altro {

// The arrays of one call (rows R = batch * nseed, row r = b * nseed + s); any input may be null (zero), any output may be null.
struct SensIO {
  const double *inx, *inu, *in0;   // seeds / tangents: [R][N][n], [R][N-1][m], [R][n] (in0: the JVP's vx0)
  double *o0, *ox, *ou;            // s_0 [R][n] (the VJP's gx0); xi [R][N][n], nu [R][N-1][m], weighted in the VJP
  double* dws;                     // [R][N-1][m]: d_k between the sweeps (null unless both sweeps run)
  int* fb;                         // [batch]
  int jvp, bwd, fwd;               // the operation; which sweeps run
};

__device__ __forceinline__ double sens_nan() { return __builtin_nan(""); }
// -(w * v), the product rounded
__device__ __forceinline__ double sens_negw(double w, double v) {
#pragma clang fp contract(off)
  const double p = w * v;
  return -p;
}

// ------------------------------------------------------------------ the sweep core
// The per-knot bodies of the two sweeps, written once per backend and called by the kernels below and by sensitivity_data.h's
// (DESIGN.md 7w); the loops over the knots stay in the kernels.  Everything is inlined by force, so a member of SensRow that a
// kernel fills with a constant (k_sens_data*: negw = false, need_d = true) folds and that kernel keeps its own code.
// One row's view of a call: its seed arrays (null: zero) and whether they are weighted (the JVP: g = -(w v)), its slice of the
// workspace for d_k and whether d_k is needed (both sweeps run).
struct SensRow {
  const double *gx, *gu;   // [N][n], [N-1][m]
  double* d;               // [N-1][m]
  bool negw, need_d;
};

// ------------------------------------------------------------------ 16-lane backend
// One 16-lane row per (instance, seed), four per wave; rows = R padded to whole waves, rows >= R compute on row 0 and store
// nothing (eval16_row), so EXEC is all ones at every DPP move.  Lane j < n holds element j of s / xi / q_x, lane n + a element
// a of q_u / d / nu.  KD [b][k (N)][a][16]: state lane j of gain row a holds K[a][j]; control lane n + c holds entry (a, c) of
// the factors for c <= a (1 / D_a at c == a, L[a][c] below) and, for c > a, whatever the solve kernel keeps there (d: kd_drow /
// kd_dcol of solve_dpp16.h), which is masked out.  Per knot a lane loads KA[C] = element `lane` of gain row C - n for the
// control lanes C (a state lane: column `lane` of K; control lane n + a: column a of the factors, L[c][a]) and, a control lane
// only, FR[C] = element C of its own gain row (row a of the factors, L[a][C - n]).
// the gains are valid and the stored pass ran without regularisation
__device__ __forceinline__ bool sens16_valid(const double* __restrict__ kmu, size_t b) { return !(kmu[b] < 0.0); }

// gt[i] = [A B][i][lane]: the lane's column, Grow[b][lane][0..n-1], contiguous (k_eval_grad16)
__device__ __forceinline__ void sens16_col(const Eval16& P, size_t b, int lane, double (&gt)[16]) {
  const double* G = P.Grow + b * 256 + (size_t)lane * 16;
#pragma unroll
  for (int i = 0; i < 16; ++i) gt[i] = (i < P.n && lane < P.n + P.m) ? G[i] : 0.0;
}

// the lane's element of g_k
__device__ __forceinline__ double sens16_seed(const SensRow& g, const Ctx16& c, int k, int N, int n, int m) {
  const bool term = k == N - 1;
  double v = 0.0;
  bool have = false;
  if (c.isx && g.gx != nullptr) { v = g.gx[(size_t)k * n + c.lane]; have = true; }
  if (c.isu && !term && g.gu != nullptr) { v = g.gu[(size_t)k * m + (c.lane - n)]; have = true; }
  return (have && g.negw) ? sens_negw(term ? c.wf : c.wd, v) : v;
}

// q_u -> d = -Quu^-1 q_u through the factors in the control lanes of the knot's gain rows kk; KA: the lane's column of them
__device__ __forceinline__ double sens16_solve(const double* kk, const double (&KA)[16], double qu, int lane, int ua, bool isu, int n, int m) {
#pragma clang fp contract(off)
  double FR[16];
#pragma unroll
  for (int C = 0; C < 16; ++C) FR[C] = (isu && C >= n && C < lane) ? kk[(size_t)ua * 16 + C] : 0.0;
  const double dinv = isu ? kk[(size_t)ua * 16 + lane] : 0.0;
  double y = qu;
  sfor<0, 16>([&](auto cc) {   // L y = q_u: y_C is final when its turn comes
    constexpr int C = decltype(cc)::value;
    const double yc = bcast<C>(y);
    y = (isu && C >= n && C < lane) ? __builtin_fma(-FR[C], yc, y) : y;
  });
  double w = y * dinv;
  sfor<0, 16>([&](auto cc) {   // L' w = z, C = 15 .. 0
    constexpr int C = 15 - decltype(cc)::value;
    const double wc = bcast<C>(w);
    w = (isu && C > lane && C < n + m) ? __builtin_fma(-KA[C], wc, w) : w;
  });
  return 0.0 - w;
}

// knot k of the backward sweep: s_{k+1} (on the state lanes, 0 elsewhere) -> s_k; d_k into the workspace when it is needed
__device__ __forceinline__ double sens16_back_knot(const SensRow& g, const Ctx16& c, const double (&gt)[16], const double* kdp, int k, int N, int n,
                                                   int m, bool live, double s) {
#pragma clang fp contract(off)
  const int lane = c.lane, ua = c.isu ? lane - n : 0;   // ua: the control a control lane holds
  const bool isu = c.isu;
  const double* kk = kdp + (size_t)k * m * 16;
  double KA[16];
#pragma unroll
  for (int C = 0; C < 16; ++C) KA[C] = (C >= n && C < n + m && lane < n + m) ? kk[(size_t)(C - n) * 16 + lane] : 0.0;
  const double q = row_affine(gt, sens16_seed(g, c, k, N, n, m), s);   // q_x on the state lanes, q_u on the control lanes, 0 beyond
  const double qu = isu ? q : 0.0;
  if (g.need_d) {
    const double d = sens16_solve(kk, KA, qu, lane, ua, isu, n, m);
    if (live && isu) g.d[(size_t)k * m + ua] = d;
  }
  const double acc = row_affine(KA, q, qu);   // (on a control lane KA holds factors: the sum is dropped there)
  return c.isx ? acc : 0.0;
}

// the control step of knot k of the forward sweep: the row's z = [xi; nu; 0] from xi on the state lanes
__device__ __forceinline__ double sens16_control(const SensRow& g, const Ctx16& c, const double* kdp, int k, int n, int m, double xi) {
  const double* kd = kdp + (size_t)k * m * 16 + c.lane;
  const double d = (g.need_d && c.isu) ? g.d[(size_t)k * m + (c.lane - n)] : 0.0;   // (the lane's own store of the backward sweep)
  double z = xi;
  for (int a = 0; a < m; ++a) z = policy16_control(z, c.isx ? kd[(size_t)a * 16] : 0.0, xi, c.isx, c.lane == n + a, d);
  return z;
}

__global__ void __launch_bounds__(256)
k_sens16(SensIO io, const double* __restrict__ KD, const double* __restrict__ kmu, Eval16 P, int nseed, size_t R, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const Row16 row = eval16_row(R, rows, (size_t)nseed, n, m);
  if (!row.in) return;   // (whole waves only)
  const size_t r = row.r, b = row.b;
  const int lane = row.lane;
  const bool live = row.live, isx = row.isx, isu = row.isu;
  const bool valid = sens16_valid(kmu, b);
  const Ctx16 c(P, b, lane);
  const int ua = isu ? lane - n : 0;   // the control a control lane holds
  const double* kdp = KD + b * (size_t)N * m * 16;
  const SensRow g{io.inx != nullptr ? io.inx + r * (size_t)N * n : nullptr, io.inu != nullptr ? io.inu + r * (size_t)(N - 1) * m : nullptr,
                  io.dws != nullptr ? io.dws + r * (size_t)(N - 1) * m : nullptr, io.jvp != 0, io.bwd != 0 && io.fwd != 0};
  double s = 0.0;   // s_{k+1} on the state lanes, 0 elsewhere
  if (io.bwd) {
    double gt[16];
    sens16_col(P, b, lane, gt);
    s = isx ? sens16_seed(g, c, N - 1, N, n, m) : 0.0;
    for (int k = N - 2; k >= 0; --k) s = sens16_back_knot(g, c, gt, kdp, k, N, n, m, live, s);
  }
  const double nan = sens_nan();
  if (live && isx && io.o0 != nullptr) io.o0[r * (size_t)n + lane] = valid ? s : nan;
  if (live && lane == 0 && io.fb != nullptr && r == b * (size_t)nseed) io.fb[b] = valid ? 1 : 0;
  if (!io.fwd) return;
  double gd[16], fv;
  eval16_dyn(P, b, lane, gd, fv);
  double* oxr = io.ox != nullptr ? io.ox + r * (size_t)N * n : nullptr;
  double* our = io.ou != nullptr ? io.ou + r * (size_t)(N - 1) * m : nullptr;
  double xi = (isx && io.in0 != nullptr) ? io.in0[r * (size_t)n + lane] : 0.0;
  for (int k = 0;; ++k) {
    const bool term = k == N - 1;
    if (live && isx && oxr != nullptr) {
      const double v = io.jvp ? xi : sens_negw(term ? c.wf : c.wd, xi);
      oxr[(size_t)k * n + lane] = valid ? v : nan;
    }
    if (term) break;
    const double z = sens16_control(g, c, kdp, k, n, m, xi);
    if (live && isu && our != nullptr) {
      const double v = io.jvp ? z : sens_negw(c.wd, z);
      our[(size_t)k * m + ua] = valid ? v : nan;
    }
    xi = eval16_step(gd, 0.0, z, isx);
  }
}

// altro_batch_get_gain_factors_dev, 16-lane backend: the control lanes of the gain rows -> F [B][N-1][m][m], the values
// altro_batch_get_gain_factors unpacks on the host.  One thread per (instance, knot < N - 1, a, c).
__global__ void k_unpack_factors16(double* __restrict__ F, const double* __restrict__ KD, int B, int N, int n, int m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * (N - 1) * m * m) return;
  const int cc = (int)(t % m), a = (int)((t / m) % m);
  const size_t k = (t / m / m) % (size_t)(N - 1), b = t / m / m / (size_t)(N - 1);
  F[t] = cc <= a ? KD[((b * N + k) * m + a) * 16 + n + cc] : 0.0;
}

// ------------------------------------------------------------------ one-wave-per-instance backend
// One wave per (instance, seed).  Lane T < n owns element T of s / xi / q_x, lane T < m element T of q_u / d / nu.  Kg
// [B][N-1] blocks, column-major m x n (element a + m j); fac [B][N] blocks of fs = wide_fac_size(m) doubles, the packed lower
// triangle solve_wide.h's factor_solve_lane leaves: element i (i + 1) / 2 + j is L[i][j] for j < i and 1 / D_i for j == i
// (m <= 16; fac is null and both sweeps never run together where no factors are kept).  Dynamics through EvalWDynT<true>
// (evaluate.h): tstep for the transposed products, its blocks with a zero affine term for the step.
template <bool PAD>
__device__ __forceinline__ double sensw_step(const EvalWDynT<PAD>& dyn, int k, double xs, double us) {
  const int n = dyn.P.n, m = dyn.P.m, ld = evalw_ld(n, PAD);
  if (dyn.lds != nullptr) return evalw_step(dyn.lds + dyn.Tn, dyn.lds + n * ld + dyn.Tn, ld, 0.0, n, m, xs, us);
  const size_t blk = evalw_block(dyn.P, dyn.b, dyn.kref, k);
  return evalw_step(dyn.P.A + blk * n * n + dyn.Tn, dyn.P.Bm + blk * n * m + dyn.Tn, n, 0.0, n, m, xs, us);
}

// The reuse state of the instance's last backward pass as the solve kernels leave it (solve_wide.h: 136 words per instance).
struct SensWReuse {
  const unsigned* st;
  int reuse_ok;
  __device__ __forceinline__ SensWReuse(const unsigned* __restrict__ bwst, size_t b, int reuse_ok_) : st(bwst + b * 136), reuse_ok(reuse_ok_) {}
  // the gains are valid (word 128) and the stored pass ran without regularisation (word 129)
  __device__ __forceinline__ bool valid() const { return reuse_ok != 0 && st[128] != 0u && st[129] != 0u; }
  // the penalty of the stored pass (words 130-131)
  __device__ __forceinline__ double mu_pass() const { return __hiloint2double((int)st[131], (int)st[130]); }
  // the plane of the active set of the last backward pass (bits 0-1 of word 132; a zeroed state: the default roles, plane 0)
  __device__ __forceinline__ int plane() const {
    const unsigned roles = st[132];
    const int b_ = (int)(roles & 3u), q_ = (int)((roles >> 2) & 3u), a_ = (int)((roles >> 4) & 3u);
    return ((1 << b_) | (1 << q_) | (1 << a_)) == 7 ? b_ : 0;
  }
};

// the lane's element of gx_k / gu_k
__device__ __forceinline__ double sensw_seedx(const SensRow& g, const CtxW& c, int k, int N, int n) {
  if (!c.isx || g.gx == nullptr) return 0.0;
  const double v = g.gx[(size_t)k * n + c.T];
  return g.negw ? sens_negw(k == N - 1 ? c.wfx : c.wx, v) : v;
}
__device__ __forceinline__ double sensw_seedu(const SensRow& g, const CtxW& c, int k, int m) {
  if (!c.isu || g.gu == nullptr) return 0.0;
  const double v = g.gu[(size_t)k * m + c.T];
  return g.negw ? sens_negw(c.wu, v) : v;
}

// q_u -> d = -Quu^-1 q_u through the packed factors Fk of the knot (m <= 16); qu is 0 off the control lanes
__device__ __forceinline__ double sensw_solve(const double* Fk, const CtxW& c, int m, double qu) {
#pragma clang fp contract(off)
  const int T = c.T, Tm = c.Tm;
  const bool isu = c.isu;
  const int rowT = Tm * (Tm + 1) / 2;
  double fr[16], fc[16];
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) {
    fr[cc] = (isu && cc < T) ? Fk[rowT + cc] : 0.0;                          // L[T][cc]
    fc[cc] = (isu && cc > T && cc < m) ? Fk[cc * (cc + 1) / 2 + Tm] : 0.0;   // L[cc][T]
  }
  const double dinv = isu ? Fk[rowT + Tm] : 0.0;
  double y = qu;
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) {
    if (cc < m) {   // (uniform)
      const double yc = eval_readlane(y, cc);
      y = (isu && cc < T) ? __builtin_fma(-fr[cc], yc, y) : y;
    }
  }
  double w = y * dinv;
#pragma unroll
  for (int cc = 15; cc >= 0; --cc) {
    if (cc < m) {
      const double wc = eval_readlane(w, cc);
      w = (isu && cc > T) ? __builtin_fma(-fc[cc], wc, w) : w;
    }
  }
  return 0.0 - w;
}

// nu_k = K_k xi_k + d_k on the control lanes, 0 elsewhere
__device__ __forceinline__ double sensw_control(const SensRow& g, const CtxW& c, const double* Kb, int k, int n, int m, double xi) {
  const double d = (g.need_d && c.isu) ? g.d[(size_t)k * m + c.T] : 0.0;   // (the lane's own store of the backward sweep)
  const double nu = evalw_dot(Kb + (size_t)k * n * m + c.Tm, (size_t)m, xi, n, d, c.isu);   // row Tm of K: stride m
  return c.isu ? nu : 0.0;
}

__global__ void k_sens_wide(SensIO io, const double* __restrict__ Kg, const double* __restrict__ fac, int fs, const unsigned* __restrict__ bwst,
                            int reuse_ok, EvalW P, int nseed, size_t R, int use_lds) {
#pragma clang fp contract(off)
  const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int T = (int)(threadIdx.x & 63);
  if (r >= R) return;   // (whole waves)
  const size_t b = r / (size_t)nseed;
  const int n = P.n, m = P.m, N = P.N;
  const bool valid = SensWReuse(bwst, b, reuse_ok).valid();
  const CtxW c(P, b, T, false);
  const EvalWDynT<true> dyn(P, b, c.kref, T, use_lds != 0);   // (padded: tstep reads the slice transposed)
  const bool isx = c.isx, isu = c.isu;
  const double* Kb = Kg + b * (size_t)(N - 1) * n * m;
  const SensRow g{io.inx != nullptr ? io.inx + r * (size_t)N * n : nullptr, io.inu != nullptr ? io.inu + r * (size_t)(N - 1) * m : nullptr,
                  io.dws != nullptr ? io.dws + r * (size_t)(N - 1) * m : nullptr, io.jvp != 0, io.bwd != 0 && io.fwd != 0};
  double s = 0.0;
  if (io.bwd) {
    s = sensw_seedx(g, c, N - 1, N, n);
    // (the knot stands here and in k_sens_data_wide: as one function the same lines give the same loops there, 854, 209 and 223
    // instructions, but 133 or more VGPRs against the parent's 131 under every signature that returns s: DESIGN.md 7w)
    for (int k = N - 2; k >= 0; --k) {
      double qu = dyn.tstep(k, true, s, sensw_seedu(g, c, k, m), isu);
      const double qx = dyn.tstep(k, false, s, sensw_seedx(g, c, k, N, n), isx);
      qu = isu ? qu : 0.0;
      if (g.need_d) {   // (m <= 16)
        const double d = sensw_solve(fac + (b * (size_t)N + k) * fs, c, m, qu);
        if (isu) g.d[(size_t)k * m + T] = d;
      }
      const double acc = evalw_dot(Kb + (size_t)k * n * m + (size_t)c.Tn * m, 1, qu, m, qx, isx);   // column Tn of K: m consecutive doubles
      s = isx ? acc : 0.0;
    }
  }
  const double nan = sens_nan();
  if (isx && io.o0 != nullptr) io.o0[r * (size_t)n + T] = valid ? s : nan;
  if (T == 0 && io.fb != nullptr && r == b * (size_t)nseed) io.fb[b] = valid ? 1 : 0;
  if (!io.fwd) return;
  double* oxr = io.ox != nullptr ? io.ox + r * (size_t)N * n : nullptr;
  double* our = io.ou != nullptr ? io.ou + r * (size_t)(N - 1) * m : nullptr;
  double xi = (isx && io.in0 != nullptr) ? io.in0[r * (size_t)n + T] : 0.0;
  for (int k = 0;; ++k) {
    const bool term = k == N - 1;
    if (isx && oxr != nullptr) {
      const double v = io.jvp ? xi : sens_negw(term ? c.wfx : c.wx, xi);
      oxr[(size_t)k * n + T] = valid ? v : nan;
    }
    if (term) break;
    const double nu = sensw_control(g, c, Kb, k, n, m, xi);
    if (isu && our != nullptr) {
      const double v = io.jvp ? nu : sens_negw(c.wu, nu);
      our[(size_t)k * m + T] = valid ? v : nan;
    }
    const double nx = sensw_step(dyn, k, xi, nu);
    xi = isx ? nx : 0.0;
  }
}

// altro_batch_get_gain_factors_dev, one-wave-per-instance backend (m <= 16): the packed triangles -> F [B][N-1][m][m] in the
// convention of altro_batch_get_gain_factors: (a, a) = 1 / D_a, (a, c < a) = L[a][c], 0 above.
__global__ void k_unpack_factors_wide(double* __restrict__ F, const double* __restrict__ fac, int fs, int B, int N, int m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * (N - 1) * m * m) return;
  const int cc = (int)(t % m), a = (int)((t / m) % m);
  const size_t k = (t / m / m) % (size_t)(N - 1), b = t / m / m / (size_t)(N - 1);
  F[t] = cc <= a ? fac[(b * N + k) * (size_t)fs + a * (a + 1) / 2 + cc] : 0.0;
}

}  // namespace altro
