// covariance.h -- the covariance of the closed loop under the stored policy, propagated on the device
// (altro_batch_propagate_covariance(_dev); include/altro_batch.h).  With M_k = A_k + B_k K_k:
//   S_0 = Sigma0,   S_{k+1} = M_k S_k M_k' + W,   k = 0 .. N-2
// and from S_k the deviations of every state (sqrt S_k[i][i]), control (sqrt (K_k S_k K_k')[a][a]) and row of one LINEAR / SOC
// constraint (sqrt g' S_k g, g = a_x + K_k' a_u), the expected cost over the nominal and a tightened box.  One kernel per
// backend; S never reaches memory unless the caller asks for Sout, so the call allocates nothing.  The kernels read what the
// scoring kernels of evaluate.h read (Eval16 / EvalW: dynamics, weights, bounds, constraint rows, window) and the gains and
// their validity as policy.h addresses them, and write nothing the library owns.  No clamp is modelled.
// Contraction is off and every fused multiply-add is written out.  SUMMATION ORDERS
// 16-lane backend (lane i of a row holds row i of S, T, M and of [A B]; v_j = lane j's v):
//   M[i][j]        acc = A[i][j]; acc = fma(B[i][a], K[a][j], acc), a = 0 .. m-1 in turn
//   (S K_a')[i]    acc = +0; acc = fma(S[i][j], K[a][j], acc), j = 0 .. 15 in turn           (the broadcasts M uses)
//   (K S K')[a][a] p_i = K[a][i] (S K_a')[i] rounded, added over the row by an xor butterfly (strides 8, 4, 2, 1)
//   T[i][j]        acc = +0; acc = fma(M[i][l], S[l][j], acc), l = 0 .. 15 in turn
//   S'[i][j]       acc = +0; acc = fma(T[i][l], M[j][l], acc), l = 0 .. 15 in turn; then one rounded addition of W[i][j]
//   g_j            acc = a_x[j]; acc = fma(K[a][j], a_u[a], acc), a = 0 .. m-1;   (S g)[i] as (S K_a'); g' S g as (K S K')
//   dJ             every lane adds w * value knot after knot (product rounded), k = 0 .. N-1; butterfly over the row; times 0.5
// one-wave-per-instance backend (matrices in LDS, padded to np = 16 ceil(n / 16), pad zero):
//   M' = A' + K' B'   one FP64 MFMA product over a (m padded to a multiple of 4), added to A[i][l] last
//   Y = K S, T' = S' M', S' = T M'   FP64 MFMA tiles (gemm_tn of solve_wide.h: v_mfma_f64_16x16x4, k-steps of 4 in turn from
//                  +0, the four terms of a step in the order of the instruction); then one rounded addition of W[i][j]
//   (K S K')[a][a] p_j = Y[a][j] K[a][j] rounded, added over the wave by an xor butterfly (strides 32 .. 1)
//   g_j            as above;   (g' S)[j]  acc = +0; acc = fma(g_i, S[i][j], acc), i = 0 .. n-1;   g' S g: p_j = (g' S)[j] g_j, butterfly
//   dJ             as above, butterfly over the wave
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "evaluate.h"
#include "policy.h"
#include "solve_wide.h"

namespace altro {

// The caller's arrays of one call; any output may be null.
struct CovIO {
  const double *S0, *W;   // [n][n] row-major, or [batch][n][n] (pi); null: zero, and W's addition is not performed
  int pi;
  double kappa;
  double *sx, *su, *sc, *dJ;   // [batch][N][n], [batch][N-1][m], [batch][nk][p], [batch]
  int* fb;                     // [batch]
  double *zlo_t, *zhi_t;       // [batch][n + m]
  double* Sout;                // [batch][N][n][n]
};

// The rows of the LINEAR / SOC constraint whose deviations are asked for (p = 0: none), knots k0 .. k1.  16-lane backend: row
// r sits in lane (lanes >> 4 r) & 15 of the knot's table; one-wave-per-instance backend: in row r0 + r.
struct CovRows {
  int p, k0, k1, r0;
  unsigned long long lanes;
};

// max(v, 0) that keeps a NaN and never returns -0
__device__ __forceinline__ double cov_pos(double v) { return v > 0.0 ? v : (v != v ? v : 0.0); }

// The box row [lo, hi] pulled in by ks = kappa * s on every finite side, never past the midpoint
__device__ __forceinline__ void cov_tighten(double lo, double hi, double kappa, double s, double& lo_t, double& hi_t) {
#pragma clang fp contract(off)
  const bool fl = lo > -1e300, fh = hi < 1e300;
  const double ks = kappa * s;
  lo_t = lo;
  hi_t = hi;
  if (fl && fh) {
    const double mid = 0.5 * (lo + hi), a = lo + ks, b = hi - ks;
    lo_t = a > mid ? mid : a;
    hi_t = b < mid ? mid : b;
  } else if (fl) {
    lo_t = lo + ks;
  } else if (fh) {
    hi_t = hi - ks;
  }
}

// ------------------------------------------------------------------ 16-lane backend
// One 16-lane row per instance, four per wave; rows = the batch padded to whole waves, rows >= B compute on instance 0 and
// store nothing, so EXEC is all ones at every DPP move.  Lane i < n holds row i of S, T, M and [A B]; lanes >= n hold zero
// rows (their M row is zero, so their rows of T and S' are).  KD [b][k (N)][a][16]: state lane j of gain row a holds K[a][j].
// The next knot's gain rows are loaded ahead of the current knot's chain (k_sim16).

// y_i = sum_j S[i][j] v_j, j = 0 .. 15 in turn
__device__ __forceinline__ double cov16_apply(const double (&S)[16], double v) {
  double y = 0.0;
  sfor<0, 16>([&](auto j) {
    constexpr int J = decltype(j)::value;
    y = __builtin_fma(S[J], bcast<J>(v), y);
  });
  return y;
}

__global__ void __launch_bounds__(256)
k_cov16(CovIO io, CovRows cr, const double* __restrict__ KD, const double* __restrict__ kmu, Eval16 P, size_t B, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const Row16 row = eval16_row(B, rows, (size_t)1, n, m);
  if (!row.in) return;   // (whole waves only)
  const size_t b = row.b;
  const int lane = row.lane;
  const bool live = row.live, isx = row.isx, isu = row.isu;
  const bool valid = !(kmu[b] < 0.0);
  const Ctx16 c(P, b, lane);
  // the lane's row of [A B] (eval16_dyn's addressing, A and B apart: the control columns start at a run-time index)
  double ga[16], gb[16];
  {
    const double* G = P.Grow + b * 256 + lane;
#pragma unroll
    for (int j = 0; j < 16; ++j) ga[j] = (j < n && isx) ? G[j * 16] : 0.0;
#pragma unroll
    for (int a = 0; a < 16; ++a) gb[a] = (a < m && isx) ? G[(n + a) * 16] : 0.0;
  }
  const size_t mat = (io.pi ? b : 0) * (size_t)n * n + (size_t)(isx ? lane : 0) * n;
  double S[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) S[j] = (io.S0 != nullptr && isx && j < n) ? io.S0[mat + j] : 0.0;
  const double* kdp = KD + b * (size_t)N * m * 16 + lane;
  double kd_n[16];
#pragma unroll
  for (int a = 0; a < 16; ++a) kd_n[a] = (a < m && valid && isx) ? kdp[(size_t)a * 16] : 0.0;
  const int nk = cr.k1 - cr.k0 + 1;
  double cost = 0.0, smax = 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const bool inbox = k >= P.box_k0 && k <= P.box_k1;
    double kd[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) kd[a] = kd_n[a];
    if (!term) {
      const size_t k1 = (size_t)k + 1;
#pragma unroll
      for (int a = 0; a < 16; ++a) kd_n[a] = (a < m && valid && isx) ? kdp[(k1 * m + a) * 16] : 0.0;
    }
    // the states: the lane's diagonal element
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) d = lane == j ? S[j] : d;
    if (isx) {
      const double q = (term ? c.wf : c.wd) * d;
      cost = cost + q;
      const double sd = sqrt(cov_pos(d));
      if (inbox) smax = eval_max(smax, sd);
      if (live && io.sx != nullptr) io.sx[(b * (size_t)N + k) * n + lane] = sd;
      if (live && io.Sout != nullptr) {
        double* so = io.Sout + ((b * (size_t)N + k) * n + lane) * n;
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (j < n) so[j] = S[j];
      }
    }
    // M and the controls: one broadcast of K[a][j] serves M[i][j] and (S K_a')[i]
    double M[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) M[j] = ga[j];
    if (!term) {
      double uv = 0.0;
      sfor<0, 16>([&](auto a_) {
        constexpr int A = decltype(a_)::value;
        if (A < m) {   // (uniform: EXEC stays all ones at the DPP moves)
          double y = 0.0;
          sfor<0, 16>([&](auto j) {
            constexpr int J = decltype(j)::value;
            const double kb = bcast<J>(kd[A]);
            M[J] = __builtin_fma(gb[A], kb, M[J]);
            y = __builtin_fma(S[J], kb, y);
          });
          const double p = kd[A] * y;
          const double q = lanes_sum<16>(p);
          uv = lane == n + A ? q : uv;
        }
      });
      if (isu) {
        const double q = c.wd * uv;
        cost = cost + q;
        const double sd = sqrt(cov_pos(uv));
        if (inbox) smax = eval_max(smax, sd);
        if (live && io.su != nullptr) io.su[(b * (size_t)(N - 1) + k) * m + (lane - n)] = sd;
      }
    }
    // the rows of the constraint
    if (cr.p > 0 && k >= cr.k0 && k <= cr.k1) {
      for (int rr = 0; rr < cr.p; ++rr) {
        const int L = (int)((cr.lanes >> (4 * rr)) & 15ull);
        const double* ar = P.Acon + b * P.con_istride + (size_t)k * 256 + (size_t)L * 16;
        double g = isx ? ar[lane] : 0.0;
        if (!term) {
#pragma unroll
          for (int a = 0; a < 16; ++a)
            if (a < m) g = __builtin_fma(kd[a], ar[n + a], g);   // (kd is 0 off the state lanes and without valid gains)
        }
        const double y = cov16_apply(S, g);
        const double p = g * y;
        const double q = lanes_sum<16>(p);
        if (live && lane == 0 && io.sc != nullptr) io.sc[(b * (size_t)nk + (size_t)(k - cr.k0)) * cr.p + rr] = sqrt(cov_pos(q));
      }
    }
    if (term) break;
    // T = M S, S' = T M' (+ W)
    double T[16];
    sfor<0, 16>([&](auto j) {
      constexpr int J = decltype(j)::value;
      double t = 0.0;
      sfor<0, 16>([&](auto l) {
        constexpr int Lq = decltype(l)::value;
        t = __builtin_fma(M[Lq], bcast<Lq>(S[J]), t);
      });
      T[J] = t;
    });
#pragma unroll
    for (int j = 0; j < 16; ++j) S[j] = 0.0;
    sfor<0, 16>([&](auto l) {
      constexpr int Lq = decltype(l)::value;
      sfor<0, 16>([&](auto j) {
        constexpr int J = decltype(j)::value;
        S[J] = __builtin_fma(T[Lq], bcast<J>(M[Lq]), S[J]);
      });
    });
    if (io.W != nullptr) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double w = (isx && j < n) ? io.W[mat + j] : 0.0;
        S[j] = S[j] + w;
      }
    }
  }
  const double dJ = 0.5 * lanes_sum<16>(cost);
  if (!live) return;
  if (io.zlo_t != nullptr && (isx || isu)) {
    double lo_t, hi_t;
    cov_tighten(c.zlo, c.zhi, io.kappa, smax, lo_t, hi_t);
    io.zlo_t[b * (size_t)(n + m) + lane] = lo_t;
    io.zhi_t[b * (size_t)(n + m) + lane] = hi_t;
  }
  if (lane != 0) return;
  if (io.dJ != nullptr) io.dJ[b] = dJ;
  if (io.fb != nullptr) io.fb[b] = valid ? 1 : 0;
}

// ------------------------------------------------------------------ one-wave-per-instance backend
// One wave (a block of 64 threads) per instance.  LDS, in doubles, np = the padded state dimension of the handle's
// instantiation, mq = m padded to a multiple of 4, mp = m padded to 16, every pad zero:
//   Mt [np][np]  Mt[l][i] = M[i][l]          S  [np][np] row-major          Tt [max(np, mp)][np]  Y = K S, then Tt[l][i] = T[i][l]
//   Kl [mq][np]  Kl[a][l] = K[a][l]          Kt [np][mp] Kt[l][a] = K[a][l] Bl [mq][np]  Bl[a][i] = B[i][a]
// Lane T < n owns state T and column T of every row it copies (consecutive LDS addresses); lane T < m owns control T.  Kg
// [B][N-1] blocks, column-major m x n (element a + m j); A, Bm column-major blocks (evalw_block).  LDS instructions of a wave
// execute in order: the hand-over between phases needs the wave-level fence of solve_wide.h (wsync) and no barrier.
__host__ __device__ inline size_t covw_lds_doubles(int n, int m) {
  const size_t np = (size_t)altro_wide::pad16(n), mp = (size_t)altro_wide::pad16(m), mq = (size_t)((m + 3) & ~3);
  return 2 * np * np + (np > mp ? np : mp) * np + 2 * mq * np + np * mp;
}

__global__ void __launch_bounds__(64)
k_cov_wide(CovIO io, CovRows cr, const double* __restrict__ Kg, const unsigned* __restrict__ bwst, int reuse_ok, EvalW P) {
#pragma clang fp contract(off)
  using altro_wide::gemm_tn;
  using altro_wide::wsync;
  extern __shared__ double cov_lds[];
  const size_t b = blockIdx.x;
  const int T = (int)threadIdx.x;
  const int n = P.n, m = P.m, N = P.N, nz = n + m, Pn = P.Pn;
  const int np = altro_wide::pad16(n), mp = altro_wide::pad16(m), mq = (m + 3) & ~3;
  double* Mt = cov_lds;
  double* S = Mt + np * np;
  double* Tt = S + np * np;
  double* Kl = Tt + (np > mp ? np : mp) * np;
  double* Kt = Kl + mq * np;
  double* Bl = Kt + np * mp;
  const bool valid = reuse_ok != 0 && bwst[b * 136 + 128] != 0u;
  const CtxW c(P, b, T, false);
  const bool isx = c.isx, isu = c.isu;
  const int total = (int)covw_lds_doubles(n, m);
  for (int e = T; e < total; e += 64) cov_lds[e] = 0.0;
  wsync();
  const size_t mat = (io.pi ? b : 0) * (size_t)n * n;
  if (io.S0 != nullptr && isx)
    for (int i = 0; i < n; ++i) S[i * np + T] = io.S0[mat + (size_t)i * n + T];
  wsync();
  const int nk = cr.k1 - cr.k0 + 1;
  double cost = 0.0, sxmax = 0.0, sumax = 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const bool inbox = k >= P.box_k0 && k <= P.box_k1;
    if (isx) {
      const double d = S[T * np + T];
      const double q = (term ? c.wfx : c.wx) * d;
      cost = cost + q;
      const double sd = sqrt(cov_pos(d));
      if (inbox) sxmax = eval_max(sxmax, sd);
      if (io.sx != nullptr) io.sx[(b * (size_t)N + k) * n + T] = sd;
      if (io.Sout != nullptr) {
        double* so = io.Sout + (b * (size_t)N + k) * n * n + T;
        for (int i = 0; i < n; ++i) so[(size_t)i * n] = S[i * np + T];
      }
    }
    const bool fbk = valid && !term;
    if (!term) {
      // the knot's blocks into LDS: A' into Mt, B' into Bl, K into Kl and Kt
      const size_t blk = evalw_block(P, b, c.kref, k);
      const double* Ab = P.A + blk * (size_t)n * n;
      const double* Bb = P.Bm + blk * (size_t)n * m;
      const double* Kk = Kg + (b * (size_t)(N - 1) + k) * (size_t)n * m;
      if (isx) {
        for (int l = 0; l < n; ++l) Mt[l * np + T] = Ab[(size_t)l * n + T];
        if (valid) {
          for (int a = 0; a < m; ++a) Bl[a * np + T] = Bb[(size_t)a * n + T];
          for (int a = 0; a < m; ++a) Kl[a * np + T] = Kk[(size_t)T * m + a];
        }
      }
      if (valid && isu)
        for (int l = 0; l < n; ++l) Kt[l * mp + T] = Kk[(size_t)l * m + T];
      wsync();
      if (valid) {
        gemm_tn<true>(Mt, np, Kl, np, Bl, np, np, np, mq);    // Mt[l][i] += sum_a K[a][l] B[i][a]
        gemm_tn<false>(Tt, np, Kt, mp, S, np, mp, np, np);    // Y[a][j] = sum_l K[a][l] S[l][j]
        wsync();
        for (int a = 0; a < m; ++a) {
          const double p = isx ? Tt[a * np + T] * Kl[a * np + T] : 0.0;
          const double q = lanes_sum<64>(p);
          if (T == a) {
            const double qq = c.wu * q;
            cost = cost + qq;
            const double sd = sqrt(cov_pos(q));
            if (inbox) sumax = eval_max(sumax, sd);
            if (io.su != nullptr) io.su[(b * (size_t)(N - 1) + k) * m + a] = sd;
          }
        }
      } else if (isu) {   // open loop: K = 0, the controls do not deviate
        if (io.su != nullptr) io.su[(b * (size_t)(N - 1) + k) * m + T] = 0.0;
      }
    }
    // the rows of the constraint: lane j holds g_j
    if (cr.p > 0 && k >= cr.k0 && k <= cr.k1) {
      const double* Ak = P.AconT + b * P.con_istride + (size_t)k * nz * Pn;
      for (int rr = 0; rr < cr.p; ++rr) {
        const int row = cr.r0 + rr;
        double g = isx ? Ak[(size_t)T * Pn + row] : 0.0;
        if (fbk && isx)
          for (int a = 0; a < m; ++a) g = __builtin_fma(Kl[a * np + T], Ak[(size_t)(n + a) * Pn + row], g);
        double y = 0.0;
        for (int i = 0; i < n; ++i) y = __builtin_fma(eval_readlane(g, i), S[i * np + c.Tn], y);
        const double p = isx ? y * g : 0.0;
        const double q = lanes_sum<64>(p);
        if (T == 0 && io.sc != nullptr) io.sc[(b * (size_t)nk + (size_t)(k - cr.k0)) * cr.p + rr] = sqrt(cov_pos(q));
      }
    }
    if (term) break;
    wsync();
    gemm_tn<false>(Tt, np, S, np, Mt, np, np, np, np);   // Tt[l][i] = sum_j S[j][l] M[i][j] = T[i][l]
    wsync();
    gemm_tn<false>(S, np, Tt, np, Mt, np, np, np, np);   // S'[i][j] = sum_l T[i][l] M[j][l]
    wsync();
    if (io.W != nullptr && isx)
      for (int i = 0; i < n; ++i) S[i * np + T] = S[i * np + T] + io.W[mat + (size_t)i * n + T];
    wsync();
  }
  const double dJ = 0.5 * lanes_sum<64>(cost);
  if (io.zlo_t != nullptr) {
    double lo_t, hi_t;
    const size_t row = b * (size_t)nz;
    if (isx) {
      cov_tighten(c.xlo, c.xhi, io.kappa, sxmax, lo_t, hi_t);
      io.zlo_t[row + T] = lo_t;
      io.zhi_t[row + T] = hi_t;
    }
    if (isu) {
      cov_tighten(c.ulo, c.uhi, io.kappa, sumax, lo_t, hi_t);
      io.zlo_t[row + n + T] = lo_t;
      io.zhi_t[row + n + T] = hi_t;
    }
  }
  if (T != 0) return;
  if (io.dJ != nullptr) io.dJ[b] = dJ;
  if (io.fb != nullptr) io.fb[b] = valid ? 1 : 0;
}

}  // namespace altro
