// cost_to_go.h -- the quadratic cost-to-go of the stored policy around the trajectory the handle holds, on the device
// (altro_batch_cost_to_go(_dev); include/altro_batch.h):
//   V_k(x) = v_k + p_k' (x - xbar_k) + 1/2 (x - xbar_k)' P_k (x - xbar_k)
// With M_k = A_k + B_k K_k, the diagonal Hessian H = (Hx, Hu) and the local term l = (lx, lu) of a knot:
//   P_{N-1} = Hx,   P_k = Hx + K_k' Hu K_k + M_k' P_{k+1} M_k
//   p_{N-1} = lx,   p_k = lx + K_k' lu + M_k' p_{k+1}
//   v_{N-1} = the knot's value,   v_k = the knot's value + v_{k+1},   k = N-2 .. 0
// the transpose of the recursion covariance.h runs (S' = M S M' + W).
//   mode 0, the plain cost:  H = w, l = w e (e = z - zref), the knot's value its term of J of evaluate.h.  Gains that are not valid
//           (policy.h's rule): K = 0, the open loop, and fb = 0.
//   mode 1, the augmented Lagrangian inside the active set of the stored pass (box terms only):  H = hz (sensitivity_data.h's
//           sensd_hz of the stored set and penalty), l = w e + g_hi - g_lo and the knot's value its terms of L_A as evaluate_al.h
//           has them (al_lin: its g is sensd_side's), with the duals and the penalty the handle holds.  Valid by
//           sensitivity_data.h's rule (sensd16_valid / sensdw_valid); otherwise every output of the instance is a quiet NaN.
// One kernel per backend.  P lives in registers (16-lane backend) or LDS (one-wave-per-instance backend) and reaches memory only
// through the caller's P / P0, so the call allocates nothing.  The kernels read what covariance.h and sensitivity_data.h read and
// write nothing the library owns.  No masking, no clamp; a NaN stays a NaN.  P is stored as computed, not re-symmetrised.
// Contraction is off and every fused multiply-add is written out.  SUMMATION ORDERS
// both backends (the lane that owns an element forms its terms):
//   e, l           e = z - zref rounded first; ge = w * e;  mode 1: l = ge + (g_hi - g_lo)
//   knot's value   the lane adds its w (e e) (cost_term of evaluate.h) to cost and, mode 1, al_lin's terms to pen: upper side, then
//                  lower side (one-wave-per-instance backend: the state element first, then the control element), knot after knot,
//                  k = N-1 .. 0;  v_k = 0.5 * (cost over the lanes) + (pen over the lanes), each by evaluate.h's butterfly
// 16-lane backend (lane i of a row holds row i of P, T and of M', and element i of p; K[a][i] is the lane's own gain element):
//   M'[i][l]       acc = A[l][i]; acc = fma(K[a][i], B[l][a], acc), a = 0 .. m-1 in turn      (the bits of covariance.h's M[l][i])
//   T[i][j]        acc = +0; acc = fma(P[i][l], M[l][j], acc), l = 0 .. 15 in turn            (T = P M)
//   P'[i][j]       acc = +0; acc = fma(M'[i][l], T[l][j], acc), l = 0 .. 15 in turn;          (M' T)
//                  then acc = fma(K[a][i] * Hu[a] (rounded), K[a][j], acc), a = 0 .. m-1 in turn;  then, i = j: one rounded addition of Hx[i]
//   p'[i]          acc = lx[i]; acc = fma(K[a][i], lu[a], acc), a = 0 .. m-1; acc = fma(M'[i][l], p[l], acc), l = 0 .. 15 in turn
// one-wave-per-instance backend (matrices in LDS, padded to np = 16 ceil(n / 16), pad zero; the n^3 products are FP64 MFMA tiles:
// gemm_tn of solve_wide.h, v_mfma_f64_16x16x4, k-steps of 4 in turn from +0, the four terms of a step in the order of the instruction):
//   M = A + B K    one product over a (m padded to a multiple of 4), added to A[l][j] last
//   Tt = P' M      Tt[j][i] = sum_l P[l][j] M[l][i]
//   P' = Tt' M     P'[i][j] = sum_l Tt[l][i] M[l][j];  then one product (K Hu)' K over a, KH[a][i] = Hu[a] * K[a][i] rounded, added
//                  last;  then, i = j: one rounded addition of Hx[i]
//   p'[i]          as above, l = 0 .. n-1
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "evaluate.h"
#include "evaluate_al.h"
#include "policy.h"
#include "sensitivity_data.h"
#include "solve_wide.h"

namespace altro {

// The caller's arrays of one call (include/altro_batch.h: altro_ctg_out); any may be null.
struct CtgIO {
  double *P0, *p0, *v0;   // [batch][n][n], [batch][n], [batch]
  double *P, *p, *v;      // [batch][N][n][n], [batch][N][n], [batch][N]
  int* fb;                // [batch]
  int mode;
  const double *Lb, *mu;  // mode 1: the box duals and the penalty as the solve kernels keep them (evaluate_al.h)
  const int* bslot;       // 16-lane backend: [16] slot of the lane's element in the compact box rows
  int nbp;
};

// the knot's value from the sums over the lanes
__device__ __forceinline__ double ctg_value(double cost, double pen) {
#pragma clang fp contract(off)
  const double h = 0.5 * cost;
  return h + pen;
}

// ------------------------------------------------------------------ 16-lane backend
// One 16-lane row per instance, four per wave, in the layout of k_cov16: rows = the batch padded to whole waves, rows >= B
// compute on instance 0 and store nothing, so EXEC is all ones at every DPP move.  Lane i < n holds row i of P, T and M' and
// element i of p; lane n + a holds Hu[a] and lu[a], which the state lanes fetch by a shuffle inside the row.  The lane's row of
// M' is formed directly: column i of A (gt) plus K[a][i] B[.][a], B[l][a] broadcast from lane l's row of B (gb).  KD as in
// covariance.h; the gain rows and the trajectory row of the next (lower) knot are loaded ahead of the current knot's chain.
// Zp: the planes the handle holds (simulate.h).  ahash: the lane's two bits per knot (mode 1; the host refuses N > ASET_MAXN).
__global__ void __launch_bounds__(256)
k_ctg16(CtgIO io, const double* __restrict__ Zp, const int* __restrict__ cur, size_t plane, const double* __restrict__ KD,
        const double* __restrict__ kmu, const ASet* __restrict__ ahash, Eval16 P, size_t B, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const Row16 row = eval16_row(B, rows, (size_t)1, n, m);
  if (!row.in) return;   // (whole waves only)
  const size_t b = row.b;
  const int lane = row.lane;
  const bool live = row.live, isx = row.isx, isu = row.isu;
  const bool al = io.mode != 0;
  const bool gains = sens16_valid(kmu, b);                       // policy.h's rule: the gains are there
  const bool valid = al ? sensd16_valid(kmu, io.mu, b) : gains;  // what fb reports
  const bool good = !al || valid;                                // false: every output is a quiet NaN
  const double mup = kmu[b];
  const double mu = al ? io.mu[b] : 0.0;
  const Ctx16 c(P, b, lane);
  // column `lane` of A and the lane's row of B
  double gt[16], gb[16];
  {
    const double* G = P.Grow + b * 256;
#pragma unroll
    for (int i = 0; i < 16; ++i) gt[i] = (i < n && isx) ? G[(size_t)lane * 16 + i] : 0.0;
#pragma unroll
    for (int a = 0; a < 16; ++a) gb[a] = (a < m && isx) ? G[(size_t)(n + a) * 16 + lane] : 0.0;
  }
  const double* Zn = Zp + b * (2 * (size_t)N + 1) * 16 + (size_t)cur[b] * plane + lane;
  const unsigned* aw = al ? ahash[b * 16 + lane].w : nullptr;
  const int sl = al ? io.bslot[lane] : -1;
  const double* Lbr = al ? io.Lb + b * (size_t)(N + 1) * 2 * io.nbp + (sl >= 0 ? sl : 0) : nullptr;
  double cost = 0.0, pen = 0.0;
  // the lane's element at knot k: its Hessian entry hz and local term l (0 where the row holds no element), its share of the
  // knot's value added to cost / pen
  auto local = [&](int k, double zl, double zr, double& hz, double& l) __attribute__((always_inline)) {
    const bool term = k == N - 1;
    const bool on = isx || (isu && !term);
    const double w = term ? c.wf : c.wd;
    const double q = cost_term(w, zl, zr);
    cost = on ? cost + q : cost;
    const double e = on ? zl - zr : 0.0;
    const double ge = w * e;
    double h = w, g = ge;
    if (al) {
      double ghi = 0.0, glo = 0.0;
      if (k >= P.box_k0 && k <= P.box_k1) {
        const BoxSides s = box_sides(on, zl, c.zlo, c.zhi);
        if (s.has_hi) ghi = al_lin(pen, s.over(), sl >= 0 ? Lbr[(size_t)k * 2 * io.nbp] : 0.0, mu, false);
        if (s.has_lo) glo = al_lin(pen, s.under(), sl >= 0 ? Lbr[((size_t)k * 2 + 1) * io.nbp] : 0.0, mu, false);
      }
      const double cz = ghi - glo;
      g = ge + cz;
      h = sensd_hz(w, mup, on ? (aw[k >> 4] >> ((k & 15) * 2)) & 3u : 0u);
    }
    hz = on ? h : 0.0;
    l = on ? g : 0.0;
  };
  const double nan = sens_nan();
  // knot k's outputs: the lane's row of P, its element of p, the value
  auto store = [&](int k, const double (&Pr)[16], double pv) __attribute__((always_inline)) {
    if (io.v != nullptr || k == 0) {
      const double vk = ctg_value(lanes_sum<16>(cost), lanes_sum<16>(pen));
      if (live && lane == 0) {
        if (io.v != nullptr) io.v[b * (size_t)N + k] = good ? vk : nan;
        if (k == 0 && io.v0 != nullptr) io.v0[b] = good ? vk : nan;
      }
    }
    if (!live || !isx) return;
    if (io.p != nullptr) io.p[(b * (size_t)N + k) * n + lane] = good ? pv : nan;
    if (k == 0 && io.p0 != nullptr) io.p0[b * (size_t)n + lane] = good ? pv : nan;
    double* po = io.P != nullptr ? io.P + ((b * (size_t)N + k) * n + lane) * n : nullptr;
    double* p0o = (k == 0 && io.P0 != nullptr) ? io.P0 + (b * (size_t)n + lane) * n : nullptr;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < n && po != nullptr) po[j] = good ? Pr[j] : nan;
      if (j < n && p0o != nullptr) p0o[j] = good ? Pr[j] : nan;
    }
  };
  // the terminal knot
  double Pr[16], pv;
  {
    double hz, l;
    local(N - 1, Zn[(size_t)(N - 1) * 16], c.Zr[(size_t)(N - 1) * 16], hz, l);
#pragma unroll
    for (int j = 0; j < 16; ++j) Pr[j] = (lane == j && isx) ? hz : 0.0;
    pv = isx ? l : 0.0;
  }
  store(N - 1, Pr, pv);
  const double* kdp = KD + b * (size_t)N * m * 16 + lane;
  double kd_n[16], zl_n, zr_n;
  {
    const size_t k1 = (size_t)(N - 2);
#pragma unroll
    for (int a = 0; a < 16; ++a) kd_n[a] = (a < m && gains && isx) ? kdp[(k1 * m + a) * 16] : 0.0;
    zl_n = Zn[k1 * 16];
    zr_n = c.Zr[k1 * 16];
  }
  for (int k = N - 2; k >= 0; --k) {
    double kd[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) kd[a] = kd_n[a];
    const double zl = zl_n, zr = zr_n;
    if (k > 0) {
      const size_t k1 = (size_t)k - 1;
#pragma unroll
      for (int a = 0; a < 16; ++a) kd_n[a] = (a < m && gains && isx) ? kdp[(k1 * m + a) * 16] : 0.0;
      zl_n = Zn[k1 * 16];
      zr_n = c.Zr[k1 * 16];
    }
    double hz, l;
    local(k, zl, zr, hz, l);
    // the lane's row of M'
    double Mt[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) Mt[i] = gt[i];
    sfor<0, 16>([&](auto a_) {
      constexpr int A = decltype(a_)::value;
      if (A < m) {   // (uniform: EXEC stays all ones at the DPP moves)
        sfor<0, 16>([&](auto l_) {
          constexpr int L = decltype(l_)::value;
          Mt[L] = __builtin_fma(kd[A], bcast<L>(gb[A]), Mt[L]);
        });
      }
    });
    // T = P M: M[l][j] is lane j's M'[j][l]
    double T[16];
    sfor<0, 16>([&](auto j) {
      constexpr int J = decltype(j)::value;
      double t = 0.0;
      sfor<0, 16>([&](auto l_) {
        constexpr int L = decltype(l_)::value;
        t = __builtin_fma(Pr[L], bcast<J>(Mt[L]), t);
      });
      T[J] = t;
    });
    // P' = M' T
#pragma unroll
    for (int j = 0; j < 16; ++j) Pr[j] = 0.0;
    sfor<0, 16>([&](auto l_) {
      constexpr int L = decltype(l_)::value;
      sfor<0, 16>([&](auto j) {
        constexpr int J = decltype(j)::value;
        Pr[J] = __builtin_fma(Mt[L], bcast<L>(T[J]), Pr[J]);
      });
    });
    // + K' Hu K, p' = lx + K' lu + M' p
    double acc = isx ? l : 0.0;
    sfor<0, 16>([&](auto a_) {
      constexpr int A = decltype(a_)::value;
      if (A < m) {
        const double hu = __shfl(hz, n + A, 16), lu = __shfl(l, n + A, 16);
        const double kh = kd[A] * hu;
        sfor<0, 16>([&](auto j) {
          constexpr int J = decltype(j)::value;
          Pr[J] = __builtin_fma(kh, bcast<J>(kd[A]), Pr[J]);
        });
        acc = __builtin_fma(kd[A], lu, acc);
      }
    });
    // + Hx on the diagonal
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const double d = Pr[j] + hz;
      Pr[j] = (lane == j && isx) ? d : Pr[j];
    }
    const double pn = row_affine(Mt, acc, pv);
    pv = isx ? pn : 0.0;
    store(k, Pr, pv);
  }
  if (live && lane == 0 && io.fb != nullptr) io.fb[b] = valid ? 1 : 0;
}

// ------------------------------------------------------------------ one-wave-per-instance backend
// One wave (a block of 64 threads) per instance.  LDS, in doubles, np = the padded state dimension of the handle's instantiation,
// mq = m padded to a multiple of 4, every pad zero:
//   Pm [np][np]    row-major P                      Tt [np][np]  Tt[j][i] = sum_l P[l][j] M[l][i]
//   Mm [np][np+1]  row-major M = A + B K (the odd leading dimension keeps the lanes' rows on different banks when lane l copies
//                  row l of the column-major A)
//   Kl [mq][np]    Kl[a][j] = K[a][j]               Bl [mq][np]  Bl[a][l] = B[l][a], then KH[a][i] = Hu[a] K[a][i]
// so every product has its left operand transposed in place (gemm_tn's AT): M += Bl' Kl, Tt = Pm' Mm, Pm = Tt' Mm, Pm += KH' Kl.
// Lane T < n owns state T, column T of every row it copies and element T of p; lane T < m owns control T.  Kg, A, Bm as in
// covariance.h; Xp, Up, aset as in sensitivity_data.h.  LDS instructions of a wave execute in order: the hand-over between
// phases needs the wave-level fence of solve_wide.h (wsync) and no barrier.
__host__ __device__ inline size_t ctgw_lds_doubles(int n, int m) {
  const size_t np = (size_t)altro_wide::pad16(n), mq = (size_t)((m + 3) & ~3);
  return 2 * np * np + np * (np + 1) + 2 * mq * np;
}

__global__ void __launch_bounds__(64)
k_ctg_wide(CtgIO io, const double* __restrict__ Xp, const double* __restrict__ Up, const int* __restrict__ cur, const double* __restrict__ Kg,
           const unsigned* __restrict__ bwst, const unsigned char* __restrict__ aset, int reuse_ok, EvalW P) {
#pragma clang fp contract(off)
  using altro_wide::gemm_tn;
  using altro_wide::wsync;
  extern __shared__ double ctg_lds[];
  const size_t b = blockIdx.x;
  const int T = (int)threadIdx.x;
  const int n = P.n, m = P.m, N = P.N, nz = n + m;
  const int np = altro_wide::pad16(n), mq = (m + 3) & ~3, ldm = np + 1;
  double* Pm = ctg_lds;
  double* Tt = Pm + np * np;
  double* Mm = Tt + np * np;
  double* Kl = Mm + np * ldm;
  double* Bl = Kl + mq * np;
  const bool al = io.mode != 0;
  const SensWReuse st(bwst, b, reuse_ok);
  const bool gains = reuse_ok != 0 && bwst[b * 136 + 128] != 0u;   // covariance.h's rule: the gains are there
  const bool valid = al ? sensdw_valid(st, io.mu, b) : gains;      // what fb reports
  const bool good = !al || valid;                                  // false: every output is a quiet NaN
  // (mode 0 reads neither the penalty of the stored pass nor the active set: it does not depend on their being there)
  const double mup = al ? st.mu_pass() : 0.0;
  const double mu = al ? io.mu[b] : 0.0;
  const CtxW c(P, b, T, false);
  const bool isx = c.isx, isu = c.isu;
  const int Tn = c.Tn, Tm = c.Tm;
  const unsigned char* ap = al ? aset + ((b * 3 + (size_t)st.plane()) * (size_t)N) * 64 + T : nullptr;   // the lane's byte of knot 0
  const size_t pl = b * 2 + (size_t)cur[b];
  const double* Xn = Xp + pl * (size_t)N * n + Tn;
  const double* Un = Up + pl * (size_t)(N - 1) * m + Tm;
  const double* Lbx = al ? io.Lb + b * (size_t)N * 2 * nz + Tn : nullptr;
  const double* Lbu = al ? io.Lb + b * (size_t)N * 2 * nz + n + Tm : nullptr;
  const int total = (int)ctgw_lds_doubles(n, m);
  for (int e = T; e < total; e += 64) ctg_lds[e] = 0.0;
  wsync();
  double cost = 0.0, pen = 0.0;
  // the lane's state and control element at knot k: Hessian entries and local terms (0 where the lane owns none), their share of
  // the knot's value added to cost / pen
  auto local = [&](int k, double& hx, double& lx, double& hu, double& lu) __attribute__((always_inline)) {
    const bool term = k == N - 1;
    const bool uon = isu && !term;
    const double x = isx ? Xn[(size_t)k * n] : 0.0;
    const double u = uon ? Un[(size_t)k * m] : 0.0;
    const double xr = c.Xf[(size_t)k * n + Tn], ur = uon ? c.Uf[(size_t)k * m + Tm] : 0.0;
    const double wx = term ? c.wfx : c.wx;
    if (isx) cost = cost + cost_term(wx, x, xr);
    if (uon) cost = cost + cost_term(c.wu, u, ur);
    const double ex = isx ? x - xr : 0.0, eu = uon ? u - ur : 0.0;
    const double gex = wx * ex, geu = c.wu * eu;
    double hxv = wx, huv = c.wu, gx = gex, gu = geu;
    if (al) {
      double xhi = 0.0, xlo = 0.0, uhi = 0.0, ulo = 0.0;
      if (k >= P.box_k0 && k <= P.box_k1) {
        const BoxSides sx = box_sides(isx, x, c.xlo, c.xhi), su = box_sides(uon, u, c.ulo, c.uhi);
        if (sx.has_hi) xhi = al_lin(pen, sx.over(), Lbx[(size_t)k * 2 * nz], mu, false);
        if (sx.has_lo) xlo = al_lin(pen, sx.under(), Lbx[((size_t)k * 2 + 1) * nz], mu, false);
        if (su.has_hi) uhi = al_lin(pen, su.over(), Lbu[(size_t)k * 2 * nz], mu, false);
        if (su.has_lo) ulo = al_lin(pen, su.under(), Lbu[((size_t)k * 2 + 1) * nz], mu, false);
      }
      const double cx = xhi - xlo, cu = uhi - ulo;
      gx = gex + cx;
      gu = geu + cu;
      const unsigned cd = ap[(size_t)k * 64];
      hxv = sensd_hz(wx, mup, isx ? (cd & 3u) : 0u);
      huv = sensd_hz(c.wu, mup, uon ? ((cd >> 2) & 3u) : 0u);
    }
    hx = isx ? hxv : 0.0;
    lx = isx ? gx : 0.0;
    hu = uon ? huv : 0.0;
    lu = uon ? gu : 0.0;
  };
  const double nan = sens_nan();
  // knot k's outputs: lane T stores column T of every row of P, element T of p; lane 0 the value
  auto store = [&](int k, double pv) __attribute__((always_inline)) {
    if (io.v != nullptr || k == 0) {
      const double vk = ctg_value(lanes_sum<64>(cost), lanes_sum<64>(pen));
      if (T == 0) {
        if (io.v != nullptr) io.v[b * (size_t)N + k] = good ? vk : nan;
        if (k == 0 && io.v0 != nullptr) io.v0[b] = good ? vk : nan;
      }
    }
    if (!isx) return;
    if (io.p != nullptr) io.p[(b * (size_t)N + k) * n + T] = good ? pv : nan;
    if (k == 0 && io.p0 != nullptr) io.p0[b * (size_t)n + T] = good ? pv : nan;
    double* po = io.P != nullptr ? io.P + (b * (size_t)N + k) * n * n + T : nullptr;
    double* p0o = (k == 0 && io.P0 != nullptr) ? io.P0 + b * (size_t)n * n + T : nullptr;
    if (po == nullptr && p0o == nullptr) return;
    for (int i = 0; i < n; ++i) {
      const double v = good ? Pm[i * np + T] : nan;
      if (po != nullptr) po[(size_t)i * n] = v;
      if (p0o != nullptr) p0o[(size_t)i * n] = v;
    }
  };
  // the terminal knot
  double pv;
  {
    double hx, lx, hu, lu;
    local(N - 1, hx, lx, hu, lu);
    if (isx) Pm[T * np + T] = hx;
    pv = lx;
  }
  wsync();
  store(N - 1, pv);
  for (int k = N - 2; k >= 0; --k) {
    double hx, lx, hu, lu;
    local(k, hx, lx, hu, lu);
    // the knot's blocks into LDS: A into Mm (lane l copies row l), B' into Bl, K into Kl
    const size_t blk = evalw_block(P, b, c.kref, k);
    const double* Ab = P.A + blk * (size_t)n * n;
    const double* Bb = P.Bm + blk * (size_t)n * m;
    const double* Kk = Kg + (b * (size_t)(N - 1) + k) * (size_t)n * m;
    wsync();   // (the store's reads of Pm are behind us; Bl held KH)
    if (isx) {
      for (int j = 0; j < n; ++j) Mm[T * ldm + j] = Ab[(size_t)j * n + T];
      if (gains) {
        for (int a = 0; a < m; ++a) Bl[a * np + T] = Bb[(size_t)a * n + T];
        for (int a = 0; a < m; ++a) Kl[a * np + T] = Kk[(size_t)T * m + a];
      }
    }
    wsync();
    if (gains) {
      gemm_tn<true>(Mm, ldm, Bl, np, Kl, np, np, np, mq);   // Mm[l][j] += sum_a B[l][a] K[a][j]
      wsync();
    }
    // p' = lx + K' lu + M' p, and KH over Bl
    double acc = lx;
    if (gains) {
      for (int a = 0; a < m; ++a) {
        const double ka = Kl[a * np + Tn];
        acc = __builtin_fma(ka, eval_readlane(lu, a), acc);
        const double kh = eval_readlane(hu, a) * ka;
        if (isx) Bl[a * np + T] = kh;
      }
    }
    for (int l = 0; l < n; ++l) acc = __builtin_fma(Mm[l * ldm + Tn], eval_readlane(pv, l), acc);
    pv = isx ? acc : 0.0;
    gemm_tn<false>(Tt, np, Pm, np, Mm, ldm, np, np, np);   // Tt[j][i] = sum_l P[l][j] M[l][i]
    wsync();
    gemm_tn<false>(Pm, np, Tt, np, Mm, ldm, np, np, np);   // P'[i][j] = sum_l Tt[l][i] M[l][j]
    wsync();
    if (gains) {
      gemm_tn<true>(Pm, np, Bl, np, Kl, np, np, np, mq);   // P'[i][j] += sum_a KH[a][i] K[a][j]
      wsync();
    }
    if (isx) Pm[T * np + T] = Pm[T * np + T] + hx;
    wsync();
    store(k, pv);
  }
  if (T == 0 && io.fb != nullptr) io.fb[b] = valid ? 1 : 0;
}

}  // namespace altro
