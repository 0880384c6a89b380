// sensitivity_data.h -- the reverse-mode sensitivity of the SOLUTION of the last solve with respect to the problem DATA: the cost
// weights, the box bounds and the dynamics (altro_batch_solution_vjp_data(_dev)), and the active set and penalty of the backward
// pass that left the stored gains (altro_batch_get_gain_active_set(_dev); include/altro_batch.h).
// Inside the active set and penalty of the stored pass the problem the solve minimised is an LQ problem with a DIAGONAL Hessian
// hz = w + mu_p [upper side] + mu_p [lower side] (box terms only), and the stored gains are its exact Riccati solution
// (sensitivity.h).  With z = (x, u) the trajectory the handle holds, e = z - zref, and for every row (instance b, seed s):
//   SWEEP 1, backward   sensitivity.h's backward sweep of Lin((gX, gU), 0): s_k, and d_k = -Quu_k^-1 q_u into the workspace
//   SWEEP 2, forward    xi_0 = 0;  nu_k = K_k xi_k + d_k,  xi_{k+1} = A_k xi_k + B_k nu_k;  dz_k = (xi_k, nu_k) into the workspace
//                       when sweep 3 runs; lane-local sums, the lane that owns element j adds up its own:
//                         gQ_j = dt sum_{k < N-1} xi_k[j] e_k[j],   gQf_j = xi_{N-1}[j] e_{N-1}[j],   gR_a = dt sum_k nu_k[a] e_k[n + a]
//                         gzmax_e = -mu_p sum_k [upper side of e in the stored set at k] dz_k[e],  gzmin_e likewise with the lower side
//   SWEEP 3, backward   the costate of the held trajectory (evaluate_al.h's, with the duals and penalty the handle holds) and the
//                       costate of the sensitivity problem, together:
//                         lam_{N-1} = l_x,  lam_k = l_x + A_k' lam_{k+1},   l = w e + g_hi - g_lo   (g = dual + [active] mu c)
//                         dlam_{N-1} = gX_{N-1} + hz xi_{N-1},  dlam_k = gX_k + hz_k xi_k + A_k' dlam_{k+1}
//                         gA_k = lam_{k+1} xi_k' + dlam_{k+1} x_k',  gB_k = lam_{k+1} nu_k' + dlam_{k+1} u_k',  gf_k = dlam_{k+1}
//                       per_knot = 0: the blocks added up over k = N-2 .. 0; per_knot = 1: one block per knot.  Column-major.
// A sweep whose outputs are all null is not run: with gQ, gQf, gR alone the third sweep, the active set and the duals are never
// read.  d_k and dz_k go between the sweeps through a workspace in memory; the lane that stored an element reads it back, so
// there is no fence and no second launch.  (16-lane backend: the padded rows of the last wave run as clones of row 0 and read
// ITS workspace while its owner may still be writing it; they store nothing and their values go nowhere, as in k_sens16.)  The kernels write the caller's outputs and the workspace, nothing the library owns.
// valid = sensitivity.h's rule AND the penalty the instance holds equals the penalty of the stored pass (16-lane backend:
// mu[b] == kmu[b]; one-wave-per-instance backend: mu[b] == words 130-131 of the reuse state): without it every output of the
// instance is a quiet NaN.  No masking, no clamp; a NaN stays a NaN.
// Sweep 1 and the control step of sweep 2 are sensitivity.h's per-knot functions, the ones k_sens16 / k_sens_wide call, with an
// unweighted seed; the local term of sweep 3 restates k_eval_al16 / k_eval_al_wide (evaluate_al.h: 7r measured
// what sharing costs there).
// Contraction is off and every fused multiply-add is written out.  SUMMATION ORDERS of what this file adds (both backends unless
// said; the orders of the two sweeps are stated in sensitivity.h)
//   e                  z - zref, rounded first
//   gQ, gR             acc = +0; acc = fma(dz_k, e_k, acc) for k = 0, 1, .., N - 2 in turn; then dt * acc
//   gQf                xi_{N-1} * e_{N-1}: one product
//   gzmax, gzmin       acc = +0; acc = acc + dz_k for the knots k = 0, 1, .. in turn whose side is in the set; then 0 - mu_p * acc
//                      (the product rounded; an element with no side in the set: +0)
//   hz                 w, + mu_p if the upper side is in the set, + mu_p if the lower side is (the solve kernels' hz_of)
//   local terms        l = (w * e) + (g_hi - g_lo), g = fma(mu, c, dual) on an active side (c >= 0 or dual > 0), else the dual;
//                      dl = fma(hz, dz, gX or gU element) (a null seed array: +0)
//   costates           acc = local term; acc = fma([A B][i][element], costate_i, acc) for i = 0, 1, .., n - 1 in turn
//   gA, gB             per element (i, c):  G = fma(dlam_{k+1}[i], z_k[c], fma(lam_{k+1}[i], dz_k[c], G)),  k = N-2, N-3, .., 0 in turn
//                      from G = +0 (per_knot = 1: every knot from +0)
//   gf                 per_knot = 0: acc = acc + dlam_{k+1}[i], k = N-2 .. 0 in turn from +0
#pragma once
#include "evaluate.h"
#include "policy.h"
#include "sensitivity.h"
#include "solve_wide.h"

namespace altro {

// The arrays of one call (rows R = batch * nseed, row r = b * nseed + s); gX or gU may be null (zero), any output may be null.
struct SensDataIO {
  const double *gX, *gU;                                  // [R][N][n], [R][N-1][m]
  double *gQ, *gQf, *gR, *gzmin, *gzmax, *gA, *gB, *gf;   // include/altro_batch.h: altro_sens_data_out
  double *dws, *zws;            // workspace: d_k [R][N-1][m]; dz_k [R][N][n + m] (null unless sweep 3 runs)
  int* fb;                      // [batch]
  const double *Lb, *mu;        // the box duals and the penalty as the solve kernels keep them (evaluate_al.h)
  const int* bslot;             // 16-lane backend: [16] slot of the lane's element in the compact box rows
  int nbp;
  double dt;
  int per_knot;
};

// g = dL_A / dc of a BOX side of value c with dual l (evaluate_al.h's al_lin without the sum).  The two must keep ONE rule for
// `active` and one form of g: cost_to_go.h takes its g from al_lin, next to this file's hz and validity, and relies on the two
// returning the same bits.
__device__ __forceinline__ double sensd_side(double c, double l, double mu) {
#pragma clang fp contract(off)
  const bool active = !(c < 0.0) || l > 0.0;
  return active ? __builtin_fma(mu, c, l) : l;
}
// the solve kernels' hz_of
__device__ __forceinline__ double sensd_hz(double w, double mu, unsigned bits) {
#pragma clang fp contract(off)
  double hz = w;
  hz = hz + ((bits & 1u) ? mu : 0.0);
  hz = hz + ((bits & 2u) ? mu : 0.0);
  return hz;
}
// 0 - mu * acc, the product rounded
__device__ __forceinline__ double sensd_bound(double mu, double acc) {
#pragma clang fp contract(off)
  const double p = mu * acc;
  return 0.0 - p;
}

// ------------------------------------------------------------------ 16-lane backend
// sensitivity.h's rule AND the penalty the instance holds is the penalty of the stored pass
__device__ __forceinline__ bool sensd16_valid(const double* __restrict__ kmu, const double* __restrict__ mu, size_t b) {
  return sens16_valid(kmu, b) && kmu[b] == mu[b];
}

// One 16-lane row per (instance, seed), four per wave, in the layout of k_sens16: lane j < n holds element j of s / xi / lam /
// dlam, lane n + a element a of q_u / d / nu; lane c < n + m owns column c of [A B] and with it z_k[c], dz_k[c] and the
// accumulators G[i] of column c of gA (c < n) or column c - n of gB.  Zp: the planes the handle holds (simulate.h).  ahash [Bp][16]:
// the lane's two bits per knot (solve_dpp16.h ASet), read only when an output needs the set (the host refuses N > ASET_MAXN).
__global__ void __launch_bounds__(256)
k_sens_data16(SensDataIO io, const double* __restrict__ Zp, const int* __restrict__ cur, size_t plane, const double* __restrict__ KD,
              const double* __restrict__ kmu, const ASet* __restrict__ ahash, Eval16 P, int nseed, size_t R, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N, nz = P.n + P.m;
  const Row16 row = eval16_row(R, rows, (size_t)nseed, n, m);
  if (!row.in) return;   // (whole waves only)
  const size_t r = row.r, b = row.b;
  const int lane = row.lane;
  const bool live = row.live, isx = row.isx, isu = row.isu;
  const double mup = kmu[b];
  const bool valid = sensd16_valid(kmu, io.mu, b);
  const Ctx16 c(P, b, lane);
  const int ua = isu ? lane - n : 0;   // the control a control lane holds
  const bool want_box = io.gzmin != nullptr || io.gzmax != nullptr;
  const bool want3 = io.gA != nullptr || io.gB != nullptr || io.gf != nullptr;
  const double* kdp = KD + b * (size_t)N * m * 16;
  const double* Zn = Zp + b * (2 * (size_t)N + 1) * 16 + (size_t)cur[b] * plane + lane;
  const SensRow g{io.gX != nullptr ? io.gX + r * (size_t)N * n : nullptr, io.gU != nullptr ? io.gU + r * (size_t)(N - 1) * m : nullptr,
                  io.dws + r * (size_t)(N - 1) * m, false, true};
  double* zw = io.zws != nullptr ? io.zws + r * (size_t)N * nz : nullptr;
  const unsigned* aw = (want_box || want3) ? ahash[b * 16 + lane].w : nullptr;
  auto code = [&](int k) -> unsigned { return (aw[k >> 4] >> ((k & 15) * 2)) & 3u; };
  double gt[16];
  sens16_col(P, b, lane, gt);
  // ---- sweep 1
  {
    double s = isx ? sens16_seed(g, c, N - 1, N, n, m) : 0.0;   // s_{k+1} on the state lanes, 0 elsewhere
    for (int k = N - 2; k >= 0; --k) s = sens16_back_knot(g, c, gt, kdp, k, N, n, m, live, s);
  }
  const double nan = sens_nan();
  if (live && lane == 0 && io.fb != nullptr && r == b * (size_t)nseed) io.fb[b] = valid ? 1 : 0;
  // ---- sweep 2, with the lane-local sums
  {
    double gd[16], fv;
    eval16_dyn(P, b, lane, gd, fv);
    double xi = 0.0, sq = 0.0, qf = 0.0, shi = 0.0, slo = 0.0;
    for (int k = 0;; ++k) {
      const bool term = k == N - 1;
      const bool on = isx || (isu && !term);
      const double zl = Zn[(size_t)k * 16], zr = c.Zr[(size_t)k * 16];
      const double z = term ? xi : sens16_control(g, c, kdp, k, n, m, xi);
      const double dz = on ? z : 0.0;   // dz_k of the lane's element
      const double e = on ? zl - zr : 0.0;
      if (term) qf = dz * e;
      else sq = __builtin_fma(dz, e, sq);
      if (want_box && on) {
        const unsigned cd = code(k);
        shi = (cd & 1u) ? shi + dz : shi;
        slo = (cd & 2u) ? slo + dz : slo;
      }
      if (live && on && zw != nullptr) zw[(size_t)k * nz + lane] = dz;
      if (term) break;
      xi = eval16_step(gd, 0.0, z, isx);
    }
    if (live && isx) {
      if (io.gQ != nullptr) io.gQ[r * (size_t)n + lane] = valid ? io.dt * sq : nan;
      if (io.gQf != nullptr) io.gQf[r * (size_t)n + lane] = valid ? qf : nan;
    }
    if (live && isu && io.gR != nullptr) io.gR[r * (size_t)m + ua] = valid ? io.dt * sq : nan;
    if (live && lane < nz) {
      if (io.gzmax != nullptr) io.gzmax[r * (size_t)nz + lane] = valid ? sensd_bound(mup, shi) : nan;
      if (io.gzmin != nullptr) io.gzmin[r * (size_t)nz + lane] = valid ? sensd_bound(mup, slo) : nan;
    }
  }
  if (!want3) return;
  // ---- sweep 3
  const double mu = io.mu[b];
  const int sl = io.bslot[lane];
  const double* Lbr = io.Lb + b * (size_t)(N + 1) * 2 * io.nbp + (sl >= 0 ? sl : 0);
  // the local terms of knot k on the lane's element: l of the held trajectory, dl of the sensitivity problem
  // (both lambdas are called from two places: inlined by force, a call would keep their captures in scratch)
  auto local = [&](int k, double zl, double dz, double& l, double& dl) __attribute__((always_inline)) {
    const bool term = k == N - 1;
    const bool on = isx || (isu && !term);
    const double w = term ? c.wf : c.wd;
    const double e = on ? zl - c.Zr[(size_t)k * 16] : 0.0;
    const double ge = w * e;
    double ghi = 0.0, glo = 0.0;
    if (k >= P.box_k0 && k <= P.box_k1) {
      const BoxSides s = box_sides(on, zl, c.zlo, c.zhi);
      if (s.has_hi) ghi = sensd_side(s.over(), sl >= 0 ? Lbr[(size_t)k * 2 * io.nbp] : 0.0, mu);
      if (s.has_lo) glo = sensd_side(s.under(), sl >= 0 ? Lbr[((size_t)k * 2 + 1) * io.nbp] : 0.0, mu);
    }
    const double cz = ghi - glo;
    const double gl = ge + cz;
    l = on ? gl : 0.0;
    const double hz = sensd_hz(w, mup, on ? code(k) : 0u);
    const double gd = __builtin_fma(hz, dz, sens16_seed(g, c, k, N, n, m));
    dl = on ? gd : 0.0;
  };
  const size_t K1 = io.per_knot ? (size_t)(N - 1) : 1;
  double* gAr = io.gA != nullptr ? io.gA + r * K1 * n * n : nullptr;
  double* gBr = io.gB != nullptr ? io.gB + r * K1 * n * m : nullptr;
  double* gfr = io.gf != nullptr ? io.gf + r * K1 * n : nullptr;
  // the lane's column of the block at hand: column lane of gA (state lanes) or column ua of gB (control lanes)
  auto store_cols = [&](const double (&G)[16], size_t blk) __attribute__((always_inline)) {
    double* col = isx ? (gAr != nullptr ? gAr + blk * n * n + (size_t)lane * n : nullptr)
                      : (isu && gBr != nullptr ? gBr + blk * n * m + (size_t)ua * n : nullptr);
    if (!live || col == nullptr) return;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < n) col[i] = valid ? G[i] : nan;
  };
  double lam, dlam;
  {
    double l, dl;
    local(N - 1, Zn[(size_t)(N - 1) * 16], (lane < nz && isx) ? zw[(size_t)(N - 1) * nz + lane] : 0.0, l, dl);
    lam = isx ? l : 0.0;
    dlam = isx ? dl : 0.0;
  }
  double G[16], gfs = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) G[i] = 0.0;
  for (int k = N - 2; k >= 0; --k) {
    const double zl = lane < nz ? Zn[(size_t)k * 16] : 0.0;
    const double dz = lane < nz ? zw[(size_t)k * nz + lane] : 0.0;   // (the lane's own store of sweep 2)
    sfor<0, 16>([&](auto ii) {
      constexpr int I = decltype(ii)::value;
      const double li = bcast<I>(lam), di = bcast<I>(dlam);
      const double base = io.per_knot ? 0.0 : G[I];
      G[I] = __builtin_fma(di, zl, __builtin_fma(li, dz, base));
    });
    if (io.per_knot) {
      store_cols(G, (size_t)k);
      if (live && isx && gfr != nullptr) gfr[(size_t)k * n + lane] = valid ? dlam : nan;
    } else {
      gfs = gfs + dlam;
    }
    double l, dl;
    local(k, zl, dz, l, dl);
    const double al = row_affine(gt, l, lam), ad = row_affine(gt, dl, dlam);
    lam = isx ? al : 0.0;
    dlam = isx ? ad : 0.0;
  }
  if (!io.per_knot) {
    store_cols(G, 0);
    if (live && isx && gfr != nullptr) gfr[lane] = valid ? gfs : nan;
  }
}

// altro_batch_get_gain_active_set_dev, 16-lane backend: one thread per (instance, knot, element).  codes [B][N][n+m] (null: not
// written), mu_pass [B] (null: not written), fb [B] (null: not written).
__global__ void k_gain_aset16(unsigned char* __restrict__ codes, double* __restrict__ mu_pass, int* __restrict__ fb, const ASet* __restrict__ ahash,
                              const double* __restrict__ kmu, const double* __restrict__ mu, int B, int N, int n, int m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nz = n + m;
  if (t >= (size_t)B * N * nz) return;
  const int e = (int)(t % nz), k = (int)((t / nz) % N);
  const size_t b = t / nz / N;
  const double mup = kmu[b];
  const bool valid = sensd16_valid(kmu, mu, b);
  if (codes != nullptr) {
    const unsigned cd = (ahash[b * 16 + e].w[k >> 4] >> ((k & 15) * 2)) & 3u;
    codes[t] = (unsigned char)((valid && !(k == N - 1 && e >= n)) ? cd : 0u);
  }
  if (e == 0 && k == 0) {
    if (mu_pass != nullptr) mu_pass[b] = valid ? mup : sens_nan();
    if (fb != nullptr) fb[b] = valid ? 1 : 0;
  }
}

// ------------------------------------------------------------------ one-wave-per-instance backend
// sensitivity.h's rule AND the penalty the instance holds is the penalty of the stored pass
__device__ __forceinline__ bool sensdw_valid(const SensWReuse& st, const double* __restrict__ mu, size_t b) { return st.valid() && st.mu_pass() == mu[b]; }

// One wave per (instance, seed) in the layout of k_sens_wide: lane T < n owns element T of s / xi / lam / dlam, x_k[T] and column
// T of gA; lane T < m owns element T of q_u / d / nu, u_k[T] and column T of gB.  Xp, Up: the planes the handle holds
// (simulate.h).  aset [B][3][N][64]: the plane of the last backward pass (bits 0-1 of word 132 of the reuse state), one byte
// per knot and lane: bits 0-1 the sides of x_T, bits 2-3 those of u_T.  The dynamics are read from memory at every knot
// (EvalWDynT without a slice: the wave's LDS goes to the accumulators).  per_knot = 0: the n x (n + m) accumulators of gA, gB live
// in the wave's dynamic LDS, column c at c * (n | 1) (the odd leading dimension keeps the lanes' columns on different banks);
// every lane reads and writes its own columns only, so no fence is needed.  lds = null when they are not needed.
__global__ void __launch_bounds__(256)
k_sens_data_wide(SensDataIO io, const double* __restrict__ Xp, const double* __restrict__ Up, const int* __restrict__ cur,
                 const double* __restrict__ Kg, const double* __restrict__ fac, int fs, const unsigned* __restrict__ bwst,
                 const unsigned char* __restrict__ aset, int reuse_ok, EvalW P, int nseed, size_t R) {
#pragma clang fp contract(off)
  extern __shared__ double sensd_lds[];
  const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int T = (int)(threadIdx.x & 63);
  if (r >= R) return;   // (whole waves)
  const size_t b = r / (size_t)nseed;
  const int n = P.n, m = P.m, N = P.N, nz = P.n + P.m;
  const SensWReuse st(bwst, b, reuse_ok);
  const double mup = st.mu_pass();
  const bool valid = sensdw_valid(st, io.mu, b);
  const unsigned char* ap = aset + ((b * 3 + (size_t)st.plane()) * (size_t)N) * 64 + T;   // the lane's byte of knot 0
  const CtxW c(P, b, T, false);
  const EvalWDynT<true> dyn(P, b, c.kref, T, false);
  const bool isx = c.isx, isu = c.isu;
  const int Tn = c.Tn, Tm = c.Tm;
  const bool want_box = io.gzmin != nullptr || io.gzmax != nullptr;
  const bool want3 = io.gA != nullptr || io.gB != nullptr || io.gf != nullptr;
  const size_t pl = b * 2 + (size_t)cur[b];
  const double* Xn = Xp + pl * (size_t)N * n + Tn;
  const double* Un = Up + pl * (size_t)(N - 1) * m + Tm;
  const double* Kb = Kg + b * (size_t)(N - 1) * n * m;
  const SensRow g{io.gX != nullptr ? io.gX + r * (size_t)N * n : nullptr, io.gU != nullptr ? io.gU + r * (size_t)(N - 1) * m : nullptr,
                  io.dws + r * (size_t)(N - 1) * m, false, true};
  double* zw = io.zws != nullptr ? io.zws + r * (size_t)N * nz : nullptr;
  // ---- sweep 1 (m <= 16)
  {
    double s = sensw_seedx(g, c, N - 1, N, n);
    for (int k = N - 2; k >= 0; --k) {   // (k_sens_wide's knot: the note there says why it is not one function)
      double qu = dyn.tstep(k, true, s, sensw_seedu(g, c, k, m), isu);
      const double qx = dyn.tstep(k, false, s, sensw_seedx(g, c, k, N, n), isx);
      qu = isu ? qu : 0.0;
      const double d = sensw_solve(fac + (b * (size_t)N + k) * fs, c, m, qu);
      if (isu) g.d[(size_t)k * m + T] = d;
      const double acc = evalw_dot(Kb + (size_t)k * n * m + (size_t)Tn * m, 1, qu, m, qx, isx);   // column Tn of K: m consecutive doubles
      s = isx ? acc : 0.0;
    }
  }
  const double nan = sens_nan();
  if (T == 0 && io.fb != nullptr && r == b * (size_t)nseed) io.fb[b] = valid ? 1 : 0;
  // ---- sweep 2, with the lane-local sums
  {
    double xi = 0.0, sqx = 0.0, squ = 0.0, qf = 0.0, sxhi = 0.0, sxlo = 0.0, suhi = 0.0, sulo = 0.0;
    for (int k = 0;; ++k) {
      const bool term = k == N - 1;
      const bool uon = isu && !term;
      const double xl = isx ? Xn[(size_t)k * n] : 0.0;
      const double ul = uon ? Un[(size_t)k * m] : 0.0;
      const double nu = term ? 0.0 : sensw_control(g, c, Kb, k, n, m, xi);
      const double ex = isx ? xl - c.Xf[(size_t)k * n + Tn] : 0.0;
      const double eu = uon ? ul - c.Uf[(size_t)k * m + Tm] : 0.0;
      if (term) {
        qf = xi * ex;
      } else {
        sqx = __builtin_fma(xi, ex, sqx);
        squ = __builtin_fma(nu, eu, squ);
      }
      if (want_box) {
        const unsigned cd = ap[(size_t)k * 64];
        if (isx) {
          sxhi = (cd & 1u) ? sxhi + xi : sxhi;
          sxlo = (cd & 2u) ? sxlo + xi : sxlo;
        }
        if (uon) {
          suhi = (cd & 4u) ? suhi + nu : suhi;
          sulo = (cd & 8u) ? sulo + nu : sulo;
        }
      }
      if (zw != nullptr) {
        if (isx) zw[(size_t)k * nz + T] = xi;
        if (uon) zw[(size_t)k * nz + n + T] = nu;
      }
      if (term) break;
      const double nx = sensw_step(dyn, k, xi, nu);
      xi = isx ? nx : 0.0;
    }
    if (isx) {
      if (io.gQ != nullptr) io.gQ[r * (size_t)n + T] = valid ? io.dt * sqx : nan;
      if (io.gQf != nullptr) io.gQf[r * (size_t)n + T] = valid ? qf : nan;
      if (io.gzmax != nullptr) io.gzmax[r * (size_t)nz + T] = valid ? sensd_bound(mup, sxhi) : nan;
      if (io.gzmin != nullptr) io.gzmin[r * (size_t)nz + T] = valid ? sensd_bound(mup, sxlo) : nan;
    }
    if (isu) {
      if (io.gR != nullptr) io.gR[r * (size_t)m + T] = valid ? io.dt * squ : nan;
      if (io.gzmax != nullptr) io.gzmax[r * (size_t)nz + n + T] = valid ? sensd_bound(mup, suhi) : nan;
      if (io.gzmin != nullptr) io.gzmin[r * (size_t)nz + n + T] = valid ? sensd_bound(mup, sulo) : nan;
    }
  }
  if (!want3) return;
  // ---- sweep 3
  const double mu = io.mu[b];
  const double* Lbx = io.Lb + b * (size_t)N * 2 * nz + Tn;
  const double* Lbu = io.Lb + b * (size_t)N * 2 * nz + n + Tm;
  // the local terms of knot k on the lane's state element: l of the held trajectory, dl of the sensitivity problem
  auto local = [&](int k, double xl, double dxi, double& lx, double& dlx) __attribute__((always_inline)) {
    const bool term = k == N - 1;
    const unsigned cd = ap[(size_t)k * 64];
    double xhi = 0.0, xlo = 0.0;
    if (k >= P.box_k0 && k <= P.box_k1) {
      const BoxSides sx = box_sides(isx, xl, c.xlo, c.xhi);
      if (sx.has_hi) xhi = sensd_side(sx.over(), Lbx[(size_t)k * 2 * nz], mu);
      if (sx.has_lo) xlo = sensd_side(sx.under(), Lbx[((size_t)k * 2 + 1) * nz], mu);
    }
    const double wx = term ? c.wfx : c.wx;
    const double ex = isx ? xl - c.Xf[(size_t)k * n + Tn] : 0.0;
    const double ge = wx * ex;
    const double cx = xhi - xlo;
    const double gl = ge + cx;
    lx = isx ? gl : 0.0;
    const double hz = sensd_hz(wx, mup, isx ? (cd & 3u) : 0u);
    const double gd = __builtin_fma(hz, dxi, sensw_seedx(g, c, k, N, n));
    dlx = isx ? gd : 0.0;
  };
  const size_t K1 = io.per_knot ? (size_t)(N - 1) : 1;
  double* gAr = io.gA != nullptr ? io.gA + r * K1 * n * n : nullptr;
  double* gBr = io.gB != nullptr ? io.gB + r * K1 * n * m : nullptr;
  double* gfr = io.gf != nullptr ? io.gf + r * K1 * n : nullptr;
  const int ldp = n | 1;
  double* accA = io.per_knot ? nullptr : sensd_lds + (size_t)(threadIdx.x >> 6) * ldp * nz + (size_t)Tn * ldp;
  double* accB = io.per_knot ? nullptr : sensd_lds + (size_t)(threadIdx.x >> 6) * ldp * nz + (size_t)(n + Tm) * ldp;
  const bool doA = isx && gAr != nullptr, doB = isu && gBr != nullptr;
  if (!io.per_knot) {
    for (int i = 0; i < n; ++i) {
      if (doA) accA[i] = 0.0;
      if (doB) accB[i] = 0.0;
    }
  }
  double lam, dlam, gfs = 0.0;
  local(N - 1, isx ? Xn[(size_t)(N - 1) * n] : 0.0, isx ? zw[(size_t)(N - 1) * nz + T] : 0.0, lam, dlam);
  for (int k = N - 2; k >= 0; --k) {
    const double xl = isx ? Xn[(size_t)k * n] : 0.0, ul = isu ? Un[(size_t)k * m] : 0.0;
    const double dxi = isx ? zw[(size_t)k * nz + T] : 0.0, dnu = isu ? zw[(size_t)k * nz + n + T] : 0.0;   // (the lane's own stores)
    double* cA = doA && io.per_knot ? gAr + (size_t)k * n * n + (size_t)T * n : nullptr;
    double* cB = doB && io.per_knot ? gBr + (size_t)k * n * m + (size_t)T * n : nullptr;
    for (int i = 0; i < n; ++i) {
      const double li = eval_readlane(lam, i), di = eval_readlane(dlam, i);
      if (doA) {
        const double v = __builtin_fma(di, xl, __builtin_fma(li, dxi, io.per_knot ? 0.0 : accA[i]));
        if (io.per_knot) cA[i] = valid ? v : nan;
        else accA[i] = v;
      }
      if (doB) {
        const double v = __builtin_fma(di, ul, __builtin_fma(li, dnu, io.per_knot ? 0.0 : accB[i]));
        if (io.per_knot) cB[i] = valid ? v : nan;
        else accB[i] = v;
      }
    }
    if (io.per_knot) {
      if (isx && gfr != nullptr) gfr[(size_t)k * n + T] = valid ? dlam : nan;
    } else {
      gfs = gfs + dlam;
    }
    double lx, dlx;
    local(k, xl, dxi, lx, dlx);
    const double al = dyn.tstep(k, false, lam, lx, isx), ad = dyn.tstep(k, false, dlam, dlx, isx);
    lam = isx ? al : 0.0;
    dlam = isx ? ad : 0.0;
  }
  if (!io.per_knot) {
    for (int i = 0; i < n; ++i) {
      if (doA) gAr[(size_t)T * n + i] = valid ? accA[i] : nan;
      if (doB) gBr[(size_t)T * n + i] = valid ? accB[i] : nan;
    }
    if (isx && gfr != nullptr) gfr[T] = valid ? gfs : nan;
  }
}

// altro_batch_get_gain_active_set_dev, one-wave-per-instance backend: one thread per (instance, knot, element)
__global__ void k_gain_aset_wide(unsigned char* __restrict__ codes, double* __restrict__ mu_pass, int* __restrict__ fb,
                                 const unsigned char* __restrict__ aset, const unsigned* __restrict__ bwst, int reuse_ok,
                                 const double* __restrict__ mu, int B, int N, int n, int m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nz = n + m;
  if (t >= (size_t)B * N * nz) return;
  const int e = (int)(t % nz), k = (int)((t / nz) % N);
  const size_t b = t / nz / N;
  const SensWReuse st(bwst, b, reuse_ok);
  const double mup = st.mu_pass();
  const bool valid = sensdw_valid(st, mu, b);
  if (codes != nullptr) {
    const unsigned byte = aset[((b * 3 + (size_t)st.plane()) * (size_t)N + k) * 64 + (e < n ? e : e - n)];
    const unsigned cd = e < n ? (byte & 3u) : ((byte >> 2) & 3u);
    codes[t] = (unsigned char)((valid && !(k == N - 1 && e >= n)) ? cd : 0u);
  }
  if (e == 0 && k == 0) {
    if (mu_pass != nullptr) mu_pass[b] = valid ? mup : sens_nan();
    if (fb != nullptr) fb[b] = valid ? 1 : 0;
  }
}

}  // namespace altro
