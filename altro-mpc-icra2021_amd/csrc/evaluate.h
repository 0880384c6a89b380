// evaluate.h -- caller-supplied trajectories scored on the device (altro_batch_evaluate(_dev); include/altro_batch.h,
// DESIGN.md 7h): rollout x_{k+1} = A_k x_k + B_k u_k + f_k, the plain tracking cost J, the maximum constraint violation c_max
// and the dynamics defect, against the problem the next solve would see at that point of the stream.
// Two kernels per backend.  The ROLLOUT kernel writes the states to memory ([rows][N][n], rows = batch * ncand, the caller's
// layout); the SCORING kernel reads states and controls from memory in every form, so a rollout followed by a scoring of what
// it wrote gives the bytes a direct scoring of the same arrays gives.  The kernels read the tables the solve kernels read --
// dynamics, cost rows, bounds rows, reference window, constraint rows -- and write nothing the library owns.  No
// synchronisation between waves; LDS only as a wave-private copy of time-invariant dynamics on the one-wave-per-instance backend.
// THE SCORING CORE.  This file also holds, once per backend, what every kernel that scores a trajectory is
// made of -- the kernels here and those of warm_start.h, simulate.h and evaluate_grad.h: the context of a row / wave (Ctx16,
// CtxW), the value of a constraint row (con16_row, conw_row) with what the maximum (con16_max, conw_max) and the penalty
// (con16_residual, conw_residual) make of it, the two sides of a box (box_sides), the per-knot cost (cost16_knot, costw_knot)
// and score (score16_knot, scorew_knot: cost, box test, constraint rows), its reduction (score_reduce), the dynamics of a wave
// forwards and transposed (EvalWDyn) and the step of the recurrence (eval16_step, evalw_advance).  Contraction is off in every
// function that holds a product followed by a sum and each fused multiply-add is written out, so the order of every sum is
// the one stated here (evaluate_grad.h adds those of its reverse sweep):
//   dynamics / constraint row   acc = f_i (b_r); acc = fma(coefficient_j, z_j, acc) for j = 0, 1, ..., n + m - 1 in turn
//   cost                        every lane adds its own w e^2 (product e * e rounded, then w * (e e), then the addition) knot
//                               after knot, k = 0 .. N-1; the lanes are then added by an xor butterfly (strides 8, 4, 2, 1, and
//                               32, 16 first on the one-wave-per-instance backend); J = 0.5 * that sum
//   SOC residual                n2 = v_0^2 + v_1^2 + .. in turn (products rounded), nv = sqrt(n2), c = 0.5 * (1 + t / nv);
//                               element q < p - 1: v_q - c * v_q; element p - 1: t - c * nv; the violation is its fabs
//   c_max, defect               maxima (exact in any order); a NaN stays a NaN
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "solve_dpp16.h"

namespace altro {

// max that keeps a NaN once it has seen one (fmax would drop it: an overflowed rollout must not look feasible)
__device__ __forceinline__ double eval_max(double acc, double v) { return (v > acc || v != v) ? v : acc; }

// sum / eval_max over the W lanes of a row (W = 16) or wave (W = 64): xor butterfly, strides W/2 .. 1, every lane ends with it
template <int W>
__device__ __forceinline__ double lanes_sum(double v) {
  for (int s = W / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, W);
  return v;
}
template <int W>
__device__ __forceinline__ double lanes_max(double v) {
  for (int s = W / 2; s > 0; s >>= 1) v = eval_max(v, __shfl_xor(v, s, W));
  return v;
}

// one element's term of the tracking cost: w (z - zref)^2, each product rounded
__device__ __forceinline__ double cost_term(double w, double z, double zref) {
#pragma clang fp contract(off)
  const double d = z - zref;
  double q = d * d;
  q = w * q;
  return q;
}

// max(0, v) that keeps a NaN
__device__ __forceinline__ double grad_pos(double v) { return (v > 0.0 || v != v) ? v : 0.0; }

// the two sides of one element's box: whether the side is there (the solve kernels' test for a finite side; on = the lane
// holds the element) and the signed distances over() = z - hi, under() = lo - z.  box_max takes their maxima, the penalty
// max(0, .) of them.  (The distances are formed where they are used: formed ahead, box_max's second subtraction moved up in
// the knot loop of k_ws_score_wide and cost that kernel 2 %)
struct BoxSides {
  bool has_hi, has_lo;
  double z, lo, hi;
  __device__ __forceinline__ double over() const { return z - hi; }
  __device__ __forceinline__ double under() const { return lo - z; }
  __device__ __forceinline__ double res_hi() const { return has_hi ? grad_pos(over()) : 0.0; }
  __device__ __forceinline__ double res_lo() const { return has_lo ? grad_pos(under()) : 0.0; }
};
__device__ __forceinline__ BoxSides box_sides(bool on, double z, double lo, double hi) { return {on && hi < 1e300, on && lo > -1e300, z, lo, hi}; }
__device__ __forceinline__ double box_max(double viol, bool on, double z, double lo, double hi) {
  const BoxSides s = box_sides(on, z, lo, hi);
  if (s.has_hi) viol = eval_max(viol, s.over());
  if (s.has_lo) viol = eval_max(viol, s.under());
  return viol;
}

// v - Proj(v) of element `pos` of a second-order cone of dimension p (2..4) whose values are v[0..p-1] (v[q] = 0 for
// q >= p): the oracle's soc_project.  Inside the cone 0, in the polar cone v_pos, otherwise the step from the boundary point
// c (s, |s|), c = (1 + t / |s|) / 2.  The violation (the oracle's con_violation) is its magnitude, exactly.
__device__ __forceinline__ double soc_row_residual(const double (&v)[4], int p, int pos) {
#pragma clang fp contract(off)
  const int pt = p - 1;
  double n2 = 0.0, t = 0.0, mine = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    n2 = q < pt ? n2 + v[q] * v[q] : n2;
    t = q == pt ? v[q] : t;
    mine = q == pos ? v[q] : mine;
  }
  const double nv = sqrt(n2);
  if (nv <= t) return 0.0;
  if (nv <= -t) return mine;
  const double c = 0.5 * (1.0 + t / nv);
  const double proj = pos == pt ? c * nv : c * mine;
  return mine - proj;   // (a NaN anywhere in the cone fails both tests above and comes out here)
}
__device__ __forceinline__ double soc_row_violation(const double (&v)[4], int p, int pos) { return fabs(soc_row_residual(v, p, pos)); }

// What a lane has of the constraint row it owns at a knot (con16_row, conw_row): the row's value v, whether the row is on (a
// lane without an active row: v is 0 or unused), its kind, and for a cone its dimension p, the row's place pos in it and the
// cone's values vq (0 beyond p).  The maximum takes |Proj - v| / |v| / v of it, the penalty the signed residual.
struct ConRow {
  double v, vq[4];
  int p, pos;
  bool on, soc, eq;
};
__device__ __forceinline__ double row_violation(const ConRow& r) {
  return r.soc ? soc_row_violation(r.vq, r.p, r.pos) : (r.eq ? fabs(r.v) : r.v);
}
__device__ __forceinline__ double row_residual(const ConRow& r) {
  const double res = r.soc ? soc_row_residual(r.vq, r.p, r.pos) : (r.eq ? r.v : grad_pos(r.v));
  return r.on ? res : 0.0;
}

// what a scoring kernel accumulates knot after knot, per lane, and what its row / wave has in the end
struct Score {
  double cost = 0.0, viol = 0.0;
};
template <int W>
__device__ __forceinline__ void score_reduce(const Score& s, double& J, double& cmax) {
  J = 0.5 * lanes_sum<W>(s.cost);
  cmax = lanes_max<W>(s.viol);
}

__device__ __forceinline__ int eval_window(const int* window, int kref, size_t b, int N, int Nt) {
  int w = window != nullptr ? window[b] : kref;
  w = w + N > Nt ? Nt - N : w;   // (the host and the tick rule keep every window inside the track: this never moves one)
  return w < 0 ? 0 : w;
}

// ------------------------------------------------------------------ 16-lane backend (SolveParams layout)
// One 16-lane row per (instance, candidate), four per wave.  rows = batch * ncand padded to whole waves; rows >= R compute on
// row 0 and store nothing, so EXEC is all ones wherever a DPP move reads another lane.  Lane j < n holds x_j, lane n + a holds
// u_a (0 at the terminal knot), lanes >= n + m hold 0.
struct Eval16 {
  const double *Grow, *fvec;              // [Bp][16][16] Grow[b][c][i] = [A B][i][c]; [Bp][16]
  const double *wd, *wf, *zmin, *zmax;    // element (b * 16 + lane) & imask
  const double* Zref;                     // [Bp][Nt][16]
  const double *Acon, *bcon;              // [N][16][16] row-major, [N][16]; + b * con_istride, b * con_istride / 16
  const int* cmeta;                       // [N][16][4]: type, k0, k1, p
  const int* window;                      // [Bp] per-instance reference window (episode clock), or null: kref
  unsigned imask;
  size_t con_istride;
  int ncrows, N, Nt, n, m, kref, box_k0, box_k1;
};

// The row a thread works on: r = the row it computes (0 for a padded row, which stores nothing: `live`), b = r / per its
// instance, `in` = false beyond the padded rows (whole waves: such a thread leaves at once).
struct Row16 {
  size_t r, b;
  int lane;
  bool live, in, isx, isu;
};
__device__ __forceinline__ Row16 eval16_row(size_t R, size_t rows, size_t per, int n, int m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t row = t / 16;
  const int lane = (int)(t % 16);
  const bool live = row < R;
  const size_t r = live ? row : 0;
  return {r, r / per, lane, live, row < rows, lane < n, lane >= n && lane < n + m};
}

// acc + sum_c g[c] * z_c over the 16 lanes of the row, c = 0 .. 15 in turn; g[c] is 0 for c >= n + m, where z_c is 0 too
__device__ __forceinline__ double row_affine(const double (&g)[16], double acc, double z) {
  sfor<0, 16>([&](auto c) {
    constexpr int C = decltype(c)::value;
    acc = __builtin_fma(g[C], bcast<C>(z), acc);
  });
  return acc;
}

// lane i's column of [A B | f] of instance b: g[c] = [A B][i][c]
__device__ __forceinline__ void eval16_dyn(const Eval16& P, size_t b, int lane, double (&g)[16], double& fv) {
  const int nz = P.n + P.m;
  const double* G = P.Grow + b * 256 + lane;
#pragma unroll
  for (int c = 0; c < 16; ++c) g[c] = (c < nz && lane < P.n) ? G[c * 16] : 0.0;
  fv = lane < P.n ? P.fvec[b * 16 + lane] : 0.0;
}

// the step of the recurrence: the row's z = [x; u; 0] -> x_{k+1} on the state lanes, 0 elsewhere
__device__ __forceinline__ double eval16_step(const double (&g)[16], double fv, double z, bool isx) {
  const double nx = row_affine(g, fv, z);
  return isx ? nx : 0.0;
}

// what a lane of a row of instance b keeps over the knots to score them
struct Ctx16 {
  int lane, pos;
  bool isx, isu;
  double wd, wf, zlo, zhi;
  const double *Zr, *Ac, *bc;   // the lane's element of the reference row / constraint row / constraint offset of knot 0
  __device__ __forceinline__ Ctx16(const Eval16& P, size_t b, int lane_) : lane(lane_), pos(lane_ & 3) {
    isx = lane < P.n;
    isu = lane >= P.n && lane < P.n + P.m;
    const int kref = eval_window(P.window, P.kref, b, P.N, P.Nt);
    const unsigned e = ((unsigned)b * 16u + (unsigned)lane) & P.imask;
    wd = P.wd[e]; wf = P.wf[e]; zlo = P.zmin[e]; zhi = P.zmax[e];
    Zr = P.Zref + (b * (size_t)P.Nt + (size_t)kref) * 16 + lane;
    Ac = P.Acon + b * P.con_istride + (size_t)lane * 16;
    bc = P.bcon + b * (P.con_istride / 16) + lane;
  }
};

// the constraint row of knot k that lane r owns: row r of the knot's table (c.Ac, c.bc: the lane's row and offset of knot 0).
// Every lane of the row is here (the broadcasts read live lanes); P.ncrows > 0.
__device__ __forceinline__ ConRow con16_row(const Eval16& P, const Ctx16& c, int k, double z) {
  const int n = P.n, m = P.m;
  const int* cm = P.cmeta + ((size_t)k * 16 + c.lane) * 4;
  const int type = cm[0], p = cm[3];
  const bool act = type != CT_NONE && k >= cm[1] && k <= cm[2];
  double a[16], v = 0.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) a[j] = 0.0;
  if (act) {
    const double* ar = c.Ac + (size_t)k * 256;
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = j < n + m ? ar[j] : 0.0;
    v = c.bc[(size_t)k * 16];
  }
  ConRow r;
  r.v = row_affine(a, v, z);
  r.p = p; r.pos = c.pos; r.soc = type == CT_SOC; r.eq = type == CT_EQ;
  r.on = act && (!r.soc || c.pos < p);   // (a linear row may sit in a spare lane of a cone's quad)
  const double vv = (r.on && r.soc) ? r.v : 0.0;
  r.vq[0] = quad_bcast<0>(vv); r.vq[1] = quad_bcast<1>(vv); r.vq[2] = quad_bcast<2>(vv); r.vq[3] = quad_bcast<3>(vv);
  return r;
}
// the running maximum with the knot's rows (in and out by value), and the lane's signed residual (0 without an active row)
__device__ __forceinline__ double con16_max(double viol, const Eval16& P, const Ctx16& c, int k, double z) {
  if (P.ncrows > 0) {
    const ConRow r = con16_row(P, c, k, z);
    if (r.on) viol = eval_max(viol, row_violation(r));
  }
  return viol;
}
__device__ __forceinline__ double con16_residual(const Eval16& P, const Ctx16& c, int k, double z) { return row_residual(con16_row(P, c, k, z)); }

// the cost of knot k of the row added to the lane's sum: z = the lane's element (0 where the row holds none), zr = the lane's
// element of the knot's reference row (an argument: k_sim16 loads it a knot ahead)
__device__ __forceinline__ double cost16_knot(double cost, const Eval16& P, const Ctx16& c, int k, double z, double zr) {
  const bool term = k == P.N - 1;
  const bool on = c.isx | (c.isu & !term);
  const double q = cost_term(term ? c.wf : c.wd, z, zr);
  return on ? cost + q : cost;
}

// knot k of the row: cost, box, constraint rows
__device__ __forceinline__ void score16_knot(Score& s, const Eval16& P, const Ctx16& c, int k, double z, double zr) {
  const bool on = c.isx | (c.isu & (k != P.N - 1));
  s.cost = cost16_knot(s.cost, P, c, k, z, zr);
  if (on && k >= P.box_k0 && k <= P.box_k1) s.viol = box_max(s.viol, true, z, c.zlo, c.zhi);
  s.viol = con16_max(s.viol, P, c, k, z);
}

// Rollout: Xw [R][N][n] <- x_0 = x0[b] (x0s = its row stride: n for a caller's array, 16 for the handle's own), then the
// recursion under U [R][N-1][m].
__global__ void k_eval_rollout16(double* __restrict__ Xw, const double* __restrict__ U, const double* __restrict__ x0, int x0s, Eval16 P,
                                 int ncand, size_t R, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const auto [r, b, lane, live, in, isx, isu] = eval16_row(R, rows, (size_t)ncand, n, m);
  if (!in) return;
  double g[16], fv;
  eval16_dyn(P, b, lane, g, fv);
  double* Xr = Xw + r * (size_t)N * n;
  const double* Ur = U + r * (size_t)(N - 1) * m;
  double x = isx ? x0[b * (size_t)x0s + lane] : 0.0;
  for (int k = 0;; ++k) {
    if (live && isx) Xr[(size_t)k * n + lane] = x;
    if (k == N - 1) break;
    const double z = isx ? x : (isu ? Ur[(size_t)k * m + (lane - n)] : 0.0);
    x = eval16_step(g, fv, z, isx);
  }
}

// Scoring of (X [R][N][n], U [R][N-1][m]); J, cmax, defect [R], any may be null.  given = 0: defect <- +0 (the rollout form).
__global__ void k_eval_score16(double* __restrict__ J, double* __restrict__ cmax, double* __restrict__ defect, const double* __restrict__ X,
                               const double* __restrict__ U, Eval16 P, int ncand, size_t R, size_t rows, int given) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const auto [r, b, lane, live, in, isx, isu] = eval16_row(R, rows, (size_t)ncand, n, m);
  if (!in) return;
  const bool want_defect = defect != nullptr && given != 0;
  const Ctx16 c(P, b, lane);
  double g[16], fv = 0.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) g[j] = 0.0;
  if (want_defect) eval16_dyn(P, b, lane, g, fv);
  const double* Xr = X + r * (size_t)N * n;
  const double* Ur = U + r * (size_t)(N - 1) * m;
  // score16_knot's terms with the defect between the box and the constraint rows, where it always stood
  Score s;
  double dfc = 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const bool on = isx | (isu & !term);   // (cost16_knot's form of it: the two are then one value to the compiler)
    const double z = isx ? Xr[(size_t)k * n + lane] : (on ? Ur[(size_t)k * m + (lane - n)] : 0.0);
    s.cost = cost16_knot(s.cost, P, c, k, z, c.Zr[(size_t)k * 16]);
    if (on && k >= P.box_k0 && k <= P.box_k1) s.viol = box_max(s.viol, true, z, c.zlo, c.zhi);
    if (want_defect && !term) {
      const double pred = row_affine(g, fv, z);
      if (isx) dfc = eval_max(dfc, fabs(pred - Xr[(size_t)(k + 1) * n + lane]));
    }
    s.viol = con16_max(s.viol, P, c, k, z);
  }
  double Jr, cr;
  score_reduce<16>(s, Jr, cr);
  dfc = lanes_max<16>(dfc);
  if (!live || lane != 0) return;
  if (J != nullptr) J[r] = Jr;
  if (cmax != nullptr) cmax[r] = cr;
  if (defect != nullptr) defect[r] = dfc;   // (+0 in the rollout form)
}

// ------------------------------------------------------------------ one-wave-per-instance backend (wide::Params layout)
// One wave per (instance, candidate).  Lane T < n owns x_T, lane T < m owns u_T, lane T < Pn owns constraint row T.  A, Bm
// are column-major and AconT has the rows of a knot's table as columns, so the loads of one term of a sum are consecutive
// addresses over the lanes; x_j / u_j come from lane j by v_readlane (j is uniform).
struct EvalW {
  const double *A, *Bm, *f;               // column-major blocks, block arithmetic of solve_wide.h dynblk()
  const double *wd, *wf, *zmin, *zmax;    // rows b * w_pi resp. b * b_pi
  const double *Xref, *Uref;              // [B][Nt][n], [B][Nt-1][m]
  const double *AconT, *bcon;             // [N][n+m][Pn], [N][Pn]; + b * con_istride, b * bcon_istride
  const int *ctype, *rowc0, *rowcp;       // [N][Pn], [Pn], [Pn]
  const int* window;
  size_t con_istride, bcon_istride;
  int w_pi, b_pi, ltv, dyn_pi, dyn_blocks, dyn_stride, Pn, N, Nt, n, m, kref, box_k0, box_k1;
  int lds_dyn;   // 1: time-invariant dynamics whose [A | B] block fits: every wave keeps its instance's block in its slice of LDS
};

// The leading dimension ld of a wave's LDS copy of [A | B] (n, or n | 1 for a kernel that also reads it transposed: EvalWDyn),
// the LDS doubles a wave needs for it, the bytes a 256-thread block of four waves asks for, and the rule for it: inside the
// 64 KB a kernel gets without asking for more (ld (n + m) <= 2048: up to (32, 32), (40, 11), ...; padded (32, 16), (30, 25)).
// Larger blocks are read from memory at every knot.
__host__ __device__ inline int evalw_ld(int n, bool pad) { return pad ? n | 1 : n; }
__host__ __device__ inline size_t evalw_lds_doubles(int ld, int n, int m) { return (size_t)ld * (n + m); }
__host__ __device__ inline size_t evalw_lds_bytes(int ld, int n, int m) { return 4 * evalw_lds_doubles(ld, n, m) * sizeof(double); }
__host__ __device__ inline bool evalw_lds_fits(int ld, int n, int m, int ltv) { return !ltv && evalw_lds_bytes(ld, n, m) <= 65536; }

__device__ __forceinline__ double eval_readlane(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ size_t evalw_block(const EvalW& P, size_t b, int kref, int k) {
  size_t kb = 0;
  if (P.ltv) {
    kb = (size_t)kref * P.dyn_stride + k;
    kb = kb < (size_t)P.dyn_blocks ? kb : (size_t)P.dyn_blocks - 1;   // (never taken: the host checks that the window's blocks exist)
  }
  return (P.dyn_pi ? b : 0) * (size_t)(P.ltv ? P.dyn_blocks : 1) + kb;
}

// acc + sum_j col[j * stride] * v_j, j = 0 .. cnt-1 in turn, v_j = lane j's v.  The loads go out eight at a time (a plain
// accumulate loop would wait a memory round trip per term); `on` = false: the lane owns no row, its coefficients are 0.
__device__ __forceinline__ double evalw_dot(const double* col, size_t stride, double v, int cnt, double acc, bool on) {
  for (int j0 = 0; j0 < cnt; j0 += 8) {
    double a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = on ? col[(size_t)(j0 + u < cnt ? j0 + u : cnt - 1) * stride] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (j0 + u < cnt) acc = __builtin_fma(a[u], eval_readlane(v, j0 + u), acc);
  }
  return acc;
}

// row Tn of A x + B u + f0: Acol / Bcol point at element Tn of the first column, the next column is ld doubles on; xs / us
// are the lane's own elements
__device__ __forceinline__ double evalw_step(const double* Acol, const double* Bcol, int ld, double f0, int n, int m, double xs, double us) {
  const double acc = evalw_dot(Acol, (size_t)ld, xs, n, f0, true);
  return evalw_dot(Bcol, (size_t)ld, us, m, acc, true);
}

// The dynamics of instance b as one wave reads them at knot k, forwards (step: row T of [A | B]) and transposed (tstep: column
// T).  Time-invariant blocks that fit are copied once into the wave's own slice of LDS -- every knot of every candidate would
// otherwise read the same n (n + m) doubles from memory again, and at (32, 16), batch 8192, ncand 8 that traffic (12 KB per
// knot and wave) was the whole run time.  The slice is written and read by the same wave only: LDS instructions of a wave
// execute in order, so the hand-over needs a wave-level fence for the compiler and no barrier.  The values and the order of
// every sum are the same either way.  PAD: the kernel also reads the slice transposed, so its leading dimension is padded to
// an odd number of doubles: lane j's transposed run starts at j * ld, and a ds_read_b64 of 32 lanes is conflict-free exactly
// when j * ld mod 32 takes 32 values (MI355X: 64 banks of 4 bytes, a double takes two).  The forward reads
// (element T + j * ld, j uniform) are consecutive either way.
template <bool PAD>
struct EvalWDynT {
  const EvalW& P;
  size_t b;
  int kref, Tn, Tm;
  const double* lds;   // the wave's [A | B] in LDS, or null
  double f0;
  // T: the lane; `copy` = false: no slice (the kernel will not step, or the block does not fit: the launch decides)
  __device__ __forceinline__ EvalWDynT(const EvalW& p, size_t b_, int kref_, int T, bool copy)
      : P(p), b(b_), kref(kref_), Tn(T < p.n ? T : p.n - 1), Tm(T < p.m ? T : p.m - 1), lds(nullptr), f0(0.0) {
    if (!copy) return;
    extern __shared__ double eval_lds[];
    const int n = P.n, na = P.n * P.n, nb = P.n * P.m, ld = evalw_ld(P.n, PAD);
    double* slice = eval_lds + (threadIdx.x >> 6) * evalw_lds_doubles(ld, P.n, P.m);
    const size_t blk = evalw_block(P, b, kref, 0);
    auto at = [&](int e) { return PAD ? (e / n) * ld + e % n : e; };   // element e of the column-major [A | B]
    for (int e = T; e < na; e += 64) slice[at(e)] = P.A[blk * na + e];
    for (int e = T; e < nb; e += 64) slice[at(na + e)] = P.Bm[blk * nb + e];
    f0 = P.f != nullptr ? P.f[blk * P.n + Tn] : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    lds = slice;
  }
  __device__ __forceinline__ double step(int k, double xs, double us) const {
    const int n = P.n, m = P.m, ld = evalw_ld(P.n, PAD);
    if (lds != nullptr) return evalw_step(lds + Tn, lds + n * ld + Tn, ld, f0, n, m, xs, us);
    const size_t blk = evalw_block(P, b, kref, k);
    return evalw_step(P.A + blk * n * n + Tn, P.Bm + blk * n * m + Tn, n, P.f != nullptr ? P.f[blk * n + Tn] : 0.0, n, m, xs, us);
  }
  // acc + column Tn of A_k (bt: column Tm of B_k) times lambda, i = 0 .. n-1 in turn
  __device__ __forceinline__ double tstep(int k, bool bt, double lam, double acc, bool on) const {
    const int n = P.n, m = P.m;
    if (lds != nullptr) return evalw_dot(lds + (size_t)(bt ? n + Tm : Tn) * evalw_ld(n, PAD), 1, lam, n, acc, on);
    const size_t blk = evalw_block(P, b, kref, k);
    const double* col = bt ? P.Bm + blk * n * m + (size_t)Tm * n : P.A + blk * n * n + (size_t)Tn * n;
    return evalw_dot(col, 1, lam, n, acc, on);
  }
};
using EvalWDyn = EvalWDynT<false>;

// the step of the recurrence: (x, u) of knot k -> x_{k+1} on the state lanes, 0 elsewhere
template <bool PAD>
__device__ __forceinline__ double evalw_advance(const EvalWDynT<PAD>& dyn, int k, double x, double u, bool isx) {
  const double nx = dyn.step(k, x, u);
  return isx ? nx : 0.0;
}

// what lane T of a wave of instance b keeps over the knots to score and to step them (members in the order their loads go out)
struct CtxW {
  int T;
  bool isx, isu, isr;
  int Tn, Tm, kref;
  double wx, wfx, wu, xlo, xhi, ulo, uhi;
  const double *Xf, *Uf, *At, *bc;   // reference rows of knot 0; the lane's constraint row / offset of knot 0
  int c0, cp;
  EvalWDyn dyn;
  __device__ __forceinline__ CtxW(const EvalW& P, size_t b, int T_, bool want_dyn)
      : T(T_), isx(T_ < P.n), isu(T_ < P.m), isr(T_ < P.Pn), Tn(isx ? T_ : P.n - 1), Tm(isu ? T_ : P.m - 1),
        kref(eval_window(P.window, P.kref, b, P.N, P.Nt)),
        wx(P.wd[b * (size_t)P.w_pi * (P.n + P.m) + Tn]), wfx(P.wf[b * (size_t)P.w_pi * P.n + Tn]),
        wu(P.wd[b * (size_t)P.w_pi * (P.n + P.m) + P.n + Tm]),
        xlo(P.zmin[b * (size_t)P.b_pi * (P.n + P.m) + Tn]), xhi(P.zmax[b * (size_t)P.b_pi * (P.n + P.m) + Tn]),
        ulo(P.zmin[b * (size_t)P.b_pi * (P.n + P.m) + P.n + Tm]), uhi(P.zmax[b * (size_t)P.b_pi * (P.n + P.m) + P.n + Tm]),
        Xf(P.Xref + (b * (size_t)P.Nt + (size_t)kref) * P.n), Uf(P.Uref + (b * (size_t)(P.Nt - 1) + (size_t)kref) * P.m),
        At(P.AconT + b * P.con_istride + (isr ? T_ : 0)), bc(P.bcon + b * P.bcon_istride + (isr ? T_ : 0)),
        c0(isr ? P.rowc0[T_] : 0), cp(isr ? P.rowcp[T_] : 0), dyn(P, b, kref, T_, want_dyn && P.lds_dyn) {}
};

// the constraint row of knot k that lane T < Pn owns (c.At, c.bc: the lane's row and offset of knot 0; c.c0, c.cp: its cone).
// Every lane of the wave is here (the shuffles read live lanes); P.Pn > 0.
__device__ __forceinline__ ConRow conw_row(const EvalW& P, const CtxW& c, int k, double x, double u) {
  const int n = P.n, m = P.m, nz = P.n + P.m, Pn = P.Pn;
  const bool term = k == P.N - 1;
  const int ct = c.isr ? P.ctype[(size_t)k * Pn + c.T] : 0;
  ConRow r;
  r.on = ct != CT_NONE; r.soc = ct == CT_SOC; r.eq = ct == CT_EQ; r.p = c.cp; r.pos = c.T - c.c0;
  const double* Ak = c.At + (size_t)k * nz * Pn;
  double v = r.on ? c.bc[(size_t)k * Pn] : 0.0;
  v = evalw_dot(Ak, (size_t)Pn, x, n, v, r.on);
  if (!term) v = evalw_dot(Ak + (size_t)n * Pn, (size_t)Pn, u, m, v, r.on);
  r.v = v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double s = __shfl(v, (c.c0 + q) & 63, 64);
    r.vq[q] = q < c.cp ? s : 0.0;
  }
  return r;
}
// the running maximum with the knot's rows (in and out by value), and the lane's signed residual (0 without an active row)
__device__ __forceinline__ double conw_max(double viol, const EvalW& P, const CtxW& c, int k, double x, double u) {
  if (P.Pn > 0) {
    const ConRow r = conw_row(P, c, k, x, u);
    if (r.on) viol = eval_max(viol, row_violation(r));
  }
  return viol;
}
__device__ __forceinline__ double conw_residual(const EvalW& P, const CtxW& c, int k, double x, double u) {
  return row_residual(conw_row(P, c, k, x, u));
}

// the cost of knot k of the wave added to the lane's sum: x, u = the lane's elements (0 where it owns none, u = 0 at the
// terminal knot)
__device__ __forceinline__ double costw_knot(double cost, const EvalW& P, const CtxW& c, int k, double x, double u) {
  const bool term = k == P.N - 1;
  if (c.isx) cost += cost_term(term ? c.wfx : c.wx, x, c.Xf[(size_t)k * P.n + c.T]);
  if (c.isu && !term) cost += cost_term(c.wu, u, c.Uf[(size_t)k * P.m + c.T]);
  return cost;
}

// knot k of the wave: cost, box, constraint rows
__device__ __forceinline__ void scorew_knot(Score& s, const EvalW& P, const CtxW& c, int k, double x, double u) {
  const bool uon = c.isu && k != P.N - 1;
  s.cost = costw_knot(s.cost, P, c, k, x, u);
  if (k >= P.box_k0 && k <= P.box_k1) {
    s.viol = box_max(s.viol, c.isx, x, c.xlo, c.xhi);
    s.viol = box_max(s.viol, uon, u, c.ulo, c.uhi);
  }
  s.viol = conw_max(s.viol, P, c, k, x, u);
}

__global__ void k_eval_rollout_wide(double* __restrict__ Xw, const double* __restrict__ U, const double* __restrict__ x0, EvalW P, int ncand,
                                    size_t R) {
#pragma clang fp contract(off)
  const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int T = (int)(threadIdx.x & 63);
  if (r >= R) return;   // (whole waves)
  const size_t b = r / (size_t)ncand;
  const int n = P.n, m = P.m, N = P.N;
  const bool isx = T < n, isu = T < m;
  double* Xr = Xw + r * (size_t)N * n;
  const double* Ur = U + r * (size_t)(N - 1) * m;
  const EvalWDyn dyn(P, b, eval_window(P.window, P.kref, b, N, P.Nt), T, P.lds_dyn != 0);
  double x = isx ? x0[b * (size_t)n + T] : 0.0;
  for (int k = 0;; ++k) {
    if (isx) Xr[(size_t)k * n + T] = x;
    if (k == N - 1) break;
    const double u = isu ? Ur[(size_t)k * m + T] : 0.0;
    x = evalw_advance(dyn, k, x, u, isx);
  }
}

__global__ void k_eval_score_wide(double* __restrict__ J, double* __restrict__ cmax, double* __restrict__ defect, const double* __restrict__ X,
                                  const double* __restrict__ U, EvalW P, int ncand, size_t R, int given) {
#pragma clang fp contract(off)
  const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int T = (int)(threadIdx.x & 63);
  if (r >= R) return;
  const size_t b = r / (size_t)ncand;
  const int n = P.n, m = P.m, N = P.N;
  const bool want_defect = defect != nullptr && given != 0;
  const CtxW c(P, b, T, want_defect);
  const bool isx = c.isx;
  const double* Xr = X + r * (size_t)N * n;
  const double* Ur = U + r * (size_t)(N - 1) * m;
  Score s;
  double dfc = 0.0;
  for (int k = 0; k < N; ++k) {
    const bool term = k == N - 1;
    const double x = isx ? Xr[(size_t)k * n + T] : 0.0;
    const bool uon = c.isu && !term;
    const double u = uon ? Ur[(size_t)k * m + T] : 0.0;
    // scorew_knot's terms with the defect between the box and the constraint rows, where it always stood
    s.cost = costw_knot(s.cost, P, c, k, x, u);
    if (k >= P.box_k0 && k <= P.box_k1) {
      s.viol = box_max(s.viol, isx, x, c.xlo, c.xhi);
      s.viol = box_max(s.viol, uon, u, c.ulo, c.uhi);
    }
    if (want_defect && !term) {
      const double pred = c.dyn.step(k, x, u);
      if (isx) dfc = eval_max(dfc, fabs(pred - Xr[(size_t)(k + 1) * n + T]));
    }
    s.viol = conw_max(s.viol, P, c, k, x, u);
  }
  double Jr, cr;
  score_reduce<64>(s, Jr, cr);
  dfc = lanes_max<64>(dfc);
  if (T != 0) return;
  if (J != nullptr) J[r] = Jr;
  if (cmax != nullptr) cmax[r] = cr;
  if (defect != nullptr) defect[r] = dfc;
}

}  // namespace altro
