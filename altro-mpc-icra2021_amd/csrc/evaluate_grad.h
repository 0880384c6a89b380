// evaluate_grad.h -- the gradient of a candidate's merit with respect to its controls and its initial state
// (altro_batch_evaluate_grad(_dev); include/altro_batch.h).  For every row (instance b, candidate c):
//   X   the rollout of evaluate.h (eval16_step / evalw_dot in evalw_step's order: the bytes k_eval_rollout* writes)
//   J   the plain tracking cost with cost_term in the scoring core's order: the bytes k_eval_score* writes
//   P   = 1/2 sum r^2 over every constraint, every knot of its range and every row, r the signed distance to the feasible set:
//         BOX max(0, z - hi), max(0, lo - z); LINEAR v (equality), max(0, v) (inequality); SOC the vector v - Proj(v)
//   gU, gx0   the gradient of M = J + rho P:  lambda_{N-1} = wf e_x + rho c_x,  gU_k = wd e_u + rho c_u + B_k' lambda_{k+1},
//         lambda_k = wd e_x + rho c_x + A_k' lambda_{k+1},  gx0 = lambda_0,  c_z = the residuals pulled back through the rows
// ONE kernel per backend, two phases per row.  FORWARD: roll out, store the states (Xout or the handle's workspace), add up J.
// REVERSE: k = N-1 .. 0, every lane reads back the states IT stored (so no fence and no second launch is needed), forms the
// row values, the residuals and P, pulls the residuals back and steps the costate.  The row values are formed once, in the
// reverse phase, where both P and the pullback need them.  One launch because registers allow it: the forward phase's
// coefficients are dead when the reverse phase loads the transposed ones (DESIGN.md 7p has the register counts).
// Reads the tables evaluate.h reads through the same structs (Eval16 / EvalW, Ctx16 / CtxW); writes nothing the library owns.
// Contraction is off and every fused multiply-add is written out.  The order of every sum that evaluate.h does not already
// state is stated here, and here only:
//   residual pullback   c = (box: r_hi - r_lo of the element, one subtraction; 0 outside the box's range);
//                       c = fma(a_r[element], r_r, c) for the rows r = 0, 1, .. in turn (16 lanes of rows; Pn rows)
//   local term          g = w * e (one product, e = z - zref rounded first); rho > 0: g = fma(rho, c, g); rho == 0: no c at all
//   transposed product  acc = g; acc = fma([A B][i][element], lambda_i, acc) for i = 0, 1, .., n - 1 in turn
//   SOC residual        n2 = v_0^2 + v_1^2 + .. in turn (products rounded), nv = sqrt(n2), c = 0.5 * (1 + t / nv);
//                       element q < p - 1: v_q - c * v_q; element p - 1: t - c * nv
//   P                   every lane adds r * r (product rounded) knot after knot, k = N-1 .. 0, within a knot: box upper side,
//                       box lower side (one-wave-per-instance backend: state element first, then control element), then the
//                       lane's constraint row; the lanes are then added by evaluate.h's butterfly; P = 0.5 * that sum
// A NaN stays a NaN: max(0, v) keeps a NaN v.
#pragma once
#include "evaluate.h"

namespace altro {

struct GradIO {
  const double *U, *x0;       // [R][N-1][m]; [B] rows of x0s doubles
  double *J, *P, *gU, *gx0;   // [R], [R], [R][N-1][m], [R][n]; any may be null
  double* Xw;                 // [R][N][n]: Xout or the workspace
  double rho;
};

// max(0, v) that keeps a NaN
__device__ __forceinline__ double grad_pos(double v) { return (v > 0.0 || v != v) ? v : 0.0; }

// the two sides of an element's box: residuals rhi, rlo (0 for an infinite side or a lane that holds no element)
__device__ __forceinline__ void grad_box(bool on, double z, double lo, double hi, double& rhi, double& rlo) {
  const bool has_hi = hi < 1e300, has_lo = lo > -1e300;
  rhi = (on && has_hi) ? grad_pos(z - hi) : 0.0;
  rlo = (on && has_lo) ? grad_pos(lo - z) : 0.0;
}

__device__ __forceinline__ double grad_sq(double acc, double r) {
#pragma clang fp contract(off)
  const double q = r * r;
  return acc + q;
}

// element `pos` of v - Proj(v) for a second-order cone of dimension p (2..4) whose values are v[0..p-1]: soc_row_violation's
// three branches with the sign kept
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

// ------------------------------------------------------------------ 16-lane backend
// The residual of the constraint row lane r owns at knot k (0 for a lane without an active row): con16_max's row value, then the
// signed residual.
__device__ __forceinline__ double con16_residual(const Eval16& P, const double* Ac, const double* bc, int pos, int lane, int k, double z) {
  const int n = P.n, m = P.m;
  const int* cm = P.cmeta + ((size_t)k * 16 + lane) * 4;
  const int type = cm[0], p = cm[3];
  const bool act = type != CT_NONE && k >= cm[1] && k <= cm[2];
  double a[16], v = 0.0;
#pragma unroll
  for (int c = 0; c < 16; ++c) a[c] = 0.0;
  if (act) {
    const double* ar = Ac + (size_t)k * 256;
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = c < n + m ? ar[c] : 0.0;
    v = bc[(size_t)k * 16];
  }
  v = row_affine(a, v, z);
  const bool is_soc = type == CT_SOC;
  const bool row_on = act && (!is_soc || pos < p);
  const double vv = (row_on && is_soc) ? v : 0.0;
  double vq[4];
  vq[0] = quad_bcast<0>(vv); vq[1] = quad_bcast<1>(vv); vq[2] = quad_bcast<2>(vv); vq[3] = quad_bcast<3>(vv);
  const double res = is_soc ? soc_row_residual(vq, p, pos) : (type == CT_EQ ? v : grad_pos(v));
  return row_on ? res : 0.0;
}

__global__ void k_eval_grad16(GradIO io, int x0s, Eval16 P, int ncand, size_t R, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const auto [r, b, lane, live, in, isx, isu] = eval16_row(R, rows, (size_t)ncand, n, m);
  if (!in) return;
  const Ctx16 c(P, b, lane);
  double* Xr = io.Xw + r * (size_t)N * n;
  const double* Ur = io.U + r * (size_t)(N - 1) * m;
  // forward: k_eval_rollout16's recursion, k_eval_score16's cost
  double cost = 0.0;
  {
    double g[16], fv;
    eval16_dyn(P, b, lane, g, fv);
    double x = isx ? io.x0[b * (size_t)x0s + lane] : 0.0;
    for (int k = 0;; ++k) {
      if (live && isx) Xr[(size_t)k * n + lane] = x;
      const bool term = k == N - 1;
      const bool on = isx || (isu && !term);
      const double z = isx ? x : (on ? Ur[(size_t)k * m + (lane - n)] : 0.0);
      const double q = cost_term(term ? c.wf : c.wd, z, c.Zr[(size_t)k * 16]);
      cost = on ? cost + q : cost;
      if (term) break;
      x = eval16_step(g, fv, z, isx);
    }
  }
  const double Jr = 0.5 * lanes_sum<16>(cost);
  const bool want_g = io.gU != nullptr || io.gx0 != nullptr;
  if (io.P == nullptr && !want_g) {
    if (live && lane == 0 && io.J != nullptr) io.J[r] = Jr;
    return;
  }
  // reverse.  gt[i] = [A B][i][lane]: the lane's column, Grow[b][lane][0..n-1], contiguous
  double gt[16];
  {
    const double* G = P.Grow + b * 256 + (size_t)lane * 16;
#pragma unroll
    for (int i = 0; i < 16; ++i) gt[i] = (want_g && i < n && lane < n + m) ? G[i] : 0.0;
  }
  const bool use_c = io.rho > 0.0;
  double* gUr = io.gU != nullptr ? io.gU + r * (size_t)(N - 1) * m : nullptr;
  double lam = 0.0, pen = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    const bool term = k == N - 1;
    const bool on = isx || (isu && !term);
    // (a padded row reads row 0's states while their owner may still be writing them: it stores nothing)
    const double z = isx ? Xr[(size_t)k * n + lane] : (on ? Ur[(size_t)k * m + (lane - n)] : 0.0);
    double rhi = 0.0, rlo = 0.0;
    if (k >= P.box_k0 && k <= P.box_k1) grad_box(on, z, c.zlo, c.zhi, rhi, rlo);
    pen = grad_sq(pen, rhi);
    pen = grad_sq(pen, rlo);
    double cz = rhi - rlo;
    if (P.ncrows > 0) {
      const double res = con16_residual(P, c.Ac, c.bc, c.pos, lane, k, z);
      pen = grad_sq(pen, res);
      if (use_c && want_g) {
        const double* At = P.Acon + b * P.con_istride + (size_t)k * 256 + lane;   // column `lane` of the knot's table
        double at[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) at[q] = lane < n + m ? At[q * 16] : 0.0;
        cz = row_affine(at, cz, res);
      }
    }
    if (!want_g) continue;
    const double e = z - c.Zr[(size_t)k * 16];
    double g = (term ? c.wf : c.wd) * e;
    if (use_c) g = __builtin_fma(io.rho, cz, g);
    g = on ? g : 0.0;
    const double acc = term ? g : row_affine(gt, g, lam);
    if (live && isu && !term && gUr != nullptr) gUr[(size_t)k * m + (lane - n)] = acc;
    lam = isx ? acc : 0.0;
  }
  const double Pr = 0.5 * lanes_sum<16>(pen);
  if (!live) return;
  if (isx && io.gx0 != nullptr) io.gx0[r * (size_t)n + lane] = lam;
  if (lane != 0) return;
  if (io.J != nullptr) io.J[r] = Jr;
  if (io.P != nullptr) io.P[r] = Pr;
}

// ------------------------------------------------------------------ one-wave-per-instance backend
// The dynamics of instance b as the wave reads them forwards (row T of [A | B]) and transposed (column T).  Time-invariant
// blocks that fit are copied once into the wave's slice of LDS, as EvalWDyn does, but with the leading dimension padded to an
// odd number of doubles: lane j's transposed run starts at j * ld, and a ds_read_b64 of 32 lanes is conflict-free exactly when
// j * ld mod 32 takes 32 values (MI355X: 64 banks of 4 bytes, a double takes two).  The forward reads (element
// T + j * ld, j uniform) are consecutive either way.  The values and the order of every sum are those of EvalWDyn::step.
__host__ __device__ inline int gradw_ld(int n) { return n | 1; }
__host__ __device__ inline size_t gradw_lds_doubles(int n, int m) { return (size_t)gradw_ld(n) * (n + m); }
__host__ __device__ inline size_t gradw_lds_bytes(int n, int m) { return 4 * gradw_lds_doubles(n, m) * sizeof(double); }
__host__ __device__ inline bool gradw_lds_fits(int n, int m, int ltv) { return !ltv && gradw_lds_bytes(n, m) <= 65536; }

struct GradWDyn {
  const EvalW& P;
  size_t b;
  int kref, Tn, Tm;
  const double* lds;   // the wave's padded [A | B] in LDS, or null
  int ld;
  double f0;
  __device__ __forceinline__ GradWDyn(const EvalW& p, size_t b_, int kref_, int T, bool use_lds)
      : P(p), b(b_), kref(kref_), Tn(T < p.n ? T : p.n - 1), Tm(T < p.m ? T : p.m - 1), lds(nullptr), ld(p.n), f0(0.0) {
    if (!use_lds) return;
    extern __shared__ double eval_lds[];
    ld = gradw_ld(P.n);
    double* slice = eval_lds + (threadIdx.x >> 6) * gradw_lds_doubles(P.n, P.m);
    const size_t blk = evalw_block(P, b, kref, 0);
    const int n = P.n, na = P.n * P.n, nb = P.n * P.m;
    for (int e = T; e < na; e += 64) slice[(e / n) * ld + e % n] = P.A[blk * na + e];
    for (int e = T; e < nb; e += 64) slice[(n + e / n) * ld + e % n] = P.Bm[blk * nb + e];
    f0 = P.f != nullptr ? P.f[blk * P.n + Tn] : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    lds = slice;
  }
  // evalw_step's sums: row Tn of A x + B u + f
  __device__ __forceinline__ double step(int k, double xs, double us) const {
    const int n = P.n, m = P.m;
    if (lds != nullptr) return evalw_dot(lds + n * ld + Tn, (size_t)ld, us, m, evalw_dot(lds + Tn, (size_t)ld, xs, n, f0, true), true);
    const size_t blk = evalw_block(P, b, kref, k);
    return evalw_step(P.A + blk * n * n + Tn, P.Bm + blk * n * m + Tn, P.f != nullptr ? P.f[blk * n + Tn] : 0.0, n, m, xs, us);
  }
  // acc + column Tn of A_k (bt: column Tm of B_k) times lambda, i = 0 .. n-1 in turn
  __device__ __forceinline__ double tstep(int k, bool bt, double lam, double acc, bool on) const {
    const int n = P.n, m = P.m;
    if (lds != nullptr) return evalw_dot(lds + (size_t)(bt ? n + Tm : Tn) * ld, 1, lam, n, acc, on);
    const size_t blk = evalw_block(P, b, kref, k);
    const double* col = bt ? P.Bm + blk * n * m + (size_t)Tm * n : P.A + blk * n * n + (size_t)Tn * n;
    return evalw_dot(col, 1, lam, n, acc, on);
  }
};

// The residual of the constraint row lane T owns at knot k (0 for a lane without an active row): conw_max's row value, then the
// signed residual.
__device__ __forceinline__ double conw_residual(const EvalW& P, const double* At, const double* bc, int c0, int cp, bool isr, int T, int k,
                                                double x, double u) {
  const int n = P.n, m = P.m, nz = P.n + P.m, Pn = P.Pn;
  const bool term = k == P.N - 1;
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
  const double res = ct == 3 ? soc_row_residual(vq, cp, T - c0) : (ct == 1 ? v : grad_pos(v));
  return on ? res : 0.0;
}

__global__ void k_eval_grad_wide(GradIO io, EvalW P, int ncand, size_t R, int use_lds) {
#pragma clang fp contract(off)
  const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int T = (int)(threadIdx.x & 63);
  if (r >= R) return;   // (whole waves)
  const size_t b = r / (size_t)ncand;
  const int n = P.n, m = P.m, N = P.N, nz = P.n + P.m, Pn = P.Pn;
  const CtxW c(P, b, T, false);
  const GradWDyn dyn(P, b, c.kref, T, use_lds != 0);
  const bool isx = c.isx, isu = c.isu;
  double* Xr = io.Xw + r * (size_t)N * n;
  const double* Ur = io.U + r * (size_t)(N - 1) * m;
  // forward: k_eval_rollout_wide's recursion, k_eval_score_wide's cost
  double cost = 0.0;
  {
    double x = isx ? io.x0[b * (size_t)n + T] : 0.0;
    for (int k = 0;; ++k) {
      if (isx) Xr[(size_t)k * n + T] = x;
      const bool term = k == N - 1;
      const bool uon = isu && !term;
      const double u = uon ? Ur[(size_t)k * m + T] : 0.0;
      if (isx) cost += cost_term(term ? c.wfx : c.wx, x, c.Xf[(size_t)k * n + T]);
      if (uon) cost += cost_term(c.wu, u, c.Uf[(size_t)k * m + T]);
      if (term) break;
      const double nx = dyn.step(k, x, u);
      x = isx ? nx : 0.0;
    }
  }
  const double Jr = 0.5 * lanes_sum<64>(cost);
  const bool want_g = io.gU != nullptr || io.gx0 != nullptr;
  if (io.P == nullptr && !want_g) {
    if (T == 0 && io.J != nullptr) io.J[r] = Jr;
    return;
  }
  const bool use_c = io.rho > 0.0;
  double* gUr = io.gU != nullptr ? io.gU + r * (size_t)(N - 1) * m : nullptr;
  double lam = 0.0, pen = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    const bool term = k == N - 1;
    const bool uon = isu && !term;
    const double x = isx ? Xr[(size_t)k * n + T] : 0.0;   // (the lane's own stores of the forward phase)
    const double u = uon ? Ur[(size_t)k * m + T] : 0.0;
    double xhi = 0.0, xlo = 0.0, uhi = 0.0, ulo = 0.0;
    if (k >= P.box_k0 && k <= P.box_k1) {
      grad_box(isx, x, c.xlo, c.xhi, xhi, xlo);
      grad_box(uon, u, c.ulo, c.uhi, uhi, ulo);
    }
    pen = grad_sq(pen, xhi);
    pen = grad_sq(pen, xlo);
    pen = grad_sq(pen, uhi);
    pen = grad_sq(pen, ulo);
    double cx = xhi - xlo, cu = uhi - ulo;
    if (Pn > 0) {
      const double res = conw_residual(P, c.At, c.bc, c.c0, c.cp, c.isr, T, k, x, u);
      pen = grad_sq(pen, res);
      if (use_c && want_g) {   // element e's column of the knot's table: AconT[k][e][0 .. Pn-1], contiguous
        const double* Ak = P.AconT + b * P.con_istride + (size_t)k * nz * Pn;
        cx = evalw_dot(Ak + (size_t)c.Tn * Pn, 1, res, Pn, cx, isx);
        if (!term) cu = evalw_dot(Ak + (size_t)(n + c.Tm) * Pn, 1, res, Pn, cu, uon);
      }
    }
    if (!want_g) continue;
    double gx = 0.0, gu = 0.0;
    if (isx) {
      const double e = x - c.Xf[(size_t)k * n + T];
      gx = (term ? c.wfx : c.wx) * e;
      if (use_c) gx = __builtin_fma(io.rho, cx, gx);
    }
    if (uon) {
      const double e = u - c.Uf[(size_t)k * m + T];
      gu = c.wu * e;
      if (use_c) gu = __builtin_fma(io.rho, cu, gu);
    }
    if (!term) {
      gu = dyn.tstep(k, true, lam, gu, isu);
      gx = dyn.tstep(k, false, lam, gx, isx);
      if (isu && gUr != nullptr) gUr[(size_t)k * m + T] = gu;
    }
    lam = isx ? gx : 0.0;
  }
  const double Pr = 0.5 * lanes_sum<64>(pen);
  if (isx && io.gx0 != nullptr) io.gx0[r * (size_t)n + T] = lam;
  if (T != 0) return;
  if (io.J != nullptr) io.J[r] = Jr;
  if (io.P != nullptr) io.P[r] = Pr;
}

}  // namespace altro
