// evaluate_grad.h -- the gradient of a candidate's merit with respect to its controls and its initial state
// (altro_batch_evaluate_grad(_dev); include/altro_batch.h).  For every row (instance b, candidate c):
//   X   the rollout of evaluate.h (eval16_step / EvalWDyn::step: the bytes k_eval_rollout* writes)
//   J   the plain tracking cost (cost16_knot / costw_knot: the bytes k_eval_score* writes)
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
// THE KERNELS ARE MADE OF THE SCORING CORE (evaluate.h): the forward phase of its step and its per-knot cost, the
// reverse phase of the row value behind c_max (con16_residual / conw_residual: con16_row / conw_row, then the signed residual
// where the scoring kernels take the violation), of box_sides and of the dynamics slice EvalWDynT<true>.  What stands here is
// the reverse sweep alone.  Contraction is off and every fused multiply-add is written out.  The order of every sum that
// evaluate.h does not already state is stated here, and here only:
//   residual pullback   c = (box: r_hi - r_lo of the element, one subtraction; 0 outside the box's range);
//                       c = fma(a_r[element], r_r, c) for the rows r = 0, 1, .. in turn (16 lanes of rows; Pn rows)
//   local term          g = w * e (one product, e = z - zref rounded first); rho > 0: g = fma(rho, c, g); rho == 0: no c at all
//   transposed product  acc = g; acc = fma([A B][i][element], lambda_i, acc) for i = 0, 1, .., n - 1 in turn
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

__device__ __forceinline__ double grad_sq(double acc, double r) {
#pragma clang fp contract(off)
  const double q = r * r;
  return acc + q;
}

// ------------------------------------------------------------------ 16-lane backend
__global__ void k_eval_grad16(GradIO io, int x0s, Eval16 P, int ncand, size_t R, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const auto [r, b, lane, live, in, isx, isu] = eval16_row(R, rows, (size_t)ncand, n, m);
  if (!in) return;
  const Ctx16 c(P, b, lane);
  double* Xr = io.Xw + r * (size_t)N * n;
  const double* Ur = io.U + r * (size_t)(N - 1) * m;
  // forward: k_eval_rollout16's recursion with the cost of every knot it passes
  double cost = 0.0;
  {
    double g[16], fv;
    eval16_dyn(P, b, lane, g, fv);
    double x = isx ? io.x0[b * (size_t)x0s + lane] : 0.0;
    for (int k = 0;; ++k) {
      const bool term = k == N - 1;
      const bool on = isx || (isu && !term);
      const double z = isx ? x : (on ? Ur[(size_t)k * m + (lane - n)] : 0.0);
      if (live && isx) Xr[(size_t)k * n + lane] = x;   // (after the load of u: before it, the load would wait for the store)
      cost = cost16_knot(cost, P, c, k, z, c.Zr[(size_t)k * 16]);
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
    if (k >= P.box_k0 && k <= P.box_k1) {
      const BoxSides s = box_sides(on, z, c.zlo, c.zhi);
      rhi = s.res_hi(); rlo = s.res_lo();
    }
    pen = grad_sq(pen, rhi);
    pen = grad_sq(pen, rlo);
    double cz = rhi - rlo;
    if (P.ncrows > 0) {
      const double res = con16_residual(P, c, k, z);
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
__global__ void k_eval_grad_wide(GradIO io, EvalW P, int ncand, size_t R, int use_lds) {
#pragma clang fp contract(off)
  const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int T = (int)(threadIdx.x & 63);
  if (r >= R) return;   // (whole waves)
  const size_t b = r / (size_t)ncand;
  const int n = P.n, m = P.m, N = P.N, nz = P.n + P.m, Pn = P.Pn;
  const CtxW c(P, b, T, false);
  const EvalWDynT<true> dyn(P, b, c.kref, T, use_lds != 0);   // (padded: tstep reads the slice transposed)
  const bool isx = c.isx, isu = c.isu;
  double* Xr = io.Xw + r * (size_t)N * n;
  const double* Ur = io.U + r * (size_t)(N - 1) * m;
  // forward: k_eval_rollout_wide's recursion with the cost of every knot it passes
  double cost = 0.0;
  {
    double x = isx ? io.x0[b * (size_t)n + T] : 0.0;
    for (int k = 0;; ++k) {
      if (isx) Xr[(size_t)k * n + T] = x;
      const bool term = k == N - 1;
      const bool uon = isu && !term;
      const double u = uon ? Ur[(size_t)k * m + T] : 0.0;
      cost = costw_knot(cost, P, c, k, x, u);
      if (term) break;
      x = evalw_advance(dyn, k, x, u, isx);
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
      const BoxSides sx = box_sides(isx, x, c.xlo, c.xhi), su = box_sides(uon, u, c.ulo, c.uhi);
      xhi = sx.res_hi(); xlo = sx.res_lo(); uhi = su.res_hi(); ulo = su.res_lo();
    }
    pen = grad_sq(pen, xhi);
    pen = grad_sq(pen, xlo);
    pen = grad_sq(pen, uhi);
    pen = grad_sq(pen, ulo);
    double cx = xhi - xlo, cu = uhi - ulo;
    if (Pn > 0) {
      const double res = conw_residual(P, c, k, x, u);
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
