// evaluate_al.h -- the solver's augmented Lagrangian L_A(U; lambda, mu) of a control sequence, with the multipliers and the
// penalty the handle holds, its gradient with respect to the controls and the initial state, and its partial derivatives with
// respect to the problem data (altro_batch_evaluate_al(_dev); include/altro_batch.h).  For every row (instance b,
// candidate c):
//   X, J   the rollout and the plain tracking cost of evaluate.h (the bytes altro_batch_evaluate_dev writes)
//   L_A    = J + sum over every constraint, every knot of its range and every row of
//              BOX finite side / LINEAR row, value c, dual l:  l c + [a] mu c^2 / 2,  a = equality | c >= 0 | l > 0;  g = l + [a] mu c
//              SOC, value v, duals l:  (|y|^2 - |l|^2) / (2 mu),  y = Proj_K(l - mu v);  pulled back as -A' y
//   gU, gx0   one costate sweep, c_z the pullback sum (BOX: + g on the element for an upper side, - g for a lower side; a_r g
//          for a row):  lam_{N-1} = wf e_x + c_x,  gU_k = wd e_u + c_u + B_k' lam_{k+1},  lam_k = wd e_x + c_x + A_k' lam_{k+1},
//          gx0 = lam_0
//   gXref, gUref   -(w e) per knot (the cost term only);  gQ, gR = dt / 2 sum_{k < N-1} e^2,  gQf = e_{N-1}^2 / 2;
//   gzmax = - sum_k g_hi,  gzmin = + sum_k g_lo  (0 on infinite sides)
// ONE kernel per backend in the two phases of evaluate_grad.h: FORWARD rolls out, stores the states and adds up J; REVERSE,
// k = N-1 .. 0, every lane reads back the states IT stored.  The kernels are made of the scoring core (evaluate.h): its step,
// its per-knot cost, its row value (con16_row / conw_row), box_sides and the dynamics slice EvalWDynT<true>.  What stands here
// is the augmented-Lagrangian term of a row (al_lin, al_soc) beside row_residual, the reads of the duals and the penalty in
// the layouts the solve kernels keep them in, and the lane-local sums: lane j owns element j, adds up its own gQ / gR / gQf,
// gzmax and gzmin and stores its element of gXref / gUref at every knot.
//   16-lane backend:  Lb [Bp][N+1][2][nbp] (side 0 upper; the lane's slot bslot[lane], -1: no dual), Lc [Bp][N+1][16] (row =
//                     lane), mu [Bp]
//   wide backend:     Lb [B][N][2][n+m], Lc [B][N][Pn], mu [B]
// A null output skips its work: J alone ends after the forward phase; without LA, gU and gx0 no constraint row is formed;
// without gU and gx0 there is no pullback and no costate.  Contraction is off and every fused multiply-add is written out.  The
// order of every sum that evaluate.h and evaluate_grad.h do not already state:
//   linear term         t = l * c (rounded), pen += t; active: q = c * c, q = mu * q, q = 0.5 * q, pen += q; g = fma(mu, c, l)
//                       (inactive: g = l)
//   cone term           w_q = fma(-mu, v_q, l_q); y = Proj_K(w) as soc_project has it (n2 = w_0^2 + w_1^2 + .. in turn, products
//                       rounded; c = 0.5 * (1 + t / nv)); the lane adds (y * y - l * l), both products rounded, to soc; g = -y
//   per knot, per lane  k = N-1 .. 0; within a knot: box upper side, box lower side (wide: state element first, then control
//                       element), then the lane's constraint row
//   pullback            c = g_hi - g_lo (one subtraction), then fma(a_r[element], g_r, c) for the rows r = 0, 1, .. in turn
//   local term          ge = w * e (e = z - zref rounded first); g = ge + c; transposed product as evaluate_grad.h
//   L_A                 pen and soc are added over the lanes by evaluate.h's butterfly; L_A = (J + Pen) + Soc / (2 mu)
//   data sums           s2 += e * e (product rounded), k = N-2 .. 0; gQ, gR = (dt / 2) * s2; gQf = 0.5 * (e * e) of knot N-1;
//                       gzmax = -(sum of g_hi, k = N-1 .. 0), gzmin = sum of g_lo
// A NaN stays a NaN: a NaN row value counts as active.
// THE FORWARD PHASE is the scoring core's step and per-knot cost in the ten-line loop k_eval_grad16 / k_eval_grad_wide hold, and
// it is restated here, not shared: those two kernels must keep the parent's device code, and moved into one __device__ function
// called from all four the loop gave k_eval_grad16 another register allocation and 22 more instructions, and k_eval_al16 itself
// a 20 % longer run time at (12, 4, 50).
#pragma once
#include "evaluate.h"

namespace altro {

struct ALIO {
  const double *U, *x0;   // [R][N-1][m]; [B] rows of x0s doubles
  double *LA, *J, *gU, *gx0, *gXref, *gUref, *gQ, *gQf, *gR, *gzmin, *gzmax;   // any may be null
  double* Xw;             // [R][N][n]: Xout or the workspace
  const double *Lb, *Lc, *mu;   // the duals and the penalty as the solve kernels keep them
  const int* bslot;       // 16-lane backend: [16] slot of the lane's element in the compact box rows
  int nbp;
  double hdt;             // dt / 2
};

// the term of a BOX side or a LINEAR row of value c with dual l added to the lane's sum; returns g = dL_A / dc
__device__ __forceinline__ double al_lin(double& pen, double c, double l, double mu, bool eq) {
#pragma clang fp contract(off)
  const bool active = eq || !(c < 0.0) || l > 0.0;
  const double t = l * c;
  pen = pen + t;
  if (!active) return l;
  double q = c * c;
  q = mu * q;
  q = 0.5 * q;
  pen = pen + q;
  return __builtin_fma(mu, c, l);
}

// element `pos` of Proj_K(w), K the second-order cone of dimension p (2..4), w[q] = 0 for q >= p: the oracle's soc_project
// (soc_row_residual of evaluate.h is w - this)
__device__ __forceinline__ double soc_row_proj(const double (&w)[4], int p, int pos) {
#pragma clang fp contract(off)
  const int pt = p - 1;
  double n2 = 0.0, t = 0.0, mine = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    n2 = q < pt ? n2 + w[q] * w[q] : n2;
    t = q == pt ? w[q] : t;
    mine = q == pos ? w[q] : mine;
  }
  const double nv = sqrt(n2);
  if (nv <= t) return mine;
  if (nv <= -t) return 0.0;
  const double c = 0.5 * (1.0 + t / nv);
  return pos == pt ? c * nv : c * mine;   // (a NaN anywhere in the cone fails both tests above and comes out here)
}

// the lane's row of a cone with the cone's duals lq (0 beyond p) and its own dual l: y^2 - l^2 added to soc; returns g = -y
__device__ __forceinline__ double al_soc(double& soc, const ConRow& r, const double (&lq)[4], double l, double mu) {
#pragma clang fp contract(off)
  double w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = __builtin_fma(-mu, r.vq[q], lq[q]);
  const double y = soc_row_proj(w, r.p, r.pos);
  const double a = y * y, b = l * l;
  soc = soc + (a - b);
  return -y;
}

// what a row's lane makes of its row: 0 without an active row
__device__ __forceinline__ double al_row(double& pen, double& soc, const ConRow& r, const double (&lq)[4], double l, double mu) {
  if (!r.on) return 0.0;
  return r.soc ? al_soc(soc, r, lq, l, mu) : al_lin(pen, r.v, l, mu, r.eq);
}

__device__ __forceinline__ double al_sq(double acc, double e) {
#pragma clang fp contract(off)
  const double q = e * e;
  return acc + q;
}

// ------------------------------------------------------------------ 16-lane backend
__global__ void __launch_bounds__(256) k_eval_al16(ALIO io, int x0s, Eval16 P, int ncand, size_t R, size_t rows) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.m, N = P.N;
  const auto [r, b, lane, live, in, isx, isu] = eval16_row(R, rows, (size_t)ncand, n, m);
  if (!in) return;
  const Ctx16 c(P, b, lane);
  double* Xr = io.Xw + r * (size_t)N * n;
  const double* Ur = io.U + r * (size_t)(N - 1) * m;
  // forward: k_eval_grad16's loop, restated (see the note on the forward phase above)
  double cost = 0.0;
  {
    double g[16], fv;
    eval16_dyn(P, b, lane, g, fv);
    double x = isx ? io.x0[b * (size_t)x0s + lane] : 0.0;
    for (int k = 0;; ++k) {
      const bool term = k == N - 1;
      const bool on = isx || (isu && !term);
      const double z = isx ? x : (on ? Ur[(size_t)k * m + (lane - n)] : 0.0);
      if (live && isx) Xr[(size_t)k * n + lane] = x;
      cost = cost16_knot(cost, P, c, k, z, c.Zr[(size_t)k * 16]);
      if (term) break;
      x = eval16_step(g, fv, z, isx);
    }
  }
  const double Jr = 0.5 * lanes_sum<16>(cost);
  const bool want_g = io.gU != nullptr || io.gx0 != nullptr;
  const bool want_rows = want_g || io.LA != nullptr;
  const bool want_box = want_rows || io.gzmin != nullptr || io.gzmax != nullptr;
  const bool want_e = want_g || io.gXref != nullptr || io.gUref != nullptr || io.gQ != nullptr || io.gQf != nullptr || io.gR != nullptr;
  if (!want_box && !want_e) {
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
  const double mu = io.mu[b];
  const int sl = io.bslot[lane];
  const double* Lbr = io.Lb + b * (size_t)(N + 1) * 2 * io.nbp + (sl >= 0 ? sl : 0);
  const double* Lcr = io.Lc + b * (size_t)(N + 1) * 16 + lane;
  double* gUr = io.gU != nullptr ? io.gU + r * (size_t)(N - 1) * m : nullptr;
  double lam = 0.0, pen = 0.0, soc = 0.0, s2 = 0.0, ef2 = 0.0, shi = 0.0, slo = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    const bool term = k == N - 1;
    const bool on = isx || (isu && !term);
    // (a padded row reads row 0's states while their owner may still be writing them: it stores nothing)
    const double z = isx ? Xr[(size_t)k * n + lane] : (on ? Ur[(size_t)k * m + (lane - n)] : 0.0);
    double ghi = 0.0, glo = 0.0;
    if (want_box && k >= P.box_k0 && k <= P.box_k1) {
      const BoxSides s = box_sides(on, z, c.zlo, c.zhi);
      if (s.has_hi) ghi = al_lin(pen, s.over(), sl >= 0 ? Lbr[(size_t)k * 2 * io.nbp] : 0.0, mu, false);
      if (s.has_lo) glo = al_lin(pen, s.under(), sl >= 0 ? Lbr[((size_t)k * 2 + 1) * io.nbp] : 0.0, mu, false);
    }
    shi = shi + ghi;
    slo = slo + glo;
    double cz = ghi - glo;
    if (want_rows && P.ncrows > 0) {
      const ConRow row = con16_row(P, c, k, z);
      const double l = row.on ? Lcr[(size_t)k * 16] : 0.0;
      const double ls = (row.on && row.soc) ? l : 0.0;
      const double lq[4] = {quad_bcast<0>(ls), quad_bcast<1>(ls), quad_bcast<2>(ls), quad_bcast<3>(ls)};
      const double g = al_row(pen, soc, row, lq, l, mu);
      if (want_g) {
        const double* At = P.Acon + b * P.con_istride + (size_t)k * 256 + lane;   // column `lane` of the knot's table
        double at[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) at[q] = lane < n + m ? At[q * 16] : 0.0;
        cz = row_affine(at, cz, g);
      }
    }
    if (!want_e) continue;
    const double e = on ? z - c.Zr[(size_t)k * 16] : 0.0;
    const double ge = (term ? c.wf : c.wd) * e;
    if (term) ef2 = al_sq(ef2, e);
    else s2 = al_sq(s2, e);
    if (live && isx && io.gXref != nullptr) io.gXref[(r * (size_t)N + k) * n + lane] = -ge;
    if (live && isu && !term && io.gUref != nullptr) io.gUref[(r * (size_t)(N - 1) + k) * m + (lane - n)] = -ge;
    if (!want_g) continue;
    double g = ge + cz;
    g = on ? g : 0.0;
    const double acc = term ? g : row_affine(gt, g, lam);
    if (live && isu && !term && gUr != nullptr) gUr[(size_t)k * m + (lane - n)] = acc;
    lam = isx ? acc : 0.0;
  }
  const double Pen = lanes_sum<16>(pen), Soc = lanes_sum<16>(soc);
  if (!live) return;
  if (isx) {
    if (io.gx0 != nullptr) io.gx0[r * (size_t)n + lane] = lam;
    if (io.gQ != nullptr) io.gQ[r * (size_t)n + lane] = io.hdt * s2;
    if (io.gQf != nullptr) io.gQf[r * (size_t)n + lane] = 0.5 * ef2;
  }
  if (isu && io.gR != nullptr) io.gR[r * (size_t)m + (lane - n)] = io.hdt * s2;
  if (lane < n + m) {
    if (io.gzmax != nullptr) io.gzmax[r * (size_t)(n + m) + lane] = -shi;
    if (io.gzmin != nullptr) io.gzmin[r * (size_t)(n + m) + lane] = slo;
  }
  if (lane != 0) return;
  if (io.J != nullptr) io.J[r] = Jr;
  if (io.LA != nullptr) io.LA[r] = (Jr + Pen) + Soc / (2.0 * mu);
}

// ------------------------------------------------------------------ one-wave-per-instance backend
__global__ void __launch_bounds__(256) k_eval_al_wide(ALIO io, EvalW P, int ncand, size_t R, int use_lds) {
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
  // forward: k_eval_grad_wide's loop, restated
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
  const bool want_rows = want_g || io.LA != nullptr;
  const bool want_box = want_rows || io.gzmin != nullptr || io.gzmax != nullptr;
  const bool want_e = want_g || io.gXref != nullptr || io.gUref != nullptr || io.gQ != nullptr || io.gQf != nullptr || io.gR != nullptr;
  if (!want_box && !want_e) {
    if (T == 0 && io.J != nullptr) io.J[r] = Jr;
    return;
  }
  const double mu = io.mu[b];
  const double* Lbx = io.Lb + b * (size_t)N * 2 * nz + c.Tn;
  const double* Lbu = io.Lb + b * (size_t)N * 2 * nz + n + c.Tm;
  const double* Lcr = io.Lc + b * (size_t)N * (Pn > 0 ? Pn : 1) + (c.isr ? T : 0);
  double* gUr = io.gU != nullptr ? io.gU + r * (size_t)(N - 1) * m : nullptr;
  double lam = 0.0, pen = 0.0, soc = 0.0, s2x = 0.0, s2u = 0.0, ef2 = 0.0, sxhi = 0.0, sxlo = 0.0, suhi = 0.0, sulo = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    const bool term = k == N - 1;
    const bool uon = isu && !term;
    const double x = isx ? Xr[(size_t)k * n + T] : 0.0;   // (the lane's own stores of the forward phase)
    const double u = uon ? Ur[(size_t)k * m + T] : 0.0;
    double xhi = 0.0, xlo = 0.0, uhi = 0.0, ulo = 0.0;
    if (want_box && k >= P.box_k0 && k <= P.box_k1) {
      const BoxSides sx = box_sides(isx, x, c.xlo, c.xhi), su = box_sides(uon, u, c.ulo, c.uhi);
      if (sx.has_hi) xhi = al_lin(pen, sx.over(), Lbx[(size_t)k * 2 * nz], mu, false);
      if (sx.has_lo) xlo = al_lin(pen, sx.under(), Lbx[((size_t)k * 2 + 1) * nz], mu, false);
      if (su.has_hi) uhi = al_lin(pen, su.over(), Lbu[(size_t)k * 2 * nz], mu, false);
      if (su.has_lo) ulo = al_lin(pen, su.under(), Lbu[((size_t)k * 2 + 1) * nz], mu, false);
    }
    sxhi = sxhi + xhi; sxlo = sxlo + xlo; suhi = suhi + uhi; sulo = sulo + ulo;
    double cx = xhi - xlo, cu = uhi - ulo;
    if (want_rows && Pn > 0) {
      const ConRow row = conw_row(P, c, k, x, u);
      const double l = row.on ? Lcr[(size_t)k * Pn] : 0.0;
      const double ls = (row.on && row.soc) ? l : 0.0;
      double lq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double s = __shfl(ls, (c.c0 + q) & 63, 64);
        lq[q] = q < c.cp ? s : 0.0;
      }
      const double g = al_row(pen, soc, row, lq, l, mu);
      if (want_g) {   // element e's column of the knot's table: AconT[k][e][0 .. Pn-1], contiguous
        const double* Ak = P.AconT + b * P.con_istride + (size_t)k * nz * Pn;
        cx = evalw_dot(Ak + (size_t)c.Tn * Pn, 1, g, Pn, cx, isx);
        if (!term) cu = evalw_dot(Ak + (size_t)(n + c.Tm) * Pn, 1, g, Pn, cu, uon);
      }
    }
    if (!want_e) continue;
    double gx = 0.0, gu = 0.0;
    if (isx) {
      const double e = x - c.Xf[(size_t)k * n + T];
      const double ge = (term ? c.wfx : c.wx) * e;
      if (term) ef2 = al_sq(ef2, e);
      else s2x = al_sq(s2x, e);
      if (io.gXref != nullptr) io.gXref[(r * (size_t)N + k) * n + T] = -ge;
      gx = ge + cx;
    }
    if (uon) {
      const double e = u - c.Uf[(size_t)k * m + T];
      const double ge = c.wu * e;
      s2u = al_sq(s2u, e);
      if (io.gUref != nullptr) io.gUref[(r * (size_t)(N - 1) + k) * m + T] = -ge;
      gu = ge + cu;
    }
    if (!want_g) continue;
    if (!term) {
      gu = dyn.tstep(k, true, lam, gu, isu);
      gx = dyn.tstep(k, false, lam, gx, isx);
      if (isu && gUr != nullptr) gUr[(size_t)k * m + T] = gu;
    }
    lam = isx ? gx : 0.0;
  }
  const double Pen = lanes_sum<64>(pen), Soc = lanes_sum<64>(soc);
  if (isx) {
    if (io.gx0 != nullptr) io.gx0[r * (size_t)n + T] = lam;
    if (io.gQ != nullptr) io.gQ[r * (size_t)n + T] = io.hdt * s2x;
    if (io.gQf != nullptr) io.gQf[r * (size_t)n + T] = 0.5 * ef2;
    if (io.gzmax != nullptr) io.gzmax[r * (size_t)nz + T] = -sxhi;
    if (io.gzmin != nullptr) io.gzmin[r * (size_t)nz + T] = sxlo;
  }
  if (isu) {
    if (io.gR != nullptr) io.gR[r * (size_t)m + T] = io.hdt * s2u;
    if (io.gzmax != nullptr) io.gzmax[r * (size_t)nz + n + T] = -suhi;
    if (io.gzmin != nullptr) io.gzmin[r * (size_t)nz + n + T] = sulo;
  }
  if (T != 0) return;
  if (io.J != nullptr) io.J[r] = Jr;
  if (io.LA != nullptr) io.LA[r] = (Jr + Pen) + Soc / (2.0 * mu);
}

}  // namespace altro
