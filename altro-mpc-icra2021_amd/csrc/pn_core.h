// pn_core.h -- projected-Newton polish (Altro.jl solve!(::ProjectedNewtonSolver); ALTRO, IROS 2019, Algorithm 4): THE
// ALGORITHM, once, for both backends.  pn_polish.h (16-lane backend) and pn_wide.h (one wave per instance)
// are VIEWS: how a backend stores the problem and where the block in work lives; each adds its parameter struct and kernel.
// Restated in oracle/altro_oracle.c (projected_newton, multiplier_projection), which is this file's parity oracle.
// PARITY WITH Altro.jl IS UNPINNED: the reference stores no trajectory a polish produced (it is off in every live script,
// and skipped in the one old script that leaves it on).
//
// After the AL stage has stopped at projected_newton_tolerance, the primal trajectory z = (x_0, u_0, ..., x_{N-1}) is
// projected onto d(z) = 0 -- the initial condition, the dynamics defects and the ACTIVE rows of the constraints
// (equalities; inequality rows with c >= -active_set_tolerance_pn; a second-order cone through h = ||v|| - t) -- in the
// metric of the cost Hessian (diagonal here):
//     dz = -H^-1 D' (D H^-1 D')^-1 d
// S = D H^-1 D' is block tridiagonal over the knots (block k: [x_0 - x0 if k = 0; active stage rows; defect k]); it is
// factored as S + rho_chol I = L L' block by block and the solve is refined against S (Altro's reg_solve).  Then the
// multipliers are projected the same way under H = I (multiplier_projection).
//
// Mapping: ONE wave (a block of 64 threads) works on one instance at a time.  The serial structure is knot after knot (the
// block recursion); inside a knot the 64 lanes share the rows / entries of the blocks.  The blocks of L stay in HBM.  This
// is a correctness-first kernel: the polish runs once per solve, on the instances whose AL stage ended above
// constraint_tolerance, and is not on the MPC hot path (projected_newton = false in every MPC script of the reference).
//
// Every routine here and in the views is __forceinline__, so a kernel is ONE function and each pointer keeps the address space
// it has in the kernel's arguments (global loads and stores, LDS instructions).  Left to its cost model the compiler moves
// linearise, reg_solve or multiplier_projection out of line; the core object then lives in memory and every access through it
// becomes a flat one.
//
// What PnCore<View> asks of a view V:
//   V.P                      the backend's parameter block; the core reads N, n, m, box_k0, box_k1 and cur, status, cost, cmax
//   V.zs, V.ZCAP             stride of a z-vector in E / tz / gz / rz and in the element loops; size of a local z buffer.
//                            Where zs > n + m the core writes zeros into the pad columns
//   V.bind(inst)             the instance in work from here on (its window start, its rows of the weights and bounds)
//   V.load_z(pl, k, z)       knot k of plane pl, dead entries (controls of the last knot) and pads as 0
//   V.zget / V.zset          one element of the trajectory; zset may ignore dead entries, zget need not mask them
//   V.zref, V.x0, V.hdiag    reference, initial state, diagonal of the cost Hessian
//   V.G(k, i, c), V.fdyn     [A_k B_k][i][c] and the affine term of the dynamics
//   V.lo(j), V.hi(j)         the instance's box bounds (a side is finite below 1e300 in magnitude)
//   V.nrows(), V.ctype(k, r), V.row_kind(k, r), V.cone_size(k, r), V.arow(k, r, j), V.brow(k, r)
//                            the generic rows, walked in ascending order: ctype is the stored type (1 equality, 2 inequality,
//                            3 cone); row_kind is that type where the row is live at knot k -- a cone only on its first row
//                            -- and 0 elsewhere
//   V.dual(code, k)          the AL dual of a box side or of a linear row (row codes: pn_row)
//   V.Lc, V.Lp, V.vv, V.ld   the block in work, the previous knot's factor and four vectors, row stride ld
//   V.diag_block(Lk, bm, b, tid)   the factored diagonal block of a knot for a triangular solve, from its home Lk in HBM
//                            ([bm][bm], b rows used): in place, or copied next to the wave first
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/altro_batch.h"
#include "device_pool.h"

namespace altro_pn {

// The workspace of the polish: one set per BLOCK of the launch (blockIdx.x), whatever instance the block works on.  Embedded
// by value in the backend that owns it and in its kernel's parameter struct.
struct PnWork {
  double *E = nullptr, *dv = nullptr, *Ld = nullptr, *Lo = nullptr, *vec = nullptr;  // E [N][bm][zs]; dv [N][bm]; Ld, Lo [N][bm][bm];
                                                                                   // vec [6][N][bm] (lam, res, cor, Sv, dtrial, spare)
  double* tz = nullptr;                            // [3][N][zs]: t of apply_S; the cost gradient g; g + D' lam
  double* blk = nullptr;                           // [2][bm][bm+1] + [4][bm]: Lc, Lp, vv of a view that keeps them in HBM
  int *nb = nullptr, *nst = nullptr, *rinfo = nullptr;   // [N], [N], [N][bm] (row code: see pn_row)
  int bm = 0, slots = 0;                           // rows a block may hold; sets allocated.  Both 0 until every array exists

  // Host.  (Re)allocate for `slots_` blocks when the shape changed or an array is missing.  Call it before
  // the launch takes its slot of the timing ring: it is everything about the workspace that can fail.
  hipError_t alloc(altro::DevicePool& pool, hipStream_t st, int slots_, size_t N, int bm_, size_t zs, bool with_blk) {
    if (bm_ == bm && slots_ == slots && E) return hipSuccess;
    bm = slots = 0;
    const size_t S = slots_, b = bm_;
    hipError_t e = hipSuccess;
    auto A = [&](auto** p, size_t count) { if (e == hipSuccess) e = pool.alloc(p, count, st, false); };
    A(&E, S * N * b * zs); A(&dv, S * N * b); A(&Ld, S * N * b * b); A(&Lo, S * N * b * b); A(&vec, S * 6 * N * b);
    A(&tz, S * 3 * N * zs);
    if (with_blk) A(&blk, S * (2 * b * (b + 1) + 4 * b));
    A(&nb, S * N); A(&nst, S * N); A(&rinfo, S * N * b);
    if (e == hipSuccess) { bm = bm_; slots = slots_; }
    return e;
  }
};

// What the polish reports per instance: [B] each.  Embedded like PnWork.
struct PnOut {
  int *ran = nullptr, *failed = nullptr, *dfail = nullptr;
  double *res = nullptr, *dres0 = nullptr, *dres = nullptr;   // max |d| left; ||g + D' lam||_2 with the AL duals / the projected multipliers

  // Host: the body of both getters on both backends.  Synchronises, then copies B elements of every array asked for -- zeros
  // when there is nothing to report (have = false: projected_newton off, or no polish has allocated the arrays yet).
  hipError_t read(hipStream_t st, bool have, size_t B, int32_t* ran_, int32_t* failed_, double* res_, double* dres0_, double* dres_,
                  int32_t* dfail_) const {
    hipError_t e = hipStreamSynchronize(st);
    auto one = [&](auto* host, const auto* dev) {
      if (!host || e != hipSuccess) return;
      if (have) e = hipMemcpy(host, dev, B * sizeof(*host), hipMemcpyDeviceToHost);
      else std::memset(host, 0, B * sizeof(*host));
    };
    one(ran_, ran); one(failed_, failed); one(res_, res); one(dres0_, dres0); one(dres_, dres); one(dfail_, dfail);
    return e;
  }
};

__device__ __forceinline__ double wave_max(double v) {
  for (int s = 32; s >= 1; s >>= 1) v = fmax(v, __shfl_xor(v, s, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

struct DiagBlock {
  const double* p;
  int ld;
};

template <class View>
struct PnCore {
  View& V;
  const PnOut& R;
  const altro_opts& o;   // the caller's options: constraint_tolerance is the polish's
  int inst = 0, tid, N, n, nz, bm;
  double *E, *dv, *Ld, *Lo, *lam, *res, *cor, *Sv, *dtr, *spare, *tz, *gz, *rz;
  int *nb, *nst, *rinfo;
  bool unit = false;   // the metric H = I of the multiplier projection (D D' instead of D H^-1 D')

  __device__ PnCore(View& v, const PnWork& W, const PnOut& r, const altro_opts& opts) : V(v), R(r), o(opts) {
    tid = threadIdx.x;
    N = V.P.N; n = V.P.n; nz = n + V.P.m; bm = W.bm;
    const size_t s = blockIdx.x;
    E = W.E + s * N * bm * V.zs;
    dv = W.dv + s * N * bm;
    Ld = W.Ld + s * N * bm * bm;
    Lo = W.Lo + s * N * bm * bm;
    double* w = W.vec + s * 6 * N * bm;
    lam = w; res = w + (size_t)N * bm; cor = w + 2 * (size_t)N * bm; Sv = w + 3 * (size_t)N * bm; dtr = w + 4 * (size_t)N * bm;
    spare = w + 5 * (size_t)N * bm;
    tz = W.tz + s * 3 * N * V.zs;
    gz = tz + (size_t)N * V.zs;
    rz = tz + 2 * (size_t)N * V.zs;
    nb = W.nb + s * N; nst = W.nst + s * N; rinfo = W.rinfo + s * N * bm;
  }

  __device__ __forceinline__ double hinv(int k, int j) const { return unit ? 1.0 : 1.0 / (V.hdiag(k, j) + o.rho_primal); }
  __device__ __forceinline__ bool live(int k, int j) const { return j < n || (j < nz && k < N - 1); }

  // Stage rows of knot k are coded as: code < 256: box side (upper: j, lower: 128 + j); 256 + r: generic row r (a cone by
  // its first row).  The codes live in rinfo only.  Value of row `code` at z (and its Jacobian row).
  __device__ __forceinline__ double pn_row(int code, int k, const double* z, double* Erow) const {
    const bool term = k == N - 1;
    const int ncol = term ? n : nz;
    if (Erow) for (int j = 0; j < V.zs; ++j) Erow[j] = 0.0;
    if (code < 256) {
      const int j = code & 127;
      if (code < 128) { if (Erow) Erow[j] = 1.0; return z[j] - V.hi(j); }
      if (Erow) Erow[j] = -1.0;
      return V.lo(j) - z[j];
    }
    const int r0 = code - 256;
    auto val = [&](int r) {
      double acc = V.brow(k, r);
      for (int j = 0; j < ncol; ++j) acc += V.arow(k, r, j) * z[j];
      return acc;
    };
    if (V.ctype(k, r0) != 3) {
      if (Erow) for (int j = 0; j < ncol; ++j) Erow[j] = V.arow(k, r0, j);
      return val(r0);
    }
    const int p = V.cone_size(k, r0), q = p - 1;
    double v[4], nv = 0.0;
    for (int r = 0; r < p; ++r) v[r] = val(r0 + r);
    for (int r = 0; r < q; ++r) nv += v[r] * v[r];
    nv = sqrt(nv);
    if (Erow) {
      for (int j = 0; j < ncol; ++j) {
        double g = -V.arow(k, r0 + q, j);
        if (nv > 0.0) for (int r = 0; r < q; ++r) g += v[r] / nv * V.arow(k, r0 + r, j);
        Erow[j] = g;
      }
    }
    return nv - v[q];
  }

  // active set + linearisation of knot k at plane pl (one thread per knot); returns max |d| of the knot
  __device__ __forceinline__ double linearise_knot(int k, int pl) {
    const double tol = o.active_set_tolerance_pn;
    double z[View::ZCAP];
    V.load_z(pl, k, z);
    double* Ek = E + (size_t)k * bm * V.zs;
    double* dk = dv + (size_t)k * bm;
    int* ri = rinfo + (size_t)k * bm;
    int r = 0;
    if (k == 0) {
      for (int i = 0; i < n; ++i) {
        for (int j = 0; j < V.zs; ++j) Ek[(size_t)r * V.zs + j] = (j == i) ? 1.0 : 0.0;
        dk[r] = z[i] - V.x0(i);
        ++r;
      }
    }
    int ns = 0;
    auto stage_row = [&](int code, bool always) {   // into the block if active and there is room
      const double v = pn_row(code, k, z, nullptr);
      if (!(always || v >= -tol) || r >= bm - n) return;
      dk[r] = pn_row(code, k, z, Ek + (size_t)r * V.zs);
      ri[ns++] = code;
      ++r;
    };
    if (k >= V.P.box_k0 && k <= V.P.box_k1) {
      const int lim = (k == N - 1) ? n : nz;
      for (int side = 0; side < 2; ++side)
        for (int j = 0; j < lim; ++j) {
          const bool has = side == 0 ? (V.hi(j) < 1e300) : (V.lo(j) > -1e300);
          if (has) stage_row(side * 128 + j, false);
        }
    }
    for (int q = 0; q < V.nrows(); ++q) {
      const int t = V.row_kind(k, q);
      if (t != 0) stage_row(256 + q, t == 1);
    }
    nst[k] = ns;
    if (k < N - 1) {
      for (int i = 0; i < n; ++i) {
        double acc = V.fdyn(k, i);
        for (int c = 0; c < nz; ++c) {
          const double g = V.G(k, i, c);
          Ek[(size_t)r * V.zs + c] = g;
          acc += g * z[c];
        }
        for (int c = nz; c < V.zs; ++c) Ek[(size_t)r * V.zs + c] = 0.0;
        dk[r] = acc - V.zget(pl, k + 1, i);
        ++r;
      }
    }
    nb[k] = r;
    double mx = 0.0;
    for (int q = 0; q < r; ++q) mx = fmax(mx, fabs(dk[q]));
    return mx;
  }

  __device__ __forceinline__ double linearise(int pl) {
    double mx = 0.0;
    for (int k = tid; k < N; k += 64) mx = fmax(mx, linearise_knot(k, pl));
    __syncthreads();
    return wave_max(mx);
  }

  // values of the same rows at plane pl into out; returns max |d|
  __device__ __forceinline__ double values(int pl, double* out) {
    double mx = 0.0;
    for (int k = tid; k < N; k += 64) {
      double z[View::ZCAP];
      V.load_z(pl, k, z);
      double* dk = out + (size_t)k * bm;
      int r = 0;
      if (k == 0) for (int i = 0; i < n; ++i) dk[r++] = z[i] - V.x0(i);
      for (int q = 0; q < nst[k]; ++q) dk[r++] = pn_row(rinfo[(size_t)k * bm + q], k, z, nullptr);
      if (k < N - 1) {
        for (int i = 0; i < n; ++i) {
          double acc = V.fdyn(k, i);
          for (int c = 0; c < nz; ++c) acc += V.G(k, i, c) * z[c];
          dk[r++] = acc - V.zget(pl, k + 1, i);
        }
      }
      for (int q = 0; q < r; ++q) mx = fmax(mx, fabs(dk[q]));
    }
    __syncthreads();
    return wave_max(mx);
  }

  // tz = H^-1 D' v: t_k = H_k^-1 (E_k' v_k - [defect part of v_{k-1}]_x), zeros in the pad columns
  __device__ __forceinline__ void apply_Dt(const double* v) {
    for (int e = tid; e < N * V.zs; e += 64) {
      const int k = e / V.zs, j = e % V.zs;
      double acc = 0.0;
      if (j < nz) {
        const double* Ek = E + (size_t)k * bm * V.zs;
        for (int r = 0; r < nb[k]; ++r) acc += Ek[(size_t)r * V.zs + j] * v[(size_t)k * bm + r];
        if (k > 0 && j < n) acc -= v[(size_t)(k - 1) * bm + nb[k - 1] - n + j];
        acc *= hinv(k, j);
      }
      tz[e] = acc;
    }
    __syncthreads();
  }
  // y = D t   (t: [N][zs])
  __device__ __forceinline__ void apply_D(const double* t, double* y) {
    for (int e = tid; e < N * bm; e += 64) {
      const int k = e / bm, r = e % bm;
      if (r >= nb[k]) continue;
      const double* Ek = E + (size_t)k * bm * V.zs;
      double acc = 0.0;
      for (int j = 0; j < nz; ++j) acc += Ek[(size_t)r * V.zs + j] * t[(size_t)k * V.zs + j];
      const int off = nb[k] - n;
      if (k < N - 1 && r >= off) acc -= t[(size_t)(k + 1) * V.zs + (r - off)];
      y[e] = acc;
    }
    __syncthreads();
  }
  // y = S v; also leaves H^-1 D' v in tz
  __device__ __forceinline__ void apply_S(const double* v, double* y) {
    apply_Dt(v);
    apply_D(tz, y);
  }

  // S + rho_chol I = L L', block by block.  Returns false if a pivot is not positive.
  __device__ __forceinline__ bool factor() {
    double *Lc = V.Lc, *Lp = V.Lp;
    bool ok = true;
    for (int k = 0; k < N; ++k) {
      const int b = nb[k];
      const double* Ek = E + (size_t)k * bm * V.zs;
      // S_kk into Lc
      for (int e = tid; e < b * b; e += 64) {
        const int r = e / b, c = e % b;
        double acc = 0.0;
        if (c <= r) {
          for (int j = 0; j < nz; ++j) acc += Ek[(size_t)r * V.zs + j] * hinv(k, j) * Ek[(size_t)c * V.zs + j];
          if (k < N - 1 && r == c && r >= b - n) acc += hinv(k + 1, r - (b - n));
          if (r == c) acc += o.rho_chol;
        }
        Lc[r * V.ld + c] = acc;
      }
      __syncthreads();
      if (k > 0) {
        // L_{k,k-1} = S_{k,k-1} L_{k-1,k-1}^-T, row r per thread; Lp holds L_{k-1,k-1}
        const int pb = nb[k - 1], poff = pb - n;
        for (int r = tid; r < b; r += 64) {
          double* lo = Lo + (size_t)k * bm * bm + (size_t)r * bm;
          for (int c = 0; c < pb; ++c) {
            double v = (c >= poff) ? -Ek[(size_t)r * V.zs + (c - poff)] * hinv(k, c - poff) : 0.0;
            for (int q = 0; q < c; ++q) v -= lo[q] * Lp[c * V.ld + q];
            lo[c] = v / Lp[c * V.ld + c];
          }
        }
        __syncthreads();
        for (int e = tid; e < b * b; e += 64) {
          const int r = e / b, c = e % b;
          if (c > r) continue;
          const double* lr = Lo + (size_t)k * bm * bm + (size_t)r * bm;
          const double* lc = Lo + (size_t)k * bm * bm + (size_t)c * bm;
          double acc = 0.0;
          for (int q = 0; q < pb; ++q) acc += lr[q] * lc[q];
          Lc[r * V.ld + c] -= acc;
        }
        __syncthreads();
      }
      // Cholesky of the block in work, column by column
      for (int c = 0; c < b; ++c) {
        double dd = Lc[c * V.ld + c];
        for (int q = 0; q < c; ++q) dd -= Lc[c * V.ld + q] * Lc[c * V.ld + q];
        ok = ok && (dd > 0.0);
        const double piv = sqrt(dd > 0.0 ? dd : 1.0);
        __syncthreads();
        for (int r = c + 1 + tid; r < b; r += 64) {
          double v = Lc[r * V.ld + c];
          for (int q = 0; q < c; ++q) v -= Lc[r * V.ld + q] * Lc[c * V.ld + q];
          Lc[r * V.ld + c] = v / piv;
        }
        if (tid == 0) Lc[c * V.ld + c] = piv;
        __syncthreads();
      }
      for (int e = tid; e < b * b; e += 64) {
        const int r = e / b, c = e % b;
        Ld[(size_t)k * bm * bm + (size_t)r * bm + c] = (c <= r) ? Lc[r * V.ld + c] : 0.0;
        Lp[r * V.ld + c] = Lc[r * V.ld + c];
      }
      __syncthreads();
    }
    return ok;
  }

  // x = (L L')^-1 b
  __device__ __forceinline__ void chol_solve(const double* bvec, double* x) {
    double* vv = V.vv;
    for (int k = 0; k < N; ++k) {  // forward
      const int b = nb[k];
      const DiagBlock L = V.diag_block(Ld + (size_t)k * bm * bm, bm, b, tid);
      for (int r = tid; r < b; r += 64) {
        double v = bvec[(size_t)k * bm + r];
        if (k > 0) {
          const double* lo = Lo + (size_t)k * bm * bm + (size_t)r * bm;
          for (int q = 0; q < nb[k - 1]; ++q) v -= lo[q] * x[(size_t)(k - 1) * bm + q];
        }
        vv[r] = v;
      }
      __syncthreads();
      for (int c = 0; c < b; ++c) {
        const double xc = vv[c] / L.p[c * L.ld + c];
        __syncthreads();
        for (int r = c + 1 + tid; r < b; r += 64) vv[r] -= L.p[r * L.ld + c] * xc;
        if (tid == 0) vv[c] = xc;
        __syncthreads();
      }
      for (int r = tid; r < b; r += 64) x[(size_t)k * bm + r] = vv[r];
      __syncthreads();
    }
    for (int k = N - 1; k >= 0; --k) {  // backward
      const int b = nb[k];
      const DiagBlock L = V.diag_block(Ld + (size_t)k * bm * bm, bm, b, tid);
      for (int r = tid; r < b; r += 64) {
        double v = x[(size_t)k * bm + r];
        if (k < N - 1) {
          const double* ln = Lo + (size_t)(k + 1) * bm * bm;
          for (int q = 0; q < nb[k + 1]; ++q) v -= ln[(size_t)q * bm + r] * x[(size_t)(k + 1) * bm + q];
        }
        vv[r] = v;
      }
      __syncthreads();
      for (int c = b - 1; c >= 0; --c) {
        const double xc = vv[c] / L.p[c * L.ld + c];
        __syncthreads();
        for (int r = tid; r < c; r += 64) vv[r] -= L.p[c * L.ld + r] * xc;
        if (tid == 0) vv[c] = xc;
        __syncthreads();
      }
      for (int r = tid; r < b; r += 64) x[(size_t)k * bm + r] = vv[r];
      __syncthreads();
    }
  }

  // reg_solve: A x = rhs with the factors of A + rho I, refined against A (apply_S under the metric in force)
  __device__ __forceinline__ void reg_solve(const double* rhs, double* x) {
    chol_solve(rhs, x);
    for (int it = 0; it < 25; ++it) {
      apply_S(x, Sv);
      double rn = 0.0;
      for (int e = tid; e < N * bm; e += 64) {
        const double v = ((e % bm) < nb[e / bm]) ? rhs[e] - Sv[e] : 0.0;
        res[e] = v;
        rn = fmax(rn, fabs(v));
      }
      __syncthreads();
      rn = wave_max(rn);
      if (rn < 1e-8) break;
      chol_solve(res, spare);
      for (int e = tid; e < N * bm; e += 64)
        if ((e % bm) < nb[e / bm]) x[e] += spare[e];
      __syncthreads();
    }
  }

  // multiplier_projection! of Altro.jl's ProjectedNewtonSolver (oracle multiplier_projection): lam <- lam - (D D')^-1 D (g + D' lam)
  // at the polished trajectory, with the stationarity residual before and after.  The multipliers are not written back.
  __device__ __forceinline__ void multiplier_projection(int cur) {
    linearise(cur);
    unit = true;
    for (int e = tid; e < N * bm; e += 64) lam[e] = 0.0;
    for (int e = tid; e < N * V.zs; e += 64) {   // g_k = H_k (z_k - zref_k)
      const int k = e / V.zs, j = e % V.zs;
      gz[e] = live(k, j) ? V.hdiag(k, j) * (V.zget(cur, k, j) - V.zref(k, j)) : 0.0;
    }
    __syncthreads();
    for (int k = tid; k < N; k += 64) {        // lam0: the AL duals of the active box / linear rows
      const int base = (k == 0) ? n : 0;
      for (int q = 0; q < nst[k]; ++q) {
        const int code = rinfo[(size_t)k * bm + q];
        double l0 = 0.0;
        if (code < 256 || V.ctype(k, code - 256) != 3) l0 = V.dual(code, k);
        lam[(size_t)k * bm + base + q] = l0;
      }
    }
    __syncthreads();
    apply_Dt(lam);
    double r0 = 0.0;
    for (int e = tid; e < N * V.zs; e += 64) {   // (pad columns hold 0 in gz and tz)
      const double v = gz[e] + tz[e];
      rz[e] = v;
      r0 += v * v;
    }
    __syncthreads();
    r0 = wave_sum(r0);
    const bool ok = factor();
    if (ok) {
      apply_D(rz, dtr);                        // rhs = D (g + D' lam0)
      reg_solve(dtr, cor);                     // against D D'
      for (int e = tid; e < N * bm; e += 64)
        if ((e % bm) < nb[e / bm]) lam[e] -= cor[e];
      __syncthreads();
    }
    apply_Dt(lam);
    double r1 = 0.0;
    for (int e = tid; e < N * V.zs; e += 64) {
      const double v = gz[e] + tz[e];
      r1 += v * v;
    }
    r1 = wave_sum(r1);
    unit = false;
    if (tid == 0) {
      R.dfail[inst] = ok ? 0 : 1;
      R.dres0[inst] = sqrt(r0);
      R.dres[inst] = sqrt(r1);
    }
  }

  __device__ __forceinline__ void run(int instance) {
    inst = instance;
    V.bind(inst);
    const double ctol = o.constraint_tolerance;
    const int cur = V.P.cur[inst];
    const bool need = (V.P.status[inst] <= ALTRO_SOLVE_SUCCEEDED) && (V.P.cmax[inst] > ctol);
    if (!need) {
      if (tid == 0) { R.ran[inst] = 0; R.failed[inst] = 0; R.res[inst] = 0.0; R.dfail[inst] = 0; R.dres0[inst] = 0.0; R.dres[inst] = 0.0; }
      return;
    }
    double viol = linearise(cur);
    bool failed = false;
    for (int outer = 0; outer <= 10 && viol > ctol; ++outer) {
      if (outer > 0) viol = linearise(cur);
      if (!factor()) { failed = true; break; }
      double viol_prev = viol;
      for (int refine = 0; refine < 10; ++refine) {
        reg_solve(dv, lam);
        apply_S(lam, Sv);  // tz = H^-1 D' lam: dz = -tz
        double alpha = 1.0, v_new = viol;
        for (int ls = 0;; ++ls) {
          for (int e = tid; e < N * V.zs; e += 64) {   // (0 into the pads and dead entries of a view that stores them)
            const int k = e / V.zs, j = e % V.zs;
            V.zset(cur ^ 1, k, j, live(k, j) ? V.zget(cur, k, j) - alpha * tz[e] : 0.0);
          }
          __syncthreads();
          v_new = values(cur ^ 1, dtr);
          if (v_new < viol || ls >= 10) break;
          alpha *= 0.5;
        }
        for (int e = tid; e < N * V.zs; e += 64) {
          const int k = e / V.zs, j = e % V.zs;
          V.zset(cur, k, j, live(k, j) ? V.zget(cur ^ 1, k, j) : 0.0);
        }
        for (int e = tid; e < N * bm; e += 64) dv[e] = dtr[e];
        __syncthreads();
        viol = v_new;
        const double rate = log10(viol) / log10(viol_prev);
        viol_prev = viol;
        if (viol < ctol) break;
        if (rate < o.r_threshold) break;
      }
    }
    if (!failed) multiplier_projection(cur);
    else if (tid == 0) { R.dfail[inst] = 1; R.dres0[inst] = 0.0; R.dres[inst] = 0.0; }
    __syncthreads();
    // objective (no AL terms) and violation of the problem's constraints at the polished trajectory
    double J = 0.0, cm = 0.0;
    for (int k = tid; k < N; k += 64) {
      const int lim = (k == N - 1) ? n : nz;
      double z[View::ZCAP];
      V.load_z(cur, k, z);
      for (int j = 0; j < lim; ++j) {
        const double e = z[j] - V.zref(k, j);
        J += 0.5 * V.hdiag(k, j) * e * e;
      }
      for (int j = lim; j < nz; ++j) z[j] = 0.0;
      if (k >= V.P.box_k0 && k <= V.P.box_k1)
        for (int j = 0; j < lim; ++j) {
          if (V.hi(j) < 1e300) cm = fmax(cm, z[j] - V.hi(j));
          if (V.lo(j) > -1e300) cm = fmax(cm, V.lo(j) - z[j]);
        }
      for (int q = 0; q < V.nrows(); ++q) {
        const int t = V.row_kind(k, q);
        if (t == 0) continue;
        if (t == 3) {   // violation of a cone: ||Proj(v) - v||_inf (oracle con_violation)
          const int p = V.cone_size(k, q), qq = p - 1;
          double v[4], nv = 0.0;
          for (int r = 0; r < p; ++r) {
            double acc = V.brow(k, q + r);
            for (int j = 0; j < lim; ++j) acc += V.arow(k, q + r, j) * z[j];
            v[r] = acc;
          }
          for (int r = 0; r < qq; ++r) nv += v[r] * v[r];
          nv = sqrt(nv);
          const double tt = v[qq];
          if (nv <= tt) continue;
          if (nv <= -tt) { for (int r = 0; r < p; ++r) cm = fmax(cm, fabs(v[r])); continue; }
          const double c = 0.5 * (1.0 + tt / nv);
          for (int r = 0; r < qq; ++r) cm = fmax(cm, fabs(c * v[r] - v[r]));
          cm = fmax(cm, fabs(c * nv - tt));
        } else {
          const double v = pn_row(256 + q, k, z, nullptr);
          cm = fmax(cm, t == 1 ? fabs(v) : fmax(v, 0.0));
        }
      }
    }
    J = wave_sum(J);
    cm = wave_max(cm);
    if (tid == 0) {
      R.ran[inst] = 1;
      R.failed[inst] = failed ? 1 : 0;
      R.res[inst] = viol;
      V.P.cost[inst] = J;
      V.P.cmax[inst] = cm;
      // (need: the AL stage left UNSOLVED or SOLVE_SUCCEEDED -- judged at ITS tolerance, projected_newton_tolerance.  A polish
      //  that failed or stopped above constraint_tolerance must not keep that SOLVE_SUCCEEDED: oracle orc_solve)
      V.P.status[inst] = cm < ctol ? ALTRO_SOLVE_SUCCEEDED : ALTRO_UNSOLVED;
    }
  }
};

}  // namespace altro_pn
