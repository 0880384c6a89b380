// pn_wide.h -- the projected-Newton polish on the one-wave-per-instance backend (any n <= 64, m <= 32, per-knot dynamics, up
// to 64 generic rows): a VIEW of that backend's layouts for the algorithm in pn_core.h, with its parameter struct and kernel.
//
// A block of 64 threads owns one WORKSPACE SLOT and walks the instances slot, slot + nslots, ...; every matrix block lives
// in HBM (a block row of S = D H^-1 D' has up to 2 n + active rows = ~200 entries at n = 64: two such blocks do not fit LDS),
// so a triangular solve reads the knot's diagonal block in place.  Data is read in the backend's own layouts (solve_wide.h
// Params): X [B][2][N][n], U [B][2][N-1][m], column-major dynamics blocks, the transposed row table AconT.  A z-vector has
// stride n + m: no pad columns.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/altro_batch.h"
#include "pn_core.h"
#include "solve_wide.h"

namespace altro_pnw {

constexpr int ZMAX = 96;  // n + m <= 64 + 32

struct WParams {
  altro_wide::Params P;    // P.o: the caller's options (params() carries the AL stage's tolerance); P.active: the instances to polish
  altro_pn::PnOut out;
  altro_pn::PnWork ws;     // one set per slot; ws.blk holds the block in work
};

struct WideView {
  static constexpr int ZCAP = ZMAX;
  const altro_wide::Params& P;
  size_t inst = 0;
  int N, n, m, nz, zs, ld, kref = 0;
  const double *wd_, *wf_, *zmin_, *zmax_;  // this instance's row of the cost weights and of the bounds (Params::w_pi, b_pi)
  double *Lc, *Lp, *vv;                     // HBM: two blocks [bm][ld], vectors [4][bm]

  __device__ WideView(const WParams& w) : P(w.P) {
    N = P.N; n = P.n; m = P.m; nz = n + m; zs = nz; ld = w.ws.bm + 1;
    const size_t bm = w.ws.bm;
    double* b = w.ws.blk + blockIdx.x * (2 * bm * ld + 4 * bm);
    Lc = b; Lp = b + bm * ld; vv = b + 2 * bm * ld;
  }
  __device__ __forceinline__ void bind(int i) {
    inst = (size_t)i;
    kref = P.clk.start != nullptr ? P.clk.window[i] : P.kref;   // altro_mpc_set_clock: the instance's own window
    wd_ = P.wd + inst * P.w_pi * nz; wf_ = P.wf + inst * P.w_pi * n;
    zmin_ = P.zmin + inst * P.b_pi * nz; zmax_ = P.zmax + inst * P.b_pi * nz;
  }

  __device__ __forceinline__ double zget(int pl, int k, int j) const {
    if (j < n) return P.X[((inst * 2 + pl) * N + k) * n + j];
    return (k < N - 1) ? P.U[((inst * 2 + pl) * (N - 1) + k) * m + (j - n)] : 0.0;
  }
  __device__ __forceinline__ void zset(int pl, int k, int j, double v) const {   // (dead entries are not stored)
    if (j < n) P.X[((inst * 2 + pl) * N + k) * n + j] = v;
    else if (k < N - 1) P.U[((inst * 2 + pl) * (N - 1) + k) * m + (j - n)] = v;
  }
  __device__ __forceinline__ void load_z(int pl, int k, double* z) const {
    for (int j = 0; j < nz; ++j) z[j] = zget(pl, k, j);
  }
  __device__ __forceinline__ double zref(int k, int j) const {
    if (j < n) return P.Xref[(inst * P.Nt + (kref + k)) * n + j];
    return (k < N - 1) ? P.Uref[(inst * (P.Nt - 1) + (kref + k)) * m + (j - n)] : 0.0;
  }
  __device__ __forceinline__ double x0(int i) const { return P.x0[inst * n + i]; }
  __device__ __forceinline__ double hdiag(int k, int j) const { return (k < N - 1) ? wd_[j] : (j < n ? wf_[j] : 0.0); }
  __device__ __forceinline__ size_t dynblk(int k) const {
    return (P.dyn_per_instance ? inst : 0) * (P.ltv ? P.dyn_blocks : 1) + (P.ltv ? (size_t)kref * P.dyn_step_stride + k : 0);
  }
  __device__ __forceinline__ double G(int k, int i, int c) const {   // [A_k B_k][i][c]
    return c < n ? P.A[dynblk(k) * n * n + i + (size_t)n * c] : P.Bm[dynblk(k) * n * m + i + (size_t)n * (c - n)];
  }
  __device__ __forceinline__ double fdyn(int k, int i) const { return P.f[dynblk(k) * n + i]; }
  __device__ __forceinline__ double lo(int j) const { return zmin_[j]; }
  __device__ __forceinline__ double hi(int j) const { return zmax_[j]; }

  // generic rows: P.Pn rows, their knot ranges and cones (first row, size) per row, their type per knot
  __device__ __forceinline__ int nrows() const { return P.Pn; }
  __device__ __forceinline__ int ctype(int k, int r) const { return P.ctype[(size_t)k * P.Pn + r]; }
  __device__ __forceinline__ int cone_size(int, int r) const { return P.rowcp[r]; }
  __device__ __forceinline__ int row_kind(int k, int r) const {
    const int t = ctype(k, r);
    if (t == 0 || k < P.rowk0[r] || k > P.rowk1[r]) return 0;
    return (t == 3 && P.rowc0[r] != r) ? 0 : t;
  }
  __device__ __forceinline__ double arow(int k, int r, int j) const {   // row r of knot k's table, column j
    return P.AconT[inst * P.con_istride + ((size_t)k * nz + j) * P.Pn + r];
  }
  __device__ __forceinline__ double brow(int k, int r) const { return P.bcon[inst * P.bcon_istride + (size_t)k * P.Pn + r]; }
  __device__ __forceinline__ double dual(int code, int k) const {
    if (code >= 256) return P.Lc[(inst * N + k) * P.Pn + (code - 256)];
    return P.Lb[((inst * N + k) * 2 + (code >> 7)) * nz + (code & 127)];
  }

  __device__ __forceinline__ altro_pn::DiagBlock diag_block(const double* Lk, int bm, int, int) const { return {Lk, bm}; }
};

__global__ void __launch_bounds__(64) pnw_kernel(WParams w) {
  WideView v(w);
  altro_pn::PnCore<WideView> s(v, w.ws, w.out, w.P.o);
  for (int inst = blockIdx.x; inst < w.P.B; inst += gridDim.x) {
    if (w.P.active != nullptr && w.P.active[inst] == 0) continue;  // block-uniform: not polished, its statistics stay
    s.run(inst);
    __syncthreads();
  }
}

}  // namespace altro_pnw
