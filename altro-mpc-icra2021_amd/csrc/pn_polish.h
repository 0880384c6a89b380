// pn_polish.h -- the projected-Newton polish on the 16-lane backend: a VIEW of that backend's layouts for the algorithm in
// pn_core.h, with its parameter struct and kernel.  One block of 64 threads per instance; the trajectory, the reference and
// the tables are rows of 16 (LW), so a z-vector has stride 16 and its pad columns are written as zeros -- the solve kernel
// reads the rows of Z afterwards.  The block in work and the previous knot's factor sit in static LDS; a triangular solve
// first copies the knot's diagonal block there.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/altro_batch.h"
#include "pn_core.h"

namespace altro_pn {

constexpr int LW = 16;
constexpr int BMAX = 56;  // rows a block may hold (2 n + active box sides + generic rows), checked on the host

struct PnParams {
  int B, Bp, N, n, m;
  int Nt;                 // rows per instance of Zref
  int box_k0, box_k1, ncrows;
  unsigned con_istride;   // as SolveParams
  const double *Grow, *fvec, *wd, *wf, *zmin, *zmax, *x0;
  unsigned wstride, bstride;  // rows of wd / wf and of zmin / zmax: 0 (one row [16] for the batch) or 16 ([Bp][16] per instance)
  const double *Acon, *bcon;
  const int* cmeta;
  const int* active;      // [Bp] 0 / 1 per instance (altro_batch_set_active), or null: all.  An inactive instance is not polished
                          // and keeps its polish statistics
  double* Z;              // [Bp][2 N + 1][16] (two planes of N rows + trash row per instance): plane cur is polished, plane cur^1 is the trial buffer
  const double* Zref;     // window start kref
  int kref;
  const int* win;         // [Bp] per-instance window start (altro_mpc_set_clock), or null: kref for every instance
  int* cur;
  int* status;
  double *cost, *cmax;
  // multiplier projection (the dual half of the polish): the AL duals
  const double *Lb, *Lc;   // [Bp][N+1][2][nbp], [Bp][N+1][16]
  const int* bslot;        // [16]
  int nbp;
  PnOut out;
  PnWork ws;               // one set per instance (the grid is one block per instance); ws.blk is not used
  altro_opts o;
};

struct LaneView {
  static constexpr int zs = LW, ZCAP = LW, ld = BMAX + 1;
  const PnParams& P;
  size_t inst = 0;
  int N, n, nz, kref = 0;
  const double *wd_, *wf_, *zmin_, *zmax_;  // this instance's row of the cost weights and of the bounds
  double *Lc, *Lp, *vv;                     // LDS: two blocks [BMAX][ld], vectors [4][BMAX]

  __device__ LaneView(const PnParams& p, double* lds) : P(p) {
    N = P.N; n = P.n; nz = n + P.m;
    Lc = lds;
    Lp = lds + BMAX * ld;
    vv = lds + 2 * BMAX * ld;
  }
  __device__ __forceinline__ void bind(int i) {
    inst = (size_t)i;
    kref = P.win != nullptr ? P.win[i] : P.kref;
    wd_ = P.wd + inst * P.wstride; wf_ = P.wf + inst * P.wstride;
    zmin_ = P.zmin + inst * P.bstride; zmax_ = P.zmax + inst * P.bstride;
  }

  __device__ __forceinline__ double* zrow(int plane, int k) const {
    return P.Z + (inst * (2 * (size_t)N + 1) + (size_t)plane * N + k) * LW;
  }
  __device__ __forceinline__ double zget(int pl, int k, int j) const { return zrow(pl, k)[j]; }
  __device__ __forceinline__ void zset(int pl, int k, int j, double v) const { zrow(pl, k)[j] = v; }
  __device__ __forceinline__ void load_z(int pl, int k, double* z) const {
    const double* zr = zrow(pl, k);
    for (int j = 0; j < LW; ++j) z[j] = (j < n || (j < nz && k < N - 1)) ? zr[j] : 0.0;
  }
  __device__ __forceinline__ double zref(int k, int j) const { return P.Zref[(inst * P.Nt + (size_t)(kref + k)) * LW + j]; }
  __device__ __forceinline__ double x0(int i) const { return P.x0[inst * LW + i]; }
  __device__ __forceinline__ double hdiag(int k, int j) const { return (k < N - 1) ? wd_[j] : (j < n ? wf_[j] : 0.0); }
  __device__ __forceinline__ double G(int, int i, int c) const { return P.Grow[(inst * LW + c) * LW + i]; }  // [A B][i][c]
  __device__ __forceinline__ double fdyn(int, int i) const { return P.fvec[inst * LW + i]; }
  __device__ __forceinline__ double lo(int j) const { return zmin_[j]; }
  __device__ __forceinline__ double hi(int j) const { return zmax_[j]; }

  // generic rows: the 16 constraint lanes, cmeta[k][lane] = (type, first knot, last knot, cone size); a cone sits on its first lane
  __device__ __forceinline__ int nrows() const { return P.ncrows > 0 ? LW : 0; }
  __device__ __forceinline__ int ctype(int k, int r) const { return P.cmeta[((size_t)k * LW + r) * 4]; }
  __device__ __forceinline__ int cone_size(int k, int r) const { return P.cmeta[((size_t)k * LW + r) * 4 + 3]; }
  __device__ __forceinline__ int row_kind(int k, int r) const {
    const int* cm = P.cmeta + ((size_t)k * LW + r) * 4;
    if (cm[0] == 0 || k < cm[1] || k > cm[2]) return 0;
    return (cm[0] == 3 && (r & 3) != 0) ? 0 : cm[0];
  }
  __device__ __forceinline__ double arow(int k, int r, int j) const {
    return P.Acon[inst * P.con_istride + ((size_t)k * LW) * LW + (size_t)r * LW + j];
  }
  __device__ __forceinline__ double brow(int k, int r) const { return P.bcon[inst * (P.con_istride / LW) + (size_t)k * LW + r]; }
  __device__ __forceinline__ double dual(int code, int k) const {   // compact box duals through bslot; linear rows by lane
    if (code >= 256) return P.Lc[(inst * (N + 1) + k) * LW + (code - 256)];
    const int sl = P.bslot[code & 127];
    return sl >= 0 ? P.Lb[((inst * (N + 1) + k) * 2 + (code >> 7)) * P.nbp + sl] : 0.0;
  }

  __device__ __forceinline__ DiagBlock diag_block(const double* Lk, int bm, int b, int tid) const {   // (the caller's next barrier covers the copy)
    for (int e = tid; e < b * b; e += 64) Lc[(e / b) * ld + (e % b)] = Lk[(size_t)(e / b) * bm + (e % b)];
    return {Lc, ld};
  }
};

__global__ void __launch_bounds__(64) pn_kernel(PnParams p) {
  __shared__ double lds[2 * BMAX * (BMAX + 1) + 4 * BMAX];
  if (p.active != nullptr && p.active[blockIdx.x] == 0) return;  // block-uniform, before any barrier
  LaneView v(p, lds);
  PnCore<LaneView> s(v, p.ws, p.out, p.o);
  s.run(blockIdx.x);
}

}  // namespace altro_pn
