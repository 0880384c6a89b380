// wide_backend.h -- host side of the one-wave-per-instance kernel (solve_wide.h) behind the same
// C-ABI: altro_batch.hip forwards every entry point here when (n, m) is outside the 16-lane
// kernel set.  Device arrays use the ABI's own layouts, so transfers are plain copies.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/altro_batch.h"
#include "device_io.h"
#include "device_pool.h"
#include "evaluate.h"
#include "evaluate_grad.h"
#include "sensitivity.h"
#include "sensitivity_data.h"
#include "evaluate_al.h"
#include "warm_start.h"
#include "simulate.h"
#include "launch_ring.h"
#include "policy.h"
#include "solve_wide.h"
#include "covariance.h"
#include "cost_to_go.h"
#include "pn_wide.h"
#include "backend_common.h"

namespace altro_wide {

#define WCHK(call)                                                    \
  do {                                                                \
    hipError_t e_ = (call);                                           \
    if (e_ != hipSuccess) {                                           \
      err = std::string(#call) + ": " + hipGetErrorString(e_);        \
      return ALTRO_ERR_HIP;                                           \
    }                                                                 \
  } while (0)
#define WFAIL(code, msg) \
  do {                   \
    err = (msg);         \
    return (code);       \
  } while (0)

// Rows of box bounds given to altro_batch_set_bounds: no NaN, zmin <= zmax, and the finite sides of every row those of the BOX
// as it was added (lo_fin / hi_fin): the pattern fixes the dual layout, only the values may differ from row to row.
// Finite as the kernels test it: zmin > -1e300, zmax < 1e300.
static inline const char* check_bound_rows(const double* zmin, const double* zmax, size_t rows, int nz, const bool* lo_fin,
                                           const bool* hi_fin) {
  for (size_t r = 0; r < rows; ++r)
    for (int j = 0; j < nz; ++j) {
      const double lo = zmin[r * nz + j], hi = zmax[r * nz + j];
      if (std::isnan(lo) || std::isnan(hi)) return "altro_batch_set_bounds: NaN bound";
      if (lo > hi) return "altro_batch_set_bounds: zmin > zmax";
      if ((lo > -1e300) != lo_fin[j] || (hi < 1e300) != hi_fin[j])
        return "altro_batch_set_bounds: the finite sides differ from those the BOX constraint was added with";
    }
  return nullptr;
}

// dst[b][len] <- src[b][cur[b]][len]
__global__ void k_gather_plane(double* dst, const double* src, const int* cur, size_t len, int B) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * len) return;
  const size_t b = t / len, e = t - b * len;
  dst[t] = src[(b * 2 + cur[b]) * len + e];
}
// src[b][cur[b]][len] <- dst-layout host image
__global__ void k_scatter_plane(double* planes, const double* img, const int* cur, size_t len, int B) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * len) return;
  const size_t b = t / len, e = t - b * len;
  planes[(b * 2 + cur[b]) * len + e] = img[t];
}

// MPC log, projected_newton = 1 (the twin of altro_batch.hip's k_log_polished): after the polish kernel of a step's pair the
// step's records take the first control of the polished trajectory and the statistics the polish replaced where it ran.
__global__ void k_log_polished_wide(double* __restrict__ rec0, const double* __restrict__ U, const int* __restrict__ cur,
                                    const double* __restrict__ cost, const double* __restrict__ cmax, const int* __restrict__ status,
                                    const int* __restrict__ active, int B, int N, int n, int m) {
  const int inst = blockIdx.x * blockDim.x + threadIdx.x;
  if (inst >= B) return;
  if (active != nullptr && active[inst] == 0) return;  // the solve kernel wrote no record: the slot stays "never written"
  const size_t nv = (size_t)n + m;
  double* r = rec0 + (size_t)inst * (nv + altro::MLOG_TAIL);
  const double* u = U + ((size_t)inst * 2 + cur[inst]) * (size_t)(N - 1) * m;
  for (int a = 0; a < m; ++a) r[n + a] = u[a];
  r[nv] = cost[inst];
  r[nv + 1] = cmax[inst];
  reinterpret_cast<int*>(r + nv + 2)[2] = status[inst];
}

// The stored gains of every instance are no longer valid (a setter changed something they depend on) and the next launch is
// masked: the flag that says so is one per handle, and the launch clears it for the instances it runs only.  So the
// inactive instances lose their stored pass here, word 128 of their reuse state (solve_wide.h: bw_ok).
__global__ void k_drop_stored_pass(unsigned* __restrict__ bwst, int B) {
  const int inst = blockIdx.x * blockDim.x + threadIdx.x;
  if (inst < B) bwst[(size_t)inst * 136 + 128] = 0u;
}

// altro_batch_restart_instances on this backend (the twin of altro_batch.hip's k_restart): one block of 64 threads per
// instance; a selected instance takes rows `inst` of (X, U) into its current planes and goes back to what a freshly created
// handle holds -- zero duals, penalty 1.0, a zeroed reuse state (no stored pass, default roles of the active-set planes,
// which are cleared too) and the statistics of an instance that has not been solved.  The accumulating counters stay.
__global__ void __launch_bounds__(64) k_restart_wide(const int* __restrict__ which, const double* __restrict__ Xs, const double* __restrict__ Us,
                                                     Params P) {
  const int inst = blockIdx.x, T = threadIdx.x;
  if (which[inst] == 0) return;
  const size_t N = P.N, n = P.n, m = P.m, z = n + m, pl = (size_t)inst * 2 + P.cur[inst];
  if (Xs != nullptr)
    for (size_t e = T; e < N * n; e += 64) P.X[pl * N * n + e] = Xs[(size_t)inst * N * n + e];
  for (size_t e = T; e < (N - 1) * m; e += 64) P.U[pl * (N - 1) * m + e] = Us[(size_t)inst * (N - 1) * m + e];
  for (size_t e = T; e < N * 2 * z; e += 64) P.Lb[(size_t)inst * N * 2 * z + e] = 0.0;
  for (size_t e = T; e < N * (size_t)P.Pn; e += 64) P.Lc[(size_t)inst * N * P.Pn + e] = 0.0;
  for (size_t e = T; e < 136; e += 64) P.bwst[(size_t)inst * 136 + e] = 0u;
  for (size_t e = T; e < 3 * N * 64; e += 64) P.aset[(size_t)inst * 3 * N * 64 + e] = 0;
  if (T < ALTRO_TRACE_LEN) {
    P.Jtrace[(size_t)inst * ALTRO_TRACE_LEN + T] = 0.0;
    P.ctrace[(size_t)inst * ALTRO_TRACE_LEN + T] = 0.0;
    P.atrace[(size_t)inst * ALTRO_TRACE_LEN + T] = 0.0;
  }
  if (T == 0) {
    P.mu[inst] = 1.0;
    P.iters[inst] = 0;
    P.iters_outer[inst] = 0;
    P.status[inst] = ALTRO_UNSOLVED;
    P.cost[inst] = 0.0;
    P.cmax[inst] = 0.0;
    if (P.clk.start != nullptr) P.clk.window[inst] = 0;   // under an episode clock: back to the track's first window
  }
}

struct WideBackend : altro::BackendCommon {   // (what both backends hold and do alike: backend_common.h)
  // device
  double *A = nullptr, *Bm = nullptr, *f = nullptr, *wd = nullptr, *wf = nullptr, *zmin = nullptr, *zmax = nullptr;
  double *x0 = nullptr, *Xref = nullptr, *Uref = nullptr, *X = nullptr, *U = nullptr, *Lb = nullptr, *Lc = nullptr,
         *mu = nullptr, *Kg = nullptr, *dg = nullptr, *trash = nullptr, *AconT = nullptr, *bcon = nullptr, *Qz = nullptr, *fac = nullptr;
  unsigned char* aset = nullptr;   // [B][3][N][64] exact active sets (solve_wide.h: Params::aset)
  unsigned* bwst = nullptr;   // [B][136] per instance: the state of the gain reuse between launches (solve_wide.h: bw_*)
  int coop_mode = -1, static_mask = 7;  // altro_debug_set "wide_coop", "wide_static_mask" (before create)
  int compact_np_max = 48;  // wide_compact: the LDS carve-up with Qux and K inside W, for padded state dimensions up to this
  bool debug_keep_gains = false;  // altro_debug_set "keep_gains" (-DALTRO_DEBUG builds only): stale gains are kept (exists to show that the tests notice them)
  bool gains_valid = false;   // nothing the stored gains depend on (model, cost, constraints, options) has changed since the last launch
  double *Xsave = nullptr, *Usave = nullptr;  // Z0 of benchmark_solve
  std::vector<hipEvent_t> bench_ev;
  int *cur = nullptr, *ctype = nullptr, *rowk0 = nullptr, *rowk1 = nullptr, *rowc0 = nullptr, *rowcp = nullptr;
  int dyn_blocks = 1, dyn_step_stride = 0;
  size_t dyn_table_blocks = 0;   // blocks the tables A, Bm, f have room for (set_dynamics_dev reuses them while it is unchanged)
  bool ltv = false;
  std::vector<bool> box_lo_fin, box_hi_fin;   // [n+m] finite sides of the BOX (host copy: polish_prepare, set_bounds)
  int w_pi = 0, b_pi = 0;                     // wd / wf, resp. zmin / zmax, hold one row per instance
  double cost_dt = 0.0;                       // the dt of altro_batch_set_tracking_cost (evaluate_al_dev: gQ, gR)
  bool w_big = false, b_big = false;          // their device arrays have room for B rows
  struct Block {
    int id, sense, k0, k1, p, per_knot, r0;
    bool soc = false;
    bool per_instance = false;
    std::vector<double> A, b;  // row-major p x nz blocks: [instance if per_instance][knot of the range if per_knot]
    bool stale = false;        // update_constraint_data_dev wrote the device rows: A, b are refreshed before use
  };
  std::vector<Block> blocks;
  int Pn = 0, ncon = 0, ncone = 0;
  bool con_dirty = false, con_locked = false, con_per_instance = false;
  size_t acon_elems = (size_t)-1;

  int np() const { return pad16(d.n); }
  int mp() const { return pad16(d.m); }
  int nz() const { return d.n + d.m; }

  static bool supports(int n, int m) { return n >= 1 && m >= 1 && n <= kMaxN && m <= kMaxM; }

  int create(const altro_dims* dims, const altro_opts* opts, int dev) {
    d = *dims;
    o = *opts;
    device = dev;
    slots = d.batch;
    mlog_rec = (size_t)nz() + altro::MLOG_TAIL;
    noise_len = kMaxN;
    // (diagnostic switches -- compact_np_max: 0 = never, 32 / 48 = up to that padded n; coop_mode: cooperative blocks 0 = never,
    //  1 = every size with n or m > 16; static_mask: which uses of time-invariant constraint tables stay in LDS;
    //  debug_keep_gains -- are members set by the caller from altro_debug_set() before create(): nothing is read from the
    //  environment)
    WCHK(hipSetDevice(device));
    const Lds L = lds_layout(d.n, d.m, kMaxP);
    (void)L;
    WCHK(hipStreamCreate(&stream));
    WCHK(hipEventCreate(&ev0));
    WCHK(hipEventCreate(&ev1));
    ring.reset();
    bench_ev.reserve(2);
    const size_t B = d.batch, N = d.N, n = d.n, m = d.m, z = n + m;
    if (B * 3 * N * 64 >= (1ull << 32)) WFAIL(ALTRO_ERR_UNSUPPORTED, "batch x horizon too large for one handle (active-set planes are addressed with 32-bit offsets): split the batch");
    // every device array of the backend: (member, elements), zero-filled on the stream
    const size_t T = ALTRO_TRACE_LEN;
    const std::pair<double**, size_t> dbl[] = {
        {&wd, z}, {&wf, n}, {&zmin, z}, {&zmax, z}, {&x0, B * n}, {&X, B * 2 * N * n}, {&U, B * 2 * (N - 1) * m}, {&Lb, B * N * 2 * z},
        {&mu, B}, {&Kg, B * (N - 1) * n * m}, {&dg, B * (N - 1) * m}, {&trash, B * 64}, {&Qz, B * N * z},
        {&fac, m <= 16 ? B * N * wide_fac_size(m) : 1}, {&cost, B}, {&cmax, B}, {&Jtrace, B * T}, {&ctrace, B * T}, {&atrace, B * T},
        {&noise_w, kMaxN}, {&Lc, 1}, {&AconT, 1}, {&bcon, 1}};
    const std::pair<int**, size_t> ints[] = {{&cur, B}, {&iters, B}, {&iters_outer, B}, {&status, B}, {&noise_grp, kMaxN},
                                             {&ctype, 1}, {&rowk0, 1}, {&rowk1, 1}, {&rowc0, 1}, {&rowcp, 1}};
    for (const auto& a : dbl) WCHK(pool.alloc(a.first, a.second, stream));
    for (const auto& a : ints) WCHK(pool.alloc(a.first, a.second, stream));
    for (long long** c : {&n_backward, &n_rollout, &n_trials, &n_solves, &n_iters, &n_ok, &n_gconf, &n_reuse}) WCHK(pool.alloc(c, B, stream));
    WCHK(pool.alloc(&bwst, B * 136, stream));
    WCHK(pool.alloc(&aset, B * 3 * N * 64, stream));
    WCHK(pool.alloc(&refusals, 1, stream));
    {
      std::vector<double> inf(z, INFINITY), ninf(z, -INFINITY), w(kMaxN, 0.01), m0(B, 1.0);
      WCHK(hipMemcpyAsync(zmax, inf.data(), z * sizeof(double), hipMemcpyHostToDevice, stream));
      WCHK(hipMemcpyAsync(zmin, ninf.data(), z * sizeof(double), hipMemcpyHostToDevice, stream));
      WCHK(hipMemcpyAsync(noise_w, w.data(), kMaxN * sizeof(double), hipMemcpyHostToDevice, stream));
      WCHK(hipMemcpyAsync(mu, m0.data(), B * sizeof(double), hipMemcpyHostToDevice, stream));
      WCHK(hipStreamSynchronize(stream));
    }
    return ALTRO_OK;
  }

  void destroy() {
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    pool.release_all();
    ring.destroy();
    flags.destroy();
    clock.destroy();
    for (hipEvent_t e : bench_ev) hipEventDestroy(e);
    bench_ev.clear();
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    if (stream) hipStreamDestroy(stream);
  }

  // tables A, Bm, f with room for `blocks_` blocks (the caller has synchronised the stream)
  int alloc_dynamics(size_t blocks_) {
    const size_t n = d.n, m = d.m;
    dyn_table_blocks = 0;
    WCHK(pool.alloc(&A, blocks_ * n * n, stream, false));
    WCHK(pool.alloc(&Bm, blocks_ * n * m, stream, false));
    WCHK(pool.alloc(&f, blocks_ * n, stream, false));
    dyn_table_blocks = blocks_;
    return ALTRO_OK;
  }
  // blocks_per_instance knot blocks per instance (1: time-invariant)
  int upload_dynamics(const double* A_, const double* B_, const double* f_, size_t blocks_per_instance, int per_instance) {
    WCHK(hipSetDevice(device));
    WCHK(hipStreamSynchronize(stream));
    const size_t n = d.n, m = d.m;
    const size_t blocks_ = (per_instance ? (size_t)d.batch : 1) * blocks_per_instance;
    if (int rc = alloc_dynamics(blocks_)) return rc;
    WCHK(hipMemcpy(A, A_, blocks_ * n * n * sizeof(double), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(Bm, B_, blocks_ * n * m * sizeof(double), hipMemcpyHostToDevice));
    if (f_) WCHK(hipMemcpy(f, f_, blocks_ * n * sizeof(double), hipMemcpyHostToDevice));
    else WCHK(hipMemset(f, 0, blocks_ * n * sizeof(double)));
    dyn_per_instance = per_instance != 0;
    have_dyn = true;
    return ALTRO_OK;
  }
  // The same from device arrays (already validated), stream-ordered: the tables are reused while the block count is that
  // of the previous call; a call that changes it reallocates, and synchronises to do so, as the host call always does.
  int upload_dynamics_dev(const double* A_, const double* B_, const double* f_, size_t blocks_per_instance, int per_instance) {
    WCHK(hipSetDevice(device));
    const size_t n = d.n, m = d.m;
    const size_t blocks_ = (per_instance ? (size_t)d.batch : 1) * blocks_per_instance;
    if (blocks_ != dyn_table_blocks || !A || !Bm || !f) {
      WCHK(hipStreamSynchronize(stream));
      if (int rc = alloc_dynamics(blocks_)) return rc;
    }
    WCHK(hipMemcpyAsync(A, A_, blocks_ * n * n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    WCHK(hipMemcpyAsync(Bm, B_, blocks_ * n * m * sizeof(double), hipMemcpyDeviceToDevice, stream));
    if (f_) WCHK(hipMemcpyAsync(f, f_, blocks_ * n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    else WCHK(hipMemsetAsync(f, 0, blocks_ * n * sizeof(double), stream));
    dyn_per_instance = per_instance != 0;
    have_dyn = true;
    return ALTRO_OK;
  }
  int set_dynamics_dev(const double* A_, const double* B_, const double* f_, int per_knot, int per_instance) {
    gains_valid = false;
    const int rc = upload_dynamics_dev(A_, B_, f_, per_knot ? (size_t)(d.N - 1) : 1, per_instance);
    if (rc) return rc;
    ltv = per_knot != 0;
    dyn_blocks = per_knot ? d.N - 1 : 1;
    dyn_step_stride = 0;
    return ALTRO_OK;
  }

  int set_dynamics(const double* A_, const double* B_, const double* f_, int per_knot, int per_instance) {
    gains_valid = false;
    const int rc = upload_dynamics(A_, B_, f_, per_knot ? (size_t)(d.N - 1) : 1, per_instance);
    if (rc) return rc;
    ltv = per_knot != 0;
    dyn_blocks = per_knot ? d.N - 1 : 1;
    dyn_step_stride = 0;
    return ALTRO_OK;
  }

  // altro_mpc_set_dynamics_track: see include/altro_batch.h
  int mpc_set_dynamics_track(const double* A_, const double* B_, const double* f_, int nblocks, int step_stride, int per_instance) {
    gains_valid = false;
    if (nblocks < d.N - 1 || (step_stride != 1 && step_stride != d.N - 1)) WFAIL(ALTRO_ERR_INVALID_ARG, "bad dynamics track shape");
    if (clock.on) {   // the windows live on the device and a plain solve reads the blocks of the window it holds: all must exist
      std::vector<int> w(d.batch);
      WCHK(hipSetDevice(device));
      WCHK(hipStreamSynchronize(stream));
      WCHK(hipMemcpy(w.data(), clock.window, w.size() * sizeof(int), hipMemcpyDeviceToHost));
      for (int v : w)
        if ((long long)v * step_stride + (d.N - 1) > (long long)nblocks)
          WFAIL(ALTRO_ERR_STATE, "the dynamics track ends before the window an instance holds (altro_mpc_set_clock)");
    }
    const int rc = upload_dynamics(A_, B_, f_, (size_t)nblocks, per_instance);
    if (rc) return rc;
    ltv = true;
    dyn_blocks = nblocks;
    dyn_step_stride = step_stride;
    return ALTRO_OK;
  }
  // last reference-window start the dynamics table covers
  bool dyn_covers(int kref_) const { return !ltv || (long long)kref_ * dyn_step_stride + (d.N - 1) <= (long long)dyn_blocks; }

  int set_tracking_cost(const double* Qd, const double* Rd, const double* Qfd, double dt) {
    return set_cost_rows(Qd, Rd, Qfd, dt, 1);
  }
  int set_tracking_cost_per_instance(const double* Qd, const double* Rd, const double* Qfd, double dt) {
    return set_cost_rows(Qd, Rd, Qfd, dt, (size_t)d.batch);
  }
  // rows = 1: one row for the batch; rows = B: Qd [B][n], Rd [B][m], Qfd [B][n]
  int set_cost_rows(const double* Qd, const double* Rd, const double* Qfd, double dt, size_t rows) {
    gains_valid = false;
    WCHK(hipSetDevice(device));
    const size_t n = d.n, m = d.m, z = nz();
    if ((rows > 1 && !w_big) || !wd || !wf) {   // the shared arrays hold one row: room for B rows from now on
      WCHK(hipStreamSynchronize(stream));
      WCHK(pool.alloc(&wd, rows * z, stream));
      WCHK(pool.alloc(&wf, rows * n, stream));
      w_big = rows > 1;
    }
    std::vector<double> w(rows * z);
    for (size_t r = 0; r < rows; ++r) {
      for (size_t i = 0; i < n; ++i) w[r * z + i] = dt * Qd[r * n + i];
      for (size_t i = 0; i < m; ++i) w[r * z + n + i] = dt * Rd[r * m + i];
    }
    WCHK(hipMemcpy(wd, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(wf, Qfd, rows * n * sizeof(double), hipMemcpyHostToDevice));
    w_pi = rows > 1 ? 1 : 0;
    cost_dt = dt;
    have_cost = true;
    return ALTRO_OK;
  }

  // altro_batch_set_bounds: new values for the BOX, one row for the batch or one per instance (per_instance != 0).  (As for
  // every host call below, the entry point has checked the null pointers, the ranges and that the id is the BOX's.)
  int set_bounds(const double* zmin_, const double* zmax_, int per_instance) {
    const size_t rows = per_instance ? (size_t)d.batch : 1, z = nz();
    {
      bool lfb[kMaxN + kMaxM], hfb[kMaxN + kMaxM];
      for (size_t j = 0; j < z; ++j) { lfb[j] = box_lo_fin[j]; hfb[j] = box_hi_fin[j]; }
      if (const char* e = check_bound_rows(zmin_, zmax_, rows, (int)z, lfb, hfb)) WFAIL(ALTRO_ERR_INVALID_ARG, e);
    }
    gains_valid = false;
    WCHK(hipSetDevice(device));
    if ((rows > 1 && !b_big) || !zmin || !zmax) {
      WCHK(hipStreamSynchronize(stream));
      WCHK(pool.alloc(&zmin, rows * z, stream));
      WCHK(pool.alloc(&zmax, rows * z, stream));
      b_big = rows > 1;
    }
    WCHK(hipStreamSynchronize(stream));
    WCHK(hipMemcpy(zmin, zmin_, rows * z * sizeof(double), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(zmax, zmax_, rows * z * sizeof(double), hipMemcpyHostToDevice));
    b_pi = rows > 1 ? 1 : 0;
    return ALTRO_OK;
  }

  int add_constraint(int kind, int sense, int k_first, int k_last, int p, const double* A_, const double* b_, const double* zmin_,
                     const double* zmax_, int per_knot, int* con_id) {
    WCHK(hipSetDevice(device));
    if (con_locked) WFAIL(ALTRO_ERR_STATE, "constraints must be added before the first solve");
    if (kind == ALTRO_CON_BOX) {
      if (box_id >= 0) WFAIL(ALTRO_ERR_UNSUPPORTED, "one BOX constraint per problem");
      WCHK(hipMemcpy(zmin, zmin_, nz() * sizeof(double), hipMemcpyHostToDevice));
      WCHK(hipMemcpy(zmax, zmax_, nz() * sizeof(double), hipMemcpyHostToDevice));
      box_lo_fin.assign(nz(), false);
      box_hi_fin.assign(nz(), false);
      for (int j = 0; j < nz(); ++j) { box_lo_fin[j] = zmin_[j] > -1e300; box_hi_fin[j] = zmax_[j] < 1e300; }
      b_pi = 0;
      box_k0 = k_first;
      box_k1 = k_last;
      box_id = ncon++;
      if (con_id) *con_id = box_id;
      return ALTRO_OK;
    }
    if (kind == ALTRO_CON_SOC && (p < 2 || p > 4)) WFAIL(ALTRO_ERR_UNSUPPORTED, "second-order cones of dimension 2..4 only");
    if (Pn + p > kMaxP) WFAIL(ALTRO_ERR_UNSUPPORTED, "more than 64 linear constraint rows");
    // (rows a `_dev` update wrote come back while the tables still have the row count Pn they were packed with)
    if (int rcm = refresh_block_mirrors()) return rcm;
    Block bl;
    bl.id = ncon++;
    bl.soc = kind == ALTRO_CON_SOC;
    bl.sense = sense; bl.k0 = k_first; bl.k1 = k_last; bl.p = p; bl.per_knot = (per_knot & 1) ? 1 : 0; bl.r0 = Pn;
    bl.per_instance = (per_knot & 2) != 0;
    const size_t nb = (bl.per_knot ? (size_t)(k_last - k_first + 1) : 1) * (bl.per_instance ? (size_t)d.batch : 1);
    bl.A.assign(A_, A_ + nb * p * nz());
    bl.b.assign(b_, b_ + nb * p);
    blocks.push_back(bl);
    Pn += p;
    con_dirty = true;
    if (con_id) *con_id = bl.id;
    return ALTRO_OK;
  }

  Block* find(int id) {
    for (auto& b : blocks)
      if (b.id == id) return &b;
    return nullptr;
  }

  // Host mirrors after update_constraint_data_dev: the rows a `_dev` call wrote exist on the device only.  Before anything
  // reads Block::A / b the device tables are read back and the stale blocks are taken out of them (the inverse of
  // pack_constraints).  The tables are decoded with the Pn and con_per_instance they were packed with: add_constraint
  // refreshes BEFORE it changes Pn.  Synchronises; its callers (a host update, a repack, add_constraint) do anyway.
  int refresh_block_mirrors() {
    bool any = false;
    for (const auto& bl : blocks) any = any || bl.stale;
    if (!any) return ALTRO_OK;
    WCHK(hipSetDevice(device));
    const size_t N = d.N, z = nz(), P = Pn, B = d.batch;
    const size_t ninst = con_per_instance ? B : 1;
    std::vector<double> At(ninst * N * z * P), bc(ninst * N * P);
    WCHK(hipStreamSynchronize(stream));
    WCHK(hipMemcpy(At.data(), AconT, At.size() * sizeof(double), hipMemcpyDeviceToHost));
    WCHK(hipMemcpy(bc.data(), bcon, bc.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (auto& bl : blocks) {
      if (!bl.stale) continue;
      const size_t nk = bl.per_knot ? (size_t)(bl.k1 - bl.k0 + 1) : 1;
      for (size_t ib = 0; ib < (bl.per_instance ? B : 1); ++ib)
        for (size_t kk = 0; kk < nk; ++kk)
          for (int r = 0; r < bl.p; ++r) {
            const size_t blk = ib * nk + kk, e = ib * N + (size_t)bl.k0 + kk, row = (size_t)bl.r0 + r;
            bl.b[blk * bl.p + r] = bc[e * P + row];
            for (size_t j = 0; j < z; ++j) bl.A[(blk * bl.p + r) * z + j] = At[(e * z + j) * P + row];
          }
      bl.stale = false;
    }
    return ALTRO_OK;
  }

  // altro_batch_update_constraint_data_dev (pointers validated by the caller): the rows go straight into AconT / bcon on the
  // stream.  While the tables do not exist yet (con_dirty: before the first solve, or after a host update) this one call packs
  // them on the host first, which synchronises once.  bl: the constraint's block (find(), looked up by the caller).
  int update_constraint_data_dev(Block* bl, const double* A_, const double* b_) {
    WCHK(hipSetDevice(device));
    if (con_dirty) {
      WCHK(hipStreamSynchronize(stream));   // a solve in flight may still be reading the tables the repack frees or overwrites
      const int rc = pack_constraints();
      if (rc) return rc;
    }
    const int nk = bl->k1 - bl->k0 + 1;
    const size_t ninst = con_per_instance ? (size_t)d.batch : 1;
    const size_t total = ninst * nk * bl->p * (size_t)nz();
    hipLaunchKernelGGL(altro::k_pack_con_rows_wide, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, AconT, bcon, A_, b_, (int)ninst,
                       d.N, nz(), Pn, bl->r0, bl->k0, nk, bl->p, bl->per_knot, bl->per_instance ? 1 : 0);
    WCHK(hipGetLastError());
    gains_valid = false;
    bl->stale = true;
    return ALTRO_OK;
  }

  // altro_batch_set_bounds_dev (pointers validated by the caller): rows checked and written on the device
  // (device_io.h: k_set_bounds_rows).  A shared row written while the table holds one row per instance goes to every row, and the
  // table keeps that shape.  The first per-instance call on a table of one row gives it B rows: it allocates and synchronises
  // once, and every row starts as the shared one.  (The caller has checked that the id is the BOX's.)
  int set_bounds_dev(const double* lo, const double* hi, int per_instance) {
    WCHK(hipSetDevice(device));
    const size_t B = d.batch, z = nz();
    if (per_instance && !b_pi && B > 1) {
      if (!b_big) {   // the shared row goes through the host while the tables are replaced by ones of B rows
        std::vector<double> r0(2 * z);
        WCHK(hipStreamSynchronize(stream));
        WCHK(hipMemcpy(r0.data(), zmin, z * sizeof(double), hipMemcpyDeviceToHost));
        WCHK(hipMemcpy(r0.data() + z, zmax, z * sizeof(double), hipMemcpyDeviceToHost));
        WCHK(pool.alloc(&zmin, B * z, stream, false));
        WCHK(pool.alloc(&zmax, B * z, stream, false));
        WCHK(hipMemcpy(zmin, r0.data(), z * sizeof(double), hipMemcpyHostToDevice));
        WCHK(hipMemcpy(zmax, r0.data() + z, z * sizeof(double), hipMemcpyHostToDevice));
        b_big = true;
      }
      const dim3 g((unsigned)((B * z + 255) / 256));
      hipLaunchKernelGGL(altro::k_fan_row0, g, dim3(256), 0, stream, zmin, (int)z, (int)B);
      hipLaunchKernelGGL(altro::k_fan_row0, g, dim3(256), 0, stream, zmax, (int)z, (int)B);
      WCHK(hipGetLastError());
      b_pi = 1;
    }
    altro::FinMask fin{};
    for (size_t j = 0; j < z; ++j) {
      if (box_lo_fin[j]) fin.lo[j >> 6] |= 1ull << (j & 63);
      if (box_hi_fin[j]) fin.hi[j >> 6] |= 1ull << (j & 63);
    }
    const size_t rows = b_pi ? B : 1;
    hipLaunchKernelGGL(altro::k_set_bounds_rows, dim3((unsigned)((rows * 16 + 255) / 256)), dim3(256), 0, stream, zmin, zmax, lo, hi, fin, (int)z,
                       (int)z, (int)rows, (int)B, per_instance ? 1 : 0, refusals);
    WCHK(hipGetLastError());
    gains_valid = false;
    return ALTRO_OK;
  }

  int update_constraint_data(int con_id, const double* A_, const double* b_) {
    gains_valid = false;
    Block* bl = find(con_id);
    if (!bl) WFAIL(ALTRO_ERR_INVALID_ARG, "no such LINEAR constraint");
    if (int rcm = refresh_block_mirrors()) return rcm;   // (a `_dev` update before this one: its rows come back first)
    const size_t nb = (bl->per_knot ? (size_t)(bl->k1 - bl->k0 + 1) : 1) * (bl->per_instance ? (size_t)d.batch : 1);
    if (A_) bl->A.assign(A_, A_ + nb * bl->p * nz());
    if (b_) bl->b.assign(b_, b_ + nb * bl->p);
    con_dirty = true;
    return ALTRO_OK;
  }

  // per-knot tables of the generic rows (transposed: AconT[k][j][r])
  int pack_constraints() {
    if (!con_dirty) return ALTRO_OK;
    if (int rcm = refresh_block_mirrors()) return rcm;
    WCHK(hipSetDevice(device));
    const size_t N = d.N, z = nz(), P = Pn;
    // one table per instance as soon as any block carries per-instance data (grasp_mpc_helpers.jl:46-55 mutates each
    // problem's own tables); otherwise one table shared by the batch
    con_per_instance = false;
    for (const auto& bl : blocks) con_per_instance = con_per_instance || bl.per_instance;
    const size_t ninst = con_per_instance ? (size_t)d.batch : 1;
    std::vector<double> At(ninst * N * z * P, 0.0), bc(ninst * N * P, 0.0);
    std::vector<int> ct(N * P, 0), k0(P, 0), k1(P, -1), c0(P, 0), cp(P, 0);
    ncone = 0;
    for (const auto& bl : blocks) ncone += bl.soc ? 1 : 0;
    for (const auto& bl : blocks)
      for (int r = 0; r < bl.p; ++r) {
        const int row = bl.r0 + r;
        k0[row] = bl.k0;
        k1[row] = bl.k1;
        c0[row] = bl.soc ? bl.r0 : 0;
        cp[row] = bl.soc ? bl.p : 0;
        const size_t nk = bl.per_knot ? (size_t)(bl.k1 - bl.k0 + 1) : 1;
        for (int k = bl.k0; k <= bl.k1; ++k) {
          ct[k * P + row] = bl.soc ? 3 : (bl.sense == ALTRO_SENSE_EQ ? 1 : 2);
          for (size_t ib = 0; ib < ninst; ++ib) {
            const size_t blk = (bl.per_instance ? ib * nk : 0) + (bl.per_knot ? (size_t)(k - bl.k0) : 0);
            bc[(ib * N + k) * P + row] = bl.b[blk * bl.p + r];
            for (size_t j = 0; j < z; ++j) At[((ib * N + k) * z + j) * P + row] = bl.A[(blk * bl.p + r) * z + j];
          }
        }
      }
    if (At.size() != acon_elems || !AconT || !bcon) {  // the table changed shape (a block with per-instance data arrived): reallocate
      WCHK(pool.alloc(&AconT, At.size(), stream, false));
      WCHK(pool.alloc(&bcon, bc.size(), stream, false));
      acon_elems = At.size();
    }
    if (!con_locked) {
      WCHK(pool.alloc(&ctype, ct.size(), stream, false));
      for (int** p : {&rowk0, &rowk1, &rowc0, &rowcp}) WCHK(pool.alloc(p, P, stream, false));
      WCHK(pool.alloc(&Lc, (size_t)d.batch * N * P, stream));
    }
    WCHK(hipMemcpy(AconT, At.data(), At.size() * sizeof(double), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(bcon, bc.data(), bc.size() * sizeof(double), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(ctype, ct.data(), ct.size() * sizeof(int), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(rowk0, k0.data(), P * sizeof(int), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(rowk1, k1.data(), P * sizeof(int), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(rowc0, c0.data(), P * sizeof(int), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(rowcp, cp.data(), P * sizeof(int), hipMemcpyHostToDevice));
    con_dirty = false;
    return ALTRO_OK;
  }

  int set_initial_state(const double* x) {
    WCHK(hipSetDevice(device));
    WCHK(hipMemcpyAsync(x0, x, (size_t)d.batch * d.n * sizeof(double), hipMemcpyHostToDevice, stream));
    WCHK(hipStreamSynchronize(stream));
    return ALTRO_OK;
  }
  int get_initial_state(double* x) {
    WCHK(hipSetDevice(device));
    WCHK(hipStreamSynchronize(stream));
    WCHK(hipMemcpy(x, x0, (size_t)d.batch * d.n * sizeof(double), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }

  // device twins of the three calls around (altro_*_dev: pointers already validated; stream-ordered copies, no synchronisation)
  int set_initial_state_dev(const double* x) {
    WCHK(hipSetDevice(device));
    WCHK(hipMemcpyAsync(x0, x, (size_t)d.batch * d.n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    return ALTRO_OK;
  }
  int get_initial_state_dev(double* x) {
    WCHK(hipSetDevice(device));
    WCHK(hipMemcpyAsync(x, x0, (size_t)d.batch * d.n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    return ALTRO_OK;
  }
  // Xref, Uref for a track of Nt_ knots (the caller has synchronised the stream); no reference while they do not exist
  int alloc_reference(int Nt_) {
    Nt = 0;
    have_ref = false;
    WCHK(pool.alloc(&Xref, (size_t)d.batch * Nt_ * d.n, stream, false));
    WCHK(pool.alloc(&Uref, (size_t)d.batch * (Nt_ - 1) * d.m, stream, false));
    Nt = Nt_;
    return ALTRO_OK;
  }
  int set_reference_dev(const double* Xr, const double* Ur) {
    WCHK(hipSetDevice(device));
    const int Nt_ = d.N;
    if (Nt_ != Nt || !Xref || !Uref) {   // another window length than the stored one: reallocate, as the host call does
      WCHK(hipStreamSynchronize(stream));
      if (int rc = alloc_reference(Nt_)) return rc;
    }
    WCHK(hipMemcpyAsync(Xref, Xr, (size_t)d.batch * Nt * d.n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    WCHK(hipMemcpyAsync(Uref, Ur, (size_t)d.batch * (Nt - 1) * d.m * sizeof(double), hipMemcpyDeviceToDevice, stream));
    kref = 0;
    have_ref = true;
    if (clock.on) {   // a new track installs window 0 for every instance, as it does for the handle's kref
      hipLaunchKernelGGL(altro::k_clock_window, altro::EpisodeClock::grid(d.batch), dim3(256), 0, stream, clock.window, (const int*)nullptr, 0, d.batch);
      WCHK(hipGetLastError());
    }
    return ALTRO_OK;
  }

  int set_ref_common(const double* Xr, const double* Ur, int Nt_) {
    WCHK(hipSetDevice(device));
    WCHK(hipStreamSynchronize(stream));
    if (Nt_ != Nt || !Xref || !Uref) {
      if (int rc = alloc_reference(Nt_)) return rc;
    }
    WCHK(hipMemcpy(Xref, Xr, (size_t)d.batch * Nt * d.n * sizeof(double), hipMemcpyHostToDevice));
    WCHK(hipMemcpy(Uref, Ur, (size_t)d.batch * (Nt - 1) * d.m * sizeof(double), hipMemcpyHostToDevice));
    kref = 0;
    have_ref = true;
    if (clock.on) {   // a new track installs window 0 for every instance, as it does for the handle's kref
      hipLaunchKernelGGL(altro::k_clock_window, altro::EpisodeClock::grid(d.batch), dim3(256), 0, stream, clock.window, (const int*)nullptr, 0, d.batch);
      WCHK(hipGetLastError());
    }
    return ALTRO_OK;
  }
  int set_reference(const double* Xr, const double* Ur) {
    return set_ref_common(Xr, Ur, d.N);
  }

  // plane cur[b] of X / U <- host image (instance-major)
  int put_planes(const double* Xh, const double* Uh) {
    const size_t B = d.batch, lx = (size_t)d.N * d.n, lu = (size_t)(d.N - 1) * d.m;
    int rc = ensure_stage(B * (lx + lu) * sizeof(double));
    if (rc) return rc;
    if (Xh) {
      WCHK(hipMemcpyAsync(stage, Xh, B * lx * sizeof(double), hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL(k_scatter_plane, dim3((unsigned)((B * lx + 255) / 256)), dim3(256), 0, stream, X, stage, cur, lx, (int)B);
    }
    if (Uh) {
      double* su = stage + B * lx;
      WCHK(hipMemcpyAsync(su, Uh, B * lu * sizeof(double), hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL(k_scatter_plane, dim3((unsigned)((B * lu + 255) / 256)), dim3(256), 0, stream, U, su, cur, lu, (int)B);
    }
    WCHK(hipStreamSynchronize(stream));
    return ALTRO_OK;
  }
  int set_initial_trajectory(const double* Xh, const double* Uh) {
    WCHK(hipSetDevice(device));
    return put_planes(Xh, Uh);
  }
  // device twins: the scatter / gather kernels run on the caller's arrays, no staging copy
  int set_initial_trajectory_dev(const double* Xd, const double* Ud) {
    WCHK(hipSetDevice(device));
    const size_t B = d.batch, lx = (size_t)d.N * d.n, lu = (size_t)(d.N - 1) * d.m;
    if (Xd) hipLaunchKernelGGL(k_scatter_plane, dim3((unsigned)((B * lx + 255) / 256)), dim3(256), 0, stream, X, Xd, cur, lx, (int)B);
    hipLaunchKernelGGL(k_scatter_plane, dim3((unsigned)((B * lu + 255) / 256)), dim3(256), 0, stream, U, Ud, cur, lu, (int)B);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  int get_planes_dev(double* Xd, double* Ud) {
    WCHK(hipSetDevice(device));
    const size_t B = d.batch, lx = (size_t)d.N * d.n, lu = (size_t)(d.N - 1) * d.m;
    if (Xd) hipLaunchKernelGGL(k_gather_plane, dim3((unsigned)((B * lx + 255) / 256)), dim3(256), 0, stream, Xd, X, cur, lx, (int)B);
    if (Ud) hipLaunchKernelGGL(k_gather_plane, dim3((unsigned)((B * lu + 255) / 256)), dim3(256), 0, stream, Ud, U, cur, lu, (int)B);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_get_first_knot_dev: one kernel that reads plane cur[b] (device_io.h)
  int get_first_knot_dev(double* u0d, double* x1d, int32_t* st, int32_t* it) {
    WCHK(hipSetDevice(device));
    const size_t thr = (size_t)d.batch * nz();
    hipLaunchKernelGGL(altro::k_first_knot_wide, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, stream, u0d, x1d, st, it, X, U, cur,
                       status, iters, d.batch, d.N, d.n, d.m);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_eval_policy_dev (pointers validated by the caller; the host twin passes staged copies): one kernel on the
  // current planes, Kg, the reuse state and the bounds rows (policy.h)
  int eval_policy_dev(const double* xd, const int32_t* knot, int clamp, double* ud, int32_t* fb) {
    WCHK(hipSetDevice(device));
    const size_t thr = (size_t)d.batch * d.m;
    hipLaunchKernelGGL(altro::k_eval_policy_wide, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, stream, ud, fb, xd, knot, X, U, cur, Kg, bwst,
                       (gains_valid || debug_keep_gains) ? 1 : 0, zmin, zmax, b_pi, d.batch, d.N, d.n, d.m, clamp ? 1 : 0, box_k0, box_k1);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // what evaluate_dev, warm_start_dev and simulate_policy_dev check first ...
  int eval_ready() {
    if (int rc = check_ready()) return rc;
    if (!clock.on && kref + d.N > Nt) WFAIL(ALTRO_ERR_STATE, "reference window runs past the end of the stored trajectory");
    if (!clock.on && !dyn_covers(kref)) WFAIL(ALTRO_ERR_STATE, "the dynamics track ends before the window");
    if (int rc = pack_constraints()) return rc;   // (what the next solve would do first; a no-op once the tables are packed)
    return ALTRO_OK;
  }
  // ... and the tables their kernels read, as the solve kernels address them now
  altro::EvalW eval_params() const {
    altro::EvalW p{};
    p.A = A; p.Bm = Bm; p.f = f; p.wd = wd; p.wf = wf; p.zmin = zmin; p.zmax = zmax; p.Xref = Xref; p.Uref = Uref;
    p.AconT = AconT; p.bcon = bcon; p.ctype = ctype; p.rowc0 = rowc0; p.rowcp = rowcp; p.window = clock.args().window;
    p.con_istride = con_per_instance ? (size_t)d.N * nz() * Pn : 0;
    p.bcon_istride = con_per_instance ? (size_t)d.N * Pn : 0;
    p.w_pi = w_pi; p.b_pi = b_pi; p.ltv = ltv; p.dyn_pi = dyn_per_instance; p.dyn_blocks = dyn_blocks; p.dyn_stride = dyn_step_stride;
    p.Pn = Pn; p.N = d.N; p.Nt = Nt; p.n = d.n; p.m = d.m; p.kref = kref; p.box_k0 = box_k0; p.box_k1 = box_k1;
    p.lds_dyn = altro::evalw_lds_fits(d.n, d.n, d.m, ltv) ? 1 : 0;
    return p;
  }
  // the LDS a block of their kernels asks for: the wave's dynamics when p.lds_dyn says they are kept there, else 0 ...
  static size_t eval_lds(const altro::EvalW& p) { return p.lds_dyn ? altro::evalw_lds_bytes(p.n, p.n, p.m) : 0; }
  // ... and for k_eval_grad_wide, whose slice has the odd leading dimension of its transposed reads and its own rule for fitting
  static size_t eval_grad_lds(const altro::EvalW& p) {
    const int ld = altro::evalw_ld(p.n, true);
    return altro::evalw_lds_fits(ld, p.n, p.m, p.ltv) ? altro::evalw_lds_bytes(ld, p.n, p.m) : 0;
  }
  // altro_batch_evaluate_dev (evaluate.h; pointers and argument rules checked by the caller, the host twin passes staged
  // copies): the rollout kernel when there is no X, then the scoring kernel on states and controls in memory.  Reads what the
  // next solve would read; writes the caller's outputs and eval_ws only.
  int evaluate_dev(int ncand, const double* Ud, const double* Xd, const double* x0d, double* Jd, double* cd, double* dd, double* Xout) {
    WCHK(hipSetDevice(device));
    if (int rc = eval_ready()) return rc;
    const size_t R = (size_t)d.batch * ncand, lx = (size_t)d.N * d.n, lu = (size_t)(d.N - 1) * d.m;
    const size_t need = !Ud ? R * (lx + lu) : (!Xd && !Xout) ? R * lx : 0;
    if (need) WCHK(pool.reserve(&eval_ws, &eval_ws_elems, need));
    const altro::EvalW p = eval_params();
    const size_t lds = eval_lds(p);
    const dim3 grid((unsigned)((R * 64 + 255) / 256)), block(256);
    int given = 1;
    if (!Ud) {   // own trajectory: the current planes, gathered into the workspace in the caller's layout
      if (int rc = get_planes_dev(eval_ws, eval_ws + R * lx)) return rc;
      Xd = eval_ws;
      Ud = eval_ws + R * lx;
    } else if (!Xd) {
      double* Xw = Xout ? Xout : eval_ws;
      hipLaunchKernelGGL(altro::k_eval_rollout_wide, grid, block, lds, stream, Xw, Ud, x0d ? x0d : x0, p, ncand, R);
      WCHK(hipGetLastError());
      Xd = Xw;
      given = 0;
    }
    hipLaunchKernelGGL(altro::k_eval_score_wide, grid, block, (dd && given) ? lds : 0, stream, Jd, cd, dd, Xd, Ud, p, ncand, R, given);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_evaluate_grad_dev (evaluate_grad.h; pointers and argument rules checked by the caller, the host twin passes
  // staged copies): one kernel over batch * ncand waves.  Reads what the next solve would read; writes the caller's outputs and
  // eval_ws only.
  int evaluate_grad_dev(int ncand, const double* Ud, const double* x0d, double rho, double* Jd, double* Pd, double* gUd, double* gx0d,
                        double* Xout) {
    WCHK(hipSetDevice(device));
    if (int rc = eval_ready()) return rc;
    const size_t R = (size_t)d.batch * ncand;
    if (!Xout) WCHK(pool.reserve(&eval_ws, &eval_ws_elems, R * (size_t)d.N * d.n));
    const altro::EvalW p = eval_params();
    const size_t lds = eval_grad_lds(p);
    const altro::GradIO io{Ud, x0d ? x0d : x0, Jd, Pd, gUd, gx0d, Xout ? Xout : eval_ws, rho};
    hipLaunchKernelGGL(altro::k_eval_grad_wide, dim3((unsigned)((R * 64 + 255) / 256)), dim3(256), lds, stream, io, p, ncand, R, lds ? 1 : 0);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_evaluate_al_dev (evaluate_al.h; pointers and argument rules checked by the caller, the host twin passes staged
  // copies): one kernel over batch * ncand waves (after the gather of the held controls into the workspace when Ud is null).
  // Reads what the next solve would read, the duals and the penalty included; writes the caller's outputs and eval_ws only.
  int evaluate_al_dev(int ncand, const double* Ud, const double* x0d, const altro_al_out& o) {
    WCHK(hipSetDevice(device));
    if (int rc = eval_ready()) return rc;
    const size_t R = (size_t)d.batch * ncand, lx = (size_t)d.N * d.n, lu = (size_t)(d.N - 1) * d.m;
    const size_t need = (o.Xout ? 0 : R * lx) + (Ud ? 0 : R * lu);
    if (need) WCHK(pool.reserve(&eval_ws, &eval_ws_elems, need));
    if (!Ud) {
      double* Uw = eval_ws + (o.Xout ? 0 : R * lx);
      if (int rc = get_planes_dev(nullptr, Uw)) return rc;
      Ud = Uw;
    }
    const altro::EvalW p = eval_params();
    const size_t lds = eval_grad_lds(p);
    const altro::ALIO io{Ud, x0d ? x0d : x0, o.LA, o.J, o.gU, o.gx0, o.gXref, o.gUref, o.gQ, o.gQf, o.gR, o.gzmin, o.gzmax,
                         o.Xout ? o.Xout : eval_ws, Lb, Lc, mu, nullptr, 0, 0.5 * cost_dt};
    hipLaunchKernelGGL(altro::k_eval_al_wide, dim3((unsigned)((R * 64 + 255) / 256)), dim3(256), lds, stream, io, p, ncand, R, lds ? 1 : 0);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_warm_start_dev (warm_start.h; pointers and argument rules checked by the caller, the host twin passes staged
  // copies): the fused rollout-and-score kernel over batch * (ncand + inc) waves, then select-and-install over batch waves.
  // Reads what the next solve would read; writes the caller's outputs, ws_merit and plane cur[b] of X / U.
  int warm_start_dev(int ncand, const double* Ud, double rho, int inc, int32_t* chosen, double* Jd, double* cd) {
    WCHK(hipSetDevice(device));
    if (int rc = eval_ready()) return rc;
    const size_t R = (size_t)d.batch * (size_t)(ncand + inc);
    if (!Jd || !cd) {
      WCHK(pool.reserve(&ws_merit, &ws_merit_elems, 2 * R));
      if (!Jd) Jd = ws_merit;
      if (!cd) cd = ws_merit + R;
    }
    const altro::EvalW p = eval_params();
    const size_t lds = eval_lds(p);
    hipLaunchKernelGGL(altro::k_ws_score_wide, dim3((unsigned)((R * 64 + 255) / 256)), dim3(256), lds, stream, Jd, cd, Ud, U, cur, x0, p, ncand, inc, R);
    WCHK(hipGetLastError());
    hipLaunchKernelGGL(altro::k_ws_install_wide, dim3((unsigned)(((size_t)d.batch * 64 + 255) / 256)), dim3(256), lds, stream, chosen, Jd, cd, Ud, X, U,
                       cur, x0, flags.mask(), p, ncand, inc, rho, (size_t)d.batch);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_simulate_policy_dev (simulate.h; pointers and argument rules checked by the caller, the host twin passes staged
  // copies): one fused kernel over batch * nsamp waves.  Reads what the next solve and eval_policy_dev would read; writes the
  // caller's outputs only.
  int simulate_policy_dev(int nsamp, int clamp, const altro::SimIO& io) {
    WCHK(hipSetDevice(device));
    if (int rc = eval_ready()) return rc;
    const size_t R = (size_t)d.batch * (size_t)nsamp;
    const altro::EvalW p = eval_params();
    const size_t lds = eval_lds(p);
    hipLaunchKernelGGL(altro::k_sim_wide, dim3((unsigned)((R * 64 + 255) / 256)), dim3(256), lds, stream, io, X, U, cur, Kg, bwst,
                       (gains_valid || debug_keep_gains) ? 1 : 0, x0, p, nsamp, clamp ? 1 : 0, R);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_propagate_covariance_dev (covariance.h; pointers and argument rules checked by the caller, the host twin passes
  // staged copies): one kernel, one wave per instance.  Reads what the next solve and eval_policy_dev would read; writes the
  // caller's outputs only and allocates nothing.  con_id: the LINEAR / SOC constraint behind io.sc (the caller has found it), or -1.
  int propagate_covariance_dev(const altro::CovIO& io, int con_id) {
    WCHK(hipSetDevice(device));
    if (int rc = eval_ready()) return rc;
    altro::CovRows cr{};
    if (con_id >= 0) {
      const Block* bl = find(con_id);
      if (!bl) WFAIL(ALTRO_ERR_INVALID_ARG, "no such constraint");
      cr.p = bl->p; cr.k0 = bl->k0; cr.k1 = bl->k1; cr.r0 = bl->r0;
    }
    const size_t lds = altro::covw_lds_doubles(d.n, d.m) * sizeof(double);
    // the allowance belongs to the kernel, for the whole process, and another handle may have set it since: asked for at
    // every launch above the 64 KB a kernel gets unasked, as prepare_launch does for the solve kernels
    if (lds > 65536) WCHK(hipFuncSetAttribute((const void*)altro::k_cov_wide, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(altro::k_cov_wide, dim3((unsigned)d.batch), dim3(64), lds, stream, io, cr, Kg, bwst,
                       (gains_valid || debug_keep_gains) ? 1 : 0, eval_params());
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_cost_to_go_dev (cost_to_go.h; pointers and argument rules checked by the caller, the host twin passes staged
  // copies): one kernel, one wave per instance.  Reads what propagate_covariance_dev reads, the planes the handle holds and --
  // mode 1 only -- the active set of the last backward pass, the duals and the penalty; writes the caller's outputs only and
  // allocates nothing.  Mode 1 needs a diagonal Hessian: generic rows are refused.
  int cost_to_go_dev(altro::CtgIO io) {
    WCHK(hipSetDevice(device));
    if (io.mode != 0 && Pn > 0)
      WFAIL(ALTRO_ERR_UNSUPPORTED, "cost_to_go: mode 1 needs a box-only problem: with LINEAR or SOC rows the Hessian inside the active set is not diagonal");
    if (int rc = eval_ready()) return rc;
    io.Lb = Lb; io.mu = mu; io.bslot = nullptr; io.nbp = 0;
    const size_t lds = altro::ctgw_lds_doubles(d.n, d.m) * sizeof(double);
    if (lds > 65536) WCHK(hipFuncSetAttribute((const void*)altro::k_ctg_wide, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // (at every launch: propagate_covariance_dev)
    hipLaunchKernelGGL(altro::k_ctg_wide, dim3((unsigned)d.batch), dim3(64), lds, stream, io, X, U, cur, Kg, bwst, aset,
                       (gains_valid || debug_keep_gains) ? 1 : 0, eval_params());
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_solution_vjp_dev / _jvp_dev (sensitivity.h; pointers and argument rules checked by the caller, the host twins
  // pass staged copies): one kernel over batch * nseed waves.  Reads what the next solve and eval_policy_dev would read and the
  // factors of Quu; writes the caller's outputs and eval_ws (d_k between the sweeps) only.  m > 16: no factors are kept, so
  // what needs both sweeps is refused before anything is enqueued.
  int solution_sens_dev(int nseed, altro::SensIO io) {
    WCHK(hipSetDevice(device));
    const bool need_d = io.bwd && io.fwd;
    if (need_d && d.m > 16)
      WFAIL(ALTRO_ERR_UNSUPPORTED, "the one-wave-per-instance kernels keep no factors of Quu for m > 16: only the x0-only sensitivities (gx0 alone, vx0 alone) are available");
    if (int rc = eval_ready()) return rc;
    const size_t R = (size_t)d.batch * nseed;
    if (need_d) {
      WCHK(pool.reserve(&eval_ws, &eval_ws_elems, R * (size_t)(d.N - 1) * d.m));
      io.dws = eval_ws;
    }
    const altro::EvalW p = eval_params();
    const size_t lds = eval_grad_lds(p);
    hipLaunchKernelGGL(altro::k_sens_wide, dim3((unsigned)((R * 64 + 255) / 256)), dim3(256), lds, stream, io, Kg, d.m <= 16 ? fac : nullptr,
                       d.m <= 16 ? wide_fac_size(d.m) : 0, bwst, (gains_valid || debug_keep_gains) ? 1 : 0, p, nseed, R, lds ? 1 : 0);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_get_gain_factors_dev: the packed triangles of fac, unpacked in the host getter's convention (m <= 16)
  int get_gain_factors_dev(double* Fd) {
    WCHK(hipSetDevice(device));
    if (d.m > 16) WFAIL(ALTRO_ERR_UNSUPPORTED, "the one-wave-per-instance kernels keep no factors of Quu for m > 16");
    const size_t thr = (size_t)d.batch * (d.N - 1) * d.m * d.m;
    hipLaunchKernelGGL(altro::k_unpack_factors_wide, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, stream, Fd, fac, wide_fac_size(d.m), d.batch,
                       d.N, d.m);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_solution_vjp_data_dev (sensitivity_data.h; pointers and argument rules checked by the caller, the host twin
  // passes staged copies): one kernel over batch * nseed waves.  Reads what solution_sens_dev reads, the planes the handle holds
  // and -- only when an output needs them -- the active set of the last backward pass, the duals and the penalty; writes the
  // caller's outputs and eval_ws (d_k, dz_k between the sweeps) only.  Every output needs d_k: m > 16 is refused.  The active-set
  // outputs need a diagonal Hessian: generic rows are refused.
  int solution_vjp_data_dev(int nseed, altro::SensDataIO io) {
    WCHK(hipSetDevice(device));
    const bool want_set = io.gzmin || io.gzmax || io.gA || io.gB || io.gf, want3 = io.gA || io.gB || io.gf;
    if (d.m > 16) WFAIL(ALTRO_ERR_UNSUPPORTED, "the one-wave-per-instance kernels keep no factors of Quu for m > 16: no data sensitivity is available");
    if (want_set && Pn > 0)
      WFAIL(ALTRO_ERR_UNSUPPORTED, "gzmin, gzmax, gA, gB and gf need a box-only problem: with LINEAR or SOC rows the Hessian inside the active set is not diagonal");
    if (int rc = eval_ready()) return rc;
    const size_t R = (size_t)d.batch * nseed, ld = (size_t)(d.N - 1) * d.m, lz = (size_t)d.N * nz();
    WCHK(pool.reserve(&eval_ws, &eval_ws_elems, R * (ld + (want3 ? lz : 0))));
    io.dws = eval_ws;
    io.zws = want3 ? eval_ws + R * ld : nullptr;
    io.Lb = Lb; io.mu = mu; io.bslot = nullptr; io.nbp = 0; io.dt = cost_dt;
    // the accumulators of gA, gB in LDS (per_knot = 0): four waves a block while they fit the 64 KB a kernel gets unasked, else
    // one (n <= 64, m <= 16: a wave's accumulators take 65 * 80 * 8 = 41600 bytes at the most)
    const size_t acc = (!io.per_knot && (io.gA || io.gB)) ? (size_t)(d.n | 1) * nz() * sizeof(double) : 0;
    const int wpb = 4 * acc <= 65536 ? 4 : 1;
    const size_t lds = acc * wpb;
    if (lds > 65536) WFAIL(ALTRO_ERR_INTERNAL, "solution_vjp_data: the accumulators of one wave exceed 64 KB");
    hipLaunchKernelGGL(altro::k_sens_data_wide, dim3((unsigned)((R + wpb - 1) / wpb)), dim3(64 * wpb), lds, stream, io, X, U, cur, Kg, fac,
                       wide_fac_size(d.m), bwst, aset, (gains_valid || debug_keep_gains) ? 1 : 0, eval_params(), nseed, R);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_get_gain_active_set_dev: the plane of the last backward pass of aset, unpacked to one code per knot and element
  int get_gain_active_set_dev(unsigned char* codes, double* mu_pass, int32_t* fb) {
    WCHK(hipSetDevice(device));
    if (Pn > 0) WFAIL(ALTRO_ERR_UNSUPPORTED, "the active set of the stored pass is available for box-only problems");
    const size_t thr = (size_t)d.batch * d.N * nz();
    hipLaunchKernelGGL(altro::k_gain_aset_wide, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, stream, codes, mu_pass, fb, aset, bwst,
                       (gains_valid || debug_keep_gains) ? 1 : 0, mu, d.batch, d.N, d.n, d.m);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }
  // altro_batch_get_gains_dev: Kg and dg are kept in the ABI's layout
  int get_gains_dev(double* Kd, double* dd) {
    WCHK(hipSetDevice(device));
    if (Kd) WCHK(hipMemcpyAsync(Kd, Kg, (size_t)d.batch * (d.N - 1) * d.n * d.m * sizeof(double), hipMemcpyDeviceToDevice, stream));
    if (dd) WCHK(hipMemcpyAsync(dd, dg, (size_t)d.batch * (d.N - 1) * d.m * sizeof(double), hipMemcpyDeviceToDevice, stream));
    return ALTRO_OK;
  }
  int get_planes(double* Xh, double* Uh) {
    WCHK(hipSetDevice(device));
    const size_t B = d.batch, lx = (size_t)d.N * d.n, lu = (size_t)(d.N - 1) * d.m;
    int rc = ensure_stage(B * (lx + lu) * sizeof(double));
    if (rc) return rc;
    if (Xh) {
      hipLaunchKernelGGL(k_gather_plane, dim3((unsigned)((B * lx + 255) / 256)), dim3(256), 0, stream, stage, X, cur, lx, (int)B);
      WCHK(hipMemcpyAsync(Xh, stage, B * lx * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    if (Uh) {
      double* su = stage + B * lx;
      hipLaunchKernelGGL(k_gather_plane, dim3((unsigned)((B * lu + 255) / 256)), dim3(256), 0, stream, su, U, cur, lu, (int)B);
      WCHK(hipMemcpyAsync(Uh, su, B * lu * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    WCHK(hipStreamSynchronize(stream));
    return ALTRO_OK;
  }

  Params params() const {
    Params p{};
    p.B = d.batch; p.n = d.n; p.m = d.m; p.N = d.N; p.Nt = Nt; p.np = np(); p.mp = mp(); p.Pn = Pn; p.Pp = pad4(Pn);
    p.ltv = ltv; p.dyn_per_instance = dyn_per_instance;
    p.A = A; p.Bm = Bm; p.f = f; p.wd = wd; p.wf = wf; p.zmin = zmin; p.zmax = zmax; p.w_pi = w_pi; p.b_pi = b_pi;
    p.box_k0 = box_k0; p.box_k1 = box_k1;
    p.AconT = AconT; p.bcon = bcon;
    p.con_istride = con_per_instance ? (size_t)d.N * nz() * Pn : 0;
    p.bcon_istride = con_per_instance ? (size_t)d.N * Pn : 0; p.ctype = ctype; p.rowk0 = rowk0; p.rowk1 = rowk1; p.rowc0 = rowc0; p.rowcp = rowcp; p.ncone = ncone;
    p.con_static = 7;
    for (const auto& bl : blocks) p.con_static = bl.per_knot ? 0 : p.con_static;
    p.con_static &= static_mask;
    p.x0 = x0; p.Xref = Xref; p.Uref = Uref; p.X = X; p.U = U; p.cur = cur; p.Lb = Lb; p.Lc = Lc; p.mu = mu; p.Kg = Kg; p.dg = dg; p.trash = trash;
    p.iters = iters; p.iters_outer = iters_outer; p.status = status; p.cost = cost; p.cmax = cmax;
    p.Jtrace = Jtrace; p.ctrace = ctrace; p.atrace = atrace;
    p.n_backward = n_backward; p.n_rollout = n_rollout; p.n_trials = n_trials; p.n_solves = n_solves; p.n_iters = n_iters; p.n_ok = n_ok; p.n_gconf = n_gconf; p.n_gs = n_reuse; p.Qz = Qz; p.fac = fac; p.bwst = bwst; p.aset = aset; p.reuse_ok = (gains_valid || debug_keep_gains) ? 1 : 0;
    p.noise = noise; p.noise_w = noise_w; p.noise_grp = noise_grp; p.noise_mode = noise_mode; p.mpc_shift = mpc_shift;
    p.kref = kref;
    p.dyn_blocks = dyn_blocks; p.dyn_step_stride = dyn_step_stride;
    p.compact = compact();
    p.mlog = mlog;   // (the kernel writes it in MPC steps only: mpc == 1)
    p.active = flags.mask();
    p.clk = clock.args();
    p.o = o;
    if (o.projected_newton) {  // solve!(::ALTROSolver): the AL stage only has to reach the polish's tolerance
      if (o.projected_newton_tolerance >= 0) p.o.constraint_tolerance = o.projected_newton_tolerance;
      else { p.o.constraint_tolerance = 0.0; p.o.kickout_max_penalty = 1; }
    }
    return p;
  }

  // solve!(::ProjectedNewtonSolver) after the AL kernel of a plain solve: every check and allocation BEFORE the launch takes
  // its slot of the timing ring
  int polish_prepare() {
    const size_t B = d.batch;
    if (!pn_out.ran) {   // (ran last: it exists only once the other five do)
      for (double** p : {&pn_out.res, &pn_out.dres0, &pn_out.dres}) WCHK(pool.alloc(p, B, stream));
      for (int** p : {&pn_out.failed, &pn_out.dfail, &pn_out.ran}) WCHK(pool.alloc(p, B, stream));
    }
    int sides = 0;   // from the host copy of the BOX's finite sides (common to every instance)
    if (box_k1 >= box_k0)
      for (size_t j = 0; j < nz(); ++j) sides += (box_lo_fin[j] ? 1 : 0) + (box_hi_fin[j] ? 1 : 0);
    WCHK(pn_ws.alloc(pool, stream, (int)(B < 64 ? B : 64), d.N, 2 * d.n + sides + Pn, nz(), true));
    return ALTRO_OK;
  }
  // mask: the instances to polish (null: all) -- the active mask, or under an episode clock the mask of the step just solved
  int polish_launch(const int* mask) {
    altro_pnw::WParams w{};
    w.P = params();
    w.P.active = mask;
    w.P.o = o;   // the caller's tolerances (params() carries the AL stage's)
    w.out = pn_out; w.ws = pn_ws;
    hipLaunchKernelGGL(altro_pnw::pnw_kernel, dim3(pn_ws.slots), dim3(64), 0, stream, w);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }

  int compact() const {  // only for one-wave blocks: the helper waves of a cooperative block read W while wave 0 writes Qux
    if (!wide_compact(d.n, d.m, ltv, compact_np_max)) return 0;
    return wide_block_threads(d.n, d.m, (size_t)lds_layout(d.n, d.m, Pn, 1).total * sizeof(double), coop_mode) == 64 ? 1 : 0;
  }
  size_t lds_bytes() const { return (size_t)lds_layout(d.n, d.m, Pn, compact()).total * sizeof(double); }

  int prepare_launch() {
    int rc = check_ready();
    if (rc || (rc = pack_constraints())) return rc;
    con_locked = true;
    const size_t bytes = lds_bytes();
    if (bytes > 160 * 1024) WFAIL(ALTRO_ERR_UNSUPPORTED, "problem does not fit the 160 KB of LDS of one CU");
    WCHK(hipFuncSetAttribute((const void*)wide_kernel_for(d.n, d.m, Pn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    WCHK(hipFuncSetAttribute((const void*)wide_shift_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return ALTRO_OK;
  }

  int shift_fill(int primal, int dual) {
    WCHK(hipSetDevice(device));
    int rc = prepare_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(wide_shift_kernel, dim3(d.batch), dim3(64), lds_bytes(), stream, params(), primal, dual);
    WCHK(hipGetLastError());
    return ALTRO_OK;
  }

  int enqueue(int mpc, int first_step, int nsteps) {
    WCHK(hipSetDevice(device));
    int rc = prepare_launch();
    if (rc) return rc;
    // (under an episode clock every instance has a window of its own, kept inside the track and the dynamics track by the
    //  tick rule on the device)
    const int last_kref = mpc ? first_step + nsteps : kref;
    if (!clock.on && last_kref + d.N > Nt) WFAIL(ALTRO_ERR_STATE, "reference window runs past the end of the stored trajectory");
    if (mpc && ltv && dyn_step_stride == 0)
      WFAIL(ALTRO_ERR_UNSUPPORTED, "the device MPC loop over per-knot dynamics needs their table for every step: altro_mpc_set_dynamics_track");
    if (!clock.on && !dyn_covers(last_kref)) WFAIL(ALTRO_ERR_STATE, "the dynamics track ends before the last step's window");
    if (o.projected_newton && (rc = polish_prepare())) return rc;
    hipEvent_t h0, h1;
    WCHK(ring.next(&h0, &h1));
    WCHK(hipEventRecord(ev0, stream));
    WCHK(hipEventRecord(h0, stream));
    // (under an episode clock the instances idle for the whole launch are left out in the same way)
    if ((flags.on || clock.on) && !gains_valid && !debug_keep_gains)   // the instances this launch leaves out lose their stored pass too
      hipLaunchKernelGGL(k_drop_stored_pass, dim3((unsigned)((d.batch + 255) / 256)), dim3(256), 0, stream, bwst, d.batch);
    if (o.projected_newton && mpc) {
      // the steps of a fused launch as nsteps pairs of (one-step solve kernel, polish kernel): the next step's shift starts
      // from the polished trajectory and the projected multipliers, as after solve!(::ALTROSolver)
      const int kref0 = kref;
      for (int s = 0; s < nsteps && !rc; ++s) {
        const int* mask = flags.mask();
        if (clock.on) {   // the polish and the log kernel skip the instances that are idle AT THIS STEP
          hipLaunchKernelGGL(altro::k_clock_step_mask, altro::EpisodeClock::grid(d.batch), dim3(256), 0, stream, clock.stepmask, clock.args(), flags.mask(),
                             first_step + s, Nt, d.N, ltv ? dyn_blocks : 0, dyn_step_stride, d.batch);
          if (hipGetLastError() != hipSuccess) { err = "launch of the step-mask kernel failed"; rc = ALTRO_ERR_HIP; break; }
          mask = clock.stepmask;
        }
        hipLaunchKernelGGL(wide_kernel_for(d.n, d.m, Pn), dim3(d.batch), dim3(wide_block_threads(d.n, d.m, lds_bytes(), coop_mode)), lds_bytes(), stream, params(), mpc, first_step + s, 1);
        rc = hipGetLastError() == hipSuccess ? ALTRO_OK : ALTRO_ERR_HIP;
        if (rc) err = "launch of the solve kernel failed";
        gains_valid = true;   // params() of the next step: its launch may reuse the pass this one stores, as a single step would
        kref = first_step + s + 1;
        if (!rc) rc = polish_launch(mask);
        if (!rc && mlog) {
          double* rec0 = mlog + (size_t)(first_step + s) * (size_t)d.batch * mlog_rec;
          hipLaunchKernelGGL(k_log_polished_wide, dim3((unsigned)((d.batch + 255) / 256)), dim3(256), 0, stream, rec0, U, cur, cost, cmax, status,
                             mask, d.batch, d.N, d.n, d.m);
          if (hipGetLastError() != hipSuccess) { err = "launch of the log kernel failed"; rc = ALTRO_ERR_HIP; }
        }
      }
      if (rc) kref = kref0;
    } else {
      hipLaunchKernelGGL(wide_kernel_for(d.n, d.m, Pn), dim3(d.batch), dim3(wide_block_threads(d.n, d.m, lds_bytes(), coop_mode)), lds_bytes(), stream, params(), mpc, first_step, nsteps);
      rc = hipGetLastError() == hipSuccess ? ALTRO_OK : ALTRO_ERR_HIP;
      if (rc) err = "launch of the solve kernel failed";
      if (!rc && o.projected_newton) rc = polish_launch(flags.mask());
    }
    gains_valid = true;  // (until a setter changes something the stored gains depend on)
    WCHK(hipEventRecord(h1, stream));   // (every slot of the ring handed out has both events)
    if (rc) return rc;
    WCHK(hipEventRecord(ev1, stream));
    timed = true;
    if (mpc) kref = first_step + nsteps;
    return ALTRO_OK;
  }

  // altro_mpc_prepare_async: plant step + noise -> x0, reference window <- step + 1 (no shift, no solve)
  int mpc_prepare(int step) {
    if (int rcs = mpc_prepare_rules(step)) return rcs;
    if (ltv && dyn_step_stride == 0) WFAIL(ALTRO_ERR_UNSUPPORTED, "the device plant step over per-knot dynamics needs altro_mpc_set_dynamics_track");
    if (!clock.on && !dyn_covers(step + 1)) WFAIL(ALTRO_ERR_STATE, "the dynamics track ends before this step's window");
    WCHK(hipSetDevice(device));
    int rc = prepare_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(wide_kernel_for(d.n, d.m, Pn), dim3(d.batch), dim3(wide_block_threads(d.n, d.m, lds_bytes(), coop_mode)), lds_bytes(), stream, params(), 2, step, 1);
    WCHK(hipGetLastError());
    kref = step + 1;
    return ALTRO_OK;
  }

  // benchmark_solve!(solver; samples, evals): see include/altro_batch.h
  int benchmark_solve(int samples, int evals, float* sample_ms) {
    WCHK(hipSetDevice(device));
    const size_t B = d.batch, lx = (size_t)d.N * d.n, lu = (size_t)(d.N - 1) * d.m;
    if (!Xsave) WCHK(pool.alloc(&Xsave, B * lx, stream, false));
    if (!Usave) WCHK(pool.alloc(&Usave, B * lu, stream, false));
    while (bench_ev.size() < 2) {
      hipEvent_t e;
      WCHK(hipEventCreate(&e));
      bench_ev.push_back(e);
    }
    const dim3 gx((unsigned)((B * lx + 255) / 256)), gu((unsigned)((B * lu + 255) / 256));
    hipLaunchKernelGGL(k_gather_plane, gx, dim3(256), 0, stream, Xsave, X, cur, lx, (int)B);  // Z0 = copy(get_trajectory(solver))
    hipLaunchKernelGGL(k_gather_plane, gu, dim3(256), 0, stream, Usave, U, cur, lu, (int)B);
    WCHK(hipGetLastError());
    auto one = [&]() -> int {  // initial_trajectory!(solver, Z0); solve!(solver)
      hipLaunchKernelGGL(k_scatter_plane, gx, dim3(256), 0, stream, X, Xsave, cur, lx, (int)B);
      hipLaunchKernelGGL(k_scatter_plane, gu, dim3(256), 0, stream, U, Usave, cur, lu, (int)B);
      gains_valid = false;   // every evaluation recomputes its gains, as the reference's `@benchmark solve!` does
      return enqueue(0, 0, 0);
    };
    int rc = one();  // BenchmarkTools' warm-up evaluation
    if (rc) return rc;
    for (int s_ = 0; s_ < samples; ++s_) {
      WCHK(hipEventRecord(bench_ev[0], stream));
      for (int e = 0; e < evals; ++e)
        if ((rc = one())) return rc;
      WCHK(hipEventRecord(bench_ev[1], stream));
      WCHK(hipEventSynchronize(bench_ev[1]));
      float ms = 0.f;
      WCHK(hipEventElapsedTime(&ms, bench_ev[0], bench_ev[1]));
      if (sample_ms) sample_ms[s_] = ms / (float)evals;
    }
    WCHK(hipStreamSynchronize(stream));
    return ALTRO_OK;
  }

  // altro_batch_restart_instances(_dev): which [B], Xs [B][N][n] (may be null), Us [B][N-1][m]; dev: device arrays, already
  // validated, read where they are and nothing synchronises; else host arrays through the staging buffer
  int restart(const int32_t* which, const double* Xs, const double* Us, bool dev) {
    WCHK(hipSetDevice(device));
    int rc = pack_constraints();   // (before the first solve: the dual rows of constraints added so far must exist)
    if (rc) return rc;
    const size_t B = d.batch, lx = (size_t)d.N * d.n, lu = (size_t)(d.N - 1) * d.m;
    if (!dev) {
      if ((rc = ensure_stage(B * (lx + lu) * sizeof(double)))) return rc;
      if (Xs) WCHK(hipMemcpyAsync(stage, Xs, B * lx * sizeof(double), hipMemcpyHostToDevice, stream));
      WCHK(hipMemcpyAsync(stage + B * lx, Us, B * lu * sizeof(double), hipMemcpyHostToDevice, stream));
      Xs = Xs ? stage : nullptr;
      Us = stage + B * lx;
    }
    WCHK(flags.load(true, which, dev, (int)B, (int)B, stream));
    hipLaunchKernelGGL(k_restart_wide, dim3((unsigned)B), dim3(64), 0, stream, flags.which, Xs, Us, params());
    WCHK(hipGetLastError());
    if (!dev) WCHK(hipStreamSynchronize(stream));
    return ALTRO_OK;
  }

  int duals(int con_id, double* lam, bool set) {
    WCHK(hipSetDevice(device));
    WCHK(hipStreamSynchronize(stream));
    int rc = pack_constraints();
    if (rc) return rc;
    const size_t B = d.batch, N = d.N, z = nz();
    if (con_id == box_id && box_id >= 0) {
      const size_t nk = box_k1 - box_k0 + 1, w = nk * 2 * z * sizeof(double), pitch = N * 2 * z * sizeof(double);
      double* base = Lb + (size_t)box_k0 * 2 * z;
      if (set) WCHK(hipMemcpy2D(base, pitch, lam, w, w, B, hipMemcpyHostToDevice));
      else WCHK(hipMemcpy2D(lam, w, base, pitch, w, B, hipMemcpyDeviceToHost));
      return ALTRO_OK;
    }
    Block* bl = find(con_id);
    if (!bl) WFAIL(ALTRO_ERR_INVALID_ARG, "no such constraint");
    std::vector<double> all(B * N * Pn);
    WCHK(hipMemcpy(all.data(), Lc, all.size() * sizeof(double), hipMemcpyDeviceToHost));
    const size_t nk = bl->k1 - bl->k0 + 1;
    for (size_t b = 0; b < B; ++b)
      for (size_t kk = 0; kk < nk; ++kk)
        for (int r = 0; r < bl->p; ++r) {
          double& dv = all[(b * N + bl->k0 + kk) * Pn + bl->r0 + r];
          double& hv = lam[(b * nk + kk) * bl->p + r];
          if (set) dv = hv; else hv = dv;
        }
    if (set) WCHK(hipMemcpy(Lc, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice));
    return ALTRO_OK;
  }

  int get_gains(double* K, double* dd) {
    WCHK(hipSetDevice(device));
    WCHK(hipStreamSynchronize(stream));
    if (K) WCHK(hipMemcpy(K, Kg, (size_t)d.batch * (d.N - 1) * d.n * d.m * sizeof(double), hipMemcpyDeviceToHost));
    if (dd) WCHK(hipMemcpy(dd, dg, (size_t)d.batch * (d.N - 1) * d.m * sizeof(double), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }

  int mpc_set_track(const double* Xt, const double* Ut, int Nt_) {
    int rc = set_ref_common(Xt, Ut, Nt_);
    if (rc) return rc;
    // initial_trajectory!(prob, Z): the first window of the track; x0 = its first knot (mpc.jl:19-20,45)
    const size_t B = d.batch, N = d.N, n = d.n, m = d.m;
    std::vector<double> Xw(B * N * n), Uw(B * (N - 1) * m), xs(B * n);
    for (size_t b = 0; b < B; ++b) {
      std::copy(Xt + b * Nt_ * n, Xt + b * Nt_ * n + N * n, Xw.begin() + b * N * n);
      std::copy(Ut + b * (Nt_ - 1) * m, Ut + b * (Nt_ - 1) * m + (N - 1) * m, Uw.begin() + b * (N - 1) * m);
      std::copy(Xt + b * Nt_ * n, Xt + b * Nt_ * n + n, xs.begin() + b * n);
    }
    if ((rc = put_planes(Xw.data(), Uw.data()))) return rc;
    return set_initial_state(xs.data());
  }
};

#undef WCHK
#undef WFAIL

}  // namespace altro_wide
