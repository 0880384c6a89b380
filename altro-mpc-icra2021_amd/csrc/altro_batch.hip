// altro_batch.hip -- C-ABI (include/altro_batch.h) of the MI355X batched ALTRO solver.
//
// Host logic only: owns device memory (lane layout, DESIGN.md "Data layout in HBM"), converts
// the caller's instance-major host arrays to/from it with small pack kernels, and launches the
// solve kernel of solve_dpp16.h.  There is no CPU compute path in this library: every entry
// point that computes launches HIP kernels, and creation fails if no HIP device is usable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/altro_batch.h"
#include "device_io.h"
#include "device_pool.h"
#include "evaluate.h"
#include "evaluate_grad.h"
#include "evaluate_al.h"
#include "sensitivity_data.h"
#include "cost_to_go.h"
#include "launch_ring.h"
#include "pn_polish.h"
#include "policy.h"
#include "solve_dpp16.h"
#include "stage_layout.h"
#include "warm_start.h"
#include "simulate.h"
// The one-wave-per-instance kernels are compiled in translation units of their own (wide_inst.hip, _lib.build) and only
// declared here; -DALTRO_WIDE_SINGLE_TU (and the development builds) instantiate them in this unit as before.
#if !defined(ALTRO_WIDE_SINGLE_TU) && !defined(ALTRO_DEV_HEADLINE_ONLY)
#define ALTRO_WIDE_EXTERN
#endif
#include "wide_backend.h"

using altro::IPW;
using altro::LW;

static thread_local std::string g_create_err;

// Diagnostic switches (altro_debug_set, include/altro_batch.h).  The library reads NOTHING from the environment: a test or
// a measuring tool that wants a scheduling feature off says so through the entry point -- with a null handle for the
// handles this thread creates afterwards, with a handle for that handle.
struct DebugSwitches {
  int lone = 1, pair = 1, shadow = 1, resync = 1, reuse = 1, useqz = 1, mate = 1;
  int group = 1;             // 0 off, 1 sorted, 2-4: other slot orders (k_group_rank)
  int group_max_steps = 32;
  int dbg_wave = -1;         // "trace_wave": -DALTRO_PHASE_STAMPS builds
  int force_wide = 0;        // every (n, m) on the one-wave-per-instance backend
  int keep_gains = 0;        // -DALTRO_DEBUG builds only: the setters do NOT drop the stored gains (exists to show that the
                             // tests notice stale gains)
  int wide_compact = -1, wide_coop = -1, wide_static_mask = -1;   // -1: the backend's default
};
static thread_local DebugSwitches g_dbg;
// key -> member.  negate: a "no_x" key switches the feature x off; at_create: read when a handle is created, refused on one
struct SwitchKey {
  const char* key;
  int DebugSwitches::*member;
  bool negate, at_create;
};
static const SwitchKey kSwitchKeys[] = {
    {"no_lone", &DebugSwitches::lone, true, false},        // backward_split<4> (tests: lone == four-row pass bit for bit)
    {"no_pair", &DebugSwitches::pair, true, false},        // backward_split<2>: two rows need a pass
    {"no_qz_pass", &DebugSwitches::useqz, true, false},    // backward passes always recompute their cost / box expansion
    {"no_shadow", &DebugSwitches::shadow, true, false},    // rows that sit a phase out keep their own instance
    {"no_resync", &DebugSwitches::resync, true, false},    // rows never wait for their wave-mates
    {"no_mate_rank", &DebugSwitches::mate, true, false},   // issue priority from the row's own state only
    {"no_reuse", &DebugSwitches::reuse, true, false},      // gain reuse (solve_dpp16.h fosweep)
    {"no_group", &DebugSwitches::group, true, false},      // fused MPC launches run in instance order
    {"group_mode", &DebugSwitches::group, false, false},
    {"group_max_steps", &DebugSwitches::group_max_steps, false, false},   // fused launches of more steps are not grouped
    {"trace_wave", &DebugSwitches::dbg_wave, false, false},
    {"keep_gains", &DebugSwitches::keep_gains, false, false},
    {"force_wide", &DebugSwitches::force_wide, false, true},
    {"wide_compact", &DebugSwitches::wide_compact, false, true},
    {"wide_coop", &DebugSwitches::wide_coop, false, true},
    {"wide_static_mask", &DebugSwitches::wide_static_mask, false, true},
};

struct altro_handle : altro::BackendCommon {   // what both backends hold and do alike: backend_common.h (on a wide handle
                                                // the copy here keeps d, o, device and err, its arrays are never allocated)
  altro_wide::WideBackend* wide = nullptr;  // set: this handle runs on the one-wave-per-instance kernel
  DebugSwitches sw;                         // the switches as they were when the handle was created, then altro_debug_set(h, ..)
  int Bp = 0;  // batch padded to a multiple of IPW (= slots)
  double* Zsave = nullptr;       // [Bp][N][16]: Z0 of altro_batch_benchmark_solve
  hipEvent_t bev0 = nullptr, bev1 = nullptr;
  long long* wave_cycles = nullptr;
  int* dzero = nullptr;  // [Bp] the last iteration of the last solve was costate-confirmed: its d is zero
  // problem data (device)
  double *Gcol = nullptr, *Grow = nullptr, *fvec = nullptr;
  double *wd = nullptr, *wf = nullptr, *zmin = nullptr, *zmax = nullptr;  // [16] each, or [Bp][16] (tab_rows)
  // host copies of the cost weights and bounds: [rows][16] each, rows = 1 (shared by the batch) or batch (per instance)
  std::vector<double> wd_h, wf_h, zmin_h, zmax_h;
  bool bnd_stale = false;                // altro_batch_set_bounds_dev wrote the device rows: zmin_h / zmax_h are refreshed before use
  bool cost_pi = false, bnd_pi = false;  // per-instance cost weights / bounds: the device tables then hold Bp rows (imask)
  int tab_cap = 1;                       // rows the device tables have room for
  bool box_lo_fin[LW] = {}, box_hi_fin[LW] = {};  // finite sides of the BOX as it was added (altro_batch_set_bounds)
  double *x0 = nullptr, *Zref = nullptr, *Z = nullptr, *Lb = nullptr, *mu = nullptr,
         *KD = nullptr, *Qz = nullptr, *Dff = nullptr, *kmu = nullptr;
  altro::ASet* ahash = nullptr;  // [Bp][16] active set of the backward pass behind the gains in KD (gain reuse, solve_dpp16.h)
  bool d_in_kd = false;  // the last solve launch's kernel keeps d in the gain rows (altro::kd_holds_d), not in Dff
  int* cur = nullptr;
  int *perm = nullptr, *gscore = nullptr;  // [Bp] wave slot -> instance of a grouped MPC launch, and its sort key
  unsigned* simd_tab = nullptr;            // [65536][16], zero between launches
  altro::StreamLink link;   // events of altro_batch_wait_stream / altro_batch_signal_stream (device_io.h)
  int dev_via_stage = 0;    // "dev_via_stage": the _dev setters of x0 and the reference copy into `stage` first (measurement only)
  // generic affine constraints packed into 4 quads of 4 constraint rows (see solve_dpp16.h)
  double *Acon = nullptr, *bcon = nullptr, *Lc = nullptr;
  int* cmeta = nullptr;
  int* ckn = nullptr;   // [16] canonical knot of each constraint lane (time-invariant tables, see pack_constraints)
  int con_inv = 0;
  std::vector<double> Acon_h, bcon_h;  // per-knot tables [ninst][N][16][16], [ninst][N][16]; ninst = 1 (shared) or Bp
  bool con_per_instance = false;
  size_t acon_elems = 0;               // elements the device table Acon currently holds
  std::vector<int> cmeta_h;            // [N][16][4]
  int ncrows = 0;       // 16 once any generic constraint exists (kernel flag)
  bool con_dirty = false, con_locked = false;  // packing is redone until the first solve
  struct ConBlock {
    int id, kind, sense, k0, k1, p;
    int per_knot, per_instance;
    std::vector<double> A, b;  // A row-major p x nz blocks: [instance if per_instance][knot of the range if per_knot]
    int lanes[LW];
    bool stale = false;        // altro_batch_update_constraint_data_dev wrote the device rows: A, b are refreshed before use
  };
  std::vector<ConBlock> cons;
  int* lanebuf = nullptr;  // device scratch [16] for dual transfers
  int* bslot = nullptr;  // device [16]
  int bslot_h[LW];       // host copy: slot of z element j among the bounded ones, -1 if none
  int nbp = 1;           // slots per side of the compact dual rows
  int ncon = 0;
  bool have_x0 = false;
  double dt = 0.0;
};

// What the shared entry points act on: the backend the handle runs on.  They check their arguments, then
// `return fwd(h, common(h).get_stats(..))`; fwd is the one place where a wide backend's message reaches altro_last_error.
static altro::BackendCommon& common(altro_handle* h) {
  if (h->wide) return *h->wide;
  return *h;
}
static int fwd(altro_handle* h, int rc) {
  if (rc && h->wide) h->err = h->wide->err;
  return rc;
}

#define HIPCHK(h, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
      return ALTRO_ERR_HIP;                                                               \
    }                                                                                     \
  } while (0)

#define FAIL(h, code, msg) \
  do {                     \
    (h)->err = (msg);      \
    return (code);         \
  } while (0)

// forward an entry point to the wide backend when the handle runs on it: always AFTER the handle and the arguments are checked
#define WIDE_FWD(h, call)                                  \
  do {                                                     \
    if ((h)->wide) return fwd(h, (h)->wide->call);         \
  } while (0)

// ------------------------------------------------------------------ layout kernels
// All take one thread per (instance slot, lane); padded slots mirror instance B-1.

__global__ void k_pack_traj(const double* __restrict__ X, const double* __restrict__ U, double* __restrict__ Zp,
                            const int* __restrict__ cur, size_t plane, int B, int Bp, int N, int n, int m,
                            int use_cur, int have_x) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bp * LW) return;
  const int inst = t / LW, j = t % LW;
  const int b = inst < B ? inst : B - 1;
  double* dst = Zp + (size_t)inst * (2 * (size_t)N + 1) * LW + (use_cur ? (size_t)cur[inst] * plane : 0);
  for (int k = 0; k < N; ++k) {
    double v = 0.0;
    bool wr = false;
    if (j < n) {
      if (have_x) { v = X[((size_t)b * N + k) * n + j]; wr = true; }
    } else if (j < n + m) {
      if (k < N - 1) v = U[((size_t)b * (N - 1) + k) * m + (j - n)];
      wr = true;
    } else {
      wr = true;
    }
    if (wr) dst[(size_t)k * LW + j] = v;
  }
}

__global__ void k_unpack_traj(double* __restrict__ X, double* __restrict__ U, const double* __restrict__ Zp,
                              const int* __restrict__ cur, size_t plane, int B, int Bp, int N, int n, int m) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * LW) return;
  const int inst = t / LW, j = t % LW;
  const double* src = Zp + (size_t)inst * (2 * (size_t)N + 1) * LW + (size_t)cur[inst] * plane;
  for (int k = 0; k < N; ++k) {
    const double v = src[(size_t)k * LW + j];
    if (j < n) {
      if (X) X[((size_t)inst * N + k) * n + j] = v;
    } else if (j < n + m && k < N - 1) {
      if (U) U[((size_t)inst * (N - 1) + k) * m + (j - n)] = v;
    }
  }
}

// reference: Xref [B][Nt][n], Uref [B][Nt-1][m] -> Zref [Bp][Nt][16]
__global__ void k_pack_ref(const double* __restrict__ X, const double* __restrict__ U, double* __restrict__ Zr,
                           int B, int Bp, int Nt, int n, int m) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bp * LW) return;
  const int inst = t / LW, j = t % LW;
  const int b = inst < B ? inst : B - 1;
  for (int k = 0; k < Nt; ++k) {
    double v = 0.0;
    if (j < n) v = X[((size_t)b * Nt + k) * n + j];
    else if (j < n + m && k < Nt - 1) v = U[((size_t)b * (Nt - 1) + k) * m + (j - n)];
    Zr[((size_t)inst * Nt + k) * LW + j] = v;
  }
}

// dynamics: A [nb][n*n] col-major, Bm [nb][n*m] col-major, f [nb][n]; nb = B or 1
__global__ void k_pack_dyn(const double* __restrict__ A, const double* __restrict__ Bm, const double* __restrict__ f,
                           double* __restrict__ Gcol, double* __restrict__ Grow, double* __restrict__ fvec,
                           int B, int Bp, int n, int m, int per_instance) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bp * LW) return;
  const int inst = t / LW, j = t % LW;
  const int b = per_instance ? (inst < B ? inst : B - 1) : 0;
  const double* Ab = A + (size_t)b * n * n;
  const double* Bb = Bm + (size_t)b * n * m;
  // Gcol[inst][k][j] = G[k][j], G = [A B]
  for (int k = 0; k < n; ++k) {
    double v = 0.0;
    if (j < n) v = Ab[k + n * j];
    else if (j < n + m) v = Bb[k + n * (j - n)];
    Gcol[((size_t)inst * n + k) * LW + j] = v;
  }
  // Grow[inst][c][i=j] = G[j][c]
  for (int c = 0; c < LW; ++c) {
    double v = 0.0;
    if (j < n) {
      if (c < n) v = Ab[j + n * c];
      else if (c < n + m) v = Bb[j + n * (c - n)];
    }
    Grow[((size_t)inst * LW + c) * LW + j] = v;
  }
  fvec[(size_t)inst * LW + j] = (f && j < n) ? f[(size_t)b * n + j] : 0.0;
}

__global__ void k_pack_x0(const double* __restrict__ x0, double* __restrict__ dst, int B, int Bp, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bp * LW) return;
  const int inst = t / LW, j = t % LW;
  const int b = inst < B ? inst : B - 1;
  dst[t] = j < n ? x0[(size_t)b * n + j] : 0.0;
}

__global__ void k_unpack_x0(double* __restrict__ x0, const double* __restrict__ src, int B, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * LW) return;
  const int inst = t / LW, j = t % LW;
  if (j < n) x0[(size_t)inst * n + j] = src[t];
}

// box duals: host [B][nk][2][nz] (dense, zero for unbounded elements)  <->  Lb [Bp][N+1][2][nbp]
__global__ void k_duals(double* __restrict__ host, double* __restrict__ Lb, const int* __restrict__ bslot, int nbp,
                        int B, int Bp, int N, int nz, int k0, int k1, int to_host) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bp * LW) return;
  const int inst = t / LW, j = t % LW;
  if (j >= nz) return;
  const int b = inst < B ? inst : B - 1;
  const int nk = k1 - k0 + 1;
  const int sl = bslot[j];
  for (int k = k0; k <= k1; ++k) {
    const size_t hi = (((size_t)b * nk + (k - k0)) * 2 + 0) * nz + j;
    const size_t lo = (((size_t)b * nk + (k - k0)) * 2 + 1) * nz + j;
    const size_t dh = (((size_t)inst * (N + 1) + k) * 2 + 0) * nbp + (sl >= 0 ? sl : 0);
    const size_t dl = (((size_t)inst * (N + 1) + k) * 2 + 1) * nbp + (sl >= 0 ? sl : 0);
    if (to_host) {
      if (inst < B) { host[hi] = sl >= 0 ? Lb[dh] : 0.0; host[lo] = sl >= 0 ? Lb[dl] : 0.0; }
    } else if (sl >= 0) {
      Lb[dh] = host[hi];
      Lb[dl] = host[lo];
    }
  }
}

// MPC log, projected_newton = 1: the solve kernel of a step's pair wrote the step's records, then the polish kernel moved the
// trajectory and, where it ran, replaced cost / c_max / status.  The records take what the handle holds now: u0 <- first
// control of the polished trajectory, and the three statistics altro_batch_get_stats reports after the step.
// rec0 = the step's first record; one thread per instance.
__global__ void k_log_polished(double* __restrict__ rec0, const double* __restrict__ Zp, const int* __restrict__ cur, size_t plane,
                               const double* __restrict__ cost, const double* __restrict__ cmax, const int* __restrict__ status,
                               const int* __restrict__ active, int B, int N, int n, int m) {
  const int inst = blockIdx.x * blockDim.x + threadIdx.x;
  if (inst >= B) return;
  if (active != nullptr && active[inst] == 0) return;  // the solve kernel wrote no record: the slot stays "never written"
  double* r = rec0 + (size_t)inst * (LW + altro::MLOG_TAIL);
  const double* z0 = Zp + (size_t)inst * (2 * (size_t)N + 1) * LW + (size_t)cur[inst] * plane;
  for (int a = 0; a < m; ++a) r[n + a] = z0[n + a];
  r[LW] = cost[inst];
  r[LW + 1] = cmax[inst];
  reinterpret_cast<int*>(r + LW + 2)[2] = status[inst];
}

// RD.shift_fill!(Z) on the current plane and Altro.shift_fill!(conSet) on the box duals
// (random_linear_problem.jl:136,139): entry k <- entry k+1, last entry kept.
__global__ void k_shift(double* __restrict__ Zp, const int* __restrict__ cur, size_t plane, double* __restrict__ Lb,
                        int nbp, int Bp, int N, int n, int m, int k0, int k1, int primal, int dual,
                        double* __restrict__ Lc, const int* __restrict__ cmeta, int ncrows, const int* __restrict__ active) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bp * LW) return;
  const int inst = t / LW, j = t % LW;
  if (active != nullptr && active[inst] == 0) return;  // altro_batch_set_active: an inactive instance is not shifted
  const size_t ks = LW;  // rows of an instance are consecutive (instance-major arrays)
  if (primal) {
    double* z = Zp + (size_t)inst * (2 * (size_t)N + 1) * LW + (size_t)cur[inst] * plane + j;
    const int kend = (j < n) ? N - 1 : N - 2;  // x: knots 0..N-2 take k+1; u: knots 0..N-3
    if (j < n + m)
      for (int k = 0; k < kend; ++k) z[(size_t)k * ks] = z[(size_t)(k + 1) * ks];
  }
  if (dual && k1 >= k0) {  // the 16 threads of the instance share the 2*nbp elements of its compact rows
    const size_t ls = (size_t)2 * nbp;
    for (int e = j; e < 2 * nbp; e += LW) {
      double* l = Lb + (size_t)inst * (N + 1) * 2 * nbp + e;
      for (int k = k0; k < k1; ++k) l[(size_t)k * ls] = l[(size_t)(k + 1) * ls];
    }
  }
  if (dual && j < ncrows) {  // generic constraint rows on lane j: each constraint shifts inside its own range
    double* lc = Lc + (size_t)inst * (N + 1) * LW + j;
    for (int k = 0; k < N - 1; ++k) {
      const int* cm = cmeta + ((size_t)k * LW + j) * 4;
      if (cm[0] != 0 && k < cm[2]) lc[(size_t)k * ks] = lc[(size_t)(k + 1) * ks];
    }
  }
}

// altro_batch_restart_instances: the instances `which` selects go back to what a freshly created handle holds, with (X, U) as
// their trajectory.  One thread per (instance, lane), the rows of k_pack_traj for the current plane; then the instance's box
// and constraint-row duals <- 0 (trash rows included), penalty <- the 1.0 a new handle starts from (a solve with
// reset_penalties = 1 begins at penalty_initial either way), no stored gains (kmu < 0, active set cleared, dzero = 0), and
// the statistics of an instance that has not been solved.  The accumulating counters stay.
__global__ void k_restart(const int* __restrict__ which, const double* __restrict__ X, const double* __restrict__ U,
                          double* __restrict__ Zp, const int* __restrict__ cur, size_t plane, double* __restrict__ Lb, int nbp,
                          double* __restrict__ Lc, double* __restrict__ mu, double* __restrict__ kmu, altro::ASet* __restrict__ ahash,
                          int* __restrict__ dzero, int* __restrict__ iters, int* __restrict__ iters_outer, int* __restrict__ status,
                          double* __restrict__ cost, double* __restrict__ cmax, double* __restrict__ Jtrace, double* __restrict__ ctrace,
                          double* __restrict__ atrace, int* __restrict__ window, int B, int N, int n, int m, int have_x) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * LW) return;
  const int inst = t / LW, j = t % LW;
  if (which[inst] == 0) return;
  double* dst = Zp + (size_t)inst * (2 * (size_t)N + 1) * LW + (size_t)cur[inst] * plane;
  for (int k = 0; k < N; ++k) {
    if (j < n) {
      if (have_x) dst[(size_t)k * LW + j] = X[((size_t)inst * N + k) * n + j];
    } else {
      dst[(size_t)k * LW + j] = (j < n + m && k < N - 1) ? U[((size_t)inst * (N - 1) + k) * m + (j - n)] : 0.0;
    }
  }
  double* lb = Lb + (size_t)inst * (N + 1) * 2 * nbp;
  for (int e = j; e < (N + 1) * 2 * nbp; e += LW) lb[e] = 0.0;
  double* lc = Lc + (size_t)inst * (N + 1) * LW;
  for (int k = 0; k <= N; ++k) lc[(size_t)k * LW + j] = 0.0;
  altro::ASet z{};
  ahash[(size_t)inst * LW + j] = z;
  static_assert(ALTRO_TRACE_LEN == LW, "one trace entry per lane");
  Jtrace[(size_t)inst * ALTRO_TRACE_LEN + j] = 0.0;
  ctrace[(size_t)inst * ALTRO_TRACE_LEN + j] = 0.0;
  atrace[(size_t)inst * ALTRO_TRACE_LEN + j] = 0.0;
  if (j == 0) {
    mu[inst] = 1.0;
    kmu[inst] = -1.0;
    dzero[inst] = 0;
    iters[inst] = 0;
    iters_outer[inst] = 0;
    status[inst] = ALTRO_UNSOLVED;
    cost[inst] = 0.0;
    cmax[inst] = 0.0;
    if (window != nullptr) window[inst] = 0;   // under an episode clock (altro_mpc_set_clock): back to the track's first window
  }
}

// duals of one generic constraint block: host [B][nk][p]  <->  Lc [Bp][N+1][16], rows on lanes lane0..lane0+p-1
__global__ void k_cduals(double* __restrict__ host, double* __restrict__ Lc, int B, int N, const int* __restrict__ lanes,
                         int p, int k0, int k1, int to_host) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * p) return;
  const int inst = t / p, r = t % p;
  const int nk = k1 - k0 + 1;
  for (int k = k0; k <= k1; ++k) {
    const size_t hi = ((size_t)inst * nk + (k - k0)) * p + r;
    const size_t di = ((size_t)inst * (N + 1) + k) * LW + lanes[r];
    if (to_host) host[hi] = Lc[di];
    else Lc[di] = host[hi];
  }
}

// benchmark_solve!: Z0 = copy(get_trajectory(solver)) and initial_trajectory!(solver, Z0) on the current plane
__global__ void k_plane_copy(double* __restrict__ Zp, double* __restrict__ Zs, const int* __restrict__ cur, size_t plane,
                             int Bp, int N, int save) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bp * LW) return;
  const int inst = t / LW, j = t % LW;
  double* z = Zp + (size_t)inst * (2 * (size_t)N + 1) * LW + (size_t)cur[inst] * plane + j;
  double* zs = Zs + (size_t)inst * N * LW + j;
  for (int k = 0; k < N; ++k) {
    if (save) zs[(size_t)k * LW] = z[(size_t)k * LW];
    else z[(size_t)k * LW] = zs[(size_t)k * LW];
  }
}

// ---- grouping of the instances of a fused MPC launch (solve_dpp16.h: a wave executes the union of the phases its
// four rows need, so rows with the same needs belong in the same wave).  Whether an instance will need backward
// passes is decided by whether its window holds an active box row: then the active set moves with the window from one
// step to the next and the gains cannot be taken from memory (47 % of the headline's instances need no pass in 20
// steps, 40 % one at nearly every step; tools/gpu_class_persist.py).  The tracking problem follows its reference, so
// the REFERENCE tells which windows those are: score = number of the launch's steps whose window holds a reference
// knot at (or within 2 % of) a bound.  It is a scheduling heuristic only: results do not depend on which rows share a
// wave (tests: instance results do not depend on the batch; lone-row == four-row pass bit for bit).
// one 16-lane row per instance (lane j = element j of z: coalesced 128-byte reads), 16 instances per block
constexpr int GROUP_BINS = 34;   // scores 0 .. 32 of the active instances, and one bin behind them for the inactive ones
__global__ void k_group_score(const double* __restrict__ Zref, const double* __restrict__ zmin, const double* __restrict__ zmax,
                              unsigned imask, int* __restrict__ score, int Bp, int Nt, int first, int nsteps, int k0, int k1, int nz,
                              const int* __restrict__ active, altro::ClockArgs clk, int N) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = t / LW, j = t % LW;
  const bool live = b < Bp;
  const int bb = live ? b : Bp - 1;
  bool off = active != nullptr && active[bb] == 0;   // the instance takes no step of this launch: the last bin
  if (clk.start != nullptr) {
    // episode clock: the windows of the instance are those of its own local steps, and only the steps it ticks count
    // (row-uniform: the sixteen lanes of an instance take the same path, and the ballots below look at their own row only)
    int lo, hi;
    altro::clock_span(clk.start[bb], altro::clock_lmax(clk.length[bb], Nt, N, 0, 0), first, nsteps, lo, hi);
    const bool ticks = hi > lo;   // (then 0 <= first + lo - start < Nt: computed only then, any int32 start is safe)
    first = ticks ? (int)((long long)first + lo - clk.start[bb]) : 0;
    nsteps = ticks ? hi - lo : 0;
    off = off || !ticks;
  }
  const int W = k1 - k0 + 1;                 // knots of a window that carry the box rows
  const int a0 = first + 1 + k0;             // first absolute knot touched by the launch's windows
  const int na = nsteps + W - 1;             // absolute knots touched
  if (na > 256 || W < 1 || nsteps == 0) { if (live && j == 0) score[b] = off ? GROUP_BINS - 1 : 0; return; }
  const unsigned bo = ((unsigned)bb * LW + j) & imask;   // the instance's row of per-instance bounds (SolveParams::imask)
  const double lo = zmin[bo], hi = zmax[bo];
  const bool fl = (j < nz) && lo > -1e300, fh = (j < nz) && hi < 1e300;
  const double m = 0.02 * ((fl && fh) ? 0.5 * (hi - lo) : fmax(1.0, fabs(fh ? hi : lo)));
  unsigned long long bits[4] = {0ull, 0ull, 0ull, 0ull};
  const int sh = (threadIdx.x & 63) & ~15;   // this row's 16 bits of the wave's ballot
  for (int a = 0; a < na; ++a) {
    const double z = Zref[((size_t)bb * Nt + (a0 + a)) * LW + j];
    const bool act = (fh && z >= hi - m) || (fl && z <= lo + m);
    const bool any = ((__ballot(act) >> sh) & 0xFFFFull) != 0ull;
    if (any) bits[a >> 6] |= 1ull << (a & 63);
  }
  if (!live || j != 0) return;
  int cnt = 0, sc = 0;
  for (int a = 0; a < W; ++a) cnt += (int)((bits[a >> 6] >> (a & 63)) & 1ull);
  for (int st = 0; st < nsteps; ++st) {
    sc += cnt > 0 ? 1 : 0;
    const int out = st, in = st + W;
    cnt -= (int)((bits[out >> 6] >> (out & 63)) & 1ull);
    if (in < na) cnt += (int)((bits[in >> 6] >> (in & 63)) & 1ull);
  }
  // (active scores stay below the last bin, which belongs to the inactive instances of a masked launch: they sort behind
  //  everything else, four to a wave, and those waves leave at their first step begin)
  sc = sc < GROUP_BINS - 2 ? sc : GROUP_BINS - 2;
  score[b] = off ? GROUP_BINS - 1 : sc;
}

// perm = the instances in ascending order of (score, index): a stable counting sort in ONE block of 256 threads (thread t
// owns a contiguous chunk of instances; scores are at most GROUP_BINS - 1 = the steps of a grouped launch)
__global__ void __launch_bounds__(256) k_group_rank(const int* __restrict__ score, int* __restrict__ perm, int Bp, int mode) {
  __shared__ int cnt[GROUP_BINS][257];
  __shared__ int base[GROUP_BINS + 1];
  const int t = threadIdx.x;
  const int chunk = (Bp + 255) / 256;
  const int i0 = t * chunk, i1 = (i0 + chunk < Bp) ? i0 + chunk : Bp;
  for (int b = 0; b < GROUP_BINS; ++b) cnt[b][t] = 0;
  for (int i = i0; i < i1; ++i) {
    const int sc = score[i] < GROUP_BINS - 1 ? score[i] : GROUP_BINS - 1;
    cnt[sc][t] += 1;
  }
  __syncthreads();
  if (t < GROUP_BINS) {  // exclusive prefix over the threads, per bin
    int acc = 0;
    for (int q = 0; q < 256; ++q) {
      const int c = cnt[t][q];
      cnt[t][q] = acc;
      acc += c;
    }
    cnt[t][256] = acc;
  }
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int b = 0; b < GROUP_BINS; ++b) { base[b] = acc; acc += cnt[b][256]; }
  }
  __syncthreads();
  const int W = Bp / 4;
  int off[GROUP_BINS];
  for (int b = 0; b < GROUP_BINS; ++b) off[b] = base[b] + cnt[b][t];
  for (int i = i0; i < i1; ++i) {
    const int sc = score[i] < GROUP_BINS - 1 ? score[i] : GROUP_BINS - 1;
    const int rank = off[sc]++;
    int slot = rank;                                  // mode 1: sorted, the instances with the fewest expected passes first
    if (mode == 2) {                                  // sorted waves, light and heavy ones alternating in the block order
      const int wr = rank / 4, q = rank % 4;          // (a permutation for odd W too: the lighter (W + 1) / 2 take the even slots)
      slot = ((wr < (W + 1) / 2) ? 2 * wr : 2 * (W - 1 - wr) + 1) * 4 + q;
    } else if (mode == 3) {                           // every wave gets one instance of each quartile
      slot = (rank % W) * 4 + rank / W;
    } else if (mode == 4) {                           // sorted waves, the upper half in DESCENDING order: with W = 2 waves per
      const int wr = rank / 4, q = rank % 4;          // SIMD the dispatcher puts blocks i and i + W / 2 on one SIMD, so the
      const int hw = (W + 1) / 2;                     // wave with the most expected passes shares its SIMD with the one
      slot = ((wr < hw) ? wr : hw + (W - 1 - wr)) * 4 + q;   // with the fewest (min-max pairing), not with a middle one
    }
    perm[slot] = i;
  }
}

// initial_trajectory!(prob, Z): plane 0 of Z <- the first N knots of the track (mpc.jl:19-20,45)
__global__ void k_window_copy(double* __restrict__ Zp, const double* __restrict__ Zr, int Bp, int N, int Nt) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bp * LW) return;
  const int inst = t / LW, j = t % LW;
  double* z = Zp + (size_t)inst * (2 * (size_t)N + 1) * LW + j;
  const double* r = Zr + (size_t)inst * Nt * LW + j;
  for (int k = 0; k < N; ++k) z[(size_t)k * LW] = r[(size_t)k * LW];
}

__global__ void k_fill(double* p, double v, size_t nelem) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nelem) p[t] = v;
}

// ------------------------------------------------------------------ helpers
static inline dim3 grid_for(size_t threads, int block = 256) { return dim3((unsigned)((threads + block - 1) / block)); }

static bool supported_dims(int n, int m) {
  return (n == 12 && m == 4) || (n == 6 && m == 3) || (n == 6 && m == 6) || (n == 8 && m == 4) || (n == 12 && m == 3);
}

// Cost weights and bounds: one row [16] each for the batch (imask 15, the kernels read element j), or -- once either is
// given per instance -- [Bp][16] each (imask ~0u: element inst * 16 + j), the padded instances repeating the last row.
static unsigned tab_imask(const altro_handle* h) { return (h->cost_pi || h->bnd_pi) ? ~0u : 15u; }

// Host mirror of the bounds after altro_batch_set_bounds_dev: the rows the device holds are read back before anything
// reads zmin_h / zmax_h (the callers synchronise already).  The mirror holds 1 row or `batch` rows (bnd_pi), and a `_dev`
// write never changes which: the device table holds at least as many.
static int refresh_bounds_mirror(altro_handle* h) {
  if (!h->bnd_stale) return ALTRO_OK;
  const size_t rows = h->zmin_h.size() / LW;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(h->zmin_h.data(), h->zmin, rows * LW * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(h->zmax_h.data(), h->zmax, rows * LW * sizeof(double), hipMemcpyDeviceToHost));
  h->bnd_stale = false;
  return ALTRO_OK;
}

static int upload_tables(altro_handle* h) {
  if (int rcm = refresh_bounds_mirror(h)) return rcm;
  const bool pi = h->cost_pi || h->bnd_pi;
  const size_t rows = pi ? (size_t)h->Bp : 1;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if ((int)rows > h->tab_cap || !h->wd || !h->wf || !h->zmin || !h->zmax) {
    for (double** t : {&h->wd, &h->wf, &h->zmin, &h->zmax}) HIPCHK(h, h->pool.alloc(t, rows * LW, h->stream, false));
    h->tab_cap = (int)rows;
  }
  const std::vector<double>* src[] = {&h->wd_h, &h->wf_h, &h->zmin_h, &h->zmax_h};
  double* dst[] = {h->wd, h->wf, h->zmin, h->zmax};
  std::vector<double> img(rows * LW);
  for (int t = 0; t < 4; ++t) {
    const bool own = t < 2 ? h->cost_pi : h->bnd_pi;   // this table has one host row per instance
    for (size_t r = 0; r < rows; ++r) {
      const size_t sr = own ? (r < (size_t)h->d.batch ? r : (size_t)h->d.batch - 1) : 0;
      std::memcpy(&img[r * LW], &(*src[t])[sr * LW], LW * sizeof(double));
    }
    HIPCHK(h, hipMemcpy(dst[t], img.data(), rows * LW * sizeof(double), hipMemcpyHostToDevice));
  }
  return ALTRO_OK;
}

static int launch_solve(altro_handle* h, int first_step, int nsteps, int prepare_only = 0) {
  altro::SolveParams p{};
  p.prepare_only = prepare_only;
  p.B = h->d.batch; p.Bp = h->Bp; p.N = h->d.N; p.Nt = h->Nt;
  p.kref = h->kref;
  p.first_step = first_step; p.nsteps = nsteps;
  p.noise = h->noise; p.noise_w = h->noise_w; p.noise_grp = h->noise_grp; p.noise_mode = h->noise_mode; p.mpc_shift = h->mpc_shift;
  p.box_k0 = h->box_k0; p.box_k1 = h->box_k1;
  p.Gcol = h->Gcol; p.Grow = h->Grow; p.fvec = h->fvec;
  p.wd = h->wd; p.wf = h->wf; p.zmin = h->zmin; p.zmax = h->zmax; p.imask = tab_imask(h);
  p.x0 = h->x0; p.Zref = h->Zref; p.Z = h->Z; p.cur = h->cur;
  p.Lb = h->Lb; p.bslot = h->bslot; p.nbp = h->nbp; p.mu = h->mu; p.lone = h->sw.lone; p.pair = h->sw.pair; p.useqz = h->sw.useqz; p.shadow = h->sw.shadow; p.reuse = h->sw.reuse; p.resync = h->sw.resync; p.dbg_wave = h->sw.dbg_wave;
  p.Dff = h->Dff; p.ahash = h->ahash; p.kmu = h->kmu; p.n_fo = h->n_reuse;
  p.Qz = h->Qz;
  p.Acon = h->Acon; p.bcon = h->bcon; p.cmeta = h->cmeta; p.ckn = h->ckn; p.con_inv = h->con_inv;
  p.con_istride = h->con_per_instance ? (unsigned)(h->d.N * LW * LW) : 0u; p.Lc = h->Lc; p.ncrows = h->ncrows; p.KD = h->KD;
  p.iters = h->iters; p.iters_outer = h->iters_outer; p.status = h->status;
  p.cost = h->cost; p.cmax = h->cmax; p.Jtrace = h->Jtrace; p.ctrace = h->ctrace; p.atrace = h->atrace;
  p.n_backward = h->n_backward; p.n_rollout = h->n_rollout; p.wave_cycles = h->wave_cycles;
  p.simd_tab = h->sw.mate ? h->simd_tab : nullptr;
  p.n_solves = h->n_solves; p.n_iters = h->n_iters; p.n_ok = h->n_ok; p.n_trials = h->n_trials;
  p.n_gconf = h->n_gconf; p.dzero = h->dzero;
  p.mlog = (nsteps > 0 && !prepare_only) ? h->mlog : nullptr;  // MPC steps only (altro_mpc_run_async checked the capacity)
  p.o = h->o;
  if (h->o.projected_newton) {  // solve!(::ALTROSolver): the AL stage only has to reach the polish's tolerance
    if (h->o.projected_newton_tolerance >= 0) p.o.constraint_tolerance = h->o.projected_newton_tolerance;
    else { p.o.constraint_tolerance = 0.0; p.o.kickout_max_penalty = 1; }
  }
  p.perm = nullptr;
  p.active = h->flags.mask();
  p.clk = h->clock.args();
  // fused MPC launches of box-constrained problems: group the instances by how many of the launch's steps will need
  // backward passes (see k_group_score); everything else runs in instance order
  // (short launches only: over 100 steps nearly every window meets a bound at some point, the score stops separating the
  //  instances and clustering the pass-heavy rows -- they are also the ones with the hard solves -- lengthens the tail:
  //  measured 20 steps +2 %, 100 steps -3 %, tools/gpu_ab.py)
  if (h->sw.group && h->sw.reuse && !h->o.strict && nsteps >= 4 && nsteps <= h->sw.group_max_steps && !prepare_only && h->ncrows == 0 && h->box_k1 >= h->box_k0 && h->Bp <= 32768) {
    hipLaunchKernelGGL(k_group_score, grid_for((size_t)h->Bp * LW), dim3(256), 0, h->stream, h->Zref, h->zmin, h->zmax, tab_imask(h), h->gscore, h->Bp, h->Nt,
                       first_step, nsteps, h->box_k0, h->box_k1, h->d.n + h->d.m, h->flags.mask(), h->clock.args(), h->d.N);
    hipLaunchKernelGGL(k_group_rank, dim3(1), dim3(256), 0, h->stream, h->gscore, h->perm, h->Bp, h->sw.group);
    p.perm = h->perm;
  }
  const dim3 grid(h->Bp / IPW), block(64);
  const int n = h->d.n, m = h->d.m;
  const bool cones = h->ncrows > 0;
  h->d_in_kd = altro::kd_holds_d(m, cones);
#define ALTRO_LAUNCH(NX_, NU_)                                                                            \
  do {                                                                                                    \
    if (cones) hipLaunchKernelGGL((altro::solve_kernel<NX_, NU_, true>), grid, block, 0, h->stream, p);  \
    else hipLaunchKernelGGL((altro::solve_kernel<NX_, NU_, false>), grid, block, 0, h->stream, p);       \
  } while (0)
#ifdef ALTRO_DEV_HEADLINE_ONLY  // development builds: only the headline instantiation (compiles in a fraction of the time)
  if (n == 12 && m == 4 && !cones) hipLaunchKernelGGL((altro::solve_kernel<12, 4, false>), grid, block, 0, h->stream, p);
  else FAIL(h, ALTRO_ERR_UNSUPPORTED, "development build: only (12, 4) without cones");
#else
  if (n == 12 && m == 4) ALTRO_LAUNCH(12, 4);
  else if (n == 6 && m == 3) ALTRO_LAUNCH(6, 3);
  else if (n == 6 && m == 6) ALTRO_LAUNCH(6, 6);
  else if (n == 8 && m == 4) ALTRO_LAUNCH(8, 4);
  else if (n == 12 && m == 3) ALTRO_LAUNCH(12, 3);
  else FAIL(h, ALTRO_ERR_UNSUPPORTED, "no kernel built for this (n, m)");
#endif
#undef ALTRO_LAUNCH
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

// The gains kept in KD for reuse (solve_dpp16.h fosweep) depend on the dynamics, the cost weights, the set of bounded
// elements and the options: every setter of those drops them (kmu < 0: no valid gains).  Trajectories, duals and
// reference windows need no such care: the active set they produce is hashed and compared at every use.
static int drop_gains(altro_handle* h) {
  if (h->kmu && !h->sw.keep_gains) {
    hipLaunchKernelGGL(k_fill, grid_for((size_t)h->Bp), dim3(256), 0, h->stream, h->kmu, -1.0, (size_t)h->Bp);
    HIPCHK(h, hipGetLastError());
  }
  return ALTRO_OK;
}

static int upload(altro_handle* h, const double* host, size_t count, size_t stage_off_elems = 0) {
  HIPCHK(h, hipMemcpyAsync(h->stage + stage_off_elems, host, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return ALTRO_OK;
}

// Nothing may propagate across the C boundary: every entry point runs its body inside guard(), which
// turns std::bad_alloc (the std::vector / std::string members of the handle) and anything else into
// ALTRO_ERR_INTERNAL.
template <class F>
static int32_t guard(altro_handle* h, F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    try { if (h) h->err = "out of host memory"; else g_create_err = "out of host memory"; } catch (...) {}
    return ALTRO_ERR_INTERNAL;
  } catch (const std::exception& e) {
    try { if (h) h->err = std::string("internal error: ") + e.what(); else g_create_err = e.what(); } catch (...) {}
    return ALTRO_ERR_INTERNAL;
  } catch (...) {
    return ALTRO_ERR_INTERNAL;
  }
}

static void apply_wide_switches(altro_wide::WideBackend* wb) {
  wb->debug_keep_gains = g_dbg.keep_gains != 0;
  if (g_dbg.wide_compact >= 0) wb->compact_np_max = g_dbg.wide_compact;
  if (g_dbg.wide_coop >= 0) wb->coop_mode = g_dbg.wide_coop != 0 ? 1 : 0;
  if (g_dbg.wide_static_mask >= 0) wb->static_mask = g_dbg.wide_static_mask;
}

// ------------------------------------------------------------------ C-ABI
extern "C" {

int32_t altro_debug_set(altro_handle* h, const char* key, int32_t value) {
  return guard(h, [&]() -> int32_t {
    if (!key) return ALTRO_ERR_INVALID_ARG;
    const std::string k(key);
    auto bad = [&](int32_t code, const char* msg) -> int32_t {
      if (h) h->err = msg; else g_create_err = msg;
      return code;
    };
    if (k == "keep_gains") {
#ifdef ALTRO_DEBUG
      if (h && h->wide) { h->wide->debug_keep_gains = value != 0; return ALTRO_OK; }
#else
      if (value == 0) return ALTRO_OK;
      return bad(ALTRO_ERR_UNSUPPORTED, "keep_gains exists in -DALTRO_DEBUG builds of the library only");
#endif
    }
    if (k == "dev_via_stage") {   // handle switch (16-lane backend): measurement of DESIGN.md 7c
      if (!h) return bad(ALTRO_ERR_STATE, "dev_via_stage is a switch of a handle");
      h->dev_via_stage = value != 0;
      return ALTRO_OK;
    }
    const SwitchKey* sk = nullptr;
    for (const SwitchKey& c : kSwitchKeys)
      if (k == c.key) sk = &c;
    if (!sk) return bad(ALTRO_ERR_INVALID_ARG, "unknown switch");
    // create-time switches: which backend, and the LDS carve-up of the one-wave-per-instance backend
    if (sk->at_create && h) return bad(ALTRO_ERR_STATE, "this switch is read when a handle is created: pass a null handle before altro_batch_create");
    if (k == "group_mode" && (value < 0 || value > 4)) return bad(ALTRO_ERR_INVALID_ARG, "group_mode is 0..4");
    DebugSwitches& d = h ? h->sw : g_dbg;   // (a wide handle keeps its copy too: its backend reads none of the scheduling switches)
    const int reuse_was = d.reuse;
    d.*(sk->member) = sk->negate ? (value ? 0 : 1) : value;
    if (h && !h->wide && d.reuse != reuse_was) { HIPCHK(h, hipSetDevice(h->device)); return drop_gains(h); }
    return ALTRO_OK;
  });
}

int32_t altro_default_opts(altro_opts* o) {
  return guard(nullptr, [&]() -> int32_t {
    if (!o) return ALTRO_ERR_INVALID_ARG;
    o->cost_tolerance = 1e-4;
    o->cost_tolerance_intermediate = 1e-4;
    o->gradient_tolerance = 10.0;
    o->gradient_tolerance_intermediate = 1.0;
    o->constraint_tolerance = 1e-6;
    o->penalty_initial = NAN;
    o->penalty_scaling = NAN;
    o->penalty_max = 1e8;
    o->dual_max = 1e8;
    o->line_search_lower_bound = 1e-8;
    o->line_search_upper_bound = 10.0;
    o->max_cost_value = 1e8;
    o->max_state_value = 1e8;
    o->max_control_value = 1e8;
    o->bp_reg_initial = 0.0;
    o->bp_reg_increase_factor = 1.6;
    o->bp_reg_max = 1e8;
    o->bp_reg_min = 1e-8;
    o->bp_reg_fp = 10.0;
    o->iterations = 1000;
    o->iterations_inner = 300;
    o->iterations_outer = 30;
    o->iterations_linesearch = 20;
    o->dJ_counter_limit = 10;
    o->reset_duals = 1;
    o->reset_penalties = 1;
    o->bp_reg = 0;
    o->soc_second_order = 1;
    o->strict = 0;
    o->kickout_max_penalty = 0;
    o->projected_newton = 0;
    o->projected_newton_tolerance = 1e-3;
    o->active_set_tolerance_pn = 1e-3;
    o->rho_chol = 1e-2;
    o->rho_primal = 1e-8;
    o->r_threshold = 1.1;
    return ALTRO_OK;
  });
}

const char* altro_last_error(const altro_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int32_t altro_batch_create(const altro_dims* dims, const altro_opts* opts, int32_t device, altro_handle** out) {
  return guard(nullptr, [&]() -> int32_t {
    if (!dims || !out) { g_create_err = "null argument"; return ALTRO_ERR_INVALID_ARG; }
    *out = nullptr;
    if (dims->batch < 1 || dims->n < 1 || dims->m < 1 || dims->N < 3) { g_create_err = "bad dims"; return ALTRO_ERR_INVALID_ARG; }
    // (n, m) of the 16-lane kernel set run there; everything else up to n <= 64, m <= 32 runs on the
    // one-wave-per-instance MFMA kernel (altro_debug_set(NULL, "force_wide", 1) sends every size there: used by the tests)
    const bool use_wide = !supported_dims(dims->n, dims->m) || g_dbg.force_wide != 0;
    if (use_wide && !altro_wide::WideBackend::supports(dims->n, dims->m)) {
      g_create_err = "unsupported (n, m): the wide kernel holds n <= 64, m <= 32";
      return ALTRO_ERR_UNSUPPORTED;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) {
      g_create_err = std::string("no HIP device: ") + hipGetErrorString(e);
      return ALTRO_ERR_HIP;
    }
    if (device < 0 || device >= ndev) { g_create_err = "device index out of range"; return ALTRO_ERR_INVALID_ARG; }
    if (use_wide) {
      altro_handle* hw = new (std::nothrow) altro_handle();
      altro_wide::WideBackend* wb = new (std::nothrow) altro_wide::WideBackend();
      if (!hw || !wb) { g_create_err = "out of host memory"; delete hw; delete wb; return ALTRO_ERR_INVALID_ARG; }
      struct WOwner {  // releases both on every path out of this block (exceptions included) unless handed over
        altro_handle* hw;
        altro_wide::WideBackend* wb;
        ~WOwner() { if (wb) { wb->destroy(); delete wb; } delete hw; }
      } wo{hw, wb};
      altro_opts o0;
      if (opts) o0 = *opts; else altro_default_opts(&o0);
      hw->d = *dims;
      hw->o = o0;
      hw->device = device;
      apply_wide_switches(wb);
      const int rc = wb->create(dims, &o0, device);
      if (rc) {
        g_create_err = wb->err;
        return rc;
      }
      hw->wide = wb;
      wo.hw = nullptr;
      wo.wb = nullptr;
      *out = hw;
      return ALTRO_OK;
    }
    altro_handle* h = new (std::nothrow) altro_handle();
    if (!h) { g_create_err = "out of host memory"; return ALTRO_ERR_INVALID_ARG; }
    // anything that throws below (std::vector::assign, std::string) unwinds through this guard: the handle, its stream,
    // events and every array allocated so far are released before guard() turns the exception into an error code
    struct Owner {
      altro_handle* p;
      ~Owner() { if (p) altro_batch_destroy(p); }
    } owner{h};
    h->d = *dims;
    if (opts) h->o = *opts; else altro_default_opts(&h->o);
    h->device = device;
    h->sw = g_dbg;
    h->Bp = (dims->batch + IPW - 1) / IPW * IPW;
    h->slots = h->Bp;
    h->mlog_rec = LW + altro::MLOG_TAIL;
    h->noise_len = LW;
    auto fail = [&](const char* what, hipError_t er) {
      g_create_err = std::string(what) + ": " + hipGetErrorString(er);
      return ALTRO_ERR_HIP;      // (the Owner releases the handle)
    };
  #define CCHK(call) do { hipError_t e2 = (call); if (e2 != hipSuccess) return fail(#call, e2); } while (0)
    CCHK(hipSetDevice(device));
    CCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CCHK(hipEventCreate(&h->ev0));
    CCHK(hipEventCreate(&h->ev1));
    CCHK(hipEventCreate(&h->bev0));
    CCHK(hipEventCreate(&h->bev1));
    h->ring.reset();
    const size_t Bp = h->Bp, N = dims->N, n = dims->n, m = dims->m;
    const size_t row = Bp * LW;
    // the kernels address every array with 32-bit element offsets
    if ((2 * N + 1) * row * sizeof(double) >= (1ull << 32) || N * Bp * m * LW * sizeof(double) >= (1ull << 32)) {
      g_create_err = "batch * N too large for one handle (arrays must stay below 4 GiB); split the batch";
      return ALTRO_ERR_UNSUPPORTED;
    }
    for (int j = 0; j < LW; ++j) h->bslot_h[j] = -1;
    // every device array of the backend: (member, elements), zero-filled on the stream
  #define DA(member, count) CCHK(h->pool.alloc(&h->member, (count), h->stream))
    DA(Gcol, Bp * n * LW); DA(Grow, Bp * LW * LW); DA(fvec, row);
    DA(wd, LW); DA(wf, LW); DA(zmin, LW); DA(zmax, LW);
    DA(x0, row);
    DA(Z, (2 * N + 1) * row);    // + one trash row at the end of each (stores of rows that sit out a phase land there)
    DA(Lb, (N + 1) * Bp * 2 * h->nbp); DA(bslot, LW); DA(Lc, (N + 1) * row);
    DA(Acon, N * LW * LW); DA(bcon, N * LW); DA(cmeta, N * LW * 4); DA(ckn, LW); DA(lanebuf, LW);
    DA(noise_w, LW); DA(noise_grp, LW);
    DA(mu, Bp); DA(kmu, Bp); DA(ahash, row); DA(dzero, Bp);
    DA(KD, N * Bp * m * LW);     // N-1 gain blocks + a trash slot
    DA(Qz, (N + 1) * row); DA(Dff, (N + 1) * row);
    DA(pn_out.ran, Bp); DA(pn_out.failed, Bp); DA(pn_out.dfail, Bp); DA(pn_out.res, Bp); DA(pn_out.dres0, Bp); DA(pn_out.dres, Bp);
    DA(cur, Bp); DA(perm, Bp); DA(gscore, Bp); DA(refusals, 1);
    DA(iters, Bp); DA(iters_outer, Bp); DA(status, Bp); DA(cost, Bp); DA(cmax, Bp);
    DA(Jtrace, Bp * ALTRO_TRACE_LEN); DA(ctrace, Bp * ALTRO_TRACE_LEN); DA(atrace, Bp * ALTRO_TRACE_LEN);
    DA(n_backward, Bp); DA(n_rollout, Bp); DA(n_solves, Bp); DA(n_iters, Bp); DA(n_ok, Bp); DA(n_trials, Bp); DA(n_gconf, Bp); DA(n_reuse, Bp);
    DA(wave_cycles, Bp * 6 + 4096); DA(simd_tab, (size_t)65536 * 16);
  #undef DA
    // what does not start at zero: no bounds until a BOX constraint is added, no bounded element, no constraint row on any
    // lane, 1 % of ||x0||_inf of plant noise (random_linear_problem.jl:129), penalty 1, no gains yet
    h->zmin_h.assign(LW, -INFINITY); h->zmax_h.assign(LW, INFINITY);
    h->wd_h.assign(LW, 0.0); h->wf_h.assign(LW, 0.0);
    h->Acon_h.assign(N * LW * LW, 0.0);
    h->bcon_h.assign(N * LW, 0.0);
    h->cmeta_h.assign(N * LW * 4, 0);
    for (size_t e = 0; e < N * LW; ++e) h->cmeta_h[4 * e + 2] = -1;
    CCHK(hipMemcpyAsync(h->cmeta, h->cmeta_h.data(), h->cmeta_h.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    CCHK(hipMemcpyAsync(h->bslot, h->bslot_h, LW * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, h->stream, h->zmin, -INFINITY, (size_t)LW);
    hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, h->stream, h->zmax, INFINITY, (size_t)LW);
    hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, h->stream, h->noise_w, 0.01, (size_t)LW);
    hipLaunchKernelGGL(k_fill, grid_for(Bp), dim3(256), 0, h->stream, h->mu, 1.0, (size_t)Bp);
    hipLaunchKernelGGL(k_fill, grid_for(Bp), dim3(256), 0, h->stream, h->kmu, -1.0, (size_t)Bp);
    CCHK(hipGetLastError());
    CCHK(hipStreamSynchronize(h->stream));
  #undef CCHK
    owner.p = nullptr;
    *out = h;
    return ALTRO_OK;
  });
}

// release everything the 16-lane backend owns on the device (the handle itself stays)
static void free_dpp_backend(altro_handle* h) {
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  h->pool.release_all();
  h->stage_bytes = 0;
  h->eval_ws_elems = 0;
  h->mlog_cap = 0;
  h->pn_ws.bm = h->pn_ws.slots = 0;
  h->ring.destroy();
  if (h->bev0) { hipEventDestroy(h->bev0); h->bev0 = nullptr; }
  if (h->bev1) { hipEventDestroy(h->bev1); h->bev1 = nullptr; }
  if (h->ev0) { hipEventDestroy(h->ev0); h->ev0 = nullptr; }
  if (h->ev1) { hipEventDestroy(h->ev1); h->ev1 = nullptr; }
  if (h->stream) { hipStreamDestroy(h->stream); h->stream = nullptr; }
}

int32_t altro_batch_destroy(altro_handle* h) {
  if (!h) return ALTRO_OK;
  if (h->wide) {
    h->wide->destroy();
    delete h->wide;
  } else {
    free_dpp_backend(h);
  }
  h->flags.destroy();
  h->clock.destroy();
  h->link.destroy();
  delete h;
  return ALTRO_OK;
}

// Per-knot (LTV) dynamics exist on the one-wave-per-instance kernel only.  A 16-lane handle on which nothing
// but create has happened moves there; the Julia model is fixed when ALTROSolver(prob, opts) is built
// (ALTROParams.jl:61,96), so set_dynamics is the first call of every harness.
static int migrate_to_wide(altro_handle* h) {
  if (h->have_cost || h->have_ref || h->have_dyn || h->ncon > 0 || h->timed)
    FAIL(h, ALTRO_ERR_UNSUPPORTED, "per-knot dynamics on an (n, m) of the 16-lane kernel set: call altro_batch_set_dynamics "
                                   "first after altro_batch_create (or altro_debug_set(NULL, \"force_wide\", 1) before it)");
  altro_wide::WideBackend* wb = new (std::nothrow) altro_wide::WideBackend();
  if (!wb) FAIL(h, ALTRO_ERR_INTERNAL, "out of host memory");
  apply_wide_switches(wb);
  // the wide backend is created BEFORE the 16-lane one is released: if it cannot be (e.g. no device
  // memory for its arrays) the handle stays a working 16-lane handle and only this call fails
  const int rc = wb->create(&h->d, &h->o, h->device);
  if (rc) {
    h->err = wb->err;
    wb->destroy();
    delete wb;
    return rc;
  }
  if (h->have_x0) {  // an initial state uploaded before the model: carried over, not dropped
    std::vector<double> x((size_t)h->d.batch * h->d.n);
    int rcx = h->ensure_stage(x.size() * sizeof(double));
    if (!rcx) {
      hipLaunchKernelGGL(k_unpack_x0, grid_for((size_t)h->d.batch * LW), dim3(256), 0, h->stream, h->stage, h->x0, h->d.batch, h->d.n);
      if (hipMemcpyAsync(x.data(), h->stage, x.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
          hipStreamSynchronize(h->stream) != hipSuccess) rcx = ALTRO_ERR_HIP;
    }
    if (!rcx) rcx = wb->set_initial_state(x.data());
    if (rcx) {
      h->err = rcx == ALTRO_ERR_HIP ? "copying the initial state to the wide backend failed" : wb->err;
      wb->destroy();
      delete wb;
      return rcx;
    }
  }
  if (h->mlog_cap > 0) {  // altro_mpc_set_log before the model: the setting moves with the handle (the records start empty)
    const int rcl = wb->set_log(h->mlog_cap);
    if (rcl) {
      h->err = wb->err;
      wb->destroy();
      delete wb;
      return rcl;
    }
  }
  wb->flags = h->flags;   // a mask set before the model moves with the handle (its buffers hold Bp >= batch entries)
  h->flags = altro::InstanceFlags{};
  wb->clock = h->clock;   // and so does an episode clock
  h->clock = altro::EpisodeClock{};
  free_dpp_backend(h);
  h->wide = wb;
  return ALTRO_OK;
}

// time-invariant dynamics of a 16-lane handle.  dev: A, B, f are device arrays (validated by the caller): the layout kernel
// reads them where they are, nothing is staged and the stream is not synchronised
static int set_dynamics_16(altro_handle* h, const double* A, const double* B, const double* f, int32_t per_instance, bool dev) {
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = h->d.n, m = h->d.m;
  const size_t nb = per_instance ? h->d.batch : 1;
  if (!dev) {
    const size_t tot = nb * (n * n + n * m + n);
    int rc = h->ensure_stage(tot * sizeof(double));
    if (rc) return rc;
    if ((rc = upload(h, A, nb * n * n, 0))) return rc;
    if ((rc = upload(h, B, nb * n * m, nb * n * n))) return rc;
    if (f && (rc = upload(h, f, nb * n, nb * (n * n + n * m)))) return rc;
    A = h->stage;
    B = h->stage + nb * n * n;
    if (f) f = h->stage + nb * (n * n + n * m);
  }
  hipLaunchKernelGGL(k_pack_dyn, grid_for((size_t)h->Bp * LW), dim3(256), 0, h->stream, A, B, f, h->Gcol, h->Grow, h->fvec,
                     h->d.batch, h->Bp, (int)n, (int)m, per_instance ? 1 : 0);
  HIPCHK(h, hipGetLastError());
  if (int rcd = drop_gains(h)) return rcd;
  if (!dev) HIPCHK(h, hipStreamSynchronize(h->stream));
  h->have_dyn = true;
  h->dyn_per_instance = per_instance != 0;
  return ALTRO_OK;
}

int32_t altro_batch_set_dynamics(altro_handle* h, const double* A, const double* B, const double* f,
                                 int32_t per_knot, int32_t per_instance) {
  return guard(h, [&]() -> int32_t {
    if (!h || !A || !B) return ALTRO_ERR_INVALID_ARG;
    if (per_knot && !h->wide) {
      if (int rc = migrate_to_wide(h)) return rc;
    }
    WIDE_FWD(h, set_dynamics(A, B, f, per_knot, per_instance));
    return set_dynamics_16(h, A, B, f, per_instance, false);
  });
}

// altro_batch_set_tracking_cost(_per_instance): Qd [rows][n], Rd [rows][m], Qfd [rows][n], rows = 1 or batch
static int set_cost_rows(altro_handle* h, const double* Qd, const double* Rd, const double* Qfd, double dt, bool per_instance) {
  HIPCHK(h, hipSetDevice(h->device));
  const int n = h->d.n, m = h->d.m;
  const size_t rows = per_instance ? (size_t)h->d.batch : 1;
  std::vector<double> wd(rows * LW, 0.0), wf(rows * LW, 0.0);
  for (size_t r = 0; r < rows; ++r) {
    for (int j = 0; j < n; ++j) { wd[r * LW + j] = dt * Qd[r * n + j]; wf[r * LW + j] = Qfd[r * n + j]; }
    for (int j = 0; j < m; ++j) wd[r * LW + n + j] = dt * Rd[r * m + j];
  }
  h->wd_h.swap(wd);
  h->wf_h.swap(wf);
  h->cost_pi = per_instance;
  if (int rc = upload_tables(h)) return rc;
  if (int rcd = drop_gains(h)) return rcd;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->dt = dt;
  h->have_cost = true;
  return ALTRO_OK;
}

int32_t altro_batch_set_tracking_cost(altro_handle* h, const double* Qd, const double* Rd, const double* Qfd, double dt) {
  return guard(h, [&]() -> int32_t {
    if (!h || !Qd || !Rd || !Qfd || !(dt > 0)) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, set_tracking_cost(Qd, Rd, Qfd, dt));
    return set_cost_rows(h, Qd, Rd, Qfd, dt, false);
  });
}

int32_t altro_batch_set_tracking_cost_per_instance(altro_handle* h, const double* Qd, const double* Rd, const double* Qfd,
                                                   double dt) {
  return guard(h, [&]() -> int32_t {
    if (!h || !Qd || !Rd || !Qfd || !(dt > 0)) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, set_tracking_cost_per_instance(Qd, Rd, Qfd, dt));
    return set_cost_rows(h, Qd, Rd, Qfd, dt, true);
  });
}

// Pack the recorded LINEAR / SOC constraints onto the 16 constraint-row lanes and fill the per-knot
// tables.  A constraint keeps the same lanes over its whole knot range (shift_fill moves duals
// along the knot axis); two constraints may share lanes when their ranges do not overlap (e.g. the
// goal at knot N-1 and the stage constraints on 0..N-2).  Every cone takes the first p lanes of an
// aligned quad, linear rows fill whatever lanes remain (also the spare lanes of a cone's quad).
// Redone whenever a constraint is added before the first solve.
// Host mirrors after altro_batch_update_constraint_data_dev: the rows a `_dev` call wrote exist on the device only.  Before
// anything reads cb.A / cb.b (pack_constraints rebuilds the tables from the blocks of EVERY constraint) the device tables are
// read back and the stale blocks are taken out of them, the exact inverse of the packing below.  Synchronises; its callers do.
static int refresh_con_mirrors(altro_handle* h) {
  bool any = false;
  for (const auto& cb : h->cons) any = any || cb.stale;
  if (!any) return ALTRO_OK;
  const size_t nz = h->d.n + h->d.m, N = h->d.N, B = h->d.batch;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(h->Acon_h.data(), h->Acon, h->Acon_h.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(h->bcon_h.data(), h->bcon, h->bcon_h.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (auto& cb : h->cons) {
    if (!cb.stale) continue;
    const size_t nk = cb.per_knot ? (size_t)(cb.k1 - cb.k0 + 1) : 1;
    for (size_t ib = 0; ib < (cb.per_instance ? B : 1); ++ib)
      for (size_t kk = 0; kk < nk; ++kk)
        for (int r = 0; r < cb.p; ++r) {
          const size_t blk = ib * nk + kk;
          const size_t et = (ib * N + (size_t)cb.k0 + kk) * LW + cb.lanes[r];
          for (size_t jj = 0; jj < nz; ++jj) cb.A[(blk * cb.p + r) * nz + jj] = h->Acon_h[et * LW + jj];
          cb.b[blk * cb.p + r] = h->bcon_h[et];
        }
    cb.stale = false;
  }
  return ALTRO_OK;
}

static int pack_constraints(altro_handle* h) {
  if (!h->con_dirty) return ALTRO_OK;
  if (int rcm = refresh_con_mirrors(h)) return rcm;
  const int nz = h->d.n + h->d.m, N = h->d.N;
  // one table per instance as soon as any block carries per-instance data (grasp_mpc_helpers.jl:46-55 mutates each
  // problem's own per-knot tables); the lane assignment (cmeta) is common to the batch either way
  h->con_per_instance = false;
  for (const auto& cb : h->cons) h->con_per_instance = h->con_per_instance || cb.per_instance;
  const size_t ninst = h->con_per_instance ? (size_t)h->Bp : 1, B = h->d.batch;
  if (ninst * N * LW * LW * sizeof(double) >= (1ull << 32)) FAIL(h, ALTRO_ERR_UNSUPPORTED, "per-instance constraint tables of this batch exceed 4 GiB; split the batch");
  h->Acon_h.assign(ninst * N * LW * LW, 0.0);
  h->bcon_h.assign(ninst * N * LW, 0.0);
  std::fill(h->cmeta_h.begin(), h->cmeta_h.end(), 0);
  for (size_t e = 0; e < (size_t)N * LW; ++e) h->cmeta_h[4 * e + 2] = -1;
  std::vector<char> used((size_t)N * LW, 0);      // lane taken at knot k
  std::vector<char> quad_soc((size_t)N * 4, 0);   // quad holds a cone at knot k
  auto lane_free = [&](int lane, int k0, int k1) {
    for (int k = k0; k <= k1; ++k) if (used[(size_t)k * LW + lane]) return false;
    return true;
  };
  auto place = [&](altro_handle::ConBlock& cb, int r, int lane, int type, int pdim) {
    cb.lanes[r] = lane;
    const size_t nk = cb.per_knot ? (size_t)(cb.k1 - cb.k0 + 1) : 1;
    for (int k = cb.k0; k <= cb.k1; ++k) {
      const size_t e = (size_t)k * LW + lane;
      used[e] = 1;
      for (size_t ib = 0; ib < ninst; ++ib) {
        const size_t src = ib < B ? ib : B - 1;      // padded slots mirror the last instance
        const size_t blk = (cb.per_instance ? src * nk : 0) + (cb.per_knot ? (size_t)(k - cb.k0) : 0);
        const size_t et = ib * N * LW + e;
        for (int jj = 0; jj < nz; ++jj) h->Acon_h[et * LW + jj] = cb.A[(blk * cb.p + r) * nz + jj];
        h->bcon_h[et] = cb.b[blk * cb.p + r];
      }
      h->cmeta_h[4 * e + 0] = type;
      h->cmeta_h[4 * e + 1] = cb.k0;
      h->cmeta_h[4 * e + 2] = cb.k1;
      h->cmeta_h[4 * e + 3] = pdim;
    }
  };
  for (auto& cb : h->cons) {
    if (cb.kind != ALTRO_CON_SOC) continue;
    int q = -1;
    for (int c = 0; c < 4 && q < 0; ++c) {
      bool ok = true;
      for (int k = cb.k0; k <= cb.k1 && ok; ++k) ok = !quad_soc[(size_t)k * 4 + c];
      for (int r = 0; r < cb.p && ok; ++r) ok = lane_free(4 * c + r, cb.k0, cb.k1);
      if (ok) q = c;
    }
    if (q < 0) FAIL(h, ALTRO_ERR_UNSUPPORTED, "no free quad of constraint-row lanes for a second-order cone (4 cones per knot)");
    for (int k = cb.k0; k <= cb.k1; ++k) quad_soc[(size_t)k * 4 + q] = 1;
    for (int r = 0; r < cb.p; ++r) place(cb, r, 4 * q + r, 3, cb.p);
  }
  for (auto& cb : h->cons) {
    if (cb.kind != ALTRO_CON_LINEAR) continue;
    int lane = 0;
    for (int r = 0; r < cb.p; ++r) {
      while (lane < LW && !lane_free(lane, cb.k0, cb.k1)) ++lane;
      if (lane == LW) FAIL(h, ALTRO_ERR_UNSUPPORTED, "more than 16 constraint rows at one knot");
      place(cb, r, lane, cb.sense == ALTRO_SENSE_EQ ? 1 : 2, 0);
    }
  }
  // every lane of a quad carries the dimension of the cone the quad holds at that knot (a linear
  // row in a spare lane is excluded from the cone by pos >= p)
  for (int k = 0; k < N; ++k)
    for (int q = 0; q < 4; ++q) {
      int pdim = 0;
      for (int i = 0; i < 4; ++i) {
        const size_t e = (size_t)k * LW + 4 * q + i;
        if (h->cmeta_h[4 * e] == 3) pdim = h->cmeta_h[4 * e + 3];
      }
      for (int i = 0; i < 4; ++i) h->cmeta_h[4 * ((size_t)k * LW + 4 * q + i) + 3] = pdim;
    }
  h->ncrows = h->cons.empty() ? 0 : LW;
  if (h->Acon_h.size() != h->acon_elems || !h->Acon || !h->bcon) {  // the table changed shape (per-instance data arrived): reallocate
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, h->pool.alloc(&h->Acon, h->Acon_h.size(), h->stream, false));
    HIPCHK(h, h->pool.alloc(&h->bcon, h->bcon_h.size(), h->stream, false));
    h->acon_elems = h->Acon_h.size();
  }
  HIPCHK(h, hipMemcpyAsync(h->Acon, h->Acon_h.data(), h->Acon_h.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->bcon, h->bcon_h.data(), h->bcon_h.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->cmeta, h->cmeta_h.data(), h->cmeta_h.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  // Time-invariant tables (rocket landing: every constraint has ONE block of data and its own lanes): the row a lane
  // holds is the same at every knot of its range, so the streaming sweeps load it once per sweep from one canonical
  // knot instead of once per knot (solve_dpp16.h trial_costs).  Decided on the packed tables themselves.
  {
    bool inv = !h->con_per_instance;
    int ckn[LW];
    for (int lane = 0; lane < LW; ++lane) {
      int first = -1;
      for (int k = 0; k < N && inv; ++k) {
        const size_t e = (size_t)k * LW + lane;
        if (h->cmeta_h[4 * e] == 0) continue;
        if (first < 0) { first = k; continue; }
        const size_t f = (size_t)first * LW + lane;
        for (int q = 0; q < 4; ++q) inv = inv && h->cmeta_h[4 * e + q] == h->cmeta_h[4 * f + q];
        inv = inv && h->bcon_h[e] == h->bcon_h[f];
        for (int jj = 0; jj < LW; ++jj) inv = inv && h->Acon_h[e * LW + jj] == h->Acon_h[f * LW + jj];
      }
      ckn[lane] = first < 0 ? 0 : first;
    }
    // a lane without rows must be empty at its canonical knot 0 too: true by construction (it is empty everywhere)
    h->con_inv = inv ? 1 : 0;
    HIPCHK(h, hipMemcpyAsync(h->ckn, ckn, LW * sizeof(int), hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->con_dirty = false;
  return ALTRO_OK;
}

int32_t altro_batch_add_constraint(altro_handle* h, int32_t kind, int32_t sense, int32_t k_first, int32_t k_last,
                                   int32_t p, const double* A, const double* b, const double* zmin, const double* zmax,
                                   int32_t per_knot, int32_t* con_id) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    if (k_first < 0 || k_last >= h->d.N || k_last < k_first) FAIL(h, ALTRO_ERR_INVALID_ARG, "bad knot range");
    if (kind == ALTRO_CON_BOX ? (!zmin || !zmax) : (kind != ALTRO_CON_LINEAR && kind != ALTRO_CON_SOC) || !A || !b || p < 1) return ALTRO_ERR_INVALID_ARG;
    if (kind == ALTRO_CON_LINEAR && sense != ALTRO_SENSE_EQ && sense != ALTRO_SENSE_INEQ) return ALTRO_ERR_INVALID_ARG;
    // (what a backend cannot hold, and what the state of the handle forbids, is each backend's own answer from here on)
    WIDE_FWD(h, add_constraint(kind, sense, k_first, k_last, p, A, b, zmin, zmax, per_knot, con_id));
    HIPCHK(h, hipSetDevice(h->device));
    const int nz = h->d.n + h->d.m;
    if (kind == ALTRO_CON_LINEAR || kind == ALTRO_CON_SOC) {
      if (kind == ALTRO_CON_SOC && (p < 2 || p > 4)) FAIL(h, ALTRO_ERR_UNSUPPORTED, "second-order cones of dimension 2..4 are built");
      if (h->con_locked) FAIL(h, ALTRO_ERR_STATE, "constraints must be added before the first solve");
      altro_handle::ConBlock cb;
      cb.id = h->ncon; cb.kind = kind; cb.sense = sense; cb.k0 = k_first; cb.k1 = k_last; cb.p = p;
      cb.per_knot = (per_knot & 1) ? 1 : 0;
      cb.per_instance = (per_knot & 2) ? 1 : 0;
      const size_t nblk = (cb.per_knot ? (size_t)(k_last - k_first + 1) : 1) * (cb.per_instance ? (size_t)h->d.batch : 1);
      cb.A.assign(A, A + nblk * p * nz);
      cb.b.assign(b, b + nblk * p);
      for (int r = 0; r < LW; ++r) cb.lanes[r] = -1;
      h->cons.push_back(cb);
      h->con_dirty = true;
      int rc = pack_constraints(h);
      if (rc) { h->cons.pop_back(); h->con_dirty = true; pack_constraints(h); return rc; }
      if (con_id) *con_id = h->ncon;
      h->ncon++;
      return ALTRO_OK;
    }
    if (h->box_id >= 0) FAIL(h, ALTRO_ERR_UNSUPPORTED, "one BOX constraint per problem");
    std::vector<double> lo(LW, -INFINITY), hi(LW, INFINITY);
    for (int j = 0; j < nz; ++j) { lo[j] = zmin[j]; hi[j] = zmax[j]; }
    for (int j = 0; j < LW; ++j) { h->box_lo_fin[j] = j < nz && lo[j] > -1e300; h->box_hi_fin[j] = j < nz && hi[j] < 1e300; }
    h->zmin_h = lo;
    h->zmax_h = hi;
    h->bnd_pi = false;
    if (h->cost_pi) {   // the tables hold one row per instance: the BOX's row goes to every one of them
      if (int rc = upload_tables(h)) return rc;
    } else {
      HIPCHK(h, hipMemcpyAsync(h->zmin, lo.data(), LW * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(h->zmax, hi.data(), LW * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    // compact dual rows: one slot per element with at least one finite bound
    int nb = 0;
    for (int j = 0; j < LW; ++j) h->bslot_h[j] = (j < nz && (std::isfinite(lo[j]) || std::isfinite(hi[j]))) ? nb++ : -1;
    h->nbp = nb > 0 ? nb : 1;
    HIPCHK(h, hipMemcpyAsync(h->bslot, h->bslot_h, LW * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, h->pool.alloc(&h->Lb, (size_t)(h->d.N + 1) * h->Bp * 2 * h->nbp, h->stream));
    if (int rcd = drop_gains(h)) return rcd;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->box_k0 = k_first;
    h->box_k1 = k_last;
    h->box_id = h->ncon++;
    if (con_id) *con_id = h->box_id;
    return ALTRO_OK;
  });
}

int32_t altro_batch_update_constraint_data(altro_handle* h, int32_t con_id, const double* A, const double* b) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, update_constraint_data(con_id, A, b));
    HIPCHK(h, hipSetDevice(h->device));
    const int nz = h->d.n + h->d.m;
    for (auto& cb : h->cons) {
      if (cb.id != con_id) continue;
      const size_t nblk = (cb.per_knot ? (size_t)(cb.k1 - cb.k0 + 1) : 1) * (cb.per_instance ? (size_t)h->d.batch : 1);
      if (int rcm = refresh_con_mirrors(h)) return rcm;   // (a `_dev` update before this one: its rows come back first)
      if (A) cb.A.assign(A, A + nblk * cb.p * nz);
      if (b) cb.b.assign(b, b + nblk * cb.p);
      // same lanes, new coefficients: refresh the tables (the solver sees it at the next solve, as
      // the reference's in-place mutation does: grasp_mpc_helpers.jl:46-55)
      HIPCHK(h, hipStreamSynchronize(h->stream));
      h->con_dirty = true;
      return pack_constraints(h);
    }
    FAIL(h, ALTRO_ERR_INVALID_ARG, "unknown or non-affine constraint id");
  });
}

int32_t altro_batch_set_bounds(altro_handle* h, int32_t con_id, const double* zmin, const double* zmax, int32_t per_instance) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    if (common(h).box_id < 0 || con_id != common(h).box_id) FAIL(h, ALTRO_ERR_INVALID_ARG, "altro_batch_set_bounds: con_id is not a BOX constraint");
    if (!zmin || !zmax) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, set_bounds(zmin, zmax, per_instance));
    const int nz = h->d.n + h->d.m;
    const size_t rows = per_instance ? (size_t)h->d.batch : 1;
    if (const char* e = altro_wide::check_bound_rows(zmin, zmax, rows, nz, h->box_lo_fin, h->box_hi_fin)) FAIL(h, ALTRO_ERR_INVALID_ARG, e);
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<double> lo(rows * LW, -INFINITY), hi(rows * LW, INFINITY);
    for (size_t r = 0; r < rows; ++r)
      for (int j = 0; j < nz; ++j) { lo[r * LW + j] = zmin[r * nz + j]; hi[r * LW + j] = zmax[r * nz + j]; }
    h->zmin_h.swap(lo);
    h->zmax_h.swap(hi);
    h->bnd_stale = false;   // (the whole mirror is new)
    h->bnd_pi = per_instance != 0;
    if (int rc = upload_tables(h)) return rc;
    if (int rcd = drop_gains(h)) return rcd;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ALTRO_OK;
  });
}

// Copy of a caller's device array into `stage` ("dev_via_stage": the alternative to packing from the caller's pointer that
// DESIGN.md 7c measures).  The staging buffer grows only when a larger array than ever before arrives.
static int stage_d2d(altro_handle* h, const double* src, size_t count, size_t stage_off_elems = 0) {
  HIPCHK(h, hipMemcpyAsync(h->stage + stage_off_elems, src, count * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return ALTRO_OK;
}

// dev: x0 is a device array (validated by the caller); only enqueues
static int set_x0_16(altro_handle* h, const double* x0, bool dev) {
  HIPCHK(h, hipSetDevice(h->device));
  const size_t cnt = (size_t)h->d.batch * h->d.n;
  if (!dev || h->dev_via_stage) {
    int rc = h->ensure_stage(cnt * sizeof(double));
    if (rc) return rc;
    if ((rc = dev ? stage_d2d(h, x0, cnt) : upload(h, x0, cnt))) return rc;
    x0 = h->stage;
  }
  hipLaunchKernelGGL(k_pack_x0, grid_for((size_t)h->Bp * LW), dim3(256), 0, h->stream, x0, h->x0, h->d.batch,
                     h->Bp, h->d.n);
  HIPCHK(h, hipGetLastError());
  if (!dev) HIPCHK(h, hipStreamSynchronize(h->stream));
  h->have_x0 = true;
  return ALTRO_OK;
}

int32_t altro_batch_set_initial_state(altro_handle* h, const double* x0) {
  return guard(h, [&]() -> int32_t {
    if (!h || !x0) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, set_initial_state(x0));
    return set_x0_16(h, x0, false);
  });
}

static int get_x0_16(altro_handle* h, double* x0, bool dev) {
  HIPCHK(h, hipSetDevice(h->device));
  const size_t cnt = (size_t)h->d.batch * h->d.n;
  if (!dev) {
    int rc = h->ensure_stage(cnt * sizeof(double));
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_unpack_x0, grid_for((size_t)h->d.batch * LW), dim3(256), 0, h->stream, dev ? x0 : h->stage, h->x0,
                     h->d.batch, h->d.n);
  HIPCHK(h, hipGetLastError());
  if (dev) return ALTRO_OK;
  HIPCHK(h, hipMemcpyAsync(x0, h->stage, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return ALTRO_OK;
}

int32_t altro_batch_get_initial_state(altro_handle* h, double* x0) {
  return guard(h, [&]() -> int32_t {
    if (!h || !x0) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, get_initial_state(x0));
    return get_x0_16(h, x0, false);
  });
}

static int set_ref_common(altro_handle* h, const double* Xref, const double* Uref, int Nt, bool dev = false) {
  const size_t B = h->d.batch, n = h->d.n, m = h->d.m;
  const size_t cx = B * Nt * n, cu = B * (Nt - 1) * m;
  const bool staged = !dev || h->dev_via_stage;
  int rc = staged ? h->ensure_stage((cx + cu) * sizeof(double)) : ALTRO_OK;
  if (rc) return rc;
  if ((size_t)Nt * h->Bp * LW * sizeof(double) >= (1ull << 32)) FAIL(h, ALTRO_ERR_UNSUPPORTED, "reference trajectory too large for one handle (below 4 GiB)");
  if (h->Nt != Nt || !h->Zref) {
    h->Nt = 0;   // (no reference while the array does not exist: a failure below leaves a handle that says so)
    h->have_ref = false;
    HIPCHK(h, h->pool.alloc(&h->Zref, (size_t)Nt * h->Bp * LW, h->stream, false));
    h->Nt = Nt;
  }
  if (staged) {
    if ((rc = dev ? stage_d2d(h, Xref, cx, 0) : upload(h, Xref, cx, 0))) return rc;
    if ((rc = dev ? stage_d2d(h, Uref, cu, cx) : upload(h, Uref, cu, cx))) return rc;
    Xref = h->stage;
    Uref = h->stage + cx;
  }
  hipLaunchKernelGGL(k_pack_ref, grid_for((size_t)h->Bp * LW), dim3(256), 0, h->stream, Xref, Uref,
                     h->Zref, h->d.batch, h->Bp, Nt, (int)n, (int)m);
  HIPCHK(h, hipGetLastError());
  if (h->clock.on) {   // a new track installs window 0 for every instance, as it does for the handle's kref
    hipLaunchKernelGGL(altro::k_clock_window, altro::EpisodeClock::grid(h->Bp), dim3(256), 0, h->stream, h->clock.window, (const int*)nullptr, 0, h->Bp);
    HIPCHK(h, hipGetLastError());
  }
  if (!dev) HIPCHK(h, hipStreamSynchronize(h->stream));
  h->kref = 0;
  h->have_ref = true;
  return ALTRO_OK;
}

int32_t altro_batch_set_reference(altro_handle* h, const double* Xref, const double* Uref) {
  return guard(h, [&]() -> int32_t {
    if (!h || !Xref || !Uref) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, set_reference(Xref, Uref));
    HIPCHK(h, hipSetDevice(h->device));
    return set_ref_common(h, Xref, Uref, h->d.N);
  });
}

static int set_traj_16(altro_handle* h, const double* X, const double* U, bool dev) {
  HIPCHK(h, hipSetDevice(h->device));
  const size_t B = h->d.batch, N = h->d.N, n = h->d.n, m = h->d.m;
  const size_t cx = X ? B * N * n : 0, cu = B * (N - 1) * m;
  const int have_x = X ? 1 : 0;
  if (!dev) {
    int rc = h->ensure_stage((cx + cu) * sizeof(double));
    if (rc) return rc;
    if (X && (rc = upload(h, X, cx, 0))) return rc;
    if ((rc = upload(h, U, cu, cx))) return rc;
    X = h->stage;
    U = h->stage + cx;
  }
  const size_t plane = N * (size_t)LW;   // offset of plane 1 inside an instance's block of Z
  hipLaunchKernelGGL(k_pack_traj, grid_for((size_t)h->Bp * LW), dim3(256), 0, h->stream, X, U, h->Z,
                     h->cur, plane, (int)B, h->Bp, (int)N, (int)n, (int)m, 1, have_x);
  HIPCHK(h, hipGetLastError());
  if (!dev) HIPCHK(h, hipStreamSynchronize(h->stream));
  return ALTRO_OK;
}

int32_t altro_batch_set_initial_trajectory(altro_handle* h, const double* X, const double* U) {
  return guard(h, [&]() -> int32_t {
    if (!h || !U) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, set_initial_trajectory(X, U));
    return set_traj_16(h, X, U, false);
  });
}

int32_t altro_batch_shift_fill(altro_handle* h, int32_t primal, int32_t dual) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, shift_fill(primal, dual));
    HIPCHK(h, hipSetDevice(h->device));
    const size_t plane = (size_t)h->d.N * LW;
    hipLaunchKernelGGL(k_shift, grid_for((size_t)h->Bp * LW), dim3(256), 0, h->stream, h->Z, h->cur, plane, h->Lb,
                       h->nbp, h->Bp, h->d.N, h->d.n, h->d.m, h->box_k0, h->box_k1, primal ? 1 : 0, dual ? 1 : 0, h->Lc,
                       h->cmeta, h->ncrows, h->flags.mask());
    HIPCHK(h, hipGetLastError());
    return ALTRO_OK;
  });
}

int32_t altro_batch_set_options(altro_handle* h, const altro_opts* o) {
  return guard(h, [&]() -> int32_t {
    if (!h || !o) return ALTRO_ERR_INVALID_ARG;
    h->o = *o;
    if (h->wide) { h->wide->o = *o; h->wide->gains_valid = false; return ALTRO_OK; }
    HIPCHK(h, hipSetDevice(h->device));
    return drop_gains(h);
  });
}

// solve!(::ProjectedNewtonSolver) after the AL kernel of a plain solve (altro_opts.projected_newton).
// prepare_polish: every check and allocation the polish needs -- run BEFORE a launch takes its slot of the timing ring, so
// that a failure leaves no slot with a start event and no end event.
static int prepare_polish(altro_handle* h) {
  int nbounded = 0;
  for (int j = 0; j < LW; ++j) nbounded += h->bslot_h[j] >= 0 ? 1 : 0;
  const int bm = 2 * h->d.n + (h->box_k1 >= h->box_k0 ? 2 * nbounded : 0) + (h->ncrows > 0 ? LW : 0);
  if (bm > altro_pn::BMAX) FAIL(h, ALTRO_ERR_UNSUPPORTED, "projected_newton: more rows per knot than pn_polish.h holds");
  HIPCHK(h, h->pn_ws.alloc(h->pool, h->stream, (int)h->Bp, h->d.N, bm, LW, false));
  return ALTRO_OK;
}

// mask: the instances to polish (null: all) -- the active mask, or under an episode clock the mask of the step just solved
static int launch_polish(altro_handle* h, const int* mask) {
  altro_pn::PnParams q{};
  q.B = h->d.batch; q.Bp = h->Bp; q.N = h->d.N; q.Nt = h->Nt; q.n = h->d.n; q.m = h->d.m;
  q.box_k0 = h->box_k0; q.box_k1 = h->box_k1; q.ncrows = h->ncrows;
  q.con_istride = h->con_per_instance ? (unsigned)(h->d.N * LW * LW) : 0u;
  q.Grow = h->Grow; q.fvec = h->fvec; q.wd = h->wd; q.wf = h->wf; q.zmin = h->zmin; q.zmax = h->zmax; q.x0 = h->x0;
  q.wstride = q.bstride = tab_imask(h) == 15u ? 0u : (unsigned)LW;
  q.Acon = h->Acon; q.bcon = h->bcon; q.cmeta = h->cmeta; q.active = mask;
  q.Z = h->Z; q.Zref = h->Zref; q.kref = h->kref; q.win = h->clock.on ? h->clock.window : nullptr; q.cur = h->cur; q.status = h->status; q.cost = h->cost; q.cmax = h->cmax;
  q.Lb = h->Lb; q.Lc = h->Lc; q.bslot = h->bslot; q.nbp = h->nbp;
  q.out = h->pn_out; q.ws = h->pn_ws;
  q.o = h->o;
  hipLaunchKernelGGL(altro_pn::pn_kernel, dim3(h->d.batch), dim3(64), 0, h->stream, q);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

static int enqueue_solve(altro_handle* h, int first_step, int nsteps) {
  HIPCHK(h, hipSetDevice(h->device));
  int rc = h->check_ready();
  if (rc) return rc;
  if ((rc = pack_constraints(h))) return rc;
  h->con_locked = true;
  // (under an episode clock every instance has a window of its own, kept inside the track by the tick rule on the device)
  const int last_kref = nsteps > 0 ? first_step + nsteps : h->kref;
  if (!h->clock.on && last_kref + h->d.N > h->Nt) FAIL(h, ALTRO_ERR_STATE, "reference window runs past the end of the stored trajectory");
  // everything that can refuse the launch comes before it takes a slot of the timing ring
  if (h->o.projected_newton && (rc = prepare_polish(h))) return rc;
  if (!supported_dims(h->d.n, h->d.m)) FAIL(h, ALTRO_ERR_UNSUPPORTED, "no kernel built for this (n, m)");
  hipEvent_t h0, h1;
  HIPCHK(h, h->ring.next(&h0, &h1));
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  HIPCHK(h, hipEventRecord(h0, h->stream));
  if (h->o.projected_newton && nsteps > 0) {
    // solve!(::ALTROSolver) ends with the polish, and the next step's shift starts from what it left: the steps of a fused
    // launch run as nsteps pairs of (one-step solve kernel, polish kernel) on the stream, the polish over the step's window
    const int kref0 = h->kref;
    for (int s = 0; s < nsteps && !rc; ++s) {
      const int* mask = h->flags.mask();
      if (h->clock.on) {   // the polish and the log kernel skip the instances that are idle AT THIS STEP
        hipLaunchKernelGGL(altro::k_clock_step_mask, altro::EpisodeClock::grid(h->Bp), dim3(256), 0, h->stream, h->clock.stepmask, h->clock.args(),
                           h->flags.mask(), first_step + s, h->Nt, h->d.N, 0, 0, h->Bp);
        if (hipGetLastError() != hipSuccess) { h->err = "launch of the step-mask kernel failed"; rc = ALTRO_ERR_HIP; break; }
        mask = h->clock.stepmask;
      }
      rc = launch_solve(h, first_step + s, 1);
      h->kref = first_step + s + 1;
      if (!rc) rc = launch_polish(h, mask);
      if (!rc && h->mlog) {
        double* rec0 = h->mlog + (size_t)(first_step + s) * (size_t)h->d.batch * h->mlog_rec;
        hipLaunchKernelGGL(k_log_polished, grid_for((size_t)h->d.batch), dim3(256), 0, h->stream, rec0, h->Z, h->cur, (size_t)h->d.N * LW,
                           h->cost, h->cmax, h->status, mask, h->d.batch, h->d.N, h->d.n, h->d.m);
        if (hipGetLastError() != hipSuccess) { h->err = "launch of the log kernel failed"; rc = ALTRO_ERR_HIP; }
      }
    }
    if (rc) h->kref = kref0;
  } else {
    rc = launch_solve(h, first_step, nsteps);
    if (!rc && h->o.projected_newton) rc = launch_polish(h, h->flags.mask());
  }
  // (a launch that failed after all -- a HIP error -- still closes its slot: every slot handed out has both events)
  HIPCHK(h, hipEventRecord(h1, h->stream));
  if (rc) return rc;
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  h->timed = true;
  if (nsteps > 0) h->kref = first_step + nsteps;
  return ALTRO_OK;
}

int32_t altro_batch_solve_async(altro_handle* h) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, enqueue(0, 0, 0));
    return enqueue_solve(h, 0, 0);
  });
}

int32_t altro_batch_synchronize(altro_handle* h) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).synchronize());
  });
}

int32_t altro_batch_solve(altro_handle* h) {
  return guard(h, [&]() -> int32_t {
    int rc = altro_batch_solve_async(h);
    if (rc) return rc;
    return altro_batch_synchronize(h);
  });
}

static int get_traj(altro_handle* h, double* X, double* U, bool dev = false) {
  HIPCHK(h, hipSetDevice(h->device));
  const size_t B = h->d.batch, N = h->d.N, n = h->d.n, m = h->d.m;
  const size_t cx = B * N * n, cu = B * (N - 1) * m;
  const size_t plane = N * (size_t)LW;
  if (dev) {  // the unpack kernel writes the caller's device arrays; only enqueued
    hipLaunchKernelGGL(k_unpack_traj, grid_for(B * LW), dim3(256), 0, h->stream, X, U, h->Z, h->cur, plane, (int)B, h->Bp, (int)N,
                       (int)n, (int)m);
    HIPCHK(h, hipGetLastError());
    return ALTRO_OK;
  }
  int rc = h->ensure_stage((cx + cu) * sizeof(double));
  if (rc) return rc;
  hipLaunchKernelGGL(k_unpack_traj, grid_for(B * LW), dim3(256), 0, h->stream, X ? h->stage : nullptr,
                     U ? h->stage + cx : nullptr, h->Z, h->cur, plane, (int)B, h->Bp, (int)N, (int)n, (int)m);
  HIPCHK(h, hipGetLastError());
  if (X) HIPCHK(h, hipMemcpyAsync(X, h->stage, cx * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (U) HIPCHK(h, hipMemcpyAsync(U, h->stage + cx, cu * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return ALTRO_OK;
}

int32_t altro_batch_get_states(altro_handle* h, double* X) {
  return guard(h, [&]() -> int32_t {
    if (!h || !X) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, get_planes(X, nullptr));
    return get_traj(h, X, nullptr);
  });
}

int32_t altro_batch_get_controls(altro_handle* h, double* U) {
  return guard(h, [&]() -> int32_t {
    if (!h || !U) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, get_planes(nullptr, U));
    return get_traj(h, nullptr, U);
  });
}

static int duals_xfer(altro_handle* h, int32_t con_id, double* lambda, int to_host) {
  HIPCHK(h, hipSetDevice(h->device));
  for (const auto& cb : h->cons) {
    if (cb.id != con_id) continue;
    const size_t nk = cb.k1 - cb.k0 + 1;
    const size_t cnt = (size_t)h->d.batch * nk * cb.p;
    int rc = h->ensure_stage(cnt * sizeof(double));
    if (rc) return rc;
    if (!to_host && (rc = upload(h, lambda, cnt))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->lanebuf, cb.lanes, LW * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_cduals, grid_for((size_t)h->d.batch * cb.p), dim3(256), 0, h->stream, h->stage, h->Lc,
                       h->d.batch, h->d.N, h->lanebuf, cb.p, cb.k0, cb.k1, to_host);
    HIPCHK(h, hipGetLastError());
    if (to_host) HIPCHK(h, hipMemcpyAsync(lambda, h->stage, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ALTRO_OK;
  }
  if (con_id != h->box_id || h->box_id < 0) FAIL(h, ALTRO_ERR_INVALID_ARG, "unknown constraint id");
  const int nz = h->d.n + h->d.m;
  const size_t nk = h->box_k1 - h->box_k0 + 1;
  const size_t cnt = (size_t)h->d.batch * nk * 2 * nz;
  int rc = h->ensure_stage(cnt * sizeof(double));
  if (rc) return rc;
  if (!to_host && (rc = upload(h, lambda, cnt))) return rc;
  hipLaunchKernelGGL(k_duals, grid_for((size_t)h->Bp * LW), dim3(256), 0, h->stream, h->stage, h->Lb, h->bslot, h->nbp,
                     h->d.batch, h->Bp, h->d.N, nz, h->box_k0, h->box_k1, to_host);
  HIPCHK(h, hipGetLastError());
  if (to_host) HIPCHK(h, hipMemcpyAsync(lambda, h->stage, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return ALTRO_OK;
}

int32_t altro_batch_get_duals(altro_handle* h, int32_t con_id, double* lambda) {
  return guard(h, [&]() -> int32_t {
    if (!h || !lambda) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, duals(con_id, lambda, false));
    return duals_xfer(h, con_id, lambda, 1);
  });
}

int32_t altro_batch_set_duals(altro_handle* h, int32_t con_id, const double* lambda) {
  return guard(h, [&]() -> int32_t {
    if (!h || !lambda) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, duals(con_id, const_cast<double*>(lambda), true));
    return duals_xfer(h, con_id, const_cast<double*>(lambda), 0);
  });
}

int32_t altro_batch_get_stats(altro_handle* h, int32_t* iterations, int32_t* iterations_outer, int32_t* status,
                              double* cost, double* c_max, double* cost_trace, double* cmax_trace) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).get_stats(iterations, iterations_outer, status, cost, c_max, cost_trace, cmax_trace));
  });
}

int32_t altro_batch_get_alpha_trace(altro_handle* h, double* alpha_trace) {
  return guard(h, [&]() -> int32_t {
    if (!h || !alpha_trace) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).get_alpha_trace(alpha_trace));
  });
}

// KD of the handle on the host (gains, factors of Quu and, where the last launch's kernel keeps it there, d)
static int fetch_kd(altro_handle* h, std::vector<double>& kd) {
  kd.resize((size_t)h->d.N * h->Bp * h->d.m * LW);
  HIPCHK(h, hipMemcpy(kd.data(), h->KD, kd.size() * sizeof(double), hipMemcpyDeviceToHost));
  return ALTRO_OK;
}

int32_t altro_batch_get_gains(altro_handle* h, double* K, double* d) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    // (both null: the header says only that either may be; the 16-lane backend has always refused it, the wide one copies nothing)
    if (!K && !d && !h->wide) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, get_gains(K, d));
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t n = h->d.n, m = h->d.m, N = h->d.N, B = h->d.batch, Bp = h->Bp;
    std::vector<double> kd;
    if (int rc = fetch_kd(h, kd)) return rc;
    // an iteration confirmed by the costate sweep ran no backward pass: K is the previous pass's (the same
    // matrix: the active set was verified unchanged), its feedforward terms are zero (include/altro_batch.h, strict)
    std::vector<int> dz(Bp);
    HIPCHK(h, hipMemcpy(dz.data(), h->dzero, Bp * sizeof(int), hipMemcpyDeviceToHost));
    // device layout KD [instance][k][control a][lane]: state lane j holds K[a][j] (the control lanes carry the factors of
    // Quu and, in the box-only kernels, d: altro::kd_drow / kd_dcol); Dff [instance][k (N + 1 rows)][lane], conic kernels:
    // control lane n+a holds d[a].  Which of the two the last launch wrote: launch_solve recorded it
    const bool dkd = h->d_in_kd;
    std::vector<double> df;
    if (d && !dkd) {
      df.resize((N + 1) * Bp * LW);
      HIPCHK(h, hipMemcpy(df.data(), h->Dff, df.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (size_t b = 0; b < B; ++b)
      for (size_t k = 0; k + 1 < N; ++k)
        for (size_t a = 0; a < m; ++a) {
          const double* row = kd.data() + ((b * N + k) * m + a) * LW;
          if (K) for (size_t j = 0; j < n; ++j) K[((b * (N - 1) + k) * n + j) * m + a] = row[j];
          if (d) {
            const double da = dkd ? kd[((b * N + k) * m + altro::kd_drow((int)a)) * LW + n + altro::kd_dcol((int)a, (int)m)]
                                  : df[(b * (N + 1) + k) * LW + n + a];
            d[(b * (N - 1) + k) * m + a] = dz[b] ? 0.0 : da;
          }
        }
    return ALTRO_OK;
  });
}

int32_t altro_batch_get_gain_factors(altro_handle* h, double* F) {
  return guard(h, [&]() -> int32_t {
    if (!h || !F) return ALTRO_ERR_INVALID_ARG;
    if (h->wide) FAIL(h, ALTRO_ERR_UNSUPPORTED, "the one-wave-per-instance kernels keep no factors of Quu");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t n = h->d.n, m = h->d.m, N = h->d.N, B = h->d.batch;
    std::vector<double> kd;
    if (int rc = fetch_kd(h, kd)) return rc;
    for (size_t b = 0; b < B; ++b)
      for (size_t k = 0; k + 1 < N; ++k)
        for (size_t a = 0; a < m; ++a)
          for (size_t c = 0; c < m; ++c)   // control lane n + c of gain row a: entry (a, c) of the factors, c <= a
            F[((b * (N - 1) + k) * m + a) * m + c] = (c <= a) ? kd[((b * N + k) * m + a) * LW + n + c] : 0.0;
    return ALTRO_OK;
  });
}

int32_t altro_batch_last_solve_ms(altro_handle* h, float* ms) {
  return guard(h, [&]() -> int32_t {
    if (!h || !ms) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).last_solve_ms(ms));
  });
}

int32_t altro_batch_timing_reset(altro_handle* h) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).timing_reset());
  });
}

int32_t altro_batch_timing_get(altro_handle* h, float* ms, int32_t capacity, int32_t* count) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    // (count null: the header is silent; the 16-lane backend has always refused it, the wide one takes it as "not asked for")
    if (!count && !h->wide) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).timing_get(ms, capacity, count));
  });
}

int32_t altro_batch_get_solve_counters(altro_handle* h, int64_t* solves, int64_t* iterations, int64_t* succeeded) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    altro::BackendCommon& c = common(h);
    long long* const src[3] = {c.n_solves, c.n_iters, c.n_ok};
    return fwd(h, c.counters(src, solves, iterations, succeeded));
  });
}

int32_t altro_batch_get_work_counters(altro_handle* h, int64_t* backward_passes, int64_t* rollouts, int64_t* trials) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    altro::BackendCommon& c = common(h);
    long long* const src[3] = {c.n_backward, c.n_rollout, c.n_trials};
    return fwd(h, c.counters(src, backward_passes, rollouts, trials));
  });
}

int32_t altro_batch_get_reuse_counter(altro_handle* h, int64_t* reused) {
  return guard(h, [&]() -> int32_t {
    if (!h || !reused) return ALTRO_ERR_INVALID_ARG;
    long long* const src[3] = {common(h).n_reuse, nullptr, nullptr};
    return fwd(h, common(h).counters(src, reused, nullptr, nullptr));
  });
}

// Both polish getters on both backends (BackendCommon::read_polish): zeros while projected_newton is off, or before a handle
// on the one-wave-per-instance backend has polished.  (Only the 16-lane backend, whose arrays exist from create on, puts the
// statistics back to zero when they are asked for while the option is off.)
int32_t altro_batch_get_polish_stats(altro_handle* h, int32_t* ran, int32_t* failed, double* residual) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).read_polish(!h->wide, ran, failed, residual, nullptr, nullptr, nullptr));
  });
}

int32_t altro_batch_get_polish_dual_residuals(altro_handle* h, double* before, double* after, int32_t* failed) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).read_polish(false, nullptr, nullptr, nullptr, before, after, failed));
  });
}

int32_t altro_batch_get_confirm_counter(altro_handle* h, int64_t* confirmed) {
  return guard(h, [&]() -> int32_t {
    if (!h || !confirmed) return ALTRO_ERR_INVALID_ARG;
    long long* const src[3] = {common(h).n_gconf, nullptr, nullptr};
    return fwd(h, common(h).counters(src, confirmed, nullptr, nullptr));
  });
}

int32_t altro_batch_get_wave_cycles(altro_handle* h, int64_t* cycles, int32_t capacity, int32_t* count) {
  return guard(h, [&]() -> int32_t {
    if (h && h->wide) { if (count) *count = 0; return ALTRO_OK; }
    if (!h || !count) return ALTRO_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // (diagnostic builds append a 4096-word per-turn trace of one wave, ALTRO_DEBUG_TRACE_WAVE: returned to callers that
    //  offer the room)
    const int32_t n = h->Bp / IPW * 16 + ((capacity >= h->Bp / IPW * 16 + 4096) ? 4096 : 0);
    *count = n;
    if (cycles) HIPCHK(h, hipMemcpy(cycles, h->wave_cycles, (size_t)(n < capacity ? n : capacity) * sizeof(long long), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  });
}

int32_t altro_batch_get_wave_passes(altro_handle* h, int64_t* passes, int32_t capacity, int32_t* count) {
  return guard(h, [&]() -> int32_t {
    if (h && h->wide) { if (count) *count = 0; return ALTRO_OK; }
    if (!h || !count) return ALTRO_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int32_t n = h->Bp / IPW * 8;
    *count = n;
    if (passes) HIPCHK(h, hipMemcpy(passes, h->wave_cycles + (size_t)h->Bp / IPW * 16 + 4096, (size_t)(n < capacity ? n : capacity) * sizeof(long long), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  });
}

int32_t altro_mpc_set_track(altro_handle* h, const double* Xtrack, const double* Utrack, int32_t Nt) {
  return guard(h, [&]() -> int32_t {
    if (!h || !Xtrack || !Utrack) return ALTRO_ERR_INVALID_ARG;
    if (Nt < h->d.N) FAIL(h, ALTRO_ERR_INVALID_ARG, "track shorter than the horizon");
    WIDE_FWD(h, mpc_set_track(Xtrack, Utrack, Nt));
    HIPCHK(h, hipSetDevice(h->device));
    int rc = set_ref_common(h, Xtrack, Utrack, Nt);
    if (rc) return rc;
    // initial_trajectory!(prob, Z): the first window of the track (mpc.jl:19-20,45)
    HIPCHK(h, hipMemsetAsync(h->cur, 0, h->Bp * sizeof(int), h->stream));
    hipLaunchKernelGGL(k_window_copy, grid_for((size_t)h->Bp * LW), dim3(256), 0, h->stream, h->Z, h->Zref, h->Bp, h->d.N, Nt);
    HIPCHK(h, hipGetLastError());
    // x0 <- the track's first state, through the pack path (its lanes >= n must be zero)
    {
      const size_t cnt = (size_t)h->d.batch * h->d.n;
      std::vector<double> x0(cnt);
      const size_t n = h->d.n;
      for (size_t b = 0; b < (size_t)h->d.batch; ++b)
        for (size_t j = 0; j < n; ++j) x0[b * n + j] = Xtrack[(b * Nt + 0) * n + j];
      HIPCHK(h, hipStreamSynchronize(h->stream));
      rc = altro_batch_set_initial_state(h, x0.data());
      if (rc) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ALTRO_OK;
  });
}

int32_t altro_mpc_set_noise(altro_handle* h, const double* noise, int32_t steps) {
  return guard(h, [&]() -> int32_t {
    if (!h || !noise || steps < 1) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).set_noise(noise, steps));
  });
}

int32_t altro_mpc_set_noise_model(altro_handle* h, int32_t mode, const double* weights, const int32_t* groups) {
  return guard(h, [&]() -> int32_t {
    if (!h || !weights || mode < 0 || mode > 2) return ALTRO_ERR_INVALID_ARG;
    for (int i = 0; groups && i < h->d.n; ++i)
      if (groups[i] != 0 && groups[i] != 1) FAIL(h, ALTRO_ERR_INVALID_ARG, "noise groups are 0 or 1");
    return fwd(h, common(h).set_noise_model(mode, weights, groups));
  });
}

int32_t altro_mpc_set_shift(altro_handle* h, int32_t shift) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    common(h).mpc_shift = shift ? 1 : 0;
    return ALTRO_OK;
  });
}

int32_t altro_mpc_run_async(altro_handle* h, int32_t first_step, int32_t nsteps) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    if (int rc = fwd(h, common(h).mpc_run_rules(first_step, nsteps))) return rc;
    WIDE_FWD(h, enqueue(1, first_step, nsteps));
    return enqueue_solve(h, first_step, nsteps);
  });
}

int32_t altro_mpc_step_async(altro_handle* h, int32_t step) { return altro_mpc_run_async(h, step, 1); }

int32_t altro_mpc_set_log(altro_handle* h, int32_t capacity_steps) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    if (capacity_steps < 0) FAIL(h, ALTRO_ERR_INVALID_ARG, "negative log capacity");
    return fwd(h, common(h).set_log(capacity_steps));
  });
}

int32_t altro_mpc_get_log(altro_handle* h, int32_t first_step, int32_t nsteps, double* x0, double* u0, int32_t* iterations,
                          int32_t* iterations_outer, int32_t* status, double* cost, double* c_max) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    return fwd(h, common(h).get_log(first_step, nsteps, x0, u0, iterations, iterations_outer, status, cost, c_max));
  });
}

int32_t altro_mpc_set_dynamics_track(altro_handle* h, const double* A, const double* B, const double* f, int32_t nblocks,
                                     int32_t step_stride, int32_t per_instance) {
  return guard(h, [&]() -> int32_t {
    if (!h || !A || !B) return ALTRO_ERR_INVALID_ARG;
    if (!h->wide) {
      const int rc = migrate_to_wide(h);
      if (rc) return rc;
    }
    return fwd(h, h->wide->mpc_set_dynamics_track(A, B, f, nblocks, step_stride, per_instance));
  });
}

int32_t altro_mpc_prepare_async(altro_handle* h, int32_t step) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    WIDE_FWD(h, mpc_prepare(step));   // (the shared step rules, then its two of the dynamics track)
    if (int rc = h->mpc_prepare_rules(step)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = h->check_ready();
    if (rc) return rc;
    if ((rc = launch_solve(h, step, 1, 1))) return rc;  // the solve kernel's own plant step, nothing else
    h->kref = step + 1;
    return ALTRO_OK;
  });
}

int32_t altro_batch_benchmark_solve(altro_handle* h, int32_t samples, int32_t evals, float* sample_ms) {
  return guard(h, [&]() -> int32_t {
    if (!h) return ALTRO_ERR_INVALID_ARG;
    if (samples < 1 || evals < 1) FAIL(h, ALTRO_ERR_INVALID_ARG, "samples and evals must be positive");
    if (common(h).flags.on) FAIL(h, ALTRO_ERR_STATE, "altro_batch_benchmark_solve restores and repeats whole batches: clear the active mask first");
    if (common(h).clock.on) FAIL(h, ALTRO_ERR_STATE, "altro_batch_benchmark_solve restores and repeats whole batches: clear the episode clock first");
    WIDE_FWD(h, benchmark_solve(samples, evals, sample_ms));
    HIPCHK(h, hipSetDevice(h->device));
    const size_t plane = (size_t)h->d.N * LW;
    if (!h->Zsave) HIPCHK(h, h->pool.alloc(&h->Zsave, plane * h->Bp, h->stream, false));
    const dim3 grid = grid_for((size_t)h->Bp * LW);
    // Z0 = deepcopy(get_trajectory(solver))
    hipLaunchKernelGGL(k_plane_copy, grid, dim3(256), 0, h->stream, h->Z, h->Zsave, h->cur, plane, h->Bp, h->d.N, 1);
    HIPCHK(h, hipGetLastError());
    auto one = [&]() -> int {  // initial_trajectory!(solver, Z0); solve!(solver)
      hipLaunchKernelGGL(k_plane_copy, grid, dim3(256), 0, h->stream, h->Z, h->Zsave, h->cur, plane, h->Bp, h->d.N, 0);
      // every evaluation recomputes its gains, as an evaluation of the reference's `@benchmark solve!` does (the gains of
      // the previous evaluation would otherwise serve the next one: same start, same active sets)
      if (int rcd = drop_gains(h)) return rcd;
      return enqueue_solve(h, 0, 0);
    };
    int rc = one();  // BenchmarkTools' warm-up evaluation
    if (rc) return rc;
    for (int32_t s = 0; s < samples; ++s) {
      HIPCHK(h, hipEventRecord(h->bev0, h->stream));
      for (int32_t e = 0; e < evals; ++e)
        if ((rc = one())) return rc;
      HIPCHK(h, hipEventRecord(h->bev1, h->stream));
      HIPCHK(h, hipEventSynchronize(h->bev1));
      float ms = 0.f;
      HIPCHK(h, hipEventElapsedTime(&ms, h->bev0, h->bev1));
      if (sample_ms) sample_ms[s] = ms / (float)evals;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ALTRO_OK;
  });
}

// ------------------------------------------------------------------ device-pointer I/O (include/altro_batch.h)
// Every entry point validates ALL its pointers first (device_io.h: dev_extent_check) and refuses with ALTRO_ERR_INVALID_ARG
// before anything is enqueued or changed; then it only enqueues on the handle's stream.
static int32_t dev_null_handle(const char* fn) {
  g_create_err = std::string(fn) + ": null handle";
  return ALTRO_ERR_INVALID_ARG;
}
static int dev_arg(altro_handle* h, const char* fn, const char* what, const void* p, size_t bytes, bool optional = false) {
  if (!p && optional) return ALTRO_OK;
  if (const char* e = altro::dev_extent_check(p, bytes, h->device))
    FAIL(h, ALTRO_ERR_INVALID_ARG, std::string(fn) + ": " + what + ": " + e);
  return ALTRO_OK;
}
#define DEV_ENTER(h, fn)                      \
  if (!(h)) return dev_null_handle(fn);       \
  HIPCHK(h, hipSetDevice((h)->device));       \
  const char* const fn_ = fn;                 \
  const size_t B_ = (h)->d.batch, N_ = (h)->d.N, n_ = (h)->d.n, m_ = (h)->d.m; \
  (void)B_; (void)N_; (void)n_; (void)m_
#define DEV_ARG(h, what, p, count, type, optional)                                         \
  do {                                                                                      \
    if (int rc_ = dev_arg(h, fn_, what, p, (size_t)(count) * sizeof(type), optional)) return rc_; \
  } while (0)

int32_t altro_batch_set_initial_state_dev(altro_handle* h, const double* x0) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_set_initial_state_dev");
    DEV_ARG(h, "x0", x0, B_ * n_, double, false);
    WIDE_FWD(h, set_initial_state_dev(x0));
    return set_x0_16(h, x0, true);
  });
}

int32_t altro_batch_get_initial_state_dev(altro_handle* h, double* x0) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_get_initial_state_dev");
    DEV_ARG(h, "x0", x0, B_ * n_, double, false);
    WIDE_FWD(h, get_initial_state_dev(x0));
    return get_x0_16(h, x0, true);
  });
}

int32_t altro_batch_set_reference_dev(altro_handle* h, const double* Xref, const double* Uref) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_set_reference_dev");
    DEV_ARG(h, "Xref", Xref, B_ * N_ * n_, double, false);
    DEV_ARG(h, "Uref", Uref, B_ * (N_ - 1) * m_, double, false);
    WIDE_FWD(h, set_reference_dev(Xref, Uref));
    return set_ref_common(h, Xref, Uref, h->d.N, true);
  });
}

int32_t altro_batch_set_initial_trajectory_dev(altro_handle* h, const double* X, const double* U) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_set_initial_trajectory_dev");
    DEV_ARG(h, "X", X, B_ * N_ * n_, double, true);
    DEV_ARG(h, "U", U, B_ * (N_ - 1) * m_, double, false);
    WIDE_FWD(h, set_initial_trajectory_dev(X, U));
    return set_traj_16(h, X, U, true);
  });
}

int32_t altro_batch_set_dynamics_dev(altro_handle* h, const double* A, const double* B, const double* f, int32_t per_knot,
                                     int32_t per_instance) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_set_dynamics_dev");
    const size_t nb = (per_instance ? B_ : 1) * (per_knot ? N_ - 1 : 1);
    DEV_ARG(h, "A", A, nb * n_ * n_, double, false);
    DEV_ARG(h, "B", B, nb * n_ * m_, double, false);
    DEV_ARG(h, "f", f, nb * n_, double, true);
    if (per_knot && !h->wide) {  // the first call on an (n, m) of the 16-lane set: the handle moves to the one-wave-per-instance kernel
      if (int rc = migrate_to_wide(h)) return rc;
    }
    WIDE_FWD(h, set_dynamics_dev(A, B, f, per_knot, per_instance));
    return set_dynamics_16(h, A, B, f, per_instance, true);
  });
}

int32_t altro_batch_get_states_dev(altro_handle* h, double* X) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_get_states_dev");
    DEV_ARG(h, "X", X, B_ * N_ * n_, double, false);
    WIDE_FWD(h, get_planes_dev(X, nullptr));
    return get_traj(h, X, nullptr, true);
  });
}

int32_t altro_batch_get_controls_dev(altro_handle* h, double* U) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_get_controls_dev");
    DEV_ARG(h, "U", U, B_ * (N_ - 1) * m_, double, false);
    WIDE_FWD(h, get_planes_dev(nullptr, U));
    return get_traj(h, nullptr, U, true);
  });
}

int32_t altro_batch_get_first_knot_dev(altro_handle* h, double* u0, double* x1, int32_t* status, int32_t* iterations) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_get_first_knot_dev");
    DEV_ARG(h, "u0", u0, B_ * m_, double, true);
    DEV_ARG(h, "x1", x1, B_ * n_, double, true);
    DEV_ARG(h, "status", status, B_, int32_t, true);
    DEV_ARG(h, "iterations", iterations, B_, int32_t, true);
    if (!u0 && !x1 && !status && !iterations) return ALTRO_OK;
    WIDE_FWD(h, get_first_knot_dev(u0, x1, status, iterations));
    hipLaunchKernelGGL(altro::k_first_knot, grid_for(B_ * LW), dim3(256), 0, h->stream, u0, x1, status, iterations, h->Z, h->cur,
                       h->status, h->iters, N_ * (size_t)LW, (int)B_, (int)N_, (int)n_, (int)m_);
    HIPCHK(h, hipGetLastError());
    return ALTRO_OK;
  });
}

// ---- constraint data and bounds from device pointers
// altro_batch_update_constraint_data with A, b on the device: the rows go straight to the constraint's lanes of Acon / bcon.
// cmeta, ckn, the duals and the lane assignment are untouched.  con_inv (the sweeps load a lane's row once, from its
// canonical knot) survives only an update that cannot break it: one shared block, fanned out to every knot.
int32_t altro_batch_update_constraint_data_dev(altro_handle* h, int32_t con_id, const double* A, const double* b) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_update_constraint_data_dev");
    const int box_id = common(h).box_id;
    if (box_id >= 0 && con_id == box_id) FAIL(h, ALTRO_ERR_INVALID_ARG, std::string(fn_) + ": con_id is a BOX constraint (altro_batch_set_bounds_dev)");
    altro_handle::ConBlock* cb = nullptr;
    altro_wide::WideBackend::Block* bl = nullptr;
    size_t nblk = 0, p = 0;
    if (h->wide) {
      if ((bl = h->wide->find(con_id))) {
        nblk = (bl->per_knot ? (size_t)(bl->k1 - bl->k0 + 1) : 1) * (bl->per_instance ? B_ : 1);
        p = bl->p;
      }
    } else {
      for (auto& c : h->cons)
        if (c.id == con_id) cb = &c;
      if (cb) {
        nblk = (cb->per_knot ? (size_t)(cb->k1 - cb->k0 + 1) : 1) * (cb->per_instance ? B_ : 1);
        p = cb->p;
      }
    }
    if (!nblk) FAIL(h, ALTRO_ERR_INVALID_ARG, std::string(fn_) + ": unknown constraint id");
    if (!A && !b) FAIL(h, ALTRO_ERR_INVALID_ARG, std::string(fn_) + ": A and b are both null");
    DEV_ARG(h, "A", A, nblk * p * (n_ + m_), double, true);
    DEV_ARG(h, "b", b, nblk * p, double, true);
    WIDE_FWD(h, update_constraint_data_dev(bl, A, b));
    if (h->con_dirty) {   // (only after a packing that failed: the tables are rebuilt on the host first)
      if (int rc = pack_constraints(h)) return rc;
    }
    altro::ConLanes lanes{};
    for (int r = 0; r < LW; ++r) lanes.lane[r] = cb->lanes[r] >= 0 ? cb->lanes[r] : 0;
    const int nk = cb->k1 - cb->k0 + 1;
    const size_t ninst = h->con_per_instance ? (size_t)h->Bp : 1;
    hipLaunchKernelGGL(altro::k_pack_con_rows, grid_for(ninst * nk * p * LW), dim3(256), 0, h->stream, h->Acon, h->bcon, A, b, lanes, (int)ninst,
                       (int)B_, (int)N_, (int)(n_ + m_), cb->k0, nk, (int)p, cb->per_knot, cb->per_instance);
    HIPCHK(h, hipGetLastError());
    if (cb->per_knot || cb->per_instance) h->con_inv = 0;
    cb->stale = true;
    return drop_gains(h);
  });
}

// altro_batch_set_bounds with zmin, zmax on the device: checked and written row by row on the device (device_io.h:
// k_set_bounds_rows).  Going from one shared row to one row per instance is the one case that changes the tables' shape: it
// goes through upload_tables (every row starts as the old shared row), which synchronises.  A shared row given while the
// tables hold one row per instance is written to every row and the tables keep their shape: equal rows, the same results.
int32_t altro_batch_set_bounds_dev(altro_handle* h, int32_t con_id, const double* zmin, const double* zmax, int32_t per_instance) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_set_bounds_dev");
    const int box_id = common(h).box_id;
    if (box_id < 0 || con_id != box_id) FAIL(h, ALTRO_ERR_INVALID_ARG, std::string(fn_) + ": con_id is not a BOX constraint");
    const size_t rows = per_instance ? B_ : 1;
    DEV_ARG(h, "zmin", zmin, rows * (n_ + m_), double, false);
    DEV_ARG(h, "zmax", zmax, rows * (n_ + m_), double, false);
    WIDE_FWD(h, set_bounds_dev(zmin, zmax, per_instance));
    if (per_instance && !h->bnd_pi) {
      if (int rc = refresh_bounds_mirror(h)) return rc;
      std::vector<double> lo(B_ * LW), hi(B_ * LW);
      for (size_t r = 0; r < B_; ++r) {
        std::memcpy(&lo[r * LW], h->zmin_h.data(), LW * sizeof(double));
        std::memcpy(&hi[r * LW], h->zmax_h.data(), LW * sizeof(double));
      }
      h->zmin_h.swap(lo);
      h->zmax_h.swap(hi);
      h->bnd_pi = true;
      if (int rc = upload_tables(h)) {   // the handle keeps the shape it had
        h->zmin_h.swap(lo);
        h->zmax_h.swap(hi);
        h->bnd_pi = false;
        return rc;
      }
    }
    altro::FinMask fin{};
    for (int j = 0; j < LW; ++j) {
      if (h->box_lo_fin[j]) fin.lo[0] |= 1ull << j;
      if (h->box_hi_fin[j]) fin.hi[0] |= 1ull << j;
    }
    const size_t trows = (h->cost_pi || h->bnd_pi) ? (size_t)h->Bp : 1;
    hipLaunchKernelGGL(altro::k_set_bounds_rows, grid_for(trows * LW), dim3(256), 0, h->stream, h->zmin, h->zmax, zmin, zmax, fin, (int)(n_ + m_), LW,
                       (int)trows, (int)B_, per_instance ? 1 : 0, h->refusals);
    HIPCHK(h, hipGetLastError());
    h->bnd_stale = true;
    return drop_gains(h);
  });
}

int32_t altro_batch_get_dev_refusals(altro_handle* h, int64_t* rows) {
  return guard(h, [&]() -> int32_t {
    if (!h) return dev_null_handle("altro_batch_get_dev_refusals");
    if (!rows) FAIL(h, ALTRO_ERR_INVALID_ARG, "altro_batch_get_dev_refusals: null pointer");
    return fwd(h, common(h).get_dev_refusals(rows));
  });
}

// ---- host/device twin pairs: a `_dev` form on the caller's device arrays and a host twin on host arrays
// The array arguments of one call of either form, as the pair's table names them (stage_layout.h).  f64() / i32() are what the launch
// gets.  `_dev` form: validate() checks every pointer against its extent, and the launch gets the caller's own pointers.  Host twin:
// open() makes room in the staging buffer of whichever backend the handle runs on and copies in what the caller passed, the launch
// gets the staged sub-arrays, close() copies the outputs back and synchronises once: the SAME kernels run on the staged copies, so
// the bytes are those of the `_dev` call by construction.
struct TwinArgs : altro::StageLayout {
  altro_handle* h;
  const bool host;
  hipStream_t st = nullptr;
  char* base = nullptr;
  TwinArgs(altro_handle* h_, bool host_) : h(h_), host(host_) {}
  int validate(const char* fn) {
    for (int i = 0; i < nslots; ++i)
      if (int rc = dev_arg(h, fn, slot[i].name, slot[i].arg(), slot[i].extent, !slot[i].required)) return rc;
    return ALTRO_OK;
  }
  int open() {
    if (int rc = fwd(h, common(h).ensure_stage(bytes))) return rc;
    st = common(h).stream;
    base = reinterpret_cast<char*>(common(h).stage);
    for (int i = 0; i < nslots; ++i)
      if (slot[i].in) HIPCHK(h, hipMemcpyAsync(base + slot[i].off, slot[i].in, slot[i].bytes, hipMemcpyHostToDevice, st));
    return ALTRO_OK;
  }
  void* dev(int i) const { return !host ? const_cast<void*>(slot[i].arg()) : slot[i].dev ? base + slot[i].off : nullptr; }
  double* f64(int i) const { return static_cast<double*>(dev(i)); }
  int32_t* i32(int i) const { return static_cast<int32_t*>(dev(i)); }
  uint8_t* u8(int i) const { return static_cast<uint8_t*>(dev(i)); }
  int close() {
    for (int i = 0; i < nslots; ++i)
      if (slot[i].out) HIPCHK(h, hipMemcpyAsync(slot[i].out, base + slot[i].off, slot[i].bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return ALTRO_OK;
  }
};

// what the launches of the scoring pairs check first on the 16-lane path (the one-wave-per-instance backend has
// WideBackend::eval_ready)
static int score_ready(altro_handle* h) {
  if (int rc = h->check_ready()) return rc;
  if (!h->clock.on && h->kref + h->d.N > h->Nt) FAIL(h, ALTRO_ERR_STATE, "reference window runs past the end of the stored trajectory");
  return pack_constraints(h);   // (what the next solve would do first; a no-op once the tables are packed)
}

// Both forms of every pair: the handle, the pair's argument rules, the device, then the caller's pointers validated (`_dev`) or the
// handle found ready and the arrays staged (host twin), the launch, and for the twin the copies back.  `ready`: the pair's launch
// opens with score_ready / WideBackend::eval_ready; the twin asks first, so that ALTRO_ERR_STATE allocates and copies nothing.
extern "C++" {   // (a template, inside the extern "C" of the entry points)
template <class Rules, class Table, class Launch>
static int32_t twin_call(altro_handle* h, const char* fn, bool host, bool ready, Rules&& rules, Table&& table, Launch&& launch) {
  return guard(h, [&]() -> int32_t {
    if (!h) return dev_null_handle(fn);
    if (int rc = rules()) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    TwinArgs a(h, host);
    table(a);
    if (!host) {
      if (int rc = a.validate(fn)) return rc;
      return launch(a);
    }
    if (ready)
      if (int rc = h->wide ? fwd(h, h->wide->eval_ready()) : score_ready(h)) return rc;
    if (int rc = a.open()) return rc;
    if (int rc = launch(a)) return rc;
    return a.close();
  });
}
}   // extern "C++"

// ---- feedback policy on the device (kernels in policy.h)
// x, knot, u, fb: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues one kernel.
static int eval_policy_launch(altro_handle* h, const double* x, const int32_t* knot, int32_t clamp, double* u, int32_t* fb) {
  if (h->wide) return fwd(h, h->wide->eval_policy_dev(x, knot, clamp, u, fb));
  hipLaunchKernelGGL(altro::k_eval_policy, grid_for((size_t)h->Bp * LW), dim3(256), 0, h->stream, u, fb, x, knot, h->Z, h->cur, h->KD, h->kmu,
                     h->zmin, h->zmax, tab_imask(h), (size_t)h->d.N * LW, h->Bp, h->d.batch, h->d.N, h->d.n, h->d.m, clamp ? 1 : 0, h->box_k0,
                     h->box_k1);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

// the host twin alone: x and u are required and knot is checked on the host, before anything is staged (the `_dev` form cannot
// read knot: its kernel reports an out-of-range knot through fb)
static int eval_policy_host_rules(altro_handle* h, const char* fn, const double* x, const int32_t* knot, const double* u) {
  const std::string f(fn);
  if (!x || !u) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": x and u are required");
  const size_t B = h->d.batch, N = h->d.N;
  for (size_t b = 0; knot && b < B; ++b)
    if (knot[b] < 0 || knot[b] > (int32_t)N - 2)
      FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": knot[" + std::to_string(b) + "] = " + std::to_string(knot[b]) + " is outside 0 .. N-2");
  return ALTRO_OK;
}

static int32_t eval_policy_call(altro_handle* h, const char* fn, bool host, const double* x, const int32_t* knot, int32_t clamp, double* u,
                                int32_t* fb) {
  return twin_call(
      h, fn, host, false, [&] { return host ? eval_policy_host_rules(h, fn, x, knot, u) : ALTRO_OK; },
      [&](TwinArgs& a) { altro::stage_eval_policy(a, h->d.batch, h->d.n, h->d.m, x, knot, u, fb); },
      [&](const TwinArgs& a) {
        return eval_policy_launch(h, a.f64(altro::EP_X), a.i32(altro::EP_KNOT), clamp, a.f64(altro::EP_U), a.i32(altro::EP_FB));
      });
}
int32_t altro_batch_eval_policy_dev(altro_handle* h, const double* x, const int32_t* knot, int32_t clamp, double* u, int32_t* fb) {
  return eval_policy_call(h, "altro_batch_eval_policy_dev", false, x, knot, clamp, u, fb);
}
int32_t altro_batch_eval_policy(altro_handle* h, const double* x, const int32_t* knot, int32_t clamp, double* u, int32_t* fb) {
  return eval_policy_call(h, "altro_batch_eval_policy", true, x, knot, clamp, u, fb);
}

// altro_batch_get_gains on the device: the unpack of KD / Dff that the host call does in a loop (k_unpack_gains), resp. two
// device-to-device copies of Kg / dg
int32_t altro_batch_get_gains_dev(altro_handle* h, double* K, double* d) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_get_gains_dev");
    if (!K && !d) FAIL(h, ALTRO_ERR_INVALID_ARG, std::string(fn_) + ": K and d are both null");
    DEV_ARG(h, "K", K, B_ * (N_ - 1) * n_ * m_, double, true);
    DEV_ARG(h, "d", d, B_ * (N_ - 1) * m_, double, true);
    WIDE_FWD(h, get_gains_dev(K, d));
    altro::DSlots at{};
    for (int a = 0; a < (int)m_; ++a) { at.row[a] = altro::kd_drow(a); at.col[a] = altro::kd_dcol(a, (int)m_); }
    hipLaunchKernelGGL(altro::k_unpack_gains, grid_for(B_ * (N_ - 1) * m_ * LW), dim3(256), 0, h->stream, K, d, h->KD, h->Dff, h->dzero,
                       h->d_in_kd ? 1 : 0, at, (int)B_, (int)N_, (int)n_, (int)m_);
    HIPCHK(h, hipGetLastError());
    return ALTRO_OK;
  });
}

// ---- caller-supplied trajectories scored on the device (kernels in evaluate.h)
// the tables a scoring kernel of evaluate.h / warm_start.h / simulate.h reads, as the solve kernels address them now
static altro::Eval16 eval16_params(altro_handle* h) {
  const size_t N = h->d.N;
  altro::Eval16 p{};
  p.Grow = h->Grow; p.fvec = h->fvec; p.wd = h->wd; p.wf = h->wf; p.zmin = h->zmin; p.zmax = h->zmax; p.Zref = h->Zref;
  p.Acon = h->Acon; p.bcon = h->bcon; p.cmeta = h->cmeta; p.window = h->clock.args().window; p.imask = tab_imask(h);
  p.con_istride = h->con_per_instance ? N * LW * LW : 0; p.ncrows = h->ncrows;
  p.N = (int)N; p.Nt = h->Nt; p.n = h->d.n; p.m = h->d.m; p.kref = h->kref; p.box_k0 = h->box_k0; p.box_k1 = h->box_k1;
  return p;
}

// the argument rules both forms share, checked before anything else
static int evaluate_rules(altro_handle* h, const char* fn, int32_t ncand, const double* U, const double* X, const double* x0, double* J,
                          double* c_max, double* defect, double* Xout) {
  const std::string f(fn);
  if (ncand < 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": ncand must be at least 1");
  if (!U && ncand != 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": the handle's own trajectory (U null) is one candidate: ncand must be 1");
  if (!U && (X || x0 || Xout)) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": X, x0 and Xout must be null when U is null");
  if (X && (x0 || Xout)) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": x0 and Xout belong to the rollout form: they must be null when X is given");
  if (!J && !c_max && !defect) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": J, c_max and defect are all null");
  return ALTRO_OK;
}

// U, X, x0, J, c_max, defect, Xout: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues
// the rollout kernel when there is no X, then the scoring kernel; allocates only when the workspace has to grow.
static int evaluate_launch(altro_handle* h, int32_t ncand, const double* U, const double* X, const double* x0, double* J, double* c_max,
                           double* defect, double* Xout) {
  if (h->wide) return fwd(h, h->wide->evaluate_dev(ncand, U, X, x0, J, c_max, defect, Xout));
  int rc = score_ready(h);
  if (rc) return rc;
  const size_t B = h->d.batch, N = h->d.N, n = h->d.n, m = h->d.m;
  const size_t R = B * (size_t)ncand, lx = N * n, lu = (N - 1) * m;
  const size_t need = !U ? R * (lx + lu) : (!X && !Xout) ? R * lx : 0;
  if (need) HIPCHK(h, h->pool.reserve(&h->eval_ws, &h->eval_ws_elems, need));
  const altro::Eval16 p = eval16_params(h);
  const size_t rows = (R + 3) & ~(size_t)3;   // whole waves of four rows
  int given = 1;
  if (!U) {   // own trajectory: the current plane, unpacked into the workspace in the caller's layout
    if ((rc = get_traj(h, h->eval_ws, h->eval_ws + R * lx, true))) return rc;
    X = h->eval_ws;
    U = h->eval_ws + R * lx;
  } else if (!X) {
    double* Xw = Xout ? Xout : h->eval_ws;
    hipLaunchKernelGGL(altro::k_eval_rollout16, grid_for(rows * LW), dim3(256), 0, h->stream, Xw, U, x0 ? x0 : h->x0, x0 ? (int)n : LW, p, (int)ncand, R, rows);
    HIPCHK(h, hipGetLastError());
    X = Xw;
    given = 0;
  }
  hipLaunchKernelGGL(altro::k_eval_score16, grid_for(rows * LW), dim3(256), 0, h->stream, J, c_max, defect, X, U, p, (int)ncand, R, rows, given);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

static int32_t evaluate_call(altro_handle* h, const char* fn, bool host, int32_t ncand, const double* U, const double* X, const double* x0,
                             double* J, double* c_max, double* defect, double* Xout) {
  return twin_call(
      h, fn, host, true, [&] { return evaluate_rules(h, fn, ncand, U, X, x0, J, c_max, defect, Xout); },
      [&](TwinArgs& a) { altro::stage_evaluate(a, h->d.batch, h->d.N, h->d.n, h->d.m, ncand, U, X, x0, J, c_max, defect, Xout); },
      [&](const TwinArgs& a) {
        return evaluate_launch(h, ncand, a.f64(altro::EV_U), a.f64(altro::EV_X), a.f64(altro::EV_X0), a.f64(altro::EV_J),
                               a.f64(altro::EV_CMAX), a.f64(altro::EV_DEFECT), a.f64(altro::EV_XOUT));
      });
}
int32_t altro_batch_evaluate_dev(altro_handle* h, int32_t ncand, const double* U, const double* X, const double* x0, double* J, double* c_max,
                                 double* defect, double* Xout) {
  return evaluate_call(h, "altro_batch_evaluate_dev", false, ncand, U, X, x0, J, c_max, defect, Xout);
}
int32_t altro_batch_evaluate(altro_handle* h, int32_t ncand, const double* U, const double* X, const double* x0, double* J, double* c_max,
                             double* defect, double* Xout) {
  return evaluate_call(h, "altro_batch_evaluate", true, ncand, U, X, x0, J, c_max, defect, Xout);
}

// ---- gradient of a candidate's merit with respect to its controls and initial state (kernels in evaluate_grad.h)
// the argument rules both forms share, checked before anything else
static int evaluate_grad_rules(altro_handle* h, const char* fn, int32_t ncand, const double* U, double rho, double* J, double* P, double* gU,
                               double* gx0) {
  const std::string f(fn);
  if (!U) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": U is required");
  if (ncand < 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": ncand must be at least 1");
  if (!(rho >= 0.0) || std::isinf(rho)) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": rho must be finite and not negative");
  if (!J && !P && !gU && !gx0) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": J, P, gU and gx0 are all null");
  return ALTRO_OK;
}

// U, x0, J, P, gU, gx0, Xout: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues one
// kernel; allocates only when there is no Xout and the state workspace has to grow.
static int evaluate_grad_launch(altro_handle* h, int32_t ncand, const double* U, const double* x0, double rho, double* J, double* P, double* gU,
                                double* gx0, double* Xout) {
  if (h->wide) return fwd(h, h->wide->evaluate_grad_dev(ncand, U, x0, rho, J, P, gU, gx0, Xout));
  if (int rc = score_ready(h)) return rc;
  const size_t B = h->d.batch, N = h->d.N, n = h->d.n;
  const size_t R = B * (size_t)ncand;
  if (!Xout) HIPCHK(h, h->pool.reserve(&h->eval_ws, &h->eval_ws_elems, R * N * n));
  const altro::Eval16 p = eval16_params(h);
  const size_t rows = (R + 3) & ~(size_t)3;   // whole waves of four rows
  const altro::GradIO io{U, x0 ? x0 : h->x0, J, P, gU, gx0, Xout ? Xout : h->eval_ws, rho};
  hipLaunchKernelGGL(altro::k_eval_grad16, grid_for(rows * LW), dim3(256), 0, h->stream, io, x0 ? (int)n : LW, p, (int)ncand, R, rows);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

static int32_t evaluate_grad_call(altro_handle* h, const char* fn, bool host, int32_t ncand, const double* U, const double* x0, double rho,
                                  double* J, double* P, double* gU, double* gx0, double* Xout) {
  return twin_call(
      h, fn, host, true, [&] { return evaluate_grad_rules(h, fn, ncand, U, rho, J, P, gU, gx0); },
      [&](TwinArgs& a) { altro::stage_evaluate_grad(a, h->d.batch, h->d.N, h->d.n, h->d.m, ncand, U, x0, J, P, gU, gx0, Xout); },
      [&](const TwinArgs& a) {
        return evaluate_grad_launch(h, ncand, a.f64(altro::EG_U), a.f64(altro::EG_X0), rho, a.f64(altro::EG_J), a.f64(altro::EG_P),
                                    a.f64(altro::EG_GU), a.f64(altro::EG_GX0), a.f64(altro::EG_XOUT));
      });
}
int32_t altro_batch_evaluate_grad_dev(altro_handle* h, int32_t ncand, const double* U, const double* x0, double rho, double* J, double* P,
                                      double* gU, double* gx0, double* Xout) {
  return evaluate_grad_call(h, "altro_batch_evaluate_grad_dev", false, ncand, U, x0, rho, J, P, gU, gx0, Xout);
}
int32_t altro_batch_evaluate_grad(altro_handle* h, int32_t ncand, const double* U, const double* x0, double rho, double* J, double* P,
                                  double* gU, double* gx0, double* Xout) {
  return evaluate_grad_call(h, "altro_batch_evaluate_grad", true, ncand, U, x0, rho, J, P, gU, gx0, Xout);
}

// ---- the solver's augmented Lagrangian of a control sequence, its gradient and its data derivatives (kernels in
// evaluate_al.h).  The argument rules both forms share, checked before anything else
static int evaluate_al_rules(altro_handle* h, const char* fn, int32_t ncand, const double* U, const altro_al_out* out) {
  const std::string f(fn);
  if (!out) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": out is required");
  if (ncand < 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": ncand must be at least 1");
  if (!U && ncand != 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": the controls the handle holds (U null) are one candidate: ncand must be 1");
  if (!out->LA && !out->J && !out->gU && !out->gx0 && !out->gXref && !out->gUref && !out->gQ && !out->gQf && !out->gR && !out->gzmin &&
      !out->gzmax)
    FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": every output other than Xout is null");
  return ALTRO_OK;
}

// U, x0 and the pointers of o: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues one
// kernel (after the unpack of the held controls into the workspace when U is null); allocates only when the workspace has to grow.
static int evaluate_al_launch(altro_handle* h, int32_t ncand, const double* U, const double* x0, const altro_al_out& o) {
  if (h->wide) return fwd(h, h->wide->evaluate_al_dev(ncand, U, x0, o));
  if (int rc = score_ready(h)) return rc;
  const size_t B = h->d.batch, N = h->d.N, n = h->d.n, m = h->d.m;
  const size_t R = B * (size_t)ncand, lx = N * n, lu = (N - 1) * m;
  const size_t need = (o.Xout ? 0 : R * lx) + (U ? 0 : R * lu);
  if (need) HIPCHK(h, h->pool.reserve(&h->eval_ws, &h->eval_ws_elems, need));
  if (!U) {   // the controls held: the current plane, unpacked behind the workspace's states in the caller's layout
    double* Uw = h->eval_ws + (o.Xout ? 0 : R * lx);
    if (int rc = get_traj(h, nullptr, Uw, true)) return rc;
    U = Uw;
  }
  const altro::Eval16 p = eval16_params(h);
  const size_t rows = (R + 3) & ~(size_t)3;   // whole waves of four rows
  const altro::ALIO io{U, x0 ? x0 : h->x0, o.LA, o.J, o.gU, o.gx0, o.gXref, o.gUref, o.gQ, o.gQf, o.gR, o.gzmin, o.gzmax,
                       o.Xout ? o.Xout : h->eval_ws, h->Lb, h->Lc, h->mu, h->bslot, h->nbp, 0.5 * h->dt};
  hipLaunchKernelGGL(altro::k_eval_al16, grid_for(rows * LW), dim3(256), 0, h->stream, io, x0 ? (int)n : LW, p, (int)ncand, R, rows);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

static int32_t evaluate_al_call(altro_handle* h, const char* fn, bool host, int32_t ncand, const double* U, const double* x0,
                                const altro_al_out* out) {
  return twin_call(
      h, fn, host, true, [&] { return evaluate_al_rules(h, fn, ncand, U, out); },
      [&](TwinArgs& a) {
        double* const po[12] = {out->LA, out->J, out->gU, out->gx0, out->gXref, out->gUref, out->gQ, out->gQf, out->gR, out->gzmin, out->gzmax,
                                out->Xout};
        altro::stage_evaluate_al(a, h->d.batch, h->d.N, h->d.n, h->d.m, ncand, U, x0, po);
      },
      [&](const TwinArgs& a) {
        const altro_al_out o{a.f64(altro::AL_LA), a.f64(altro::AL_J), a.f64(altro::AL_GU), a.f64(altro::AL_GX0), a.f64(altro::AL_GXREF),
                             a.f64(altro::AL_GUREF), a.f64(altro::AL_GQ), a.f64(altro::AL_GQF), a.f64(altro::AL_GR), a.f64(altro::AL_GZMIN),
                             a.f64(altro::AL_GZMAX), a.f64(altro::AL_XOUT)};
        return evaluate_al_launch(h, ncand, a.f64(altro::AL_U), a.f64(altro::AL_X0), o);
      });
}
int32_t altro_batch_evaluate_al_dev(altro_handle* h, int32_t ncand, const double* U, const double* x0, const altro_al_out* out) {
  return evaluate_al_call(h, "altro_batch_evaluate_al_dev", false, ncand, U, x0, out);
}
int32_t altro_batch_evaluate_al(altro_handle* h, int32_t ncand, const double* U, const double* x0, const altro_al_out* out) {
  return evaluate_al_call(h, "altro_batch_evaluate_al", true, ncand, U, x0, out);
}

// the penalty of every instance: the mu altro_batch_evaluate_al uses
int32_t altro_batch_get_penalty_dev(altro_handle* h, double* mu) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_get_penalty_dev");
    DEV_ARG(h, "mu", mu, B_, double, false);
    HIPCHK(h, hipMemcpyAsync(mu, h->wide ? h->wide->mu : h->mu, B_ * sizeof(double), hipMemcpyDeviceToDevice, common(h).stream));
    return ALTRO_OK;
  });
}

int32_t altro_batch_get_penalty(altro_handle* h, double* mu) {
  return guard(h, [&]() -> int32_t {
    if (!h) return dev_null_handle("altro_batch_get_penalty");
    if (!mu) FAIL(h, ALTRO_ERR_INVALID_ARG, "altro_batch_get_penalty: null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(mu, h->wide ? h->wide->mu : h->mu, (size_t)h->d.batch * sizeof(double), hipMemcpyDeviceToHost, common(h).stream));
    HIPCHK(h, hipStreamSynchronize(common(h).stream));
    return ALTRO_OK;
  });
}

// ---- warm start from the best of several candidates (kernels in warm_start.h)
// the argument rules both forms share, checked before anything else
static int warm_start_rules(altro_handle* h, const char* fn, int32_t ncand, const double* U, double rho, int32_t include_current) {
  const std::string f(fn);
  if (!U) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": U is required");
  if (ncand < 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": ncand must be at least 1");
  if (!(rho >= 0.0) || std::isinf(rho)) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": rho must be finite and not negative");
  if (include_current != 0 && include_current != 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": include_current must be 0 or 1");
  return ALTRO_OK;
}

// U, chosen, J, c_max: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues the scoring
// kernel, then the select-and-install kernel; allocates only when J or c_max is null and the merit workspace has to grow.
static int warm_start_launch(altro_handle* h, int32_t ncand, const double* U, double rho, int32_t inc, int32_t* chosen, double* J,
                             double* c_max) {
  if (h->wide) return fwd(h, h->wide->warm_start_dev(ncand, U, rho, inc, chosen, J, c_max));
  if (int rc = score_ready(h)) return rc;
  const size_t B = h->d.batch, N = h->d.N, n = h->d.n, m = h->d.m;
  const size_t R = B * (size_t)(ncand + inc);
  if (!J || !c_max) {
    HIPCHK(h, h->pool.reserve(&h->ws_merit, &h->ws_merit_elems, 2 * R));
    if (!J) J = h->ws_merit;
    if (!c_max) c_max = h->ws_merit + R;
  }
  const altro::Eval16 p = eval16_params(h);
  const size_t plane = N * (size_t)LW;
  const size_t rows = (R + 3) & ~(size_t)3;   // whole waves of four rows
  hipLaunchKernelGGL(altro::k_ws_score16, grid_for(rows * LW), dim3(256), 0, h->stream, J, c_max, U, h->Z, h->cur, plane, h->x0, p, (int)ncand,
                     (int)inc, R, rows);
  HIPCHK(h, hipGetLastError());
  const size_t slots = ((size_t)h->Bp + 3) & ~(size_t)3;
  hipLaunchKernelGGL(altro::k_ws_install16, grid_for(slots * LW), dim3(256), 0, h->stream, chosen, J, c_max, U, h->Z, h->cur, plane, h->x0,
                     h->flags.mask(), p, (int)ncand, (int)inc, rho, (int)B, h->Bp, slots);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

static int32_t warm_start_call(altro_handle* h, const char* fn, bool host, int32_t ncand, const double* U, double rho, int32_t include_current,
                               int32_t* chosen, double* J, double* c_max) {
  return twin_call(
      h, fn, host, true, [&] { return warm_start_rules(h, fn, ncand, U, rho, include_current); },
      [&](TwinArgs& a) { altro::stage_warm_start(a, h->d.batch, h->d.N, h->d.m, ncand, include_current, U, chosen, J, c_max); },
      [&](const TwinArgs& a) {
        return warm_start_launch(h, ncand, a.f64(altro::WS_U), rho, include_current, a.i32(altro::WS_CHOSEN), a.f64(altro::WS_J),
                                 a.f64(altro::WS_CMAX));
      });
}
int32_t altro_batch_warm_start_dev(altro_handle* h, int32_t ncand, const double* U, double rho, int32_t include_current, int32_t* chosen,
                                   double* J, double* c_max) {
  return warm_start_call(h, "altro_batch_warm_start_dev", false, ncand, U, rho, include_current, chosen, J, c_max);
}
int32_t altro_batch_warm_start(altro_handle* h, int32_t ncand, const double* U, double rho, int32_t include_current, int32_t* chosen,
                               double* J, double* c_max) {
  return warm_start_call(h, "altro_batch_warm_start", true, ncand, U, rho, include_current, chosen, J, c_max);
}

// ---- closed-loop simulation of the stored policy under disturbances (kernels in simulate.h)
// the argument rules both forms share, checked before anything else
static int simulate_rules(altro_handle* h, const char* fn, int32_t nsamp, int32_t clamp, bool any_out) {
  const std::string f(fn);
  if (nsamp < 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": nsamp must be at least 1");
  if (clamp != 0 && clamp != 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": clamp must be 0 or 1");
  if (!any_out) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": J, c_max, dx_max, fb, Xout and Uout are all null");
  return ALTRO_OK;
}

// io: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues one kernel, allocates nothing.
static int simulate_launch(altro_handle* h, int32_t nsamp, int32_t clamp, const altro::SimIO& io) {
  if (h->wide) return fwd(h, h->wide->simulate_policy_dev(nsamp, clamp, io));
  if (int rc = score_ready(h)) return rc;
  const size_t R = (size_t)h->d.batch * (size_t)nsamp;
  const altro::Eval16 p = eval16_params(h);
  const size_t rows = (R + 3) & ~(size_t)3;   // whole waves of four rows
  hipLaunchKernelGGL(altro::k_sim16, grid_for(rows * LW), dim3(256), 0, h->stream, io, h->Z, h->cur, (size_t)h->d.N * LW, h->KD, h->kmu, h->x0, p,
                     (int)nsamp, clamp ? 1 : 0, R, rows);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

static int32_t simulate_call(altro_handle* h, const char* fn, bool host, int32_t nsamp, const double* x0, const double* w, int32_t clamp,
                             double* J, double* c_max, double* dx_max, int32_t* fb, double* Xout, double* Uout) {
  return twin_call(
      h, fn, host, true, [&] { return simulate_rules(h, fn, nsamp, clamp, J || c_max || dx_max || fb || Xout || Uout); },
      [&](TwinArgs& a) { altro::stage_simulate(a, h->d.batch, h->d.N, h->d.n, h->d.m, nsamp, x0, w, J, c_max, dx_max, fb, Xout, Uout); },
      [&](const TwinArgs& a) {
        const altro::SimIO io{a.f64(altro::SIM_X0), a.f64(altro::SIM_W), a.f64(altro::SIM_J), a.f64(altro::SIM_CMAX),
                              a.f64(altro::SIM_DXMAX), a.i32(altro::SIM_FB), a.f64(altro::SIM_XOUT), a.f64(altro::SIM_UOUT)};
        return simulate_launch(h, nsamp, clamp, io);
      });
}
int32_t altro_batch_simulate_policy_dev(altro_handle* h, int32_t nsamp, const double* x0, const double* w, int32_t clamp, double* J,
                                        double* c_max, double* dx_max, int32_t* fb, double* Xout, double* Uout) {
  return simulate_call(h, "altro_batch_simulate_policy_dev", false, nsamp, x0, w, clamp, J, c_max, dx_max, fb, Xout, Uout);
}
int32_t altro_batch_simulate_policy(altro_handle* h, int32_t nsamp, const double* x0, const double* w, int32_t clamp, double* J,
                                    double* c_max, double* dx_max, int32_t* fb, double* Xout, double* Uout) {
  return simulate_call(h, "altro_batch_simulate_policy", true, nsamp, x0, w, clamp, J, c_max, dx_max, fb, Xout, Uout);
}

// ---- closed-loop covariance of the stored policy (kernels in covariance.h)
// The argument rules both forms share, checked before anything else; nsc <- the doubles of sc per instance (nk * p of con_id).
// any_in: Sigma0 or W is given; any_out: one of the eight outputs is.
static int covariance_rules(altro_handle* h, const char* fn, bool any_in, bool any_out, int32_t per_instance, int32_t con_id, double kappa,
                            const double* sc, const double* zmin_t, const double* zmax_t, size_t* nsc) {
  const std::string f(fn);
  *nsc = 0;
  if (!any_in) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": Sigma0 and W are both null");
  if (!any_out) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": sx, su, sc, dJ, fb, zmin_t, zmax_t and Sout are all null");
  if (per_instance != 0 && per_instance != 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": per_instance must be 0 or 1");
  if (!(kappa >= 0.0) || std::isinf(kappa)) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": kappa must be finite and not negative");
  if ((zmin_t != nullptr) != (zmax_t != nullptr)) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": zmin_t and zmax_t go together: both or neither");
  const int box_id = common(h).box_id;
  if (zmin_t && box_id < 0) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": zmin_t / zmax_t need a BOX constraint on the handle");
  if (con_id < 0) {
    if (con_id != -1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": unknown constraint id");
    if (sc) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": sc needs the id of a LINEAR or SOC constraint (con_id = -1)");
    return ALTRO_OK;
  }
  if (con_id == box_id) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": con_id is a BOX constraint: its deviations are sx and su");
  if (h->wide) {
    if (const auto* bl = h->wide->find(con_id)) *nsc = (size_t)(bl->k1 - bl->k0 + 1) * bl->p;
  } else {
    for (const auto& cb : h->cons)
      if (cb.id == con_id) *nsc = (size_t)(cb.k1 - cb.k0 + 1) * cb.p;
  }
  if (!*nsc) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": unknown constraint id");
  if (!sc) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": con_id is given without sc");
  return ALTRO_OK;
}

// io: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues one kernel, allocates nothing:
// the covariance lives in registers (16-lane backend) or LDS (one-wave-per-instance backend).
static int covariance_launch(altro_handle* h, const altro::CovIO& io, int32_t con_id) {
  if (h->wide) return fwd(h, h->wide->propagate_covariance_dev(io, con_id));
  if (int rc = score_ready(h)) return rc;
  altro::CovRows cr{};
  for (const auto& cb : h->cons) {
    if (cb.id != con_id) continue;
    cr.p = cb.p; cr.k0 = cb.k0; cr.k1 = cb.k1;
    for (int r = 0; r < cb.p; ++r) cr.lanes |= (unsigned long long)(cb.lanes[r] & 15) << (4 * r);
  }
  const size_t B = h->d.batch;
  const size_t rows = (B + 3) & ~(size_t)3;   // whole waves of four rows
  hipLaunchKernelGGL(altro::k_cov16, grid_for(rows * LW), dim3(256), 0, h->stream, io, cr, h->KD, h->kmu, eval16_params(h), B, rows);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

static int32_t covariance_call(altro_handle* h, const char* fn, bool host, const double* Sigma0, const double* W, int32_t per_instance,
                               int32_t con_id, double kappa, double* sx, double* su, double* sc, double* dJ, int32_t* fb, double* zmin_t,
                               double* zmax_t, double* Sout) {
  size_t nsc = 0;
  return twin_call(
      h, fn, host, true,
      [&] {
        return covariance_rules(h, fn, Sigma0 || W, sx || su || sc || dJ || fb || zmin_t || zmax_t || Sout, per_instance, con_id, kappa, sc,
                                zmin_t, zmax_t, &nsc);
      },
      [&](TwinArgs& a) {
        altro::stage_covariance(a, h->d.batch, h->d.N, h->d.n, h->d.m, per_instance, nsc, Sigma0, W, sx, su, sc, dJ, fb, zmin_t, zmax_t, Sout);
      },
      [&](const TwinArgs& a) {
        const altro::CovIO io{a.f64(altro::COV_S0), a.f64(altro::COV_W), per_instance, kappa, a.f64(altro::COV_SX), a.f64(altro::COV_SU),
                              a.f64(altro::COV_SC), a.f64(altro::COV_DJ), a.i32(altro::COV_FB), a.f64(altro::COV_ZLO), a.f64(altro::COV_ZHI),
                              a.f64(altro::COV_SOUT)};
        return covariance_launch(h, io, con_id);
      });
}
int32_t altro_batch_propagate_covariance_dev(altro_handle* h, const double* Sigma0, const double* W, int32_t per_instance, int32_t con_id,
                                             double kappa, double* sx, double* su, double* sc, double* dJ, int32_t* fb, double* zmin_t,
                                             double* zmax_t, double* Sout) {
  return covariance_call(h, "altro_batch_propagate_covariance_dev", false, Sigma0, W, per_instance, con_id, kappa, sx, su, sc, dJ, fb, zmin_t,
                         zmax_t, Sout);
}
int32_t altro_batch_propagate_covariance(altro_handle* h, const double* Sigma0, const double* W, int32_t per_instance, int32_t con_id,
                                         double kappa, double* sx, double* su, double* sc, double* dJ, int32_t* fb, double* zmin_t,
                                         double* zmax_t, double* Sout) {
  return covariance_call(h, "altro_batch_propagate_covariance", true, Sigma0, W, per_instance, con_id, kappa, sx, su, sc, dJ, fb, zmin_t,
                         zmax_t, Sout);
}

// ---- sensitivity of the solution through the stored gains (kernels in sensitivity.h)
// The argument rules the VJP and the JVP share with their twins, checked before anything else.  io: the call's arrays as the
// kernels name them (VJP: inx = gX, inu = gU, o0 = gx0, ox = gXref, ou = gUref; JVP: inx = vXref, inu = vUref, in0 = vx0,
// ox = dX, ou = dU).
static int sens_rules(altro_handle* h, const char* fn, int32_t nseed, const altro::SensIO& io, bool have_out) {
  const std::string f(fn);
  if (nseed < 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": nseed must be at least 1");
  if (io.jvp) {
    if (!io.in0 && !io.inx && !io.inu) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": vx0, vXref and vUref are all null");
    if (!io.ox && !io.ou) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": dX and dU are both null");
  } else {
    if (!io.inx && !io.inu) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": gX and gU are both null");
    if (!have_out) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": out is required");
    if (!io.o0 && !io.ox && !io.ou) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": gx0, gXref and gUref are all null");
  }
  if (h->wide && h->d.m > 16 && io.bwd && io.fwd)   // (what needs d_k: a seed AND an output of the forward sweep)
    FAIL(h, ALTRO_ERR_UNSUPPORTED, f + ": the one-wave-per-instance kernels keep no factors of Quu for m > 16: only the x0-only sensitivities "
                                       "(gx0 alone, vx0 alone) are available");
  return ALTRO_OK;
}
// which sweeps a call needs: the backward one when there is a seed, the forward one when xi or nu is asked for
static altro::SensIO sens_io(bool jvp, const double* inx, const double* inu, const double* in0, double* o0, double* ox, double* ou, int32_t* fb) {
  altro::SensIO io{inx, inu, in0, o0, ox, ou, nullptr, fb, jvp ? 1 : 0, 0, 0};
  io.bwd = (inx || inu) ? 1 : 0;
  io.fwd = (ox || ou) ? 1 : 0;
  return io;
}

// io: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues one kernel; allocates only
// when both sweeps run and the workspace that carries d_k between them has to grow.
static int sens_launch(altro_handle* h, int32_t nseed, altro::SensIO io) {
  if (h->wide) return fwd(h, h->wide->solution_sens_dev(nseed, io));
  if (int rc = score_ready(h)) return rc;
  const size_t B = h->d.batch, N = h->d.N, m = h->d.m;
  const size_t R = B * (size_t)nseed;
  if (io.bwd && io.fwd) {
    HIPCHK(h, h->pool.reserve(&h->eval_ws, &h->eval_ws_elems, R * (N - 1) * m));
    io.dws = h->eval_ws;
  }
  const size_t rows = (R + 3) & ~(size_t)3;   // whole waves of four rows
  hipLaunchKernelGGL(altro::k_sens16, grid_for(rows * LW), dim3(256), 0, h->stream, io, h->KD, h->kmu, eval16_params(h), (int)nseed, R, rows);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

// io: the caller's arrays in the kernels' order (sens_io), which is the order of the table
static int32_t sens_call(altro_handle* h, const char* fn, bool host, int32_t nseed, const altro::SensIO& io, bool have_out) {
  return twin_call(
      h, fn, host, true, [&] { return sens_rules(h, fn, nseed, io, have_out); },
      [&](TwinArgs& a) {
        altro::stage_solution_sens(a, h->d.batch, h->d.N, h->d.n, h->d.m, nseed, io.jvp != 0, io.inx, io.inu, io.in0, io.o0, io.ox, io.ou, io.fb);
      },
      [&](const TwinArgs& a) {
        return sens_launch(h, nseed, sens_io(io.jvp != 0, a.f64(altro::SS_INX), a.f64(altro::SS_INU), a.f64(altro::SS_IN0), a.f64(altro::SS_O0),
                                             a.f64(altro::SS_OX), a.f64(altro::SS_OU), a.i32(altro::SS_FB)));
      });
}
static altro::SensIO vjp_io(const double* gX, const double* gU, const altro_sens_out* out, int32_t* fb) {
  return sens_io(false, gX, gU, nullptr, out ? out->gx0 : nullptr, out ? out->gXref : nullptr, out ? out->gUref : nullptr, fb);
}
int32_t altro_batch_solution_vjp_dev(altro_handle* h, int32_t nseed, const double* gX, const double* gU, const altro_sens_out* out, int32_t* fb) {
  return sens_call(h, "altro_batch_solution_vjp_dev", false, nseed, vjp_io(gX, gU, out, fb), out != nullptr);
}
int32_t altro_batch_solution_vjp(altro_handle* h, int32_t nseed, const double* gX, const double* gU, const altro_sens_out* out, int32_t* fb) {
  return sens_call(h, "altro_batch_solution_vjp", true, nseed, vjp_io(gX, gU, out, fb), out != nullptr);
}
int32_t altro_batch_solution_jvp_dev(altro_handle* h, int32_t nseed, const double* vx0, const double* vXref, const double* vUref, double* dX,
                                     double* dU, int32_t* fb) {
  return sens_call(h, "altro_batch_solution_jvp_dev", false, nseed, sens_io(true, vXref, vUref, vx0, nullptr, dX, dU, fb), true);
}
int32_t altro_batch_solution_jvp(altro_handle* h, int32_t nseed, const double* vx0, const double* vXref, const double* vUref, double* dX,
                                 double* dU, int32_t* fb) {
  return sens_call(h, "altro_batch_solution_jvp", true, nseed, sens_io(true, vXref, vUref, vx0, nullptr, dX, dU, fb), true);
}

// altro_batch_get_gain_factors on the device: the unpack that call does in a loop on the host (k_unpack_factors16), resp. the
// unpack of the packed triangles of the one-wave-per-instance kernels
int32_t altro_batch_get_gain_factors_dev(altro_handle* h, double* F) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_get_gain_factors_dev");
    DEV_ARG(h, "F", F, B_ * (N_ - 1) * m_ * m_, double, false);
    WIDE_FWD(h, get_gain_factors_dev(F));
    hipLaunchKernelGGL(altro::k_unpack_factors16, grid_for(B_ * (N_ - 1) * m_ * m_), dim3(256), 0, h->stream, F, h->KD, (int)B_, (int)N_, (int)n_,
                       (int)m_);
    HIPCHK(h, hipGetLastError());
    return ALTRO_OK;
  });
}

// ---- sensitivity of the solution with respect to cost weights, box bounds and dynamics; the active set of the stored pass
// (kernels in sensitivity_data.h).  What the active-set outputs (gzmin, gzmax, gA, gB, gf) and the getter need: a
// box-only problem, and on the 16-lane backend a horizon the exact sets cover.
static int active_set_rules(altro_handle* h, const std::string& f) {
  const bool rows = h->wide ? h->wide->Pn > 0 : h->ncrows > 0;
  if (rows)
    FAIL(h, ALTRO_ERR_UNSUPPORTED, f + ": the active set of the stored pass is kept for box-only problems: with LINEAR or SOC rows the Hessian "
                                       "inside it is not diagonal (gQ, gQf, gR are available)");
  if (!h->wide && h->d.N > altro::ASET_MAXN)
    FAIL(h, ALTRO_ERR_UNSUPPORTED, f + ": the 16-lane kernels keep the exact active set for N <= 128 (gQ, gQf, gR are available)");
  return ALTRO_OK;
}
// the argument rules both forms share, checked before anything else
static int sens_data_rules(altro_handle* h, const char* fn, int32_t nseed, const double* gX, const double* gU, int32_t per_knot,
                           const altro_sens_data_out* out) {
  const std::string f(fn);
  if (nseed < 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": nseed must be at least 1");
  if (!gX && !gU) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": gX and gU are both null");
  if (!out) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": out is required");
  const bool want_set = out->gzmin || out->gzmax || out->gA || out->gB || out->gf;
  if (!want_set && !out->gQ && !out->gQf && !out->gR) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": every member of out is null");
  if (per_knot != 0 && per_knot != 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": per_knot must be 0 or 1");
  if (h->wide && h->d.m > 16)
    FAIL(h, ALTRO_ERR_UNSUPPORTED, f + ": the one-wave-per-instance kernels keep no factors of Quu for m > 16: no data sensitivity is available");
  if (want_set)
    if (int rc = active_set_rules(h, f)) return rc;
  return ALTRO_OK;
}

// io: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues one kernel; allocates only when
// the workspace that carries d_k and dz_k between the sweeps has to grow.
static int sens_data_launch(altro_handle* h, int32_t nseed, altro::SensDataIO io) {
  if (h->wide) return fwd(h, h->wide->solution_vjp_data_dev(nseed, io));
  if (int rc = score_ready(h)) return rc;
  const size_t B = h->d.batch, N = h->d.N, n = h->d.n, m = h->d.m;
  const size_t R = B * (size_t)nseed, ld = (N - 1) * m, lz = N * (n + m);
  const bool want3 = io.gA || io.gB || io.gf;
  HIPCHK(h, h->pool.reserve(&h->eval_ws, &h->eval_ws_elems, R * (ld + (want3 ? lz : 0))));
  io.dws = h->eval_ws;
  io.zws = want3 ? h->eval_ws + R * ld : nullptr;
  io.Lb = h->Lb; io.mu = h->mu; io.bslot = h->bslot; io.nbp = h->nbp; io.dt = h->dt;
  const size_t rows = (R + 3) & ~(size_t)3;   // whole waves of four rows
  hipLaunchKernelGGL(altro::k_sens_data16, grid_for(rows * LW), dim3(256), 0, h->stream, io, h->Z, h->cur, N * (size_t)LW, h->KD, h->kmu,
                     h->ahash, eval16_params(h), (int)nseed, R, rows);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

static int32_t sens_data_call(altro_handle* h, const char* fn, bool host, int32_t nseed, const double* gX, const double* gU, int32_t per_knot,
                              const altro_sens_data_out* out, int32_t* fb) {
  return twin_call(
      h, fn, host, true, [&] { return sens_data_rules(h, fn, nseed, gX, gU, per_knot, out); },
      [&](TwinArgs& a) {
        double* const po[8] = {out->gQ, out->gQf, out->gR, out->gzmin, out->gzmax, out->gA, out->gB, out->gf};
        altro::stage_solution_vjp_data(a, h->d.batch, h->d.N, h->d.n, h->d.m, nseed, per_knot, gX, gU, po, fb);
      },
      [&](const TwinArgs& a) {
        altro::SensDataIO io{};
        io.gX = a.f64(altro::SD_GX); io.gU = a.f64(altro::SD_GU);
        io.gQ = a.f64(altro::SD_GQ); io.gQf = a.f64(altro::SD_GQF); io.gR = a.f64(altro::SD_GR);
        io.gzmin = a.f64(altro::SD_GZMIN); io.gzmax = a.f64(altro::SD_GZMAX);
        io.gA = a.f64(altro::SD_GA); io.gB = a.f64(altro::SD_GB); io.gf = a.f64(altro::SD_GF);
        io.fb = a.i32(altro::SD_FB);
        io.per_knot = per_knot;
        return sens_data_launch(h, nseed, io);
      });
}
int32_t altro_batch_solution_vjp_data_dev(altro_handle* h, int32_t nseed, const double* gX, const double* gU, int32_t per_knot,
                                          const altro_sens_data_out* out, int32_t* fb) {
  return sens_data_call(h, "altro_batch_solution_vjp_data_dev", false, nseed, gX, gU, per_knot, out, fb);
}
int32_t altro_batch_solution_vjp_data(altro_handle* h, int32_t nseed, const double* gX, const double* gU, int32_t per_knot,
                                      const altro_sens_data_out* out, int32_t* fb) {
  return sens_data_call(h, "altro_batch_solution_vjp_data", true, nseed, gX, gU, per_knot, out, fb);
}

// codes, mu_pass, fb: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues one kernel.
static int gain_active_set_launch(altro_handle* h, uint8_t* codes, double* mu_pass, int32_t* fb) {
  if (h->wide) return fwd(h, h->wide->get_gain_active_set_dev(codes, mu_pass, fb));
  const size_t B = h->d.batch, N = h->d.N, n = h->d.n, m = h->d.m;
  hipLaunchKernelGGL(altro::k_gain_aset16, grid_for(B * N * (n + m)), dim3(256), 0, h->stream, codes, mu_pass, fb, h->ahash, h->kmu, h->mu, (int)B,
                     (int)N, (int)n, (int)m);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}
static int32_t gain_active_set_call(altro_handle* h, const char* fn, bool host, uint8_t* codes, double* mu_pass, int32_t* fb) {
  return twin_call(
      h, fn, host, true,
      [&]() -> int {
        if (!codes && !mu_pass) FAIL(h, ALTRO_ERR_INVALID_ARG, std::string(fn) + ": codes and mu_pass are both null");
        return active_set_rules(h, fn);
      },
      [&](TwinArgs& a) { altro::stage_gain_active_set(a, h->d.batch, h->d.N, h->d.n, h->d.m, codes, mu_pass, fb); },
      [&](const TwinArgs& a) -> int {
        if (!host)
          if (int rc = h->wide ? fwd(h, h->wide->eval_ready()) : score_ready(h)) return rc;
        return gain_active_set_launch(h, a.u8(altro::GA_CODES), a.f64(altro::GA_MU), a.i32(altro::GA_FB));
      });
}
int32_t altro_batch_get_gain_active_set_dev(altro_handle* h, uint8_t* codes, double* mu_pass, int32_t* fb) {
  return gain_active_set_call(h, "altro_batch_get_gain_active_set_dev", false, codes, mu_pass, fb);
}
int32_t altro_batch_get_gain_active_set(altro_handle* h, uint8_t* codes, double* mu_pass, int32_t* fb) {
  return gain_active_set_call(h, "altro_batch_get_gain_active_set", true, codes, mu_pass, fb);
}

// ---- the quadratic cost-to-go of the stored policy (kernels in cost_to_go.h)
// io: device arrays (the caller's, validated; or the staged copies of the host twin).  Enqueues one kernel, allocates nothing:
// P lives in registers (16-lane backend) or LDS (one-wave-per-instance backend).
static int cost_to_go_launch(altro_handle* h, altro::CtgIO io) {
  if (h->wide) return fwd(h, h->wide->cost_to_go_dev(io));
  if (int rc = score_ready(h)) return rc;
  io.Lb = h->Lb; io.mu = h->mu; io.bslot = h->bslot; io.nbp = h->nbp;
  const size_t B = h->d.batch;
  const size_t rows = (B + 3) & ~(size_t)3;   // whole waves of four rows
  hipLaunchKernelGGL(altro::k_ctg16, grid_for(rows * LW), dim3(256), 0, h->stream, io, h->Z, h->cur, (size_t)h->d.N * LW, h->KD, h->kmu, h->ahash,
                     eval16_params(h), B, rows);
  HIPCHK(h, hipGetLastError());
  return ALTRO_OK;
}

static int32_t cost_to_go_call(altro_handle* h, const char* fn, bool host, int32_t mode, const altro_ctg_out* out, int32_t* fb) {
  return twin_call(
      h, fn, host, true,
      [&]() -> int {
        const std::string f(fn);
        if (!out) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": out is required");
        if (!out->P0 && !out->p0 && !out->v0 && !out->P && !out->p && !out->v) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": every member of out is null");
        if (mode != 0 && mode != 1) FAIL(h, ALTRO_ERR_INVALID_ARG, f + ": mode must be 0 or 1");
        return mode ? active_set_rules(h, f) : ALTRO_OK;
      },
      [&](TwinArgs& a) {
        double* const po[6] = {out->P0, out->p0, out->v0, out->P, out->p, out->v};
        altro::stage_cost_to_go(a, h->d.batch, h->d.N, h->d.n, po, fb);
      },
      [&](const TwinArgs& a) {
        altro::CtgIO io{};
        io.P0 = a.f64(altro::CTG_P0); io.p0 = a.f64(altro::CTG_SP0); io.v0 = a.f64(altro::CTG_V0);
        io.P = a.f64(altro::CTG_P); io.p = a.f64(altro::CTG_SP); io.v = a.f64(altro::CTG_V);
        io.fb = a.i32(altro::CTG_FB);
        io.mode = mode;
        return cost_to_go_launch(h, io);
      });
}
int32_t altro_batch_cost_to_go_dev(altro_handle* h, int32_t mode, const altro_ctg_out* out, int32_t* fb) {
  return cost_to_go_call(h, "altro_batch_cost_to_go_dev", false, mode, out, fb);
}
int32_t altro_batch_cost_to_go(altro_handle* h, int32_t mode, const altro_ctg_out* out, int32_t* fb) {
  return cost_to_go_call(h, "altro_batch_cost_to_go", true, mode, out, fb);
}

// ---- per-instance active mask and cold restart
static int set_active_common(altro_handle* h, const int32_t* active, bool dev) {
  altro::InstanceFlags& fl = common(h).flags;
  const hipStream_t st = common(h).stream;
  if (!active) { fl.on = false; return ALTRO_OK; }
  HIPCHK(h, fl.load(false, active, dev, h->d.batch, common(h).slots, st));
  if (!dev) HIPCHK(h, hipStreamSynchronize(st));
  fl.on = true;
  return ALTRO_OK;
}

int32_t altro_batch_set_active(altro_handle* h, const int32_t* active) {
  return guard(h, [&]() -> int32_t {
    if (!h) return dev_null_handle("altro_batch_set_active");
    HIPCHK(h, hipSetDevice(h->device));
    return set_active_common(h, active, false);
  });
}

int32_t altro_batch_set_active_dev(altro_handle* h, const int32_t* active) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_set_active_dev");
    DEV_ARG(h, "active", active, B_, int32_t, true);
    return set_active_common(h, active, true);
  });
}

int32_t altro_batch_get_active(altro_handle* h, int32_t* active) {
  return guard(h, [&]() -> int32_t {
    if (!h) return dev_null_handle("altro_batch_get_active");
    if (!active) FAIL(h, ALTRO_ERR_INVALID_ARG, "altro_batch_get_active: null pointer");
    const altro::InstanceFlags& fl = common(h).flags;
    const size_t B = h->d.batch;
    if (!fl.on) { for (size_t i = 0; i < B; ++i) active[i] = 1; return ALTRO_OK; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(common(h).stream));
    HIPCHK(h, hipMemcpy(active, fl.active, B * sizeof(int), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  });
}

// X, U: host arrays (staged) or validated device arrays (read where they are); `which` likewise, through InstanceFlags
static int restart_16(altro_handle* h, const int32_t* which, const double* X, const double* U, bool dev) {
  const size_t B = h->d.batch, N = h->d.N, n = h->d.n, m = h->d.m;
  const size_t cx = X ? B * N * n : 0, cu = B * (N - 1) * m;
  if (!dev) {
    int rc = h->ensure_stage((cx + cu) * sizeof(double));
    if (rc) return rc;
    if (X && (rc = upload(h, X, cx, 0))) return rc;
    if ((rc = upload(h, U, cu, cx))) return rc;
    X = X ? h->stage : nullptr;
    U = h->stage + cx;
  }
  HIPCHK(h, h->flags.load(true, which, dev, (int)B, h->Bp, h->stream));
  hipLaunchKernelGGL(k_restart, grid_for(B * LW), dim3(256), 0, h->stream, h->flags.which, X, U, h->Z, h->cur, N * (size_t)LW, h->Lb,
                     h->nbp, h->Lc, h->mu, h->kmu, h->ahash, h->dzero, h->iters, h->iters_outer, h->status, h->cost, h->cmax,
                     h->Jtrace, h->ctrace, h->atrace, h->clock.on ? h->clock.window : nullptr, (int)B, (int)N, (int)n, (int)m, X ? 1 : 0);
  HIPCHK(h, hipGetLastError());
  if (!dev) HIPCHK(h, hipStreamSynchronize(h->stream));
  return ALTRO_OK;
}

int32_t altro_batch_restart_instances(altro_handle* h, const int32_t* which, const double* X, const double* U) {
  return guard(h, [&]() -> int32_t {
    if (!h) return dev_null_handle("altro_batch_restart_instances");
    if (!which || !U) FAIL(h, ALTRO_ERR_INVALID_ARG, "altro_batch_restart_instances: which and U are required");
    HIPCHK(h, hipSetDevice(h->device));
    WIDE_FWD(h, restart(which, X, U, false));
    return restart_16(h, which, X, U, false);
  });
}

int32_t altro_batch_restart_instances_dev(altro_handle* h, const int32_t* which, const double* X, const double* U) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_restart_instances_dev");
    DEV_ARG(h, "which", which, B_, int32_t, false);
    DEV_ARG(h, "X", X, B_ * N_ * n_, double, true);
    DEV_ARG(h, "U", U, B_ * (N_ - 1) * m_, double, false);
    WIDE_FWD(h, restart(which, X, U, true));
    return restart_16(h, which, X, U, true);
  });
}

// ---- per-instance episode clock
static int set_clock_common(altro_handle* h, const int32_t* start, const int32_t* length, bool dev) {
  altro::EpisodeClock& ck = common(h).clock;
  const hipStream_t st = common(h).stream;
  int& kref = common(h).kref;
  const size_t B = h->d.batch;
  if (!start) {   // clear: the handle goes back to ONE window, which must be the one every instance holds
    if (!ck.on) return ALTRO_OK;
    std::vector<int> w(B);
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipMemcpy(w.data(), ck.window, B * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t i = 1; i < B; ++i)
      if (w[i] != w[0]) FAIL(h, ALTRO_ERR_STATE, "altro_mpc_set_clock: the instances hold different reference windows, the clock cannot be cleared");
    kref = w[0];
    ck.on = false;
    return ALTRO_OK;
  }
  if (common(h).Nt < 1 || !common(h).have_ref)
    FAIL(h, ALTRO_ERR_STATE, "altro_mpc_set_clock: no track (altro_mpc_set_track)");
  HIPCHK(h, ck.load(start, length, dev, (int)B, common(h).slots, kref, st));
  if (!dev) HIPCHK(h, hipStreamSynchronize(st));
  ck.on = true;
  return ALTRO_OK;
}

int32_t altro_mpc_set_clock(altro_handle* h, const int32_t* start, const int32_t* length) {
  return guard(h, [&]() -> int32_t {
    if (!h) return dev_null_handle("altro_mpc_set_clock");
    HIPCHK(h, hipSetDevice(h->device));
    return set_clock_common(h, start, length, false);
  });
}

int32_t altro_mpc_set_clock_dev(altro_handle* h, const int32_t* start, const int32_t* length) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_mpc_set_clock_dev");
    DEV_ARG(h, "start", start, B_, int32_t, true);
    DEV_ARG(h, "length", length, B_, int32_t, true);
    return set_clock_common(h, start, length, true);
  });
}

int32_t altro_mpc_get_clock(altro_handle* h, int32_t* start, int32_t* length, int32_t* window) {
  return guard(h, [&]() -> int32_t {
    if (!h) return dev_null_handle("altro_mpc_get_clock");
    if (!start && !length && !window) FAIL(h, ALTRO_ERR_INVALID_ARG, "altro_mpc_get_clock: every output pointer is null");
    const altro::EpisodeClock& ck = common(h).clock;
    const size_t B = h->d.batch;
    if (!ck.on) {
      const int kref = common(h).kref;
      for (size_t i = 0; i < B; ++i) {
        if (start) start[i] = 0;
        if (length) length[i] = -1;
        if (window) window[i] = kref;
      }
      return ALTRO_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(common(h).stream));
    if (start) HIPCHK(h, hipMemcpy(start, ck.start, B * sizeof(int), hipMemcpyDeviceToHost));
    if (length) HIPCHK(h, hipMemcpy(length, ck.length, B * sizeof(int), hipMemcpyDeviceToHost));
    if (window) HIPCHK(h, hipMemcpy(window, ck.window, B * sizeof(int), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  });
}

int32_t altro_batch_wait_stream(altro_handle* h, void* producer) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_wait_stream");
    HIPCHK(h, h->link.wait(common(h).stream, (hipStream_t)producer));
    return ALTRO_OK;
  });
}

int32_t altro_batch_signal_stream(altro_handle* h, void* consumer) {
  return guard(h, [&]() -> int32_t {
    DEV_ENTER(h, "altro_batch_signal_stream");
    HIPCHK(h, h->link.signal(common(h).stream, (hipStream_t)consumer));
    return ALTRO_OK;
  });
}
#undef DEV_ENTER
#undef DEV_ARG

int32_t altro_batch_get_stream(altro_handle* h, void** stream) {
  return guard(h, [&]() -> int32_t {
    if (h && h->wide && stream) { *stream = (void*)h->wide->stream; return ALTRO_OK; }
    if (!h || !stream) return ALTRO_ERR_INVALID_ARG;
    *stream = (void*)h->stream;
    return ALTRO_OK;
  });
}

}  // extern "C"
