// backend_common.h -- what the two backends behind the C-ABI hold and do alike, declared and written once.
// altro_handle (altro_batch.hip: the 16-lane backend) and altro_wide::WideBackend (wide_backend.h) both derive from
// BackendCommon, so `h->iters` and `iters` in the kernel argument lists read as members of either.  No virtual functions:
// what differs between the backends is three numbers set once at create (slots, mlog_rec, noise_len), everything else
// here is the same code for both.  The C-ABI entry points check their arguments, then call these methods on
// common(h) (altro_batch.hip); nothing here looks at a caller's pointer for null.  Host logic only.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/altro_batch.h"
#include "device_io.h"
#include "device_pool.h"
#include "launch_ring.h"
#include "mpc_log.h"
#include "pn_core.h"

namespace altro {

#define BCHK(call)                                                    \
  do {                                                                \
    hipError_t e_ = (call);                                           \
    if (e_ != hipSuccess) {                                           \
      err = std::string(#call) + ": " + hipGetErrorString(e_);        \
      return ALTRO_ERR_HIP;                                           \
    }                                                                 \
  } while (0)
#define BFAIL(code, msg) \
  do {                   \
    err = (msg);         \
    return (code);       \
  } while (0)

struct BackendCommon {
  altro_dims d{};
  altro_opts o{};
  int device = 0;
  std::string err;
  DevicePool pool;   // owns every device array of the backend (device_pool.h); the members stay plain pointers
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the last solve launch (altro_batch_last_solve_ms)
  bool timed = false;
  LaunchRing ring;        // start/end event pairs of the most recent solve launches
  InstanceFlags flags;    // active mask and restart selection, [slots] (device_io.h)
  EpisodeClock clock;     // per-instance episode clock, [slots] (device_io.h)
  // the three facts that differ between the backends, set once at create
  int slots = 0;          // entries of the per-instance arrays: the batch padded to whole waves (16-lane), or the batch (wide)
  size_t mlog_rec = 0;    // doubles of one log record (mpc_log.h): 16 + MLOG_TAIL, or n + m + MLOG_TAIL
  int noise_len = 0;      // entries of noise_w / noise_grp: 16, or kMaxN
  double* stage = nullptr;     // device staging buffer of the host entry points (grow-only)
  size_t stage_bytes = 0;
  double* eval_ws = nullptr;   // altro_batch_evaluate(_dev): states of a rollout without Xout, or the gathered own trajectory (grow-only)
  size_t eval_ws_elems = 0;
  double* ws_merit = nullptr;  // altro_batch_warm_start(_dev): J, c_max [batch * (ncand + 1)] each when the caller passes none (grow-only)
  size_t ws_merit_elems = 0;
  // per-instance results of the last launch, [slots] (the traces: [slots][ALTRO_TRACE_LEN])
  int *iters = nullptr, *iters_outer = nullptr, *status = nullptr;
  double *cost = nullptr, *cmax = nullptr, *Jtrace = nullptr, *ctrace = nullptr, *atrace = nullptr;
  // work counters, [slots], accumulating until altro_batch_timing_reset (n_reuse: iterations that reused stored gains)
  long long *n_backward = nullptr, *n_rollout = nullptr, *n_trials = nullptr, *n_solves = nullptr, *n_iters = nullptr,
            *n_ok = nullptr, *n_gconf = nullptr, *n_reuse = nullptr;
  // projected-Newton polish (pn_core.h): per-instance results, and the workspace allocated by the first solve that asks
  altro_pn::PnOut pn_out;
  altro_pn::PnWork pn_ws;
  unsigned long long* refusals = nullptr;   // device counter: rows altro_batch_set_bounds_dev refused since create
  double *noise = nullptr, *noise_w = nullptr;
  int* noise_grp = nullptr;
  int noise_mode = 0, noise_steps = 0, mpc_shift = 1;
  double* mlog = nullptr;  // per-step log of the MPC loop (mpc_log.h): [mlog_cap][batch][mlog_rec]; null: off
  int mlog_cap = 0;        // steps it holds
  int Nt = 0;              // knots of the stored reference
  int kref = 0;            // current reference window start
  int box_k0 = 0, box_k1 = -1, box_id = -1;
  bool have_dyn = false, have_cost = false, have_ref = false, dyn_per_instance = false;

  int ensure_stage(size_t bytes) {
    BCHK(pool.reserve(reinterpret_cast<char**>(&stage), &stage_bytes, bytes));
    return ALTRO_OK;
  }
  // the device is current and the stream has drained: how every blocking read below starts
  int synchronize() {
    BCHK(hipSetDevice(device));
    BCHK(hipStreamSynchronize(stream));
    return ALTRO_OK;
  }
  int check_ready() {
    if (!have_dyn) BFAIL(ALTRO_ERR_STATE, "altro_batch_set_dynamics has not been called");
    if (!have_cost) BFAIL(ALTRO_ERR_STATE, "altro_batch_set_tracking_cost has not been called");
    if (!have_ref) BFAIL(ALTRO_ERR_STATE, "no reference trajectory (altro_batch_set_reference / altro_mpc_set_track)");
    return ALTRO_OK;
  }

  int get_stats(int32_t* it, int32_t* ito, int32_t* st, double* J, double* c, double* Jt, double* ct) {
    if (int rc = synchronize()) return rc;
    const size_t B = d.batch;
    if (it) BCHK(hipMemcpy(it, iters, B * sizeof(int), hipMemcpyDeviceToHost));
    if (ito) BCHK(hipMemcpy(ito, iters_outer, B * sizeof(int), hipMemcpyDeviceToHost));
    if (st) BCHK(hipMemcpy(st, status, B * sizeof(int), hipMemcpyDeviceToHost));
    if (J) BCHK(hipMemcpy(J, cost, B * sizeof(double), hipMemcpyDeviceToHost));
    if (c) BCHK(hipMemcpy(c, cmax, B * sizeof(double), hipMemcpyDeviceToHost));
    if (Jt) BCHK(hipMemcpy(Jt, Jtrace, B * ALTRO_TRACE_LEN * sizeof(double), hipMemcpyDeviceToHost));
    if (ct) BCHK(hipMemcpy(ct, ctrace, B * ALTRO_TRACE_LEN * sizeof(double), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }
  int get_alpha_trace(double* a) {
    if (int rc = synchronize()) return rc;
    BCHK(hipMemcpy(a, atrace, (size_t)d.batch * ALTRO_TRACE_LEN * sizeof(double), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }
  // three counter arrays (or fewer: a null destination is skipped) -> the caller's, `batch` entries each
  int counters(long long* const src[3], int64_t* a, int64_t* b, int64_t* c) {
    if (int rc = synchronize()) return rc;
    int64_t* dst[3] = {a, b, c};
    for (int i = 0; i < 3; ++i)
      if (dst[i]) BCHK(hipMemcpy(dst[i], src[i], (size_t)d.batch * sizeof(long long), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }
  int get_dev_refusals(int64_t* rows) {
    if (int rc = synchronize()) return rc;
    unsigned long long v = 0;
    BCHK(hipMemcpy(&v, refusals, sizeof(v), hipMemcpyDeviceToHost));
    *rows = (int64_t)v;
    return ALTRO_OK;
  }
  // Both polish getters (pn_core.h PnOut::read): zeros while projected_newton is off, or before the backend has allocated the
  // arrays.  reset_off: asked for the statistics while the option is off, the arrays themselves go back to zero -- an instance
  // that a mask keeps out of the first polish after the option is switched on reports them.
  int read_polish(bool reset_off, int32_t* ran, int32_t* failed, double* res, double* dres0, double* dres, int32_t* dfail) {
    BCHK(hipSetDevice(device));
    const bool on = o.projected_newton != 0;
    if (reset_off && !on) {
      BCHK(hipMemsetAsync(pn_out.ran, 0, slots * sizeof(int), stream));
      BCHK(hipMemsetAsync(pn_out.failed, 0, slots * sizeof(int), stream));
      BCHK(hipMemsetAsync(pn_out.res, 0, slots * sizeof(double), stream));
    }
    BCHK(pn_out.read(stream, on && pn_out.ran, (size_t)d.batch, ran, failed, res, dres0, dres, dfail));
    return ALTRO_OK;
  }

  int last_solve_ms(float* ms) {
    if (!timed) BFAIL(ALTRO_ERR_STATE, "no solve has been launched");
    BCHK(hipSetDevice(device));
    BCHK(hipEventSynchronize(ev1));
    BCHK(hipEventElapsedTime(ms, ev0, ev1));
    return ALTRO_OK;
  }
  // the launch history and every work counter back to zero (both backends keep the same eight)
  int timing_reset() {
    if (int rc = synchronize()) return rc;
    ring.reset();
    for (long long* p : {n_backward, n_rollout, n_trials, n_solves, n_iters, n_ok, n_gconf, n_reuse})
      BCHK(hipMemsetAsync(p, 0, slots * sizeof(long long), stream));
    BCHK(hipStreamSynchronize(stream));
    return ALTRO_OK;
  }
  int timing_get(float* ms, int capacity, int* count) {
    if (int rc = synchronize()) return rc;
    const int nl = (int)ring.readable();
    if (count) *count = nl;
    for (int i = 0; ms && i < nl && i < capacity; ++i) BCHK(ring.elapsed((size_t)i, &ms[i]));
    return ALTRO_OK;
  }

  int set_noise(const double* nzv, int steps) {
    BCHK(hipSetDevice(device));
    const size_t cnt = (size_t)steps * d.batch * d.n;
    BCHK(pool.alloc(&noise, cnt, stream, false));
    BCHK(hipMemcpy(noise, nzv, cnt * sizeof(double), hipMemcpyHostToDevice));
    noise_steps = steps;
    return ALTRO_OK;
  }
  // w [n], g [n] or null (every element in group 0): the caller has checked mode and the groups
  int set_noise_model(int mode, const double* w, const int32_t* g) {
    BCHK(hipSetDevice(device));
    std::vector<double> wv(noise_len, 0.0);
    std::vector<int> gv(noise_len, 0);
    for (int i = 0; i < d.n; ++i) {
      wv[i] = w[i];
      gv[i] = g ? g[i] : 0;
    }
    BCHK(hipMemcpyAsync(noise_w, wv.data(), noise_len * sizeof(double), hipMemcpyHostToDevice, stream));
    BCHK(hipMemcpyAsync(noise_grp, gv.data(), noise_len * sizeof(int), hipMemcpyHostToDevice, stream));
    BCHK(hipStreamSynchronize(stream));
    noise_mode = mode;
    return ALTRO_OK;
  }
  // per-step log of the MPC loop (include/altro_batch.h: altro_mpc_set_log / altro_mpc_get_log)
  int set_log(int capacity_steps) {
    if (int rc = synchronize()) return rc;  // a launch in flight may still be writing the old log
    mlog_cap = 0;
    BCHK(pool.release(&mlog));
    if (capacity_steps == 0) return ALTRO_OK;
    const size_t elems = (size_t)capacity_steps * (size_t)d.batch * mlog_rec;
    BCHK(pool.alloc(&mlog, elems, stream, false));
    BCHK(hipMemsetAsync(mlog, 0xFF, elems * sizeof(double), stream));  // never written: -1 / NaN
    mlog_cap = capacity_steps;
    return ALTRO_OK;
  }
  int get_log(int first_step, int nsteps, double* x0h, double* u0h, int32_t* it, int32_t* ito, int32_t* st, double* J, double* c) {
    if (!mlog) BFAIL(ALTRO_ERR_STATE, "no log: altro_mpc_set_log has not been called");
    if (first_step < 0 || nsteps < 0 || first_step > mlog_cap - nsteps) BFAIL(ALTRO_ERR_INVALID_ARG, "steps outside the capacity of the log");
    if (int rc = synchronize()) return rc;
    const size_t B = d.batch;
    std::vector<double> img((size_t)nsteps * B * mlog_rec);
    if (!img.empty()) BCHK(hipMemcpy(img.data(), mlog + (size_t)first_step * B * mlog_rec, img.size() * sizeof(double), hipMemcpyDeviceToHost));
    mlog_unpack(img.data(), (size_t)nsteps, B, mlog_rec, d.n, d.m, x0h, u0h, it, ito, st, J, c);
    return ALTRO_OK;
  }

  // the step range of altro_mpc_run_async, resp. the step of altro_mpc_prepare_async, against what the handle holds
  int mpc_run_rules(int first_step, int nsteps) {
    if (nsteps < 1 || first_step < 0) BFAIL(ALTRO_ERR_INVALID_ARG, "bad step range");
    if (noise && first_step + nsteps > noise_steps) BFAIL(ALTRO_ERR_INVALID_ARG, "steps outside the uploaded noise");
    // (under an episode clock an instance that runs off the end of its track goes idle there: altro_mpc_set_clock)
    if (!clock.on && first_step + nsteps + d.N > Nt) BFAIL(ALTRO_ERR_INVALID_ARG, "steps run past the end of the track");
    if (mlog && first_step + nsteps > mlog_cap) BFAIL(ALTRO_ERR_INVALID_ARG, "steps outside the capacity of the log (altro_mpc_set_log)");
    return ALTRO_OK;
  }
  int mpc_prepare_rules(int step) {
    if (step < 0) BFAIL(ALTRO_ERR_INVALID_ARG, "bad step");
    if (noise && step + 1 > noise_steps) BFAIL(ALTRO_ERR_INVALID_ARG, "step outside the uploaded noise");
    if (!clock.on && step + 1 + d.N > Nt) BFAIL(ALTRO_ERR_INVALID_ARG, "step runs past the end of the track");
    return ALTRO_OK;
  }
};

#undef BCHK
#undef BFAIL

}  // namespace altro
