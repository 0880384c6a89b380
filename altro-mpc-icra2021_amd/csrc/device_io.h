// device_io.h -- what the device-pointer entry points (altro_*_dev, altro_batch_wait_stream / _signal_stream;
// include/altro_batch.h) share between the two backends: the validation of a caller's device pointer, the pair of events a
// handle orders its stream against a caller's stream with, the read-out kernels of altro_batch_get_first_knot_dev, and the
// kernels that write constraint rows and box bounds from a caller's device arrays.
// Nothing here synchronises a stream or touches host memory.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "episode_clock.h"

namespace altro {

// A caller's pointer may reach a kernel only if the runtime knows it as device memory of the handle's device and the
// allocation it lies in holds at least `bytes` from that address on.  Returns nullptr when it does, else the reason.
// (hipPointerGetAttributes answers an error for plain host memory: an error is a refusal, and is cleared.)
inline const char* dev_extent_check(const void* p, size_t bytes, int device) {
  if (!p) return "null pointer";
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return "not a pointer the HIP runtime knows (host memory?)";
  }
  if (at.type != hipMemoryTypeDevice) return "not device memory";
  if (at.device != device) return "memory of another device than the handle's";
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();
    return "the extent of the allocation is unknown to the HIP runtime";
  }
  const uintptr_t a = (uintptr_t)p, b0 = (uintptr_t)base;
  if (a < b0 || a - b0 > size || size - (a - b0) < bytes) return "the allocation is shorter than the array the call reads or writes";
  return nullptr;
}

// Stream hand-over without the host: an event recorded on one stream and waited on by the other.  One event per direction,
// created on first use, owned and reused by the handle (a recorded event may be recorded again: a wait already enqueued keeps
// the state it captured).
struct StreamLink {
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  hipError_t wait(hipStream_t self, hipStream_t producer) {
    hipError_t e;
    if (!ev_in && (e = hipEventCreateWithFlags(&ev_in, hipEventDisableTiming)) != hipSuccess) return e;
    if ((e = hipEventRecord(ev_in, producer)) != hipSuccess) return e;
    return hipStreamWaitEvent(self, ev_in, 0);
  }
  hipError_t signal(hipStream_t self, hipStream_t consumer) {
    hipError_t e;
    if (!ev_out && (e = hipEventCreateWithFlags(&ev_out, hipEventDisableTiming)) != hipSuccess) return e;
    if ((e = hipEventRecord(ev_out, self)) != hipSuccess) return e;
    return hipStreamWaitEvent(consumer, ev_out, 0);
  }
  void destroy() {
    if (ev_in) hipEventDestroy(ev_in);
    if (ev_out) hipEventDestroy(ev_out);
    ev_in = ev_out = nullptr;
  }
};

// Per-instance active mask and restart selection (altro_batch_set_active / _restart_instances, host and _dev forms): the
// library's own copies of the caller's int32 arrays, normalised to 0 / 1, `cap` entries (the batch padded to whole waves on
// the 16-lane backend; padded slots hold 0: inactive whenever a mask is set, never restarted).  Both buffers are allocated
// by the first call that needs them and reused from then on.
__global__ void k_flags_copy(int* __restrict__ dst, const int* __restrict__ src, int B, int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  dst[i] = (i < B && src[i] != 0) ? 1 : 0;
}
struct InstanceFlags {
  int* active = nullptr;  // [cap]; read by the kernels only while `on`
  int* which = nullptr;   // [cap] selection of the restart in flight
  int* hstage = nullptr;  // [cap] where a host array lands before it is normalised
  bool on = false;        // a mask is set (off: every entry point acts on the whole batch)
  const int* mask() const { return on ? active : nullptr; }
  hipError_t ensure(int cap) {
    hipError_t e;
    if (!active && (e = hipMalloc(&active, (size_t)cap * sizeof(int))) != hipSuccess) return e;
    if (!which && (e = hipMalloc(&which, (size_t)cap * sizeof(int))) != hipSuccess) return e;
    if (!hstage && (e = hipMalloc(&hstage, (size_t)cap * sizeof(int))) != hipSuccess) return e;
    return hipSuccess;
  }
  // active (or which) <- the caller's array src [B], on the host (copied through hstage; the caller waits for the stream
  // before it returns) or on the device (read where it is); the same kernel writes dst either way
  hipError_t load(bool to_which, const int* src, bool dev, int B, int cap, hipStream_t st) {
    hipError_t e;
    if ((e = ensure(cap)) != hipSuccess) return e;
    int* dst = to_which ? which : active;
    if (!dev) {
      if ((e = hipMemcpyAsync(hstage, src, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
      src = hstage;
    }
    hipLaunchKernelGGL(k_flags_copy, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, dst, src, B, cap);
    return hipGetLastError();
  }
  void destroy() {
    if (active) hipFree(active);
    if (which) hipFree(which);
    if (hstage) hipFree(hstage);
    active = which = hstage = nullptr;
    on = false;
  }
};

// Per-instance episode clock (altro_mpc_set_clock, host and _dev forms; episode_clock.h has the tick rule): the library's own
// copies of the caller's two int32 arrays and the per-instance reference window, `cap` entries each (the batch padded to
// whole waves on the 16-lane backend; padded slots hold start 0, length 0: they never tick).  length: a caller's negative
// entry is stored as 0 (no local step is below it), -1 stands for "no length array".  All buffers are allocated by the first
// call and reused from then on.
__global__ void k_clock_load(int* __restrict__ start, int* __restrict__ length, const int* __restrict__ src_start,
                             const int* __restrict__ src_length, int B, int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  start[i] = i < B ? src_start[i] : 0;
  length[i] = i < B ? (src_length != nullptr ? (src_length[i] > 0 ? src_length[i] : 0) : -1) : 0;
}
// which == nullptr: every entry; else the entries it selects (the rewind of altro_batch_restart_instances)
__global__ void k_clock_window(int* __restrict__ window, const int* __restrict__ which, int value, int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap && (which == nullptr || which[i] != 0)) window[i] = value;
}
// mask[i] = instance i takes part in absolute step `step`: active (null: all) and ticking.  What the polish and the log kernel
// behind a one-step solve kernel go by (projected_newton = 1 inside the MPC loop)
__global__ void k_clock_step_mask(int* __restrict__ mask, ClockArgs clk, const int* __restrict__ active, int step, int Nt, int N,
                                  int dyn_blocks, int dyn_step_stride, int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  int lo, hi;
  clock_span(clk.start[i], clock_lmax(clk.length[i], Nt, N, dyn_blocks, dyn_step_stride), step, 1, lo, hi);
  mask[i] = (hi > lo && (active == nullptr || active[i] != 0)) ? 1 : 0;
}
struct EpisodeClock {
  int* start = nullptr;     // [cap]
  int* length = nullptr;    // [cap]
  int* window = nullptr;    // [cap] kept by the kernels while `on`
  int* stepmask = nullptr;  // [cap] k_clock_step_mask of the step being enqueued
  int* hstage = nullptr;    // [2 cap] where host arrays land
  bool on = false;
  ClockArgs args() const { return on ? ClockArgs{start, length, window} : ClockArgs{nullptr, nullptr, nullptr}; }
  static dim3 grid(int cap) { return dim3((unsigned)((cap + 255) / 256)); }
  hipError_t ensure(int cap) {
    hipError_t e;
    int** bufs[] = {&start, &length, &window, &stepmask};
    for (int** b : bufs)
      if (!*b && (e = hipMalloc(b, (size_t)cap * sizeof(int))) != hipSuccess) return e;
    if (!hstage && (e = hipMalloc(&hstage, 2 * (size_t)cap * sizeof(int))) != hipSuccess) return e;
    return hipSuccess;
  }
  // start / length <- the caller's arrays [B] (src_length may be null), on the host (through hstage; the caller waits for the
  // stream before it returns) or on the device; a clock that was off starts every window at `kref`, one that was on keeps them
  hipError_t load(const int* src_start, const int* src_length, bool dev, int B, int cap, int kref, hipStream_t st) {
    hipError_t e;
    if ((e = ensure(cap)) != hipSuccess) return e;
    if (!dev) {
      if ((e = hipMemcpyAsync(hstage, src_start, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
      src_start = hstage;
      if (src_length) {
        if ((e = hipMemcpyAsync(hstage + cap, src_length, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        src_length = hstage + cap;
      }
    }
    hipLaunchKernelGGL(k_clock_load, grid(cap), dim3(256), 0, st, start, length, src_start, src_length, B, cap);
    if (!on) hipLaunchKernelGGL(k_clock_window, grid(cap), dim3(256), 0, st, window, (const int*)nullptr, kref, cap);
    return hipGetLastError();
  }
  void destroy() {
    int** bufs[] = {&start, &length, &window, &stepmask, &hstage};
    for (int** b : bufs) {
      if (*b) hipFree(*b);
      *b = nullptr;
    }
    on = false;
  }
};

// altro_batch_update_constraint_data_dev, 16-lane backend: the caller's rows A [ninst_src][nk_src][p][nz] (row-major), b
// [ninst_src][nk_src][p] go straight to the lanes pack_constraints gave the constraint: Acon [ninst][N][16 lanes][16 columns],
// bcon [ninst][N][16].  One thread per (table slot ib, knot of the range, row, column 0..15); columns >= nz are written as 0,
// padded slots ib >= B mirror instance B - 1, a constraint with one block (per_knot = 0) fans out to every knot of its range
// and one with shared data (per_instance = 0) to every slot of the table.  A or b may be null (left as it is).
struct ConLanes {
  int lane[16];
};
__global__ void k_pack_con_rows(double* __restrict__ Acon, double* __restrict__ bcon, const double* __restrict__ A,
                                const double* __restrict__ b, ConLanes lanes, int ninst, int B, int N, int nz, int k0, int nk, int p,
                                int per_knot, int per_instance) {
  constexpr int LW_ = 16;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)ninst * nk * p * LW_) return;
  const int col = (int)(t % LW_);
  const int r = (int)((t / LW_) % p);
  const int kk = (int)((t / LW_ / p) % nk);
  const size_t ib = t / LW_ / p / nk;
  const size_t src = ib < (size_t)B ? ib : (size_t)B - 1;
  const size_t nks = per_knot ? (size_t)nk : 1;
  const size_t blk = (per_instance ? src * nks : 0) + (per_knot ? (size_t)kk : 0);
  const size_t et = (ib * N + (size_t)(k0 + kk)) * LW_ + lanes.lane[r];
  if (A) Acon[et * LW_ + col] = col < nz ? A[(blk * p + r) * nz + col] : 0.0;
  if (b && col == 0) bcon[et] = b[blk * p + r];
}

// The same on the one-wave-per-instance backend: AconT [ninst][N][z][P] (transposed), bcon [ninst][N][P]; the constraint's
// rows are r0 .. r0 + p - 1 of the P rows.  One thread per (table slot, knot of the range, row, element of z).
__global__ void k_pack_con_rows_wide(double* __restrict__ AconT, double* __restrict__ bcon, const double* __restrict__ A,
                                     const double* __restrict__ b, int ninst, int N, int z, int P, int r0, int k0, int nk, int p,
                                     int per_knot, int per_instance) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)ninst * nk * p * z) return;
  const int j = (int)(t % z);
  const int r = (int)((t / z) % p);
  const int kk = (int)((t / z / p) % nk);
  const size_t ib = t / z / p / nk;
  const size_t nks = per_knot ? (size_t)nk : 1;
  const size_t blk = (per_instance ? ib * nks : 0) + (per_knot ? (size_t)kk : 0);
  const size_t e = ib * N + (size_t)(k0 + kk);
  if (A) AconT[(e * z + j) * P + r0 + r] = A[(blk * p + r) * z + j];
  if (b && j == 0) bcon[e * P + r0 + r] = b[blk * p + r];
}

// altro_batch_set_bounds_dev, both backends.  One 16-lane group per row of the device tables zmin / zmax [rows][stride]
// (stride 16 on the 16-lane backend, n + m on the other); the group of row ib reads the caller's row src = ib (per_instance;
// rows ib >= B repeat row B - 1) or row 0 (shared), checks on the device what check_bound_rows checks on the host -- no NaN,
// zmin <= zmax, the finite sides those the BOX was added with (bit j of fin.lo / fin.hi; finite as the kernels test it) --
// and writes it only if the whole row passes, with the infinities of the absent sides and of the columns past nz regenerated.
// A row that fails leaves its table row as it was and adds 1 to *refusals (once per caller's row).  A shared row gets the
// same verdict in every group, so the table changes as a whole or not at all.
struct FinMask {
  unsigned long long lo[2], hi[2];   // elements 0..63, 64..127
};
__global__ void k_set_bounds_rows(double* __restrict__ zmin, double* __restrict__ zmax, const double* __restrict__ src_lo,
                                  const double* __restrict__ src_hi, FinMask fin, int nz, int stride, int rows, int B,
                                  int per_instance, unsigned long long* __restrict__ refusals) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t row = t / 16;
  const int lane = (int)(t % 16);
  const bool live = row < (size_t)rows;      // (every lane of the wave takes part in the shuffles)
  const size_t ib = live ? row : 0;
  const size_t src = per_instance ? (ib < (size_t)B ? ib : (size_t)B - 1) : 0;
  int bad = 0;
  for (int j = lane; j < nz; j += 16) {
    const double lo = src_lo[src * nz + j], hi = src_hi[src * nz + j];
    const bool lf = (fin.lo[j >> 6] >> (j & 63)) & 1ull, hf = (fin.hi[j >> 6] >> (j & 63)) & 1ull;
    if (lo != lo || hi != hi || lo > hi || (lo > -1e300) != lf || (hi < 1e300) != hf) bad = 1;
  }
  for (int s = 8; s > 0; s >>= 1) bad |= __shfl_xor(bad, s, 16);
  if (!live) return;
  if (bad) {
    if (lane == 0 && (per_instance ? ib < (size_t)B : ib == 0)) atomicAdd(refusals, 1ull);
    return;
  }
  for (int j = lane; j < stride; j += 16) {
    const bool lf = j < nz && ((fin.lo[j >> 6] >> (j & 63)) & 1ull), hf = j < nz && ((fin.hi[j >> 6] >> (j & 63)) & 1ull);
    zmin[ib * stride + j] = lf ? src_lo[src * nz + j] : -INFINITY;
    zmax[ib * stride + j] = hf ? src_hi[src * nz + j] : INFINITY;
  }
}
// rows 1 .. rows - 1 of a [rows][len] table <- row 0 (a shared row of bounds becomes one row per instance)
__global__ void k_fan_row0(double* __restrict__ tab, int len, int rows) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)rows * len || t < (size_t)len) return;
  tab[t] = tab[t % len];
}

// altro_batch_get_first_knot_dev, 16-lane backend: Zp holds [Bp] blocks of (2N + 1) knots x 16 lanes, two planes of N knots;
// lanes 0..n-1 of a knot are its state, n..n+m-1 its control.  One thread per (instance, lane) reads plane cur[inst]:
// u0 <- control of knot 0, x1 <- state of knot 1; lane 0 also copies the instance's status and iteration count.
__global__ void k_first_knot(double* __restrict__ u0, double* __restrict__ x1, int* __restrict__ status_out, int* __restrict__ iters_out,
                             const double* __restrict__ Zp, const int* __restrict__ cur, const int* __restrict__ status,
                             const int* __restrict__ iters, size_t plane, int B, int N, int n, int m) {
  constexpr int LW_ = 16;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * LW_) return;
  const int inst = t / LW_, j = t % LW_;
  const double* src = Zp + (size_t)inst * (2 * (size_t)N + 1) * LW_ + (size_t)cur[inst] * plane;
  if (j < n) {
    if (x1) x1[(size_t)inst * n + j] = src[LW_ + j];
  } else if (j < n + m) {
    if (u0) u0[(size_t)inst * m + (j - n)] = src[j];
  }
  if (j == 0) {
    if (status_out) status_out[inst] = status[inst];
    if (iters_out) iters_out[inst] = iters[inst];
  }
}

// The same on the one-wave-per-instance backend: X [B][2][N][n], U [B][2][N-1][m].  One thread per (instance, element of
// z = [x; u]).
__global__ void k_first_knot_wide(double* __restrict__ u0, double* __restrict__ x1, int* __restrict__ status_out, int* __restrict__ iters_out,
                                  const double* __restrict__ X, const double* __restrict__ U, const int* __restrict__ cur,
                                  const int* __restrict__ status, const int* __restrict__ iters, int B, int N, int n, int m) {
  const int nz = n + m;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * nz) return;
  const size_t inst = t / nz;
  const int j = (int)(t - inst * nz);
  const size_t pl = inst * 2 + cur[inst];
  if (j < n) {
    if (x1) x1[inst * n + j] = X[(pl * N + 1) * n + j];
  } else {
    if (u0) u0[inst * m + (j - n)] = U[pl * (size_t)(N - 1) * m + (j - n)];
  }
  if (j == 0) {
    if (status_out) status_out[inst] = status[inst];
    if (iters_out) iters_out[inst] = iters[inst];
  }
}

}  // namespace altro
