// episode_clock.h -- the tick rule of the per-instance episode clock (altro_mpc_set_clock), shared by the two solve kernels,
// the grouping score and the per-step mask of the polish.
//
// While a clock is set, instance b at absolute MPC step i has local step l = i - start[b] and ticks iff 0 <= l < lmax, with
// lmax the smallest of: its episode length (length[b] < 0: unbounded), Nt - N (the next window, l + 1 .. l + N, fits the
// uploaded track) and, with a dynamics track, the number of windows whose last block (l + 1) * step_stride + N - 2 exists.
// Every bound is an upper bound on l, so the steps an instance ticks inside a launch are ONE interval of launch-relative
// steps [lo, hi): the kernels compute it once per instance and compare step counters against it.
#pragma once
#include <hip/hip_runtime.h>

namespace altro {

// the device arrays of a clock as the kernels see them; start == nullptr: no clock is set
struct ClockArgs {
  const int* start;   // [cap] absolute step of the instance's local step 0 (may be negative)
  const int* length;  // [cap] steps of its episode; < 0: unbounded
  int* window;        // [cap] first knot of its reference window inside the track (what `kref` is without a clock)
};

// exclusive upper bound of the local steps that tick.  dyn_blocks <= 0: no dynamics track
__host__ __device__ inline int clock_lmax(int length, int Nt, int N, int dyn_blocks, int dyn_step_stride) {
  long long a = (long long)Nt - N;
  if (length >= 0 && length < a) a = length;
  if (dyn_blocks > 0 && dyn_step_stride > 0) {
    const long long w = ((long long)dyn_blocks - N + 1) / dyn_step_stride;   // windows 1 .. w have all their blocks
    if (w < a) a = w;
  }
  return a > 0 ? (int)a : 0;
}

// launch-relative steps [lo, hi) of first_step .. first_step + nsteps - 1 that the instance ticks (hi <= lo: none)
__host__ __device__ inline void clock_span(int start, int lmax, int first_step, int nsteps, int& lo, int& hi) {
  const long long t0 = (long long)start - first_step, t1 = t0 + lmax;
  lo = (int)(t0 < 0 ? 0 : t0 > nsteps ? nsteps : t0);
  hi = (int)(t1 < 0 ? 0 : t1 > nsteps ? nsteps : t1);
}

}  // namespace altro
