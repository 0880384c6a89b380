// mpc_log.h -- the per-step log of the device-resident MPC loop (altro_mpc_set_log / altro_mpc_get_log).
//
// What the reference's MPC loops record at every step -- X_traj[i+1] = prob_mpc.x0, iters[i], status[i], costs[i]
// (simple_rocket.jl:137-205, random_linear_problem.jl:166-174) -- for a launch that runs its steps inside one kernel.
// One record per (absolute step, instance), step-major and indexed by the CALLER's instance index (never by the wave slot
// a grouped launch gives an instance):
//
//   log [capacity][batch][rec] doubles,  rec = nv + MLOG_TAIL
//     [0, nv)    x0 of the step's solve in [0, n), first control of the trajectory the step left in [n, n + m)
//                (nv = 16 on the 16-lane backend: the row as its lanes hold it; nv = n + m on the wide backend)
//     [nv]       cost      [nv + 1]  c_max
//     [nv + 2]   two int32: iterations, iterations_outer      [nv + 3]  two int32: status, 0
//
// A slot no step has written since altro_mpc_set_log holds 0xFF bytes: -1 in the integers, NaN in the doubles.
// Offsets are size_t everywhere: the log is the one array of a handle that may grow past 4 GiB.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace altro {

constexpr int MLOG_TAIL = 4;

// the scalars of one record, written by one lane
__device__ __forceinline__ void mlog_tail(double* tail, double cost, double cmax, int iters, int iters_outer, int status) {
  tail[0] = cost;
  tail[1] = cmax;
  int* ti = reinterpret_cast<int*>(tail + 2);
  ti[0] = iters;
  ti[1] = iters_outer;
  ti[2] = status;
  ti[3] = 0;
}

// host image of `nsteps` step records -> the caller's arrays (any of them may be null)
inline void mlog_unpack(const double* img, size_t nsteps, size_t B, size_t rec, int n, int m, double* x0, double* u0,
                        int32_t* iterations, int32_t* iterations_outer, int32_t* status, double* cost, double* c_max) {
  const size_t nv = rec - MLOG_TAIL;
  for (size_t e = 0; e < nsteps * B; ++e) {
    const double* r = img + e * rec;
    if (x0) std::memcpy(x0 + e * n, r, (size_t)n * sizeof(double));
    if (u0) std::memcpy(u0 + e * m, r + n, (size_t)m * sizeof(double));
    if (cost) cost[e] = r[nv];
    if (c_max) c_max[e] = r[nv + 1];
    int32_t ti[4];
    std::memcpy(ti, r + nv + 2, sizeof(ti));
    if (iterations) iterations[e] = ti[0];
    if (iterations_outer) iterations_outer[e] = ti[1];
    if (status) status[e] = ti[2];
  }
}

}  // namespace altro
