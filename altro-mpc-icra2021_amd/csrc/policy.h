// policy.h -- the feedback policy of the last solve, evaluated on the device (altro_batch_eval_policy(_dev),
// altro_batch_get_gains_dev; include/altro_batch.h):  u = u_k + K_k (x - x_k), saturated at the BOX.
// The kernels read what the solve kernels left in HBM -- the current plane of the trajectory, the gains, the marker that says
// whether the gains are valid, the bounds tables -- and write nothing the library owns.  No LDS, no synchronisation; the host
// twin of eval_policy runs the same kernel on staged copies, so both forms write the same bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace altro {

// What both kernels do with the sum s = sum_j K[a][j] dx_j once it is formed: the addition of the nominal control is the last
// operation, and a sum that is zero (x on the trajectory: every term is K * (+-0)) leaves the nominal control's bytes alone.
__device__ __forceinline__ double policy_add(double ubar, double s) { return s == 0.0 ? ubar : ubar + s; }
__device__ __forceinline__ double policy_clamp(double u, double lo, double hi) {
  u = u < lo ? lo : u;   // (an infinite side never compares: it does nothing)
  return u > hi ? hi : u;
}

// Control a of a 16-lane row: kd = the lane's element of gain row a, `on` = the gains are valid and the lane is a state lane.
// Lane j holds K[a][j] * dx_j (the others +0), the xor butterfly over the row adds them (strides 8, 4, 2, 1: after stride s
// every lane holds the sum of its aligned group of 16 / s lanes, built pairwise), and lane n + a (`mine`) takes
// policy_add(zl, sum) for `out`.  The product is rounded before the first addition and IEEE addition commutes, so every lane of
// the row ends with the same bits.  Every lane of the wave must be here (EXEC all ones at the shuffles).
__device__ __forceinline__ double policy16_control(double out, double kd, double dx, bool on, bool mine, double zl) {
#pragma clang fp contract(off)
  double p = on ? kd * dx : 0.0;
  for (int s = 8; s > 0; s >>= 1) p += __shfl_xor(p, s, 16);
  return mine ? policy_add(zl, p) : out;
}

// 16-lane backend.  One 16-lane row per instance, four instances per wave (256 threads: 16 rows); `rows` = the batch padded to
// whole waves, rows >= B compute on instance 0 and write nothing.  Zp: [Bp] blocks of (2N + 1) knots x 16 lanes, plane cur[b];
// lane j < n of knot k holds x_k[j], lane n + a holds u_k[a].  KD [b][k (N)][a][16]: state lane j of gain row a holds K[a][j];
// the control lanes hold factors of Quu and d and are masked out of the product.  kmu[b] < 0: no valid gains (fb 0).
// Summation order: policy16_control.
// Bounds: zmin / zmax element (b * 16 + lane) & imask, as the solve kernels address them (imask 15: one shared row).
__global__ void k_eval_policy(double* __restrict__ u, int* __restrict__ fb, const double* __restrict__ x, const int* __restrict__ knot,
                              const double* __restrict__ Zp, const int* __restrict__ cur, const double* __restrict__ KD,
                              const double* __restrict__ kmu, const double* __restrict__ zmin, const double* __restrict__ zmax,
                              unsigned imask, size_t plane, int rows, int B, int N, int n, int m, int clamp, int box_k0, int box_k1) {
#pragma clang fp contract(off)
  constexpr int LW_ = 16;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t row = t / LW_;
  const int lane = (int)(t % LW_);
  if (row >= (size_t)rows) return;           // (whole rows only: the shuffles below stay inside a row)
  const bool live = row < (size_t)B;
  const size_t b = live ? row : 0;
  const int kq = knot != nullptr ? knot[b] : 0;
  const bool inside = kq >= 0 && kq <= N - 2;
  const size_t k = inside ? (size_t)kq : 0;
  const bool valid = !(kmu[b] < 0.0);
  const double zl = Zp[b * (2 * (size_t)N + 1) * LW_ + (size_t)cur[b] * plane + k * LW_ + lane];
  const double dx = lane < n ? x[b * n + lane] - zl : 0.0;
  const double* kd = KD + ((b * N + k) * m) * LW_ + lane;
  double out = zl;
  const bool on = valid && lane < n;
  for (int a = 0; a < m; ++a) out = policy16_control(out, on ? kd[(size_t)a * LW_] : 0.0, dx, on, lane == n + a, zl);
  if (!live) return;
  if (lane == 0 && fb != nullptr) fb[b] = inside ? (valid ? 1 : 0) : -1;
  if (!inside || lane < n || lane >= n + m) return;
  if (clamp && (int)k >= box_k0 && (int)k <= box_k1) {
    const unsigned e = ((unsigned)b * LW_ + lane) & imask;
    out = policy_clamp(out, zmin[e], zmax[e]);
  }
  u[b * m + (lane - n)] = out;
}

// One-wave-per-instance backend.  One thread per (instance, control a): consecutive threads read consecutive elements of a
// column of Kg ([B][N-1] blocks, column-major m x n: element a + m j), so every load of the j loop is coalesced; x and the
// nominal state are the same address for the m threads of an instance.  X [B][2][N][n], U [B][2][N-1][m], plane cur[b].
// Summation order: s = fma(K[a][j], dx_j, s) for j = 0, 1, ..., n - 1 from s = +0.
// valid: reuse_ok (no setter has dropped the stored pass since the last launch) and word 128 of the instance's reuse state
// (solve_wide.h: bw_ok), the pair the solve kernel itself goes by.  Bounds: row b of zmin / zmax when b_pi, else row 0.
__global__ void k_eval_policy_wide(double* __restrict__ u, int* __restrict__ fb, const double* __restrict__ x, const int* __restrict__ knot,
                                   const double* __restrict__ X, const double* __restrict__ U, const int* __restrict__ cur,
                                   const double* __restrict__ Kg, const unsigned* __restrict__ bwst, int reuse_ok,
                                   const double* __restrict__ zmin, const double* __restrict__ zmax, int b_pi, int B, int N, int n, int m,
                                   int clamp, int box_k0, int box_k1) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * m) return;
  const size_t b = t / m;
  const int a = (int)(t - b * m);
  const int kq = knot != nullptr ? knot[b] : 0;
  const bool inside = kq >= 0 && kq <= N - 2;
  const bool valid = reuse_ok != 0 && bwst[b * 136 + 128] != 0u;
  if (a == 0 && fb != nullptr) fb[b] = inside ? (valid ? 1 : 0) : -1;
  if (!inside) return;
  const size_t k = (size_t)kq, pl = b * 2 + cur[b];
  const double* xk = X + (pl * N + k) * n;
  const double* xb = x + b * n;
  const double* kg = Kg + (b * (size_t)(N - 1) + k) * n * m + a;
  double s = 0.0;
  if (valid)
    for (int j = 0; j < n; ++j) s = fma(kg[(size_t)m * j], xb[j] - xk[j], s);
  double out = policy_add(U[(pl * (size_t)(N - 1) + k) * m + a], s);
  if (clamp && kq >= box_k0 && kq <= box_k1) {
    const size_t e = (b_pi ? b * (size_t)(n + m) : 0) + n + a;
    out = policy_clamp(out, zmin[e], zmax[e]);
  }
  u[b * m + a] = out;
}

// altro_batch_get_gains_dev, 16-lane backend: KD / Dff -> K [B][N-1] blocks of m x n column-major, d [B][N-1][m], the values
// altro_batch_get_gains unpacks on the host.  One thread per (instance, knot < N - 1, control a, lane); lane j < n writes
// K[a][j], lane 0 writes d[a]: from the gain rows (d_in_kd: control lane n + at.col[a] of gain row at.row[a], the host fills
// the table from kd_drow / kd_dcol of solve_dpp16.h) or from Dff [b][N + 1][16], and 0 where the instance's last iteration was
// confirmed by the costate sweep.
struct DSlots {
  int row[16], col[16];
};
__global__ void k_unpack_gains(double* __restrict__ K, double* __restrict__ d, const double* __restrict__ KD, const double* __restrict__ Dff,
                               const int* __restrict__ dzero, int d_in_kd, DSlots at, int B, int N, int n, int m) {
  constexpr int LW_ = 16;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)B * (N - 1) * m * LW_) return;
  const int lane = (int)(t % LW_);
  const int a = (int)((t / LW_) % m);
  const size_t k = (t / LW_ / m) % (size_t)(N - 1);
  const size_t b = t / LW_ / m / (size_t)(N - 1);
  if (K != nullptr && lane < n) K[((b * (N - 1) + k) * n + lane) * m + a] = KD[((b * N + k) * m + a) * LW_ + lane];
  if (d != nullptr && lane == 0) {
    const double da = d_in_kd ? KD[((b * N + k) * m + at.row[a]) * LW_ + n + at.col[a]] : Dff[(b * (N + 1) + k) * LW_ + n + a];
    d[(b * (N - 1) + k) * m + a] = dzero[b] != 0 ? 0.0 : da;
  }
}

}  // namespace altro
