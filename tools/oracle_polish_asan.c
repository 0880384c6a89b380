/* Stand-alone sanitizer check of the oracle's projected-Newton polish at n + m > 32 (CPU only).
 *
 *   make -C oracle asan
 *   gcc -O1 -g -std=c99 -fsanitize=address,undefined -Ioracle tools/oracle_polish_asan.c \
 *       -Loracle/_build -laltro_oracle_asan -Wl,-rpath,$PWD/oracle/_build -lm -o oracle/_build/polish_asan
 *   oracle/_build/polish_asan
 *
 * A (40, 6) problem with a BOX on every coordinate (2 (n + m) = 92 values per evaluation): the shape at which pn_row's
 * fixed buffer of 64 doubles overflowed.  Prints the polish statistics; exit status 0 when the polish ran and converged. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "altro_oracle.h"

static unsigned long long state = 88172645463325252ull;
static double rnd(void) {   /* xorshift, uniform in (-1, 1) */
  state ^= state << 13; state ^= state >> 7; state ^= state << 17;
  return (double)(state >> 11) / 4503599627370496.0 - 1.0;
}

int main(int argc, char** argv) {
  int n = argc > 1 ? atoi(argv[1]) : 40, m = argc > 2 ? atoi(argv[2]) : 6, N = argc > 3 ? atoi(argv[3]) : 8;
  int nz = n + m;
  double dt = 0.1;
  orc_solver* s = orc_create(n, m, N, dt);
  double *A = calloc((size_t)n * n, sizeof(double)), *B = calloc((size_t)n * m, sizeof(double));
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) A[i + n * j] = (i == j ? 0.9 : 0.0) + 0.3 * rnd() / sqrt((double)n);
  for (int i = 0; i < n * m; ++i) B[i] = rnd() / sqrt((double)m);
  orc_set_dynamics(s, A, B, NULL, 0);
  double *Q = calloc(n, sizeof(double)), *R = calloc(m, sizeof(double));
  for (int i = 0; i < n; ++i) Q[i] = 10.0;
  for (int i = 0; i < m; ++i) R[i] = 10.0;
  orc_set_cost(s, Q, R, Q);
  double *Xr = calloc((size_t)N * n, sizeof(double)), *Ur = calloc((size_t)(N - 1) * m, sizeof(double)), *x0 = calloc(n, sizeof(double));
  for (int k = 0; k < N; ++k)
    for (int i = 0; i < n; ++i) Xr[k * n + i] = 3.0 * k / (N - 1.0) * ((i & 1) ? 1.0 : -1.0);
  for (int i = 0; i < n; ++i) x0[i] = 0.5 * rnd();
  orc_set_reference(s, Xr, Ur);
  orc_set_initial_state(s, x0);
  orc_set_controls(s, Ur);
  double *zmin = calloc(nz, sizeof(double)), *zmax = calloc(nz, sizeof(double));
  for (int j = 0; j < nz; ++j) { zmax[j] = j < n ? 50.0 : 0.5; zmin[j] = -zmax[j]; }
  orc_add_constraint(s, ORC_BOX, ORC_INEQ, 1, N - 1, 0, NULL, NULL, zmin, zmax, 0);
  orc_opts o;
  orc_default_opts(&o);
  o.penalty_initial = 10.0; o.penalty_scaling = 10.0; o.iterations_outer = 40;
  o.constraint_tolerance = 1e-8; o.projected_newton = 1;
  orc_set_opts(s, &o);
  orc_solve(s);
  const orc_stats* st = orc_get_stats(s);
  printf("(%d, %d, %d): status %d, iterations %d, polish ran %d failed %d residual %.3e, c_max %.3e, dual residual %.3e -> %.3e\n",
         n, m, N, st->status, st->iterations, st->pn_ran, st->pn_failed, st->pn_residual, st->c_max, st->pn_dual_residual0, st->pn_dual_residual);
  int ok = st->pn_ran == 1 && st->pn_failed == 0 && st->pn_residual < 1e-8;
  orc_destroy(s);
  free(A); free(B); free(Q); free(R); free(Xr); free(Ur); free(x0); free(zmin); free(zmax);
  return ok ? 0 : 1;
}
