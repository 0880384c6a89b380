/*
 * altro_batch.h -- C-ABI of libaltro_hip.so: batched ALTRO (AL-iLQR) MPC solves on MI355X.
 *
 * The reference (RoboticExplorationLab/altro-mpc-icra2021) has no FFI: its benchmark scripts
 * call the exported Julia API of Altro.jl / TrajectoryOptimization.jl / RobotDynamics.jl
 * in-process.  Each entry point below replaces one of those calls for a BATCH of independent
 * MPC instances; the reference call site it mirrors is cited (paths relative to the reference
 * repo).  A Julia `ccall` shim over these symbols is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns int32 (0 = ALTRO_OK); nothing throws or aborts across the ABI;
 *     altro_last_error() returns a message for the last failing call of a handle (or of
 *     altro_batch_create when called with NULL).
 *   - solver failures are NOT errors: they are per-instance status values (enum below), as in
 *     the reference (random_linear_problem.jl:166, altro_solver.jl:81).
 *   - the caller owns every buffer it passes; the library copies in/out and keeps no caller
 *     pointer after return (Julia's GC may move or free them).
 *   - host arrays are instance-major: X is [batch][N][n], U is [batch][N-1][m]; matrices are
 *     COLUMN-major n x n / n x m blocks (Julia layout).
 *   - a handle is single-owner (not thread-safe) and owns one HIP stream and all its device
 *     memory.  Different handles may be driven from different threads.
 *   - all arithmetic is FP64, as in the reference.
 */
#ifndef ALTRO_BATCH_H
#define ALTRO_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  ALTRO_OK = 0,
  ALTRO_ERR_INVALID_ARG = 1,
  ALTRO_ERR_UNSUPPORTED = 2, /* problem shape/constraint outside the built kernel set */
  ALTRO_ERR_HIP = 3,         /* HIP runtime failure (message has the HIP error string) */
  ALTRO_ERR_STATE = 4,       /* call sequence error (e.g. solve before set_dynamics) */
  ALTRO_ERR_INTERNAL = 5     /* host allocation failure or any other C++ exception inside the library:
                                caught at the boundary, never propagated to the caller */
};

/* Altro.TerminationStatus.  Only UNSOLVED and SOLVE_SUCCEEDED are named in the reference
 * (simple_rocket.jl:144, random_linear_problem.jl:166); order restated from Altro.jl v0.2. */
enum {
  ALTRO_UNSOLVED = 0,
  ALTRO_SOLVE_SUCCEEDED = 1,
  ALTRO_MAX_ITERATIONS = 2,
  ALTRO_MAX_ITERATIONS_OUTER = 3,
  ALTRO_MAXIMUM_COST = 4,
  ALTRO_STATE_LIMIT = 5,
  ALTRO_CONTROL_LIMIT = 6,
  ALTRO_NO_PROGRESS = 7,
  ALTRO_COST_INCREASE = 8
};

/* constraint menu: user constraint types of the reference are Julia closures
 * (new_constraints.jl:31-62), which cannot cross a C ABI; they are all affine maps of
 * z = [x;u] into {=0, <=0, second-order cone} and are passed as data. */
enum { ALTRO_CON_BOX = 0, ALTRO_CON_LINEAR = 1, ALTRO_CON_SOC = 2 };
enum { ALTRO_SENSE_EQ = 0, ALTRO_SENSE_INEQ = 1 };

typedef struct altro_dims {
  int32_t batch; /* number of independent MPC instances */
  int32_t n;     /* state dimension   */
  int32_t m;     /* control dimension */
  int32_t N;     /* knot points       */
} altro_dims;

/* Altro.SolverOptions: fields the reference sets (run_random_linear.jl:41-49,
 * run_simple_rocket.jl:39-50, grasp_benchmark.jl:19-34, ALTROParams.jl:86-95) plus the
 * iLQR/AL internals they rely on.  altro_default_opts() fills Altro.jl's defaults. */
typedef struct altro_opts {
  double cost_tolerance;
  double cost_tolerance_intermediate;
  double gradient_tolerance;
  double gradient_tolerance_intermediate;
  double constraint_tolerance;
  double penalty_initial;  /* NaN = per-constraint default (1.0) */
  double penalty_scaling;  /* NaN = per-constraint default (10)  */
  double penalty_max;
  double dual_max;
  double line_search_lower_bound;
  double line_search_upper_bound;
  double max_cost_value;
  double max_state_value;
  double max_control_value;
  double bp_reg_initial;
  double bp_reg_increase_factor;
  double bp_reg_max;
  double bp_reg_min;
  double bp_reg_fp;
  int32_t iterations;
  int32_t iterations_inner;
  int32_t iterations_outer;
  int32_t iterations_linesearch;
  int32_t dJ_counter_limit;
  int32_t reset_duals;
  int32_t reset_penalties;
  int32_t bp_reg;
  int32_t soc_second_order;
  /* 0 (default): the 16-lane kernels take these shortcuts relative to Altro.jl's forwardpass! / backwardpass!
   *   - confirmation iterations.  The last iteration of nearly every warm MPC solve only confirms convergence: the
   *     problem is quadratic inside an active set, so at the point the previous Newton step reached the backward
   *     pass returns feedforward terms at rounding level; the reference then rolls out Z + O(|d|), finds
   *     |dJ| ~ 1e-13 and stops (step accepted, or after iterations_linesearch fruitless halvings, whichever way
   *     the rounding of J falls).  Such an iteration is booked as converged on the trajectory it holds, with the
   *     same status and iteration count, when (a) on box-constrained problems, from the second iteration of an
   *     inner solve on, the first-order costate sweep finds |l_u + B' lambda| <= 0.25e-9 dt R (1 + |u|) at every
   *     knot (so |d| <= 0.5e-9 (1 + |u|)) and the active set unchanged since the previous backward pass -- no
   *     backward pass is run, the gains reported are that pass's (the same matrices) with d = 0; or (b) a backward
   *     pass returns |d| <= 1e-9 (1 + |u|) at every knot -- its rollout, line search and gradient sweep are skipped;
   *   - a line search whose alpha = 1 trial moved no element by more than 1e-7 (1 + |z|) while the quadratic
   *     model promised less than cost_tolerance / 1000 is ended there (the reference halves alpha
   *     iterations_linesearch more times, fails the same way, and the iteration ends "converged" either way);
   *   - S is not re-symmetrised after every knot of the backward pass (the asymmetry stays at rounding level).
   * 1: none of them, the reference's exact sequence (about half the throughput on BASELINE's headline workload).
   * The one-wave-per-instance kernel (sizes outside the 16-lane set, per-knot dynamics) takes (b) and the line-search
   * early-out the same way in the default mode and always re-symmetrises S; for n, m <= 16 (at most 16 linear rows,
   * no cones) and for box-only time-invariant problems with n > 16, m <= 16 it also has a costate sweep (a), which
   * solves for the feedforward terms with the factors of Quu the last backward pass stored and applies test (b) to them.
   * For the n > 16 class it goes one step further (gain reuse): any iteration whose active set and penalty are those of
   * the stored pass takes its gains K from memory -- inside a fixed active set they do not depend on the trajectory --
   * and only its feedforward terms from that first-order pass; dynamics, cost, constraint data and options setters
   * drop the stored pass. */
  int32_t strict;
  /* Altro.SolverOptions.kickout_max_penalty (default false): with 0 the AL outer loop does not stop when the penalty
   * has reached penalty_max -- it goes on with dual updates at the cap until the constraints are satisfied or
   * iterations_outer runs out (MAX_ITERATIONS_OUTER); 1 ends the solve there (status UNSOLVED if the violation is
   * still above the tolerance). */
  int32_t kickout_max_penalty;
  /* Projected-Newton polish (Altro.jl solve!(::ALTROSolver): AL stage to projected_newton_tolerance, then
   * solve!(::ProjectedNewtonSolver) if the violation is still above constraint_tolerance; ALTRO, IROS 2019, Algorithm 4).
   * altro_default_opts() gives 0: Altro.jl's own default is true, but every script of the reference on this path sets
   * projected_newton = false (eleven occurrences), and the ccall shim passes the Julia-side value explicitly.  1: plain
   * solves (altro_batch_solve) run the polish after the AL kernel -- the algorithm is csrc/pn_core.h, seen through
   * csrc/pn_polish.h on the 16-lane backend and through csrc/pn_wide.h on the one-wave-per-instance backend (any n <= 64,
   * m <= 32, per-knot dynamics) -- primal projection first, then
   * Altro's multiplier projection (altro_batch_get_polish_dual_residuals).  Inside the device-resident MPC loop
   * (altro_mpc_step_async / altro_mpc_run_async) every step is then a one-step solve kernel followed by the polish kernel:
   * the next step shifts the polished trajectory and the AL duals (the projected multipliers stay inside the polish).
   * Where the polish ran, the status is SOLVE_SUCCEEDED only if the violation it left is below constraint_tolerance, and
   * UNSOLVED otherwise (it failed, or stopped above the tolerance) -- whatever the AL stage reported at its looser one.
   * PARITY UNPINNED: the reference stores no polished trajectory. */
  int32_t projected_newton;
  double projected_newton_tolerance;   /* 1e-3 */
  double active_set_tolerance_pn;      /* 1e-3: inequality rows with c >= -tol join the polish's active set */
  double rho_chol;                     /* 1e-2: S + rho I is factored, the solve is refined against S */
  double rho_primal;                   /* 1e-8: added to the diagonal cost Hessian */
  double r_threshold;                  /* 1.1 */
} altro_opts;

#define ALTRO_TRACE_LEN 16 /* per-instance trace depth kept on device */

typedef struct altro_handle altro_handle;

/* SolverOptions() defaults */
int32_t altro_default_opts(altro_opts* opts);

/* ALTROSolver(prob, opts): random_linear_problem.jl:87, simple_rocket.jl:128,
 * grasp_mpc.jl:35, ALTROParams.jl:96.  Allocates every device workspace. */
int32_t altro_batch_create(const altro_dims* dims, const altro_opts* opts, int32_t device,
                           altro_handle** out);
int32_t altro_batch_destroy(altro_handle* h);
const char* altro_last_error(const altro_handle* h);

/* RD.LinearModel(A, B[, d]; dt): random_linear_problem.jl:8; LTV/affine: ALTROParams.jl:61,
 * linearized_dynamics.jl:69-96.   x+ = A x + B u + f.
 *   per_instance != 0: arrays hold `batch` blocks, else one block shared by all instances
 *   per_knot     != 0: each block holds N-1 knot blocks (LTV); for an (n, m) of the 16-lane kernel set this
 *                      must be the first call after create (the handle then moves to the wide kernel)
 * f may be NULL (zero). */
int32_t altro_batch_set_dynamics(altro_handle* h, const double* A, const double* B, const double* f,
                                 int32_t per_knot, int32_t per_instance);

/* TO.TrackingObjective(Q, R, Z; Qf) / LQRObjective with diagonal weights: mpc.jl:26-29.
 * Stage costs are scaled by dt, the terminal cost is not (random_linear_problem.jl:52-53). */
int32_t altro_batch_set_tracking_cost(altro_handle* h, const double* Qdiag, const double* Rdiag,
                                      const double* Qfdiag, double dt);
/* The same with weights PER INSTANCE: Qdiag [batch][n], Rdiag [batch][m], Qfdiag [batch][n] -- every problem of the batch
 * owns its TrackingObjective, as the reference's generator builds them (random_linear_problem.jl:11-13: Q = Diagonal(10 rand(n)),
 * Qf = (N-1) Q per problem; mpc.jl:26-29).  dt is common.  Callable wherever altro_batch_set_tracking_cost is; a call of
 * either replaces what the other set.  Results of instance i are bit-identical to those of a handle given instance i's
 * weights through altro_batch_set_tracking_cost.  Drops the stored gains. */
int32_t altro_batch_set_tracking_cost_per_instance(altro_handle* h, const double* Qdiag, const double* Rdiag,
                                                   const double* Qfdiag, double dt);

/* add_constraint!(cons, con, inds): random_linear_problem.jl:23-24 (BoundConstraint),
 * rocket_landing_problem.jl:96,123-124,142,165, grasp_problem.jl:29-67, ALTROParams.jl:67-78.
 *   k_first..k_last: 0-based inclusive knot range (knot N-1 is terminal: state columns only)
 *   BOX:    zmin, zmax of length n+m (+-inf = absent)
 *   LINEAR: A [p][n+m] ROW-major, b [p]; value A z + b {= 0 | <= 0}
 *   SOC:    A, b as above; value v = A z + b with ||v[0..p-2]|| <= v[p-1]
 *   per_knot: bit 0 set: A, b hold one block per knot of the range (grasp_problem.jl:35-67);
 *             bit 1 set (values 2, 3): A, b hold those blocks once PER INSTANCE ([batch][knots][p][n+m] and
 *             [batch][knots][p]): every problem of the batch owns its tables, as the reference's problems do
 *             when mpc_update! rewrites them in place (grasp_mpc_helpers.jl:46-55) -- instances may then sit at
 *             different MPC steps or footholds.  The structure (kind, sense, knot range, p) stays common.
 * Without bit 1 the data is shared by all instances of the batch.  HIP library limits: one BOX; cones of
 * dimension 2..4; on the 16-lane kernels ((n,m) in (12,4) (12,3) (8,4) (6,6) (6,3)) at most
 * 16 LINEAR / SOC rows are active at any one knot (a cone of dimension 2..4 takes the first lanes
 * of an aligned group of 4, linear rows take any free lane; constraints with disjoint knot
 * ranges share lanes); every other (n <= 64, m <= 32) runs on the one-wave-per-instance kernel with
 * up to 64 LINEAR / SOC rows in total; constraints are added before the first solve. */
int32_t altro_batch_add_constraint(altro_handle* h, int32_t kind, int32_t sense, int32_t k_first,
                                   int32_t k_last, int32_t p, const double* A, const double* b,
                                   const double* zmin, const double* zmax, int32_t per_knot,
                                   int32_t* con_id);
/* in-place mutation of per-knot constraint data: grasp_mpc_helpers.jl:46-55.  A, b in the layout the
 * constraint was added with (per instance if it was); either may be NULL (unchanged). */
int32_t altro_batch_update_constraint_data(altro_handle* h, int32_t con_id, const double* A,
                                           const double* b);
/* New bounds for the BOX constraint con_id, in place: BoundConstraint(n, m; x_min, x_max, u_min, u_max) per problem
 * (random_linear_problem.jl:16-23 draws u_bnd for each problem it generates).  per_instance = 0: zmin, zmax are one
 * [n+m] pair for the batch; 1: [batch][n+m] each.  The knot range and the PATTERN of finite sides (which elements have a
 * finite lower and which a finite upper bound, finite meaning zmin > -1e300 / zmax < 1e300) stay those the BOX was added
 * with: they fix the layout of its duals.  ALTRO_ERR_INVALID_ARG for a con_id that is not a BOX (also before any BOX is
 * added), a row whose pattern differs, a NaN, or zmin > zmax; nothing changes then.  Callable before the first solve, between
 * solves and between MPC steps, like altro_batch_update_constraint_data; drops the stored gains.  Results of instance i are
 * bit-identical to those of a handle whose BOX was added with instance i's row. */
int32_t altro_batch_set_bounds(altro_handle* h, int32_t con_id, const double* zmin, const double* zmax,
                               int32_t per_instance);

/* TO.set_initial_state!: random_linear_problem.jl:130.  x0 is [batch][n]. */
int32_t altro_batch_set_initial_state(altro_handle* h, const double* x0);
/* TO.update_trajectory!(obj, Z_track, k): random_linear_problem.jl:133.
 * Xref [batch][N][n], Uref [batch][N-1][m]. */
int32_t altro_batch_set_reference(altro_handle* h, const double* Xref, const double* Uref);
/* initial_trajectory! / initial_controls! / initial_states!: mpc.jl:45, altro_solver.jl:70-71.
 * X may be NULL (iLQR re-rolls the states out from x0). */
int32_t altro_batch_set_initial_trajectory(altro_handle* h, const double* X, const double* U);
/* RD.shift_fill!(Z) and Altro.shift_fill!(conSet): random_linear_problem.jl:136,139 */
int32_t altro_batch_shift_fill(altro_handle* h, int32_t shift_primal, int32_t shift_dual);
/* set_options!: flexible_sat_mpc.jl:163 */
int32_t altro_batch_set_options(altro_handle* h, const altro_opts* opts);

/* solve!(solver): random_linear_problem.jl:113.  Synchronous on return. */
int32_t altro_batch_solve(altro_handle* h);
/* Same, but only enqueued on the handle's stream; pair with altro_batch_synchronize. */
int32_t altro_batch_solve_async(altro_handle* h);
int32_t altro_batch_synchronize(altro_handle* h);

/* benchmark_solve!(solver; samples, evals): random_linear_problem.jl:161 (samples = 5, evals = 5),
 * simple_rocket.jl:171, run_simple_rocket.jl:67,102, flexible_sat_mpc.jl:166.  Altro.jl's harness
 * around BenchmarkTools: Z0 = copy of the solver's trajectory; then 1 warm-up evaluation and
 * samples x evals timed evaluations of { initial_trajectory!(solver, Z0); solve!(solver) }.
 * Only the primal trajectory is restored: with reset_duals = false (run_random_linear.jl:47) every
 * repetition starts from the multipliers the previous one left, which is what the iteration counts
 * and times stored in the reference's *.jld2 files measure (the statistics of the LAST repetition;
 * random_linear_problem.jl:171-173).  On return the handle holds the result of the last repetition.
 * sample_ms (may be NULL) receives `samples` values: device time of one sample divided by evals,
 * i.e. BenchmarkTools' per-evaluation time of each sample, in ms for the whole batch.  Synchronous.
 * ALTRO_ERR_STATE while an active mask is set (altro_batch_set_active). */
int32_t altro_batch_benchmark_solve(altro_handle* h, int32_t samples, int32_t evals, float* sample_ms);

/* states(solver), controls(solver), Altro.get_duals: random_linear_problem.jl:177-181 */
int32_t altro_batch_get_states(altro_handle* h, double* X);
int32_t altro_batch_get_controls(altro_handle* h, double* U);
/* duals of one constraint: BOX -> [batch][nk][2][n+m] (upper rows, then lower rows; zero for
 * unbounded elements), LINEAR/SOC -> [batch][nk][p] */
int32_t altro_batch_get_duals(altro_handle* h, int32_t con_id, double* lambda);
int32_t altro_batch_set_duals(altro_handle* h, int32_t con_id, const double* lambda);

/* iterations(solver), status(solver), cost(solver), max_violation(solver), solver.stats:
 * random_linear_problem.jl:166-174.  Any output pointer may be NULL.  Arrays have `batch`
 * entries; traces are [batch][ALTRO_TRACE_LEN] (cost and max violation after each of the
 * first ALTRO_TRACE_LEN iLQR iterations). */
int32_t altro_batch_get_stats(altro_handle* h, int32_t* iterations, int32_t* iterations_outer,
                              int32_t* status, double* cost, double* c_max, double* cost_trace,
                              double* cmax_trace);
/* accepted line-search step of each of the first ALTRO_TRACE_LEN iLQR iterations of the last
 * solve, [batch][ALTRO_TRACE_LEN] (0 = the search failed and the trajectory was kept) */
int32_t altro_batch_get_alpha_trace(altro_handle* h, double* alpha_trace);
/* feedback gains K [batch][N-1] blocks of m x n (column-major) and feedforward d [batch][N-1][m]
 * left by the last backward pass of the last solve (backwardpass!, ilqr K/d; either may be NULL) */
int32_t altro_batch_get_gains(altro_handle* h, double* K, double* d);
/* factors of Quu = L D L' kept with the gains for the first-order sweep (16-lane kernels; ALTRO_ERR_UNSUPPORTED on the
 * one-wave-per-instance path): F [batch][N-1][m][m] row-major, entry (a, a) = 1 / D_a, (a, b < a) = L[a][b], 0 above */
int32_t altro_batch_get_gain_factors(altro_handle* h, double* F);
/* device time of the last solve launch sequence on the handle's stream, HIP events (ms) */
int32_t altro_batch_last_solve_ms(altro_handle* h, float* ms);
/* Launch-duration history of the solve kernel (HIP events recorded on the handle's stream around
 * every solve launch since the last reset): the measurement behind bench.py's roofline figure.
 * reset also clears the work counters below.  Synchronises the stream.  timing_get returns the most recent
 * launches, at most 1024 of them (launch_ring.h CAP); the work counters keep accumulating over ALL launches since the
 * reset, so a caller that relates the two (bench.py) must stay within 1024 launches per reset (it asserts so). */
int32_t altro_batch_timing_reset(altro_handle* h);
int32_t altro_batch_timing_get(altro_handle* h, float* ms, int32_t capacity, int32_t* count);
/* Work done since the last timing reset, per instance: iLQR backward passes, rollouts (open-loop
 * + the alpha = 1 trial of every line search) and further line-search trials (evaluated without a
 * rollout, DESIGN.md "Line search").  These are the measured counts SURVEY 8(d)'s flops_solve
 * formula is evaluated with.  Arrays of `batch` int64; any pointer may be NULL. */
int32_t altro_batch_get_work_counters(altro_handle* h, int64_t* backward_passes, int64_t* rollouts,
                                      int64_t* trials);
/* Per instance since the last timing reset: solves run, iLQR iterations, solves that ended
 * SOLVE_SUCCEEDED.  Arrays of `batch` int64; any pointer may be NULL. */
int32_t altro_batch_get_solve_counters(altro_handle* h, int64_t* solves, int64_t* iterations, int64_t* succeeded);
/* Per instance since the last timing reset: iLQR iterations of the default (non-strict) mode that were confirmed
 * as converged by the first-order costate sweep alone -- no backward pass, no first-order sweep with the stored gains,
 * no rollout (altro_opts.strict).  Every iteration is exactly one of three kinds:
 * iterations = backward_passes + reused (altro_batch_get_reuse_counter) + confirmed. */
int32_t altro_batch_get_confirm_counter(altro_handle* h, int64_t* confirmed);
/* Per instance since the last timing reset: iLQR iterations of the default mode that took their gains from memory
 * instead of running a backward pass -- the active set (hashed knot by knot) and the penalty were those of the pass
 * that left the gains there, in this solve or an earlier one, and inside a fixed active set K and Quu do not depend
 * on the trajectory.  Such an iteration runs the first-order recursion (d_k = -Quu^-1 Qu, s_k = Qx + K' Qu, dV) and
 * then its rollout as usual; counted in `iterations`, not in `backward_passes` (altro_opts.strict = 1: never taken).
 * Every setter the gains depend on (dynamics, cost, constraints, options) drops them. */
int32_t altro_batch_get_reuse_counter(altro_handle* h, int64_t* reused);
/* Projected-Newton polish of the last solve, per instance (arrays of `batch`; any pointer may be NULL): ran (the AL
 * stage ended SOLVE_SUCCEEDED-or-unsolved above constraint_tolerance), failed (a block of D H^-1 D' + rho I was not
 * positive definite), residual (final max |d| over the active rows, the initial condition and the dynamics defects).
 * All zero when altro_opts.projected_newton = 0. */
int32_t altro_batch_get_polish_stats(altro_handle* h, int32_t* ran, int32_t* failed, double* residual);
/* The dual half of the polish (multiplier_projection! of Altro.jl's ProjectedNewtonSolver; ALTRO, IROS 2019, IV-B): at
 * the polished trajectory the multipliers of the polish's active rows D (initial condition, active constraint rows,
 * dynamics) are projected, lam <- lam - (D D')^-1 D (g + D' lam), g the gradient of the cost.  Per instance (arrays of
 * `batch`; any pointer may be NULL): the stationarity residual ||g + D' lam||_2 `before` (AL duals on the active box /
 * linear rows, zero elsewhere) and `after` the projection, and whether a block of D D' was not positive definite.  The
 * projected multipliers stay inside the polish, as Altro's do; the AL duals (altro_batch_get_duals) are untouched.
 * All zero when the polish did not run. */
int32_t altro_batch_get_polish_dual_residuals(altro_handle* h, double* before, double* after, int32_t* failed);
/* Diagnostic (16-lane kernels): 16 int64 per wave (4 instances) of the last solve launch.  [0] s_memtime ticks in
 * total; [7] backward passes the wave ran in the lone-row form (one instance over the four DPP rows).  The
 * -DALTRO_PHASE_STAMPS build also fills ticks per phase -- [1] four-row backward passes, [2] closed-loop rollouts,
 * [3] open-loop rollouts, [4] Todorov gradient, [5] dual update, [6] line-search sweeps, [8] lone-row backward passes,
 * [9] first-order sweeps, [10] costate sweeps -- and how many of each the wave ran: [11] four-row passes, [12]
 * first-order sweeps, [13] costate sweeps, [14] closed-loop rollouts, [15] trial sweeps.  count = 16 * waves. */
int32_t altro_batch_get_wave_cycles(altro_handle* h, int64_t* cycles, int32_t capacity, int32_t* count);

/* Pass records of the last solve launch (16-lane kernels), 8 words per wave.  [0] (every build) backward passes that ran
 * in the pair form (two rows of the wave needed one; "no_pair" keeps the four-row form).  The shipped build also fills
 * the four-row phases by form (box-only kernels): [1] open-loop rollouts, [2] closed-loop rollouts, [3] first-order sweeps;
 * each word holds the ones that ran as the wave-uniform variant in bits 0-15 and the ones that ran in the generic form in
 * the bits above ("no_shadow": none is uniform).
 * Diagnostic builds (-DALTRO_PHASE_STAMPS) fill instead [1..3] four-row passes with 2, 3 and 4 rows needing them,
 * [4..6] their ticks and [7] the ticks of the pair passes.  count = 8 * waves; 0 for the one-wave-per-instance backend. */
int32_t altro_batch_get_wave_passes(altro_handle* h, int64_t* passes, int32_t capacity, int32_t* count);

/* ---- device-resident MPC harness (reference random_linear_problem.jl:121-139, mpc.jl:11-47).
 * The reference's MPC loop runs on the host around solve!; for a batch that lives in HBM the
 * same update sequence is provided on device so that no step crosses PCIe. */

/* Long reference trajectory Z_track (run_random_linear.jl:111-112): Xtrack [batch][Nt][n],
 * Utrack [batch][Nt-1][m].  Also installs window 0 as reference and initial trajectory
 * (gen_tracking_problem, mpc.jl:19-45). */
int32_t altro_mpc_set_track(altro_handle* h, const double* Xtrack, const double* Utrack, int32_t Nt);
/* unit-normal samples for the 1 % plant noise (random_linear_problem.jl:129): [steps][batch][n] */
int32_t altro_mpc_set_noise(altro_handle* h, const double* noise, int32_t steps);
/* Plant-noise model of the device-side MPC step: x0_i += noise_i * weights[i] * norm, with
 *   mode 0: norm = ||x0||_inf over all states (random_linear_problem.jl:129; default, weights 1/100)
 *   mode 1: norm = ||x0[group_i]||_2, groups[i] in {0,1} (simple_rocket.jl:65-71: positions with
 *           weight 1/1000, velocities with weight 1/100)
 *   mode 2: norm = 1, absolute noise (flexible_sat_mpc.jl:266: 0.0002 * randn)
 * A mode outside 0..2 or a group outside {0,1} is ALTRO_ERR_INVALID_ARG on both backends, and nothing changes. */
int32_t altro_mpc_set_noise_model(altro_handle* h, int32_t mode, const double* weights, const int32_t* groups);
/* shift = 0: the device MPC step keeps the previous solution and duals as the warm start instead of
 * shifting them by one knot (flexible_sat_mpc.jl:275-276 leaves both shift_fill! calls commented
 * out); default 1 */
int32_t altro_mpc_set_shift(altro_handle* h, int32_t shift);
/* Per-knot (LTV) dynamics for the device-resident MPC loop.  The reference re-linearises its model before
 * every solve (update_dynamics_matrices!, altro_solver.jl:5-37: model.A[k], B[k], d[k] for the knots of the
 * new horizon); for a loop that runs on the device the blocks of every step are uploaded once.  Each
 * instance (or all of them, per_instance = 0) owns `nblocks` knot blocks A [n x n], B [n x m], f [n]
 * (column-major, f may be NULL); the solve whose reference window starts at knot r -- MPC step i has
 * r = i + 1, a plain solve before the loop r = 0 -- reads block r * step_stride + k for its knot k:
 *   step_stride = 1      blocks indexed by absolute knot, like the reference track (a linearisation that
 *                        depends on time only: gait schedule, planned footholds); nblocks >= steps + N
 *   step_stride = N - 1  one full table of N - 1 blocks per step (re-linearisation about anything)
 * The plant step of altro_mpc_step_async uses knot 0 of the window that is current before the step.
 * Replaces altro_batch_set_dynamics; like it, must be the first call on an (n, m) of the 16-lane set. */
int32_t altro_mpc_set_dynamics_track(altro_handle* h, const double* A, const double* B, const double* f,
                                     int32_t nblocks, int32_t step_stride, int32_t per_instance);
/* One MPC step i (0-based), enqueued on the handle's stream, in the reference's order
 * (random_linear_problem.jl:125-139,161): x0 <- A x_1 + B u_1 + noise_i*||.||_inf/100;
 * reference window <- i+1; primal shift_fill; dual shift_fill; solve. */
int32_t altro_mpc_step_async(altro_handle* h, int32_t step);
/* The first half of that sequence only, for harnesses that keep the reference's own call order
 * around benchmark_solve! (random_linear_problem.jl:125-133): x0 <- A x_1 + B u_1 + noise_step*...,
 * reference window <- step+1.  No shift_fill and no solve: follow with altro_batch_shift_fill and
 * altro_batch_solve / altro_batch_benchmark_solve. */
int32_t altro_mpc_prepare_async(altro_handle* h, int32_t step);
/* The same for `nsteps` consecutive steps first_step .. first_step+nsteps-1 in ONE launch.
 * Instances are independent closed loops, so inside the launch each wavefront runs its own four
 * instances through all the steps without waiting for the rest of the batch; results are
 * bit-identical to nsteps calls of altro_mpc_step_async.  Per-step statistics are accumulated
 * (altro_batch_get_solve_counters); altro_batch_get_stats reports the last step; altro_mpc_set_log keeps every step's. */
int32_t altro_mpc_run_async(altro_handle* h, int32_t first_step, int32_t nsteps);
/* Per-step log of the device-resident MPC loop.  The reference's loops record every step -- X_traj[i+1] = prob_mpc.x0,
 * iters[i], status[i], costs[i] (simple_rocket.jl:137-205, rocket_landing_problem.jl:262-337, random_linear_problem.jl:166-174,
 * grasp_mpc.jl:93-94) -- while a fused launch returns the state after its LAST step; with the log on, every step of
 * altro_mpc_step_async / altro_mpc_run_async also writes one small record on the device, read back once after the run.
 * capacity_steps > 0: allocate a log of that many steps (slot = absolute step index, 0-based; every slot empty) and start
 * logging; 0: stop and free.  Default: off -- no result, counter or launch differs from a handle without a log, and results
 * do not depend on the log being on.  Synchronises the stream.  With a log set, a run whose steps reach past capacity_steps
 * is refused (ALTRO_ERR_INVALID_ARG, nothing enqueued).  Plain solves, altro_batch_benchmark_solve and
 * altro_mpc_prepare_async write nothing.  A handle that moves to the one-wave-per-instance kernel afterwards
 * (altro_batch_set_dynamics per_knot, altro_mpc_set_dynamics_track) keeps the setting.
 * ALTRO_ERR_INVALID_ARG: NULL handle, negative capacity. */
int32_t altro_mpc_set_log(altro_handle* h, int32_t capacity_steps);
/* Records of steps first_step .. first_step+nsteps-1, step-major, indexed by the caller's instance index whatever order the
 * launch ran them in; any output pointer may be NULL:
 *   x0 [nsteps][batch][n]   the initial state the step's solve started from (after plant step + noise): X_traj[i+1] of
 *                           simple_rocket.jl:164
 *   u0 [nsteps][batch][m]   first control of the trajectory the handle holds at the end of the step, i.e. the control the
 *                           NEXT plant step applies (the polished one when projected_newton = 1)
 *   iterations, iterations_outer, status [nsteps][batch] int32;  cost, c_max [nsteps][batch] double:
 *                           what altro_batch_get_stats would have returned after that step (projected_newton = 1: cost,
 *                           c_max and status after the polish, as altro_batch_get_stats reports them)
 * Running a step again overwrites its slot; a slot no step has written since altro_mpc_set_log reads iterations =
 * iterations_outer = status = -1 and NaN in every double.  Synchronises the stream.
 * ALTRO_ERR_STATE: no log is set; ALTRO_ERR_INVALID_ARG: NULL handle, range outside the capacity. */
int32_t altro_mpc_get_log(altro_handle* h, int32_t first_step, int32_t nsteps, double* x0, double* u0,
                          int32_t* iterations, int32_t* iterations_outer, int32_t* status, double* cost, double* c_max);
/* x0 currently installed: [batch][n] */
int32_t altro_batch_get_initial_state(altro_handle* h, double* x0);

/* Diagnostic switches (no Julia counterpart: Altro.jl has no scheduling to switch).  The library reads nothing from the
 * environment; a test or a measuring tool that wants one of the kernels' scheduling features off -- to show that it
 * changes no result, or to time it -- says so here.  h == NULL: for the handles THIS THREAD creates afterwards;
 * otherwise for that handle, from its next launch on.  Keys (value 0 restores the default):
 *   "no_lone", "no_pair", "no_shadow", "no_resync", "no_group", "no_reuse", "no_qz_pass", "no_mate_rank"   one scheduling feature of the 16-lane kernels off
 *   "group_mode" 0..4, "group_max_steps", "trace_wave"              slot order of a grouped launch / diagnostic builds
 *   "force_wide", "wide_compact", "wide_coop", "wide_static_mask"   read at altro_batch_create: NULL handle only
 *   "keep_gains"   the setters stop dropping the stored gains (the product then returns results from STALE gains: it
 *                  exists to show that the tests notice).  Compiled into -DALTRO_DEBUG builds only; a release build
 *                  answers ALTRO_ERR_UNSUPPORTED.
 *   "dev_via_stage" (handle only, 16-lane kernels)   altro_batch_set_initial_state_dev / _set_reference_dev copy the caller's
 *                  array into the staging buffer before the layout kernel reads it (the alternative DESIGN.md 7c measures)
 * Unknown key: ALTRO_ERR_INVALID_ARG. */
int32_t altro_debug_set(altro_handle* h, const char* key, int32_t value);

/* the handle's hipStream_t, for callers that order their own device work after a solve (see also
 * altro_batch_wait_stream / altro_batch_signal_stream below) */
int32_t altro_batch_get_stream(altro_handle* h, void** stream);


/* ---- device-pointer I/O: set and read a batch in GPU memory, stream-ordered.
 * The reference's loops hand Julia arrays to the solver on every tick (TO.set_initial_state!, update_trajectory!,
 * update_dynamics_matrices!: random_linear_problem.jl:130-133, altro_solver.jl:5-37,60-71) and read states(solver) /
 * controls(solver) back; for a plant, a learned model or a linearisation that runs on the same GPU as the batch these are
 * the same calls on arrays that never leave HBM.
 * Every `_dev` entry point takes DEVICE pointers (hipMalloc memory of the handle's device; a ROCArray, a torch tensor) to
 * FP64 / int32 arrays in exactly the layout of the host call of the same name.  It only enqueues on the handle's stream:
 * it does not synchronise, does not touch host memory, and does not allocate while the shapes are those of the previous
 * call.  The library has consumed (setters) or produced (getters) the caller's buffer once the handle's stream has passed
 * that point -- order other streams against it with altro_batch_wait_stream / altro_batch_signal_stream, or wait with
 * altro_batch_synchronize.  The library keeps no caller pointer after its stream has passed the call.
 * Validation happens before anything is enqueued or changed: every pointer must be known to the HIP runtime as device memory
 * of the handle's device (hipPointerGetAttributes) and the allocation it lies in must hold at least the bytes the call reads
 * or writes from that address on (hipMemGetAddressRange).  Otherwise -- a host pointer, memory of another device, a buffer
 * that is too short, NULL where it is not allowed, a NULL handle -- the call returns ALTRO_ERR_INVALID_ARG with a message in
 * altro_last_error (of the handle; of NULL for a NULL handle), nothing is launched and the handle is unchanged and usable.
 * A setter leaves the handle in the byte-identical device state its host twin would, a getter writes byte-identical values.
 * Not covered, on purpose (set once, or packed on the host): cost weights, duals, traces,
 * altro_mpc_set_track / _noise / _dynamics_track and the MPC log.  (Gains: altro_batch_get_gains_dev, below.) */

/* altro_batch_set_initial_state with x0 [batch][n] on the device */
int32_t altro_batch_set_initial_state_dev(altro_handle* h, const double* x0);
/* altro_batch_set_reference with Xref [batch][N][n], Uref [batch][N-1][m] on the device */
int32_t altro_batch_set_reference_dev(altro_handle* h, const double* Xref, const double* Uref);
/* altro_batch_set_initial_trajectory with X [batch][N][n] (may be NULL), U [batch][N-1][m] on the device */
int32_t altro_batch_set_initial_trajectory_dev(altro_handle* h, const double* X, const double* U);
/* altro_batch_set_dynamics with A, B, f (f may be NULL) on the device; drops the stored gains, and per_knot != 0 on an (n, m)
 * of the 16-lane set must be the first call after create, as for the host call.  On the one-wave-per-instance kernel the
 * tables are reused while the number of blocks is that of the previous call (host or device); a call that changes it, or that
 * moves the handle to that kernel, allocates and synchronises the stream once. */
int32_t altro_batch_set_dynamics_dev(altro_handle* h, const double* A, const double* B, const double* f,
                                     int32_t per_knot, int32_t per_instance);
/* altro_batch_get_states / _get_controls / _get_initial_state into device arrays X [batch][N][n], U [batch][N-1][m],
 * x0 [batch][n] */
int32_t altro_batch_get_states_dev(altro_handle* h, double* X);
int32_t altro_batch_get_controls_dev(altro_handle* h, double* U);
int32_t altro_batch_get_initial_state_dev(altro_handle* h, double* x0);
/* What an MPC consumer reads each tick (altro_solver.jl:84-88: the forces of knot 1; random_linear_problem.jl:125-129: the
 * plant step from the first control), in one kernel that reads the current trajectory directly: u0 [batch][m] the first
 * control, x1 [batch][n] the state the model predicts after it (knot 1), status, iterations [batch] int32 as
 * altro_batch_get_stats reports them.  Any pointer may be NULL (skipped).  For an instance that is inactive
 * (altro_batch_set_active) these are its LAST values: those of the last solve it took part in. */
int32_t altro_batch_get_first_knot_dev(altro_handle* h, double* u0, double* x1, int32_t* status, int32_t* iterations);

/* ---- constraint data and box bounds from device pointers: the grasp loop (grasp_mpc_helpers.jl:46-55 rewrites the torque
 * balance, the grasp-force rows and both friction cones of the shifted window on every step) and per-tick actuator limits,
 * under the rules of the device-pointer block above.
 * altro_batch_update_constraint_data_dev: A, b on the device in the layout the constraint was added with
 * ([batch][knots][p][n+m] / [batch][knots][p] when it was added with per-instance data); either may be NULL (unchanged), not
 * both.  A kernel writes the rows straight into the constraint's place in the device tables; lane assignment, knot ranges and
 * duals are untouched, the stored gains are dropped stream-ordered.  On the one-wave-per-instance kernel the tables are packed
 * on the host before the first solve and after a host altro_batch_update_constraint_data: a `_dev` call that finds them
 * unpacked packs them once, which synchronises the stream.
 * altro_batch_set_bounds_dev: zmin, zmax on the device, [n+m] (per_instance = 0) or [batch][n+m].  What
 * altro_batch_set_bounds checks on the host is checked on the DEVICE, row by row: no NaN, zmin <= zmax, the pattern of finite
 * sides that of the BOX as it was added.  A row that passes is written (the infinities of absent sides regenerated); a row that
 * fails leaves that instance's bounds exactly as they were -- with per_instance = 0 the whole table -- and adds 1 to a counter
 * on the device; the call still returns ALTRO_OK.  altro_batch_get_dev_refusals: the count since create; synchronises.
 * The first per-instance call on a handle whose bounds are one shared row changes the shape of the tables: that one call
 * reallocates and synchronises the stream once (every instance starts from the shared row).  A shared row given while the
 * tables hold one row per instance goes to every row.
 * Host and device calls may be mixed in any order and give what host calls alone give: the host copies the library keeps of
 * these tables are marked stale by a `_dev` write and read back from the device before a host call next needs them.
 * ALTRO_ERR_INVALID_ARG (nothing launched, the handle unchanged): NULL handle; unknown con_id; a BOX id given to
 * update_constraint_data_dev, a LINEAR / SOC id to set_bounds_dev; A and b both NULL; get_dev_refusals: NULL rows; what the
 * device-pointer block refuses. */
int32_t altro_batch_update_constraint_data_dev(altro_handle* h, int32_t con_id, const double* A, const double* b);
int32_t altro_batch_set_bounds_dev(altro_handle* h, int32_t con_id, const double* zmin, const double* zmax,
                                   int32_t per_instance);
int32_t altro_batch_get_dev_refusals(altro_handle* h, int64_t* rows);

/* ---- feedback policy on the device: the second rate of a two-rate controller.  The reference's quadruped loop solves at
 * 50-100 Hz (Woofer/MPCControl/altro_solver.jl) while the plant runs at 1 kHz; between two solver ticks it is driven by the
 * policy the last solve already holds, u = u_k + K_k (x - x_k), saturated at the actuator limits.
 * altro_batch_eval_policy_dev: x [batch][n] measured states, knot [batch] the knot of the current horizon each instance is
 * at (NULL: knot 0 for every instance), u [batch][m] output, fb [batch] output (may be NULL), all on the device under the rules
 * of the device-pointer block (validated before anything is enqueued, stream-ordered behind the solve that wrote the gains, no
 * host synchronisation, no allocation; NULL x or u is refused).  For instance b at k = knot[b], for every control a
 *     u[b][a] = u_k[a] + sum_j K_k[a][j] (x[b][j] - x_k[j])
 * with (x_k, u_k) the trajectory the handle holds (altro_batch_get_states / _get_controls: the polished one when
 * projected_newton = 1) and K_k the matrix altro_batch_get_gains returns.  The feedforward term d is NOT applied: the
 * trajectory already contains the accepted step.  The order of the sum over j is fixed per backend (16-lane kernels: the
 * products sit on their state lanes and are added by an xor butterfly over the 16 lanes, strides 8, 4, 2, 1; one-wave-per-
 * instance kernels: fused multiply-adds for j = 0 .. n-1 in turn) and the nominal control is added last, so x = x_k returns
 * u_k bit for bit.
 * clamp = 1 on a handle with a BOX, k inside the BOX's knot range: u[b][a] <- min(max(u[b][a], zmin[n+a]), zmax[n+a]) with
 * instance b's row of bounds as the solve kernels see it at that point of the stream (altro_batch_set_bounds(_dev) included);
 * infinite sides do nothing.  clamp = 0: no saturation.
 * fb[b] = 1: feedback was applied.  0: instance b holds no valid stored gains -- before its first solve, after any setter
 * that drops the stored gains, after altro_batch_restart_instances, or when its last backward pass was regularised or failed
 * -- and u[b] = u_k (clamped if asked).  -1: knot[b] is outside 0 .. N-2; row u[b] is not written (nothing is counted in
 * altro_batch_get_dev_refusals).  The call is not masked: an instance the active mask or the clock leaves out answers from its
 * last solve, as in altro_batch_get_first_knot_dev.
 * altro_batch_eval_policy: the same with host arrays, through the handle's staging buffer; synchronises; writes the bytes the
 * `_dev` call writes.  An out-of-range knot is found on the host instead: ALTRO_ERR_INVALID_ARG, nothing enqueued.
 * altro_batch_get_gains_dev: altro_batch_get_gains into device arrays K [batch][N-1] blocks of m x n (column-major),
 * d [batch][N-1][m], byte-identical to the host call (d = 0 after a costate-sweep confirmation included); either may be NULL,
 * not both.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle unchanged): NULL handle, NULL x or u, K and d both NULL; _dev: what the
 * device-pointer block refuses. */
int32_t altro_batch_eval_policy_dev(altro_handle* h, const double* x, const int32_t* knot, int32_t clamp, double* u, int32_t* fb);
int32_t altro_batch_eval_policy(altro_handle* h, const double* x, const int32_t* knot, int32_t clamp, double* u, int32_t* fb);
int32_t altro_batch_get_gains_dev(altro_handle* h, double* K, double* d);

/* ---- caller-supplied trajectories scored on the device: rollout!(prob) (random_linear_problem.jl:30,
 * rocket_landing_problem.jl:183, run_simple_rocket.jl:63,87, grasp_problem.jl:104), cost(prob_mpc) / cost(prob_mpc.obj, Z)
 * (simple_rocket.jl:198-200: the plain objective, of the solver's trajectory and of ECOS's), max_violation(...) and
 * dynamics_violation(prob, X, U) (simple_rocket.jl:191,208-216).  A caller that holds several candidate control sequences per
 * instance -- the shifted previous solution, the reference controls, a learned guess -- has them scored against the problem
 * the next altro_batch_solve would see at that point of the stream.  (To have the best of them chosen and installed as the
 * warm start in the same call, use altro_batch_warm_start_dev below: it scores with the arithmetic of this call.)
 * altro_batch_evaluate_dev: every pointer is a device pointer under the rules of the device-pointer block (validated before
 * anything is enqueued, stream-ordered, no host synchronisation, no caller pointer kept).  ncand >= 1 candidates per instance:
 *   U      [batch][ncand][N-1][m]
 *   J, c_max, defect   [batch][ncand] outputs; any may be NULL, not all
 * Rollout form (X == NULL): x_0 = x0[b] (x0 [batch][n]; NULL: the initial state the handle holds), x_{k+1} = A_k x_k + B_k u_k
 *   + f_k; Xout [batch][ncand][N][n] (may be NULL) receives the states; defect receives +0.0.  With Xout == NULL the states go
 *   to a grow-only workspace of the handle: the one allocation, on the first call or when batch * ncand grows.
 * Given form (X [batch][ncand][N][n] not NULL): (X, U) are scored as they are; x0 and Xout must be NULL;
 *   defect[b][c] = max_k max_i |A_k x_k + B_k u_k + f_k - x_{k+1}|_i, the maximum over ALL knots.  (The reference's
 *   dynamics_violation overwrites its `err` in every pass of the loop and so returns the last knot's value only; the maximum
 *   is what it evidently means.)
 * Own trajectory (U == NULL): ncand must be 1 and X, x0, Xout NULL; the given form on the trajectory the handle holds
 *   (altro_batch_get_states / _get_controls): cost(prob_mpc) and max_violation(solver) without the augmented-Lagrangian terms.
 * J = sum_{k<N-1} dt (1/2 dx' Q dx + 1/2 du' R du) + 1/2 dx_N' Qf dx_N with dx, du the distance to the reference window the
 *   handle holds (under an episode clock: the instance's own window) and the instance's own weights when they are per
 *   instance; no AL terms.  The dynamics are the blocks of that window (altro_mpc_set_dynamics_track: kref * step_stride + k).
 * c_max = the maximum over every constraint and every knot of its range of the violation (the oracle's con_violation): BOX
 *   max(0, z - zmax, zmin - z) over finite sides, state columns only at knot N-1; LINEAR |v| for an equality row, max(0, v)
 *   for an inequality row; SOC ||Proj(v) - v||_inf.  The data is the device tables as the solve kernels address them, with
 *   whatever altro_batch_set_bounds(_dev) / altro_batch_update_constraint_data(_dev) wrote earlier on the stream.
 * No masking, no clamping, no status: an instance the active mask or the clock leaves out is scored like any other; a
 * rollout that overflows puts Inf or NaN into its own outputs and nothing else.  Nothing the library owns changes: every later
 * solve, MPC step, counter and log record is bit-identical to a handle that never made the call (the stored gains stay).
 * Results are a function of the call's inputs: candidate c of instance b gets the bytes it would get alone (ncand = 1) or on a
 * batch-1 handle holding instance b's data, and the rollout form with Xout followed by the given form on (Xout, U) returns the
 * same bytes of J and c_max (one scoring kernel reads states from memory in both forms).  Summation orders: csrc/evaluate.h.
 * One caveat to "no host synchronisation, no allocation": like a solve, the call first packs constraint tables that a HOST
 * altro_batch_add_constraint / altro_batch_update_constraint_data has left unpacked -- host copies, and before the first solve a
 * reallocation of the tables and of the (still zero) duals of the constraint rows.  It is exactly what the next solve would do
 * first, it happens only after such a host-side edit, and it is a no-op otherwise (the `_dev` setters never leave tables unpacked).
 * altro_batch_evaluate: the same with host arrays, through the handle's staging buffer (grown if needed); synchronises; writes
 * the bytes the `_dev` call writes.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle unchanged and usable): NULL handle; ncand < 1; U == NULL with ncand != 1
 * or with X, x0 or Xout; X together with x0 or Xout; J, c_max and defect all NULL; _dev: what the device-pointer block
 * refuses.  ALTRO_ERR_STATE: dynamics, cost or reference not set, or the window runs past the stored reference.  All indexing
 * is size_t: the 4 GiB rule of the handle's own arrays does not apply to the caller's. */
int32_t altro_batch_evaluate_dev(altro_handle* h, int32_t ncand, const double* U, const double* X, const double* x0, double* J,
                                 double* c_max, double* defect, double* Xout);
int32_t altro_batch_evaluate(altro_handle* h, int32_t ncand, const double* U, const double* X, const double* x0, double* J,
                             double* c_max, double* defect, double* Xout);

/* ---- gradient of a candidate's merit with respect to its controls and its initial state, on the device.  The calls above say
 * how good a control sequence is for the problem the next solve will see; this one says which way it should move: what a
 * trained warm-start generator needs to learn against the handle's own cost and constraints, and what a few gradient steps on
 * the candidates of altro_batch_warm_start_dev need, without the host.  The rollout form of altro_batch_evaluate_dev only.
 * altro_batch_evaluate_grad_dev: every pointer is a device pointer under the rules of the device-pointer block (validated before
 * anything is enqueued, stream-ordered, no host synchronisation, no caller pointer kept).  ncand >= 1 candidates per instance:
 *   U      [batch][ncand][N-1][m]   required
 *   x0     [batch][n]               NULL: the initial state the handle holds
 *   rho    >= 0, finite             the weight of P in the merit M = J + rho P (the library does not form M)
 *   J, P   [batch][ncand]           outputs
 *   gU     [batch][ncand][N-1][m]   dM/dU
 *   gx0    [batch][ncand][n]        dM/dx0
 *   Xout   [batch][ncand][N][n]     the states; NULL: they go to the grow-only workspace altro_batch_evaluate_dev uses (the one
 *                                   allocation, on the first call or when batch * ncand grows)
 * Any of J, P, gU, gx0 may be NULL, not all four; which of them are NULL changes no other output.
 * The window, the dynamics blocks, the weights, the bounds and the constraint tables are those altro_batch_evaluate_dev sees at
 * that point of the stream (under an episode clock the instance's own window); like it the call first packs constraint tables
 * a HOST edit has left unpacked.
 *   X (Xout) the rollout of altro_batch_evaluate_dev: the same bytes.
 *   J      the plain tracking cost of altro_batch_evaluate_dev: the same bytes.
 *   P      = 1/2 sum r^2 over every constraint, every knot of its range and every row, r the signed distance of the row to its
 *          feasible set: BOX finite side max(0, z - zmax), max(0, zmin - z), state columns only at knot N-1; LINEAR v for an
 *          equality row, max(0, v) for an inequality row; SOC the vector v - Proj(v) (0 inside the cone, v in the polar cone,
 *          ((1 - c) s, t - c |s|) with c = (1 + t / |s|) / 2 otherwise).  It is the augmented-Lagrangian penalty of the solver
 *          with zero multipliers and unit penalty.
 *   gU, gx0   the gradient of M by one costate sweep, with c_k = sum_rows a_r r_r (BOX: r on the element, signed), e = z - zref
 *          and the weights as altro_batch_evaluate_dev applies them (wd = dt Q, dt R; wf = Qf):
 *            lambda_{N-1} = wf e_x + rho c_x;  gU_k = wd e_u + rho c_u + B_k' lambda_{k+1};
 *            lambda_k = wd e_x + rho c_x + A_k' lambda_{k+1};  gx0 = lambda_0.
 *          With rho == 0 no constraint term enters the gradient, not even as a product with zero; P is still computed.
 *          M is piecewise quadratic and once differentiable; where a row value sits exactly on its kink the gradient is that of
 *          the side the comparison above picks.
 * No masking, no status; a NaN stays a NaN.  Nothing the library owns changes.  Candidate c of instance b gets the bytes it would
 * get alone (ncand = 1) or on a batch-1 handle holding instance b's data; x0 == NULL and the handle's state passed explicitly
 * give the same bytes.  Summation orders: csrc/evaluate_grad.h.
 * altro_batch_evaluate_grad: the same with host arrays, through the handle's staging buffer; synchronises; writes the bytes the
 * `_dev` call writes.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle unchanged and usable): NULL handle; NULL U; ncand < 1; rho negative, NaN
 * or infinite; J, P, gU and gx0 all NULL; _dev: what the device-pointer block refuses.  ALTRO_ERR_STATE: as
 * altro_batch_evaluate_dev. */
int32_t altro_batch_evaluate_grad_dev(altro_handle* h, int32_t ncand, const double* U, const double* x0, double rho, double* J,
                                      double* P, double* gU, double* gx0, double* Xout);
int32_t altro_batch_evaluate_grad(altro_handle* h, int32_t ncand, const double* U, const double* x0, double rho, double* J, double* P,
                                  double* gU, double* gx0, double* Xout);

/* ---- the solver's own augmented Lagrangian L_A(U; lambda, mu) of a control sequence, on the device: the function a solve
 * minimises, with the multipliers the handle holds (altro_batch_get_duals) and the penalty of every instance
 * (altro_batch_get_penalty), where altro_batch_evaluate_grad_dev scores a stand-in with zero multipliers.  Three uses: the
 * stationarity residual dL_A/dU at the trajectory a solve left (an optimality certificate: U == NULL); by the envelope theorem
 * the derivative of the optimal cost with respect to a problem datum is the partial derivative of L_A at the optimum, so the
 * same sweep gives dJ-star/dx0, the derivatives with respect to the reference and the cost weights and the shadow prices of the
 * box bounds -- exact up to that stationarity residual, no KKT solve; and with them a differentiable layer over x0 and the
 * reference.
 * altro_batch_evaluate_al_dev: every pointer is a device pointer under the rules of the device-pointer block (validated before
 * anything is enqueued, stream-ordered, no host synchronisation, no caller pointer kept).  ncand >= 1 candidates per instance:
 *   U      [batch][ncand][N-1][m]   NULL: the controls the handle holds (ncand must be 1)
 *   x0     [batch][n]               NULL: the initial state the handle holds
 *   out    a struct of output pointers, each may be NULL, not all of those other than Xout:
 *     LA, J        [batch][ncand]
 *     gU           [batch][ncand][N-1][m]   dL_A/dU
 *     gx0          [batch][ncand][n]        dL_A/dx0
 *     gXref        [batch][ncand][N][n]     dL_A/dXref_k = -(w e_x)_k (w = dt Q, Qf at knot N-1): the cost term only
 *     gUref        [batch][ncand][N-1][m]   dL_A/dUref_k = -(dt R e_u)_k
 *     gQ, gQf      [batch][ncand][n]        dt/2 sum_{k<N-1} e_x^2;  e_{x,N-1}^2 / 2   (the arguments of altro_batch_set_tracking_cost)
 *     gR           [batch][ncand][m]        dt/2 sum e_u^2
 *     gzmin, gzmax [batch][ncand][n+m]      + sum_k g_lo;  - sum_k g_hi; 0 on infinite sides
 *     Xout         [batch][ncand][N][n]     the states; NULL: the grow-only workspace altro_batch_evaluate_dev uses
 *   The data derivatives are partial derivatives of L_A per (instance, candidate), also where the handle shares the datum
 *   across the batch (the derivative with respect to a shared datum is their sum).
 * Which pointers are NULL changes no other output.  X (Xout) and J are altro_batch_evaluate_dev's bytes.  With e = z - zref:
 *   L_A = J + sum over every constraint, every knot of its range and every row:
 *     BOX finite side, value c = z - zmax resp. zmin - z (state columns only at knot N-1), and LINEAR inequality row,
 *     c = a'z + b, dual l:   l c + [a] mu c^2 / 2 with a = (c >= 0) | (l > 0);   g = l + [a] mu c
 *     LINEAR equality row:   the same with a = true
 *     SOC, v = A z + b, duals l:   (|y|^2 - |l|^2) / (2 mu), y = Proj_K(l - mu v)
 *   pulled back to z as + g on the element (upper side), - g (lower side), a_r g (row), - A' y (cone): c_k their sum, then
 *     lam_{N-1} = Qf e_x + c_x;  gU_k = dt R e_u + c_u + B_k' lam_{k+1};  lam_k = dt Q e_x + c_x + A_k' lam_{k+1};  gx0 = lam_0.
 *   It is the oracle's con_cost / cost_expansion.  L_A is once differentiable everywhere: at c == 0 with l == 0 both sides give
 *   the same g.  Duals on infinite box sides are not read.
 * The window, the dynamics, the weights, the bounds and the constraint tables are those altro_batch_evaluate_dev sees at that
 * point of the stream (under an episode clock the instance's own window).  No masking, no status; a NaN stays a NaN.  Nothing
 * the library owns changes.  Candidate c of instance b gets the bytes it would get alone or on a batch-1 handle holding
 * instance b's data; x0 == NULL / U == NULL and the held state / altro_batch_get_controls_dev's array passed explicitly give
 * the same bytes.  Summation orders: csrc/evaluate_al.h.
 * altro_batch_evaluate_al: the same with host arrays, through the handle's staging buffer; synchronises; the same bytes.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle unchanged and usable): NULL handle; NULL out; ncand < 1; U NULL with
 * ncand != 1; every output other than Xout NULL; _dev: what the device-pointer block refuses.  ALTRO_ERR_STATE: as
 * altro_batch_evaluate_dev.
 * altro_batch_get_penalty(_dev): mu [batch], the penalty every instance holds (1 on a new or restarted handle; after a solve
 * the penalty its last inner solve ran with); _dev is stream-ordered, the host form synchronises. */
typedef struct altro_al_out {
  double *LA, *J, *gU, *gx0, *gXref, *gUref, *gQ, *gQf, *gR, *gzmin, *gzmax, *Xout;
} altro_al_out;
int32_t altro_batch_evaluate_al_dev(altro_handle* h, int32_t ncand, const double* U, const double* x0, const altro_al_out* out);
int32_t altro_batch_evaluate_al(altro_handle* h, int32_t ncand, const double* U, const double* x0, const altro_al_out* out);
int32_t altro_batch_get_penalty_dev(altro_handle* h, double* mu);
int32_t altro_batch_get_penalty(altro_handle* h, double* mu);

/* ---- sensitivity of the SOLUTION of the last solve, through the stored gains, on the device.  Inside the
 * active set and penalty of the last backward pass the problem the solve minimised is an LQ problem and the stored gains are
 * its exact Riccati solution; the derivative of its minimiser (X*, U*) with respect to x0 and the reference is two sweeps with
 * what the solve left in memory: the gains K_k (altro_batch_get_gains), the factors Quu_k = L D L'
 * (altro_batch_get_gain_factors_dev) and the dynamics blocks (A_k, B_k) of the window altro_batch_evaluate_dev sees at that
 * point of the stream.  For g = (gx [N][n], gu [N-1][m]) define  Lin(g, xi_0) -> (s_0, xi, nu):
 *   backward  s_{N-1} = gx_{N-1};  k = N-2 .. 0:  q_x = gx_k + A_k' s_{k+1},  q_u = gu_k + B_k' s_{k+1},
 *             d_k = -Quu_k^-1 q_u,  s_k = q_x + K_k' q_u
 *   forward   xi_0 given;  k = 0 .. N-2:  nu_k = K_k xi_k + d_k,  xi_{k+1} = A_k xi_k + B_k nu_k
 * With w = dt Q (Qf at knot N-1) and dt R as altro_batch_evaluate_dev applies them (per instance where the handle holds them so):
 *   altro_batch_solution_vjp_dev (reverse mode): seeds gX = dl/dX*, gU = dl/dU*;  (s_0, xi, nu) = Lin((gX, gU), 0);
 *     out->gx0 = s_0,  out->gXref_k = -(w xi)_k,  out->gUref_k = -(dt R nu)_k
 *   altro_batch_solution_jvp_dev (forward mode): tangents vx0, vXref, vUref;  (., xi, nu) = Lin((-w vXref, -dt R vUref), vx0);
 *     dX = xi,  dU = nu
 * nseed >= 1 seeds per instance.  gX, vXref, dX, gXref: [batch][nseed][N][n];  gU, vUref, dU, gUref: [batch][nseed][N-1][m];
 * vx0, gx0: [batch][nseed][n];  fb: [batch] (may be NULL).  A NULL input is zero; any output may be NULL, not all of them.
 * The result is the exact derivative of the minimiser of the augmented Lagrangian at the multipliers and the penalty of the
 * stored pass, inside its active set; it differs from the derivative of the constrained optimum by O(1 / mu) on active rows.
 * For conic handles the gains are those of the last quadratic model (soc_second_order as set).
 * fb[b] = 1 iff altro_batch_eval_policy_dev would report valid gains AND the stored pass ran without regularisation;
 * otherwise fb[b] = 0 and every output row of that instance is a quiet NaN.  No masking, no clamp, no status; a NaN stays a
 * NaN.  Nothing the library owns changes: the stored gains stay, and every later solve, step, counter and log record is that of
 * a handle that never made the call.  Row (b, s) gets the bytes it would get alone (nseed = 1) or on a batch-1 handle holding
 * instance b's data; which outputs are NULL changes no other output.  Summation orders: csrc/sensitivity.h.
 * The _dev forms follow the rules of the device-pointer block (validated before anything is enqueued, stream-ordered behind
 * the solve that wrote the gains, no host synchronisation, no caller pointer kept); the only allocation is a grow-only
 * workspace of batch * nseed * (N-1) * m doubles that carries d_k between the sweeps.  The host twins go through the staging
 * buffer, synchronise and write the same bytes.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle unchanged and usable): NULL handle; nseed < 1; vjp: gX and gU both NULL,
 * out NULL or its three members all NULL; jvp: vx0, vXref and vUref all NULL, or dX and dU both NULL; _dev: what the
 * device-pointer block refuses.  ALTRO_ERR_STATE: as altro_batch_evaluate_dev.  ALTRO_ERR_UNSUPPORTED (nothing enqueued): the
 * one-wave-per-instance kernels with m > 16 keep no factors of Quu, so what needs d_k is refused there -- out->gXref,
 * out->gUref, vXref, vUref; the x0-only paths (gx0 alone; vx0 alone) need K alone and work.
 * altro_batch_get_gain_factors_dev: F [batch][N-1][m][m] on the device, stream-ordered, in the layout of
 * altro_batch_get_gain_factors: (a, a) = 1 / D_a, (a, c < a) = L[a][c], 0 above.  16-lane kernels: that call's bytes;
 * one-wave-per-instance kernels: m <= 16 unpacked from the packed triangles, m > 16 ALTRO_ERR_UNSUPPORTED. */
typedef struct altro_sens_out {
  double *gx0, *gXref, *gUref;
} altro_sens_out;
int32_t altro_batch_solution_vjp_dev(altro_handle* h, int32_t nseed, const double* gX, const double* gU, const altro_sens_out* out,
                                     int32_t* fb);
int32_t altro_batch_solution_vjp(altro_handle* h, int32_t nseed, const double* gX, const double* gU, const altro_sens_out* out,
                                 int32_t* fb);
int32_t altro_batch_solution_jvp_dev(altro_handle* h, int32_t nseed, const double* vx0, const double* vXref, const double* vUref,
                                     double* dX, double* dU, int32_t* fb);
int32_t altro_batch_solution_jvp(altro_handle* h, int32_t nseed, const double* vx0, const double* vXref, const double* vUref,
                                 double* dX, double* dU, int32_t* fb);
int32_t altro_batch_get_gain_factors_dev(altro_handle* h, double* F);

/* ---- sensitivity of the SOLUTION of the last solve with respect to the cost weights, the box bounds and the dynamics, and the
 * active set of the stored pass, on the device: what training a cost or a model through the solver needs.  With
 * box terms only, the Hessian of the augmented Lagrangian inside the active set of the stored backward pass is diagonal,
 *   hz_{k,j} = w_{k,j} + mu_p [upper side of element j in the set at knot k] + mu_p [lower side],   mu_p the penalty of that pass,
 * so next to the two sweeps of altro_batch_solution_vjp_dev, (s_0, xi, nu) = Lin((gX, gU), 0), one more backward sweep gives the
 * costate of the sensitivity problem, and no value Hessian is needed.  With (x_k, u_k) the trajectory the handle holds,
 * e = z - zref, dz = (xi, nu), and lam_k the costate of altro_batch_evaluate_al_dev at U == NULL on that trajectory
 * (lam_{N-1} = Qf e_x + c_x, lam_k = dt Q e_x + c_x + A_k' lam_{k+1}):
 *   dlam_{N-1} = gX_{N-1} + hz_{N-1} xi_{N-1};   dlam_k = gX_k + hz_k xi_k + A_k' dlam_{k+1},  k = N-2 .. 0
 *   gQ_j  = dt sum_{k<N-1} xi_k[j] e_k[j]      gQf_j = xi_{N-1}[j] e_{N-1}[j]      gR_a = dt sum_k nu_k[a] e_{u,k}[a]
 *   gzmax_e = -mu_p sum_k [upper side of e in the set at k] dz_k[e]      gzmin_e = -mu_p sum_k [lower side ..] dz_k[e]
 *   gA_k = lam_{k+1} xi_k' + dlam_{k+1} x_k'      gB_k = lam_{k+1} nu_k' + dlam_{k+1} u_k'      gf_k = dlam_{k+1}
 * gQ, gQf, gR are derivatives with respect to the ARGUMENTS of altro_batch_set_tracking_cost (they carry dt, as those of
 * altro_al_out); gzmin, gzmax are +0 on sides that are not in the set (infinite sides never are).  As for
 * altro_batch_solution_vjp_dev the result is the exact derivative of the minimiser of the augmented Lagrangian at the
 * multipliers, the penalty and the active set of the stored pass; its distance to the derivative of the constrained optimum
 * has not been measured.  There is no forward mode: the response of the solution to a tangent of the dynamics needs the
 * value Hessians S_k; altro_batch_cost_to_go_dev (mode 1) now computes them, the forward mode itself is still not built.
 * altro_batch_solution_vjp_data_dev: nseed >= 1 seeds per instance, gX [batch][nseed][N][n], gU [batch][nseed][N-1][m] (a NULL
 * one is zero, not both); out a struct of output pointers, each may be NULL, not all:
 *     gQ, gQf       [batch][nseed][n]            gR   [batch][nseed][m]            gzmin, gzmax   [batch][nseed][n+m]
 *     per_knot = 0: gA [batch][nseed][n x n], gB [batch][nseed][n x m], gf [batch][nseed][n]: the blocks summed over the knots --
 *       the derivative with respect to a time-invariant block; on a handle with per-knot dynamics, with respect to a
 *       perturbation common to all blocks of the window
 *     per_knot = 1: the same blocks per knot, [batch][nseed][N-1][..]
 *   Matrices are column-major, as altro_batch_set_dynamics takes them.  Derivatives are per (instance, seed), also where the
 *   handle shares the datum across the batch (the derivative with respect to a shared datum is their sum).  The window, the
 *   dynamics blocks, the weights, the bounds and the duals are those altro_batch_evaluate_al_dev sees at that point of the stream.
 * altro_batch_get_gain_active_set_dev: codes [batch][N][n+m] bytes: bit 0 = the upper side of the element entered the Hessian of
 * the stored pass at that knot, bit 1 = the lower side (control columns at knot N-1: 0); mu_pass [batch]: the penalty of that
 * pass.  Either may be NULL, not both; fb [batch] may be NULL.  codes is the region of the piecewise-affine solution map the
 * instance is in.
 * fb[b] = 1 iff altro_batch_solution_vjp_dev would report 1 AND the penalty the instance holds (altro_batch_get_penalty) equals
 * the penalty of the stored pass; otherwise fb[b] = 0 and every output row of the instance is a quiet NaN (the getter: codes 0,
 * mu_pass NaN).  Which outputs are NULL changes no other output and not fb.  No masking, no status; a NaN stays a NaN.  Nothing
 * the library owns changes: the stored gains stay, and the next solve is that of a handle that never made the call.  Row (b, s)
 * gets the bytes it would get alone (nseed = 1) or on a batch-1 handle holding instance b's data.  Summation orders:
 * csrc/sensitivity_data.h.  The _dev forms follow the rules of the device-pointer block (validated before anything is
 * enqueued, stream-ordered, no host synchronisation, no caller pointer kept); the only allocation is the grow-only workspace
 * of altro_batch_evaluate_dev, batch * nseed * ((N-1) m [+ N (n+m) with gA, gB or gf]) doubles.  The host twins go through the
 * staging buffer, synchronise and write the same bytes.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle unchanged and usable): NULL handle; nseed < 1; gX and gU both NULL; out
 * NULL or all eight members NULL; per_knot not 0 or 1; the getter: codes and mu_pass both NULL; _dev: what the device-pointer
 * block refuses.  ALTRO_ERR_STATE: as altro_batch_evaluate_dev.  ALTRO_ERR_UNSUPPORTED (nothing enqueued): gzmin, gzmax, gA, gB,
 * gf and the getter on a handle that holds a LINEAR or SOC constraint (the Hessian inside the set is not diagonal, and the
 * conic 16-lane kernels keep no exact set) or on the 16-lane kernels with N > 128 (the exact set covers 128 knots); every
 * output on the one-wave-per-instance kernels with m > 16 (all need d_k, no factors of Quu are kept there).  gQ, gQf, gR work
 * wherever the full altro_batch_solution_vjp_dev works, conic handles included. */
typedef struct altro_sens_data_out {
  double *gQ, *gQf, *gR, *gzmin, *gzmax, *gA, *gB, *gf;
} altro_sens_data_out;
int32_t altro_batch_solution_vjp_data_dev(altro_handle* h, int32_t nseed, const double* gX, const double* gU, int32_t per_knot,
                                          const altro_sens_data_out* out, int32_t* fb);
int32_t altro_batch_solution_vjp_data(altro_handle* h, int32_t nseed, const double* gX, const double* gU, int32_t per_knot,
                                      const altro_sens_data_out* out, int32_t* fb);
int32_t altro_batch_get_gain_active_set_dev(altro_handle* h, uint8_t* codes, double* mu_pass, int32_t* fb);
int32_t altro_batch_get_gain_active_set(altro_handle* h, uint8_t* codes, double* mu_pass, int32_t* fb);

/* ---- the quadratic cost-to-go of the stored policy: value Hessians, gradients and values, on the device.  Around the
 * trajectory (xbar, ubar) the handle holds, with K_k the matrix altro_batch_get_gains returns and M_k = A_k + B_k K_k,
 *   V_k(x) = v_k + p_k' (x - xbar_k) + 1/2 (x - xbar_k)' P_k (x - xbar_k)
 *   P_{N-1} = Hx_{N-1}                 P_k = Hx_k + K_k' Hu_k K_k + M_k' P_{k+1} M_k
 *   p_{N-1} = lx_{N-1}                 p_k = lx_k + K_k' lu_k + M_k' p_{k+1}
 *   v_{N-1} = the value of knot N-1    v_k = the value of knot k + v_{k+1},      k = N-2 .. 0
 * the transpose of the recursion of altro_batch_propagate_covariance_dev.  e = z - zref, w the weights as
 * altro_batch_evaluate_dev applies them (dt Q, dt R; Qf at knot N-1).
 * mode = 0, the plain cost: H = diag(w), l = w e, the value of a knot its term of J of altro_batch_evaluate_dev.  The model is
 *   exact: for the unclamped loop of altro_batch_simulate_policy_dev started at xbar_0 + d with w = NULL,
 *   J = v_0 + p_0' d + 1/2 d' P_0 d, and v_0 is J of the held trajectory.  1/2 tr(P_0 Sigma0) + 1/2 sum_{k=1..N-1} tr(P_k W) is
 *   the dJ of altro_batch_propagate_covariance_dev, for every (Sigma0, W) at once.  fb as altro_batch_eval_policy_dev; with 0
 *   the loop is open, K = 0.  Works on every handle: conic, m > 16, any N.
 * mode = 1, the augmented Lagrangian inside the active set of the stored pass, box terms only: H = diag(hz),
 *   hz = w + mu_p [upper side in the set] + mu_p [lower side] (the codes and mu_pass of altro_batch_get_gain_active_set_dev);
 *   l the local term of altro_batch_evaluate_al_dev at U == NULL, w e + g_hi - g_lo with the duals and the penalty the handle
 *   holds; the value of a knot its terms of L_A as that call values them.  P_k is the value Hessian of the LQ problem the stored
 *   gains solve, P_0 the Hessian of the optimal L_A with respect to x0 inside that set.  fb as
 *   altro_batch_get_gain_active_set_dev; with 0 every output row of the instance is a quiet NaN.
 * out: a struct of output pointers, each may be NULL, not all:
 *     P0 [batch][n][n]   p0 [batch][n]   v0 [batch]   P [batch][N][n][n]   p [batch][N][n]   v [batch][N]
 *   Matrices are row-major, as computed and not re-symmetrised (as Sout).  fb [batch] may be NULL.  Which outputs are NULL
 *   changes no other output and not fb.
 * The call sees the window, the dynamics blocks, the weights, the bounds and the duals altro_batch_evaluate_al_dev sees at that
 * point of the stream (episode clock included).  No masking, no clamp; a NaN stays in its instance.  Instance b gets the bytes it
 * would get on a batch-1 handle.  Nothing the library owns changes, and the next solve is that of a handle that never made the
 * call.  The call allocates nothing: P lives in registers or LDS.  Constraint tables a host edit left unpacked are packed first,
 * as by the sibling calls.  Summation orders: csrc/cost_to_go.h.  The _dev form follows the rules of the device-pointer block;
 * the host twin goes through the staging buffer, synchronises and writes the same bytes.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle usable): NULL handle; out NULL or all six members NULL; mode not 0 or 1;
 * _dev: what the device-pointer block refuses.  ALTRO_ERR_STATE: as altro_batch_propagate_covariance_dev.
 * ALTRO_ERR_UNSUPPORTED (nothing enqueued): mode 1 exactly where altro_batch_get_gain_active_set_dev answers so -- a handle with
 * a LINEAR or SOC constraint, and the 16-lane kernels with N > 128. */
typedef struct altro_ctg_out {
  double *P0, *p0, *v0, *P, *p, *v;
} altro_ctg_out;
int32_t altro_batch_cost_to_go_dev(altro_handle* h, int32_t mode, const altro_ctg_out* out, int32_t* fb);
int32_t altro_batch_cost_to_go(altro_handle* h, int32_t mode, const altro_ctg_out* out, int32_t* fb);

/* ---- warm start from the best of several candidates, chosen on the device.  The closed loops of the reference start every
 * solve from ONE guess (the shifted previous solution: random_linear_problem.jl:136, simple_rocket.jl:160); a loop that also
 * holds the reference controls and a learned or sampled guess wants the best of them, and the 20-step launch lasts as long as
 * its hardest instance.  One call rolls out and scores every candidate, chooses per instance and installs the winner as the
 * initial trajectory of the next solve.
 * altro_batch_warm_start_dev: every pointer is a device pointer under the rules of the device-pointer block (validated before
 * anything is enqueued, stream-ordered on the handle's stream, no host synchronisation, no caller pointer kept).
 *   U        [batch][ncand][N-1][m], ncand >= 1
 *   rho      >= 0, finite
 *   include_current   0 or 1: the controls the handle holds (altro_batch_get_controls) compete as one more candidate, the
 *            incumbent, in the LAST column (index ncand)
 *   chosen   [batch] int32 output, may be NULL
 *   J, c_max [batch][ncand + include_current] outputs, may be NULL
 * Scoring: every candidate is rolled out from the initial state the handle holds at that point of the stream (there is no x0
 *   argument: the plane installed must be consistent with the handle) and scored exactly as the rollout form of
 *   altro_batch_evaluate_dev scores it -- the same window (kref, or the instance's own under an episode clock), dynamics
 *   blocks, weights, device tables and summation orders: J[b][c] and c_max[b][c] are the bytes that call writes for the same
 *   U, and the incumbent's are those of altro_batch_evaluate_dev on the output of altro_batch_get_controls_dev.  The states
 *   never reach memory (csrc/warm_start.h): no workspace grows with ncand * N * n; with J or c_max NULL the merits go to a
 *   grow-only workspace of 2 * batch * (ncand + include_current) doubles, the one allocation.
 * Choice: merit = fma(rho, c_max, J), one rounding (rho = 0: the plain cost).  best = +Inf, chosen = -1; the incumbent is
 *   visited first if included, then c = 0 .. ncand-1 in turn, and a candidate takes over only if merit < best.  Hence the
 *   incumbent wins ties, among candidates the lowest index wins ties, and a NaN or +Inf merit never wins.
 *   chosen[b] = 0 .. ncand-1: that candidate; ncand: the incumbent; -1: nothing had a finite merit, nothing of instance b is
 *   written; -2: the active mask leaves instance b out.
 * Install: plane cur[b] receives the winner's controls and its rolled-out states and is then byte-identical to what
 *   altro_batch_set_initial_trajectory_dev(X_w, U_w) leaves, X_w the Xout of altro_batch_evaluate_dev for that candidate --
 *   also when the incumbent wins (its states are re-rolled from the handle's x0, its controls stay).  Nothing else the
 *   library owns changes: duals, penalty, statistics, counters, log, clocks and the stored gains with their validity stay.
 * Mask: the call transforms the trajectory like altro_batch_shift_fill and is masked like it: while altro_batch_set_active is
 *   in force nothing the library owns changes for an inactive instance and chosen[b] = -2; its rows of J / c_max are still
 *   written (scoring is not masked, as in altro_batch_evaluate_dev).  The episode clock only selects the window.
 * Like a solve and like altro_batch_evaluate_dev the call first packs constraint tables a HOST edit has left unpacked.
 * altro_batch_warm_start: the same with host arrays, through the handle's staging buffer (grown if needed); synchronises;
 * writes the bytes the `_dev` call writes.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle unchanged and usable): NULL handle or NULL U; ncand < 1; rho negative,
 * NaN or infinite; include_current not 0 or 1; _dev: what the device-pointer block refuses.  ALTRO_ERR_STATE: dynamics, cost
 * or reference not set, or the window runs past the stored reference.  Caller arrays are indexed with size_t. */
int32_t altro_batch_warm_start_dev(altro_handle* h, int32_t ncand, const double* U, double rho, int32_t include_current,
                                   int32_t* chosen, double* J, double* c_max);
int32_t altro_batch_warm_start(altro_handle* h, int32_t ncand, const double* U, double rho, int32_t include_current,
                               int32_t* chosen, double* J, double* c_max);

/* ---- closed-loop simulation of the stored policy under disturbances.  Every closed loop of the reference perturbs the plant
 * state on every tick (random_linear_problem.jl:129, simple_rocket.jl:65-71, flexible_sat_mpc.jl:266); what the policy a
 * handle holds is worth under such perturbations -- before it is trusted between two ticks, to size a constraint back-off, to
 * decide whether an instance needs a re-solve -- is a Monte-Carlo study with many samples per instance.  One call runs it.
 * altro_batch_simulate_policy_dev: every pointer is a device pointer under the rules of the device-pointer block (validated
 * before anything is enqueued, stream-ordered on the handle's stream, no host synchronisation, no caller pointer kept).
 *   nsamp    >= 1 samples per instance
 *   x0       [batch][nsamp][n] start states; NULL: every sample starts from the initial state the handle holds
 *   w        [batch][nsamp][N-1][n] additive disturbances; NULL: none, and no addition is performed at all
 *   clamp    0 or 1: saturate every control at the BOX, as altro_batch_eval_policy_dev does
 *   J, c_max, dx_max   [batch][nsamp] outputs;  fb [batch] int32 output
 *   Xout     [batch][nsamp][N][n],  Uout [batch][nsamp][N-1][m]   optional outputs
 *   Any output may be NULL, not all six of them.
 * For sample s of instance b, with (xbar, ubar) the trajectory the handle holds and K the gains altro_batch_get_gains returns:
 *   x_0     = x0[b][s]
 *   u_k     = the bytes altro_batch_eval_policy_dev writes for x = x_k, knot = k, clamp          k = 0 .. N-2
 *   x_{k+1} = the rollout arithmetic of altro_batch_evaluate_dev on (x_k, u_k); with w one more rounded addition of
 *             w[b][s][k], performed last
 *   J, c_max = what the given form of altro_batch_evaluate_dev returns for (X, U) = the simulated pair
 *   dx_max  = max over k = 0 .. N-1 and i of |x_k[i] - xbar_k[i]| (the subtraction the policy makes; a NaN stays)
 *   fb[b]   = 1 / 0 as altro_batch_eval_policy_dev reports the validity of the stored gains; with 0 the loop is open:
 *             u_k = ubar_k, clamped if asked
 * The window, the dynamics blocks, the weights, the bounds and the device tables are those altro_batch_evaluate_dev sees at
 * that point of the stream (under an episode clock the instance's own window).  One fused kernel (csrc/simulate.h): the states
 * stay in registers, no workspace grows with nsamp * N * n, and nothing the library owns changes -- the stored gains stay.
 * There is no masking and no status.  Like a solve the call first packs constraint tables a HOST edit has left unpacked.
 * altro_batch_simulate_policy: the same with host arrays, through the handle's staging buffer (grown if needed);
 * synchronises; writes the bytes the `_dev` call writes.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle unchanged and usable): NULL handle; nsamp < 1; clamp not 0 or 1; every
 * output NULL; _dev: what the device-pointer block refuses.  ALTRO_ERR_STATE: dynamics, cost or reference not set, or the
 * window runs past the stored reference.  Caller arrays are indexed with size_t. */
int32_t altro_batch_simulate_policy_dev(altro_handle* h, int32_t nsamp, const double* x0, const double* w, int32_t clamp,
                                        double* J, double* c_max, double* dx_max, int32_t* fb, double* Xout, double* Uout);
int32_t altro_batch_simulate_policy(altro_handle* h, int32_t nsamp, const double* x0, const double* w, int32_t clamp, double* J,
                                    double* c_max, double* dx_max, int32_t* fb, double* Xout, double* Uout);

/* ---- closed-loop covariance of the stored policy: the analytic twin of the simulation above.  The perturbations of the
 * reference's closed loops (random_linear_problem.jl:129, simple_rocket.jl:65-71, flexible_sat_mpc.jl:266) are additive and
 * zero-mean; the model is affine and the policy u = ubar_k + K_k (x - xbar_k) is too, so while no control saturates the first
 * two moments of the loop obey an exact recursion and one pass over the horizon gives, without samples, what sizes a constraint
 * back-off: the standard deviation of every state, control and constraint row, the expected cost increase and a tightened box.
 * altro_batch_propagate_covariance_dev: every pointer is a device pointer under the rules of the device-pointer block (validated
 * before anything is enqueued, stream-ordered on the handle's stream, no host synchronisation, no caller pointer kept).
 *   Sigma0, W  n x n row-major: the covariance of x_0 - xbar_0 and of the disturbance added at every step.  per_instance = 0:
 *            one matrix for the batch; 1: [batch][n][n].  Either may be NULL -- zero, and for W no addition is performed --
 *            not both.  The matrices are used as given: symmetry is the caller's responsibility and is not checked.
 *   con_id   a LINEAR or SOC constraint whose rows' deviations go to sc, or -1 (then sc must be NULL)
 *   kappa    >= 0, finite: the back-off of the tightened box in standard deviations
 * With K_k the matrix altro_batch_get_gains returns and M_k = A_k + B_k K_k:
 *   S_0 = Sigma0,   S_{k+1} = M_k S_k M_k' + W,   k = 0 .. N-2
 * fb[b] (int32 [batch]) has the validity meaning of altro_batch_eval_policy_dev: 1 the stored gains are valid, 0 they are not
 * and the loop is open, K = 0, as in altro_batch_simulate_policy_dev.  No clamp is modelled: the augmented-Lagrangian gains
 * already shrink the rows of controls held at a bound, and the saturated loop is what altro_batch_simulate_policy_dev is for.
 * Outputs, each may be NULL, not all:
 *   sx    [batch][N][n]      sqrt(max(S_k[i][i], 0))
 *   su    [batch][N-1][m]    sqrt(max((K_k S_k K_k')[a][a], 0))
 *   sc    [batch][nk][p]     in the layout of altro_batch_get_duals for con_id: the standard deviation of the row value
 *                            (A z + b)_r, sqrt(max(g' S_k g, 0)) with g = a_x + K_k' a_u (at knot N-1: g = a_x)
 *   dJ    [batch]            E[J] - J(xbar, ubar) with the instance's own weights as altro_batch_evaluate_dev applies them:
 *                            1/2 sum_{k<N-1} dt (sum_i Q_i S_k[i][i] + sum_a R_a (K S_k K')[a][a]) + 1/2 sum_i Qf_i S_{N-1}[i][i]
 *   zmin_t, zmax_t [batch][n+m]   both or neither; they need a BOX on the handle.  s_e = the maximum of element e's deviation
 *                            over the knots of the BOX's range (control columns: up to knot N-2).  Two finite sides, mid =
 *                            0.5 (lo + hi): lo' = min(lo + kappa s_e, mid), hi' = max(hi - kappa s_e, mid); a lone finite
 *                            side lo + kappa s_e or hi - kappa s_e; infinite sides stay.  The row has lo' <= hi' and the
 *                            BOX's pattern of finite sides: altro_batch_set_bounds_dev(.., per_instance = 1) accepts it as
 *                            it is, which closes solve -> propagate -> tighten -> solve on the device.
 *   Sout  [batch][N][n][n]   the matrices S_k as computed, not re-symmetrised
 * The window, the dynamics blocks (altro_mpc_set_dynamics_track: kref * step_stride + k), the weights, the bounds and the
 * constraint tables are those altro_batch_evaluate_dev sees at that point of the stream (under an episode clock the instance's
 * own window).  A NaN stays a NaN.  Nothing the library owns changes and the stored gains stay.  There is no masking: an
 * instance the active mask or the clock leaves out answers from its last solve.  Instance b gets the bytes it would get on a
 * batch-1 handle holding its data.  One kernel (csrc/covariance.h, with the summation orders); the covariance stays in
 * registers or LDS, so the call allocates nothing, with or without Sout.  Like altro_batch_evaluate_dev the call first packs
 * constraint tables a HOST edit has left unpacked.
 * altro_batch_propagate_covariance: the same with host arrays, through the handle's staging buffer (grown if needed);
 * synchronises; writes the bytes the `_dev` call writes.
 * ALTRO_ERR_INVALID_ARG (nothing enqueued, the handle unchanged and usable): NULL handle; Sigma0 and W both NULL; every output
 * NULL; per_instance not 0 or 1; kappa negative, NaN or infinite; exactly one of zmin_t / zmax_t; the pair on a handle with no
 * BOX; sc with con_id = -1, or con_id >= 0 without sc; an unknown or BOX con_id; _dev: what the device-pointer block refuses.
 * ALTRO_ERR_STATE: dynamics, cost or reference not set, or the window runs past the stored reference or dynamics track. */
int32_t altro_batch_propagate_covariance_dev(altro_handle* h, const double* Sigma0, const double* W, int32_t per_instance,
                                             int32_t con_id, double kappa, double* sx, double* su, double* sc, double* dJ,
                                             int32_t* fb, double* zmin_t, double* zmax_t, double* Sout);
int32_t altro_batch_propagate_covariance(altro_handle* h, const double* Sigma0, const double* W, int32_t per_instance,
                                         int32_t con_id, double kappa, double* sx, double* su, double* sc, double* dJ, int32_t* fb,
                                         double* zmin_t, double* zmax_t, double* Sout);

/* ---- per-instance active mask and cold restart: ragged batches of closed loops.
 * The reference runs one problem per loop, and a loop that ends simply stops calling solve! (simple_rocket.jl:137-205); in a
 * batch the instance whose rocket has landed, or whose episode has ended and is re-spawned, sits among others that go on.
 *
 * Active mask.  active [batch], nonzero = active; NULL = every instance (the default: with no mask set nothing differs, bit for
 * bit).  The library copies the array into a buffer of its own and keeps no caller pointer.  While a mask is set,
 * altro_batch_solve / _solve_async, altro_batch_shift_fill, altro_mpc_step_async / _run_async / _prepare_async and the
 * projected-Newton polish behind them (projected_newton = 1) launch work for the active instances only.  For an inactive
 * instance NOTHING the library owns changes: trajectory, current plane and x0 (it takes no plant step inside a fused run),
 * the duals of every constraint, the penalty, the statistics (iterations, status, cost, c_max, the three traces), gains, gain
 * factors and their validity, every work / solve / confirm / reuse counter, the polish statistics, and its slots of the MPC
 * log, which stay in the "never written" state of altro_mpc_get_log.  The results of an active instance are bit-identical to
 * those of the same call sequence on a handle with no mask.  Setters and getters are not masked: the caller may write x0 or a
 * reference for any instance.  A launch under a mask with no active instance is still a launch: it takes its slot of
 * altro_batch_timing_get.  altro_batch_benchmark_solve with a mask set returns ALTRO_ERR_STATE (its restore / repeat protocol
 * is about whole batches).
 * altro_batch_set_active_dev: `active` on the device, under the rules of the device-pointer block above (validated before
 * anything is enqueued, stream-ordered, no host synchronisation, no allocation after the first call); it leaves the handle in
 * the device state its host twin would.  altro_batch_get_active: the mask in force as 0 / 1, all ones when none is set;
 * synchronises the stream.
 * ALTRO_ERR_INVALID_ARG (nothing changes): NULL handle; get_active: NULL array; _dev: what the device-pointer block refuses. */
int32_t altro_batch_set_active(altro_handle* h, const int32_t* active);
int32_t altro_batch_set_active_dev(altro_handle* h, const int32_t* active);
int32_t altro_batch_get_active(altro_handle* h, int32_t* active);
/* Cold restart of single instances.  which [batch], nonzero selects an instance; X [batch][N][n] (may be NULL, as in
 * altro_batch_set_initial_trajectory) and U [batch][N-1][m]: only the rows of selected instances are read.  For each selected
 * instance the trajectory becomes (X, U), the duals of every constraint become zero, the penalty becomes the initial value a
 * new handle holds, the stored gains are dropped (no valid gains, active set cleared), and status becomes ALTRO_UNSOLVED with
 * iteration counts, cost, c_max and traces as a new handle holds them.  Instances not selected are untouched, bit for bit, and
 * the counters that accumulate since altro_batch_timing_reset are not reset.  x0 and the reference are the caller's to set.
 * Contract: the next solve of a restarted instance gives, bit for bit, what a freshly created handle given the same problem
 * data, that instance's x0, reference and (X, U) gives on its first solve.  Independent of the active mask.
 * _dev: which, X, U on the device, under the rules of the device-pointer block.
 * ALTRO_ERR_INVALID_ARG (nothing changes, the handle stays usable): NULL handle, NULL which or U; _dev: what that block refuses. */
int32_t altro_batch_restart_instances(altro_handle* h, const int32_t* which, const double* X, const double* U);
int32_t altro_batch_restart_instances_dev(altro_handle* h, const int32_t* which, const double* X, const double* U);
/* ---- per-instance episode clock: staggered and re-spawned episodes inside the device-resident MPC loop.
 * The reference runs one closed loop per problem, each from its own step 0 (simple_rocket.jl:137-205,
 * random_linear_problem.jl:121-139); in a batch the episodes start and end at different times, and without a clock
 * altro_mpc_step_async / _run_async put every instance at the SAME step of its track.
 *
 * altro_mpc_set_clock: start [batch] (any int32, negative too), length [batch] or NULL (unbounded; a negative entry counts
 * as 0).  start == NULL clears the clock.  The library copies the arrays into buffers of its own and keeps no caller pointer.
 * With no clock set nothing differs, bit for bit.  Needs a track (altro_mpc_set_track).
 * While a clock is set, instance b at absolute step i -- the index passed to altro_mpc_step_async / _run_async /
 * _prepare_async -- is at LOCAL step l = i - start[b], and it ticks at step i iff
 *     0 <= l,   l < length[b] (when given),   l + 1 + N <= Nt (its next window fits the track),
 *     and with altro_mpc_set_dynamics_track: (l + 1) * step_stride + N - 2 < nblocks (so do that window's blocks);
 * otherwise it is idle at that step.  Running off the end of a track ends the episode and is no error: under a clock the
 * "steps run past the end of the track" refusals of the three calls give way to this rule (the noise-range and log-capacity
 * checks stay, keyed by the absolute step).  The rule is evaluated on the device: the host never needs the values.
 * A ticking instance does what step l does on a handle without a clock -- plant step, reference window <- l + 1, dynamics
 * block r = l + 1, primal and dual shift, solve, and with projected_newton = 1 the polish over that window -- except that its
 * plant step takes the noise row of the ABSOLUTE step, noise[i][b] (a re-spawned instance does not replay the noise of its
 * first life), and its log record goes to slot i.
 * An idle instance is treated as an inactive one is (altro_batch_set_active): nothing the library owns for it changes, its
 * log slot i stays never written; an instance the active mask leaves out is idle whatever its clock says.
 * Per-instance window.  The reference window becomes per-instance state: altro_mpc_set_clock on a handle without a clock
 * starts every instance at the handle's current window (a call that only changes a clock in force keeps the windows); a
 * tick sets it to l + 1; altro_batch_restart_instances(_dev) under a clock rewinds the selected instances to window 0 (without
 * a clock that call is unchanged); altro_mpc_set_track / altro_batch_set_reference put every instance back to window 0.  Plain
 * solves and the polish read the instance's own window; altro_mpc_set_dynamics_track under a clock is refused (ALTRO_ERR_STATE)
 * when its table ends before the window some instance holds.  Clearing the clock while the windows differ is refused
 * (ALTRO_ERR_STATE): one scalar cannot hold them; when they agree, that window becomes the handle's.
 * Re-spawning between two launches: restart the instance (window 0), set its x0, run altro_batch_solve under a mask of just
 * that instance, restore the mask, set start[b] to the next absolute step -- from there its records are those of a new
 * handle's solve-then-steps 0, 1, ... with the noise rows of the absolute steps.
 * altro_mpc_set_clock_dev: the arrays on the device, under the rules of the device-pointer block (validated before anything
 * is enqueued, stream-ordered, no host synchronisation unless it clears, no allocation after the first call); it leaves the
 * handle in the device state its host twin would.
 * altro_mpc_get_clock: start, length (-1: unbounded), window, each [batch], any may be NULL but not all; with no clock set
 * start = 0, length = -1 and window = the handle's window for every instance.  Synchronises the stream.
 * altro_batch_benchmark_solve under a clock returns ALTRO_ERR_STATE, as under a mask.  A handle that moves to the
 * one-wave-per-instance kernel afterwards keeps the clock, as it keeps the log setting.
 * ALTRO_ERR_INVALID_ARG (nothing changes): NULL handle; get_clock with all three outputs NULL; _dev: what the device-pointer
 * block refuses.  ALTRO_ERR_STATE: no track set; the clearing case above. */
int32_t altro_mpc_set_clock(altro_handle* h, const int32_t* start, const int32_t* length);
int32_t altro_mpc_set_clock_dev(altro_handle* h, const int32_t* start, const int32_t* length);
int32_t altro_mpc_get_clock(altro_handle* h, int32_t* start, int32_t* length, int32_t* window);
/* Stream hand-over without the host: an event recorded on one stream and waited on by the other (the events belong to the
 * handle and are reused).  wait_stream: work enqueued on the handle's stream from now on starts after everything enqueued so
 * far on `producer` (a hipStream_t).  signal_stream: work enqueued on `consumer` from now on starts after everything enqueued
 * so far on the handle's stream.  NULL names the default stream. */
int32_t altro_batch_wait_stream(altro_handle* h, void* producer);
int32_t altro_batch_signal_stream(altro_handle* h, void* consumer);

#ifdef __cplusplus
}
#endif
#endif
