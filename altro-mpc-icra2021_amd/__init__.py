"""MI355X-native batched ALTRO (AL-iLQR) MPC solver -- host-side package.

The compute path is the HIP shared library built from csrc/ and reached through the C-ABI
declared in include/altro_batch.h.  This package mirrors the Altro.jl /
TrajectoryOptimization.jl call surface the reference's benchmark scripts use (api.py) and
restates the reference's problem generators and MPC harness (problems.py, mpc.py).
"""
from . import _lib, benchmarks, mpc, parallel, problems, results_io  # noqa: F401
from ._lib import SOLVE_SUCCEEDED, STATUS_NAMES, debug_set  # noqa: F401
from .mpc import ExternalMPC, MPCLog, x_traj  # noqa: F401
from .api import first_knot, initial_state, signal_stream, solve_async, synchronize, wait_stream  # noqa: F401
from .api import evaluate, evaluate_grad, merit, propagate_covariance, rollout, simulate_policy, warm_start  # noqa: F401
from .api import evaluate_al, optimal_cost, penalty  # noqa: F401
from .api import get_gain_factors_dev, solution, solution_jvp, solution_vjp  # noqa: F401
from .api import cost_to_go, gain_active_set, mpc_layer, solution_vjp_data  # noqa: F401
from .api import alpha_trace, dev_refusals, eval_policy, gain_factors, gains, get_gains_dev, set_bounds, set_dynamics, set_dynamics_track  # noqa: F401
from .api import (ALTROSolver, AltroError, BoundConstraint, ConstraintList, GoalConstraint, LinearConstraint,
                  LinearModel, NormConstraint, Problem,  # noqa: F401
                  SolverOptions, TrackingObjective, benchmark_solve, confirm_counter, reuse_counter, polish_stats, polish_dual_residuals, controls, cost, get_duals, initial_controls,
                  iterations, max_violation, set_duals, set_initial_state, set_options, set_tracking_cost, shift_fill,
                  solve, solve_counters, states, stats, status, timing_get, timing_reset, update_constraint_data, update_trajectory,
                  wave_cycles, wave_passes, work_counters)
