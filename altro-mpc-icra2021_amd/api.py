"""Host-side mirror of the Altro.jl / TrajectoryOptimization.jl / RobotDynamics.jl calls the
reference's benchmark scripts make, for a BATCH of independent instances solved on MI355X.

Julia name (reference call site)                      -> here
  RD.LinearModel(A, B[, d]; dt)   (random_linear_problem.jl:8)  -> LinearModel
  TO.TrackingObjective / LQRObjective (mpc.jl:29)      -> TrackingObjective
  BoundConstraint(n,m,u_min,u_max) (random_linear_problem.jl:23) -> BoundConstraint
  ConstraintList / add_constraint! (random_linear_problem.jl:22-24) -> ConstraintList.add_constraint
  Problem(model,obj,xf,tf;x0,constraints) (mpc.jl:42)  -> Problem
  SolverOptions(...) / set_options! (run_random_linear.jl:41-49) -> SolverOptions / set_options
  ALTROSolver(prob, opts) (random_linear_problem.jl:87) -> ALTROSolver
  solve!(altro) (:113)                                  -> solve(altro)
  TO.set_initial_state! (:130)                          -> set_initial_state(altro, x0)
  TO.update_trajectory!(obj, Z_track, k) (:133)         -> update_trajectory(altro, Xref, Uref)
  RD.shift_fill!(Z) (:136), Altro.shift_fill!(conSet) (:139) -> shift_fill(altro, primal, dual)
  states / controls / iterations / status / cost / max_violation (:166-181) -> same names
  benchmark_solve!(altro; samples, evals) (:161)        -> benchmark_solve(altro, ...)

Arrays are numpy, instance-major: X (B, N, n), U (B, N-1, m), A (B, n, n) in natural
(row, col) indexing; conversion to the C-ABI's column-major blocks happens here.

Device-resident I/O: set_initial_state, update_trajectory, initial_controls, set_dynamics, update_constraint_data and
set_bounds also take torch tensors that
live on the solver's GPU (the altro_*_dev entry points: nothing crosses PCIe, nothing synchronises), and states, controls
and first_knot write into such tensors; eval_policy (the feedback policy between two ticks), get_gains_dev, evaluate and
rollout (candidate trajectories scored against the next solve's problem) read and write them.  warm_start scores candidate
controls the same way and installs the best as the next solve's initial trajectory; simulate_policy runs the policy the last
solve holds in closed loop on the model, many disturbed samples per instance, and propagate_covariance gives the first two
moments of that loop without samples.  A GPU tensor is never copied, cast or moved behind the caller's back: float64,
contiguous, on the solver's device and of the exact shape, or ValueError.  Matrices keep their natural (row, col) indexing;
since the C-ABI reads column-major blocks, a dynamics tensor must be STORED column-major, i.e. `At.transpose(-1, -2)` of a
contiguous tensor At that holds the transposed blocks.  Every tensor call is ordered against torch's current stream
(wait_stream before, signal_stream after), so a caller that stays on one torch stream needs no synchronisation.  This
module imports without torch.
"""
import ctypes as C
import sys
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import AltroError, SOLVE_SUCCEEDED, STATUS_NAMES  # noqa: F401

_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int32)


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(_DP)


def _is_tensor(a):
    """a torch tensor?  (without importing torch: if it was never imported there are no tensors)"""
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(a, torch.Tensor)


def _on_gpu(a):
    """a torch tensor in GPU memory: takes the device path.  Everything else (numpy, lists, CPU tensors) goes through
    np.asarray as before."""
    return _is_tensor(a) and a.device.type != "cpu"


def _gpu_form(what, args, nreq=0):
    """Which form of a twin pair the arrays of a call select: True when they are GPU tensors (or None; the first nreq may not be
    None), the device form; False when none is a GPU tensor, the host twin.  A mix is refused: nothing is converted."""
    if not any(_on_gpu(a) for a in args):
        return False
    if not all(_on_gpu(a) or (a is None and i >= nreq) for i, a in enumerate(args)):
        raise ValueError(f"{what} must all be GPU tensors (or None), or none of them")
    return True


def _check_np_out(fn, nm, o, shp, dt=np.float64):
    """o is an array a host twin can write into as it is"""
    if not (isinstance(o, np.ndarray) and o.dtype == dt and o.flags.c_contiguous and o.shape == shp):
        raise ValueError(f"{fn}: {nm} must be a C-contiguous {np.dtype(dt).name} array of shape {shp}")


def _dense_strides(shape, colmajor=False):
    """element strides of a dense array of `shape`; colmajor: the last two dimensions stored transposed (column-major blocks)"""
    shape = list(shape)
    if colmajor:
        shape[-1], shape[-2] = shape[-2], shape[-1]
    st, acc = [], 1
    for k in reversed(shape):
        st.append(acc)
        acc *= int(k)
    st.reverse()
    if colmajor:
        st[-1], st[-2] = st[-2], st[-1]
    return tuple(st)


def check_device_tensor(t, shape, device, name="tensor", dtype="torch.float64", colmajor=False):
    """The whole validation of a GPU tensor before its address is handed to the library -- a plain function of t.shape,
    t.dtype, t.stride() and t.device, so any object with those four works.  Raises ValueError; never copies, casts or moves."""
    shape = tuple(int(k) for k in shape)
    if t.device.type != "cuda" or (t.device.index if t.device.index is not None else 0) != int(device):
        raise ValueError(f"{name}: tensor on {t.device}, the solver runs on cuda:{int(device)}")
    if str(t.dtype) != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype} (no implicit cast)")
    if tuple(t.shape) != shape:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {shape}")
    want = _dense_strides(shape, colmajor)
    if any(k > 1 and int(a) != b for k, a, b in zip(shape, t.stride(), want)):
        how = "stored column-major (the transpose(-1, -2) of a contiguous tensor)" if colmajor else "contiguous"
        raise ValueError(f"{name}: strides {tuple(t.stride())}, expected {want}: the tensor must be {how} (no implicit copy)")
    return t


def _stream_handle(stream, device):
    """hipStream_t of a torch stream (default: torch's current stream on `device`), as an integer address"""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(device)
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)) or None)


def wait_stream(solver, stream=None):
    """Work enqueued on the solver's stream from now on starts after everything enqueued so far on `stream` (a torch stream;
    default torch's current one).  No host synchronisation (altro_batch_wait_stream)."""
    solver._chk(solver._L.altro_batch_wait_stream(solver.h, _stream_handle(stream, solver.device)))


def signal_stream(solver, stream=None):
    """Work enqueued on `stream` from now on starts after everything enqueued so far on the solver's stream
    (altro_batch_signal_stream)."""
    solver._chk(solver._L.altro_batch_signal_stream(solver.h, _stream_handle(stream, solver.device)))


class _bracket:
    """wait_stream ... signal_stream against torch's current stream around the tensor calls inside"""

    def __init__(self, solver):
        self.solver = solver

    def __enter__(self):
        _lib.check_single_runtime()
        wait_stream(self.solver)

    def __exit__(self, *exc):
        signal_stream(self.solver)
        return False


def _addr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def SolverOptions(**kw):
    """Altro.SolverOptions with Altro.jl's defaults; keyword names as in the reference."""
    o = _lib.Opts()
    rc = _lib.lib().altro_default_opts(C.byref(o))
    if rc:
        raise AltroError(rc, "altro_default_opts")
    for k, v in kw.items():
        if k in ("verbose", "show_summary", "static_bp", "save_S"):
            # accepted for source compatibility: they only affect printing or Julia-side memory layout
            continue
        if not hasattr(o, k):
            raise KeyError(f"unknown SolverOptions field {k}")
        setattr(o, k, v)
    return o


@dataclass
class LinearModel:
    """RD.LinearModel: x+ = A x + B u (+ d).  A: (n,n) shared or (B,n,n) per instance; with
    per_knot=True (a model built with `times`, ALTROParams.jl:61) one block per knot:
    (N-1,n,n) or (B,N-1,n,n), d likewise."""
    A: np.ndarray
    B: np.ndarray
    d: Optional[np.ndarray] = None
    dt: float = 0.1
    per_knot: bool = False


def _rows(arrs, B):
    """Shared or per-instance data: every array 1-D -> (False, the arrays as (k,)); any of them (B, k) -> (True, all of them as
    (B, k), the 1-D ones broadcast).  A 2-D array whose leading dimension is not B raises AltroError(ERR_INVALID_ARG)."""
    arrs = [np.asarray(a, dtype=np.float64) for a in arrs]
    for a in arrs:
        if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[0] != B):
            raise AltroError(_lib.ERR_INVALID_ARG, f"expected ({B}, k) or (k,) per-instance data, got shape {a.shape}")
    if all(a.ndim == 1 for a in arrs):
        return False, [_c(a) for a in arrs]
    return True, [_c(np.broadcast_to(a, (B, a.shape[-1]))) for a in arrs]


def cost_rows(Q, R, Qf, B):
    """(per_instance, Q, R, Qf) as the C-ABI takes them: (n,), (m,), (n,) for altro_batch_set_tracking_cost, or (B, n),
    (B, m), (B, n) for altro_batch_set_tracking_cost_per_instance when any of them is given per instance."""
    pi, (q, r, qf) = _rows((Q, R, Qf), B)
    return pi, q, r, qf


@dataclass
class TrackingObjective:
    """Diagonal tracking cost about (Xref, Uref); stage costs are scaled by dt.  Q, R, Qf are (n,), (m,), (n,) for the
    whole batch or (B, n), (B, m), (B, n) per instance (random_linear_problem.jl:11-13 draws them per problem)."""
    Q: np.ndarray
    R: np.ndarray
    Qf: np.ndarray
    Xref: np.ndarray   # (B, N, n)
    Uref: np.ndarray   # (B, N-1, m)


@dataclass
class BoundConstraint:
    """Each field: None (unbounded), a scalar, (k,) for the whole batch, or (B, k) per instance (which elements are bounded
    must then be the same in every row: altro_batch_set_bounds)."""
    n: int
    m: int
    x_min: Optional[np.ndarray] = None
    x_max: Optional[np.ndarray] = None
    u_min: Optional[np.ndarray] = None
    u_max: Optional[np.ndarray] = None

    def per_instance(self):
        return any(v is not None and np.ndim(v) == 2 for v in (self.x_min, self.x_max, self.u_min, self.u_max))

    def zbounds(self, B=None):
        """(zmin, zmax): (n+m,) each, or (B, n+m) each when a field is given per instance (B: the batch, checked)."""
        pi = self.per_instance()
        rows = None
        if pi:
            rows = B if B is not None else next(np.shape(v)[0] for v in (self.x_min, self.x_max, self.u_min, self.u_max)
                                                if v is not None and np.ndim(v) == 2)

        def full(v, k, fill):
            if v is None:
                v = fill
            v = np.asarray(v, dtype=np.float64)
            if v.ndim == 2 and (v.shape[0] != rows or v.shape[1] != k):
                raise AltroError(_lib.ERR_INVALID_ARG, f"bound of shape {v.shape}: expected ({rows}, {k}) or ({k},)")
            return np.broadcast_to(v, (rows, k) if pi else (k,)).copy()
        zmin = np.concatenate([full(self.x_min, self.n, -np.inf), full(self.u_min, self.m, -np.inf)], axis=-1)
        zmax = np.concatenate([full(self.x_max, self.n, np.inf), full(self.u_max, self.m, np.inf)], axis=-1)
        return zmin, zmax


@dataclass
class LinearConstraint:
    """A z + b {= 0 | <= 0}; A is (p, n+m) on z = [x; u].  Mirrors TO.LinearConstraint /
    GoalConstraint(xf) (A = [I 0], b = -xf) / LinearizedFrictionConstraint."""
    A: np.ndarray
    b: np.ndarray
    equality: bool = False
    per_instance: bool = False   # A is (B, p, n+m) or (B, nk, p, n+m): every instance of the batch owns its data


@dataclass
class NormConstraint:
    """Second-order cone: ||(A z + b)[0:p-1]|| <= (A z + b)[p-1].  Mirrors NormConstraint(n, m, val,
    SecondOrderCone(), :control) (rocket_landing_problem.jl:123) and NormConstraint2 ([A y; c'y],
    new_constraints.jl:72-120) with their rows written on z."""
    A: np.ndarray
    b: np.ndarray
    per_instance: bool = False   # as LinearConstraint.per_instance


def GoalConstraint(xf, n, m):
    """GoalConstraint(xf) (rocket_landing_problem.jl:96): x_N = xf, added at knot N."""
    xf = np.asarray(xf, dtype=np.float64)
    return LinearConstraint(np.hstack([np.eye(n), np.zeros((n, m))]), -xf, equality=True)


@dataclass
class ConstraintList:
    n: int
    m: int
    N: int
    items: List = field(default_factory=list)

    def add_constraint(self, con, inds):
        """inds: 1-based inclusive range (first, last) as in Julia's `1:N-1`."""
        first, last = (inds.start, inds.stop - 1) if isinstance(inds, range) else inds
        self.items.append((con, int(first), int(last)))


@dataclass
class Problem:
    model: LinearModel
    obj: TrackingObjective
    constraints: ConstraintList
    x0: np.ndarray          # (B, n)
    N: int
    U0: Optional[np.ndarray] = None  # (B, N-1, m) initial controls; default: the reference controls

    @property
    def batch(self):
        return self.x0.shape[0]


class ALTROSolver:
    """ALTROSolver(prob, opts): owns a device-resident batch of solver workspaces."""

    def __init__(self, prob: Problem, opts=None, device=0):
        L = _lib.lib()
        self._L = L
        self.prob = prob
        B, n = prob.x0.shape
        m = np.asarray(prob.obj.R).shape[-1]
        self.B, self.n, self.m, self.N = B, n, m, prob.N
        self.device = int(device)
        self.opts = opts if opts is not None else SolverOptions()
        dims = _lib.Dims(B, n, m, prob.N)
        h = C.c_void_p()
        _lib.sync_debug_env()   # the tests' / tools' ALTRO_* switches reach the library through altro_debug_set, not getenv
        rc = L.altro_batch_create(C.byref(dims), C.byref(self.opts), device, C.byref(h))
        if rc:
            raise AltroError(rc, L.altro_last_error(None).decode())
        self.h = h
        self.con_ids = []
        mdl = prob.model
        set_dynamics(self, mdl)
        set_tracking_cost(self, prob.obj.Q, prob.obj.R, prob.obj.Qf, mdl.dt)
        for con, first, last in prob.constraints.items:
            if isinstance(con, BoundConstraint):
                zmin, zmax = con.zbounds(B)
                cid = C.c_int32(-1)
                # per-instance bounds: the BOX is added with instance 0's row (it fixes the pattern of finite sides), then
                # every instance gets its own
                self._chk(L.altro_batch_add_constraint(h, _lib.CON_BOX, _lib.SENSE_INEQ, first - 1, last - 1, 0,
                                                       None, None, _p(_c(zmin.reshape(-1, n + m)[0])),
                                                       _p(_c(zmax.reshape(-1, n + m)[0])), 0, C.byref(cid)))
                self.con_ids.append(cid.value)
                if zmin.ndim == 2:
                    self._chk(L.altro_batch_set_bounds(h, cid.value, _p(_c(zmin)), _p(_c(zmax)), 1))
            elif isinstance(con, (LinearConstraint, NormConstraint)):
                A, b = _c(con.A), _c(con.b)
                per_inst = bool(getattr(con, "per_instance", False))
                per_knot = A.ndim == (4 if per_inst else 3)   # (nk, p, n+m): LinearConstraintTraj / AffineSOCTraj
                assert A.shape[-1] == n + m and A.shape[:-1] == b.shape
                assert not per_inst or A.shape[0] == B
                assert not per_knot or A.shape[-3] == last - first + 1
                soc = isinstance(con, NormConstraint)
                kind = _lib.CON_SOC if soc else _lib.CON_LINEAR
                sense = _lib.SENSE_EQ if (not soc and con.equality) else _lib.SENSE_INEQ
                cid = C.c_int32(-1)
                self._chk(L.altro_batch_add_constraint(h, kind, sense, first - 1, last - 1, A.shape[-2],
                                                       _p(A), _p(b), None, None, int(per_knot) | (2 if per_inst else 0), C.byref(cid)))
                self.con_ids.append(cid.value)
            else:
                raise AltroError(_lib.ERR_UNSUPPORTED, f"constraint type {type(con).__name__} is not built yet")
        update_trajectory(self, prob.obj.Xref, prob.obj.Uref)
        set_initial_state(self, prob.x0)
        U0 = prob.U0 if prob.U0 is not None else prob.obj.Uref
        initial_controls(self, U0)

    def _chk(self, rc):
        if rc:
            raise AltroError(rc, self._L.altro_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self._L.altro_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def set_dynamics(solver, mdl):
    """Install (or replace) the dynamics: the quadruped controller rewrites model.A[k], B[k], d[k]
    before every solve (altro_solver.jl:5-37).  With GPU tensors (all of A, B and d, stored column-major: see the module
    docstring) the tables are read on the device."""
    if any(_on_gpu(a) for a in (mdl.A, mdl.B, mdl.d)):
        with _bracket(solver):
            return _set_dynamics_dev(solver, mdl)
    A = np.asarray(mdl.A, dtype=np.float64)
    Bm = np.asarray(mdl.B, dtype=np.float64)
    per_instance = A.ndim == (4 if mdl.per_knot else 3)
    Ac = _c(np.swapaxes(A, -1, -2))
    Bc = _c(np.swapaxes(Bm, -1, -2))
    dc = _c(mdl.d) if mdl.d is not None else None
    solver._chk(solver._L.altro_batch_set_dynamics(solver.h, _p(Ac), _p(Bc), _p(dc), int(mdl.per_knot), int(per_instance)))


def _set_dynamics_dev(solver, mdl):
    A, Bm, d = mdl.A, mdl.B, mdl.d
    if not (_on_gpu(A) and _on_gpu(Bm) and (d is None or _on_gpu(d))):
        raise ValueError("set_dynamics: A, B and d must all be GPU tensors, or none of them")
    n, m = solver.n, solver.m
    lead_ndim = A.ndim - 2
    if lead_ndim != (1 if mdl.per_knot else 0) and lead_ndim != (2 if mdl.per_knot else 1):
        raise ValueError(f"set_dynamics: A of shape {tuple(A.shape)}")
    per_instance = lead_ndim == (2 if mdl.per_knot else 1)
    lead = ((solver.B,) if per_instance else ()) + ((solver.N - 1,) if mdl.per_knot else ())
    check_device_tensor(A, lead + (n, n), solver.device, "A", colmajor=True)
    check_device_tensor(Bm, lead + (n, m), solver.device, "B", colmajor=True)
    if d is not None:
        check_device_tensor(d, lead + (n,), solver.device, "d")
    solver._chk(solver._L.altro_batch_set_dynamics_dev(solver.h, _addr(A), _addr(Bm), _addr(d), int(mdl.per_knot), int(per_instance)))


def set_dynamics_track(solver, A, B, d=None, step_stride=1):
    """Per-knot dynamics of every MPC step, uploaded once for the device-resident loop
    (altro_mpc_set_dynamics_track; reference: update_dynamics_matrices!, altro_solver.jl:5-37).
    A: (nblocks, n, n) shared or (B, nblocks, n, n) per instance, B and d likewise; the solve of MPC
    step i reads block (i + 1) * step_stride + k for knot k (step_stride 1: blocks indexed by absolute
    knot; N - 1: one table per step)."""
    A = np.asarray(A, dtype=np.float64)
    Bm = np.asarray(B, dtype=np.float64)
    per_instance = A.ndim == 4
    nblocks = A.shape[-3]
    Ac = _c(np.swapaxes(A, -1, -2))
    Bc = _c(np.swapaxes(Bm, -1, -2))
    dc = _c(d) if d is not None else None
    solver._chk(solver._L.altro_mpc_set_dynamics_track(solver.h, _p(Ac), _p(Bc), _p(dc), int(nblocks), int(step_stride), int(per_instance)))


def set_tracking_cost(solver, Q, R, Qf, dt=None):
    """Replace the diagonal weights of the tracking objective (TO.TrackingObjective(Q, R, Z; Qf), mpc.jl:26-29).  Q, R, Qf
    are (n,), (m,), (n,) for the batch or (B, n), (B, m), (B, n) per instance (any 2-D one makes the call per instance)."""
    dt = solver.prob.model.dt if dt is None else dt
    pi, q, r, qf = cost_rows(Q, R, Qf, solver.B)
    fn = solver._L.altro_batch_set_tracking_cost_per_instance if pi else solver._L.altro_batch_set_tracking_cost
    solver._chk(fn(solver.h, _p(q), _p(r), _p(qf), dt))


def set_bounds(solver, con, zmin, zmax):
    """New bounds of the BOX constraint `con` (index into the problem's constraint list), in place: (n+m,) each for the
    batch or (B, n+m) each per instance; the finite sides must be those the BOX was added with (altro_batch_set_bounds).
    With GPU tensors (both) the rows are checked and written on the device (altro_batch_set_bounds_dev): a row that fails
    leaves that instance's bounds as they were and is counted (dev_refusals) instead of raising."""
    if _on_gpu(zmin) or _on_gpu(zmax):
        if not (_on_gpu(zmin) and _on_gpu(zmax)):
            raise ValueError("set_bounds: zmin and zmax must both be GPU tensors, or neither")
        with _bracket(solver):
            return _set_bounds_dev(solver, con, zmin, zmax)
    pi, (lo, hi) = _rows((zmin, zmax), solver.B)
    solver._chk(solver._L.altro_batch_set_bounds(solver.h, solver.con_ids[con], _p(lo), _p(hi), int(pi)))


def _set_bounds_dev(solver, con, zmin, zmax):
    nz = solver.n + solver.m
    pi = len(zmin.shape) == 2
    shape = (solver.B, nz) if pi else (nz,)
    check_device_tensor(zmin, shape, solver.device, "zmin")
    check_device_tensor(zmax, shape, solver.device, "zmax")
    solver._chk(solver._L.altro_batch_set_bounds_dev(solver.h, solver.con_ids[con], _addr(zmin), _addr(zmax), int(pi)))


def dev_refusals(solver):
    """rows the device-side check of set_bounds (GPU tensors) has refused since the solver was created
    (altro_batch_get_dev_refusals); synchronises"""
    v = C.c_int64(0)
    solver._chk(solver._L.altro_batch_get_dev_refusals(solver.h, C.byref(v)))
    return int(v.value)


def set_options(solver, **kw):
    for k, v in kw.items():
        setattr(solver.opts, k, v)
    solver._chk(solver._L.altro_batch_set_options(solver.h, C.byref(solver.opts)))


def _set_initial_state_dev(solver, x0):
    check_device_tensor(x0, (solver.B, solver.n), solver.device, "x0")
    solver._chk(solver._L.altro_batch_set_initial_state_dev(solver.h, _addr(x0)))


def _update_trajectory_dev(solver, Xref, Uref):
    if not (_on_gpu(Xref) and _on_gpu(Uref)):
        raise ValueError("update_trajectory: Xref and Uref must both be GPU tensors, or neither")
    check_device_tensor(Xref, (solver.B, solver.N, solver.n), solver.device, "Xref")
    check_device_tensor(Uref, (solver.B, solver.N - 1, solver.m), solver.device, "Uref")
    solver._chk(solver._L.altro_batch_set_reference_dev(solver.h, _addr(Xref), _addr(Uref)))


def _initial_trajectory_dev(solver, X, U):
    if X is not None:
        check_device_tensor(X, (solver.B, solver.N, solver.n), solver.device, "X")
    check_device_tensor(U, (solver.B, solver.N - 1, solver.m), solver.device, "U")
    solver._chk(solver._L.altro_batch_set_initial_trajectory_dev(solver.h, _addr(X), _addr(U)))


def set_initial_state(solver, x0):
    if _on_gpu(x0):
        with _bracket(solver):
            return _set_initial_state_dev(solver, x0)
    x0 = _c(x0)
    assert x0.shape == (solver.B, solver.n)
    solver._chk(solver._L.altro_batch_set_initial_state(solver.h, _p(x0)))


def update_trajectory(solver, Xref, Uref):
    if _on_gpu(Xref) or _on_gpu(Uref):
        with _bracket(solver):
            return _update_trajectory_dev(solver, Xref, Uref)
    Xr, Ur = _c(Xref), _c(Uref)
    assert Xr.shape == (solver.B, solver.N, solver.n) and Ur.shape == (solver.B, solver.N - 1, solver.m)
    solver._chk(solver._L.altro_batch_set_reference(solver.h, _p(Xr), _p(Ur)))


def initial_controls(solver, U):
    if _on_gpu(U):
        with _bracket(solver):
            return _initial_trajectory_dev(solver, None, U)
    U = _c(U)
    assert U.shape == (solver.B, solver.N - 1, solver.m)
    solver._chk(solver._L.altro_batch_set_initial_trajectory(solver.h, None, _p(U)))


def _flags_i32(a, B, name):
    a = np.ascontiguousarray(np.asarray(a) != 0, dtype=np.int32)
    if a.shape != (B,):
        raise ValueError(f"{name}: shape {a.shape}, expected ({B},)")
    return a


def _set_active_dev(solver, active):
    check_device_tensor(active, (solver.B,), solver.device, "active", dtype="torch.int32")
    solver._chk(solver._L.altro_batch_set_active_dev(solver.h, _addr(active)))


def set_active(solver, active):
    """Per-instance active mask (altro_batch_set_active): solves, shift_fill and MPC steps then act on the instances with a
    nonzero entry only, and everything the solver holds for the others stays as it is.  active: (B,) numpy / list, or an
    int32 GPU tensor (device path, stream-ordered); None clears the mask."""
    if active is None:
        solver._chk(solver._L.altro_batch_set_active(solver.h, None))
    elif _on_gpu(active):
        with _bracket(solver):
            _set_active_dev(solver, active)
    else:
        a = _flags_i32(active, solver.B, "active")
        solver._chk(solver._L.altro_batch_set_active(solver.h, a.ctypes.data_as(_IP)))


def get_active(solver):
    """(B,) int32 of 0 / 1: the mask in force (all ones when none is set)"""
    a = np.empty(solver.B, dtype=np.int32)
    solver._chk(solver._L.altro_batch_get_active(solver.h, a.ctypes.data_as(_IP)))
    return a


def _clock_i32(a, B, name):
    """(B,) int32 from an integer array or list; anything else is refused before the library sees it"""
    a = np.asarray(a)
    if a.shape != (B,):
        raise ValueError(f"{name}: shape {a.shape}, expected ({B},)")
    if a.dtype.kind not in "iu":
        raise TypeError(f"{name}: dtype {a.dtype}, expected an integer type")
    if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):
        raise ValueError(f"{name}: values outside int32")
    return np.ascontiguousarray(a, dtype=np.int32)


def set_clock(solver, start, length=None):
    """Per-instance episode clock of the device-resident MPC loop (altro_mpc_set_clock): at absolute step i instance b is at
    local step i - start[b] and takes the step only while 0 <= local step < length[b] (length None: until its track ends);
    otherwise it is idle, exactly as an inactive instance is.  start, length: (B,) integer numpy arrays / lists, or int32
    GPU tensors (device path, stream-ordered); start None clears the clock."""
    if start is None:
        if length is not None:
            raise ValueError("set_clock: length without start")
        solver._chk(solver._L.altro_mpc_set_clock(solver.h, None, None))
    elif _on_gpu(start) or _on_gpu(length):
        if not (_on_gpu(start) and (length is None or _on_gpu(length))):
            raise ValueError("set_clock: start and length must both be GPU tensors, or neither")
        check_device_tensor(start, (solver.B,), solver.device, "start", dtype="torch.int32")
        if length is not None:
            check_device_tensor(length, (solver.B,), solver.device, "length", dtype="torch.int32")
        with _bracket(solver):
            solver._chk(solver._L.altro_mpc_set_clock_dev(solver.h, _addr(start), _addr(length)))
    else:
        st = _clock_i32(start, solver.B, "start")
        ln = None if length is None else _clock_i32(length, solver.B, "length")
        solver._chk(solver._L.altro_mpc_set_clock(solver.h, st.ctypes.data_as(_IP), None if ln is None else ln.ctypes.data_as(_IP)))


def get_clock(solver):
    """(start, length, window), each (B,) int32: the clock in force and every instance's reference window (with no clock:
    zeros, -1 = unbounded, and the solver's one window)"""
    out = [np.empty(solver.B, dtype=np.int32) for _ in range(3)]
    solver._chk(solver._L.altro_mpc_get_clock(solver.h, *(a.ctypes.data_as(_IP) for a in out)))
    return tuple(out)


def _restart_instances_dev(solver, which, U, X=None):
    check_device_tensor(which, (solver.B,), solver.device, "which", dtype="torch.int32")
    if X is not None:
        check_device_tensor(X, (solver.B, solver.N, solver.n), solver.device, "X")
    check_device_tensor(U, (solver.B, solver.N - 1, solver.m), solver.device, "U")
    solver._chk(solver._L.altro_batch_restart_instances_dev(solver.h, _addr(which), _addr(X), _addr(U)))


def restart_instances(solver, which, U, X=None):
    """Cold restart of the instances `which` selects (altro_batch_restart_instances): trajectory <- rows of (X, U), zero
    duals, initial penalty, no stored gains, statistics of an unsolved instance -- their next solve is that of a new solver.
    which (B,), U (B, N-1, m), X (B, N, n) or None: numpy, or all GPU tensors (which int32; device path)."""
    if _on_gpu(which) or _on_gpu(U) or _on_gpu(X):
        if not (_on_gpu(which) and _on_gpu(U) and (X is None or _on_gpu(X))):
            raise ValueError("restart_instances: which, U and X must all be GPU tensors, or none of them")
        with _bracket(solver):
            return _restart_instances_dev(solver, which, U, X)
    w = _flags_i32(which, solver.B, "which")
    U = _c(U)
    assert U.shape == (solver.B, solver.N - 1, solver.m)
    if X is not None:
        X = _c(X)
        assert X.shape == (solver.B, solver.N, solver.n)
    solver._chk(solver._L.altro_batch_restart_instances(solver.h, w.ctypes.data_as(_IP), _p(X), _p(U)))


def shift_fill(solver, primal=True, dual=True):
    solver._chk(solver._L.altro_batch_shift_fill(solver.h, int(primal), int(dual)))


def solve(solver):
    solver._chk(solver._L.altro_batch_solve(solver.h))
    return solver


def solve_async(solver):
    """solve!(solver), only enqueued on the solver's stream (altro_batch_solve_async); pair with synchronize, or with
    signal_stream / the tensor getters, which are ordered after it."""
    solver._chk(solver._L.altro_batch_solve_async(solver.h))
    return solver


def synchronize(solver):
    solver._chk(solver._L.altro_batch_synchronize(solver.h))


def benchmark_solve(solver, samples=10, evals=10):
    """benchmark_solve!(solver; samples, evals) (random_linear_problem.jl:161 with samples=5, evals=5):
    the solver's trajectory is saved, then 1 warm-up + samples x evals repetitions of
    { initial_trajectory!(solver, Z0); solve!(solver) } run on the device.  Duals and penalties are
    NOT restored between repetitions (Altro.jl restores the primal trajectory only), so with
    reset_duals=false the statistics left behind -- the ones the reference stores in its *.jld2
    files -- are those of a solve from converged multipliers.  Returns the per-sample times in ms
    for the whole batch (BenchmarkTools' trial: time of a sample / evals)."""
    ms = np.zeros(samples, dtype=np.float32)
    solver._chk(solver._L.altro_batch_benchmark_solve(solver.h, int(samples), int(evals),
                                                      ms.ctypes.data_as(C.POINTER(C.c_float))))
    return ms


def states(solver, out=None):
    """states(solver): (B, N, n) numpy; out = a GPU tensor of that shape: written on the device and returned."""
    if out is not None:
        if not _on_gpu(out):
            raise ValueError("states: out must be a GPU tensor")
        with _bracket(solver):
            check_device_tensor(out, (solver.B, solver.N, solver.n), solver.device, "out")
            solver._chk(solver._L.altro_batch_get_states_dev(solver.h, _addr(out)))
        return out
    X = np.empty((solver.B, solver.N, solver.n))
    solver._chk(solver._L.altro_batch_get_states(solver.h, _p(X)))
    return X


def controls(solver, out=None):
    """controls(solver): (B, N-1, m) numpy; out = a GPU tensor of that shape: written on the device and returned."""
    if out is not None:
        if not _on_gpu(out):
            raise ValueError("controls: out must be a GPU tensor")
        with _bracket(solver):
            check_device_tensor(out, (solver.B, solver.N - 1, solver.m), solver.device, "out")
            solver._chk(solver._L.altro_batch_get_controls_dev(solver.h, _addr(out)))
        return out
    U = np.empty((solver.B, solver.N - 1, solver.m))
    solver._chk(solver._L.altro_batch_get_controls(solver.h, _p(U)))
    return U


def initial_state(solver, out=None):
    """x0 currently installed: (B, n) numpy; out = a GPU tensor of that shape: written on the device and returned."""
    if out is not None:
        if not _on_gpu(out):
            raise ValueError("initial_state: out must be a GPU tensor")
        with _bracket(solver):
            check_device_tensor(out, (solver.B, solver.n), solver.device, "out")
            solver._chk(solver._L.altro_batch_get_initial_state_dev(solver.h, _addr(out)))
        return out
    x = np.empty((solver.B, solver.n))
    solver._chk(solver._L.altro_batch_get_initial_state(solver.h, _p(x)))
    return x


def _first_knot_dev(solver, out=None):
    import torch
    if out is None:
        dev = torch.device("cuda", solver.device)
        out = (torch.empty((solver.B, solver.m), dtype=torch.float64, device=dev),
               torch.empty((solver.B, solver.n), dtype=torch.float64, device=dev),
               torch.empty((solver.B,), dtype=torch.int32, device=dev), torch.empty((solver.B,), dtype=torch.int32, device=dev))
    u0, x1, st, it = out
    for t, shape, dt, nm in ((u0, (solver.B, solver.m), "torch.float64", "u0"), (x1, (solver.B, solver.n), "torch.float64", "x1"),
                             (st, (solver.B,), "torch.int32", "status"), (it, (solver.B,), "torch.int32", "iterations")):
        if t is not None:
            check_device_tensor(t, shape, solver.device, nm, dtype=dt)
    solver._chk(solver._L.altro_batch_get_first_knot_dev(solver.h, _addr(u0), _addr(x1), _addr(st), _addr(it)))
    return u0, x1, st, it


def first_knot(solver, out=None):
    """What an MPC consumer reads each tick, as GPU tensors and without a host synchronisation: (u0 (B, m) the control to
    apply, x1 (B, n) the predicted next state, status (B,) int32, iterations (B,) int32) of the trajectory the solver holds
    once its stream reaches this point (altro_batch_get_first_knot_dev).  out: a tuple of four tensors to write into, any of
    them None to skip it; default: new tensors."""
    with _bracket(solver):
        return _first_knot_dev(solver, out)


def get_duals(solver, con=0):
    c, first, last = solver.prob.constraints.items[con]
    nk = last - first + 1
    if isinstance(c, BoundConstraint):
        lam = np.empty((solver.B, nk, 2, solver.n + solver.m))
    else:
        lam = np.empty((solver.B, nk, np.asarray(c.b).shape[-1]))
    solver._chk(solver._L.altro_batch_get_duals(solver.h, solver.con_ids[con], _p(lam)))
    return lam


def set_duals(solver, lam, con=0):
    lam = _c(lam)
    solver._chk(solver._L.altro_batch_set_duals(solver.h, solver.con_ids[con], _p(lam)))


@dataclass
class Stats:
    iterations: np.ndarray
    iterations_outer: np.ndarray
    status: np.ndarray
    cost: np.ndarray
    c_max: np.ndarray
    cost_trace: np.ndarray
    cmax_trace: np.ndarray
    tsolve_ms: float


def stats(solver):
    B = solver.B
    it = np.empty(B, dtype=np.int32)
    ito = np.empty(B, dtype=np.int32)
    st = np.empty(B, dtype=np.int32)
    cost_ = np.empty(B)
    cm = np.empty(B)
    jt = np.empty((B, _lib.TRACE_LEN))
    ct = np.empty((B, _lib.TRACE_LEN))
    solver._chk(solver._L.altro_batch_get_stats(
        solver.h, it.ctypes.data_as(_IP), ito.ctypes.data_as(_IP), st.ctypes.data_as(_IP),
        _p(cost_), _p(cm), _p(jt), _p(ct)))
    ms = C.c_float(0)
    rc = solver._L.altro_batch_last_solve_ms(solver.h, C.byref(ms))
    return Stats(it, ito, st, cost_, cm, jt, ct, ms.value if rc == 0 else float("nan"))


def iterations(solver):
    return stats(solver).iterations


def status(solver):
    return stats(solver).status


def cost(solver):
    return stats(solver).cost


def max_violation(solver):
    return stats(solver).c_max


def timing_reset(solver):
    solver._chk(solver._L.altro_batch_timing_reset(solver.h))


def timing_get(solver):
    """Durations (ms) of every solve-kernel launch since timing_reset, from HIP events recorded
    on the library's own stream."""
    cnt = C.c_int32(0)
    solver._chk(solver._L.altro_batch_timing_get(solver.h, None, 0, C.byref(cnt)))
    ms = np.zeros(cnt.value, dtype=np.float32)
    if cnt.value:
        solver._chk(solver._L.altro_batch_timing_get(solver.h, ms.ctypes.data_as(C.POINTER(C.c_float)), cnt.value, C.byref(cnt)))
    return ms


def work_counters(solver):
    """(backward passes, rollouts, interpolated line-search trials) per instance since
    timing_reset."""
    i64 = C.POINTER(C.c_int64)
    a = [np.zeros(solver.B, dtype=np.int64) for _ in range(3)]
    solver._chk(solver._L.altro_batch_get_work_counters(solver.h, *[x.ctypes.data_as(i64) for x in a]))
    return tuple(a)


def confirm_counter(solver):
    """iterations per instance (since timing_reset) that the default mode confirmed as converged with the
    first-order costate sweep instead of a backward pass (altro_batch_get_confirm_counter)."""
    a = np.zeros(solver.B, dtype=np.int64)
    solver._chk(solver._L.altro_batch_get_confirm_counter(solver.h, a.ctypes.data_as(C.POINTER(C.c_int64))))
    return a


def polish_stats(solver):
    """(ran, failed, residual) of the projected-Newton polish of the last solve, per instance
    (altro_batch_get_polish_stats; all zero with projected_newton = false)."""
    ran, failed = np.zeros(solver.B, dtype=np.int32), np.zeros(solver.B, dtype=np.int32)
    res = np.zeros(solver.B)
    ip = C.POINTER(C.c_int32)
    solver._chk(solver._L.altro_batch_get_polish_stats(solver.h, ran.ctypes.data_as(ip), failed.ctypes.data_as(ip), _p(res)))
    return ran, failed, res


def polish_dual_residuals(solver):
    """(before, after, failed) of the polish's multiplier projection, per instance: the stationarity residual
    ||g + D' lam||_2 with the AL duals and with the projected multipliers (altro_batch_get_polish_dual_residuals)."""
    a, b = np.zeros(solver.B), np.zeros(solver.B)
    f = np.zeros(solver.B, dtype=np.int32)
    solver._chk(solver._L.altro_batch_get_polish_dual_residuals(solver.h, _p(a), _p(b), f.ctypes.data_as(C.POINTER(C.c_int32))))
    return a, b, f


def reuse_counter(solver):
    """iterations per instance (since timing_reset) that took their gains from memory instead of running a backward
    pass (altro_batch_get_reuse_counter)."""
    a = np.zeros(solver.B, dtype=np.int64)
    solver._chk(solver._L.altro_batch_get_reuse_counter(solver.h, a.ctypes.data_as(C.POINTER(C.c_int64))))
    return a


def wave_cycles(solver):
    """(waves, 16) per wave of the last solve launch (16-lane kernels): s_memtime ticks in total (column 0) and, in
    the -DALTRO_PHASE_STAMPS build, per phase: 1 four-row backward passes, 2 closed-loop rollouts, 3 open-loop rollouts,
    4 Todorov gradient, 5 dual update, 6 line-search sweeps, 8 lone-row backward passes, 9 first-order sweeps,
    10 costate sweeps; 11-15 how many four-row passes, first-order sweeps, costate sweeps, closed-loop rollouts and
    trial sweeps the wave ran.  Column 7 (every build): backward passes run in the lone-row form."""
    cnt = C.c_int32(0)
    solver._chk(solver._L.altro_batch_get_wave_cycles(solver.h, None, 0, C.byref(cnt)))
    out = np.zeros(cnt.value, dtype=np.int64)
    solver._chk(solver._L.altro_batch_get_wave_cycles(solver.h, out.ctypes.data_as(C.POINTER(C.c_int64)), cnt.value, C.byref(cnt)))
    return out.reshape(-1, 16)


def wave_passes(solver):
    """(waves, 8) per wave of the last solve launch (16-lane kernels): column 0 (every build) backward passes run in the
    pair form; columns 1-3 (shipped build, box-only kernels) the open-loop rollouts, closed-loop rollouts and first-order
    sweeps that ran in the four-row form: bits 0-15 the ones that took the wave-uniform variant, the bits above the ones
    in the generic form.  The -DALTRO_PHASE_STAMPS build fills instead 1-3 four-row passes with 2, 3 and 4 rows needing
    them, 4-6 their ticks, 7 the ticks of the pair passes."""
    cnt = C.c_int32(0)
    solver._chk(solver._L.altro_batch_get_wave_passes(solver.h, None, 0, C.byref(cnt)))
    out = np.zeros(cnt.value, dtype=np.int64)
    solver._chk(solver._L.altro_batch_get_wave_passes(solver.h, out.ctypes.data_as(C.POINTER(C.c_int64)), cnt.value, C.byref(cnt)))
    return out.reshape(-1, 8)


def solve_counters(solver):
    """(solves, iLQR iterations, SOLVE_SUCCEEDED count) per instance since timing_reset."""
    i64 = C.POINTER(C.c_int64)
    a = [np.zeros(solver.B, dtype=np.int64) for _ in range(3)]
    solver._chk(solver._L.altro_batch_get_solve_counters(solver.h, *[x.ctypes.data_as(i64) for x in a]))
    return tuple(a)


def update_constraint_data(solver, con, A=None, b=None):
    """In-place mutation of a constraint's (per-knot) data: grasp_mpc_helpers.jl:46-55.  With GPU tensors (A, b in the
    shape the constraint was given with; either may be None) the rows are written on the device, stream-ordered
    (altro_batch_update_constraint_data_dev)."""
    if _on_gpu(A) or _on_gpu(b):
        if not ((A is None or _on_gpu(A)) and (b is None or _on_gpu(b))):
            raise ValueError("update_constraint_data: A and b must both be GPU tensors (or None), or neither")
        with _bracket(solver):
            return _update_constraint_data_dev(solver, con, A, b)
    solver._chk(solver._L.altro_batch_update_constraint_data(
        solver.h, solver.con_ids[con], _p(_c(A)) if A is not None else None, _p(_c(b)) if b is not None else None))


def con_data_shape(solver, con):
    """shape of the A a LINEAR / SOC constraint of the problem was given with (b: the same without the last dimension)"""
    c, first, last = solver.prob.constraints.items[con]
    if isinstance(c, BoundConstraint):
        raise AltroError(_lib.ERR_INVALID_ARG, "update_constraint_data: a BoundConstraint has no A, b (set_bounds)")
    return tuple(np.shape(c.A))


def _update_constraint_data_dev(solver, con, A, b):
    shape = con_data_shape(solver, con)
    if A is not None:
        check_device_tensor(A, shape, solver.device, "A")
    if b is not None:
        check_device_tensor(b, shape[:-1], solver.device, "b")
    solver._chk(solver._L.altro_batch_update_constraint_data_dev(solver.h, solver.con_ids[con], _addr(A), _addr(b)))


def alpha_trace(solver):
    """Accepted line-search step of the first TRACE_LEN iLQR iterations of the last solve."""
    a = np.empty((solver.B, _lib.TRACE_LEN))
    solver._chk(solver._L.altro_batch_get_alpha_trace(solver.h, _p(a)))
    return a


def gains(solver):
    """(K, d) of the last backward pass: K (B, N-1, m, n), d (B, N-1, m)."""
    K = np.empty((solver.B, solver.N - 1, solver.n, solver.m))
    d = np.empty((solver.B, solver.N - 1, solver.m))
    solver._chk(solver._L.altro_batch_get_gains(solver.h, _p(K), _p(d)))
    return np.swapaxes(K, -1, -2).copy(), d


def gain_factors(solver):
    """Factors of Quu = L D L' kept with the gains (16-lane kernels): (B, N-1, m, m), 1 / D on the diagonal, L below it."""
    F = np.empty((solver.B, solver.N - 1, solver.m, solver.m))
    solver._chk(solver._L.altro_batch_get_gain_factors(solver.h, _p(F)))
    return F


def _eval_policy_dev(solver, x, knot=None, clamp=True, out=None, fb=None):
    import torch
    dev = torch.device("cuda", solver.device)
    check_device_tensor(x, (solver.B, solver.n), solver.device, "x")
    if knot is not None:
        check_device_tensor(knot, (solver.B,), solver.device, "knot", dtype="torch.int32")
    if out is None:
        out = torch.empty((solver.B, solver.m), dtype=torch.float64, device=dev)
    check_device_tensor(out, (solver.B, solver.m), solver.device, "out")
    if fb is not None:
        check_device_tensor(fb, (solver.B,), solver.device, "fb", dtype="torch.int32")
    solver._chk(solver._L.altro_batch_eval_policy_dev(solver.h, _addr(x), _addr(knot), int(bool(clamp)), _addr(out), _addr(fb)))
    return out


def eval_policy(solver, x, knot=None, clamp=True, out=None, fb=None):
    """The feedback policy of the last solve, u = u_k + K_k (x - x_k), saturated at the BOX when clamp (altro_batch_eval_policy
    / _dev): what drives the plant between two solver ticks.  x (B, n) measured states, knot (B,) the knot of the current
    horizon each instance is at (None: knot 0).  With GPU tensors (x float64, knot int32) the call is stream-ordered behind
    the solve and nothing synchronises; out (B, m) and fb (B,) int32 are tensors to write into (out defaults to a new one).
    With numpy the host twin runs (the same bytes), and fb may be a (B,) int32 array to fill.  fb: 1 feedback applied, 0 no
    valid stored gains (u = u_k), -1 knot outside 0 .. N-2 (device path only: the row of u is left as it was; the host path
    raises).  Returns u."""
    if _gpu_form("eval_policy: x, knot, out and fb", (x, knot, out, fb), nreq=1):
        with _bracket(solver):
            return _eval_policy_dev(solver, x, knot, clamp, out, fb)
    x = _c(x)
    assert x.shape == (solver.B, solver.n)
    kn = None if knot is None else _clock_i32(knot, solver.B, "knot")
    if out is None:
        out = np.empty((solver.B, solver.m))
    _check_np_out("eval_policy", "out", out, (solver.B, solver.m))
    if fb is not None:
        _check_np_out("eval_policy", "fb", fb, (solver.B,), np.int32)
    solver._chk(solver._L.altro_batch_eval_policy(solver.h, _p(x), None if kn is None else kn.ctypes.data_as(_IP), int(bool(clamp)),
                                                  _p(out), None if fb is None else fb.ctypes.data_as(_IP)))
    return out


def get_gains_dev(solver, K=None, d=None):
    """altro_batch_get_gains into GPU tensors, stream-ordered and without a host synchronisation: K (B, N-1, m, n) in natural
    (row, col) indexing, i.e. STORED column-major like a dynamics tensor (the transpose(-1, -2) of a contiguous (B, N-1, n, m)
    tensor), d (B, N-1, m).  With neither given both are allocated; with one given only that one is written.  Returns (K, d)."""
    import torch
    if K is None and d is None:
        dev = torch.device("cuda", solver.device)
        K = torch.empty((solver.B, solver.N - 1, solver.n, solver.m), dtype=torch.float64, device=dev).transpose(-1, -2)
        d = torch.empty((solver.B, solver.N - 1, solver.m), dtype=torch.float64, device=dev)
    if K is not None:
        check_device_tensor(K, (solver.B, solver.N - 1, solver.m, solver.n), solver.device, "K", colmajor=True)
    if d is not None:
        check_device_tensor(d, (solver.B, solver.N - 1, solver.m), solver.device, "d")
    with _bracket(solver):
        solver._chk(solver._L.altro_batch_get_gains_dev(solver.h, _addr(K), _addr(d)))
    return K, d


def _evaluate_shapes(solver, U, X, x0, name):
    """(ncand, shape of the outputs, shape U / X / x0 must have): U (B, N-1, m) is one candidate per instance with (B,) outputs,
    U (B, ncand, N-1, m) gives (B, ncand); U None (the solver's own trajectory) is one candidate"""
    B, N, n, m = solver.B, solver.N, solver.n, solver.m
    if U is None:
        if X is not None or x0 is not None:
            raise ValueError(f"{name}: X and x0 need U (U None scores the solver's own trajectory)")
        return 1, (B,), None, None, None
    shp = tuple(int(k) for k in U.shape)
    if len(shp) == 3:
        ncand, lead = 1, (B,)
    elif len(shp) == 4 and shp[1] >= 1:
        ncand, lead = shp[1], (B, shp[1])
    else:
        raise ValueError(f"{name}: U: shape {shp}, expected ({B}, {N - 1}, {m}) or ({B}, ncand, {N - 1}, {m})")
    if X is not None and x0 is not None:
        raise ValueError(f"{name}: x0 belongs to the rollout form: it must be None when X is given")
    return ncand, lead, lead + (N - 1, m), lead + (N, n), (B, n)


def _evaluate_dev(solver, U=None, X=None, x0=None, out=None, Xout=None):
    """device form of evaluate: every tensor is validated (shape, dtype, strides, device) before the library is called"""
    import torch
    dev = torch.device("cuda", solver.device)
    ncand, lead, su, sx, s0 = _evaluate_shapes(solver, U, X, x0, "evaluate")
    if U is not None:
        check_device_tensor(U, su, solver.device, "U")
    if X is not None:
        check_device_tensor(X, sx, solver.device, "X")
        if Xout is not None:
            raise ValueError("evaluate: Xout belongs to the rollout form: it must be None when X is given")
    if x0 is not None:
        check_device_tensor(x0, s0, solver.device, "x0")
    if Xout is not None:
        if U is None:
            raise ValueError("evaluate: Xout needs U")
        check_device_tensor(Xout, sx, solver.device, "Xout")
    if out is None:
        out = tuple(torch.empty(lead, dtype=torch.float64, device=dev) for _ in range(3))
    out = tuple(out)
    if len(out) != 3 or all(o is None for o in out):
        raise ValueError("evaluate: out is (J, c_max, defect); any may be None, not all")
    for o, nm in zip(out, ("J", "c_max", "defect")):
        if o is not None:
            check_device_tensor(o, lead, solver.device, nm)
    solver._chk(solver._L.altro_batch_evaluate_dev(solver.h, ncand, _addr(U), _addr(X), _addr(x0), _addr(out[0]), _addr(out[1]),
                                                   _addr(out[2]), _addr(Xout)))
    return out


def evaluate(solver, U=None, X=None, x0=None, out=None, Xout=None):
    """Score trajectories the solver did not make against the problem its next solve would see (altro_batch_evaluate / _dev):
    returns (J, c_max, defect) -- the plain tracking cost without augmented-Lagrangian terms, the maximum constraint violation
    and the dynamics defect max_k |A x_k + B u_k + f - x_{k+1}|_inf.
    U (B, N-1, m): one candidate per instance, outputs (B,); U (B, ncand, N-1, m): outputs (B, ncand).  With X None the states
    are rolled out from x0 (B, n) (None: the solver's initial state), written to Xout (shape of U with (N, n)) when given, and
    defect is +0; with X (the shape of Xout) the pair is scored as it is.  U None: the solver's own trajectory.
    With GPU tensors (float64, contiguous) the call is stream-ordered and nothing synchronises; out = (J, c_max, defect) are
    tensors to write into (any may be None, not all; default: three new ones).  With numpy the host twin runs: the same bytes."""
    args = (U, X, x0, Xout) + (tuple(out) if out is not None else ())
    if _gpu_form("evaluate: U, X, x0, Xout and out", args):
        with _bracket(solver):
            return _evaluate_dev(solver, U, X, x0, out, Xout)
    U = None if U is None else _c(U)
    X = None if X is None else _c(X)
    x0 = None if x0 is None else _c(x0)
    ncand, lead, su, sx, s0 = _evaluate_shapes(solver, U, X, x0, "evaluate")
    for a, shp, nm in ((U, su, "U"), (X, sx, "X"), (x0, s0, "x0")):
        if a is not None and a.shape != shp:
            raise ValueError(f"evaluate: {nm}: shape {a.shape}, expected {shp}")
    if Xout is not None and (U is None or X is not None):
        raise ValueError("evaluate: Xout belongs to the rollout form (U given, X None)")
    if out is None:
        out = tuple(np.empty(lead) for _ in range(3))
    out = tuple(out)
    if len(out) != 3 or all(o is None for o in out):
        raise ValueError("evaluate: out is (J, c_max, defect); any may be None, not all")
    for o, shp, nm in tuple(zip(out, (lead,) * 3, ("J", "c_max", "defect"))) + ((Xout, sx, "Xout"),):
        if o is not None:
            _check_np_out("evaluate", nm, o, shp)
    solver._chk(solver._L.altro_batch_evaluate(solver.h, ncand, _p(U), _p(X), _p(x0), _p(out[0]), _p(out[1]), _p(out[2]), _p(Xout)))
    return out


def _evaluate_grad_shapes(solver, U, name):
    """(ncand, shapes of J and P / U and gU / gx0 / Xout / x0) from U, by evaluate's rule for U"""
    if U is None:
        raise ValueError(f"{name}: U is required")
    ncand, lead, su, sx, s0 = _evaluate_shapes(solver, U, None, None, name)
    return ncand, lead, su, lead + (solver.n,), sx, s0


def _evaluate_grad_out(out, name):
    out = tuple(out)
    if len(out) != 4 or all(o is None for o in out):
        raise ValueError(f"{name}: out is (J, P, gU, gx0); any may be None, not all")
    return out


def _check_rho(rho, name):
    rho = float(rho)
    if not (rho >= 0.0) or rho == float("inf"):
        raise ValueError(f"{name}: rho must be finite and not negative")
    return rho


def _evaluate_grad_dev(solver, U, x0=None, rho=0.0, out=None, Xout=None):
    """device form of evaluate_grad: every tensor is validated (shape, dtype, strides, device) before the library is called"""
    import torch
    dev = torch.device("cuda", solver.device)
    ncand, lead, su, sg, sx, s0 = _evaluate_grad_shapes(solver, U, "evaluate_grad")
    rho = _check_rho(rho, "evaluate_grad")
    check_device_tensor(U, su, solver.device, "U")
    if x0 is not None:
        check_device_tensor(x0, s0, solver.device, "x0")
    if Xout is not None:
        check_device_tensor(Xout, sx, solver.device, "Xout")
    shapes = (lead, lead, su, sg)
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float64, device=dev) for s in shapes)
    out = _evaluate_grad_out(out, "evaluate_grad")
    for o, s, nm in zip(out, shapes, ("J", "P", "gU", "gx0")):
        if o is not None:
            check_device_tensor(o, s, solver.device, nm)
    solver._chk(solver._L.altro_batch_evaluate_grad_dev(solver.h, ncand, _addr(U), _addr(x0), rho, _addr(out[0]), _addr(out[1]),
                                                        _addr(out[2]), _addr(out[3]), _addr(Xout)))
    return out


def evaluate_grad(solver, U, x0=None, rho=0.0, out=None, Xout=None):
    """The merit of control sequences the solver did not make and its gradient, against the problem the next solve would see
    (altro_batch_evaluate_grad / _dev): returns (J, P, gU, gx0) -- the plain tracking cost evaluate returns, the penalty
    P = 1/2 sum r^2 of the signed constraint residuals (BOX, LINEAR, SOC: the distance of every row to its feasible set), and
    the gradient of M = J + rho P with respect to the controls and to the initial state, by one rollout and one costate sweep.
    U (B, N-1, m): one candidate per instance, J and P (B,), gx0 (B, n); U (B, ncand, N-1, m): J and P (B, ncand), gx0
    (B, ncand, n); gU has the shape of U.  The states are rolled out from x0 (B, n) (None: the solver's initial state) and
    written to Xout (shape of U with (N, n)) when given.  With rho = 0 the gradient is that of J alone.
    With GPU tensors (float64, contiguous) the call is stream-ordered and nothing synchronises; out = (J, P, gU, gx0) are
    tensors to write into (any may be None, not all; default: four new ones).  With numpy the host twin runs: the same bytes."""
    args = (U, x0, Xout) + (tuple(out) if out is not None else ())
    if _gpu_form("evaluate_grad: U, x0, Xout and out", args):
        with _bracket(solver):
            return _evaluate_grad_dev(solver, U, x0, rho, out, Xout)
    U = None if U is None else _c(U)
    x0 = None if x0 is None else _c(x0)
    ncand, lead, su, sg, sx, s0 = _evaluate_grad_shapes(solver, U, "evaluate_grad")
    rho = _check_rho(rho, "evaluate_grad")
    for a, shp, nm in ((U, su, "U"), (x0, s0, "x0")):
        if a is not None and a.shape != shp:
            raise ValueError(f"evaluate_grad: {nm}: shape {a.shape}, expected {shp}")
    shapes = (lead, lead, su, sg)
    if out is None:
        out = tuple(np.empty(s) for s in shapes)
    out = _evaluate_grad_out(out, "evaluate_grad")
    for o, shp, nm in tuple(zip(out, shapes, ("J", "P", "gU", "gx0"))) + ((Xout, sx, "Xout"),):
        if o is not None:
            _check_np_out("evaluate_grad", nm, o, shp)
    solver._chk(solver._L.altro_batch_evaluate_grad(solver.h, ncand, _p(U), _p(x0), rho, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]),
                                                    _p(Xout)))
    return out


_merit_fn = None


def _merit_function():
    """the torch.autograd.Function behind merit, made on first use (the package imports without torch)"""
    global _merit_fn
    if _merit_fn is not None:
        return _merit_fn
    import torch
    from torch.autograd.function import once_differentiable

    class Merit(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, U, x0, rho):
            J, P, gU, gx0 = evaluate_grad(solver, U.detach(), None if x0 is None else x0.detach(), rho)
            ctx.save_for_backward(J, P, gU, gx0)
            return J + rho * P

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_out):
            J, P, gU, gx0 = ctx.saved_tensors
            dU = grad_out[..., None, None] * gU if ctx.needs_input_grad[1] else None
            dx0 = None
            if ctx.needs_input_grad[2]:
                dx0 = grad_out[..., None] * gx0
                if dx0.dim() == 3:
                    dx0 = dx0.sum(dim=1)
            return None, dU, dx0, None

    _merit_fn = Merit
    return Merit


def merit(solver, U, x0=None, rho=0.0):
    """M = J + rho P of evaluate_grad as a tensor torch can differentiate once: U (and x0, when it is a tensor that requires
    grad) are GPU tensors, M has the shape of J and a grad_fn.  The single device call happens in forward; backward hands
    grad[..., None, None] * gU to U and grad[..., None] * gx0, summed over the candidates, to x0."""
    if not _on_gpu(U) or not (x0 is None or _on_gpu(x0)):
        raise ValueError("merit: U (and x0, if given) must be GPU tensors")
    return _merit_function().apply(solver, U, x0, _check_rho(rho, "merit"))


def _evaluate_al_shapes(solver, U, name):
    """(ncand, shape of x0, {output name: shape}) from U by evaluate's rule; U None: the controls the solver holds, one candidate"""
    B, N, n, m = solver.B, solver.N, solver.n, solver.m
    if U is None:
        ncand, lead = 1, (B,)
    else:
        ncand, lead = _evaluate_shapes(solver, U, None, None, name)[:2]
    su, sx = lead + (N - 1, m), lead + (N, n)
    shapes = dict(LA=lead, J=lead, gU=su, gx0=lead + (n,), gXref=sx, gUref=su, gQ=lead + (n,), gQf=lead + (n,), gR=lead + (m,),
                  gzmin=lead + (n + m,), gzmax=lead + (n + m,), Xout=sx)
    return ncand, su, (B, n), shapes


def _evaluate_al_out(out, shapes, make, name):
    """the dict of outputs: out None -> all twelve made new; a sequence of names -> those made new; a dict name -> array (None
    entries and missing names are skipped)"""
    if out is None:
        out = tuple(_lib.AL_OUT_FIELDS)
    if not isinstance(out, dict):
        names = tuple(out)
        if any(not isinstance(k, str) for k in names):
            raise ValueError(f"{name}: out is a dict of arrays or a sequence of names out of {_lib.AL_OUT_FIELDS}")
        out = {k: None for k in names}
        fill = True
    else:
        fill = False
    unknown = [k for k in out if k not in shapes]
    if unknown:
        raise ValueError(f"{name}: out: unknown output {unknown[0]!r}; the outputs are {_lib.AL_OUT_FIELDS}")
    res = {k: (make(shapes[k]) if fill else out[k]) for k in _lib.AL_OUT_FIELDS if k in out and (fill or out[k] is not None)}
    if not any(k != "Xout" for k in res):
        raise ValueError(f"{name}: out needs at least one output other than Xout")
    return res


def _al_struct(res, addr):
    return _lib.ALOut(**{k: (addr(res[k]) if k in res else None) for k in _lib.AL_OUT_FIELDS})


def evaluate_al(solver, U=None, x0=None, out=None):
    """The solver's own augmented Lagrangian L_A(U; lambda, mu) -- the function a solve minimises, with the duals and the penalty
    the solver holds -- of control sequences, its gradient and its partial derivatives with respect to the problem data
    (altro_batch_evaluate_al / _dev), as a dict: LA, J; gU = dL_A/dU and gx0 = dL_A/dx0 by one costate sweep; gXref, gUref; gQ, gQf,
    gR (with respect to the arguments of the tracking objective); gzmin, gzmax (the shadow prices of the box bounds); Xout (the
    states).  U None: the controls the solver holds -- after a solve gU is then the stationarity residual the solve stopped at,
    and by the envelope theorem the other derivatives are those of the optimal cost, up to that residual.  U (B, N-1, m) or
    (B, ncand, N-1, m) as in evaluate; x0 (B, n), None: the solver's initial state.  out: None (all twelve outputs), a sequence
    of names (those, made new), or a dict name -> array to write into; an output left out costs nothing.  With GPU tensors
    (float64, contiguous) the call is stream-ordered and nothing synchronises; with numpy the host twin runs: the same bytes.
    Nothing the solver holds changes."""
    given = (U, x0) + (tuple(out.values()) if isinstance(out, dict) else ())
    ncand, su, s0, shapes = _evaluate_al_shapes(solver, U, "evaluate_al")
    if _gpu_form("evaluate_al: U, x0 and the arrays of out", given):
        import torch
        dev = torch.device("cuda", solver.device)
        if U is not None:
            check_device_tensor(U, su, solver.device, "U")
        if x0 is not None:
            check_device_tensor(x0, s0, solver.device, "x0")
        res = _evaluate_al_out(out, shapes, lambda s: torch.empty(s, dtype=torch.float64, device=dev), "evaluate_al")
        for k, t in res.items():
            if not _on_gpu(t):
                raise ValueError(f"evaluate_al: {k} must be a GPU tensor")
            check_device_tensor(t, shapes[k], solver.device, k)
        st = _al_struct(res, lambda t: t.data_ptr())
        with _bracket(solver):
            solver._chk(solver._L.altro_batch_evaluate_al_dev(solver.h, ncand, _addr(U), _addr(x0), C.byref(st)))
        return res
    U = None if U is None else _c(U)
    x0 = None if x0 is None else _c(x0)
    for a, shp, nm in ((U, su, "U"), (x0, s0, "x0")):
        if a is not None and a.shape != shp:
            raise ValueError(f"evaluate_al: {nm}: shape {a.shape}, expected {shp}")
    res = _evaluate_al_out(out, shapes, np.empty, "evaluate_al")
    for k, a in res.items():
        _check_np_out("evaluate_al", k, a, shapes[k])
    st = _al_struct(res, lambda a: a.ctypes.data)
    solver._chk(solver._L.altro_batch_evaluate_al(solver.h, ncand, _p(U), _p(x0), C.byref(st)))
    return res


def penalty(solver, out=None):
    """the penalty mu of every instance, (B,): the one evaluate_al uses (altro_batch_get_penalty); out = a GPU tensor of that
    shape: written on the device, stream-ordered, and returned"""
    if out is not None:
        if not _on_gpu(out):
            raise ValueError("penalty: out must be a GPU tensor")
        check_device_tensor(out, (solver.B,), solver.device, "out")
        with _bracket(solver):
            solver._chk(solver._L.altro_batch_get_penalty_dev(solver.h, _addr(out)))
        return out
    mu = np.empty(solver.B)
    solver._chk(solver._L.altro_batch_get_penalty(solver.h, _p(mu)))
    return mu


_optimal_cost_fn = None


def _optimal_cost_function():
    """the torch.autograd.Function behind optimal_cost, made on first use (the package imports without torch)"""
    global _optimal_cost_fn
    if _optimal_cost_fn is not None:
        return _optimal_cost_fn
    import torch
    from torch.autograd.function import once_differentiable

    class OptimalCost(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, x0, Xref, Uref):
            # all three validated before the first setter: a refused tensor leaves the solver as it was
            check_device_tensor(x0, (solver.B, solver.n), solver.device, "x0")
            check_device_tensor(Xref, (solver.B, solver.N, solver.n), solver.device, "Xref")
            check_device_tensor(Uref, (solver.B, solver.N - 1, solver.m), solver.device, "Uref")
            with _bracket(solver):
                _set_initial_state_dev(solver, x0.detach())
                _update_trajectory_dev(solver, Xref.detach(), Uref.detach())
                solver._chk(solver._L.altro_batch_solve_async(solver.h))
            r = evaluate_al(solver, out={k: torch.empty(s, dtype=torch.float64, device=x0.device) for k, s in
                                         (("LA", (solver.B,)), ("gx0", (solver.B, solver.n)), ("gXref", (solver.B, solver.N, solver.n)),
                                          ("gUref", (solver.B, solver.N - 1, solver.m)))})
            ctx.save_for_backward(r["gx0"], r["gXref"], r["gUref"])
            return r["LA"]

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_out):
            gx0, gXref, gUref = ctx.saved_tensors
            need = ctx.needs_input_grad
            return (None, grad_out[:, None] * gx0 if need[1] else None, grad_out[:, None, None] * gXref if need[2] else None,
                    grad_out[:, None, None] * gUref if need[3] else None)

    _optimal_cost_fn = OptimalCost
    return OptimalCost


def optimal_cost(solver, x0, Xref, Uref):
    """The cost a solve ends at as a tensor torch can differentiate once with respect to what a learned component produces: the
    initial state x0 (B, n) and the reference Xref (B, N, n), Uref (B, N-1, m): GPU tensors on the solver's device, float64,
    contiguous, of exactly these shapes (nothing is cast, copied or moved; a tensor that is not is refused with ValueError before
    anything is installed, the solver unchanged).  Forward CHANGES THE SOLVER: it
    installs the three on it (the device setters), solves, and returns L_A (B,) of the controls the solve left, with the duals
    and the penalty it left (evaluate_al with U None); all of it stream-ordered.  Backward hands grad * gx0, grad * gXref and
    grad * gUref back.  By the envelope theorem these are the derivatives of the optimal cost min_U L_A, EXACT UP TO THE
    STATIONARITY RESIDUAL the solve stopped at (gU of evaluate_al(solver): the tolerances of the solver bound it); the duals
    and the penalty are held fixed, no KKT system is solved."""
    if not (_on_gpu(x0) and _on_gpu(Xref) and _on_gpu(Uref)):
        raise ValueError("optimal_cost: x0, Xref and Uref must be GPU tensors")
    return _optimal_cost_function().apply(solver, x0, Xref, Uref)


def get_gain_factors_dev(solver, out=None):
    """altro_batch_get_gain_factors into a GPU tensor (B, N-1, m, m), stream-ordered and without a host synchronisation:
    1 / D on the diagonal, L below it, 0 above (Quu = L D L').  Also on the one-wave-per-instance kernels with m <= 16, where
    gain_factors is not available.  out: the tensor to write into (default: a new one); returned."""
    import torch
    shp = (solver.B, solver.N - 1, solver.m, solver.m)
    if out is None:
        out = torch.empty(shp, dtype=torch.float64, device=torch.device("cuda", solver.device))
    if not _on_gpu(out):
        raise ValueError("get_gain_factors_dev: out must be a GPU tensor")
    check_device_tensor(out, shp, solver.device, "out")
    with _bracket(solver):
        solver._chk(solver._L.altro_batch_get_gain_factors_dev(solver.h, _addr(out)))
    return out


def _sens_kinds(solver):
    """the trailing shape of every array of solution_vjp / solution_jvp"""
    sx, su, s0 = (solver.N, solver.n), (solver.N - 1, solver.m), (solver.n,)
    return dict(gX=sx, gU=su, gx0=s0, gXref=sx, gUref=su, vx0=s0, vXref=sx, vUref=su, dX=sx, dU=su)


def _sens_lead(solver, arrs, name):
    """(nseed, leading shape) from the arrays given ({name: array}): (B,) + trailing shape is one seed per instance (a seed
    axis is added for the call and dropped from the results), (B, nseed) + trailing shape is nseed of them; all must agree"""
    kinds = _sens_kinds(solver)
    lead = None
    for k, a in arrs.items():
        if a is None:
            continue
        shp, tail = tuple(int(v) for v in a.shape), kinds[k]
        ok = len(shp) in (1 + len(tail), 2 + len(tail)) and shp[len(shp) - len(tail):] == tail and shp[0] == solver.B
        if not ok:
            raise ValueError(f"{name}: {k}: shape {shp}, expected {(solver.B,) + tail} or {(solver.B, 'nseed') + tail}")
        ld = shp[:len(shp) - len(tail)]
        if len(ld) == 2 and ld[1] < 1:
            raise ValueError(f"{name}: {k}: nseed must be at least 1")
        if lead is not None and ld != lead:
            raise ValueError(f"{name}: {k}: leading shape {ld}, the other arrays have {lead}")
        lead = ld
    return (lead[1] if len(lead) == 2 else 1), lead


def _sens_out(out, names, name):
    """the outputs asked for: None -> all of `names`; a sequence of names; a dict name -> array to write into ('fb' may be among
    them).  Returns ({name: array or None}, fb or None)"""
    if out is None:
        out = names
    if not isinstance(out, dict):
        out = {k: None for k in out}
    out = dict(out)
    fb = out.pop("fb", None)
    unknown = [k for k in out if k not in names]
    if unknown:
        raise ValueError(f"{name}: out: unknown output {unknown[0]!r}; the outputs are {names} and 'fb'")
    if not out:
        raise ValueError(f"{name}: out needs at least one of {names}")
    return out, fb


def _solution_sens(solver, name, ins, out, names, call):
    """what solution_vjp and solution_jvp share: shapes, the device / host split, the outputs.  call(dev, nseed, ins, res, fb)
    makes the C call from {name: array or None} dicts whose arrays are addressed by the function it is given."""
    if all(a is None for a in ins.values()):
        raise ValueError(f"{name}: at least one of {tuple(ins)} is required")
    want, fb = _sens_out(out, names, name)
    given = tuple(ins.values()) + tuple(want.values()) + (fb,)
    gpu = _gpu_form(f"{name}: the inputs and the arrays of out", given)
    if not gpu:
        ins = {k: (None if a is None else _c(a)) for k, a in ins.items()}
    nseed, lead = _sens_lead(solver, ins, name)
    kinds = _sens_kinds(solver)
    if gpu:
        import torch
        dev = torch.device("cuda", solver.device)
        for k, a in ins.items():
            if a is not None:
                check_device_tensor(a, lead + kinds[k], solver.device, k)
        res = {k: (torch.empty(lead + kinds[k], dtype=torch.float64, device=dev) if a is None else a) for k, a in want.items()}
        for k, t in res.items():
            check_device_tensor(t, lead + kinds[k], solver.device, k)
        if fb is None:
            fb = torch.empty((solver.B,), dtype=torch.int32, device=dev)
        check_device_tensor(fb, (solver.B,), solver.device, "fb", dtype="torch.int32")
        with _bracket(solver):
            solver._chk(call(True, nseed, ins, res, fb, lambda t: None if t is None else t.data_ptr()))
    else:
        res = {k: (np.empty(lead + kinds[k]) if a is None else a) for k, a in want.items()}
        for k, a in res.items():
            _check_np_out(name, k, a, lead + kinds[k])
        if fb is None:
            fb = np.empty(solver.B, dtype=np.int32)
        _check_np_out(name, "fb", fb, (solver.B,), np.int32)
        solver._chk(call(False, nseed, ins, res, fb, lambda a: None if a is None else a.ctypes.data))
    res["fb"] = fb
    return res


def solution_vjp(solver, gX=None, gU=None, out=None):
    """Reverse-mode sensitivity of the SOLUTION of the last solve through the stored gains (altro_batch_solution_vjp / _dev):
    for seeds gX = dl/dX* (B, N, n) and gU = dl/dU* (B, N-1, m) -- or (B, nseed, ...) for several seeds per instance; None is
    zero -- the gradients of l with respect to the initial state and the reference, as a dict: gx0 (B[, nseed], n), gXref,
    gUref (the shapes of gX, gU), and fb (B,) int32: 1 where the instance holds valid gains of an unregularised backward pass,
    0 where it does not -- every row of that instance is then NaN.  Exact for the minimiser of the augmented Lagrangian at the
    multipliers, penalty and active set of the stored pass.  out: None (all three), a sequence of names, or a
    dict name -> array to write into ('fb' too); an output left out costs nothing (gx0 alone runs one sweep and needs no factors
    of Quu).  With GPU tensors (float64, contiguous; fb int32) the call is stream-ordered and nothing synchronises; with numpy
    the host twin runs: the same bytes.  Nothing the solver holds changes."""
    def call(dev, nseed, ins, res, fb, addr):
        st = _lib.SensOut(**{k: addr(res.get(k)) for k in _lib.SENS_OUT_FIELDS})
        if dev:
            return solver._L.altro_batch_solution_vjp_dev(solver.h, nseed, addr(ins["gX"]), addr(ins["gU"]), C.byref(st), addr(fb))
        return solver._L.altro_batch_solution_vjp(solver.h, nseed, _p(ins["gX"]), _p(ins["gU"]), C.byref(st), fb.ctypes.data_as(_IP))
    return _solution_sens(solver, "solution_vjp", dict(gX=gX, gU=gU), out, _lib.SENS_OUT_FIELDS, call)


def solution_jvp(solver, vx0=None, vXref=None, vUref=None, out=None):
    """Forward-mode sensitivity of the SOLUTION of the last solve through the stored gains (altro_batch_solution_jvp / _dev):
    for tangents vx0 (B, n), vXref (B, N, n), vUref (B, N-1, m) -- or (B, nseed, ...); None is zero -- the directional
    derivatives of the solution, as a dict: dX, dU (the shapes of vXref, vUref) and fb as in solution_vjp.  vx0 = e_j alone
    gives dU[:, 0] = column j of the first gain.  out: None (both), a sequence of names, or a dict name -> array ('fb' too).
    GPU tensors: stream-ordered; numpy: the host twin, the same bytes.  Nothing the solver holds changes."""
    def call(dev, nseed, ins, res, fb, addr):
        if dev:
            return solver._L.altro_batch_solution_jvp_dev(solver.h, nseed, addr(ins["vx0"]), addr(ins["vXref"]), addr(ins["vUref"]),
                                                          addr(res.get("dX")), addr(res.get("dU")), addr(fb))
        return solver._L.altro_batch_solution_jvp(solver.h, nseed, _p(ins["vx0"]), _p(ins["vXref"]), _p(ins["vUref"]), _p(res.get("dX")),
                                                  _p(res.get("dU")), fb.ctypes.data_as(_IP))
    return _solution_sens(solver, "solution_jvp", dict(vx0=vx0, vXref=vXref, vUref=vUref), out, ("dX", "dU"), call)


def solution_vjp_data(solver, gX=None, gU=None, per_knot=False, out=None):
    """Reverse-mode sensitivity of the SOLUTION of the last solve with respect to the problem data
    (altro_batch_solution_vjp_data / _dev): for seeds gX = dl/dX* (B, N, n) and gU = dl/dU* (B, N-1, m) -- or
    (B, nseed, ...); None is zero -- the gradients of l, as a dict: gQ, gQf (B[, nseed], n) and gR (.., m) with respect to the
    arguments of set_tracking_cost; gzmin, gzmax (.., n+m) with respect to the box bounds; gA (.., n, n), gB (.., n, m), gf (.., n)
    with respect to the dynamics, summed over the knots, or with per_knot=True one block per knot, (.., N-1, n, n) and so on; and
    fb (B,) int32: 1 where solution_vjp reports 1 and the instance still holds the penalty of the stored pass, else 0 and every
    row of the instance is NaN.  gA[..., i, j] = dl/dA[i, j]; the blocks are stored column-major, as set_dynamics_dev takes them, so
    gA and gB are the transpose(-1, -2) of contiguous arrays (one given in out must be such a view).  Exact for the
    minimiser of the augmented Lagrangian at the multipliers, penalty and active set of the stored pass.  gzmin, gzmax, gA, gB, gf
    need a box-only problem (AltroError UNSUPPORTED otherwise); gQ, gQf, gR do not.  out: None (all eight), a sequence of names,
    or a dict name -> array to write into ('fb' too); gQ, gQf, gR alone never read the active set.  GPU tensors: stream-ordered,
    nothing synchronises; numpy: the host twin, the same bytes.  Nothing the solver holds changes."""
    name = "solution_vjp_data"
    n, m, N = solver.n, solver.m, solver.N
    if gX is None and gU is None:
        raise ValueError(f"{name}: at least one of ('gX', 'gU') is required")
    want, fb = _sens_out(out, _lib.SENS_DATA_OUT_FIELDS, name)
    ins = dict(gX=gX, gU=gU)
    gpu = _gpu_form(f"{name}: the inputs and the arrays of out", tuple(ins.values()) + tuple(want.values()) + (fb,))
    if not gpu:
        ins = {k: (None if a is None else _c(a)) for k, a in ins.items()}
    nseed, lead = _sens_lead(solver, ins, name)
    kn = (N - 1,) if per_knot else ()
    tail = dict(gQ=(n,), gQf=(n,), gR=(m,), gzmin=(n + m,), gzmax=(n + m,), gA=kn + (n, n), gB=kn + (n, m), gf=kn + (n,))
    mats = ("gA", "gB")   # column-major blocks: an array given or returned is the transpose(-1, -2) of a contiguous one
    st = _lib.SensDataOut()
    if gpu:
        import torch
        dev = torch.device("cuda", solver.device)
        kinds = _sens_kinds(solver)
        for k, a in ins.items():
            if a is not None:
                check_device_tensor(a, lead + kinds[k], solver.device, k)
        new = lambda k: torch.empty(lead + tail[k][:-2] + tail[k][:-3:-1], dtype=torch.float64, device=dev).transpose(-1, -2) if k in mats else \
            torch.empty(lead + tail[k], dtype=torch.float64, device=dev)
        res = {k: (new(k) if a is None else a) for k, a in want.items()}
        for k, t in res.items():
            check_device_tensor(t, lead + tail[k], solver.device, k, colmajor=k in mats)
        if fb is None:
            fb = torch.empty((solver.B,), dtype=torch.int32, device=dev)
        check_device_tensor(fb, (solver.B,), solver.device, "fb", dtype="torch.int32")
        for k, t in res.items():
            setattr(st, k, t.data_ptr())
        with _bracket(solver):
            solver._chk(solver._L.altro_batch_solution_vjp_data_dev(solver.h, nseed, _addr(ins["gX"]), _addr(ins["gU"]), 1 if per_knot else 0,
                                                                    C.byref(st), _addr(fb)))
    else:
        new = lambda k: np.swapaxes(np.empty(lead + tail[k][:-2] + tail[k][:-3:-1]), -1, -2) if k in mats else np.empty(lead + tail[k])
        res = {k: (new(k) if a is None else a) for k, a in want.items()}
        for k, a in res.items():
            if not (isinstance(a, np.ndarray) and a.shape == lead + tail[k]):
                raise ValueError(f"{name}: {k} must be a float64 array of shape {lead + tail[k]}")
            raw = np.swapaxes(a, -1, -2) if k in mats else a
            _check_np_out(name, k + (" (transposed: the blocks are column-major)" if k in mats else ""), raw, raw.shape)
            setattr(st, k, raw.ctypes.data)
        if fb is None:
            fb = np.empty(solver.B, dtype=np.int32)
        _check_np_out(name, "fb", fb, (solver.B,), np.int32)
        solver._chk(solver._L.altro_batch_solution_vjp_data(solver.h, nseed, _p(ins["gX"]), _p(ins["gU"]), 1 if per_knot else 0, C.byref(st),
                                                            fb.ctypes.data_as(_IP)))
    res["fb"] = fb
    return res


def gain_active_set(solver, out=None):
    """The active set and the penalty of the backward pass that left the stored gains (altro_batch_get_gain_active_set / _dev), as a
    dict: codes (B, N, n+m) uint8 -- bit 0: the upper side of the element entered that pass's Hessian at the knot, bit 1: the
    lower side; the region of the piecewise-affine solution map the instance is in -- mu_pass (B,) and fb (B,) int32 (0: no valid
    gains of an unregularised pass at the penalty held; codes 0, mu_pass NaN).  out: None -> new GPU tensors; a dict name -> array
    to write into chooses the form: GPU tensors (stream-ordered) or numpy arrays (the host twin, the same bytes); "numpy" -> new
    numpy arrays.  Box-only problems (AltroError UNSUPPORTED otherwise).  Nothing the solver holds changes."""
    name = "gain_active_set"
    shp = dict(codes=(solver.B, solver.N, solver.n + solver.m), mu_pass=(solver.B,), fb=(solver.B,))
    if isinstance(out, str):
        if out != "numpy":
            raise ValueError(f"{name}: out: {out!r}; a dict of arrays, None or 'numpy'")
        out = dict(codes=np.empty(shp["codes"], dtype=np.uint8), mu_pass=np.empty(shp["mu_pass"]), fb=np.empty(shp["fb"], dtype=np.int32))
    out = dict(out or {})
    unknown = [k for k in out if k not in shp]
    if unknown:
        raise ValueError(f"{name}: out: unknown output {unknown[0]!r}; the outputs are ('codes', 'mu_pass', 'fb')")
    gpu = not out or _gpu_form(f"{name}: the arrays of out", tuple(out.values()))
    if gpu:
        import torch
        dev = torch.device("cuda", solver.device)
        if not out:
            out = dict(codes=None, mu_pass=None)
        if "codes" not in out and "mu_pass" not in out:
            raise ValueError(f"{name}: out needs 'codes' or 'mu_pass'")
        dt = dict(codes=torch.uint8, mu_pass=torch.float64, fb=torch.int32)
        out.setdefault("fb", None)
        res = {k: (torch.empty(shp[k], dtype=dt[k], device=dev) if a is None else a) for k, a in out.items()}
        for k, t in res.items():
            check_device_tensor(t, shp[k], solver.device, k, dtype=str(dt[k]))
        ptr = lambda k: res[k].data_ptr() if k in res else None
        with _bracket(solver):
            solver._chk(solver._L.altro_batch_get_gain_active_set_dev(solver.h, ptr("codes"), ptr("mu_pass"), ptr("fb")))
        return res
    if "codes" not in out and "mu_pass" not in out:
        raise ValueError(f"{name}: out needs 'codes' or 'mu_pass'")
    dt = dict(codes=np.uint8, mu_pass=np.float64, fb=np.int32)
    out.setdefault("fb", None)
    res = {k: (np.empty(shp[k], dtype=dt[k]) if a is None else a) for k, a in out.items()}
    for k, a in res.items():
        _check_np_out(name, k, a, shp[k], dt[k])
    cp = lambda k, t: res[k].ctypes.data_as(t) if k in res else None
    solver._chk(solver._L.altro_batch_get_gain_active_set(solver.h, cp("codes", C.POINTER(C.c_uint8)), cp("mu_pass", _DP), cp("fb", _IP)))
    return res


CTG_OUTPUTS = _lib.CTG_OUT_FIELDS + ("fb",)


def _cost_to_go_args(solver, out):
    """({name: array or None} in the order of CTG_OUTPUTS, {name: shape}); refuses here what the library would refuse"""
    B, N, n = solver.B, solver.N, solver.n
    shp = dict(P0=(B, n, n), p0=(B, n), v0=(B,), P=(B, N, n, n), p=(B, N, n), v=(B, N), fb=(B,))
    if out is None:
        out = ("P0", "p0", "v0", "fb")
    if not isinstance(out, dict):
        if isinstance(out, str) or not all(isinstance(k, str) for k in out):
            raise ValueError(f"cost_to_go: out is a sequence of names or a dict name -> array; the outputs are {CTG_OUTPUTS}")
        out = {k: None for k in out}
    unknown = [k for k in out if k not in shp]
    if unknown:
        raise ValueError(f"cost_to_go: out: unknown output {unknown[0]!r}; the outputs are {CTG_OUTPUTS}")
    if not any(k in out for k in _lib.CTG_OUT_FIELDS):
        raise ValueError(f"cost_to_go: out needs at least one of {_lib.CTG_OUT_FIELDS}")
    return {k: out[k] for k in CTG_OUTPUTS if k in out}, shp


def _cost_to_go_dev(solver, penalty=False, out=None):
    """device form of cost_to_go: every tensor is validated (shape, dtype, strides, device) before the library is called; an
    output named without an array gets a new tensor"""
    out, shp = _cost_to_go_args(solver, out)
    dt = lambda k: "torch.int32" if k == "fb" else "torch.float64"
    if any(a is None for a in out.values()):
        import torch
        dev = torch.device("cuda", solver.device)
        out = {k: (torch.empty(shp[k], dtype=torch.int32 if k == "fb" else torch.float64, device=dev) if a is None else a) for k, a in out.items()}
    for k, t in out.items():
        check_device_tensor(t, shp[k], solver.device, k, dtype=dt(k))
    st = _lib.CtgOut()
    for k in _lib.CTG_OUT_FIELDS:
        if k in out:
            setattr(st, k, out[k].data_ptr())
    solver._chk(solver._L.altro_batch_cost_to_go_dev(solver.h, 1 if penalty else 0, C.byref(st), _addr(out.get("fb"))))
    return out


def cost_to_go(solver, penalty=False, out=None):
    """The quadratic cost-to-go of the stored policy around the trajectory the solver holds (altro_batch_cost_to_go / _dev,
    DESIGN.md 7x):  V_k(x) = v_k + p_k'(x - xbar_k) + 1/2 (x - xbar_k)' P_k (x - xbar_k), by the backward recursion
    P_k = Hx + K_k' Hu K_k + M_k' P_{k+1} M_k, M_k = A_k + B_k K_k -- the transpose of propagate_covariance's.  Returns a dict:
    P0 (B, n, n), p0 (B, n), v0 (B,) and fb (B,) int32; out may name any subset of those plus the tracks P (B, N, n, n), p (B, N, n)
    and v (B, N): a sequence of names (new numpy arrays) or a dict name -> array to write into.  penalty=False, the plain cost:
    the model is exact, J of simulate_policy (clamp off, no disturbance) from xbar_0 + d is v0 + p0'd + d'P0 d / 2, and
    tr(P0 Sigma0) / 2 + sum_{k>=1} tr(P_k W) / 2 is propagate_covariance's dJ; fb = 0: no valid gains, the loop is open.
    penalty=True, the augmented Lagrangian inside the active set of the stored pass (box-only problems, AltroError UNSUPPORTED
    otherwise): P_k is the value Hessian of the LQ problem the stored gains solve, P0 the Hessian of the optimal L_A with respect
    to x0; fb = 0 (gain_active_set's): every row of the instance is NaN.  Matrices are as computed, not re-symmetrised.  GPU
    tensors (float64, contiguous; fb int32): stream-ordered, nothing synchronises; numpy: the host twin, the same bytes.  Nothing
    is converted, a mix is refused, and nothing the solver holds changes."""
    if _gpu_form("cost_to_go: the arrays of out", tuple(a for a in out.values() if a is not None) if isinstance(out, dict) else ()):
        with _bracket(solver):
            return _cost_to_go_dev(solver, penalty, out)
    out, shp = _cost_to_go_args(solver, out)
    dt = lambda k: np.int32 if k == "fb" else np.float64
    out = {k: (np.empty(shp[k], dtype=dt(k)) if a is None else a) for k, a in out.items()}
    for k, a in out.items():
        _check_np_out("cost_to_go", k, a, shp[k], dt(k))
    st = _lib.CtgOut()
    for k in _lib.CTG_OUT_FIELDS:
        if k in out:
            setattr(st, k, out[k].ctypes.data)
    solver._chk(solver._L.altro_batch_cost_to_go(solver.h, 1 if penalty else 0, C.byref(st), out["fb"].ctypes.data_as(_IP) if "fb" in out else None))
    return out


_solution_fn = None


def _solution_function():
    """the torch.autograd.Function behind solution, made on first use (the package imports without torch)"""
    global _solution_fn
    if _solution_fn is not None:
        return _solution_fn
    import torch
    from torch.autograd.function import once_differentiable

    class Solution(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, x0, Xref, Uref, invalid):
            # all three validated before the first setter: a refused tensor leaves the solver as it was
            check_device_tensor(x0, (solver.B, solver.n), solver.device, "x0")
            check_device_tensor(Xref, (solver.B, solver.N, solver.n), solver.device, "Xref")
            check_device_tensor(Uref, (solver.B, solver.N - 1, solver.m), solver.device, "Uref")
            X = torch.empty((solver.B, solver.N, solver.n), dtype=torch.float64, device=x0.device)
            U = torch.empty((solver.B, solver.N - 1, solver.m), dtype=torch.float64, device=x0.device)
            with _bracket(solver):
                _set_initial_state_dev(solver, x0.detach())
                _update_trajectory_dev(solver, Xref.detach(), Uref.detach())
                solver._chk(solver._L.altro_batch_solve_async(solver.h))
                solver._chk(solver._L.altro_batch_get_states_dev(solver.h, _addr(X)))
                solver._chk(solver._L.altro_batch_get_controls_dev(solver.h, _addr(U)))
            # the validity of the gains the backward will go through, read once (x0-only: one sweep, no factors needed)
            fb = solution_jvp(solver, vx0=torch.zeros_like(x0), out=("dU",))["fb"]
            bad = (fb == 0).nonzero().flatten().tolist()
            if bad and invalid != "zero":
                raise AltroError(_lib.ERR_STATE, f"solution: instances {bad} hold no valid gains of an unregularised backward pass: "
                                 "the solution is not differentiable through them (invalid='zero' zeroes their gradients)")
            ctx.solver = solver
            ctx.bad = (fb == 0) if bad else None
            return X, U

        @staticmethod
        @once_differentiable
        def backward(ctx, gX, gU):
            solver, need = ctx.solver, ctx.needs_input_grad
            names = tuple(k for k, nd in (("gx0", need[1]), ("gXref", need[2]), ("gUref", need[3])) if nd)
            if not names:
                return None, None, None, None, None
            r = solution_vjp(solver, gX.contiguous(), gU.contiguous(), out=names)
            if ctx.bad is not None:
                for k in names:
                    r[k][ctx.bad] = 0.0
            return None, r.get("gx0"), r.get("gXref"), r.get("gUref"), None

    _solution_fn = Solution
    return Solution


def solution(solver, x0, Xref, Uref, invalid="raise"):
    """The solution (X, U) of a solve as tensors torch can differentiate once with respect to the initial state x0 (B, n) and
    the reference Xref (B, N, n), Uref (B, N-1, m): GPU tensors on the solver's device, float64, contiguous, of exactly these
    shapes (a tensor that is not is refused with ValueError before anything is installed).  Forward CHANGES THE SOLVER: it
    installs the three on it, solves, and returns the trajectory the solver holds.  Backward is one solution_vjp call through
    the gains the solve stored: the exact derivative of the minimiser of the augmented Lagrangian at the multipliers, penalty
    and active set of the last backward pass, so the solver must not be changed between forward and backward.
    The forward reads the validity of the stored gains once (it synchronises): with an instance that holds none, or whose last
    pass was regularised, it raises AltroError -- unless invalid="zero", which zeroes the gradient rows of those instances."""
    if invalid not in ("raise", "zero"):
        raise ValueError("solution: invalid must be 'raise' or 'zero'")
    if not (_on_gpu(x0) and _on_gpu(Xref) and _on_gpu(Uref)):
        raise ValueError("solution: x0, Xref and Uref must be GPU tensors")
    return _solution_function().apply(solver, x0, Xref, Uref, invalid)


_mpc_layer_fn = None
_LAYER_DATA = ("A", "B", "f", "Q", "R", "Qf", "zmin", "zmax")


def _mpc_layer_function():
    """the torch.autograd.Function behind mpc_layer, made on first use (the package imports without torch)"""
    global _mpc_layer_fn
    if _mpc_layer_fn is not None:
        return _mpc_layer_fn
    import torch
    from torch.autograd.function import once_differentiable

    class MPCLayer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, invalid, box, x0, Xref, Uref, A, Bm, f, Q, R, Qf, zmin, zmax):
            B, n, m, N = solver.B, solver.n, solver.m, solver.N
            # everything validated before the first setter: a refused tensor leaves the solver as it was
            check_device_tensor(x0, (B, n), solver.device, "x0")
            check_device_tensor(Xref, (B, N, n), solver.device, "Xref")
            check_device_tensor(Uref, (B, N - 1, m), solver.device, "Uref")
            per_knot = A is not None and A.dim() == 4
            if A is not None:
                kn = (N - 1,) if per_knot else ()
                check_device_tensor(A, (B,) + kn + (n, n), solver.device, "A", colmajor=True)
                check_device_tensor(Bm, (B,) + kn + (n, m), solver.device, "B", colmajor=True)
                check_device_tensor(f, (B,) + kn + (n,), solver.device, "f")
            if Q is not None:
                for nm, t, k in (("Q", Q, n), ("R", R, m), ("Qf", Qf, n)):
                    check_device_tensor(t, (B, k), solver.device, nm)
            if zmin is not None:
                check_device_tensor(zmin, (B, n + m), solver.device, "zmin")
                check_device_tensor(zmax, (B, n + m), solver.device, "zmax")
            if Q is not None:   # (the host setter: it synchronises)
                set_tracking_cost(solver, Q.detach().cpu().numpy(), R.detach().cpu().numpy(), Qf.detach().cpu().numpy())
            X = torch.empty((B, N, n), dtype=torch.float64, device=x0.device)
            U = torch.empty((B, N - 1, m), dtype=torch.float64, device=x0.device)
            with _bracket(solver):
                if A is not None:
                    solver._chk(solver._L.altro_batch_set_dynamics_dev(solver.h, _addr(A.detach()), _addr(Bm.detach()), _addr(f.detach()),
                                                                       int(per_knot), 1))
                if zmin is not None:
                    _set_bounds_dev(solver, box, zmin.detach(), zmax.detach())
                _set_initial_state_dev(solver, x0.detach())
                _update_trajectory_dev(solver, Xref.detach(), Uref.detach())
                solver._chk(solver._L.altro_batch_solve_async(solver.h))
                solver._chk(solver._L.altro_batch_get_states_dev(solver.h, _addr(X)))
                solver._chk(solver._L.altro_batch_get_controls_dev(solver.h, _addr(U)))
            # the validity of what the backward will go through, read once
            data = any(t is not None for t in (A, Q, zmin))
            if data:
                fb = solution_vjp_data(solver, gX=torch.zeros_like(X), out=("gQf",))["fb"]
            else:
                fb = solution_jvp(solver, vx0=torch.zeros_like(x0), out=("dU",))["fb"]
            bad = (fb == 0).nonzero().flatten().tolist()
            if bad and invalid != "zero":
                raise AltroError(_lib.ERR_STATE, f"mpc_layer: instances {bad} hold no valid gains of an unregularised backward pass at the "
                                 "penalty they hold: the solution is not differentiable through them (invalid='zero' zeroes their gradients)")
            ctx.solver, ctx.per_knot = solver, per_knot
            ctx.bad = (fb == 0) if bad else None
            return X, U

        @staticmethod
        @once_differentiable
        def backward(ctx, gX, gU):
            solver, need = ctx.solver, ctx.needs_input_grad[3:]
            gX, gU = gX.contiguous(), gU.contiguous()
            grads = {}
            names = tuple(k for k, nd in zip(("gx0", "gXref", "gUref"), need[:3]) if nd)
            if names:
                grads.update(solution_vjp(solver, gX, gU, out=names))
            names = tuple("g" + k for k, nd in zip(_LAYER_DATA, need[3:]) if nd)
            if names:
                grads.update(solution_vjp_data(solver, gX, gU, per_knot=ctx.per_knot, out=names))
            grads.pop("fb", None)
            if ctx.bad is not None:
                for t in grads.values():
                    t[ctx.bad] = 0.0
            return (None, None, None) + tuple(grads.get(k) for k in ("gx0", "gXref", "gUref") + tuple("g" + k for k in _LAYER_DATA))

    _mpc_layer_fn = MPCLayer
    return MPCLayer


def mpc_layer(solver, x0, Xref, Uref, *, A=None, B=None, f=None, Q=None, R=None, Qf=None, zmin=None, zmax=None, invalid="raise"):
    """solution() with the problem data as further differentiable inputs: the solution (X, U) of a solve as tensors torch can
    differentiate once with respect to x0 (B, n), Xref (B, N, n), Uref (B, N-1, m) and whichever of these are given as tensors --
    the dynamics A (B, n, n), B (B, n, m), f (B, n) per instance, or (B, N-1, ..) per knot (all three together; A and B stored
    column-major, the transpose(-1, -2) of contiguous tensors, as set_dynamics takes them); the cost weights Q (B, n), R (B, m),
    Qf (B, n) (all three together); the bounds zmin, zmax (B, n+m) of the problem's BOX constraint (both together; infinite sides
    stay infinite).  None means what the solver holds.  GPU tensors on the solver's device, float64; one that is not as
    described is refused with ValueError before anything is installed.  Forward CHANGES THE SOLVER: it installs what is given
    -- dynamics and bounds through the device setters, per instance; the weights through
    altro_batch_set_tracking_cost_per_instance, a host call that copies them to the host and SYNCHRONISES -- solves, and returns
    the trajectory the solver holds.  Backward is one solution_vjp call and one solution_vjp_data call through the gains the
    solve stored: the exact derivative of the minimiser of the augmented Lagrangian at the multipliers, penalty and active set
    of the last backward pass, so the solver must not be changed between forward and backward.  Derivatives
    with respect to the dynamics and the bounds need a box-only problem.  The forward reads the validity of the stored gains
    once (it synchronises): invalid means what it means in solution()."""
    if invalid not in ("raise", "zero"):
        raise ValueError("mpc_layer: invalid must be 'raise' or 'zero'")
    data = dict(A=A, B=B, f=f, Q=Q, R=R, Qf=Qf, zmin=zmin, zmax=zmax)
    if not all(_on_gpu(t) for t in (x0, Xref, Uref)) or not all(t is None or _on_gpu(t) for t in data.values()):
        raise ValueError("mpc_layer: x0, Xref, Uref and the data given must be GPU tensors")
    for group in (("A", "B", "f"), ("Q", "R", "Qf"), ("zmin", "zmax")):
        if len({data[k] is None for k in group}) != 1:
            raise ValueError(f"mpc_layer: {', '.join(group)} go together: all or none")
    box = None
    if zmin is not None:
        box = next((i for i, (con, _, _) in enumerate(solver.prob.constraints.items) if isinstance(con, BoundConstraint)), None)
        if box is None:
            raise ValueError("mpc_layer: zmin / zmax need a BOX constraint on the problem")
    return _mpc_layer_function().apply(solver, invalid, box, x0, Xref, Uref, A, B, f, Q, R, Qf, zmin, zmax)


def rollout(solver, U, x0=None, out=None):
    """rollout!(prob): the states of the model under the controls U from x0 (None: the solver's initial state), on the device
    (the rollout form of altro_batch_evaluate).  U (B, N-1, m) -> X (B, N, n); U (B, ncand, N-1, m) -> X (B, ncand, N, n).  GPU
    tensors: stream-ordered, out is the tensor to write into; numpy: the host twin."""
    if U is None:
        raise ValueError("rollout: U is required")
    shp = tuple(int(k) for k in U.shape)[:-2] + (solver.N, solver.n)
    # (the C-ABI wants one of J, c_max, defect: c_max goes to a scratch array kept with the solver, so that a rollout per tick
    #  allocates nothing but `out` when the caller does not pass it)
    if _on_gpu(U):
        import torch
        dev = torch.device("cuda", solver.device)
        if out is None:
            out = torch.empty(shp, dtype=torch.float64, device=dev)
        c = getattr(solver, "_rollout_scratch", None)
        if c is None or not _on_gpu(c) or tuple(c.shape) != shp[:-2]:
            c = solver._rollout_scratch = torch.empty(shp[:-2], dtype=torch.float64, device=dev)
        evaluate(solver, U, x0=x0, out=(None, c, None), Xout=out)
        return out
    if out is None:
        out = np.empty(shp)
    evaluate(solver, U, x0=x0, out=(None, np.empty(shp[:-2]), None), Xout=out)
    return out


def _simulate_shapes(solver, x0, w, nsamp):
    """(nsamp, shape x0 / w / the per-sample outputs / Xout / Uout must have); nsamp comes from x0 (B, nsamp, n) or
    w (B, nsamp, N-1, n) when given, and what is given must agree"""
    B, N, n, m = solver.B, solver.N, solver.n, solver.m
    seen = []
    if x0 is not None:
        shp = tuple(int(k) for k in x0.shape)
        if len(shp) != 3 or shp[1] < 1:
            raise ValueError(f"simulate_policy: x0: shape {shp}, expected ({B}, nsamp, {n})")
        seen.append(shp[1])
    if w is not None:
        shp = tuple(int(k) for k in w.shape)
        if len(shp) != 4 or shp[1] < 1:
            raise ValueError(f"simulate_policy: w: shape {shp}, expected ({B}, nsamp, {N - 1}, {n})")
        seen.append(shp[1])
    if nsamp is not None:
        if int(nsamp) != nsamp or int(nsamp) < 1:
            raise ValueError(f"simulate_policy: nsamp = {nsamp}: it must be an integer >= 1")
        seen.append(int(nsamp))
    if any(k != seen[0] for k in seen):
        raise ValueError(f"simulate_policy: x0, w and nsamp disagree on the number of samples: {seen}")
    ns = seen[0] if seen else 1
    return ns, (B, ns, n), (B, ns, N - 1, n), (B, ns), (B, ns, N, n), (B, ns, N - 1, m)


def _simulate_policy_dev(solver, x0=None, w=None, nsamp=None, clamp=True, out=None, fb=None, Xout=None, Uout=None):
    """device form of simulate_policy: every tensor is validated (shape, dtype, strides, device) before the library is called"""
    ns, s0, sw, lead, sx, su = _simulate_shapes(solver, x0, w, nsamp)
    if x0 is not None:
        check_device_tensor(x0, s0, solver.device, "x0")
    if w is not None:
        check_device_tensor(w, sw, solver.device, "w")
    if out is None:
        import torch
        dev = torch.device("cuda", solver.device)
        out = tuple(torch.empty(lead, dtype=torch.float64, device=dev) for _ in range(3))
    out = tuple(out)
    if len(out) != 3:
        raise ValueError("simulate_policy: out is (J, c_max, dx_max); any may be None")
    if all(o is None for o in out + (fb, Xout, Uout)):
        raise ValueError("simulate_policy: J, c_max, dx_max, fb, Xout and Uout are all None")
    for o, nm in zip(out, ("J", "c_max", "dx_max")):
        if o is not None:
            check_device_tensor(o, lead, solver.device, nm)
    if fb is not None:
        check_device_tensor(fb, (solver.B,), solver.device, "fb", dtype="torch.int32")
    if Xout is not None:
        check_device_tensor(Xout, sx, solver.device, "Xout")
    if Uout is not None:
        check_device_tensor(Uout, su, solver.device, "Uout")
    solver._chk(solver._L.altro_batch_simulate_policy_dev(solver.h, ns, _addr(x0), _addr(w), int(bool(clamp)), _addr(out[0]), _addr(out[1]),
                                                          _addr(out[2]), _addr(fb), _addr(Xout), _addr(Uout)))
    return out


def simulate_policy(solver, x0=None, w=None, nsamp=None, clamp=True, out=None, fb=None, Xout=None, Uout=None):
    """The stored policy of the last solve run in closed loop on the model, nsamp samples per instance
    (altro_batch_simulate_policy / _dev): from x_0 = x0[b, s] (None: the solver's initial state), u_k = eval_policy(x_k, knot k,
    clamp), x_{k+1} = the model's step (+ w[b, s, k] when w is given), over the whole horizon in one kernel.  Returns
    (J, c_max, dx_max), each (B, nsamp): the plain tracking cost and the maximum constraint violation as evaluate gives them
    for the simulated pair, and max_k |x_k - xbar_k|_inf, the largest excursion from the trajectory the solver holds.
    x0 (B, nsamp, n), w (B, nsamp, N-1, n); nsamp is inferred from them when given (default 1).  fb (B,) int32 receives 1 where
    the stored gains are valid, 0 where they are not and the loop is open (u_k = ubar_k); Xout (B, nsamp, N, n) and Uout
    (B, nsamp, N-1, m) receive the simulated states and controls.  Nothing the solver owns changes.
    With GPU tensors (float64, contiguous; fb int32) the call is stream-ordered and nothing synchronises; out = (J, c_max,
    dx_max) are tensors to write into (any may be None; default: three new ones).  With numpy -- or with no array at all --
    the host twin runs: the same bytes."""
    args = (x0, w, fb, Xout, Uout) + (tuple(out) if out is not None else ())
    if _gpu_form("simulate_policy: x0, w, out, fb, Xout and Uout", args):
        with _bracket(solver):
            return _simulate_policy_dev(solver, x0, w, nsamp, clamp, out, fb, Xout, Uout)
    x0 = None if x0 is None else _c(x0)
    w = None if w is None else _c(w)
    ns, s0, sw, lead, sx, su = _simulate_shapes(solver, x0, w, nsamp)
    for a, shp, nm in ((x0, s0, "x0"), (w, sw, "w")):
        if a is not None and a.shape != shp:
            raise ValueError(f"simulate_policy: {nm}: shape {a.shape}, expected {shp}")
    if out is None:
        out = tuple(np.empty(lead) for _ in range(3))
    out = tuple(out)
    if len(out) != 3:
        raise ValueError("simulate_policy: out is (J, c_max, dx_max); any may be None")
    if all(o is None for o in out + (fb, Xout, Uout)):
        raise ValueError("simulate_policy: J, c_max, dx_max, fb, Xout and Uout are all None")
    for o, shp, dt, nm in zip(out + (fb, Xout, Uout), (lead,) * 3 + ((solver.B,), sx, su), (np.float64,) * 3 + (np.int32, np.float64, np.float64),
                              ("J", "c_max", "dx_max", "fb", "Xout", "Uout")):
        if o is not None:
            _check_np_out("simulate_policy", nm, o, shp, dt)
    solver._chk(solver._L.altro_batch_simulate_policy(solver.h, ns, _p(x0), _p(w), int(bool(clamp)), _p(out[0]), _p(out[1]), _p(out[2]),
                                                      None if fb is None else fb.ctypes.data_as(_IP), _p(Xout), _p(Uout)))
    return out


COV_OUTPUTS = ("sx", "su", "sc", "dJ", "fb", "zmin_t", "zmax_t", "Sout")


def _covariance_args(solver, Sigma0, W, con_id, kappa, out):
    """(per_instance, library constraint id or -1, kappa, {name: shape} of every output the call may write, the names a default
    `out` gets); refuses here what the library would refuse, so that it is not called with it"""
    B, N, n, m = solver.B, solver.N, solver.n, solver.m
    if Sigma0 is None and W is None:
        raise ValueError("propagate_covariance: Sigma0 and W are both None")
    shp = {tuple(int(k) for k in a.shape) for a in (Sigma0, W) if a is not None}
    if len(shp) != 1 or next(iter(shp)) not in ((n, n), (B, n, n)):
        raise ValueError(f"propagate_covariance: Sigma0 / W: shapes {sorted(shp)}, expected ({n}, {n}) or ({B}, {n}, {n}), the same for both")
    pi = int(len(next(iter(shp))) == 3)
    shapes = {"sx": (B, N, n), "su": (B, N - 1, m), "dJ": (B,), "fb": (B,), "Sout": (B, N, n, n)}
    default = ["sx", "su", "dJ", "fb"]
    cid = -1
    if con_id is not None:
        items = solver.prob.constraints.items
        if int(con_id) != con_id or not 0 <= int(con_id) < len(items) or isinstance(items[int(con_id)][0], BoundConstraint):
            raise ValueError(f"propagate_covariance: con_id = {con_id}: it must index a LINEAR or SOC constraint of the problem "
                             "(the deviations of a BOX are sx and su)")
        c, first, last = items[int(con_id)]
        shapes["sc"] = (B, last - first + 1, int(np.asarray(c.b).shape[-1]))
        default.append("sc")
        cid = solver.con_ids[int(con_id)]
    if kappa is not None:
        if not (float(kappa) >= 0.0) or float(kappa) == float("inf"):
            raise ValueError(f"propagate_covariance: kappa = {kappa}: it must be finite and not negative")
        shapes["zmin_t"] = shapes["zmax_t"] = (B, n + m)
        default += ["zmin_t", "zmax_t"]
    if out is not None:
        if not isinstance(out, dict) or not out or any(o is None for o in out.values()):
            raise ValueError("propagate_covariance: out is a dict {name: array} with at least one of " + ", ".join(COV_OUTPUTS))
        for k in out:
            if k not in shapes:
                why = "unknown" if k not in COV_OUTPUTS else "needs con_id" if k == "sc" else "needs kappa"
                raise ValueError(f"propagate_covariance: out[{k!r}]: {why}")
        if ("zmin_t" in out) != ("zmax_t" in out):
            raise ValueError("propagate_covariance: zmin_t and zmax_t go together")
        if con_id is not None and "sc" not in out:
            raise ValueError("propagate_covariance: con_id is given: out needs 'sc'")
    return pi, cid, 0.0 if kappa is None else float(kappa), shapes, default


def _propagate_covariance_dev(solver, Sigma0=None, W=None, con_id=None, kappa=None, out=None):
    """device form of propagate_covariance: every tensor is validated (shape, dtype, strides, device) before the library is called"""
    pi, cid, kap, shapes, default = _covariance_args(solver, Sigma0, W, con_id, kappa, out)
    mat = (solver.B, solver.n, solver.n) if pi else (solver.n, solver.n)
    for t, nm in ((Sigma0, "Sigma0"), (W, "W")):
        if t is not None:
            check_device_tensor(t, mat, solver.device, nm)
    if out is None:
        import torch
        dev = torch.device("cuda", solver.device)
        out = {k: torch.empty(shapes[k], dtype=torch.int32 if k == "fb" else torch.float64, device=dev) for k in default}
    for k, t in out.items():
        check_device_tensor(t, shapes[k], solver.device, k, dtype="torch.int32" if k == "fb" else "torch.float64")
    solver._chk(solver._L.altro_batch_propagate_covariance_dev(solver.h, _addr(Sigma0), _addr(W), pi, cid, kap, *(_addr(out.get(k)) for k in COV_OUTPUTS)))
    return out


def propagate_covariance(solver, Sigma0=None, W=None, con_id=None, kappa=None, out=None):
    """The covariance of the closed loop under the stored policy, propagated over the horizon on the device
    (altro_batch_propagate_covariance / _dev):  S_0 = Sigma0, S_{k+1} = (A_k + B_k K_k) S_k (A_k + B_k K_k)' + W -- the analytic
    twin of simulate_policy for the unsaturated loop (no clamp is modelled).  Sigma0 and W are (n, n) for the batch or (B, n, n)
    per instance, the same shape for both; either may be None (zero), not both; symmetry is the caller's business.
    Returns a dict: sx (B, N, n) and su (B, N-1, m) the standard deviations of states and controls, dJ (B,) the expected cost
    over the nominal, fb (B,) int32 1 where the stored gains are valid (0: the loop is open, K = 0); with con_id (the index of a
    LINEAR or SOC constraint of the problem) sc (B, nk, p), the deviations of its row values; with kappa (>= 0) zmin_t and
    zmax_t (B, n+m), the BOX pulled in by kappa deviations, which set_bounds accepts as they are.  out: a dict of arrays to
    write into instead, any subset of those names plus Sout (B, N, n, n), the matrices themselves.  Nothing the solver owns
    changes.  With GPU tensors (float64, contiguous; fb int32) the call is stream-ordered and nothing synchronises; with numpy
    the host twin runs: the same bytes.  Nothing is converted: a mix of the two is refused."""
    args = (Sigma0, W) + (tuple(out.values()) if isinstance(out, dict) else ())
    if _gpu_form("propagate_covariance: Sigma0, W and the arrays of out", args):
        with _bracket(solver):
            return _propagate_covariance_dev(solver, Sigma0, W, con_id, kappa, out)
    for a, nm in ((Sigma0, "Sigma0"), (W, "W")):
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
            raise ValueError(f"propagate_covariance: {nm} must be a C-contiguous float64 array (or a GPU tensor)")
    pi, cid, kap, shapes, default = _covariance_args(solver, Sigma0, W, con_id, kappa, out)
    if out is None:
        out = {k: np.empty(shapes[k], dtype=np.int32 if k == "fb" else np.float64) for k in default}
    for k, o in out.items():
        _check_np_out("propagate_covariance", k, o, shapes[k], np.int32 if k == "fb" else np.float64)
    ptr = lambda k: None if k not in out else out[k].ctypes.data_as(_IP) if k == "fb" else _p(out[k])
    solver._chk(solver._L.altro_batch_propagate_covariance(solver.h, _p(Sigma0), _p(W), pi, cid, kap, *(ptr(k) for k in COV_OUTPUTS)))
    return out


def _warm_start_args(solver, U, rho, include_current):
    """(ncand, shape U must have as (B, ncand, N-1, m) or (B, N-1, m), shape of J / c_max); refuses a bad rho here: the library
    is not called with one"""
    B, N, m = solver.B, solver.N, solver.m
    if U is None:
        raise ValueError("warm_start: U is required")
    rho = float(rho)
    if not (rho >= 0.0) or rho == float("inf"):
        raise ValueError(f"warm_start: rho = {rho}: it must be finite and not negative")
    shp = tuple(int(k) for k in U.shape)
    if len(shp) == 3:
        ncand = 1
    elif len(shp) == 4 and shp[1] >= 1:
        ncand = shp[1]
    else:
        raise ValueError(f"warm_start: U: shape {shp}, expected ({B}, {N - 1}, {m}) or ({B}, ncand, {N - 1}, {m})")
    want = (B, N - 1, m) if len(shp) == 3 else (B, ncand, N - 1, m)
    return ncand, want, (B, ncand + (1 if include_current else 0)), rho


def _warm_start_dev(solver, U, rho=0.0, include_current=True, out=None):
    """device form of warm_start: every tensor is validated (shape, dtype, strides, device) before the library is called"""
    ncand, su, lead, rho = _warm_start_args(solver, U, rho, include_current)
    check_device_tensor(U, su, solver.device, "U")
    if out is None:
        import torch
        dev = torch.device("cuda", solver.device)
        out = (torch.empty((solver.B,), dtype=torch.int32, device=dev),) + tuple(torch.empty(lead, dtype=torch.float64, device=dev) for _ in range(2))
    out = tuple(out)
    if len(out) != 3:
        raise ValueError("warm_start: out is (chosen, J, c_max); any may be None")
    if out[0] is not None:
        check_device_tensor(out[0], (solver.B,), solver.device, "chosen", dtype="torch.int32")
    for o, nm in zip(out[1:], ("J", "c_max")):
        if o is not None:
            check_device_tensor(o, lead, solver.device, nm)
    solver._chk(solver._L.altro_batch_warm_start_dev(solver.h, ncand, _addr(U), rho, 1 if include_current else 0, _addr(out[0]), _addr(out[1]),
                                                     _addr(out[2])))
    return out


def warm_start(solver, U, rho=0.0, include_current=True, out=None):
    """Warm start from the best of several candidates (altro_batch_warm_start / _dev): every candidate control sequence is rolled
    out from the solver's initial state and scored as evaluate's rollout form scores it, merit = fma(rho, c_max, J); per
    instance the lowest merit wins -- the trajectory the solver holds competes as the incumbent when include_current (last
    column, wins ties; among candidates the lowest index wins ties; NaN / Inf never win) -- and the winner's controls and
    rolled-out states become the initial trajectory of the next solve, as initial_controls / set_initial_trajectory would
    leave them.  Duals, penalties, statistics and stored gains stay.  While a mask is set (set_active) inactive instances
    are scored but left as they are.
    U (B, ncand, N-1, m), or (B, N-1, m) for one candidate.  Returns (chosen, J, c_max): chosen (B,) int32 -- 0 .. ncand-1 that
    candidate, ncand the incumbent, -1 nothing had a finite merit (instance untouched), -2 inactive; J, c_max
    (B, ncand + include_current).  With GPU tensors (float64, contiguous; chosen int32) the call is stream-ordered and nothing
    synchronises; out = (chosen, J, c_max) are tensors to write into (any may be None; default: three new ones).  With numpy
    the host twin runs: the same bytes."""
    args = (U,) + (tuple(out) if out is not None else ())
    if _gpu_form("warm_start: U and out", args):
        with _bracket(solver):
            return _warm_start_dev(solver, U, rho, include_current, out)
    U = None if U is None else _c(U)
    ncand, su, lead, rho = _warm_start_args(solver, U, rho, include_current)
    if U.shape != su:
        raise ValueError(f"warm_start: U: shape {U.shape}, expected {su}")
    if out is None:
        out = (np.empty(solver.B, dtype=np.int32), np.empty(lead), np.empty(lead))
    out = tuple(out)
    if len(out) != 3:
        raise ValueError("warm_start: out is (chosen, J, c_max); any may be None")
    for o, shp, dt, nm in zip(out, ((solver.B,), lead, lead), (np.int32, np.float64, np.float64), ("chosen", "J", "c_max")):
        if o is not None:
            _check_np_out("warm_start", nm, o, shp, dt)
    ch = None if out[0] is None else out[0].ctypes.data_as(_IP)
    solver._chk(solver._L.altro_batch_warm_start(solver.h, ncand, _p(U), rho, 1 if include_current else 0, ch, _p(out[1]), _p(out[2])))
    return out
