"""Host-side mirror of the reference's operator interface for the linear MPC path.

The reference is Julia; `julia` is not in this image, so the host side above the C ABI is Python that
keeps the reference's names, argument meaning and error behaviour (the Julia shim a maintainer would use
is julia/AlmpcHIP.jl).  Reference (paths relative to /root/reference):

  proceed_controller                     src/main/main_mpc.jl:22-53
  _design_reference_mpc                  src/main/main_mpc.jl:105-117
  _model_predictive_control_design       src/sub/design_mpc.jl:54-129   (ConstrainedLinearControlDiscreteSystem)
                                         src/sub/design_mpc.jl:22-41    (ConstrainedLinearControlContinuousSystem: discretise, recurse)
  _create_weights_coefficients           src/sub/design_mpc.jl:264-283
  _IMPLEMENTATION_SOLVER_LIST            src/sub/solver_selection.jl:9-14  (+ new tag "hip")
  update_initialization!                 src/main/computation_mpc.jl:17-29  -> update_initialization
  calculate!                             src/main/computation_mpc.jl:38-55  -> calculate
  structs                                src/types/types.jl:24-27,46-50,89-92,114-122,134-139,151-156

`_model_predictive_control_computation` is named by BASELINE.json but does not exist in the reference
(SURVEY.md section 0); here it is update_initialization + calculate for a batch.

Every solve goes through libalmpc.so (HIP); there is no CPU path in this module.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Any, Optional

import numpy as np

from . import _capi
from .sharding import shard_range  # noqa: F401  (re-exported)

__all__ = [
    "Hyperrectangle", "ConstrainedLinearControlDiscreteSystem", "ConstrainedBlackBoxControlDiscreteSystem",
    "ConstrainedLinearControlContinuousSystem", "ConstrainedBlackBoxControlContinuousSystem", "proceed_system_discretization", "Fnn", "ResNet", "PolyNet", "Icnn", "DenseNet",
    "proceed_system_linearization", "ReferencesStateInput", "WeightsCoefficient",
    "TerminalIngredient", "ModelPredictiveControlTuning", "ModelPredictiveControlResults",
    "ModelPredictiveControlController", "proceed_controller", "_design_reference_mpc",
    "_model_predictive_control_design", "_create_weights_coefficients", "update_initialization", "calculate",
    "_model_predictive_control_computation", "sensitivity", "sensitivity_params", "certificate", "HipModeler", "shard_range",
]


# ---- stand-ins for LazySets.Hyperrectangle / MathematicalSystems.ConstrainedLinearControlDiscreteSystem ----
@dataclasses.dataclass
class Hyperrectangle:
    low: np.ndarray
    high: np.ndarray

    def __post_init__(self):
        self.low = np.asarray(self.low, dtype=np.float64)
        self.high = np.asarray(self.high, dtype=np.float64)
        if self.low.shape != self.high.shape or np.any(self.low > self.high):
            raise ValueError("Hyperrectangle: need low <= high of equal length")


@dataclasses.dataclass
class ConstrainedLinearControlDiscreteSystem:
    A: np.ndarray
    B: np.ndarray
    X: Hyperrectangle
    U: Hyperrectangle

    def __post_init__(self):
        self.A = np.asarray(self.A, dtype=np.float64)
        self.B = np.asarray(self.B, dtype=np.float64)
        n, m = self.B.shape
        if self.A.shape != (n, n) or self.X.low.shape != (n,) or self.U.low.shape != (m,):
            raise ValueError(f"{type(self).__name__}: inconsistent dimensions")


@dataclasses.dataclass
class ConstrainedLinearControlContinuousSystem:
    """Stand-in for MathematicalSystems.ConstrainedLinearControlContinuousSystem(A, B, X, U): x' = A x + B u.  The same fields and the
    same validation as the discrete twin; the design discretises it first (src/sub/design_mpc.jl:22-41)."""
    A: np.ndarray
    B: np.ndarray
    X: Hyperrectangle
    U: Hyperrectangle

    __post_init__ = ConstrainedLinearControlDiscreteSystem.__post_init__


@dataclasses.dataclass
class Fnn:
    """Feed-forward network in the layout the reference reads from Flux.params
    (src/sub/model_modeler_implementation/fnn/mpc_modeler_implementation_fnn.jl:88-107): W_in H x (n+m) (no bias, no
    activation), hidden layers (W_h[l], b_h[l]) with activation `act` ("identity" | "relu" | "tanh" | "sigmoid" | "swish"), W_out n x H (no bias).
    Also the model tag AutomationLabsSystems.Fnn() of src/sub/design_mpc.jl:176."""
    W_in: np.ndarray
    W_h: list
    b_h: list
    W_out: np.ndarray
    act: str = "relu"


@dataclasses.dataclass
class ResNet(Fnn):
    """Residual network in the Fnn layout (.../resnet/mpc_modeler_implementation_resnet.jl:123-142): hidden layer
    y' = y + act(W_h[l] y + b_h[l]).  Also the model tag AutomationLabsSystems.ResNet()."""


@dataclasses.dataclass
class PolyNet(Fnn):
    """PolyNet in the Fnn layout (.../polynet/mpc_modeler_implementation_polynet.jl:123-151): hidden layer p = act(W_h[l] y + b_h[l]),
    y' = y + p + act(W_h[l] p + b_h[l]) -- the same weights twice.  Also the model tag AutomationLabsSystems.PolyNet()."""


@dataclasses.dataclass
class Icnn(Fnn):
    """Input-convex network: the reference models it with the Fnn equations (its modeler is the Fnn file with the tag changed,
    get_activation_function treats it as an Fnn: src/sub/design_mpc.jl:472-483).  Runs on the Fnn kernels."""


@dataclasses.dataclass
class DenseNet:
    """DenseNet (.../densenet/mpc_modeler_implementation_densenet.jl:85-161): y_1 = W_in [x; u] (no bias, no activation),
    y_{l+2} = [act(W_h[l] y_{l+1} + b_h[l]); y_{l+1}] -- the new features first, so W_h[l] is H x (l+1) H and its column c multiplies
    entry c of y_{l+1} (newest first) --, x+ = W_out y_{L+1} with W_out n x (L+1) H (no bias).  The Fnn field names in the DenseNet
    shapes (include/almpc.h); its own calls (_capi.densenet_linearize, *_densenet_setup), not the Fnn layout.
    Also the model tag AutomationLabsSystems.DenseNet()."""
    W_in: np.ndarray
    W_h: list
    b_h: list
    W_out: np.ndarray
    act: str = "relu"


# model family -> network kind of the library (_capi.NET_KINDS, and "densenet": its own calls), by EXACT type: a subclass of Fnn is not
# silently an Fnn
_NET_OF_MODEL = {Fnn: "fnn", Icnn: "fnn", ResNet: "resnet", PolyNet: "polynet", DenseNet: "densenet"}
_MODEL_REFUSALS = {
    "DenseNet": "its layer widths grow (y_j has j H rows), which an [L] H x H Fnn layout cannot hold: use controller.DenseNet",
    "Rbf": "its NLP modeler reuses the Fnn layer equations without the deviation and reference constraints: there is no "
           "well-defined network to restate",
    "NeuralODE": "its integrator lives in AutomationLabsSystems, outside the reference",
    "Rknn1": "its integrator lives in AutomationLabsSystems, outside the reference",
    "Rknn2": "its integrator lives in AutomationLabsSystems, outside the reference",
    "Rknn4": "its integrator lives in AutomationLabsSystems, outside the reference",
}


def _net_kind(f) -> str:
    """Network kind of a black-box model: "fnn" (Fnn, Icnn), "resnet", "polynet" or "densenet"; NotImplementedError for any other
    family."""
    kind = _NET_OF_MODEL.get(type(f))
    if kind is None:
        name = type(f).__name__
        why = _MODEL_REFUSALS.get(name, "only the Fnn, Icnn, ResNet, PolyNet and DenseNet families are built")
        raise NotImplementedError(f"black-box model family {name!r} is not supported: {why}")
    return kind


@dataclasses.dataclass
class ConstrainedBlackBoxControlDiscreteSystem:
    """Stand-in for MathematicalSystems.ConstrainedBlackBoxControlDiscreteSystem(f, statedim, inputdim, X, U)."""
    f: Fnn
    statedim: int
    inputdim: int
    X: Hyperrectangle
    U: Hyperrectangle


@dataclasses.dataclass
class ConstrainedBlackBoxControlContinuousSystem:
    """Stand-in for MathematicalSystems.ConstrainedBlackBoxControlContinuousSystem(f, statedim, inputdim, X, U): x' = f(x, u) (the
    Continuous half of the union the reference's black-box design method takes, src/sub/design_mpc.jl:143-147).  Same fields as the
    discrete twin."""
    f: Fnn
    statedim: int
    inputdim: int
    X: Hyperrectangle
    U: Hyperrectangle


def proceed_system_discretization(system, sample_time) -> ConstrainedLinearControlDiscreteSystem:
    """AutomationLabsSystems.proceed_system_discretization (call site: src/sub/design_mpc.jl:35).  The function itself lives outside
    the reference tree, so its method and its sample time are not there to read: this build's reading is the exact zero-order hold
    [A_d B_d; 0 I] = exp([A B; 0 0] Ts) at Ts = the controller's sample time (almpc_c2d)."""
    Ts = float(sample_time)
    if not (Ts > 0.0 and np.isfinite(Ts)):
        raise ValueError("a continuous-time system needs a positive sample time (mpc_sample_time)")
    Ad, Bd = _capi.c2d(system.A, system.B, Ts)
    return ConstrainedLinearControlDiscreteSystem(np.array(Ad), np.array(Bd), system.X, system.U)


def proceed_system_linearization(system, state, input, device: int = 0):
    """AutomationLabsSystems.proceed_system_linearization(system, x, u) (call sites: .../fnn/...:42-46,
    src/sub/design_mpc.jl:319-326): the linear system (A, B) = Jacobians of f at (x, u), same constraint sets -- discrete for a
    discrete black-box system, continuous for a continuous one.  Computed on the GPU (k_fnn_jacobian)."""
    f = system.f
    x, u = np.asarray(state, dtype=np.float64).reshape(1, -1), np.asarray(input, dtype=np.float64).reshape(1, -1)
    net = _net_kind(f)
    if net == "densenet":
        A, B = _capi.densenet_linearize(f.W_in, f.W_h, f.b_h, f.W_out, x, u, act=f.act, device=device)
    else:
        A, B = _capi.fnn_linearize(f.W_in, f.W_h, f.b_h, f.W_out, x, u, act=f.act, device=device, net=net)
    lin = ConstrainedLinearControlContinuousSystem if isinstance(system, ConstrainedBlackBoxControlContinuousSystem) else ConstrainedLinearControlDiscreteSystem
    return lin(A[0], B[0], system.X, system.U)


# ---- structs of src/types/types.jl ------------------------------------------------------------------------
@dataclasses.dataclass
class ReferencesStateInput:
    x: np.ndarray  # n x (N+1)
    u: np.ndarray  # m x N


@dataclasses.dataclass
class WeightsCoefficient:
    Q: np.ndarray
    R: np.ndarray
    S: np.ndarray


@dataclasses.dataclass
class TerminalIngredient:
    Xf: Any
    P: np.ndarray


@dataclasses.dataclass
class ModelPredictiveControlTuning:
    modeler: Any  # the reference stores a JuMP model here (`modeler::Any`, types.jl:115); here a HipModeler
    reference: ReferencesStateInput
    horizon: int
    weights: WeightsCoefficient
    terminal_ingredient: TerminalIngredient
    sample_time: float
    max_time: int


@dataclasses.dataclass
class ModelPredictiveControlResults:
    x: np.ndarray
    e_x: np.ndarray
    u: np.ndarray
    e_u: np.ndarray


@dataclasses.dataclass
class ModelPredictiveControlController:
    system: Any
    tuning: ModelPredictiveControlTuning
    initialization: np.ndarray
    computation_results: ModelPredictiveControlResults


_DEFAULT_PARAMETERS_MODEL_PREDICTIVE_CONTROL = dict(  # src/main/main_mpc.jl:87-94
    mpc_solver="auto", mpc_terminal_ingredient="none", mpc_Q=100.0, mpc_R=0.1, mpc_S=0.0, mpc_max_time=30.0)

# src/sub/solver_selection.jl:9-14 plus the new "hip" tag; "auto" for the linear method resolves to "hip" here
# (the reference resolves it to SCIP, solver_selection.jl:56-65); the CPU solvers are not part of this build.
_IMPLEMENTATION_SOLVER_LIST = ("osqp", "scip", "ipopt", "auto", "hip")
IMPLEMENTATION_PROGRAMMING_LIST = ("linear", "non_linear", "mixed_linear", "fuzzy_linear")  # src/types/types.jl:229-234


def _kws(kws_):
    # the reference's idiom: dict_kws = Dict(kws_); kws = get(dict_kws, :kws, kws_)  (src/main/main_mpc.jl:33-34)
    return dict(kws_.get("kws", kws_))


class HipModeler:
    """What sits in `tuning.modeler` instead of a JuMP model: the almpc handle plus solver options."""

    def __init__(self, solver: _capi.Solver, opts: _capi.almpc_opts, batch: int):
        self.solver, self.opts, self.batch = solver, opts, batch
        self.relinearize = None  # dict for mpc_linearization='step' (black-box models), see _design_blackbox
        self.sqp = None          # dict for mpc_programming_type='non_linear', see _design_blackbox_nonlinear
        self.allow_unsolved = False  # kw mpc_allow_unsolved: calculate! returns the iterate of an instance without a certificate instead of raising
        self.state_rows = False      # a linear design with a state box or the terminal equality: sensitivity(C) takes the rows form


def _design_reference_mpc(state_reference, input_reference, horizon: int) -> ReferencesStateInput:
    xr = np.asarray(state_reference, dtype=np.float64).reshape(-1, 1)
    ur = np.asarray(input_reference, dtype=np.float64).reshape(-1, 1)
    return ReferencesStateInput(xr * np.ones((xr.shape[0], horizon + 1)), ur * np.ones((ur.shape[0], horizon)))


def _create_weights_coefficients(system: ConstrainedLinearControlDiscreteSystem, **kws_) -> WeightsCoefficient:
    kws = _kws(kws_)
    D = _DEFAULT_PARAMETERS_MODEL_PREDICTIVE_CONTROL
    n, m = system.B.shape
    return WeightsCoefficient(float(kws.get("mpc_Q", D["mpc_Q"])) * np.eye(n),
                              float(kws.get("mpc_R", D["mpc_R"])) * np.eye(m),
                              float(kws.get("mpc_S", D["mpc_S"])) * np.eye(m))


def proceed_controller(system, mpc_controller_type: str, mpc_horizon: int, mpc_sample_time: int,
                       mpc_state_reference, mpc_input_reference, **kws_):
    """Same positional contract as the reference (src/main/main_mpc.jl:22-30).  Returns None for a
    controller type other than "model_predictive_control", as the reference falls through."""
    kws = _kws(kws_)
    if not isinstance(mpc_horizon, (int, np.integer)) or not isinstance(mpc_sample_time, (int, np.integer)):
        raise TypeError("mpc_horizon and mpc_sample_time must be Int (src/main/main_mpc.jl:25-26)")
    if mpc_controller_type == "model_predictive_control":
        refs = _design_reference_mpc(mpc_state_reference, mpc_input_reference, mpc_horizon)
        return _model_predictive_control_design(system, mpc_horizon, mpc_sample_time, refs, kws=kws)
    return None


def _model_predictive_control_design(system, horizon: int, sample_time: int, references: ReferencesStateInput, **kws_):
    if isinstance(system, (ConstrainedBlackBoxControlDiscreteSystem, ConstrainedBlackBoxControlContinuousSystem)):
        return _design_blackbox(system, horizon, sample_time, references, **kws_)
    if _kws(kws_).get("mpc_terminal_weight", "reference") != "reference":   # (a linear system is never re-linearised)
        raise ValueError("mpc_terminal_weight = 'step' needs a black-box model with mpc_linearization = 'step'")
    if isinstance(system, ConstrainedLinearControlContinuousSystem):
        # src/sub/design_mpc.jl:22-41: discretise, then the discrete method (whose controller, on the discrete system, is returned).
        # Zero-order hold at Ts = mpc_sample_time is this build's reading of proceed_system_discretization (see there).
        system_d = proceed_system_discretization(system, sample_time)
        return _model_predictive_control_design(system_d, horizon, sample_time, references, **kws_)
    return _design_linear(system, horizon, sample_time, references, **kws_)


def _design_blackbox(system: ConstrainedBlackBoxControlDiscreteSystem, horizon: int, sample_time: int,
                     references: ReferencesStateInput, **kws_):
    """Black-box (Fnn, Icnn, ResNet, PolyNet, DenseNet) model, LinearProgramming branch (src/sub/design_mpc.jl:143-225 ->
    .../fnn/mpc_modeler_implementation_fnn.jl:23-58): dynamics linearised at the FIRST reference, terminal weight
    P = DARE at the linearisation about the LAST reference (src/sub/design_mpc.jl:312-327), then the linear path.

    Extension of this build (BASELINE.json configs[3]), kw mpc_linearization = "step": the dynamics are re-linearised at every
    instance's own current state (and the first input reference) in update_initialization!, each instance gets the
    reference's QP for its own (A_i, B_i) (almpc_design_batched); P stays the design-time terminal weight.  The default
    "reference" is the reference's behaviour: one linearisation at design time, shared by the batch.

    With it, kw mpc_terminal_weight = "step": the terminal weight follows the model too -- every step solves DARE(A_i, B_i, Q, R) of
    the step's own linearisation on the device (almpc_set_terminal_weight); the design-time P serves an instance whose linearisation
    has no stabilising solution (modeler.solver.relin_terminal_status() says which).  The default "reference" keeps the design-time P.

    A ConstrainedBlackBoxControlContinuousSystem (x' = f(x, u)) is an extension of this build: the reference's method takes the
    Discrete | Continuous union but has no network modeler for the continuous half.  Here the order is the reference's
    linearise-then-discretise (.../physical/mpc_modeler_implementation_physical.jl:75-116): the linearisation at the first reference is
    discretised by zero-order hold at Ts = mpc_sample_time and takes the linear path; P is the DARE of the discretised linearisation at
    the last reference.  mpc_linearization = "step" runs the device pipeline with almpc_set_model_time: every step's Jacobians are
    discretised on the device (k_c2d) in front of the design.  mpc_programming_type = "non_linear" raises NotImplementedError (a
    continuous network inside the NLP needs an integrator)."""
    kws = _kws(kws_)
    cont = isinstance(system, ConstrainedBlackBoxControlContinuousSystem)
    if cont and kws.get("mpc_programming_type", "linear") == "non_linear":
        raise NotImplementedError("mpc_programming_type = 'non_linear' with a continuous-time black-box system: the network inside the "
                                  "NLP would need an integrator; use a discrete model or mpc_programming_type = 'linear'")
    lin_mode = kws.get("mpc_linearization", "reference")
    if lin_mode not in ("reference", "step"):
        raise ValueError("mpc_linearization must be 'reference' or 'step'")
    tw_mode = kws.get("mpc_terminal_weight", "reference")
    if tw_mode not in ("reference", "step"):
        raise ValueError("mpc_terminal_weight must be 'reference' or 'step'")
    if tw_mode == "step" and lin_mode != "step":
        raise ValueError("mpc_terminal_weight = 'step' needs mpc_linearization = 'step'")
    net = _net_kind(system.f)   # Fnn, Icnn, ResNet, PolyNet, DenseNet; the other families raise NotImplementedError with the reason
    dev = int(kws.get("mpc_device", 0))
    x_ref, u_ref = np.asarray(references.x, dtype=np.float64), np.asarray(references.u, dtype=np.float64)
    lin_first = proceed_system_linearization(system, x_ref[:, 0], u_ref[:, 0], device=dev)
    lin_last = proceed_system_linearization(system, x_ref[:, -1], u_ref[:, -1], device=dev)
    if cont:   # (the Jacobians of x' = f(x, u) are continuous-time)
        lin_first = proceed_system_discretization(lin_first, sample_time)
        lin_last = proceed_system_discretization(lin_last, sample_time)
    weights = _create_weights_coefficients(lin_first, kws=kws)
    P = _capi.dare(lin_last.A, lin_last.B, weights.Q, weights.R)
    if kws.get("mpc_programming_type", "linear") == "non_linear":
        return _design_blackbox_nonlinear(system, horizon, sample_time, references, weights, P, kws)
    C = _design_linear(lin_first, horizon, sample_time, references, kws=kws, _terminal_P=P)
    C.system = system
    if lin_mode == "step":
        state_box = "mpc_state_constraint" in kws   # the rows of .../fnn/mpc_modeler_implementation_fnn.jl:52-58, per instance
        term_eq = kws.get("mpc_terminal_ingredient", "none") == "equality"
        mod = C.tuning.modeler
        sopt = dict(kws.get("mpc_solver_options", {}))
        f = system.f
        # instances whose linearisation is open-loop unstable (condensed Hessian singular to working precision) are redone in the
        # multiple-shooting form by the stage-wise solvers: the library's default; mpc_structured_fallback = False switches it off
        if not kws.get("mpc_structured_fallback", True):
            mod.solver._check(mod.solver.L.almpc_set_structured_fallback(mod.solver.h, 0))
        mod.solver.set_terminal_weight("dare_device" if tw_mode == "step" else "given")
        mod.solver.set_model_time("continuous" if cont else "discrete", float(sample_time) if cont else 0.0)
        # device-resident pipeline (almpc_relin_fnn_*): Jacobians -> per-instance designs -> step, no host pointers per step
        setup = mod.solver.relin_densenet_setup if net == "densenet" else functools.partial(mod.solver.relin_fnn_setup, net=net)
        setup(f.W_in, f.W_h, f.b_h, f.W_out, references.x, references.u, weights.Q, weights.R, weights.S, np.array(P),
              system.U.low, system.U.high, act=f.act, rho=float(sopt.get("rho", 0.1)),
              sigma=float(sopt.get("sigma", 1e-6)), rho_profile=kws.get("mpc_rho_profile", "scalar"),
              xmin=system.X.low if state_box else None, xmax=system.X.high if state_box else None,
              terminal="equality" if term_eq else "none")
        mod.relinearize = dict(system=system, device=dev)
    return C


def _design_blackbox_nonlinear(system, horizon, sample_time, references, weights, P, kws):
    """Black-box (Fnn, Icnn, ResNet, PolyNet, DenseNet) model, NonLinearProgramming branch (.../fnn/mpc_modeler_implementation_fnn.jl:73-189): the network itself
    is the equality constraint x[:,k+1] = fnn(x[:,k], u[:,k]) and the reference gives the NLP to Ipopt
    (src/sub/solver_selection.jl:100-104).  Here the same NLP goes through the device-resident SQP loop (almpc_sqp_fnn_*).
    Keys of this build: mpc_sqp_iterations (outer iterations per calculate!, default 10), mpc_sqp_step (step length, default 1),
    mpc_sqp_step_rule ("merit": steps safeguarded by the l1 merit function, default; "fixed"),
    mpc_sqp_warm_start (start each calculate! from the previous inputs shifted by one stage, default True),
    mpc_sqp_hessian ("gauss_newton", default, or "exact": the exact Lagrangian Hessian in every QP of the loop),
    mpc_sqp_tolerance (None, default: a fixed mpc_sqp_iterations per calculate!; a number: solve every instance to that first-order
    residual in at most mpc_sqp_iterations full steps, almpc_sqp_fnn_solve -- an instance left at the iteration limit raises
    ArithmeticError unless mpc_allow_unsolved; modeler.last_sqp_status / last_sqp_iters / last_sqp_kkt record the outcome).
    With mpc_state_constraint or mpc_terminal_ingredient = "equality" (condensed QP route) the multipliers of those rows are switched on
    (almpc_sqp_fnn_set_row_multipliers): they are part of the stopping test and of the exact Hessian's Lagrangian, so both
    mpc_sqp_tolerance and mpc_sqp_hessian = "exact" work with constrained states; modeler.last_sqp_state_multipliers holds them
    ((batch, n, N): the row of x[:, k+1] at [:, :, k]) after a tolerance solve."""
    D = _DEFAULT_PARAMETERS_MODEL_PREDICTIVE_CONTROL
    solver_name = kws.get("mpc_solver", D["mpc_solver"])
    if solver_name not in _IMPLEMENTATION_SOLVER_LIST:
        raise KeyError(solver_name)
    if solver_name in ("osqp", "scip", "ipopt"):
        raise NotImplementedError(f"mpc_solver={solver_name!r} is the reference's CPU path; this build provides 'hip' (and 'auto' -> 'hip')")
    terminal = kws.get("mpc_terminal_ingredient", D["mpc_terminal_ingredient"])
    if terminal == "contractive":
        raise NotImplementedError("terminal ingredient 'contractive' is a quadratic constraint (src/sub/design_mpc.jl:333-340), not a QP row")
    state_box = "mpc_state_constraint" in kws       # .../fnn/mpc_modeler_implementation_fnn.jl:146-153: rows of every SQP iteration's QP
    f = system.f
    n, m = system.statedim, system.inputdim
    batch = int(kws.get("mpc_batch", 1))
    x_ref, u_ref = np.asarray(references.x, dtype=np.float64), np.asarray(references.u, dtype=np.float64)
    if x_ref.shape != (n, horizon + 1) or u_ref.shape != (m, horizon):
        raise ValueError("references must be n x (N+1) and m x N")
    tol = kws.get("mpc_sqp_tolerance", None)
    if tol is not None:
        tol = float(tol)
        if not tol > 0.0:
            raise ValueError("mpc_sqp_tolerance must be > 0 (or None)")
        if float(kws.get("mpc_sqp_step", 1.0)) != 1.0:
            raise ValueError("mpc_sqp_tolerance solves with full steps (under mpc_sqp_step_rule): mpc_sqp_step must be 1")
        if float(np.asarray(weights.R, dtype=np.float64).reshape(m, m)[0, 0]) == 0.0:
            raise ValueError("mpc_sqp_tolerance: the first-order residual scales the gradient by 1 / (2 R_aa): R must not be 0")
    sopt = dict(kws.get("mpc_solver_options", {}))
    solver = _capi.Solver(n, m, horizon, batch, device=int(kws.get("mpc_device", 0)), timing=bool(kws.get("mpc_timing", False)))
    net = _net_kind(f)
    setup = solver.sqp_densenet_setup if net == "densenet" else functools.partial(solver.sqp_fnn_setup, net=net)
    setup(f.W_in, f.W_h, f.b_h, f.W_out, x_ref, u_ref, weights.Q, weights.R, weights.S, P, system.U.low, system.U.high,
          act=f.act, rho=float(sopt.get("rho", 0.1)), sigma=float(sopt.get("sigma", 1e-6)),
          rho_profile=kws.get("mpc_rho_profile", "scalar"),
          xmin=system.X.low if state_box else None, xmax=system.X.high if state_box else None,
          terminal="equality" if terminal == "equality" else "none",
          qp_solver=kws.get("mpc_sqp_qp_solver", "condensed"))   # "structured": every QP through k_riccati
    state_rows = (state_box or terminal == "equality") and kws.get("mpc_sqp_qp_solver", "condensed") == "condensed"
    if state_rows:   # (before set_hessian: the exact mode takes state rows only with their multipliers)
        solver.sqp_fnn_set_row_multipliers(True)
    hess = kws.get("mpc_sqp_hessian", "gauss_newton")
    if hess not in _capi.SQP_HESSIANS:
        solver.close()
        raise ValueError(f"mpc_sqp_hessian must be one of {sorted(_capi.SQP_HESSIANS)}")
    try:
        solver.sqp_fnn_set_hessian(hess)
    except _capi.AlmpcError:
        solver.close()
        raise
    mod = HipModeler(solver, _capi.default_opts(**sopt), batch)
    mod.allow_unsolved = bool(kws.get("mpc_allow_unsolved", False))
    mod.sqp = dict(iterations=int(kws.get("mpc_sqp_iterations", 10)), step=float(kws.get("mpc_sqp_step", 1.0)),
                   warm_start=bool(kws.get("mpc_sqp_warm_start", True)), u_prev=None,
                   step_rule=kws.get("mpc_sqp_step_rule", "merit"), tolerance=tol, state_rows=state_rows)
    mod.last_sqp_status = mod.last_sqp_iters = mod.last_sqp_kkt = mod.last_sqp_state_multipliers = None
    tuning = ModelPredictiveControlTuning(mod, references, horizon, weights, TerminalIngredient(terminal, np.array(P)),
                                          float(sample_time), int(kws.get("mpc_max_time", D["mpc_max_time"])))
    shape = (lambda *s: s) if batch == 1 else (lambda *s: (batch, *s))
    results = ModelPredictiveControlResults(np.empty(shape(n, horizon + 1)), np.empty(shape(n, horizon + 1)),
                                            np.empty(shape(m, horizon)), np.empty(shape(m, horizon)))
    return ModelPredictiveControlController(system, tuning, np.empty(shape(n)), results)


def _design_linear(system: ConstrainedLinearControlDiscreteSystem, horizon: int, sample_time: int,
                   references: ReferencesStateInput, _terminal_P=None, **kws_):
    """Design for the discrete linear system (src/sub/design_mpc.jl:54-129).  Extra keys of this build:
    mpc_batch (instances sharing this design, default 1), mpc_device (HIP device id, default 0),
    mpc_solver_options (dict of almpc_opts fields), mpc_timing (bool)."""
    kws = _kws(kws_)
    D = _DEFAULT_PARAMETERS_MODEL_PREDICTIVE_CONTROL
    ptype = kws.get("mpc_programming_type", "linear")
    if ptype not in IMPLEMENTATION_PROGRAMMING_LIST:
        raise KeyError(ptype)  # the reference indexes a NamedTuple and throws
    if ptype != "linear":
        raise NotImplementedError(f"mpc_programming_type={ptype!r}: only the LinearProgramming path is built (SURVEY.md section 8)")
    solver_name = kws.get("mpc_solver", D["mpc_solver"])
    if solver_name not in _IMPLEMENTATION_SOLVER_LIST:
        raise KeyError(solver_name)
    if solver_name in ("osqp", "scip", "ipopt"):
        raise NotImplementedError(f"mpc_solver={solver_name!r} is the reference's CPU path; this build provides 'hip' (and 'auto' -> 'hip')")
    terminal = kws.get("mpc_terminal_ingredient", D["mpc_terminal_ingredient"])
    if terminal == "contractive":
        raise NotImplementedError("terminal ingredient 'contractive' is a quadratic constraint (src/sub/design_mpc.jl:333-340), "
                                  "not a QP row: the reference itself cannot pass it to OSQP")
    if terminal == "neighborhood":  # the reference only warns and adds nothing (src/sub/design_mpc.jl:342-345)
        import warnings
        warnings.warn("neighborhood terminal state constraint is not yet implemented")
    elif terminal not in ("none", "equality"):
        # the reference's final `else` (src/sub/design_mpc.jl:389-391): an unknown string adds no terminal constraint; it is stored as given
        # in TerminalIngredient.Xf there, and here
        pass
    # the state box exists only if the kw is PRESENT (its value is never read), bounds come from system.X (..linear.jl:62-70)
    state_box = "mpc_state_constraint" in kws
    max_time = kws.get("mpc_max_time", D["mpc_max_time"])
    weights = _create_weights_coefficients(system, kws=kws)
    n, m = system.B.shape
    batch = int(kws.get("mpc_batch", 1))
    x_ref, u_ref = np.asarray(references.x, dtype=np.float64), np.asarray(references.u, dtype=np.float64)
    if x_ref.shape != (n, horizon + 1) or u_ref.shape != (m, horizon):
        raise ValueError("references must be n x (N+1) and m x N")
    sopt = dict(kws.get("mpc_solver_options", {}))
    rho, sigma = float(sopt.get("rho", 0.1)), float(sopt.get("sigma", 1e-6))
    solver = _capi.Solver(n, m, horizon, batch, device=int(kws.get("mpc_device", 0)), timing=bool(kws.get("mpc_timing", False)))
    # bounds as the reference reads them: low = last vertex, high = first vertex of the hyperrectangle
    # (..linear.jl:34-38); P = DARE at the (linear) system (src/sub/design_mpc.jl:327), computed in the library.
    solver.design_shared(system.A, system.B, weights.Q, weights.R, weights.S, _terminal_P, system.U.low, system.U.high,
                         xmin=system.X.low if state_box else None, xmax=system.X.high if state_box else None,
                         rho=rho, sigma=sigma, terminal="equality" if terminal == "equality" else "none",
                         rho_profile=kws.get("mpc_rho_profile", "scalar"))
    solver.set_reference(x_ref, u_ref)
    P = solver.get_design()["P"]
    opts = _capi.default_opts(**sopt)
    modeler_ = HipModeler(solver, opts, batch)
    modeler_.allow_unsolved = bool(kws.get("mpc_allow_unsolved", False))
    modeler_.state_rows = state_box or terminal == "equality"   # (sensitivity(C) then takes the rows form)
    tuning = ModelPredictiveControlTuning(modeler_, references, horizon, weights,
                                          TerminalIngredient(terminal, np.array(P)), float(sample_time), int(max_time))
    shape = (lambda *s: s) if batch == 1 else (lambda *s: (batch, *s))
    results = ModelPredictiveControlResults(np.empty(shape(n, horizon + 1)), np.empty(shape(n, horizon + 1)),
                                            np.empty(shape(m, horizon)), np.empty(shape(m, horizon)))
    return ModelPredictiveControlController(system, tuning, np.empty(shape(n)), results)


def update_initialization(C: ModelPredictiveControlController, initialization) -> None:
    """update_initialization!(C, x0): x0 of length n (batch 1) or shape (batch, n)."""
    mod: HipModeler = C.tuning.modeler
    x0 = np.asarray(initialization, dtype=np.float64)
    n = C.tuning.modeler.solver.n
    if x0.size != mod.batch * n:
        raise ValueError(f"initialization must hold {mod.batch} x {n} values")
    C.initialization = x0.reshape((n,) if mod.batch == 1 else (mod.batch, n)).copy()
    if getattr(mod, "sqp", None) is not None:  # non_linear: the SQP iterate restarts from the network's own rollout
        up = mod.sqp["u_prev"] if mod.sqp["warm_start"] else None
        ug = None if up is None else np.concatenate([up[:, :, 1:], up[:, :, -1:]], axis=2)
        mod.solver.sqp_fnn_start(x0.reshape(mod.batch, n), ug)
        return
    # mpc_linearization='step': the Jacobians at (x0_i, u_ref[:,1]) and the per-instance designs are part of calculate! (on the device)
    mod.solver.update_initialization(x0.reshape(mod.batch, n))


def calculate(C: ModelPredictiveControlController) -> None:
    """calculate!(C): solve and copy u, e_u, x, e_x into C.computation_results.  The reference does not
    check the solver status and lets JuMP.value throw when no solution exists; here a non-finite instance
    raises ArithmeticError, and per-instance status/iterations are kept on the modeler."""
    mod: HipModeler = C.tuning.modeler
    if getattr(mod, "sqp", None) is not None and mod.sqp.get("tolerance") is not None:
        out = mod.solver.sqp_fnn_solve(mod.sqp["iterations"], mod.sqp["tolerance"], mod.opts, step_rule=mod.sqp["step_rule"])
        mod.last_sqp_status, mod.last_sqp_iters, mod.last_sqp_kkt = out["status"], out["iters"], out["kkt"]
        if mod.sqp.get("state_rows"):
            mod.last_sqp_state_multipliers = mod.solver.sqp_fnn_state_multipliers()
        if np.any(out["status"] != 0) and not getattr(mod, "allow_unsolved", False):   # as the status-1 rule below
            raise ArithmeticError(f"calculate!: {int((out['status'] != 0).sum())} instance(s) not solved to mpc_sqp_tolerance in "
                                  "mpc_sqp_iterations iterations (mpc_allow_unsolved = True returns the iterate; modeler.last_sqp_status says which)")
    elif getattr(mod, "sqp", None) is not None:
        mod.last_sqp_history = mod.solver.sqp_fnn_iterate(mod.sqp["iterations"], mod.sqp["step"], mod.opts, step_rule=mod.sqp["step_rule"])
    elif getattr(mod, "relinearize", None) is not None:
        mod.solver.relin_fnn_step(mod.opts)
    else:
        mod.solver.calculate(mod.opts)
    r = mod.solver.get_results()
    mod.last_status, mod.last_iters, mod.last_polish_iters = r["status"], r["iters"], r["polish_iters"]
    if np.any(r["status"] == _capi.NON_FINITE):
        raise ArithmeticError("calculate!: non-finite values in at least one instance (no solution to read)")
    if np.any(r["status"] == _capi.INFEASIBLE):  # the reference: JuMP.value throws when the solver has no primal
        raise ArithmeticError("calculate!: infeasible problem in at least one instance (state box / terminal equality)")
    # status 1 with the exact finish on: no certificate even after the library's stage-wise redo (an iteration cap, a working set
    # beyond 128 rows).  The reference returns a solution or throws: raise, unless kw mpc_allow_unsolved = True asked for the iterate
    # (with polish off status 1 is OSQP's ITERATION_LIMIT, with which JuMP.value still returns)
    if np.any(r["status"] == 1) and int(mod.opts.polish) != 0 and not getattr(mod, "allow_unsolved", False):
        raise ArithmeticError(f"calculate!: {int((r['status'] == 1).sum())} instance(s) without an optimality certificate "
                              "(mpc_allow_unsolved = True returns the iterate; modeler.last_status says which)")
    res = C.computation_results
    for k in ("x", "e_x", "u", "e_u"):
        getattr(res, k)[...] = r[k][0] if mod.batch == 1 else r[k]
    if getattr(mod, "sqp", None) is not None:
        mod.sqp["u_prev"] = r["u"].copy()


def sensitivity(C: ModelPredictiveControlController, want=("K0",), act_tol: float = 0.0, act_tol_x: float = 0.0) -> dict:
    """Derivatives of the last calculate!(C) with respect to the initial state.  An extension of this build: the reference's
    surface stops at the four result matrices (src/main/computation_mpc.jl:50-53).  Returns {"K0": du[:,1]/dx0 (m, n), "dU":
    (m, N, n), "dX": (n, N+1, n), "rows": rows at a bound} for what `want` names, with a leading batch axis when the controller
    has more than one instance; u ~ u* + K0 (x - x0) is the exact local law on the current critical region.  Linear controllers
    with an input box; with mpc_state_constraint or mpc_terminal_ingredient = "equality" the rows form is taken (rows then counts
    state rows too, act_tol_x is their threshold: Solver.sensitivity_rows).  modeler.solver.sensitivity / sensitivity_rows say what
    is refused."""
    mod: HipModeler = C.tuning.modeler
    if mod.state_rows:
        out = mod.solver.sensitivity_rows(want, act_tol, act_tol_x)
    else:
        out = mod.solver.sensitivity(want, act_tol)
    return {k: (v[0] if mod.batch == 1 else v) for k, v in out.items()}


def certificate(C: ModelPredictiveControlController, want=("cost", "res", "grad", "costate")) -> dict:
    """Certificate of the last calculate!(C) (beside `sensitivity`, an extension of this build): {"cost": the objective value JuMP
    would report, "res": the KKT residual of the returned inputs (0 at an optimum, whatever the solver's own status says), "grad":
    the gradient of the objective in the inputs (m, N), "costate": (n, N+1), whose first column is d cost / d x0} for what `want`
    names, with a leading batch axis when the controller has more than one instance.  The multipliers of the input box are
    _capi.multipliers(grad, u, umin, umax).  Linear controllers; with mpc_state_constraint or the terminal equality only "cost"
    is served (Solver.certificate says what is refused)."""
    mod: HipModeler = C.tuning.modeler
    out = mod.solver.certificate(want)
    return {k: (v[0] if mod.batch == 1 else v) for k, v in out.items()}


def sensitivity_params(C: ModelPredictiveControlController, g_u, g_x=None, want=_capi.PARAM_GROUPS, act_tol: float = 0.0,
                       terminal: str = "data") -> dict:
    """Gradients of a loss on the last calculate!(C) in the problem data (beside `sensitivity`, an extension of this build): for loss
    gradients g_u (m, N) and g_x (n, N+1) on the returned trajectories (a leading batch axis when the controller has more than one
    instance) the gradients in x0, the QP's linear term f, u_ref, the input box (u_min, u_max), the weights Q, P, R, S and the model
    A, B -- what `want` names -- per instance, and rows.  Linear controllers with an input box (Solver.sensitivity_params_vjp says
    what is refused).  terminal="data": the terminal weight counts as data also where the design computed it.  terminal="dare": the
    gradient of the reference's own problem, whose P is always are(Discrete, A, B, Q, R) (src/sub/design_mpc.jl:318-327) -- Q, R, A, B
    also gain what the loss gains through P, and the dict carries dare_status (0: followed; else that instance's P is not the
    stabilising DARE solution of its model and it keeps the "data" values)."""
    mod: HipModeler = C.tuning.modeler
    out = mod.solver.sensitivity_params_vjp(g_u, g_x, want, act_tol, terminal)
    return {k: (v[0] if mod.batch == 1 else v) for k, v in out.items()}


def _model_predictive_control_computation(C: ModelPredictiveControlController, X0):
    """Batch step: update_initialization! + calculate!; returns C.computation_results."""
    update_initialization(C, X0)
    calculate(C)
    return C.computation_results
