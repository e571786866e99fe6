"""mujoco_template_amd — MI355X-native batched step/rollout engine behind the
``Env`` / ``Controller`` / ``ObservationSpec`` API of ChenDavidTimothy/mujoco-template.

Only the per-step physics path is rebuilt: ``Env.step`` / ``Env.passive`` /
``ModelHandle`` / ``ObservationExtractor`` / ``linearize_discrete`` /
``compute_requested_jacobians`` / ``iterate_passive`` dispatch through the C ABI of
``include/mjbatch.h`` into hand-written HIP kernels (``csrc/``).  ``mj`` is the slice of the
``mujoco`` surface the path uses, backed by the same engine.
"""

from __future__ import annotations

from . import mj
from ._typing import InfoDict, JacobianDict, JacobiansDict, Observation, ObservationArray, ObservationDict, StateSnapshot
from .compat import CompatibilityReport, check_controller_compat
from .control import ControlSpace, Controller, ControllerCapabilities, uses_device_arrays
from .controllers import LinearFeedbackController, PositionTargetDemo, RandomCtrlController, ZeroController
from .device_data import DeviceData
from .env import Env, StepResult
from .exceptions import CompatibilityError, ConfigError, LinearizationError, NameLookupError, TemplateError
from .feedback import DeviceFeedbackController, FeedbackRollout, feedback_ctrl, rollout_feedback
from .jacobians import compute_requested_jacobians
from .linearization import linearize_discrete
from .model import ModelHandle
from .observations import ObservationExtractor, ObservationProducer, ObservationSpec
from .rollout import linearize_rollout, rollout
from .logging import DataProbe, StateControlRecorder
from .runtime import StepHook, TrajectoryLogger, iterate_passive, run_passive_headless
from .setpoints import SetpointResult, solve_setpoint, steady_ctrl0, steady_ctrl0_device
from .trajopt import DareResult, KalmanResult, solve_kalman, LqrBackwardResult, LqrBoxResult, LyapResult, PolesResult, TrajCostResult, TrajSelectResult, lqr_backward, lqr_candidates, select_candidates, solve_dare, closed_loop_poles, closed_loop_cost, trajectory_cost

__version__ = "0.1.0"

__all__ = [
    "mj", "TemplateError", "NameLookupError", "CompatibilityError", "LinearizationError", "ConfigError",
    "ControlSpace", "Controller", "ControllerCapabilities", "ObservationSpec", "ObservationExtractor",
    "ObservationProducer", "ModelHandle", "CompatibilityReport", "StepResult", "Env", "ZeroController",
    "PositionTargetDemo", "RandomCtrlController", "LinearFeedbackController", "check_controller_compat", "linearize_discrete",
    "compute_requested_jacobians", "StepHook", "iterate_passive", "run_passive_headless", "steady_ctrl0", "DataProbe",
    "StateControlRecorder", "TrajectoryLogger", "rollout", "linearize_rollout", "ObservationDict", "DeviceData", "uses_device_arrays",
    "ObservationArray", "Observation", "JacobianDict", "JacobiansDict", "InfoDict", "StateSnapshot", "lqr_backward", "lqr_candidates", "trajectory_cost", "select_candidates", "TrajCostResult", "TrajSelectResult",
    "LqrBackwardResult", "LqrBoxResult", "solve_dare", "DareResult", "solve_kalman", "KalmanResult", "closed_loop_poles", "PolesResult", "closed_loop_cost", "LyapResult", "solve_setpoint", "steady_ctrl0_device", "SetpointResult",
    "feedback_ctrl", "rollout_feedback", "FeedbackRollout", "DeviceFeedbackController", "__version__",
]
