"""ctypes binding of ``libmjbatch.so`` (C ABI: ``include/mjbatch.h``) and the thin
:class:`BatchSim` object the Python front (``model.py`` / ``env.py``) dispatches through.

There is no CPU fallback: if the HIP library is missing or no device is
visible, construction raises :class:`~mujoco_template_amd.exceptions.TemplateError`.
"""

from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Sequence

import numpy as np

from ._pack import PackedTable
from .exceptions import ConfigError, NameLookupError, TemplateError, raise_for_status
from .mjcf import CompiledModel

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("MJB_LIB") or os.path.join(_HERE, "libmjbatch_prof.so" if os.environ.get("MJB_PROFILE") == "1" else "libmjbatch.so")
_LIB: ctypes.CDLL | None = None

MJB_F32, MJB_F64 = 0, 1
MJB_KERNEL_STEP, MJB_KERNEL_FD, MJB_KERNEL_STEP2 = 1, 2, 3      # kinds of per-model specialised kernel
CTRL_KEEP, CTRL_ZERO, CTRL_RANDOM, CTRL_FEEDBACK = 0, 1, 2, 3
COUNTER_NAMES = ("ncon", "nefc", "solver_niter", "con_dropped", "efc_dropped", "warn_badqpos", "warn_badqvel", "warn_badqacc")


def build_library(force: bool = False) -> str:
    """Compile the HIP sources in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "-j6"], stdout=subprocess.DEVNULL)
    return _LIB_PATH


class Strided(ctypes.Structure):
    """``mjbStrided``: block (t, e) at ptr + t * step_stride + e * env_stride, strides in elements."""
    _fields_ = [("ptr", ctypes.c_void_p), ("step_stride", ctypes.c_long), ("env_stride", ctypes.c_long)]


class LqrBackwardStruct(ctypes.Structure):
    """``mjbLqrBackward`` (include/mjbatch.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("T", "batch", "nx", "nu")] + \
               [(n, Strided) for n in ("A", "B", "lx", "lu", "lxx", "luu", "lux", "VxT", "VxxT", "mu")] + \
               [(n, ctypes.c_void_p) for n in ("k", "K", "dV", "V0x", "V0xx", "status")]


class LqrBackwardBoxStruct(ctypes.Structure):
    """``mjbLqrBackwardBox`` (include/mjbatch.h)."""
    _fields_ = [("base", LqrBackwardStruct), ("u", Strided)] + [(n, ctypes.c_void_p) for n in ("lo", "hi", "clamped", "qp_iters")]


class LqrCandidatesStruct(ctypes.Structure):
    """``mjbLqrCandidates`` (include/mjbatch.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("T", "batch", "nx", "nu", "nalpha", "out_f32")] + \
               [(n, Strided) for n in ("A", "B", "k", "K", "u", "dx0")] + \
               [(n, ctypes.c_void_p) for n in ("alphas", "lo", "hi", "cand")]


class LqrDareStruct(ctypes.Structure):
    """``mjbLqrDare`` (include/mjbatch.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("batch", "nx", "nu", "max_iter")] + [("tol", ctypes.c_double)] + \
               [(n, Strided) for n in ("A", "B", "Q", "R")] + \
               [(n, ctypes.c_void_p) for n in ("X", "K", "change", "iters", "status")]


class LqrEigStruct(ctypes.Structure):
    """``mjbLqrEig`` (include/mjbatch.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("batch", "nx", "nu", "feedback_sign", "balance", "max_sweeps")] + \
               [(n, Strided) for n in ("A", "B", "K")] + \
               [(n, ctypes.c_void_p) for n in ("wr", "wi", "rho", "scale", "sweeps", "status")]


class LqrDlyapStruct(ctypes.Structure):
    """``mjbLqrDlyap`` (include/mjbatch.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("batch", "nx", "nu", "feedback_sign", "transpose", "max_iter")] + [("tol", ctypes.c_double)] + \
               [(n, Strided) for n in ("A", "B", "K", "Q", "R", "x0")] + \
               [(n, ctypes.c_void_p) for n in ("P", "J", "change", "iters", "status")]


class StridedIn(ctypes.Structure):
    """``mjbStridedIn``: an ``mjbStrided`` array of float32 (dtype 0) or float64 (dtype 1) elements."""
    _fields_ = [("ptr", ctypes.c_void_p), ("step_stride", ctypes.c_long), ("env_stride", ctypes.c_long), ("dtype", ctypes.c_int)]


class TrajCostStruct(ctypes.Structure):
    """``mjbTrajCost`` (include/mjbatch.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("T", "batch")] + \
               [(n, StridedIn) for n in ("qpos0", "qvel0", "qpos", "qvel", "ctrl")] + \
               [(n, Strided) for n in ("qref", "vref", "uref", "Q", "R", "Qf")] + \
               [(n, ctypes.c_void_p) for n in ("cost", "cost_t", "lx", "lu", "VxT")]


class SetpointStruct(ctypes.Structure):
    """``mjbSetpoint`` (include/mjbatch.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("batch", "nu", "nv", "max_sweeps")] + [("rcond_min", ctypes.c_double)] + \
               [(n, StridedIn) for n in ("moment", "qfrc")] + \
               [(n, ctypes.c_void_p) for n in ("ctrl", "sv", "rcond", "residual", "pinv", "rank", "sweeps", "status")]


class FeedbackLawStruct(ctypes.Structure):
    """``mjbFeedbackLaw`` (include/mjbatch.h)."""
    _fields_ = [(n, StridedIn) for n in ("K", "u0", "q0", "v0")] + [(n, ctypes.c_int) for n in ("feedback_sign", "clip")] + \
               [(n, ctypes.c_void_p) for n in ("env_mask", "status", "u_rec")] + \
               [(n, ctypes.c_long) for n in ("u_rec_step_stride", "u_rec_env_stride")]


class TrajSelectStruct(ctypes.Structure):
    """``mjbTrajSelect`` (include/mjbatch.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("nprob", "ncand", "T", "nu", "mode", "cand_dtype", "out_dtype")] + \
               [("temperature", ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ("cost", "cand", "u_out", "best", "best_cost", "weights")]


def load_library() -> ctypes.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        raise TemplateError(
            f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the batched engine has no CPU fallback)")
    # torch bundles its own libamdhip64 (same SONAME as /opt/rocm's): import it first so both share one HIP runtime
    import torch  # noqa: F401

    L = ctypes.CDLL(_LIB_PATH)
    vp, ci, cd, cu, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint, ctypes.c_long
    pvp = ctypes.POINTER(ctypes.c_void_p)
    pci = ctypes.POINTER(ctypes.c_int)
    L.mjb_last_error.restype = ctypes.c_char_p
    L.mjb_device_count.restype = ci
    L.mjb_model_create.argtypes = [ci, vp, vp, vp, vp, pvp]
    L.mjb_model_free.argtypes = [vp]
    L.mjb_model_set_disableactuator.argtypes = [vp, ci]
    L.mjb_model_set_solver.argtypes = [vp, ci, cd]
    L.mjb_data_create.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, pvp]
    L.mjb_data_free.argtypes = [vp]
    L.mjb_set_stream.argtypes = [vp, vp]
    L.mjb_sync.argtypes = [vp]
    L.mjb_engine_flags.argtypes = [vp, pci]
    L.mjb_data_info.argtypes = [vp, pci, pci, pci, pci, pci, pci]
    L.mjb_array_ptr.argtypes = [vp, ctypes.c_char_p, pvp, ctypes.POINTER(cl), pci]
    L.mjb_get_array.argtypes = [vp, ctypes.c_char_p, vp]
    L.mjb_set_array.argtypes = [vp, ctypes.c_char_p, vp]
    L.mjb_get_counters.argtypes = [vp, vp]
    L.mjb_reset.argtypes = [vp, ci]
    L.mjb_forward.argtypes = [vp]
    L.mjb_reset_envs.argtypes = [vp, ci, vp, cu, cd, cd]
    L.mjb_forward_envs.argtypes = [vp, vp]
    L.mjb_engine_flags_peek.argtypes = [vp, pci]
    L.mjb_model_kernel_source.argtypes = [vp, ci, ci, ci, ci, ci, ctypes.c_char_p, cl]
    L.mjb_model_kernel_source.restype = cl
    L.mjb_kernel_source.argtypes = [vp, ci, ctypes.c_char_p, cl]
    L.mjb_kernel_source.restype = cl
    L.mjb_kernel_load.argtypes = [vp, ci, ctypes.c_char_p, cl]
    L.mjb_kernel_unload.argtypes = [vp, ci]
    L.mjb_model_kernel_source_params.argtypes = [vp, ci, ci, ci, ci, ci, ci, ctypes.c_char_p, cl]
    L.mjb_model_kernel_source_params.restype = cl
    L.mjb_set_env_param.argtypes = [vp, ctypes.c_char_p, vp, ci, ci, vp]
    L.mjb_get_env_param.argtypes = [vp, ctypes.c_char_p, vp]
    L.mjb_clear_env_param.argtypes = [vp, ctypes.c_char_p]
    L.mjb_env_param_mask.argtypes = [vp, pci]
    L.mjb_inverse.argtypes = [vp]
    L.mjb_step.argtypes = [vp, ci]
    L.mjb_rollout.argtypes = [vp, ci, ci, cu, cu, cd, vp, vp, ci]
    L.mjb_rollout_ctrl.argtypes = [vp, ci, vp, cl, cl, vp, vp, ci]
    L.mjb_set_feedback.argtypes = [vp, vp, vp, vp, vp]
    L.mjb_set_feedback.restype = ci
    L.mjb_set_feedback_noise.argtypes = [vp, vp, vp, ci, ci]
    L.mjb_set_feedback_noise.restype = ci
    L.mjb_feedback_ctrl.argtypes = [vp, ci]
    L.mjb_feedback_ctrl.restype = ci
    L.mjb_obs_spec_create.argtypes = [vp, ci, ci, vp, ci, vp, ci, vp, ci, vp, pvp]
    L.mjb_obs_spec_free.argtypes = [vp]
    L.mjb_obs_dim.argtypes = [vp]
    L.mjb_obs_gather.argtypes = [vp, vp, vp]
    L.mjb_transition_fd.argtypes = [vp, cd, ci, vp, vp]
    L.mjb_transition_fd_pinned.argtypes = [vp, cd, ci, ctypes.POINTER(ctypes.POINTER(cd)), ctypes.POINTER(ctypes.POINTER(cd))]
    L.mjb_transition_fd_pinned.restype = ci
    L.mjb_transition_fd_points.argtypes = [vp, ci, vp, cl, cl, vp, cl, cl, vp, cl, cl, vp, cl, cl, cd, ci, vp, vp]
    L.mjb_transition_fd_points.restype = ci
    L.mjb_fd_points_slabs.argtypes = [vp]
    L.mjb_fd_points_slabs.restype = ci
    L.mjb_transition_fd_sensors.argtypes = [vp, cd, ci] + [ctypes.POINTER(ctypes.POINTER(cd))] * 4
    L.mjb_transition_fd_sensors.restype = ci
    L.mjb_transition_fd_points_sensors.argtypes = [vp, ci, vp, cl, cl, vp, cl, cl, vp, cl, cl, vp, cl, cl, cd, ci, vp, vp, vp, vp]
    L.mjb_transition_fd_points_sensors.restype = ci
    L.mjb_lqr_backward.argtypes = [vp, ctypes.POINTER(LqrBackwardStruct)]
    L.mjb_lqr_backward.restype = ci
    L.mjb_lqr_backward_box.argtypes = [vp, ctypes.POINTER(LqrBackwardBoxStruct)]
    L.mjb_lqr_backward_box.restype = ci
    L.mjb_lqr_candidates.argtypes = [vp, ctypes.POINTER(LqrCandidatesStruct)]
    L.mjb_lqr_candidates.restype = ci
    L.mjb_lqr_dare.argtypes = [vp, ctypes.POINTER(LqrDareStruct)]
    L.mjb_lqr_dare.restype = ci
    L.mjb_lqr_eig.argtypes = [vp, ctypes.POINTER(LqrEigStruct)]
    L.mjb_lqr_eig.restype = ci
    L.mjb_lqr_dlyap.argtypes = [vp, ctypes.POINTER(LqrDlyapStruct)]
    L.mjb_lqr_dlyap.restype = ci
    L.mjb_setpoint_ctrl.argtypes = [vp, ctypes.POINTER(SetpointStruct)]
    L.mjb_setpoint_ctrl.restype = ci
    L.mjb_lqr_gemm_tn.argtypes = [vp, ci, ci, ci, vp, vp, vp]
    L.mjb_lqr_gemm_tn.restype = ci
    L.mjb_traj_cost.argtypes = [vp, ctypes.POINTER(TrajCostStruct)]
    L.mjb_traj_cost.restype = ci
    L.mjb_traj_select.argtypes = [vp, ctypes.POINTER(TrajSelectStruct)]
    L.mjb_traj_select.restype = ci
    L.mjb_feedback_law.argtypes = [vp, ctypes.POINTER(FeedbackLawStruct), ci]
    L.mjb_rollout_feedback.argtypes = [vp, ctypes.POINTER(FeedbackLawStruct), ci, vp, vp, ci]
    L.mjb_jac.argtypes = [vp, ci, vp, vp, vp, vp]
    L.mjb_profile_get.argtypes = [vp, vp]
    L.mjb_profile_get.restype = ci
    L.mjb_profile_env_get.argtypes = [vp, vp]
    L.mjb_step_schedule.argtypes = [vp, vp]
    L.mjb_step_schedule.restype = ci
    L.mjb_profile_env_get.restype = ci
    L.mjb_debug_forward.argtypes = [vp]
    L.mjb_debug_get.argtypes = [vp, ctypes.c_char_p, vp, cl]
    pcl = ctypes.POINTER(cl)
    L.mjb_model_name2id.argtypes = [vp, ci, ctypes.c_char_p]
    L.mjb_model_name2id.restype = ci
    L.mjb_model_id2name.argtypes = [vp, ci, ci]
    L.mjb_model_id2name.restype = ctypes.c_char_p
    L.mjb_model_field.argtypes = [vp, ctypes.c_char_p, pvp, pcl, pci]
    L.mjb_model_field_at.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_char_p), pvp, pcl, pci]
    L.mjb_model_load_xml.argtypes = [ctypes.c_char_p, pvp]
    L.mjb_model_load_xml_string.argtypes = [ctypes.c_char_p, ctypes.c_char_p, pvp]
    L.mjb_model_save.argtypes = [vp, ctypes.c_char_p]
    L.mjb_model_load.argtypes = [ctypes.c_char_p, pvp]
    L.mjb_integrate_pos.argtypes = [vp, ci, vp, vp, cd]
    L.mjb_differentiate_pos.argtypes = [vp, ci, vp, cd, vp, vp]
    L.mjb_host_view.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.POINTER(cd)), pcl]
    L.mjb_sync_to_host.argtypes = [vp]
    L.mjb_sync_to_device.argtypes = [vp, ci]
    L.mjb_step_host.argtypes = [vp, ci, ci]
    L.mjb_mirror_edited_mask.argtypes = [vp, ctypes.POINTER(ci)]
    L.mjb_mirror_commit.argtypes = [vp, ci]
    L.mjb_step_host_auto.argtypes = [vp, ci, ci, ctypes.POINTER(ci)]
    for name in ("mjb_model_create", "mjb_model_set_disableactuator", "mjb_model_set_solver", "mjb_data_create", "mjb_set_stream",
                 "mjb_sync", "mjb_data_info", "mjb_array_ptr", "mjb_get_array", "mjb_set_array", "mjb_get_counters", "mjb_reset",
                 "mjb_forward", "mjb_inverse", "mjb_kernel_load", "mjb_kernel_unload", "mjb_step", "mjb_rollout", "mjb_rollout_ctrl", "mjb_obs_spec_create", "mjb_obs_dim", "mjb_obs_gather",
                 "mjb_transition_fd", "mjb_jac", "mjb_debug_forward", "mjb_debug_get", "mjb_model_field", "mjb_model_field_at", "mjb_model_save",
                 "mjb_model_load", "mjb_model_load_xml", "mjb_model_load_xml_string", "mjb_integrate_pos", "mjb_differentiate_pos", "mjb_host_view", "mjb_sync_to_host", "mjb_sync_to_device",
                 "mjb_step_host", "mjb_mirror_edited_mask", "mjb_mirror_commit", "mjb_step_host_auto", "mjb_engine_flags",
                 "mjb_reset_envs", "mjb_forward_envs", "mjb_engine_flags_peek", "mjb_set_env_param", "mjb_get_env_param", "mjb_clear_env_param",
                 "mjb_env_param_mask", "mjb_feedback_law", "mjb_rollout_feedback"):
        getattr(L, name).restype = ci
    _LIB = L
    return L


def _check(rc: int) -> None:
    """Turn a C status code into the exception of ``exceptions.raise_for_status``."""
    if rc != 0:
        raise_for_status(rc, load_library().mjb_last_error().decode())


class _CudaArray:
    """``__cuda_array_interface__`` shim so torch can wrap library-owned device memory zero-copy."""

    def __init__(self, ptr: int, shape: tuple[int, ...], typestr: str, owner: object):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}
        self._owner = owner


def _manifold_batch(arr: np.ndarray, n: int, what: str) -> int:
    """Batch size of a caller-owned [n] / [batch, n] float64 vector the C side edits in place."""
    if not isinstance(arr, np.ndarray) or arr.dtype != np.float64 or not arr.flags.c_contiguous or not arr.flags.writeable:
        raise ConfigError(f"{what} must be a writeable C-contiguous float64 numpy array (it is modified in place)")
    if n == 0 or arr.size % n or arr.ndim not in (1, 2) or arr.shape[-1] != n:
        raise ConfigError(f"{what} must have shape [{n}] or [batch, {n}]")
    return arr.size // n


def _ids(seq: Sequence[int]):
    arr = np.ascontiguousarray(np.asarray(list(seq), dtype=np.int32))
    return arr, (arr.ctypes.data if arr.size else None)



# ----------------------------------------------------------------------------------
# per-model specialised kernels (include/mjbatch.h: mjb_*kernel_source, mjb_kernel_load)
# ----------------------------------------------------------------------------------
_WARNED_NO_SPEC = False
_CSRC = os.path.join(_HERE, "csrc")
_JIT_DIR = os.path.join(_HERE, "_jit")


def _source_from(fn, *args) -> str:
    n = fn(*args, None, 0)
    if n < 0:
        _check(-1)
    buf = ctypes.create_string_buffer(int(n) + 1)
    fn(*args, buf, int(n) + 1)
    return buf.value.decode()


def spec_scheduler(source: str) -> str | None:
    """The machine scheduler the specialised kernel is compiled with — a stated rule, not a retry: the iterative ILP strategy
    (measured on the same box, default scheduler -> iterative: humanoid +4 %, drone2 +8 %, cart-pole +5 %) for every model that can
    have constraints worth scheduling for (row cap ``nefc_max >= 8``, or one wave per environment); LLVM's default for the
    degenerate ones (pendulum: 2 rows, the tests' BASE_XML: 2 rows), whose kernels are tiny and where the one compiler crash
    with this flag was seen (ROCm 7.2.0 clang, greedy register allocator, ``profiles/r02_hipcc_iterative_ilp_crash.txt``)."""
    import re

    g = re.search(r"#define MJB_SPEC_G (\d+)", source)
    ne = re.search(r"nefc_max == (\d+)", source)
    lanes, rows = (int(g.group(1)) if g else 0), (int(ne.group(1)) if ne else 0)
    return "iterative-ilp" if lanes == 64 or rows >= 8 else None


def _private_cache_dir() -> str:
    """Per-user cache for read-only installs: created 0700, must be a real directory owned by this user with no group / other
    write bit (another local user must not be able to plant a code object that ``hipModuleLoadData`` would then run)."""
    base = os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache")
    path = os.path.join(base, "mujoco_template_amd", "jit")
    try:
        os.makedirs(path, mode=0o700, exist_ok=True)
        st = os.lstat(path)
    except OSError as exc:
        raise TemplateError(f"no writable cache directory for the specialised kernel: {exc}") from exc
    import stat

    if not stat.S_ISDIR(st.st_mode) or st.st_uid != os.getuid() or (st.st_mode & 0o022):
        raise TemplateError(f"refusing the kernel cache {path}: it must be a directory owned by uid {os.getuid()} without group/other write access")
    return path


def _read_private(path: str) -> bytes:
    """Read a cached code object without following a symlink at the final component.  Objects in the in-tree cache carry the
    trust of the package itself (they ship beside ``libmjbatch.so``); anything else must be owned by this user and not writable
    by others."""
    fd = os.open(path, os.O_RDONLY | getattr(os, "O_NOFOLLOW", 0))
    try:
        st = os.fstat(fd)
        in_tree = os.path.dirname(os.path.abspath(path)) == os.path.abspath(_JIT_DIR)
        if not in_tree and (st.st_uid != os.getuid() or (st.st_mode & 0o022)):
            raise TemplateError(f"refusing the cached kernel {path}: not owned by uid {os.getuid()} or writable by others")
        with os.fdopen(fd, "rb", closefd=False) as fh:
            return fh.read()
    finally:
        os.close(fd)


def compile_spec(source: str, *, force: bool = False) -> str:
    """Compile a specialised translation unit (``mjb_*kernel_source``) to a gfx950 code object; returns its path.

    Cached in-tree (``mujoco_template_amd/_jit/``, keyed by the source text, the kernel headers and the scheduler rule), so
    the objects built by ``__graft_entry__.build()`` on a GPU-less machine travel with the tree; a read-only install uses a
    private per-user cache (0700, ownership checked).  hipcc cross-compiles without a GPU.
    """
    import hashlib
    import shutil
    import subprocess

    extra = os.environ.get("MJB_SPEC_FLAGS", "").split()        # experiments, e.g. -DMJB_WPS=3 (register budget for 3 waves/SIMD)
    sched = spec_scheduler(source)
    h = hashlib.sha1((source + " ".join(extra) + f" sched={sched} nolicm").encode())
    for f in ("mjb_types.hpp", "mjb_device.hpp", "mjb_kernels.hpp"):
        with open(os.path.join(_CSRC, f), "rb") as fh:
            h.update(fh.read())
    key = h.hexdigest()[:20]
    jit_dir = _JIT_DIR
    try:
        os.makedirs(jit_dir, exist_ok=True)
        if not os.access(jit_dir, os.W_OK):
            raise OSError("not writable")
    except OSError:                                            # read-only install
        jit_dir = _private_cache_dir()
    out = os.path.join(jit_dir, f"k_step_spec_{key}.hsaco")
    if os.path.exists(out) and not force:
        return out
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise TemplateError("hipcc not found: cannot specialise the step kernel (the generic kernel remains available)")
    src = os.path.join(jit_dir, f"k_step_spec_{key}.hip")
    tmp = out + f".tmp{os.getpid()}"
    try:
        fd = os.open(src, os.O_WRONLY | os.O_CREAT | os.O_TRUNC | getattr(os, "O_NOFOLLOW", 0), 0o600)
        with os.fdopen(fd, "w") as fh:
            fh.write(source)
    except OSError as exc:
        raise TemplateError(f"cannot write the specialised kernel source: {exc}") from exc
    # same floating-point flags as csrc/Makefile (contraction per source expression, correctly rounded division / sqrt): bitwise equal to the generic kernel
    # -disable-machine-licm: the step kernel is one persistent loop around the whole forward pipeline; hoisting the body's literal
    # constants out of it costs more registers than the kernel has (csrc/Makefile, STEPFLAGS)
    base = [hipcc, "--genco", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-ffp-contract=on", "-mllvm", "-disable-machine-licm"]
    tail = [*extra, "-I", _CSRC, "-o", tmp, src]
    if "#define MJB_SPEC_KERNEL 2" in source:                   # the finite-difference kernel has no persistent loop around its body
        base = [x for x in base if x not in ("-mllvm", "-disable-machine-licm")]
    attempts = [[*base, "-mllvm", f"-amdgpu-sched-strategy={sched}", *tail], [*base, *tail]] if sched else [[*base, *tail]]
    err = ""
    for k, cmd in enumerate(attempts):
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except (OSError, subprocess.SubprocessError) as exc:
            raise TemplateError(f"hipcc could not be run: {exc}") from exc
        if r.returncode == 0 and os.path.exists(tmp):
            if k > 0:                                          # the rule's scheduler failed: say so, with the evidence
                import warnings

                warnings.warn(f"hipcc failed with -amdgpu-sched-strategy={sched} on this specialised kernel; compiled with the default "
                              f"scheduler instead (same arithmetic).  stderr tail:\n{err[-1200:]}", RuntimeWarning, stacklevel=2)
            break
        err = r.stderr
        if os.path.exists(tmp):
            os.remove(tmp)
    else:
        raise TemplateError("specialised kernel failed to compile:\n" + err[-2000:])
    os.replace(tmp, out)
    return out


class ObsSpecHandle:
    def __init__(self, sim: "BatchSim", flags: int, site_ids, body_ids, geom_ids, subtree_ids):
        L = load_library()
        self.sim = sim
        self.ptr = ctypes.c_void_p()
        s, sp = _ids(site_ids); b, bp = _ids(body_ids); g, gp = _ids(geom_ids); t, tp = _ids(subtree_ids)
        _check(L.mjb_obs_spec_create(sim.ptr, flags, s.size, sp, b.size, bp, g.size, gp, t.size, tp, ctypes.byref(self.ptr)))
        self.dim = int(L.mjb_obs_dim(self.ptr))

    def __del__(self):
        try:
            if self.ptr:
                load_library().mjb_obs_spec_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


MIRROR_FIELDS = ("qpos", "qvel", "ctrl", "qacc", "qacc_warmstart", "time")     # bit order of the field masks of mjb_sync_to_device / mjb_step_host

# model fields that may differ per environment (mjb_set_env_param), in the bit order of the C masks (MJB_PRM_*)
ENV_PARAM_FIELDS = ("body_mass", "body_inertia", "dof_damping", "dof_armature", "actuator_gear", "actuator_gainprm", "actuator_biasprm",
                    "geom_friction", "gravity")


def env_param_shape(compiled: CompiledModel, name: str) -> tuple[int, ...]:
    """Per-environment shape of a field of ``ENV_PARAM_FIELDS``."""
    m = compiled
    shapes = {"body_mass": (m.nbody,), "body_inertia": (m.nbody, 3), "dof_damping": (m.nv,), "dof_armature": (m.nv,),
              "actuator_gear": (m.nu, 6), "actuator_gainprm": (m.nu, 3), "actuator_biasprm": (m.nu, 3), "geom_friction": (m.ngeom, 3),
              "gravity": (3,)}
    if name not in shapes:
        raise ConfigError(f"{name!r} is not a per-environment model field (one of {', '.join(ENV_PARAM_FIELDS)})")
    return shapes[name]


def env_param_mask(params) -> int:
    """Bit mask (MJB_PRM_*) of a collection of field names."""
    mask = 0
    for name in params:
        if name not in ENV_PARAM_FIELDS:
            raise ConfigError(f"{name!r} is not a per-environment model field (one of {', '.join(ENV_PARAM_FIELDS)})")
        mask |= 1 << ENV_PARAM_FIELDS.index(name)
    return mask


class DeviceModel:
    """Handle of ``mjbModel`` (host copy of the compiled model inside the library)."""

    def __init__(self, compiled: CompiledModel | None, *, _ptr: ctypes.c_void_p | None = None):
        L = load_library()
        if _ptr is not None:                                   # adopted handle (DeviceModel.load)
            self.ptr, self._packed = _ptr, None
            self.compiled = self._compiled_from_library()
            return
        self.compiled = compiled
        self._packed = PackedTable(compiled)
        p = self._packed
        self.ptr = ctypes.c_void_p()
        _check(L.mjb_model_create(p.n, ctypes.cast(p.names, ctypes.c_void_p), ctypes.cast(p.ptrs, ctypes.c_void_p),
                                  ctypes.cast(p.dtypes, ctypes.c_void_p), ctypes.cast(p.counts, ctypes.c_void_p), ctypes.byref(self.ptr)))

    # -- MjModel.from_binary_path / mj_saveModel (reference model.py:28-31,:49) -----------------------
    @classmethod
    def load(cls, path: str) -> "DeviceModel":
        ptr = ctypes.c_void_p()
        _check(load_library().mjb_model_load(os.fsencode(path), ctypes.byref(ptr)))
        return cls(None, _ptr=ptr)

    def save(self, path: str) -> None:
        _check(load_library().mjb_model_save(self.ptr, os.fsencode(path)))

    # -- MjModel.from_xml_path / from_xml_string (reference model.py:22-27): the native MJCF compiler -----
    @classmethod
    def load_xml(cls, path: str) -> "DeviceModel":
        ptr = ctypes.c_void_p()
        _check(load_library().mjb_model_load_xml(os.fsencode(os.path.abspath(path)), ctypes.byref(ptr)))
        return cls(None, _ptr=ptr)

    @classmethod
    def load_xml_string(cls, xml_text: str, base_dir: str = ".") -> "DeviceModel":
        ptr = ctypes.c_void_p()
        _check(load_library().mjb_model_load_xml_string(xml_text.encode(), os.fsencode(os.path.abspath(base_dir)), ctypes.byref(ptr)))
        return cls(None, _ptr=ptr)

    def fields(self) -> dict[str, np.ndarray]:
        """Every field of the model table as a numpy copy (``mjb_model_field_at``)."""
        L = load_library()
        out: dict[str, np.ndarray] = {}
        name, ptr, cnt, dt = ctypes.c_char_p(), ctypes.c_void_p(), ctypes.c_long(), ctypes.c_int()
        i = 0
        while L.mjb_model_field_at(self.ptr, i, ctypes.byref(name), ctypes.byref(ptr), ctypes.byref(cnt), ctypes.byref(dt)) == 0:
            ctype, npdt = {0: (ctypes.c_double, np.float64), 1: (ctypes.c_int, np.int32), 2: (ctypes.c_ubyte, np.uint8)}[dt.value]
            n = int(cnt.value)
            out[name.value.decode()] = (np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(n,)).astype(npdt, copy=True)
                                        if n else np.zeros(0, dtype=npdt))
            i += 1
        return out

    def _compiled_from_library(self) -> CompiledModel:
        from ._pack import compiled_from_fields

        return compiled_from_fields(self.fields())

    # -- names (mj_name2id / mj_id2name) ----------------------------------------------------------------
    def name2id(self, objtype: int, name: str) -> int:
        return int(load_library().mjb_model_name2id(self.ptr, int(objtype), str(name).encode()))

    def id2name(self, objtype: int, idx: int) -> str | None:
        r = load_library().mjb_model_id2name(self.ptr, int(objtype), int(idx))
        return r.decode() if r is not None else None

    # -- position manifold (mj_integratePos / mj_differentiatePos), host float64, batched -------------
    def integrate_pos(self, qpos: np.ndarray, qvel: np.ndarray, dt: float) -> None:
        """In place on ``qpos`` ([nq] or [batch, nq], float64, C-contiguous)."""
        batch = _manifold_batch(qpos, self.compiled.nq, "qpos")
        v = np.ascontiguousarray(qvel, dtype=np.float64)
        if v.size != batch * self.compiled.nv:
            raise ConfigError("mj_integratePos: qvel must have nv entries per environment")
        _check(load_library().mjb_integrate_pos(self.ptr, batch, qpos.ctypes.data, v.ctypes.data, float(dt)))

    def differentiate_pos(self, qvel: np.ndarray, dt: float, qpos1: np.ndarray, qpos2: np.ndarray) -> None:
        """``qvel <- (qpos2 (-) qpos1) / dt`` in place on ``qvel`` ([nv] or [batch, nv], float64, C-contiguous)."""
        batch = _manifold_batch(qvel, self.compiled.nv, "qvel")
        q1 = np.ascontiguousarray(qpos1, dtype=np.float64)
        q2 = np.ascontiguousarray(qpos2, dtype=np.float64)
        if q1.size != batch * self.compiled.nq or q2.size != q1.size:
            raise ConfigError("mj_differentiatePos: qpos1 / qpos2 must have nq entries per environment")
        _check(load_library().mjb_differentiate_pos(self.ptr, batch, qvel.ctypes.data, float(dt), q1.ctypes.data, q2.ctypes.data))

    def set_disableactuator(self, mask: int) -> None:
        _check(load_library().mjb_model_set_disableactuator(self.ptr, int(mask)))

    def set_solver(self, iterations: int, tolerance: float) -> None:
        _check(load_library().mjb_model_set_solver(self.ptr, int(iterations), float(tolerance)))

    def _model_source(self, kind: int, dtype: int, lanes: int, nconmax: int, nefcmax: int, params=()) -> str:
        return _source_from(load_library().mjb_model_kernel_source_params, self.ptr, kind, dtype, int(lanes), int(nconmax), int(nefcmax),
                            env_param_mask(params))

    def spec_source(self, *, lanes: int = 0, nconmax: int = 0, nefcmax: int = 0, params=()) -> str:
        """Translation unit of the specialised fp32 step kernel for these creation arguments (no GPU needed); ``params``: the
        per-environment fields (``ENV_PARAM_FIELDS``) of the data objects it is for."""
        return self._model_source(MJB_KERNEL_STEP, MJB_F32, lanes, nconmax, nefcmax, params)

    def step2_spec_source(self, *, lanes: int = 0, nconmax: int = 0, nefcmax: int = 0, params=()) -> str | None:
        """Translation unit of the specialised two-wave step kernel (small batches), or None when that kernel does not apply."""
        try:
            return self._model_source(MJB_KERNEL_STEP2, MJB_F32, lanes, nconmax, nefcmax, params)
        except TemplateError:
            return None

    def fd_spec_source(self, *, dtype: str = "float32", lanes: int = 0, nconmax: int = 0, nefcmax: int = 0, params=()) -> str:
        """Translation unit of the specialised float64 finite-difference kernel for these creation arguments (no GPU needed)."""
        return self._model_source(MJB_KERNEL_FD, MJB_F32 if dtype == "float32" else MJB_F64, lanes, nconmax, nefcmax, params)

    def __del__(self):
        try:
            if self.ptr:
                load_library().mjb_model_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


class BatchSim:
    """``batch`` replicas of one model resident on one GPU (handle of ``mjbData``)."""

    def __init__(self, model: DeviceModel, batch: int, *, dtype: str = "float32", lanes: int = 0, nconmax: int = 0,
                 nefcmax: int = 0, device: int = 0, env0: int = 0, specialize: bool | None = None):
        L = load_library()
        if dtype not in ("float32", "float64"):
            raise ConfigError("dtype must be 'float32' or 'float64'")
        self.model = model
        self.batch = int(batch)
        self.dtype = dtype
        self.np_dtype = np.float32 if dtype == "float32" else np.float64
        self.device = int(device)
        self.ptr = ctypes.c_void_p()
        _check(L.mjb_data_create(model.ptr, self.batch, MJB_F32 if dtype == "float32" else MJB_F64, int(lanes), int(nconmax),
                                 int(nefcmax), self.device, int(env0), ctypes.byref(self.ptr)))
        info = [ctypes.c_int() for _ in range(6)]
        _check(L.mjb_data_info(self.ptr, *[ctypes.byref(x) for x in info]))
        self.lanes, self.nconmax, self.nefcmax, self.lds_bytes_per_env = info[2].value, info[3].value, info[4].value, info[5].value
        self.specialized = False
        self.fd_specialized = False
        self._fd_spec_tried = False                                 # the FD kernel is specialised by the first transition_fd
        self._spec_policy = specialize                             # None: default (on unless MJB_SPECIALIZE=0); True: required; False: never
        self._specialize_by_policy(self.specialize, "step kernel", default=dtype == "float32", once_per_process=True)

    # -- per-model specialised kernels ------------------------------------------------
    def _specialize_by_policy(self, specialize, what: str, *, default: bool, once_per_process: bool = False) -> None:
        """Run ``specialize`` under the ``specialize=`` policy of this object: None = where ``default`` says so unless
        MJB_SPECIALIZE=0, True = required (a failure raises), False = never.  A default that cannot be built falls back to the
        generic kernel with one warning (per object, or per process with ``once_per_process``)."""
        policy = self._spec_policy
        if not (policy if policy is not None else default and os.environ.get("MJB_SPECIALIZE", "1") != "0"):
            return
        try:
            specialize()
        except TemplateError as exc:
            if policy:
                raise
            global _WARNED_NO_SPEC
            if once_per_process:
                if _WARNED_NO_SPEC:
                    return
                _WARNED_NO_SPEC = True
            import warnings

            warnings.warn(f"{what} not specialised, using the generic kernel: {exc}", RuntimeWarning, stacklevel=3)

    def _load_kernel(self, kind: int) -> None:
        """This object's translation unit of ``kind`` -> code object (compiled, or from the cache) -> used by every later launch."""
        image = _read_private(compile_spec(_source_from(load_library().mjb_kernel_source, self.ptr, kind)))
        _check(load_library().mjb_kernel_load(self.ptr, kind, image, len(image)))

    def spec_source(self) -> str:
        return _source_from(load_library().mjb_kernel_source, self.ptr, MJB_KERNEL_STEP)

    def specialize(self) -> None:
        """Compile (or fetch from the in-tree cache) the step kernel specialised to this model's sizes and LDS layout and
        use it for every later launch on this object.  float32 only; identical arithmetic to the generic kernel."""
        if self.dtype != "float32":
            raise ConfigError("only the float32 step kernel is specialised")
        self._load_kernel(MJB_KERNEL_STEP)
        self.specialized = True
        # small batches are stepped by the two-wave kernel where it applies (its source length is -1 where not): specialise that one too
        if self.batch <= 1024 and load_library().mjb_kernel_source(self.ptr, MJB_KERNEL_STEP2, None, 0) >= 0:
            self._load_kernel(MJB_KERNEL_STEP2)

    def unspecialize(self) -> None:
        _check(load_library().mjb_kernel_unload(self.ptr, MJB_KERNEL_STEP2))
        _check(load_library().mjb_kernel_unload(self.ptr, MJB_KERNEL_STEP))
        self.specialized = False

    def fd_spec_source(self) -> str:
        return _source_from(load_library().mjb_kernel_source, self.ptr, MJB_KERNEL_FD)

    def specialize_fd(self) -> None:
        """The float64 finite-difference kernel behind ``transition_fd`` specialised to this model (sizes, float64 LDS layout,
        the model baked in as constants); identical arithmetic to the generic kernel.  Done lazily by the first ``transition_fd``."""
        self._load_kernel(MJB_KERNEL_FD)
        self.fd_specialized = True

    def unspecialize_fd(self) -> None:
        _check(load_library().mjb_kernel_unload(self.ptr, MJB_KERNEL_FD))
        self.fd_specialized = False

    # -- per-environment model parameters (mjb_set_env_param) -----------------------------------
    def env_param_mask(self) -> int:
        out = ctypes.c_int(0)
        _check(load_library().mjb_env_param_mask(self.ptr, ctypes.byref(out)))
        return int(out.value)

    def env_param_fields(self) -> tuple[str, ...]:
        """The fields that are batched on this object."""
        mask = self.env_param_mask()
        return tuple(f for k, f in enumerate(ENV_PARAM_FIELDS) if (mask >> k) & 1)

    def _respecialize(self, mask_before: int) -> None:
        """The library unloads the specialised kernels when the set of batched fields changes: rebuild them for the new set (the
        kernel source carries the set, so the in-tree cache keeps one code object per set)."""
        if self.env_param_mask() == mask_before:
            return
        if self.specialized:
            self.specialized = False
            self._specialize_by_policy(self.specialize, "step kernel", default=True)
        if self.fd_specialized:
            self.fd_specialized = False
            self._specialize_by_policy(self.specialize_fd, "finite-difference kernel", default=True)

    def set_env_params(self, envs=None, **fields) -> None:
        """Per-environment model parameters (domain randomisation), e.g. ``set_env_params(body_mass=m, gravity=g)``.  Each value is
        ``[batch, *shape]`` or ``[*shape]`` (broadcast to the rows written), shape as in ``env_param_shape``: a torch tensor on this
        object's GPU (copied on the device, enqueued on torch's current stream: nothing crosses to the host) or anything numpy takes
        (host float64, finiteness checked).  ``envs``: the environments whose rows are written, a mask or an index list as for
        ``reset_envs`` (``None`` = all); the other rows keep their values (the model's, the first time a field is set).  Semantics,
        derived quantities and what stays the compiled model's: ``include/mjbatch.h`` / INTEGRATION.md."""
        import torch

        L = load_library()
        mask_before = self.env_param_mask()
        m = self.env_mask(envs)
        self._prm_mask_keep = m
        dev = torch.device(f"cuda:{self.device}")
        keep = []
        try:
            for name, value in fields.items():
                shape = env_param_shape(self.model.compiled, name)
                n = int(np.prod(shape))
                if isinstance(value, torch.Tensor):
                    if value.device != dev:
                        raise ConfigError(f"set_env_params: {name} must live on {dev}, got {value.device}")
                    if value.dtype not in (torch.float32, torch.float64):
                        raise ConfigError(f"set_env_params: {name} must be float32 or float64, got {value.dtype}")
                    if tuple(value.shape) == shape:
                        value = value.reshape(1, n).expand(self.batch, n)
                    elif tuple(value.shape) != (self.batch, *shape):
                        raise ConfigError(f"set_env_params: {name} must have shape {[self.batch, *shape]} or {list(shape)}, got {list(value.shape)}")
                    value = value.reshape(self.batch, n).contiguous()
                    keep.append(value)
                    self.use_torch_stream()
                    _check(L.mjb_set_env_param(self.ptr, name.encode(), ctypes.c_void_p(value.data_ptr()) if n else None,
                                               MJB_F32 if value.dtype == torch.float32 else MJB_F64, 1,
                                               ctypes.c_void_p(m.data_ptr()) if m is not None else None))
                else:
                    arr = np.asarray(value, dtype=np.float64)
                    if arr.shape == shape:
                        arr = np.broadcast_to(arr.reshape(1, n), (self.batch, n))
                    elif arr.shape != (self.batch, *shape):
                        raise ConfigError(f"set_env_params: {name} must have shape {[self.batch, *shape]} or {list(shape)}, got {list(arr.shape)}")
                    arr = np.ascontiguousarray(arr.reshape(self.batch, n))
                    if m is not None:
                        self.use_torch_stream()              # the mask was uploaded on torch's stream
                    _check(L.mjb_set_env_param(self.ptr, name.encode(), arr.ctypes.data if n else None, MJB_F64, 0,
                                               ctypes.c_void_p(m.data_ptr()) if m is not None else None))
        finally:
            self._prm_keep = keep                                    # alive at least until the next call on this object
            self._respecialize(mask_before)

    def env_params(self, name: str) -> np.ndarray:
        """``[batch, *shape]`` float64: the rows of a batched field, or the model's value broadcast (synchronises)."""
        shape = env_param_shape(self.model.compiled, name)
        out = np.zeros((self.batch, *shape), dtype=np.float64)
        _check(load_library().mjb_get_env_param(self.ptr, name.encode(), out.ctypes.data))
        return out

    def clear_env_params(self, *names: str) -> None:
        """Return these fields (none given: every batched one) to the shared model value."""
        mask_before = self.env_param_mask()
        for name in names or self.env_param_fields():
            env_param_shape(self.model.compiled, name)
            _check(load_library().mjb_clear_env_param(self.ptr, name.encode()))
        self._respecialize(mask_before)

    # -- plumbing -----------------------------------------------------------------
    def set_stream(self, stream_handle: int) -> None:
        _check(load_library().mjb_set_stream(self.ptr, ctypes.c_void_p(stream_handle)))

    def use_torch_stream(self) -> None:
        import torch

        stream = torch.cuda.current_stream(self.device)
        self.set_stream(stream.cuda_stream)
        self._torch_stream = stream                                 # the library's stream handle stays valid while it is bound

    def sync(self) -> None:
        _check(load_library().mjb_sync(self.ptr))

    def array_ptr(self, name: str) -> tuple[int, int, int]:
        p, n, dt = ctypes.c_void_p(), ctypes.c_long(), ctypes.c_int()
        _check(load_library().mjb_array_ptr(self.ptr, name.encode(), ctypes.byref(p), ctypes.byref(n), ctypes.byref(dt)))
        return int(p.value or 0), int(n.value), int(dt.value)

    def torch_view(self, name: str):
        """Zero-copy torch tensor [batch, n] over the library-owned device array."""
        import torch

        ptr, n, dt = self.array_ptr(name)
        typestr = {0: "<f4", 1: "<f8", 2: "<i4"}[dt]
        if n == 0 or ptr == 0:
            return torch.zeros((self.batch, 0), device=f"cuda:{self.device}")
        return torch.as_tensor(_CudaArray(ptr, (self.batch, n), typestr, self), device=f"cuda:{self.device}")

    def get(self, name: str) -> np.ndarray:
        _, n, _ = self.array_ptr(name)
        out = np.zeros((self.batch, n), dtype=np.float64)
        if n:
            _check(load_library().mjb_get_array(self.ptr, name.encode(), out.ctypes.data))
        return out

    def set(self, name: str, value: np.ndarray) -> None:
        _, n, _ = self.array_ptr(name)
        arr = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64).reshape(-1, n) if n else np.zeros((self.batch, 0)), (self.batch, n)))
        if n:
            _check(load_library().mjb_set_array(self.ptr, name.encode(), arr.ctypes.data))

    # -- host mirror (mjb_host_view): pinned float64 block, one packed copy per direction ------------
    def host_view(self, name: str) -> np.ndarray:
        """numpy view [batch, n] over the library's pinned float64 mirror of ``name`` (valid while this object lives)."""
        p, n = ctypes.POINTER(ctypes.c_double)(), ctypes.c_long()
        _check(load_library().mjb_host_view(self.ptr, name.encode(), ctypes.byref(p), ctypes.byref(n)))
        if name == "engine_flags":
            return np.ctypeslib.as_array(p, shape=(1,))
        if n.value == 0:
            return np.zeros((self.batch, 0))
        arr = np.ctypeslib.as_array(p, shape=(self.batch, int(n.value)))
        self._keep = getattr(self, "_keep", [])
        self._keep.append(arr)
        return arr

    def sync_to_host(self) -> None:
        _check(load_library().mjb_sync_to_host(self.ptr))

    def sync_to_device(self, field_mask: int) -> None:
        _check(load_library().mjb_sync_to_device(self.ptr, int(field_mask)))

    def mirror_edited_mask(self) -> int:
        """Fields of the pinned mirror block the host edited in place since the library last refreshed / uploaded them (bit order of MIRROR_FIELDS)."""
        out = ctypes.c_int(0)
        _check(load_library().mjb_mirror_edited_mask(self.ptr, ctypes.byref(out)))
        return out.value

    def mirror_commit(self, field_mask: int = 63) -> None:
        _check(load_library().mjb_mirror_commit(self.ptr, int(field_mask)))

    def step_host_auto(self, nstep: int, compare: bool = True) -> int:
        """Edit detection + ``step_host`` + shadow refresh in ONE library call; returns the mask that was uploaded."""
        out = ctypes.c_int(0)
        _check(load_library().mjb_step_host_auto(self.ptr, int(nstep), 1 if compare else 0, ctypes.byref(out)))
        return out.value

    def step_host(self, nstep: int, field_mask: int = 0) -> None:
        """upload the edited mirror fields, ``nstep`` x mj_step (0: mj_forward), refresh the mirror — one library call."""
        _check(load_library().mjb_step_host(self.ptr, int(nstep), int(field_mask)))

    def engine_flags_peek(self) -> int:
        """The same word WITHOUT waiting for the stream (``mjb_engine_flags_peek``): what the launches that have finished so far raised."""
        out = ctypes.c_int(0)
        _check(load_library().mjb_engine_flags_peek(self.ptr, ctypes.byref(out)))
        return int(out.value)

    def engine_flags(self) -> int:
        """Sticky flag word of the batch after waiting for the stream (``mjb_engine_flags``): bit 0 contacts dropped, 1 constraint rows
        dropped, 2 bad-state auto-reset, 3 a ticket-mode launch timed out on a hand-over (the one that makes every synchronising call
        raise ``TemplateError`` until ``reset``).  No copy: the kernels keep the word in pinned host memory."""
        out = ctypes.c_int(0)
        _check(load_library().mjb_engine_flags(self.ptr, ctypes.byref(out)))
        return int(out.value)

    def counters(self) -> dict[str, np.ndarray]:
        out = np.zeros((self.batch, 8), dtype=np.int32)
        _check(load_library().mjb_get_counters(self.ptr, out.ctypes.data))
        return {k: out[:, i] for i, k in enumerate(COUNTER_NAMES)}

    # -- physics ------------------------------------------------------------------
    def reset(self, key: int = -1) -> None:
        _check(load_library().mjb_reset(self.ptr, int(key)))

    def forward(self) -> None:
        _check(load_library().mjb_forward(self.ptr))

    # -- per-environment reset / forward (mjb_reset_envs / mjb_forward_envs): the mask is read on the device ------------------------
    def env_mask(self, mask):
        """``mask`` as a [batch] one-byte torch tensor on this object's GPU (``None`` stays ``None`` = every environment).  A torch bool /
        uint8 tensor on that device is used as it is (zero-copy); an index sequence or a numpy bool array is uploaded once."""
        import torch

        if mask is None:
            return None
        dev = torch.device(f"cuda:{self.device}")
        if isinstance(mask, torch.Tensor):
            if mask.dtype not in (torch.bool, torch.uint8):
                raise ConfigError(f"environment mask must be a bool or uint8 tensor, got {mask.dtype}")
            if tuple(mask.shape) != (self.batch,):
                raise ConfigError(f"environment mask must have shape [{self.batch}], got {list(mask.shape)}")
            if mask.device != dev:
                raise ConfigError(f"environment mask must live on {dev}, got {mask.device}")
            return mask if mask.is_contiguous() else mask.contiguous()
        arr = np.asarray(mask)
        if arr.dtype == np.bool_:
            if arr.shape != (self.batch,):
                raise ConfigError(f"environment mask must have shape [{self.batch}], got {list(arr.shape)}")
            host = arr.astype(np.uint8)
        else:
            if arr.ndim != 1 or (arr.size and not np.issubdtype(arr.dtype, np.integer)):
                raise ConfigError("environment mask must be a bool mask [batch] or a sequence of environment indices")
            idx = arr.astype(np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= self.batch):
                raise ConfigError(f"environment index out of range [0, {self.batch})")
            host = np.zeros(self.batch, dtype=np.uint8)
            host[idx] = 1
        return torch.from_numpy(host).to(dev)

    def reset_envs(self, mask=None, key: int = -1, seed: int = 0, qpos_noise: float = 0.0, qvel_noise: float = 0.0) -> None:
        """mj_resetData / mj_resetDataKeyframe (key < 0: qpos0) of the masked environments only, with optional uniform reset noise
        (``mjb_reset_envs``); the sticky engine flags are left alone.  Runs on the data's stream, no host synchronisation."""
        m = self.env_mask(mask)
        self._mask_keep = m                                         # alive at least until the next masked call on this object
        _check(load_library().mjb_reset_envs(self.ptr, int(key), ctypes.c_void_p(m.data_ptr()) if m is not None else None,
                                             int(seed) & 0xFFFFFFFF, float(qpos_noise), float(qvel_noise)))

    def forward_envs(self, mask=None) -> None:
        """mj_forward of the masked environments only (``mjb_forward_envs``): the others keep every array."""
        m = self.env_mask(mask)
        self._mask_keep_fwd = m
        _check(load_library().mjb_forward_envs(self.ptr, ctypes.c_void_p(m.data_ptr()) if m is not None else None))

    def inverse(self) -> None:
        """mj_inverse on every environment: fills the arrays ``qfrc_inverse`` [B, nv] and ``actuator_moment`` [B, nu*nv]."""
        _check(load_library().mjb_inverse(self.ptr))

    def step(self, nstep: int = 1) -> None:
        _check(load_library().mjb_step(self.ptr, int(nstep)))

    def rollout(self, nstep: int, ctrl_mode: int = CTRL_KEEP, seed: int = 0, step0: int = 0, ctrl_scale: float = 1.0,
                obs_spec: ObsSpecHandle | None = None, obs_out_ptr: int = 0, obs_every: int = 0) -> None:
        _check(load_library().mjb_rollout(self.ptr, int(nstep), int(ctrl_mode), int(seed) & 0xFFFFFFFF, int(step0) & 0xFFFFFFFF,
                                          float(ctrl_scale), obs_spec.ptr if obs_spec else None,
                                          ctypes.c_void_p(obs_out_ptr) if obs_out_ptr else None, int(obs_every)))

    def rollout_ctrl(self, nstep: int, ctrl, obs_spec: ObsSpecHandle | None = None, obs_out_ptr: int = 0, obs_every: int = 0) -> None:
        """Open-loop rollout (``mjb_rollout_ctrl``): ``nstep`` steps, step ``s`` of environment ``e`` applying ``ctrl[e, s]`` (``[B, T, nu]``)
        or ``ctrl[s]`` (``[T, nu]``, every environment), ``T >= nstep``.  ``ctrl`` is a torch tensor on this object's GPU in the data's
        dtype; its own strides address it, so an ``expand``-ed tensor (stride 0) broadcasts without a copy.  The launch goes to torch's
        current stream (``use_torch_stream``) and the tensor is kept referenced until the next call, so the caching allocator cannot
        hand its memory out before the kernel has read it.  Observation ring as in ``rollout``."""
        import torch

        nstep = int(nstep)
        if nstep < 1:
            raise ConfigError("rollout_ctrl: nstep must be >= 1")
        if not isinstance(ctrl, torch.Tensor):
            raise ConfigError(f"rollout_ctrl: ctrl must be a torch tensor on cuda:{self.device}, got {type(ctrl).__name__}")
        want = torch.float32 if self.dtype == "float32" else torch.float64
        if ctrl.dtype != want:
            raise ConfigError(f"rollout_ctrl: ctrl must have the data's dtype {want}, got {ctrl.dtype}")
        if ctrl.device != torch.device(f"cuda:{self.device}"):
            raise ConfigError(f"rollout_ctrl: ctrl must live on cuda:{self.device}, got {ctrl.device}")
        nu = self.model.compiled.nu
        if ctrl.ndim == 2 and ctrl.shape[1] == nu and ctrl.shape[0] >= nstep:
            pass
        elif ctrl.ndim == 3 and ctrl.shape[0] == self.batch and ctrl.shape[2] == nu and ctrl.shape[1] >= nstep:
            pass
        else:
            raise ConfigError(f"rollout_ctrl: ctrl must have shape [T, {nu}] or [{self.batch}, T, {nu}] with T >= nstep = {nstep}, "
                              f"got {list(ctrl.shape)}")
        if nu > 1 and ctrl.stride(-1) != 1:
            ctrl = ctrl.contiguous()
        step_stride, env_stride = (ctrl.stride(0), 0) if ctrl.ndim == 2 else (ctrl.stride(1), ctrl.stride(0))
        self.use_torch_stream()
        self._ctrl_keep = ctrl                                      # alive at least until the next rollout_ctrl on this object
        _check(load_library().mjb_rollout_ctrl(self.ptr, nstep, ctypes.c_void_p(ctrl.data_ptr()) if ctrl.numel() else None,
                                               int(step_stride), int(env_stride), obs_spec.ptr if obs_spec else None,
                                               ctypes.c_void_p(obs_out_ptr) if obs_out_ptr else None, int(obs_every)))

    def set_feedback(self, K: np.ndarray, u0: np.ndarray, q0: np.ndarray, v0: np.ndarray | None = None) -> None:
        m = self.model.compiled
        K = np.ascontiguousarray(K, dtype=np.float64)
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
        q0 = np.ascontiguousarray(q0, dtype=np.float64)
        v0 = np.zeros(m.nv) if v0 is None else np.ascontiguousarray(v0, dtype=np.float64)
        if K.shape != (m.nu, 2 * m.nv) or u0.shape != (m.nu,) or q0.shape != (m.nq,) or v0.shape != (m.nv,):
            raise ConfigError("feedback gains must have shapes K [nu, 2nv], u0 [nu], q0 [nq], v0 [nv]")
        _check(load_library().mjb_set_feedback(self.ptr, K.ctypes.data, u0.ctypes.data, q0.ctypes.data, v0.ctypes.data))

    def set_feedback_noise(self, std: np.ndarray | None, table: np.ndarray | None, env_stride: int = 0) -> None:
        """ctrl noise of the feedback law: ``+ std[a] * table[(step + env * env_stride) % nsteps, a]`` before the clip; None switches it off."""
        if std is None or table is None:
            _check(load_library().mjb_set_feedback_noise(self.ptr, None, None, 0, 0))
            return
        m = self.model.compiled
        std = np.ascontiguousarray(std, dtype=np.float64)
        table = np.ascontiguousarray(table, dtype=np.float64)
        if std.shape != (m.nu,) or table.ndim != 2 or table.shape[1] != m.nu or table.shape[0] < 1:
            raise ConfigError("feedback noise must have shapes std [nu], table [nsteps, nu]")
        _check(load_library().mjb_set_feedback_noise(self.ptr, std.ctypes.data, table.ctypes.data, int(table.shape[0]), int(env_stride)))

    def feedback_ctrl(self, step: int = 0) -> None:
        """Evaluate the feedback law for every environment on the device (fp32: MFMA GEMM) and write ``ctrl`` there."""
        _check(load_library().mjb_feedback_ctrl(self.ptr, int(step)))

    def make_obs_spec(self, flags: int, site_ids=(), body_ids=(), geom_ids=(), subtree_ids=()) -> ObsSpecHandle:
        return ObsSpecHandle(self, flags, site_ids, body_ids, geom_ids, subtree_ids)

    def obs_gather(self, spec: ObsSpecHandle, out_ptr: int) -> None:
        _check(load_library().mjb_obs_gather(self.ptr, spec.ptr, ctypes.c_void_p(out_ptr)))

    def transition_fd(self, eps: float = 1e-6, centered: bool = True, *, copy: bool = True, sensors: bool = False):
        """(A [batch, 2nv, 2nv], B [batch, 2nv, nu]).  ``copy=False`` returns views of the library's pinned result blocks (no
        16 MB host copy at humanoid batch 512), valid until the next ``transition_fd`` on this object.

        ``sensors=True`` returns ``(A, B, C, D)`` with the sensor Jacobians ``C [batch, ns, 2nv] = d sensordata / d[dq; dv]`` and
        ``D [batch, ns, nu] = d sensordata / d ctrl`` (``mjb_transition_fd_sensors``; ``ns = nsensordata``, empty for a model
        without sensors): the same columns, ``A`` and ``B`` bitwise those of the plain call."""
        m = self.model.compiled
        if not self._fd_spec_tried:                                # first call: the per-model specialised kernel, by the same policy as the step kernel
            self._fd_spec_tried = True
            self._specialize_by_policy(self.specialize_fd, "finite-difference kernel", default=True)
        pa, pb = ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_double)()
        if sensors:
            pc, pd = ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_double)()
            _check(load_library().mjb_transition_fd_sensors(self.ptr, float(eps), int(bool(centered)), ctypes.byref(pa), ctypes.byref(pb),
                                                             ctypes.byref(pc), ctypes.byref(pd)))
        else:
            _check(load_library().mjb_transition_fd_pinned(self.ptr, float(eps), int(bool(centered)), ctypes.byref(pa), ctypes.byref(pb)))
        A = np.ctypeslib.as_array(pa, shape=(self.batch, 2 * m.nv, 2 * m.nv))
        Bv = np.ctypeslib.as_array(pb, shape=(self.batch, 2 * m.nv, m.nu)) if m.nu else np.zeros((self.batch, 2 * m.nv, 0))
        if not sensors:
            return (A.copy(), Bv.copy()) if copy else (A, Bv)
        ns = m.nsensordata
        C = np.ctypeslib.as_array(pc, shape=(self.batch, ns, 2 * m.nv)) if ns else np.zeros((self.batch, 0, 2 * m.nv))
        D = np.ctypeslib.as_array(pd, shape=(self.batch, ns, m.nu)) if ns and m.nu else np.zeros((self.batch, ns, m.nu))
        return (A.copy(), Bv.copy(), C.copy(), D.copy()) if copy else (A, Bv, C, D)

    def transition_fd_points(self, qpos, qvel, ctrl, qacc_warmstart=None, *, eps: float = 1e-6, centered: bool = True, out=None,
                             sensors: bool = False):
        """Finite-difference transition matrices at caller-chosen points (``mjb_transition_fd_points``): ``qpos [T, B, nq]``,
        ``qvel [T, B, nv]``, ``ctrl [T, B, nu]`` and ``qacc_warmstart [T, B, nv]`` (``None`` = zeros) are torch tensors on this
        object's GPU in the data's dtype, or ``[B, n]`` for one point per environment.  Their own strides address them: column views
        of a rollout ring and ``expand``-ed tensors are read in place.  Returns ``(A [T, B, 2nv, 2nv], B [T, B, 2nv, nu])`` float64 on
        the GPU (without the leading axis for ``[B, n]`` inputs), or fills ``out=(A, B)``.  Block ``(t, e)`` is bitwise what
        ``transition_fd`` gives for environment ``e`` with the data's rows set to point ``(t, e)``; the data's own state is not
        touched.  Enqueued on torch's current stream, nothing waits for the GPU; the inputs are kept referenced until the next call.
        ``sensors=True`` (``mjb_transition_fd_points_sensors``) returns, or fills in ``out``, ``(A, B, C [T, B, ns, 2nv], D [T, B, ns, nu])``
        with the sensor Jacobians of ``transition_fd(sensors=True)``; ``A`` and ``B`` are bitwise those of the plain call."""
        import torch

        m = self.model.compiled
        nq, nv, nu, B = m.nq, m.nv, m.nu, self.batch
        nx = 2 * nv
        want = torch.float32 if self.dtype == "float32" else torch.float64
        dev = torch.device(f"cuda:{self.device}")
        lead = None
        args, keep = [], []
        for name, x, n, optional in (("qpos", qpos, nq, False), ("qvel", qvel, nv, False), ("ctrl", ctrl, nu, False),
                                     ("qacc_warmstart", qacc_warmstart, nv, True)):
            if x is None and optional:
                args += [None, 0, 0]
                continue
            if not isinstance(x, torch.Tensor):
                raise ConfigError(f"transition_fd_points: {name} must be a torch tensor on {dev}, got {type(x).__name__}")
            if x.dtype != want:
                raise ConfigError(f"transition_fd_points: {name} must have the data's dtype {want}, got {x.dtype}")
            if x.device != dev:
                raise ConfigError(f"transition_fd_points: {name} must live on {dev}, got {x.device}")
            if x.ndim not in (2, 3) or x.shape[-1] != n or x.shape[-2] != B:
                raise ConfigError(f"transition_fd_points: {name} must have shape [T, {B}, {n}] or [{B}, {n}], got {list(x.shape)}")
            T = 1 if x.ndim == 2 else int(x.shape[0])
            if lead is None:
                lead = (x.ndim, T)
            elif lead != (x.ndim, T):
                raise ConfigError(f"transition_fd_points: {name} has {list(x.shape)}: the inputs must agree in rank and in T")
            if n > 1 and x.stride(-1) != 1:
                x = x.contiguous()
            ss, es = (0, x.stride(0)) if x.ndim == 2 else (x.stride(0), x.stride(1))
            if ss < 0 or es < 0:
                raise ConfigError(f"transition_fd_points: {name} has a negative stride")
            keep.append(x)
            args += [ctypes.c_void_p(x.data_ptr()) if x.numel() else None, int(ss), int(es)]
        ndim, T = lead
        if T < 1:
            raise ConfigError("transition_fd_points: T must be >= 1")
        ns = m.nsensordata
        shapes = [("A", (T, B, nx, nx)), ("B", (T, B, nx, nu))] + ([("C", (T, B, ns, nx)), ("D", (T, B, ns, nu))] if sensors else [])
        if out is None:
            res = [torch.empty(shape, device=dev, dtype=torch.float64) for _, shape in shapes]
        else:
            res = list(out)
            if len(res) != len(shapes):
                raise ConfigError(f"transition_fd_points: out must be ({', '.join(n for n, _ in shapes)})")
            for (name, shape), x in zip(shapes, res):
                if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device != dev or not x.is_contiguous() or \
                        tuple(x.shape) not in (shape, shape[1:] if ndim == 2 else shape):
                    raise ConfigError(f"transition_fd_points: out {name} must be a contiguous float64 tensor {list(shape)} on {dev}")
        if not self._fd_spec_tried:                                # the per-model specialised kernel, by transition_fd's policy
            self._fd_spec_tried = True
            self._specialize_by_policy(self.specialize_fd, "finite-difference kernel", default=True)
        self.use_torch_stream()
        self._fd_points_keep = (keep, res)                          # alive at least until the next call on this object
        fn = load_library().mjb_transition_fd_points_sensors if sensors else load_library().mjb_transition_fd_points
        _check(fn(self.ptr, T, *args, float(eps), int(bool(centered)), *[ctypes.c_void_p(x.data_ptr()) if x.numel() else None for x in res]))
        if out is not None:
            return tuple(res)
        return tuple(x[0] for x in res) if ndim == 2 else tuple(res)

    def fd_points_slabs(self) -> int:
        """Slabs the last ``transition_fd_points`` ran in (``mjb_fd_points_slabs``)."""
        return int(load_library().mjb_fd_points_slabs(self.ptr))

    def _lqr_call(self, fn, struct, sizes: dict, arrays: dict, pointers: dict, keep) -> None:
        for k, v in sizes.items():
            setattr(struct, k, int(v))
        for k, v in arrays.items():                                 # (address, step stride, env stride[, dtype code]): mjbStrided / mjbStridedIn
            setattr(struct, k, Strided(v[0] or None, int(v[1]), int(v[2])) if len(v) == 3 else StridedIn(v[0] or None, int(v[1]), int(v[2]), int(v[3])))
        for k, ptr in pointers.items():
            setattr(struct, k, ptr or None)
        self.use_torch_stream()
        self._lqr_keep = keep                                       # temporaries made for this call (possibly on another stream): alive until the next call
        _check(fn(self.ptr, ctypes.byref(struct)))

    def lqr_backward(self, sizes: dict, arrays: dict, pointers: dict, keep=()) -> None:
        """``mjb_lqr_backward`` on raw device addresses: ``sizes`` T, batch, nx, nu; ``arrays`` name -> (address, step stride,
        env stride) of the ``mjbStrided`` inputs; ``pointers`` name -> address of the dense outputs; ``keep``: temporaries of the caller to hold until the next call (the outputs
        need none: they are allocated on the stream the kernel runs on).  Enqueued on torch's current
        stream, nothing waits for the GPU.  ``trajopt.lqr_backward`` is the checked tensor interface on top of it."""
        self._lqr_call(load_library().mjb_lqr_backward, LqrBackwardStruct(), sizes, arrays, pointers, keep)

    def lqr_backward_box(self, sizes: dict, arrays: dict, pointers: dict, keep=()) -> None:
        """``mjb_lqr_backward_box`` on raw device addresses (see ``lqr_backward``): ``arrays`` also holds ``u``, ``pointers`` also
        ``lo``, ``hi`` (0 = unbounded), ``clamped`` and ``qp_iters``."""
        struct, own = LqrBackwardBoxStruct(), ("u", "lo", "hi", "clamped", "qp_iters")
        for k, v in sizes.items():
            setattr(struct.base, k, int(v))
        for k, v in arrays.items():
            setattr(struct if k in own else struct.base, k, Strided(v[0] or None, int(v[1]), int(v[2])))
        for k, ptr in pointers.items():
            setattr(struct if k in own else struct.base, k, ptr or None)
        self._lqr_call(load_library().mjb_lqr_backward_box, struct, {}, {}, {}, keep)

    def lqr_candidates(self, sizes: dict, arrays: dict, pointers: dict, keep=()) -> None:
        """``mjb_lqr_candidates`` on raw device addresses (see ``lqr_backward``)."""
        self._lqr_call(load_library().mjb_lqr_candidates, LqrCandidatesStruct(), sizes, arrays, pointers, keep)

    def lqr_dare(self, sizes: dict, arrays: dict, pointers: dict, keep=()) -> None:
        """``mjb_lqr_dare`` on raw device addresses (see ``lqr_backward``): ``sizes`` batch, nx, nu, max_iter, tol; ``arrays`` A, B, Q, R
        as (address, 0, env stride); ``pointers`` X, K, change (0 = not wanted), iters, status.  ``trajopt.solve_dare`` is the checked
        tensor interface on top of it."""
        struct = LqrDareStruct()
        struct.tol = float(sizes["tol"])
        self._lqr_call(load_library().mjb_lqr_dare, struct, {k: v for k, v in sizes.items() if k != "tol"}, arrays, pointers, keep)

    def lqr_eig(self, sizes: dict, arrays: dict, pointers: dict, keep=()) -> None:
        """``mjb_lqr_eig`` on raw device addresses (see ``lqr_backward``): ``sizes`` batch, nx, nu, feedback_sign, balance, max_sweeps
        (0 = the default cap); ``arrays`` A and, together or not at all, B and K as (address, 0, env stride); ``pointers`` wr, wi, rho,
        scale, sweeps, status.  ``trajopt.closed_loop_poles`` is the checked tensor interface on top of it."""
        self._lqr_call(load_library().mjb_lqr_eig, LqrEigStruct(), sizes, arrays, pointers, keep)

    def lqr_dlyap(self, sizes: dict, arrays: dict, pointers: dict, keep=()) -> None:
        """``mjb_lqr_dlyap`` on raw device addresses (see ``lqr_backward``): ``sizes`` batch, nx, nu, feedback_sign, transpose, max_iter,
        tol; ``arrays`` A, Q and, where given, B, K, R, x0 as (address, 0, env stride) - an address of 0 is an absent array; ``pointers``
        P, J (0 exactly when there is no x0), change (0 = not wanted), iters, status.  ``trajopt.closed_loop_cost`` is the checked tensor
        interface on top of it."""
        struct = LqrDlyapStruct()
        struct.tol = float(sizes["tol"])
        self._lqr_call(load_library().mjb_lqr_dlyap, struct, {k: v for k, v in sizes.items() if k != "tol"}, arrays, pointers, keep)

    def setpoint_ctrl(self, sizes: dict, arrays: dict, pointers: dict, keep=()) -> None:
        """``mjb_setpoint_ctrl`` on raw device addresses (see ``lqr_backward``): ``sizes`` batch, nu, nv, max_sweeps (0 = the default),
        rcond_min; ``arrays`` moment, qfrc as (address, 0, env stride, dtype code: 0 float32, 1 float64); ``pointers`` ctrl, sv, rcond,
        residual, pinv (0 = not wanted), rank, sweeps, status.  ``setpoints.solve_setpoint`` is the checked tensor interface on top of it."""
        struct = SetpointStruct()
        struct.rcond_min = float(sizes["rcond_min"])
        self._lqr_call(load_library().mjb_setpoint_ctrl, struct, {k: v for k, v in sizes.items() if k != "rcond_min"}, arrays, pointers, keep)

    def traj_cost(self, sizes: dict, arrays: dict, pointers: dict, keep=()) -> None:
        """``mjb_traj_cost`` on raw device addresses (see ``lqr_backward``); the state and control entries of ``arrays`` carry a
        fourth element, the dtype code (0 float32, 1 float64).  ``trajopt.trajectory_cost`` is the checked tensor interface."""
        self._lqr_call(load_library().mjb_traj_cost, TrajCostStruct(), sizes, arrays, pointers, keep)

    def traj_select(self, sizes: dict, pointers: dict, keep=()) -> None:
        """``mjb_traj_select`` on raw device addresses; ``sizes`` also holds mode, cand_dtype, out_dtype and temperature."""
        struct = TrajSelectStruct()
        struct.temperature = float(sizes.get("temperature", 0.0))
        self._lqr_call(load_library().mjb_traj_select, struct, {k: v for k, v in sizes.items() if k != "temperature"}, {}, pointers, keep)

    def _feedback_struct(self, arrays: dict, options: dict) -> "FeedbackLawStruct":
        struct = FeedbackLawStruct()
        for k, v in arrays.items():                                 # (address, step stride, env stride, dtype code: 0 float32, 1 float64)
            setattr(struct, k, StridedIn(v[0] or None, int(v[1]), int(v[2]), int(v[3])))
        struct.feedback_sign, struct.clip = int(options["feedback_sign"]), int(bool(options["clip"]))
        for k in ("env_mask", "status", "u_rec"):
            setattr(struct, k, options.get(k) or None)
        struct.u_rec_step_stride, struct.u_rec_env_stride = int(options.get("u_rec_step_stride", 0)), int(options.get("u_rec_env_stride", 0))
        return struct

    def feedback_law(self, arrays: dict, options: dict, t: int = 0, keep=()) -> None:
        """``mjb_feedback_law`` on raw device addresses: ``arrays`` K, u0, q0 and optionally v0 as (address, step stride, env stride, dtype
        code: 0 float32, 1 float64); ``options`` feedback_sign, clip and the addresses env_mask, status, u_rec (0 = absent) with
        u_rec_step_stride / u_rec_env_stride.  Writes ``ctrl`` for step index ``t`` on torch's current stream; nothing waits for the GPU.
        ``feedback.feedback_ctrl`` is the checked tensor interface on top of it."""
        struct = self._feedback_struct(arrays, options)
        self.use_torch_stream()
        self._feedback_keep = keep                                  # alive at least until the next call on this object
        _check(load_library().mjb_feedback_law(self.ptr, ctypes.byref(struct), int(t)))

    def rollout_feedback(self, arrays: dict, options: dict, nstep: int, obs_spec: ObsSpecHandle | None = None, obs_out_ptr: int = 0,
                         obs_every: int = 0, keep=()) -> None:
        """``mjb_rollout_feedback`` on raw device addresses (see ``feedback_law``): per step the law kernel, what ``step(1)`` enqueues and,
        every ``obs_every`` steps, what ``obs_gather`` enqueues into the ring.  ``feedback.rollout_feedback`` is the tensor interface."""
        struct = self._feedback_struct(arrays, options)
        self.use_torch_stream()
        self._feedback_keep = keep
        _check(load_library().mjb_rollout_feedback(self.ptr, ctypes.byref(struct), int(nstep), obs_spec.ptr if obs_spec else None,
                                                   ctypes.c_void_p(obs_out_ptr) if obs_out_ptr else None, int(obs_every)))

    def lqr_gemm_tn(self, a, b):
        """``a [K, M]``, ``b [K, N]`` float64 tensors on this GPU -> ``a.T @ b`` through the kernels' f64 MFMA tile product alone."""
        import torch

        a, b = a.contiguous(), b.contiguous()
        c = torch.empty((a.shape[1], b.shape[1]), dtype=torch.float64, device=a.device)
        self.use_torch_stream()
        _check(load_library().mjb_lqr_gemm_tn(self.ptr, int(a.shape[1]), int(b.shape[1]), int(a.shape[0]), a.data_ptr(), b.data_ptr(), c.data_ptr()))
        return c

    def jac(self, kinds: Sequence[int], ids: Sequence[int]) -> tuple[np.ndarray, np.ndarray]:
        m = self.model.compiled
        k, kp = _ids(kinds); i, ip = _ids(ids)
        jp = np.zeros((self.batch, k.size, 3, m.nv))
        jr = np.zeros((self.batch, k.size, 3, m.nv))
        _check(load_library().mjb_jac(self.ptr, k.size, kp, ip, jp.ctypes.data, jr.ctypes.data))
        return jp, jr

    def profile_get(self) -> np.ndarray:
        out = np.zeros(24, dtype=np.uint64)
        _check(load_library().mjb_profile_get(self.ptr, out.ctypes.data))
        return out

    def schedule_info(self) -> dict:
        """How the last stepping launch mapped work to workgroups (``mjb_step_schedule``)."""
        out = np.zeros(6, dtype=np.int32)
        _check(load_library().mjb_step_schedule(self.ptr, out.ctypes.data))
        return {"launch_steps": int(out[0]), "env_blocks": int(out[1]), "resident_slots": int(out[2]), "chunk_steps": int(out[3]),
                "map": "tickets" if out[3] > 0 else "static", "fair_bit": int(out[4]), "waves_per_env": 2 if out[5] else 1}

    def profile_env_get(self) -> np.ndarray:
        out = np.zeros((self.batch, 4), dtype=np.uint64)
        _check(load_library().mjb_profile_env_get(self.ptr, out.ctypes.data))
        return out

    def debug_forward(self) -> None:
        _check(load_library().mjb_debug_forward(self.ptr))

    def debug_get(self, name: str) -> np.ndarray:
        m = self.model.compiled
        nv = m.nv
        per = {"qM": nv * nv, "qfrc_bias": nv, "qfrc_passive": nv, "qfrc_actuator": nv, "qacc_smooth": nv, "qfrc_constraint": nv,
               "efc_J": self.nefcmax * nv, "efc_aref": self.nefcmax, "efc_D": self.nefcmax, "efc_pos": self.nefcmax,
               "efc_force": self.nefcmax, "con": self.nconmax * 11, "cdof": 6 * nv, "cinert": 10 * m.nbody, "cvel": 6 * m.nbody,
               "efc_type": self.nefcmax}[name]
        out = np.zeros((self.batch, per), dtype=np.int32 if name == "efc_type" else np.float64)
        _check(load_library().mjb_debug_get(self.ptr, name.encode(), out.ctypes.data, out.size))
        return out

    def __del__(self):
        try:
            if self.ptr:
                load_library().mjb_data_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


__all__ = ["BatchSim", "DeviceModel", "ObsSpecHandle", "MIRROR_FIELDS", "ENV_PARAM_FIELDS", "env_param_shape", "build_library", "load_library", "CTRL_KEEP", "CTRL_ZERO", "CTRL_RANDOM", "CTRL_FEEDBACK"]
