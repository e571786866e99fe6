"""The feedback-law kernel (``mjb_feedback_law``, the law of ``mjb_rollout_feedback``) without a GPU.

  1. the kernel source itself (``mjb_feedback.hpp``) compiled for the host (``tests/feedback_host.cpp``, g++ -DMJB_HOST_EMU: one thread
     per lane) on the synthetic joint tables of ``tests/feedback_common.py`` against the numpy restatement (long double = truth,
     float64 = the measure of the bound), all four dtype pairs of (gains, data);
  2. every layout - shared, per environment, per (environment, step), a K base that is 8- but not 16-byte aligned, float32 K with an
     odd environment stride - is bitwise equal to the materialised ``[B, T, ...]`` tensors;
  3. the statuses, the clip, the mask; an environment gives the same bits at any position of any batch;
  4. the argument checker;
  5. the translation unit cross-compiles for gfx950 with 16-byte loads and without scratch, and the library exports both entry points.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import feedback_common as fc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B, T = 5, 3


class FbIn(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("ss", ctypes.c_long), ("es", ctypes.c_long), ("f32", ctypes.c_int)]


class FeedbackLawArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "nq", "nv", "nu", "njnt", "data_f32", "clip", "t")] + [("sign", ctypes.c_double)] + \
               [(n, FbIn) for n in ("K", "u0", "q0", "v0")] + \
               [(n, ctypes.c_void_p) for n in ("qpos", "qvel", "ctrl", "jnt_type", "jnt_qposadr", "jnt_dofadr", "ctrllimited", "ctrlrange",
                                               "mask", "status", "u_rec")] + \
               [(n, ctypes.c_long) for n in ("ur_ss", "ur_es")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("feedback") / "libfeedback_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "feedback_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.fbh_arg_error.argtypes = [ctypes.POINTER(FeedbackLawArgs), ctypes.c_long]
    lib.fbh_lds_doubles.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.fbh_waves.argtypes = [ctypes.c_int, ctypes.c_int]
    return lib


class Arr:
    """One strided input: the numpy buffer kept alive, the address of block (0, 0), the strides in elements."""

    def __init__(self, buf, view, ss, es):
        self.buf, self.ptr, self.ss, self.es, self.f32 = buf, view.ctypes.data, ss, es, int(view.dtype == np.float32)


def lay(full, layout, dtype=np.float64, t=None):
    """``full [B, T, *trail]`` as one of the layouts.  shared: block (0, 0) alone, strides 0.  env: the blocks of step ``t`` (default 0),
    env stride n.  full: everything.  half_aligned: full, the base 8 bytes off a 16-byte boundary (float64).  odd: env, environment
    stride n + 1 (float32: most blocks are then not 16-byte aligned)."""
    full = np.ascontiguousarray(full, dtype=dtype)
    nb, nt = full.shape[:2]
    n = int(np.prod(full.shape[2:]))
    if layout == "shared":
        v = full[0, 0].copy()
        return Arr(v, v, 0, 0)
    if layout == "env":
        v = full[:, t or 0].copy()
        return Arr(v, v, 0, n)
    if layout == "odd":
        buf = np.full((nb, n + 1), np.nan, dtype=dtype)
        buf[:, :n] = full[:, t or 0].reshape(nb, n)
        return Arr(buf, buf, 0, n + 1)
    if layout == "half_aligned":
        buf = np.full(full.size + 4, np.nan, dtype=dtype)
        off = 0 if buf.ctypes.data % 16 == 8 else 1                  # numpy allocates at 16-byte boundaries or better
        view = buf[off:off + full.size]
        assert view.ctypes.data % 16 == 8
        view[:] = full.reshape(-1)
        return Arr(buf, view, n, nt * n)
    assert layout == "full"
    return Arr(full, full, n, nt * n)


def host_law(lib, name, K, u0, q0, v0, qpos, qvel, *, t=0, sign=-1, clip=1, data_dtype=np.float64, mask=None, status=None, ctrl=None, rec=None,
             expect=0):
    """The emulated kernel for one step; ``K`` .. ``v0`` are ``Arr`` (``v0`` may be None).  Returns (ctrl [B, nu], status [B])."""
    table, nq, nv, nu = fc.shape(name)
    limited, ctrlrange = fc.limits(nu)
    qpos, qvel = np.ascontiguousarray(qpos, dtype=data_dtype), np.ascontiguousarray(qvel, dtype=data_dtype)
    nb = qpos.shape[0]
    ctrl = np.full((nb, nu), -7.0, dtype=data_dtype) if ctrl is None else ctrl
    status = np.zeros(nb, dtype=np.int32) if status is None else status
    a = FeedbackLawArgs(B=nb, nq=nq, nv=nv, nu=nu, njnt=len(table[0]), data_f32=int(data_dtype == np.float32), clip=clip, t=t, sign=float(sign))
    for key, x in (("K", K), ("u0", u0), ("q0", q0), ("v0", v0)):
        if x is not None:
            setattr(a, key, FbIn(x.ptr, x.ss, x.es, x.f32))
    a.qpos, a.qvel, a.ctrl, a.status = qpos.ctypes.data, qvel.ctypes.data, ctrl.ctypes.data, status.ctypes.data
    a.jnt_type, a.jnt_qposadr, a.jnt_dofadr = (x.ctypes.data for x in table)
    a.ctrllimited, a.ctrlrange = limited.ctypes.data, ctrlrange.ctypes.data
    if mask is not None:
        a.mask = mask.ctypes.data
    if rec is not None:
        assert rec.dtype == data_dtype and rec.flags.c_contiguous
        a.u_rec, a.ur_ss, a.ur_es = rec.ctypes.data, rec.shape[2], rec.shape[1] * rec.shape[2]
    assert lib.fbh_law(ctypes.byref(a)) == expect
    return ctrl, status


def rounded(x, dtype):
    """The values the kernel sees: float32 inputs are the case's values rounded once."""
    return [None if v is None else np.asarray(v, dtype=dtype).astype(np.float64) for v in x]


# ---- 1. the kernel source on host threads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ddtype", [np.float64, np.float32], ids=["data64", "data32"])
@pytest.mark.parametrize("gdtype", [np.float64, np.float32], ids=["gain64", "gain32"])
@pytest.mark.parametrize("name", list(fc.SHAPES))
def test_law_matches_the_restatement(driver, name, gdtype, ddtype):
    """Five environments, a gain per environment and step: step 0 with u = u0 - K dx and the clip, step 2 with u = u0 + K dx unclipped."""
    table, nq, nv, nu = fc.shape(name)
    limited, ctrlrange = fc.limits(nu)
    K, u0, q0, v0, qpos, qvel = fc.problem(table, nq, nv, nu, B, T)
    Kr, u0r, q0r, v0r = rounded((K, u0, q0, v0), gdtype)
    qposr, qvelr = rounded((qpos, qvel), ddtype)
    arrs = [lay(x, "full", gdtype) for x in (K, u0, q0, v0)]
    for t, sign, clip in ((0, -1, 1), (2, 1, 0)):
        ctrl, status = host_law(driver, name, *arrs, qpos, qvel, t=t, sign=sign, clip=clip, data_dtype=ddtype)
        tag = f"{name}/{np.dtype(gdtype).name}/{np.dtype(ddtype).name}/t{t}"
        refs = fc.references(tag, table, nv, Kr[:, t], u0r[:, t], q0r[:, t], v0r[:, t], qposr, qvelr, sign, clip, limited, ctrlrange)
        fc.judge(tag, ctrl, status, refs, f"feedback/host/{tag}", data_f32=ddtype == np.float32)
        if clip:
            assert (status == fc.CLIPPED).any() or name == "hinge_pair"
    # without v0: zeros
    ctrl, status = host_law(driver, name, *arrs[:3], None, qpos, qvel, t=1, data_dtype=ddtype)
    tag = f"{name}/{np.dtype(gdtype).name}/{np.dtype(ddtype).name}/no_v0"
    refs = fc.references(tag, table, nv, Kr[:, 1], u0r[:, 1], q0r[:, 1], None, qposr, qvelr, -1, 1, limited, ctrlrange)
    fc.judge(tag, ctrl, status, refs, f"feedback/host/{tag}", data_f32=ddtype == np.float32)


# ---- 2. layouts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gdtype", [np.float64, np.float32], ids=["gain64", "gain32"])
@pytest.mark.parametrize("name", list(fc.SHAPES))
def test_every_layout_is_bitwise_the_materialised_one(driver, name, gdtype):
    table, nq, nv, nu = fc.shape(name)
    K, u0, q0, v0, qpos, qvel = fc.problem(table, nq, nv, nu, B, T, seed=1)
    full = (K, u0, q0, v0)
    # a shared law: strides 0 against the same values materialised [B, T, ...]
    same = [np.broadcast_to(x[0, 0], x.shape) for x in full]
    want, _ = host_law(driver, name, *[lay(x, "full", gdtype) for x in same], qpos, qvel, t=0)
    for t in (0, 2):
        got, _ = host_law(driver, name, *[lay(x, "shared", gdtype) for x in same], qpos, qvel, t=t)
        assert np.array_equal(got, want), (name, "shared", t)
        got, _ = host_law(driver, name, *[lay(x, "full", gdtype) for x in same], qpos, qvel, t=t)
        assert np.array_equal(got, want), (name, "materialised", t)
    # per (environment, step) at t = 0 and t = 2 against per environment with that step's blocks; the scalar-load paths
    for t in (0, 2):
        want, _ = host_law(driver, name, *[lay(x, "full", gdtype) for x in full], qpos, qvel, t=t)
        got, _ = host_law(driver, name, *[lay(x, "env", gdtype, t=t) for x in full], qpos, qvel, t=t)
        assert np.array_equal(got, want), (name, "env", t)
        special = "odd" if gdtype == np.float32 else "half_aligned"
        Ks = lay(K, special, gdtype, t=t)
        assert any((Ks.ptr + (t * Ks.ss + e * Ks.es) * (4 if Ks.f32 else 8)) % 16 for e in range(B))   # the scalar path does run
        rest = [lay(x, "env" if special == "odd" else "full", gdtype, t=t) for x in (u0, q0, v0)]
        got, _ = host_law(driver, name, Ks, *rest, qpos, qvel, t=t)
        assert np.array_equal(got, want), (name, special, t)
    assert np.isfinite(want).all() and not (want == -7.0).any()


# ---- 3. statuses, the clip, the mask, position independence ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["drone", "humanoid"])
def test_a_value_that_is_not_finite_gives_zeros_and_bit_0(driver, name):
    table, nq, nv, nu = fc.shape(name)
    K, u0, q0, v0, qpos, qvel = fc.problem(table, nq, nv, nu, B, 1, seed=2)
    good, gstat = host_law(driver, name, *[lay(x, "full") for x in (K, u0, q0, v0)], qpos, qvel)
    for what in ("K", "q0", "qpos", "u0", "v0", "qvel", "K_inf"):
        x = {"K": K.copy(), "u0": u0.copy(), "q0": q0.copy(), "v0": v0.copy(), "qpos": qpos.copy(), "qvel": qvel.copy()}
        if what == "K_inf":
            x["K"][2, 0, nu - 1, 1] = np.inf
        elif what in ("qpos", "qvel"):
            x[what][2, -1] = np.nan
        else:
            x[what][2, 0].reshape(-1)[-1] = np.nan
        status = np.array([0, 4, 4, 0, 0], dtype=np.int32)           # sticky: the kernel ORs
        got, status = host_law(driver, name, *[lay(x[k], "full") for k in ("K", "u0", "q0", "v0")], x["qpos"], x["qvel"], status=status)
        assert (got[2] == 0.0).all() and status[2] == 4 | fc.NOT_FINITE, (what, got[2], status)
        keep = [0, 1, 3, 4]
        assert np.array_equal(got[keep], good[keep]) and np.array_equal(status[keep], gstat[keep] | np.array([0, 4, 0, 0])), what


def test_saturation_clip_and_mask(driver):
    name = "humanoid"
    table, nq, nv, nu = fc.shape(name)
    limited, ctrlrange = fc.limits(nu)
    K, u0, q0, v0, qpos, qvel = fc.problem(table, nq, nv, nu, B, 1, seed=3)
    K[1, 0] = np.abs(K[1, 0]) * 1e3
    qvel[1] = np.abs(qvel[1]) + 10.0
    v0[1] = 0.0                                                     # the velocity half of dx is large and positive: u = u0 - K dx far below lo
    arrs = [lay(x, "full") for x in (K, u0, q0, v0)]
    got, status = host_law(driver, name, *arrs, qpos, qvel)
    lim = limited != 0
    assert np.array_equal(got[1][lim], ctrlrange[lim, 0]) and status[1] == fc.CLIPPED
    free, fstat = host_law(driver, name, *arrs, qpos, qvel, clip=0)
    assert (free[1][lim] < ctrlrange[lim, 0]).all() and (fstat == 0).all()
    assert np.array_equal(free[:, ~lim], got[:, ~lim])             # actuators without a range are never clipped
    want = fc.restate(table, nv, K[1, 0], u0[1, 0], q0[1, 0], v0[1, 0], qpos[1], qvel[1], -1, 0, limited, ctrlrange, np.longdouble)
    assert want[1] == 0 and fc.figure(free[1], want[0], want[2]) <= 8 * fc.FLOOR
    # a masked environment keeps its sentinel in ctrl, status and the record row; the others are bitwise what they were
    mask = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    ctrl, st, rec = np.full((B, nu), -3.0), np.full(B, 64, dtype=np.int32), np.full((B, 2, nu), -5.0)
    host_law(driver, name, *arrs, qpos, qvel, mask=mask, ctrl=ctrl, status=st, rec=rec, t=0)
    on = mask != 0
    assert (ctrl[~on] == -3.0).all() and (st[~on] == 64).all() and (rec[~on] == -5.0).all()
    assert np.array_equal(ctrl[on], got[on]) and np.array_equal(st[on], status[on] | 64)
    assert np.array_equal(rec[on, 0], got[on]) and (rec[:, 1] == -5.0).all()


@pytest.mark.parametrize("ddtype", [np.float64, np.float32], ids=["data64", "data32"])
@pytest.mark.parametrize("name", list(fc.SHAPES))
def test_an_environment_gives_the_same_bits_at_any_position(driver, name, ddtype):
    """Environment 0 of a batch of 1 is bitwise environment 3 of a batch of 5."""
    table, nq, nv, nu = fc.shape(name)
    K, u0, q0, v0, qpos, qvel = fc.problem(table, nq, nv, nu, B, 1, seed=4)
    five, _ = host_law(driver, name, *[lay(x, "full") for x in (K, u0, q0, v0)], qpos, qvel, data_dtype=ddtype)
    one, _ = host_law(driver, name, *[lay(x[3:4], "full") for x in (K, u0, q0, v0)], qpos[3:4], qvel[3:4], data_dtype=ddtype)
    assert np.array_equal(one[0], five[3]) and np.isfinite(one).all()


# ---- 4. the checker -------------------------------------------------------------------------------------------------------------------
def test_argument_checker_rejects_each_bad_argument(driver):
    def args(**kw):
        a = FeedbackLawArgs(B=5, nq=28, nv=27, nu=21, njnt=22, data_f32=0, clip=1, t=0, sign=-1.0)
        for key in ("K", "u0", "q0"):
            setattr(a, key, FbIn(0x1000, 0, 0, 0))
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    err = lambda nstep=1, **kw: driver.fbh_arg_error(ctypes.byref(args(**kw)), nstep)
    assert err() == 0 and err(nstep=100, t=5, sign=1.0) == 0 and err(nv=64, nq=66, nu=32, njnt=54) == 0
    assert err(B=0) == 1
    assert err(nv=0) == 2 and err(nv=65, nq=65) == 2
    assert err(nu=0) == 3 and err(nu=33) == 3
    assert err(nq=26) == 4 and err(nq=55) == 4 and err(njnt=0) == 4 and err(njnt=28) == 4
    assert err(sign=0.0) == 5 and err(sign=2.0) == 5 and err(sign=float("nan")) == 5 and err(sign=-0.5) == 5
    assert err(t=-1) == 6
    assert err(nstep=0) == 7 and err(nstep=-3) == 7 and err(nstep=1 << 30, t=1) == 7
    for key in ("K", "u0", "q0", "v0"):
        assert err(**{key: FbIn(0x1000, -1, 0, 0)}) == 8 and err(**{key: FbIn(0x1000, 0, -8, 0)}) == 8, key
    assert err(ur_ss=-1) == 8 and err(ur_es=-1) == 8
    for key in ("K", "u0", "q0"):
        assert err(**{key: FbIn(None, 0, 0, 0)}) == 9, key
    assert err(v0=FbIn(None, 0, 0, 0)) == 0                          # v0 is optional
    # the emulated launch refuses what the checker refuses, before any thread runs
    table, nq, nv, nu = fc.shape("drone")
    K, u0, q0, v0, qpos, qvel = fc.problem(table, nq, nv, nu, 2, 1)
    ctrl, _ = host_law(driver, "drone", *[lay(x, "full") for x in (K, u0, q0, v0)], qpos, qvel, sign=0, expect=5)
    assert (ctrl == -7.0).all()
    # LDS: four wavefronts per workgroup where they fit 64 KiB, every wave's slice a whole number of 16-byte units
    assert driver.fbh_waves(1, 2) == 4 and driver.fbh_waves(21, 27) == 4 and driver.fbh_waves(32, 64) == 1
    for nu_, nv_ in ((1, 1), (1, 2), (4, 6), (21, 27), (31, 33), (32, 64)):
        n = driver.fbh_lds_doubles(nu_, nv_)
        assert n % 2 == 0 and n >= 2 * nv_ + nu_ * ((2 * nv_) | 1) + 32 and n * 8 * driver.fbh_waves(nu_, nv_) <= 64 * 1024


# ---- 5. cross-compilation ---------------------------------------------------------------------------------------------------------------
def test_translation_unit_cross_compiles_for_gfx950(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is required: the kernels are HIP for gfx950")
    src = os.path.join(ROOT, "mujoco_template_amd", "csrc", "mjb_feedback.hip")
    asm = str(tmp_path / "mjb_feedback.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm, src])
    text = open(asm).read()
    assert "k_feedback_law" in text and "global_load_dwordx4" in text and "v_mul_f64" in text
    assert ".vgpr_spill_count: 0" in text and ".private_segment_fixed_size: 0" in text      # no scratch memory
    assert "s_barrier" not in text                                  # one wavefront owns an environment: no workgroup barrier


def test_library_exports_the_entry_points():
    so = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    lib = ctypes.CDLL(so)
    assert hasattr(lib, "mjb_feedback_law") and hasattr(lib, "mjb_rollout_feedback")
    import mujoco_template_amd as mt

    assert callable(mt.feedback_ctrl) and callable(mt.rollout_feedback) and mt.DeviceFeedbackController.device_arrays is True
    assert mt.FeedbackRollout._fields == ("state", "sensordata", "control", "status")
