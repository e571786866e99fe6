"""The sensor Jacobians of the finite-difference path without a GPU:

  1. the slab plan of ``mjb_transition_fd_points_sensors`` counts the sensor block of the per-point scratch (``mjb_host.hpp``), against
     brute force; the three-argument ``fd_point_scratch_bytes`` is what it was;
  2. the library exports and binds the two new entry points;
  3. the specialised FD translation units of drone2 (10 sensor values) and of the humanoid cross-compile for gfx950 for both data
     dtypes, and record the point table's layout revision that ``mjb_kernel_load`` reads.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fd_sensors") / "libfd_sensors_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "fd_sensors_host.cpp")])
    lib = ctypes.CDLL(so)
    ci, cl, cull = ctypes.c_int, ctypes.c_long, ctypes.c_ulonglong
    lib.fds_point_scratch_bytes3.argtypes = [ci, ci, ci]
    lib.fds_point_scratch_bytes3.restype = cull
    lib.fds_point_scratch_bytes.argtypes = [ci, ci, ci, ci]
    lib.fds_point_scratch_bytes.restype = cull
    lib.fds_slab_points.argtypes = [cull, cull]
    lib.fds_slab_points.restype = cl
    lib.fds_slab_count.argtypes = [cl, cl]
    lib.fds_slab_count.restype = cl
    lib.fds_slab.argtypes = [cl, cl, cl, ctypes.POINTER(cl), ctypes.POINTER(cl)]
    lib.fds_slab.restype = ci
    return lib


def test_scratch_of_a_point_counts_the_sensor_block(driver):
    for nq, nv, nu, ns in ((28, 27, 21, 0), (7, 6, 4, 10), (7, 6, 2, 10), (2, 2, 1, 2), (1, 1, 0, 4), (3, 3, 2, 1)):
        ncol = 1 + 2 * (2 * nv + nu)
        plain = sum(8 for _ in range(ncol) for _ in range(nq + nv))             # every column's next state, float64
        sens = sum(8 for _ in range(ncol) for _ in range(ns))                   # every column's sensordata beside it
        assert driver.fds_point_scratch_bytes3(nq, nv, nu) == plain == driver.fds_point_scratch_bytes(nq, nv, nu, 0)
        assert driver.fds_point_scratch_bytes(nq, nv, nu, ns) == plain + sens
        assert driver.fds_point_scratch_bytes(nq, nv, nu, -1) == plain
    assert driver.fds_point_scratch_bytes3(28, 27, 21) == 66440                  # the humanoid: unchanged
    assert driver.fds_point_scratch_bytes(7, 6, 2, 10) == 29 * 23 * 8 == 5336    # the puck of tests/test_gpu_fd_sensors.py


def test_slab_plan_with_a_sensor_block_covers_every_point_once(driver):
    per_point = driver.fds_point_scratch_bytes(7, 6, 4, 10)                      # drone2
    assert per_point > driver.fds_point_scratch_bytes3(7, 6, 4)
    for npoint, budget in itertools.product((1, 2, 6, 31, 33, 4096), (1, per_point - 1, per_point, 2 * per_point + 5, 12000, 128 << 20)):
        per = driver.fds_slab_points(per_point, budget)
        assert per == max(1, budget // per_point)
        nslab = driver.fds_slab_count(npoint, per)
        assert nslab == -(-npoint // per)
        seen = np.zeros(npoint, dtype=int)
        for k in range(nslab):
            p0, n = ctypes.c_long(-1), ctypes.c_long(-1)
            assert driver.fds_slab(npoint, per, k, ctypes.byref(p0), ctypes.byref(n)) == 1
            assert n.value >= 1 and (n.value * per_point <= budget or n.value == 1)     # the sensor block fits the budget with the states
            seen[p0.value:p0.value + n.value] += 1
        assert (seen == 1).all()
        p0, n = ctypes.c_long(-1), ctypes.c_long(-1)
        assert driver.fds_slab(npoint, per, nslab, ctypes.byref(p0), ctypes.byref(n)) == 0
    # asking for the sensors never puts MORE points into a slab
    for budget in (5000, 12000, 1 << 20):
        assert driver.fds_slab_points(driver.fds_point_scratch_bytes(7, 6, 2, 10), budget) <= driver.fds_slab_points(driver.fds_point_scratch_bytes3(7, 6, 2), budget)


def _library():
    so = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    return so


def test_library_exports_and_binds_the_sensor_entry_points():
    lib = ctypes.CDLL(_library())
    from mujoco_template_amd._capi import load_library

    for sym in ("mjb_transition_fd_sensors", "mjb_transition_fd_points_sensors"):
        assert hasattr(lib, sym), sym
        assert getattr(load_library(), sym).argtypes is not None, sym
    assert len(load_library().mjb_transition_fd_points_sensors.argtypes) == len(load_library().mjb_transition_fd_points.argtypes) + 2
    header = open(os.path.join(ROOT, "include", "mjbatch.h")).read()
    assert header.count("linearization.py:28-34") >= 1            # the reference call site the two entry points complete


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", ["drone2", "humanoid"])
def test_fd_translation_units_cross_compile_with_the_sensor_store(name, dtype):
    _library()
    from mujoco_template_amd import mjcf
    from mujoco_template_amd._capi import DeviceModel, compile_spec
    from tests.conftest import MODELS

    src = DeviceModel(mjcf.compile_xml_path(MODELS[name])).fd_spec_source(dtype=dtype)
    assert "#define MJB_SPEC_KERNEL 2" in src and "mjb_spec_fd_points = MJB_FD_POINTS_ABI" in src
    blob = open(compile_spec(src), "rb").read()
    assert (blob[:4] == b"\x7fELF" or blob.startswith(b"__CLANG_OFFLOAD_BUNDLE__")) and b"mjb_k_fd_spec" in blob and b"gfx950" in blob
    assert b"mjb_spec_fd_points" in blob
    kernels = open(os.path.join(ROOT, "mujoco_template_amd", "csrc", "mjb_kernels.hpp")).read()
    assert "pt.sens_out" in kernels.split("void k_fd_body(")[1].split("template <typename T, typename TS, int G>")[0]
