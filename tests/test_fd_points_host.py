"""Finite differences at points (``mjb_transition_fd_points``) and the warm-start ring column (observation flag 128) without a GPU.

  1. the host arithmetic of the entry point's argument checks and of its slab plan (``mjb_host.hpp``), against brute force;
  2. the ring column through the host-compiled ``env_run`` (``tests/fd_points_host.cpp``, g++ -DMJB_HOST_EMU, one thread per lane):
     bitwise ``qacc_warmstart`` after stepping one step at a time, and the leading columns of the row untouched by the flag;
  3. the generic library and the humanoid's specialised FD translation unit cross-compile for gfx950 with the point table in their
     argument list.
"""

from __future__ import annotations

import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from oracle import mjo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CTRL_KEEP, CTRL_SEQUENCE = 0, 4
RING, RING_WS = 1 | 2 | 8 | 16, 1 | 2 | 8 | 16 | 128


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fd_points") / "libfd_points_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "fd_points_host.cpp")])
    lib = ctypes.CDLL(so)
    vp, ci, cl, cull, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_ulonglong, ctypes.c_longlong
    lib.fdp_run.argtypes = [ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, cl, cl] + [vp] * 9
    lib.fdp_run.restype = ci
    lib.fdp_last_error.restype = ctypes.c_char_p
    lib.fdp_highest_element.argtypes = [cl, cl, cl, cl, cl, ctypes.POINTER(cll)]
    lib.fdp_highest_element.restype = ci
    lib.fdp_extent_inside.argtypes = [cull, cll, cull, cull, cull]
    lib.fdp_extent_inside.restype = ci
    lib.fdp_point_scratch_bytes.argtypes = [ci, ci, ci]
    lib.fdp_point_scratch_bytes.restype = cull
    lib.fdp_slab_points.argtypes = [cull, cull]
    lib.fdp_slab_points.restype = cl
    lib.fdp_slab_count.argtypes = [cl, cl]
    lib.fdp_slab_count.restype = cl
    lib.fdp_slab.argtypes = [cl, cl, cl, ctypes.POINTER(cl), ctypes.POINTER(cl)]
    lib.fdp_slab.restype = ci
    lib.fdp_chunk_rule.argtypes = [cl, ci, cl]
    lib.fdp_chunk_rule.restype = ci
    return lib


# ---- 1. stride / bounds arithmetic and the slab plan ---------------------------------------------------------------------------------
def _hi(lib, T, B, n, ss, es):
    out = ctypes.c_longlong(-7)
    rc = lib.fdp_highest_element(T, B, n, ss, es, ctypes.byref(out))
    return rc, int(out.value)


def _brute(T, B, n, ss, es):
    return max((t * ss + e * es + i for t in range(T) for e in range(B) for i in range(n)), default=-1)


def test_highest_element_matches_enumeration(driver):
    """Dense [T, B, n], a column of a [T, B, dim] ring, a [B, T, n] tensor read as (t, e), and broadcast strides (0)."""
    T, B, n, dim, off = 5, 3, 4, 11, 6
    layouts = {
        "dense": (B * n, n),
        "ring column": (B * dim, dim),                          # base pointer = ring + off: the extent is relative to it
        "[B, T, n]": (n, T * n),
        "broadcast over steps": (0, n),
        "broadcast over environments": (n, 0),
        "broadcast over both": (0, 0),
    }
    for what, (ss, es) in layouts.items():
        rc, hi = _hi(driver, T, B, n, ss, es)
        assert rc == 0 and hi == _brute(T, B, n, ss, es), what
    assert off + _hi(driver, T, B, n, B * dim, dim)[1] <= T * B * dim - 1                # the ring column stays inside the ring
    rng = np.random.default_rng(0)
    for _ in range(200):
        T, B, n = (int(x) for x in rng.integers(1, 6, 3))
        ss, es = (int(x) for x in rng.integers(0, 40, 2))
        assert _hi(driver, T, B, n, ss, es) == (0, _brute(T, B, n, ss, es))
    assert _hi(driver, 4, 3, 0, 7, 9) == (0, -1)                # zero width: nothing is touched
    for bad in ((0, 3, 2, 1, 1), (3, 0, 2, 1, 1), (3, 3, 2, -1, 1), (3, 3, 2, 1, -1), (3, 3, -1, 1, 1)):
        assert _hi(driver, *bad)[0] == 1, bad
    big = (1 << 62) - 1                                         # no overflow in 128-bit arithmetic: reported as beyond 63 bits
    assert _hi(driver, 1 << 20, 1 << 20, 8, big, big)[0] == 2


def test_extent_check(driver):
    base, size = 0x7000_0000_0000, 4096
    inside = driver.fdp_extent_inside
    assert inside(base, 511, 8, base, size) == 1               # last element ends exactly at the end of the allocation
    assert inside(base, 512, 8, base, size) == 0               # one element short
    assert inside(base + 8, 511, 8, base, size) == 0           # an interior pointer shifts the extent
    assert inside(base + 8, 510, 8, base, size) == 1
    assert inside(base - 8, 0, 8, base, size) == 0             # before the allocation
    assert inside(base, 1023, 4, base, size) == 1 and inside(base, 1024, 4, base, size) == 0
    assert inside(base, -1, 8, base, 0) == 1                   # nothing touched
    assert inside(base, (1 << 62), 8, base, size) == 0         # would wrap in 64-bit arithmetic


def test_slab_plan_covers_every_point_once(driver):
    per_point = driver.fdp_point_scratch_bytes(28, 27, 21)     # the humanoid
    assert per_point == (1 + 2 * (2 * 27 + 21)) * (28 + 27) * 8 == 66440
    for npoint, budget in itertools.product((1, 2, 31, 32, 33, 500, 4096), (1, per_point - 1, per_point, 3 * per_point + 5, 10 * per_point, 128 << 20)):
        per = driver.fdp_slab_points(per_point, budget)
        assert per >= 1                                         # a point larger than the budget still runs, alone
        assert per == max(1, budget // per_point)
        nslab = driver.fdp_slab_count(npoint, per)
        seen = np.zeros(npoint, dtype=int)
        for k in range(nslab):
            p0, n = ctypes.c_long(-1), ctypes.c_long(-1)
            assert driver.fdp_slab(npoint, per, k, ctypes.byref(p0), ctypes.byref(n)) == 1
            assert n.value >= 1
            assert n.value * per_point <= budget or n.value == 1
            seen[p0.value:p0.value + n.value] += 1
        assert (seen == 1).all(), (npoint, budget)
        p0, n = ctypes.c_long(-1), ctypes.c_long(-1)
        assert driver.fdp_slab(npoint, per, nslab, ctypes.byref(p0), ctypes.byref(n)) == 0
        assert driver.fdp_slab(npoint, per, -1, ctypes.byref(p0), ctypes.byref(n)) == 0
    assert driver.fdp_slab_count(0, 4) == 0


def test_chunk_rule_is_sized_by_the_points_of_the_launch(driver):
    """Columns per job: one for a single point (latency), growing with the points of the launch up to 8 - whatever the batch is."""
    ncol, slots = 151, 256
    assert driver.fdp_chunk_rule(1, ncol, slots) == 1
    got = [driver.fdp_chunk_rule(p, ncol, slots) for p in (1, 8, 16, 64, 512, 4096)]
    assert got == sorted(got) and got[-1] == 8 and all(1 <= c <= 8 for c in got)
    assert driver.fdp_chunk_rule(512, ncol, slots) == min(8, max(1, 512 * ncol // (4 * slots)))


# ---- 2. the warm-start ring column through env_run ------------------------------------------------------------------------------------
class Batch:
    """float64 state arrays of `batch` environments, advanced in place by the emulated kernel."""

    def __init__(self, lib, cm, batch, G, use_double):
        from mujoco_template_amd._pack import PackedTable

        self.lib, self.cm, self.packed, self.B, self.G, self.use_double = lib, cm, PackedTable(cm), batch, G, use_double
        rng = np.random.default_rng(7)
        od = mjo.OracleData(mjo.OracleModel(cm))
        self.s = {
            "qpos": np.stack([od.integrate_pos(np.asarray(cm.qpos0, dtype=np.float64), rng.normal(size=cm.nv) * 0.05, 1.0) for _ in range(batch)]),
            "qvel": rng.normal(size=(batch, cm.nv)) * 0.2,
            "ctrl": np.zeros((batch, max(cm.nu, 1))), "qacc": np.zeros((batch, cm.nv)), "qacc_warmstart": np.zeros((batch, cm.nv)),
            "time": np.zeros(batch), "counters": np.zeros((batch, 8), dtype=np.int32),
            "sensordata": np.zeros((batch, max(cm.nsensordata, 1))),
        }
        if self.use_double is False:                    # fp32 state: start from fp32-representable values (the device arrays hold fp32)
            for k in ("qpos", "qvel"):
                self.s[k] = self.s[k].astype(np.float32).astype(np.float64)

    def copy(self):
        other = object.__new__(Batch)
        other.__dict__.update(self.__dict__)
        other.s = {k: v.copy() for k, v in self.s.items()}
        return other

    def run(self, flags, nstep, mode, table=None, step_stride=0, env_stride=0):
        cm = self.cm
        dim = cm.nq + cm.nv + cm.nsensordata + 1 + (cm.nv if flags & 128 else 0)
        ring = np.full((nstep, self.B, dim), np.nan)
        p, s = self.packed, self.s
        rc = self.lib.fdp_run(flags, p.n, p.names, p.ptrs, p.dtypes, p.counts, self.G, int(self.use_double), 64, 160, self.B, nstep, mode,
                              None if table is None else table.ctypes.data, step_stride, env_stride,
                              *[s[k].ctypes.data for k in ("qpos", "qvel", "ctrl", "qacc", "qacc_warmstart", "time", "counters", "sensordata")],
                              ring.ctypes.data)
        assert rc == 0, self.lib.fdp_last_error().decode()
        return ring


def _table(cm, B, T, seed=3):
    """[B, T, nu] controls inside the ctrl range, fp32-representable."""
    lo, hi = np.full(cm.nu, -1.0), np.full(cm.nu, 1.0)
    rng_ = np.reshape(np.asarray(cm.arrays["actuator_ctrlrange"], dtype=np.float64), (-1, 2))
    lim = np.asarray(cm.arrays["actuator_ctrllimited"]).astype(bool)
    lo[lim], hi[lim] = rng_[lim, 0], rng_[lim, 1]
    u = np.random.default_rng(seed).uniform(lo, hi, size=(B, T, cm.nu))
    return u.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("use_double", [True, False], ids=["float64", "float32"])
@pytest.mark.parametrize("name,T,G", [("cartpole", 12, 16), ("pendulum", 12, 16), ("humanoid", 4, 64)])
def test_warmstart_column_equals_stepwise_warmstart(driver, compiled, name, T, G, use_double):
    """Flag 128: the column of ring row t equals qacc_warmstart read back after step t of a one-step-at-a-time run, bitwise; the
    leading columns (qpos | qvel | sensordata | time at their existing offsets) are bitwise those of the ring without the flag,
    whose row keeps its width; the final state is the same with and without the flag."""
    cm = compiled(name)
    B, nq, nv, ns = 2, cm.nq, cm.nv, cm.nsensordata
    base = Batch(driver, cm, B, G, use_double)
    tab = np.ascontiguousarray(_table(cm, B, T))
    a, b, c = base.copy(), base.copy(), base.copy()
    ring = a.run(RING, T, CTRL_SEQUENCE, tab, step_stride=cm.nu, env_stride=T * cm.nu)
    ring_ws = b.run(RING_WS, T, CTRL_SEQUENCE, tab, step_stride=cm.nu, env_stride=T * cm.nu)
    assert ring.shape[-1] == nq + nv + ns + 1 and ring_ws.shape[-1] == nq + nv + ns + 1 + nv
    assert np.isfinite(ring).all() and np.isfinite(ring_ws).all()           # every element of both rows was written
    assert np.array_equal(ring_ws[..., :nq + nv + ns + 1], ring)
    for k in a.s:
        assert np.array_equal(a.s[k], b.s[k]), k
    ws = []
    for t in range(T):
        c.s["ctrl"][:, :cm.nu] = tab[:, t]
        row = c.run(RING, 1, CTRL_KEEP)[0]
        assert np.array_equal(row, ring[t])                     # existing layout: qpos | qvel | sensordata | time
        assert np.array_equal(row[:, :nq], c.s["qpos"]) and np.array_equal(row[:, nq:nq + nv], c.s["qvel"])
        assert np.array_equal(row[:, -1], c.s["time"])
        ws.append(c.s["qacc_warmstart"].copy())
    ws = np.stack(ws)
    assert np.array_equal(ring_ws[..., nq + nv + ns + 1:], ws)
    assert np.abs(ws).max() > 0                                 # not a column of zeros
    assert np.array_equal(ring_ws[-1, :, nq + nv + ns + 1:], b.s["qacc_warmstart"])


# ---- 3. cross-compilation ---------------------------------------------------------------------------------------------------------------
def test_point_table_kernels_cross_compile_for_gfx950():
    """The generic library exports the new entry points, and the humanoid's specialised FD translation unit - whose kernel takes the
    point table as its last argument - cross-compiles for gfx950 without a GPU."""
    so = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    from mujoco_template_amd import mjcf
    from mujoco_template_amd._capi import DeviceModel, compile_spec
    from tests.conftest import MODELS

    lib = ctypes.CDLL(so)
    for sym in ("mjb_transition_fd_points", "mjb_fd_points_slabs", "mjb_transition_fd", "mjb_transition_fd_pinned"):
        assert hasattr(lib, sym), sym
    kernels = open(os.path.join(ROOT, "mujoco_template_amd", "csrc", "mjb_kernels.hpp")).read()
    assert "mjb::FdPoints pt)" in kernels.split('void mjb_k_fd_spec(')[1].split("{")[0]
    for dtype in ("float32", "float64"):
        src = DeviceModel(mjcf.compile_xml_path(MODELS["humanoid"])).fd_spec_source(dtype=dtype)
        assert "#define MJB_SPEC_KERNEL 2" in src and "#define MJB_SPEC_BAKED" in src
        blob = open(compile_spec(src), "rb").read()
        assert (blob[:4] == b"\x7fELF" or blob.startswith(b"__CLANG_OFFLOAD_BUNDLE__")) and b"mjb_k_fd_spec" in blob and b"gfx950" in blob
