"""The set-point kernel (``mjb_setpoint_ctrl``) without a GPU.

  1. the kernel source itself (``mjb_setpoint.hpp``) compiled for the host (``tests/setpoint_host.cpp``, g++ -DMJB_HOST_EMU: one thread
     per lane) on every case of ``tests/setpoint_common.py`` against the numpy restatement (long double = truth, float64 = the measure
     of the bound);
  2. float32 inputs give bitwise the result of the same values passed as float64; the schedule is the documented one;
  3. the statuses: a failed problem is reported through memory, written as NaN and +inf, and leaves its neighbours bitwise untouched;
  4. the size limits and the LDS layout;
  5. the translation unit cross-compiles for gfx950 with ``k_setpoint`` in it, and the library exports the entry point.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import setpoint_common as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class SetpointArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "nu", "nv", "max_sweeps", "m_f32", "q_f32")] + [("rcond_min", ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ("moment", "qfrc")] + [(n, ctypes.c_long) for n in ("m_es", "q_es")] + \
               [(n, ctypes.c_void_p) for n in ("ctrl", "sv", "rcond", "residual", "pinv", "rank", "sweeps", "status")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("setpoint") / "libsetpoint_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "setpoint_host.cpp")])
    lib = ctypes.CDLL(so)
    cl, ci = ctypes.c_long, ctypes.c_int
    lib.setpointh_size_error.argtypes = [cl, cl, cl, cl, ctypes.c_double]
    lib.setpointh_lds_bytes.argtypes = [ci, ci]
    lib.setpointh_lds_bytes.restype = cl
    lib.setpointh_pair.argtypes = [ci, ci, ci, ctypes.POINTER(ci)]
    return lib


def host_setpoint(lib, moment, qfrc, rcond_min=sc.RCOND_MIN, max_sweeps=0, dtype=np.float64, want_pinv=True):
    """The emulated kernel on dense [n, nu, nv], [n, nv] inputs of ``dtype``; the outputs start as -7 so that anything not written shows."""
    m, q = np.ascontiguousarray(moment, dtype=dtype), np.ascontiguousarray(qfrc, dtype=dtype)
    n, nu, nv = m.shape
    f = lambda *s: np.full(s, -7.0)
    i = lambda: np.full(n, -7, dtype=np.int32)
    out = {"ctrl": f(n, nu), "sv": f(n, min(nu, nv)), "rcond": f(n), "residual": f(n), "rank": i(), "sweeps": i(), "status": i()}
    if want_pinv:
        out["pinv"] = f(n, nv, nu)
    a = SetpointArgs(B=n, nu=nu, nv=nv, max_sweeps=max_sweeps, m_f32=int(dtype == np.float32), q_f32=int(dtype == np.float32),
                     rcond_min=rcond_min, moment=m.ctypes.data, qfrc=q.ctypes.data, m_es=nu * nv, q_es=nv)
    for k, v in out.items():
        setattr(a, k, v.ctypes.data)
    assert lib.setpointh_solve(ctypes.byref(a)) == 0
    out.setdefault("pinv", None)
    return out


# ---- 1. the kernel source on host threads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make,kw,status", sc.CASES, ids=[c[0] for c in sc.CASES])
def test_jacobi_solve_matches_the_restatement(driver, name, make, kw, status):
    """ctrl, sv, pinv and residual against the long-double restatement within 8 x the float64 restatement's own figure (floors: the
    worst such figure over the case list), sweeps within 1, rank equal, rcond = sv_r / sv_1.  Two problems per launch."""
    m, q = sc.problems(name, make, 2)
    f64, _ = sc.judge(f"{name}/2", m, q, host_setpoint(driver, m, q, **kw), f"setpoint/host/{name}", expect=status, **kw)
    if name.startswith("selection"):
        got = host_setpoint(driver, m, q)
        assert got["sweeps"].tolist() == [1, 1]                   # orthogonal rows: the first sweep finds nothing to rotate
        assert np.array_equal(got["residual"], np.abs(q[:, :6]).max(axis=1))   # the root part of qfrc, which no actuator reaches
    # the truth itself against an independent route: LAPACK's minimum-norm least-squares solution (nu > nv included).  A backward-
    # stable float64 solve loses a modest multiple of eps / rcond, so in the measure of ctrl (x rcond) it is a modest multiple of
    # eps: 1e-13 = 450 eps allows for that multiple at 32 x 64 and would not pass a solution that is not the minimum-norm one.
    for e in range(2):
        lstsq = np.linalg.lstsq(m[e].T, q[e], rcond=None)[0]
        assert np.abs(f64[e]["ctrl"] - lstsq).max() / np.abs(lstsq).max() * f64[e]["rcond"] <= 1e-13, (name, e)


def test_without_pinv_nothing_else_changes(driver):
    m, q = sc.problems("gauss4x6", sc.CASES[2][1], 2)
    a, b = host_setpoint(driver, m, q), host_setpoint(driver, m, q, want_pinv=False)
    assert b["pinv"] is None
    for key in sc.OUTPUTS[:-1]:
        assert np.array_equal(a[key], b[key]), key
    for e in range(2):                                            # numpy's pinv, in the measure of pinv and with the allowance stated above
        assert np.abs(a["pinv"][e] - np.linalg.pinv(m[e])).max() / np.abs(a["pinv"][e]).max() * a["rcond"][e] <= 1e-13


# ---- 2. float32 inputs, the schedule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu,nv", [(4, 6), (21, 27), (8, 5)])
def test_float32_inputs_are_widened_exactly(driver, nu, nv):
    m, q = sc.gaussian(nu, nv, 2, seed=11)
    m32, q32 = m.astype(np.float32), q.astype(np.float32)
    narrow, wide = host_setpoint(driver, m32, q32, dtype=np.float32), host_setpoint(driver, m32.astype(np.float64), q32.astype(np.float64))
    for key in sc.OUTPUTS:
        assert np.array_equal(narrow[key], wide[key]), key
    assert narrow["status"].tolist() == [0, 0]


@pytest.mark.parametrize("nu", [1, 2, 3, 4, 7, 21, 31, 32])
def test_schedule_is_the_documented_round_robin(driver, nu):
    """The kernel's pairs are those of ``setpoint_common.schedule``; every pair i < j is met exactly once per sweep, and the pairs of a
    round are disjoint."""
    n2 = nu + (nu & 1)
    rounds = sc.schedule(nu)
    assert len(rounds) == n2 - 1
    seen = []
    for rd in range(n2 - 1):
        mine, out = [], (ctypes.c_int * 2)()
        for k in range(n2 // 2):
            if driver.setpointh_pair(nu, rd, k, out):
                mine.append((out[0], out[1]))
        assert mine == rounds[rd], (nu, rd)
        flat = [x for pr in mine for x in pr]
        assert len(set(flat)) == len(flat)
        seen += mine
    assert sorted(seen) == [(i, j) for i in range(nu) for j in range(i + 1, nu)]


# ---- 3. statuses ----------------------------------------------------------------------------------------------------------------------
def test_failures_are_reported_not_propagated(driver):
    sc.check_statuses(lambda m, q, **kw: host_setpoint(driver, m, q, **kw), "host")


def test_a_zero_guard_accepts_a_singular_matrix(driver):
    """rcond_min = 0: nothing is ill-conditioned; the zero singular value is skipped and ctrl is the minimum-norm solution."""
    m, q = sc.STATUS_CASES[2][1]()                                # the zero row in the middle
    got = host_setpoint(driver, m, q, rcond_min=0.0)
    assert got["status"].tolist() == [0, 0, 0] and got["rcond"][1] == 0.0 and got["ctrl"][1][2] == 0.0
    tr = sc.restate(m[1], q[1], np.longdouble, rcond_min=0.0)
    f64 = sc.restate(m[1], q[1], np.float64, rcond_min=0.0)
    assert tr["status"] == 0 and tr["ctrl"][2] == 0.0
    rc = float(tr["sv"][-2] / tr["sv"][0])                        # the conditioning of what is left: the smallest non-zero singular value
    err = lambda u: float(np.abs(np.asarray(u, dtype=np.longdouble) - tr["ctrl"]).max() / np.abs(tr["ctrl"]).max() * rc)
    assert err(got["ctrl"][1]) <= sc.bound(err(f64["ctrl"]), "ctrl"), (err(got["ctrl"][1]), err(f64["ctrl"]))


# ---- 4. layout --------------------------------------------------------------------------------------------------------------------------
def test_size_limits_and_lds_layout(driver):
    ok = driver.setpointh_size_error
    assert ok(1, 32, 64, 64, 0.0) == 0 and ok(4096, 1, 2, 0, 1e-12) == 0 and ok(1, 1, 1, 1, 1.0) == 0
    assert ok(0, 4, 6, 0, 1e-12) == 1
    assert ok(1, 0, 6, 0, 1e-12) == 2 and ok(1, 33, 6, 0, 1e-12) == 2
    assert ok(1, 4, 0, 0, 1e-12) == 3 and ok(1, 4, 65, 0, 1e-12) == 3
    assert ok(1, 4, 6, -1, 1e-12) == 4 and ok(1, 4, 6, 65, 1e-12) == 4
    assert ok(1, 4, 6, 0, -1e-12) == 5 and ok(1, 4, 6, 0, float("nan")) == 5 and ok(1, 4, 6, 0, float("inf")) == 5
    assert ok(1 << 30, 32, 64, 0, 1e-12) == 6
    for nu in (1, 2, 3, 4, 21, 31, 32):
        for nv in (1, 2, 6, 27, 33, 63, 64):
            assert driver.setpointh_layout_ok(nu, nv) == 1, (nu, nv)
            assert driver.setpointh_lds_bytes(nu, nv) <= 160 * 1024, (nu, nv)
    assert driver.setpointh_lds_bytes(32, 64) <= 64 * 1024         # no raised dynamic-LDS limit is needed
    assert driver.setpointh_lds_bytes(1, 2) < 4096                 # the cart-pole: many workgroups per compute unit


# ---- 5. cross-compilation ---------------------------------------------------------------------------------------------------------------
def test_translation_unit_cross_compiles_for_gfx950(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is required: the kernels are HIP for gfx950")
    src = os.path.join(ROOT, "mujoco_template_amd", "csrc", "mjb_setpoint.hip")
    asm = str(tmp_path / "mjb_setpoint.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm, src])
    text = open(asm).read()
    assert "k_setpoint" in text and "v_fma_f64" in text


def test_library_exports_the_entry_point():
    so = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    lib = ctypes.CDLL(so)
    assert hasattr(lib, "mjb_setpoint_ctrl")
    import mujoco_template_amd as mt

    assert callable(mt.solve_setpoint) and callable(mt.steady_ctrl0_device)
    assert mt.SetpointResult._fields == ("ctrl", "sv", "rcond", "rank", "residual", "status", "sweeps", "pinv")
