"""The DARE kernel (``mjb_lqr_dare``) without a GPU.

  1. the kernel source itself (``mjb_dare.hpp``) compiled for the host (``tests/dare_host.cpp``, g++ -DMJB_HOST_EMU: one thread per lane,
     the f64 MFMA emulated in its hardware fragment layout) on every case of ``tests/dare_common.py`` against the numpy restatement
     (long double = truth, float64 = the measure of the bound), and on the humanoid balance design also against scipy's
     ``solve_discrete_are``;
  2. the statuses: a failed problem is reported through memory, written as zeros, and leaves its neighbours bitwise untouched;
  3. the LDS layout and the packed G / H accessors;
  4. the translation unit cross-compiles for gfx950 with ``v_mfma_f64_16x16x4`` in its disassembly, and the library exports the entry point.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import dare_common as dc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Strided(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("ss", ctypes.c_long), ("es", ctypes.c_long)]


class DareArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "nx", "nu", "max_iter")] + [("tol", ctypes.c_double)] + \
               [(n, Strided) for n in ("A", "Bm", "Q", "R")] + [(n, ctypes.c_void_p) for n in ("X", "K", "change", "iters", "status")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dare") / "libdare_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "dare_host.cpp")])
    lib = ctypes.CDLL(so)
    cl, ci = ctypes.c_long, ctypes.c_int
    lib.dareh_size_error.argtypes = [cl] * 4 + [ctypes.c_double]
    lib.dareh_lds_bytes.argtypes = [ci, ci]
    lib.dareh_lds_bytes.restype = cl
    return lib


def host_dare(lib, case, tol=dc.TOL, max_iter=dc.MAX_ITER):
    """The emulated kernel on a case dict (dense [n, ...] inputs); the outputs start as NaN / -7 so that anything not written shows."""
    A, B, Q, R = (np.ascontiguousarray(case[k], dtype=np.float64) for k in "ABQR")
    n, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    out = {"X": np.full((n, nx, nx), np.nan), "K": np.full((n, nu, nx), np.nan), "change": np.full(n, np.nan),
           "iters": np.full(n, -7, dtype=np.int32), "status": np.full(n, -7, dtype=np.int32)}
    a = DareArgs(B=n, nx=nx, nu=nu, max_iter=max_iter, tol=tol)
    a.A, a.Bm = Strided(A.ctypes.data, 0, nx * nx), Strided(B.ctypes.data, 0, nx * nu)
    a.Q, a.R = Strided(Q.ctypes.data, 0, nx * nx), Strided(R.ctypes.data, 0, nu * nu)
    for k, v in out.items():
        setattr(a, k, v.ctypes.data)
    assert lib.dareh_solve(ctypes.byref(a)) == 0
    return out


# ---- 1. the kernel source on host threads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_doubling_matches_the_restatement(driver, name, make):
    """X and K against the long-double restatement within 8 x the float64 restatement's own error (floor 1e-13), the Riccati residual
    likewise, iters within 1 of the restatement's, X bitwise symmetric, at the default max_iter = 32 (12-14 iterations are needed).
    One problem per launch where four waves of host threads run (nx > 16), two otherwise."""
    case = make(1 if case_nx(make) > 16 else 2)
    dc.judge(case, host_dare(driver, case), f"dare/host/{name}")


def case_nx(make):
    return make(1)["A"].shape[1]


def test_humanoid_design_matches_the_restatement_and_scipy(driver):
    """The tutorial's humanoid balance design (54 x 21, marginal closed-loop modes, 19 iterations): the comparison above, then against
    scipy.linalg.solve_discrete_are within 8 x the float64 restatement's error against scipy (floor 1e-11), and the closed-loop spectral
    radius of the kernel's K within 1e-6 of that of scipy's K."""
    from scipy.linalg import solve_discrete_are

    case = dc.humanoid_case()
    got = host_dare(driver, case)
    _, f64 = dc.judge(case, got, "dare/host/humanoid")
    A, B, Q, R = (case[k][0] for k in "ABQR")
    P = solve_discrete_are(A, B, Q, R)
    Ks = np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)
    for key, ref in (("X", P), ("K", Ks)):
        mine, np64 = dc.rel_err(got[key][0], ref), dc.rel_err(f64[0][key], ref)
        print(f"humanoid {key} vs scipy: kernel {mine:.2e}  float64 numpy {np64:.2e}")
        assert mine <= dc.bound(np64, dc.FLOOR_DARE), (key, mine, np64)
    rho = lambda K: np.abs(np.linalg.eigvals(A - B @ K)).max()
    assert abs(rho(got["K"][0]) - rho(Ks)) < 1e-6


# ---- 2. statuses ----------------------------------------------------------------------------------------------------------------------
def test_failures_are_reported_not_propagated(driver):
    dc.check_statuses(lambda case, max_iter: host_dare(driver, case, max_iter=max_iter), "host")


def test_results_do_not_depend_on_the_batch_position(driver):
    """(16, 9), the <1, 32> variant: five systems in one launch against each system launched alone, every output bit for bit.  The
    emulation runs the systems one after the other in the SAME LDS buffer, so a read of LDS that the system itself has not written
    would show here."""
    case = dc.generator_case(16, 9, 5)
    got = host_dare(driver, case)
    assert got["status"].tolist() == [0] * 5
    for e in range(5):
        alone = host_dare(driver, {k: v[e:e + 1] for k, v in case.items()})
        for key in ("X", "K", "change", "iters", "status"):
            assert np.array_equal(got[key][e:e + 1], alone[key]), (e, key)


# ---- 3. layout --------------------------------------------------------------------------------------------------------------------------
def test_size_limits_and_lds_layout(driver):
    ok = driver.dareh_size_error
    assert ok(1, 64, 32, 64, 0.0) == 0 and ok(4096, 4, 1, 1, 1e-12) == 0
    assert ok(0, 4, 1, 32, 1e-12) == 1 and ok(1, 65, 1, 32, 1e-12) == 2 and ok(1, 0, 1, 32, 1e-12) == 2 and ok(1, 4, 33, 32, 1e-12) == 3
    assert ok(1, 4, 0, 32, 1e-12) == 3 and ok(1, 4, 1, 0, 1e-12) == 4 and ok(1, 4, 1, 65, 1e-12) == 4
    assert ok(1, 4, 1, 32, -1e-12) == 5 and ok(1, 4, 1, 32, float("nan")) == 5
    sizes = [(nx, nu) for nx in (1, 2, 4, 7, 16, 17, 54, 64) for nu in (1, 3, 8, 9, 21, 32)]
    for nx, nu in sizes + [s for s in dc.EDGE_SIZES if s not in sizes]:
        assert driver.dareh_packed_roundtrip(nx) == 1, nx
        assert ok(1, nx, nu, 32, 1e-12) == 0, (nx, nu)
        assert driver.dareh_layout_ok(nx, nu) == 1, (nx, nu)
        assert driver.dareh_lds_bytes(nx, nu) <= 160 * 1024, (nx, nu)
    assert driver.dareh_lds_bytes(4, 1) < 2048                  # the cart-pole: many workgroups per compute unit


# ---- 4. cross-compilation ---------------------------------------------------------------------------------------------------------------
def test_translation_unit_cross_compiles_with_the_f64_mfma(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is required: the kernels are HIP for gfx950")
    src = os.path.join(ROOT, "mujoco_template_amd", "csrc", "mjb_dare.hip")
    asm = str(tmp_path / "mjb_dare.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm, src])
    text = open(asm).read()
    assert "v_mfma_f64_16x16x4" in text
    assert "k_lqr_dare" in text


def test_library_exports_the_entry_point():
    so = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    lib = ctypes.CDLL(so)
    assert hasattr(lib, "mjb_lqr_dare")
    import mujoco_template_amd as mt

    assert callable(mt.solve_dare) and mt.DareResult._fields == ("X", "K", "status", "iters", "change")
