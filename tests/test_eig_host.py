"""The eigenvalue kernel (``mjb_lqr_eig``) without a GPU.

  1. the kernel source itself (``mjb_eig.hpp``) compiled for the host (``tests/eig_host.cpp``, g++ -DMJB_HOST_EMU: one thread per lane,
     the f64 MFMA emulated in its hardware fragment layout) on every case of ``tests/eig_common.py`` against LAPACK
     (``numpy.linalg.eigvals``): the backward error within 8 x LAPACK's own on the same matrix (floor 1e-13), the order, the exact
     conjugate pairs, the power-of-two scaling, rho;
  2. the statuses: a failed problem holds NaN / +inf and leaves its neighbours bitwise untouched;
  3. ``eig_size_error``, the LDS layout and the modulus (``eig_hypot``, correctly rounded);
  4. the translation unit cross-compiles for gfx950 with ``v_mfma_f64_16x16x4`` in its disassembly, the library exports the entry
     point and the package the public call.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import eig_common as ec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Strided(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("ss", ctypes.c_long), ("es", ctypes.c_long)]


class EigArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "nx", "nu", "max_sweeps", "balance")] + [("sign", ctypes.c_double)] + \
               [(n, Strided) for n in ("A", "Bm", "K")] + [(n, ctypes.c_void_p) for n in ("wr", "wi", "scale", "rho", "sweeps", "status")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("eig") / "libeig_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "eig_host.cpp")])
    lib = ctypes.CDLL(so)
    cl, ci, cd = ctypes.c_long, ctypes.c_int, ctypes.c_double
    lib.eigh_size_error.argtypes = [cl, cl, cl, ci, cl, cl]
    lib.eigh_lds_bytes.argtypes = [ci, ci]
    lib.eigh_lds_bytes.restype = cl
    lib.eigh_hypot.argtypes = [cd, cd]
    lib.eigh_hypot.restype = cd
    return lib


def host_solver(lib):
    """The emulated kernel as a solver of eig_common; the outputs start as -7 so that anything not written shows."""
    def solve(A, B=None, K=None, feedback_sign=-1, balance=True, max_sweeps=None):
        A = np.ascontiguousarray(A, dtype=np.float64)
        n, nx = A.shape[0], A.shape[1]
        out = {k: np.full((n, nx), -7.0) for k in ("wr", "wi", "scale")}
        out.update(rho=np.full(n, -7.0), sweeps=np.full(n, -7, dtype=np.int32), status=np.full(n, -7, dtype=np.int32))
        a = EigArgs(B=n, nx=nx, nu=0, max_sweeps=0 if max_sweeps is None else max_sweeps, balance=int(balance), sign=float(feedback_sign))
        a.A = Strided(A.ctypes.data, 0, nx * nx)
        if B is not None:
            B, K = np.ascontiguousarray(B, dtype=np.float64), np.ascontiguousarray(K, dtype=np.float64)
            a.nu = B.shape[2]
            a.Bm, a.K = Strided(B.ctypes.data, 0, nx * a.nu), Strided(K.ctypes.data, 0, nx * a.nu if K.ndim == 3 else 0)
        for k, v in out.items():
            setattr(a, k, v.ctypes.data)
        assert lib.eigh_solve(ctypes.byref(a)) == 0
        return out
    return solve


# ---- 1. the kernel source on host threads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", ec.GAUSS_SIZES)
def test_gaussian_matrices_match_lapack(driver, nx):
    """N(0, 1/n) matrices passed as A alone: 1 and 2 never chase a bulge, 3 is the first that does, 16 / 17 straddle a tile, 64 is the limit."""
    ec.check_gauss(host_solver(driver), nx, "eig/host", n=2)


@pytest.mark.parametrize("kind,nx,nu", ec.LOOP_SIZES, ids=[f"{k}{a}x{b}" for k, a, b in ec.LOOP_SIZES])
def test_closed_loops_match_lapack(driver, kind, nx, nu):
    """A - B K formed by the kernel (f64 MFMA), K per problem and one K shared by all."""
    ec.check_closed_loop(host_solver(driver), kind, nx, nu, "eig/host", n=2)


def test_humanoid_balance_design(driver):
    """54 x 21, two poles on the unit circle, badly scaled: balanced and plain, rho within 1e-6 of numpy's."""
    ec.check_humanoid(host_solver(driver), "eig/host")


def test_normal_matrix_with_a_known_spectrum(driver):
    ec.check_normal(host_solver(driver), "eig/host")


def test_degenerate_inputs_do_not_divide_by_zero(driver):
    ec.check_degenerate(host_solver(driver), "eig/host")


def test_feedback_sign_is_an_exact_negation(driver):
    ec.check_sign(host_solver(driver), "host")


# ---- 2. statuses ----------------------------------------------------------------------------------------------------------------------
def test_failures_are_reported_not_propagated(driver):
    ec.check_statuses(host_solver(driver), "host")


# ---- 3. sizes, layout, modulus ----------------------------------------------------------------------------------------------------------
def test_size_limits_and_lds_layout(driver):
    ok = driver.eigh_size_error
    assert ok(1, 64, 32, 1, 0, -1) == 0 and ok(4096, 4, 1, 1, 1, 1) == 0 and ok(1, 4, 0, 0, 300, -1) == 0 and ok(1, 64, 99, 0, 1920, 1) == 0
    assert ok(0, 4, 1, 1, 0, -1) == 1 and ok(1, 65, 1, 1, 0, -1) == 2 and ok(1, 0, 1, 1, 0, -1) == 2
    assert ok(1, 4, 33, 1, 0, -1) == 3 and ok(1, 4, 0, 1, 0, -1) == 3
    assert ok(1, 4, 1, 1, -1, -1) == 4 and ok(1, 4, 1, 1, 301, -1) == 4 and ok(1, 64, 1, 1, 1921, -1) == 4
    assert ok(1, 4, 1, 1, 0, 0) == 5 and ok(1, 4, 1, 1, 0, 2) == 5
    assert ok(1 << 30, 64, 1, 1, 0, -1) == 6
    assert driver.eigh_default_sweeps(4) == 300 and driver.eigh_default_sweeps(64) == 1920
    for nx in (1, 2, 4, 7, 16, 17, 54, 64):
        for nu in (0, 1, 3, 8, 9, 21, 32):
            assert driver.eigh_layout_ok(nx, nu) == 1, (nx, nu)
            assert driver.eigh_lds_bytes(nx, nu) <= 64 * 1024, (nx, nu)
    assert driver.eigh_lds_bytes(4, 1) < 2048                   # the cart-pole: many workgroups per compute unit


def test_modulus_is_correctly_rounded(driver):
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.normal(size=(2000, 2)), rng.normal(size=(500, 2)) * 10.0 ** rng.uniform(-12, 12, size=(500, 2)),
                         [[0.0, 0.0], [0.0, -2.5], [3.0, 4.0], [1e300, 1e300], [1e-300, 1e-300], [1.0, 1e-200]]])
    for x, y in xs:
        assert driver.eigh_hypot(x, y) == ec.exact_hypot(x, y), (x, y)


# ---- 4. cross-compilation and exports -----------------------------------------------------------------------------------------------------
def test_translation_unit_cross_compiles_with_the_f64_mfma(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is required: the kernels are HIP for gfx950")
    src = os.path.join(ROOT, "mujoco_template_amd", "csrc", "mjb_eig.hip")
    asm = str(tmp_path / "mjb_eig.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm, src])
    text = open(asm).read()
    assert "v_mfma_f64_16x16x4" in text
    assert "k_lqr_eig" in text


def test_library_exports_the_entry_point():
    so = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    lib = ctypes.CDLL(so)
    assert hasattr(lib, "mjb_lqr_eig")
    import mujoco_template_amd as mt

    assert callable(mt.closed_loop_poles) and mt.PolesResult._fields == ("wr", "wi", "rho", "status", "sweeps", "scale")
