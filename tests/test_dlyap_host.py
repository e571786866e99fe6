"""The Lyapunov kernel (``mjb_lqr_dlyap``) without a GPU.

  1. the kernel source itself (``mjb_dlyap.hpp``) compiled for the host (``tests/dlyap_host.cpp``, g++ -DMJB_HOST_EMU: one thread per
     lane, the f64 MFMA emulated in its hardware fragment layout) on every case of ``tests/dlyap_common.py`` against the numpy
     restatement (long double = truth, float64 = the measure of the bound), on the humanoid balance design against the long-double
     DARE solution and scipy, and in the Gramian form against the restatement and scipy's ``solve_discrete_lyapunov``;
  2. the optional arguments: ``M = A`` alone, no ``R``, the sign;
  3. the statuses: a failed problem is reported through memory, written as NaN and +inf, and leaves its neighbours bitwise untouched;
  4. the size limits and the LDS layout;
  5. the translation unit cross-compiles for gfx950 with ``v_mfma_f64_16x16x4`` in its disassembly, and the library exports the entry point.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import dare_common as dc
from tests import dlyap_common as lc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Strided(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("ss", ctypes.c_long), ("es", ctypes.c_long)]


class DlyapArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "nx", "nu", "transpose", "max_iter")] + [("sign", ctypes.c_double), ("tol", ctypes.c_double)] + \
               [(n, Strided) for n in ("A", "Bm", "K", "Q", "R", "x0")] + [(n, ctypes.c_void_p) for n in ("P", "J", "change", "iters", "status")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dlyap") / "libdlyap_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "dlyap_host.cpp")])
    lib = ctypes.CDLL(so)
    cl, ci = ctypes.c_long, ctypes.c_int
    lib.dlyaph_size_error.argtypes = [cl, cl, cl, ci, cl, ctypes.c_double, cl]
    lib.dlyaph_lds_bytes.argtypes = [ci, ci]
    lib.dlyaph_lds_bytes.restype = cl
    return lib


def host_dlyap(lib, case, tol=lc.TOL, max_iter=lc.MAX_ITER, feedback_sign=-1, transpose=False):
    """The emulated kernel on a case dict (dense [n, ...] inputs; B, K, R, x0 may be absent); the outputs start as -7 so that anything
    not written shows."""
    arr = {k: np.ascontiguousarray(case[k], dtype=np.float64) for k in ("A", "B", "K", "Q", "R", "x0") if case.get(k) is not None}
    n, nx = arr["A"].shape[0], arr["A"].shape[1]
    nu = arr["K"].shape[1] if "K" in arr else 0
    out = {"P": np.full((n, nx, nx), -7.0), "change": np.full(n, -7.0), "iters": np.full(n, -7, dtype=np.int32),
           "status": np.full(n, -7, dtype=np.int32)}
    if "x0" in arr:
        out["J"] = np.full(n, -7.0)
    a = DlyapArgs(B=n, nx=nx, nu=nu, transpose=int(transpose), max_iter=max_iter, sign=float(feedback_sign), tol=tol)
    for field, key in (("A", "A"), ("Bm", "B"), ("K", "K"), ("Q", "Q"), ("R", "R"), ("x0", "x0")):
        if key in arr:
            setattr(a, field, Strided(arr[key].ctypes.data, 0, arr[key][0].size))
    for k, v in out.items():
        setattr(a, k, v.ctypes.data)
    assert lib.dlyaph_solve(ctypes.byref(a)) == 0
    out.setdefault("J", None)
    return out


def case_nx(make):
    return make(1)["A"].shape[1]


# ---- 1. the kernel source on host threads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make", lc.CASES, ids=[c[0] for c in lc.CASES])
def test_smith_iteration_matches_the_restatement(driver, name, make):
    """P against the long-double restatement within 8 x the float64 restatement's own error (floor 1e-13), the Lyapunov residual
    likewise, iters within 1 of the restatement's (10-14), P bitwise symmetric, J within the bound of x0' P x0 in long double.
    One problem per launch where four waves of host threads run (nx > 16), two otherwise."""
    case = lc.gain_case(name, make, 1 if case_nx(make) > 16 else 2)
    lc.judge(case, host_dlyap(driver, case), f"dlyap/host/{name}")


def test_humanoid_policy_evaluation_is_the_dare_solution(driver):
    """The humanoid balance design (54 x 21) with its optimal gain: two closed-loop modes of modulus 1 that S does not see.  The first
    change <= 1e-12 is at iteration 19 (5e-18); from there change doubles and passes 1e-12 again at 37, so a rule that did not stop at
    the first crossing would return a drifted P.  Truth: the long-double DARE solution (2.8e-14 from the float64 restatement); scipy's
    own solve_discrete_lyapunov is 1e-10 from it, hence the floor 1e-11 against scipy."""
    from scipy.linalg import solve_discrete_lyapunov

    case = lc.humanoid_case()
    got = host_dlyap(driver, case)
    f64 = lc.judge(case, got, "dlyap/host/humanoid", truth_P=case["X"])
    assert int(got["iters"][0]) == f64[0]["iters"] == 19
    M, S = lc.closed_loop(case["A"][0], case["B"][0], case["K"][0], case["Q"][0], case["R"][0], np.float64)
    Ps = solve_discrete_lyapunov(M.T, S)
    mine, np64 = lc.rel_err(got["P"][0], Ps), lc.rel_err(f64[0]["P"], Ps)
    print(f"humanoid P vs scipy: kernel {mine:.2e}  float64 numpy {np64:.2e}")
    assert mine <= lc.bound(np64, lc.FLOOR_DARE), (mine, np64)


@pytest.mark.parametrize("nx,nu", [(12, 4), (17, 5), (16, 9), (3, 9)])
def test_gramian_form_matches_the_restatement_and_scipy(driver, nx, nu):
    """transpose: P = M P M' + S (12-14 iterations), against the restatement and scipy.linalg.solve_discrete_lyapunov(M, S)."""
    from scipy.linalg import solve_discrete_lyapunov

    case = lc.gain_case(f"gen{nx}x{nu}", lambda n: dc.generator_case(nx, nu, n), 1 if nx > 16 else 2)
    got = host_dlyap(driver, case, transpose=True)
    f64 = lc.judge(case, got, f"dlyap/host/gramian{nx}x{nu}", transpose=True)
    plain = host_dlyap(driver, case)
    assert not np.array_equal(plain["P"], got["P"])
    for e in range(case["A"].shape[0]):
        M, S = lc.closed_loop(case["A"][e], case["B"][e], case["K"][e], case["Q"][e], case["R"][e], np.float64)
        Ps = solve_discrete_lyapunov(M, S)
        mine, np64 = lc.rel_err(got["P"][e], Ps), lc.rel_err(f64[e]["P"], Ps)
        print(f"gramian {nx}x{nu} [{e}] vs scipy: kernel {mine:.2e}  float64 numpy {np64:.2e}")
        assert mine <= lc.bound(np64, lc.FLOOR_DARE), (mine, np64)


# ---- 2. the optional arguments ----------------------------------------------------------------------------------------------------------
def test_open_loop_and_missing_cost_term(driver):
    """M = A alone (no B, K, R: a stable A, 0.9 x a generator system's) and R absent (S = sym(Q) with the closed loop of K)."""
    case = lc.gain_case("gen7x3", lambda n: dc.generator_case(7, 3, n), 2)
    alone = {"A": 0.9 * case["A"], "Q": case["Q"], "x0": case["x0"]}
    lc.judge(alone, host_dlyap(driver, alone), "dlyap/host/open_loop")
    no_r = {k: v for k, v in case.items() if k != "R"}
    got = host_dlyap(driver, no_r)
    lc.judge(no_r, got, "dlyap/host/no_R")
    assert not np.array_equal(got["P"], host_dlyap(driver, case)["P"])


def test_the_sign_is_applied_to_the_gain_exactly(driver):
    """feedback_sign=+1 with -K is bitwise feedback_sign=-1 with K; +1 with K itself is another closed loop."""
    case = lc.gain_case("gen7x3", lambda n: dc.generator_case(7, 3, n), 2)
    minus = host_dlyap(driver, case)
    plus = host_dlyap(driver, {**case, "K": -case["K"]}, feedback_sign=+1)
    for key in ("P", "J", "change", "iters", "status"):
        assert np.array_equal(minus[key], plus[key]), key
    lc.judge({**case, "K": -case["K"]}, plus, "dlyap/host/sign_plus", feedback_sign=+1)
    wrong = host_dlyap(driver, case, feedback_sign=+1)
    assert not np.array_equal(wrong["P"], minus["P"], equal_nan=True)


# ---- 3. statuses ----------------------------------------------------------------------------------------------------------------------
def test_failures_are_reported_not_propagated(driver):
    lc.check_statuses(lambda case, max_iter: host_dlyap(driver, case, max_iter=max_iter), "host")


def test_results_do_not_depend_on_the_batch_position(driver):
    """(16, 9), the largest one-wave state: five systems in one launch against each system launched alone, every output bit for bit
    (the emulation runs them one after the other in the SAME LDS buffer)."""
    case = lc.gain_case("gen16x9", lambda n: dc.generator_case(16, 9, n), 5)
    got = host_dlyap(driver, case)
    assert got["status"].tolist() == [0] * 5
    for e in range(5):
        alone = host_dlyap(driver, {k: v[e:e + 1] for k, v in case.items()})
        for key in ("P", "J", "change", "iters", "status"):
            assert np.array_equal(got[key][e:e + 1], alone[key]), (e, key)


def test_near_marginal_system_converges(driver):
    """M = [[1 - 1e-9, 1], [0, 0.5]], Q = I: rho = 1 - 1e-9 converges, at iteration 35."""
    case = {"A": np.array([[[1.0 - 1e-9, 1.0], [0.0, 0.5]]]), "Q": np.eye(2)[None]}
    got = host_dlyap(driver, case)
    ref = lc.restate(case["A"][0], None, None, case["Q"][0], None, np.float64)
    assert ref["status"] == 0 and ref["iters"] == 35
    assert got["status"].tolist() == [0] and abs(int(got["iters"][0]) - 35) <= 1
    assert lc.rel_err(got["P"][0], lc.truth(case["A"][0], None, None, case["Q"][0], None)["P"]) <= lc.bound(
        lc.rel_err(ref["P"], lc.truth(case["A"][0], None, None, case["Q"][0], None)["P"]))


# ---- 4. layout --------------------------------------------------------------------------------------------------------------------------
def test_size_limits_and_lds_layout(driver):
    ok = driver.dlyaph_size_error
    assert ok(1, 64, 32, 1, 64, 0.0, -1) == 0 and ok(4096, 4, 1, 1, 1, 1e-12, 1) == 0 and ok(1, 4, 0, 0, 64, 1e-12, -1) == 0
    assert ok(0, 4, 1, 1, 64, 1e-12, -1) == 1 and ok(1, 65, 1, 1, 64, 1e-12, -1) == 2 and ok(1, 0, 1, 1, 64, 1e-12, -1) == 2
    assert ok(1, 4, 33, 1, 64, 1e-12, -1) == 3 and ok(1, 4, 0, 1, 64, 1e-12, -1) == 3
    assert ok(1, 4, 1, 1, 0, 1e-12, -1) == 4 and ok(1, 4, 1, 1, 65, 1e-12, -1) == 4
    assert ok(1, 4, 1, 1, 64, -1e-12, -1) == 5 and ok(1, 4, 1, 1, 64, float("nan"), -1) == 5
    assert ok(1, 4, 1, 1, 64, 1e-12, 0) == 6 and ok(1, 4, 1, 1, 64, 1e-12, 2) == 6
    assert ok(1 << 30, 64, 1, 1, 64, 1e-12, -1) == 7
    sizes = [(nx, nu) for nx in (1, 2, 4, 7, 16, 17, 54, 64) for nu in (0, 1, 3, 8, 9, 21, 32)]
    for nx, nu in sizes + [s for s in dc.EDGE_SIZES if s not in sizes]:
        assert ok(1, nx, nu, int(nu > 0), 64, 1e-12, -1) == 0, (nx, nu)
        assert driver.dlyaph_layout_ok(nx, nu) == 1, (nx, nu)
        assert driver.dlyaph_lds_bytes(nx, nu) <= 160 * 1024, (nx, nu)
    assert driver.dlyaph_lds_bytes(4, 1) < 2048                  # the cart-pole: many workgroups per compute unit


# ---- 5. cross-compilation ---------------------------------------------------------------------------------------------------------------
def test_translation_unit_cross_compiles_with_the_f64_mfma(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is required: the kernels are HIP for gfx950")
    src = os.path.join(ROOT, "mujoco_template_amd", "csrc", "mjb_dlyap.hip")
    asm = str(tmp_path / "mjb_dlyap.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm, src])
    text = open(asm).read()
    assert "v_mfma_f64_16x16x4" in text
    assert "k_lqr_dlyap" in text


def test_library_exports_the_entry_point():
    so = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    lib = ctypes.CDLL(so)
    assert hasattr(lib, "mjb_lqr_dlyap")
    import mujoco_template_amd as mt

    assert callable(mt.closed_loop_cost) and mt.LyapResult._fields == ("P", "J", "status", "iters", "change")
