"""The LQR kernels (``mjb_lqr_backward`` / ``mjb_lqr_candidates``) without a GPU.

  1. the kernel source itself (``mjb_lqr.hpp``) compiled for the host (``tests/lqr_host.cpp``, g++ -DMJB_HOST_EMU: one thread per lane,
     the f64 MFMA emulated in its hardware fragment layout): the tile product on exact integers, the recursion against the numpy
     restatement (``tests/lqr_common.py``: long double = truth, float64 = the measure of the bound), against scipy's
     ``solve_discrete_are``, an indefinite ``Quu`` reported through ``status``, and the candidate loop;
  2. the stride / extent arithmetic of the argument checks against enumeration, and the LDS layouts;
  3. the translation unit cross-compiles for gfx950 with ``v_mfma_f64_16x16x4`` in its disassembly, and the library exports the
     entry points.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import lqr_common as lc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Strided(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("ss", ctypes.c_long), ("es", ctypes.c_long)]


class BackwardArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("T", "B", "nx", "nu")] + \
               [(n, Strided) for n in ("A", "Bm", "lx", "lu", "lxx", "luu", "lux", "VxT", "VxxT", "mu")] + \
               [(n, ctypes.c_void_p) for n in ("k", "K", "dV", "V0x", "V0xx", "status")]


class CandArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("T", "B", "nx", "nu", "nalpha", "out_f32")] + \
               [(n, Strided) for n in ("A", "Bm", "k", "K", "u", "dx0")] + \
               [(n, ctypes.c_void_p) for n in ("alphas", "lo", "hi", "cand")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lqr") / "liblqr_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "lqr_host.cpp")])
    lib = ctypes.CDLL(so)
    cl, ci = ctypes.c_long, ctypes.c_int
    lib.lqrh_highest_element.argtypes = [cl] * 5 + [ctypes.POINTER(ctypes.c_longlong)]
    lib.lqrh_size_error.argtypes = [cl] * 4
    lib.lqrh_lds_bytes.argtypes = [ci, ci]
    lib.lqrh_lds_bytes.restype = cl
    lib.lqrh_cand_lds_bytes.argtypes = [ci, ci, ci]
    lib.lqrh_cand_lds_bytes.restype = cl
    lib.lqrh_gemm_tn.argtypes = [ci, ci, ci] + [ctypes.c_void_p] * 3
    return lib


def host_backward(lib, p, luu=None, mu=None):
    """The emulated kernel on a ``generate`` dict, dense [T, B, ...] inputs with Q, R, VxxT per system (step stride 0)."""
    T, B, nx, nu = p["A"].shape[0], p["A"].shape[1], p["A"].shape[2], p["B"].shape[3]
    luu = np.ascontiguousarray(p["R"] if luu is None else luu)
    mu = np.ascontiguousarray(np.broadcast_to(np.asarray(p["mu"] if mu is None else mu, dtype=np.float64), (B,)))
    keep = {k: np.ascontiguousarray(p[k]) for k in ("A", "B", "lx", "lu", "Q", "VxT", "VxxT")}
    out = {"k": np.full((T, B, nu), np.nan), "K": np.full((T, B, nu, nx), np.nan), "dV": np.full((B, 2), np.nan),
           "V0x": np.full((B, nx), np.nan), "V0xx": np.full((B, nx, nx), np.nan), "status": np.full(B, -7, dtype=np.int32)}
    a = BackwardArgs(T=T, B=B, nx=nx, nu=nu)
    S = lambda x, ss, es: Strided(x.ctypes.data, ss, es)
    a.A, a.Bm = S(keep["A"], B * nx * nx, nx * nx), S(keep["B"], B * nx * nu, nx * nu)
    a.lx, a.lu = S(keep["lx"], B * nx, nx), S(keep["lu"], B * nu, nu)
    a.lxx, a.luu, a.lux = S(keep["Q"], 0, nx * nx), S(luu, 0, nu * nu), Strided(None, 0, 0)
    a.VxT, a.VxxT, a.mu = S(keep["VxT"], 0, nx), S(keep["VxxT"], 0, nx * nx), S(mu, 0, 1)
    for k, v in out.items():
        setattr(a, k, v.ctypes.data)
    assert lib.lqrh_backward(ctypes.byref(a)) == 0
    out["k"], out["K"] = out["k"].transpose(1, 0, 2), out["K"].transpose(1, 0, 2, 3)
    return out


def host_candidates(lib, c, alphas, dx0, lo, hi, f32=False):
    """The emulated candidate kernel on a ``lqr_common.candidate_case`` (dense time-major inputs); dx0 None, [B, nx] or a shared [nx];
    lo / hi None or [nu].  The output starts as NaN so that anything not written shows."""
    T, B, nx, nu = c["A"].shape[0], c["A"].shape[1], c["A"].shape[2], c["B"].shape[3]
    alphas, dx0, lo, hi = (None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (alphas, dx0, lo, hi))
    cand = np.full((B, len(alphas), T, nu), np.nan, dtype=np.float32 if f32 else np.float64)
    a = CandArgs(T=T, B=B, nx=nx, nu=nu, nalpha=len(alphas), out_f32=int(f32))
    a.A, a.Bm = Strided(c["A"].ctypes.data, B * nx * nx, nx * nx), Strided(c["B"].ctypes.data, B * nx * nu, nx * nu)
    a.k, a.K, a.u = Strided(c["k"].ctypes.data, B * nu, nu), Strided(c["K"].ctypes.data, B * nu * nx, nu * nx), Strided(c["u"].ctypes.data, B * nu, nu)
    a.dx0 = Strided(None, 0, 0) if dx0 is None else Strided(dx0.ctypes.data, 0, nx if dx0.ndim == 2 else 0)
    a.alphas, a.cand = alphas.ctypes.data, cand.ctypes.data
    a.lo, a.hi = (None if x is None else x.ctypes.data for x in (lo, hi))
    assert lib.lqrh_candidates(ctypes.byref(a)) == 0
    return cand


# ---- 1. the kernel source on host threads ---------------------------------------------------------------------------------------------
# Both variants of the probe at their edges, M = 1 / 15 / 16 with one wave (N <= 64 stays within its four tiles) and 17 / 33 / 48 /
# 49 / 64 with four, N and K below, at and above a tile and a k-step.  The GPU suite runs the full product (200 shapes); a block of
# host threads costs more than a launch, so here: every (M, N) at K = 5 (a full k-step and a partial one), and every K at the four
# corner shapes of each variant.
PROBE_FIRST = [(54, 21, 54), (7, 3, 7), (64, 32, 64), (16, 64, 5), (3, 17, 1)]
PROBE_M1, PROBE_M4, PROBE_N, PROBE_K = (1, 15, 16), (17, 33, 48, 49, 64), (1, 16, 17, 33, 64), (1, 3, 4, 5, 64)
PROBE_ALL = PROBE_FIRST + [s for s in ((M, N, K) for M in PROBE_M1 + PROBE_M4 for N in PROBE_N for K in PROBE_K) if s not in PROBE_FIRST]
PROBE_HOST = [(M, N, K) for M, N, K in PROBE_ALL if (M, N, K) in PROBE_FIRST or K == 5 or (M in (1, 16, 17, 64) and N in (1, 64))]


@pytest.mark.parametrize("M,N,K", PROBE_HOST)
def test_tile_product_on_exact_integers(driver, M, N, K):
    """Small integers: every partial sum is exact, so the result must equal numpy's bit for bit whatever the summation order - any
    slip in the fragment maps (operand lane -> (row, k), result register -> row) or in the edge masking shows as a wrong entry.  The
    operands are asymmetric, so a transposed result cannot hide."""
    rng = np.random.default_rng(1)
    a = rng.integers(-9, 10, size=(K, M)).astype(np.float64)
    b = rng.integers(-9, 10, size=(K, N)).astype(np.float64)
    c = np.full((M, N), np.nan)
    driver.lqrh_gemm_tn(M, N, K, a.ctypes.data, b.ctypes.data, c.ctypes.data)
    assert np.array_equal(c, a.T @ b)


@pytest.mark.parametrize("nx,nu,T", [(4, 1, 200), (7, 3, 64), (12, 4, 200), (54, 21, 20)] + lc.EDGE_BACKWARD)
def test_recursion_matches_the_restatement(driver, nx, nu, T):
    """Error of each output against the long-double restatement, bounded by 8 x the float64 restatement's own error (floor 1e-13).
    With ``lqr_common.EDGE_BACKWARD`` every launch variant runs: <1, 8>, <1, 32> (nx <= 16 with nu > 8) and <4, 32>, and T = 1, 2."""
    B = 2 if nx > 16 else 3
    p = lc.generate(nx, nu, T, B)
    truth, f64 = lc.restate_batch(p, np.longdouble), lc.restate_batch(p, np.float64)
    got = host_backward(driver, p)
    assert (truth["status"] == 0).all() and (got["status"] == 0).all()
    assert got["K"].shape == (B, T, nu, nx) and got["k"].shape == (B, T, nu) and got["status"].tolist() == [0] * B
    for key in lc.OUTPUTS:
        mine, numpy64 = lc.rel_err(got[key], truth[key]), lc.rel_err(f64[key], truth[key])
        print(f"{(nx, nu, T)} {key}: kernel {mine:.2e}  float64 numpy {numpy64:.2e}")
        assert mine <= lc.bound(numpy64), (key, mine, numpy64)


@pytest.mark.parametrize("nx,nu", [(4, 1), (12, 4)])
def test_riccati_limit_is_scipys_dare(driver, nx, nu):
    """Constant (A, B), no linear terms, VxxT = Q, mu = 0, T = 3200 (twice the horizon the generator was first tried with: there the recursion itself has not converged): K_0 and V0xx against scipy.linalg.solve_discrete_are (the call the
    reference's controllers use).  Bound: 8 x what the float64 numpy recursion reaches, floor 1e-11."""
    from scipy.linalg import solve_discrete_are

    T = 3200        # the closed-loop spectral radii of these systems are 0.9957 / 0.9936: at 1600 steps the recursion is still 1e-7 / 1e-9 from its limit
    p = lc.generate(nx, nu, T, 1, constant=True)
    p["lx"][:] = 0; p["lu"][:] = 0; p["VxxT"] = p["Q"].copy(); p["mu"] = 0.0
    A, Bm, Q, R = p["A"][0, 0], p["B"][0, 0], p["Q"][0], p["R"][0]
    P = solve_discrete_are(A, Bm, Q, R)
    Kd = -np.linalg.solve(R + Bm.T @ P @ Bm, Bm.T @ P @ A)
    f64 = lc.restate_batch(p, np.float64)
    got = host_backward(driver, p)
    assert got["status"][0] == 0
    for key, ref, mine, np64 in (("K_0", Kd, got["K"][0, 0], f64["K"][0, 0]), ("P", P, got["V0xx"][0], f64["V0xx"][0])):
        e_mine, e_np = lc.rel_err(mine, ref), lc.rel_err(np64, ref)
        print(f"DARE {(nx, nu)} {key}: kernel {e_mine:.2e}  float64 numpy recursion {e_np:.2e}")
        assert e_mine <= lc.bound(e_np, lc.FLOOR_DARE), (key, e_mine, e_np)


def test_indefinite_quu_is_reported_not_propagated(driver):
    """luu = -I, mu = 0 for one system of five: status T (the first step solved), zeros for everything of that system; the others
    bitwise what a launch of those four alone returns."""
    nx, nu, T, B, badenv = 7, 3, 12, 5, 2
    p = lc.generate(nx, nu, T, B)
    luu = p["R"].copy(); luu[badenv] = -np.eye(nu)
    mu = np.full(B, p["mu"]); mu[badenv] = 0.0
    q = dict(p); q["R"], q["mu"] = luu, mu
    assert lc.restate_batch(q, np.longdouble)["status"][badenv] == T        # the long-double restatement finds the same pivot
    got = host_backward(driver, p, luu=luu, mu=mu)
    assert got["status"].tolist() == [0, 0, T, 0, 0]
    for key in lc.OUTPUTS:
        assert np.array_equal(got[key][badenv], np.zeros_like(got[key][badenv])), key
    keep = [e for e in range(B) if e != badenv]
    sub = {k: (v[:, keep] if k in ("A", "B", "lx", "lu") else v[keep] if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    alone = host_backward(driver, sub)
    for key in lc.OUTPUTS + ("status",):
        assert np.array_equal(got[key][keep], alone[key]), key
    assert all(np.isfinite(got[key]).all() for key in lc.OUTPUTS)


def test_candidates_match_the_restatement(driver):
    nx, nu, T, B, na = 7, 3, 30, 2, 5
    p = lc.generate(nx, nu, T, B)
    sol = lc.restate_batch(p, np.float64)
    rng = np.random.default_rng(5)
    lo, hi = np.full(nu, -0.8), np.full(nu, 0.9)
    u = np.ascontiguousarray(np.clip(rng.normal(size=(T, B, nu)), lo, hi))          # a nominal inside its bounds, some entries ON them
    k, K = np.ascontiguousarray(sol["k"].transpose(1, 0, 2)), np.ascontiguousarray(sol["K"].transpose(1, 0, 2, 3))
    alphas = np.array([0.0, 1.0, 0.5, 0.25, 0.01])
    A, Bm = np.ascontiguousarray(p["A"]), np.ascontiguousarray(p["B"])

    def run(alphas, lo, hi, f32):
        cand = np.full((B, len(alphas), T, nu), np.nan, dtype=np.float32 if f32 else np.float64)
        a = CandArgs(T=T, B=B, nx=nx, nu=nu, nalpha=len(alphas), out_f32=int(f32))
        a.A, a.Bm = Strided(A.ctypes.data, B * nx * nx, nx * nx), Strided(Bm.ctypes.data, B * nx * nu, nx * nu)
        a.k, a.K, a.u = Strided(k.ctypes.data, B * nu, nu), Strided(K.ctypes.data, B * nu * nx, nu * nx), Strided(u.ctypes.data, B * nu, nu)
        a.dx0 = Strided(None, 0, 0)
        a.alphas, a.lo, a.hi, a.cand = alphas.ctypes.data, lo.ctypes.data, hi.ctypes.data, cand.ctypes.data
        assert driver.lqrh_candidates(ctypes.byref(a)) == 0
        return cand

    got, got32 = run(alphas, lo, hi, False), run(alphas, lo, hi, True)
    for e in range(B):
        args = (A[:, e], Bm[:, e], k[:, e], K[:, e], u[:, e], alphas, None, lo, hi)
        truth, f64 = lc.restate_candidates(*args, np.longdouble), lc.restate_candidates(*args, np.float64)
        assert lc.rel_err(got[e], truth) <= lc.bound(lc.rel_err(f64, truth))
    assert np.array_equal(got[:, 0], np.clip(u, lo, hi).transpose(1, 0, 2))          # alpha = 0, dx0 = 0: clamp(u) = u, bitwise (dx stays 0)
    assert not np.array_equal(got[:, 1], got[:, 0])
    assert np.array_equal(got32, got.astype(np.float32))                              # rounded once


@pytest.mark.parametrize("nx,nu", [(12, 4), (16, 9), (17, 9)])
def test_results_do_not_depend_on_the_batch_position(driver, nx, nu):
    """One size per launch variant (<1, 8>, <1, 32>, <4, 32>): five systems in one launch against each system launched alone, every
    output bit for bit.  The emulation runs the systems one after the other in the SAME LDS buffer, so a read of LDS that the
    system itself has not written would show here."""
    T, B = 6, 5
    p = lc.generate(nx, nu, T, B)
    got = host_backward(driver, p)
    assert got["status"].tolist() == [0] * B
    for e in range(B):
        sub = {k: (v[:, e:e + 1] if k in ("A", "B", "lx", "lu") else v[e:e + 1] if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        alone = host_backward(driver, sub)
        for key in lc.OUTPUTS + ("status",):
            assert np.array_equal(got[key][e:e + 1], alone[key]), (e, key)


@pytest.mark.parametrize("dx0_kind,bounds_kind", lc.CAND_VARIANTS)
@pytest.mark.parametrize("nx,nu,T,B,na", lc.CAND_HOST_SIZES)
def test_candidates_at_the_edge_sizes(driver, nx, nu, T, B, na, dx0_kind, bounds_kind):
    """``lqr_common.CAND_HOST_SIZES`` x ``CAND_VARIANTS`` against the long-double restatement (``lqr_common.judge_candidates``); a dx0
    changes the kernel's result as it changes the restatement's; the float32 output is the float64 one rounded once."""
    c = lc.candidate_case(nx, nu, T, B, na)
    dx0, lo, hi = lc.candidate_variant(c, dx0_kind, bounds_kind)
    got = host_candidates(driver, c, c["alphas"], dx0, lo, hi)
    lc.judge_candidates(c, got, dx0_kind, bounds_kind, f"lqr/host/candidates/{nx}x{nu}x{T}x{B}x{na}/{dx0_kind}/{bounds_kind}")
    if dx0 is not None:
        assert not np.array_equal(got, host_candidates(driver, c, c["alphas"], None, lo, hi))
    assert np.array_equal(host_candidates(driver, c, c["alphas"], dx0, lo, hi, f32=True), got.astype(np.float32))


@pytest.mark.parametrize("nx,nu,T,B,na", lc.CAND_HOST_SIZES)
def test_candidates_zero_step_returns_the_clamped_nominal(driver, nx, nu, T, B, na):
    """alpha = 0 with dx0 = 0 (absent, and given as zeros) and a nominal inside its bounds, some entries on them: clamp(u) = u bit for
    bit - dx stays 0."""
    c = lc.candidate_case(nx, nu, T, B, na)
    lo, hi = np.full(nu, lc.CAND_LO), np.full(nu, lc.CAND_HI)
    alphas = np.array([0.0]) if na == 1 else c["alphas"]
    want = np.clip(c["u"], lo, hi).transpose(1, 0, 2)
    assert (want == lo).any() and (want == hi).any()
    for dx0 in (None, np.zeros((B, nx)), np.zeros(nx)):
        got = host_candidates(driver, c, alphas, dx0, lo, hi)
        assert alphas[0] == 0.0 and np.array_equal(got[:, 0], want)


# ---- 2. host arithmetic -----------------------------------------------------------------------------------------------------------------
def test_highest_element_matches_enumeration(driver):
    def hi(*a):
        out = ctypes.c_longlong(-7)
        return driver.lqrh_highest_element(*a, ctypes.byref(out)), int(out.value)

    rng = np.random.default_rng(0)
    for _ in range(300):
        T, B, n = (int(x) for x in rng.integers(1, 6, 3))
        ss, es = (int(x) for x in rng.integers(0, 40, 2))
        assert hi(T, B, n, ss, es) == (0, max(t * ss + e * es + i for t in range(T) for e in range(B) for i in range(n)))
    T, B, nx = 5, 3, 4                                          # the layouts the entry points meet
    for ss, es in ((B * nx * nx, nx * nx), (nx * nx, T * nx * nx), (0, 0), (0, nx * nx)):
        assert hi(T, B, nx * nx, ss, es)[1] == (T - 1) * ss + (B - 1) * es + nx * nx - 1
    for bad in ((0, 3, 2, 1, 1), (3, 0, 2, 1, 1), (3, 3, 0, 1, 1), (3, 3, 2, -1, 1), (3, 3, 2, 1, -1)):
        assert hi(*bad)[0] == 1, bad
    assert hi(1 << 20, 1 << 20, 8, (1 << 62) - 1, (1 << 62) - 1)[0] == 2


def test_size_limits_and_lds_layouts(driver):
    ok = driver.lqrh_size_error
    assert ok(1, 1, 64, 32) == 0 and ok(100, 4096, 4, 1) == 0
    assert ok(0, 1, 4, 1) == 1 and ok(1, 0, 4, 1) == 2 and ok(1, 1, 65, 1) == 3 and ok(1, 1, 0, 1) == 3 and ok(1, 1, 4, 33) == 4 and ok(1, 1, 4, 0) == 4
    sizes = [(nx, nu) for nx in (1, 2, 4, 7, 16, 17, 54, 64) for nu in (1, 3, 8, 9, 21, 32)]
    for nx, nu in sizes + [s for s in lc.EDGE_SIZES if s not in sizes]:
        assert ok(1, 1, nx, nu) == 0, (nx, nu)
        assert driver.lqrh_layout_ok(nx, nu) == 1, (nx, nu)
        assert driver.lqrh_lds_bytes(nx, nu) <= 160 * 1024, (nx, nu)
        assert driver.lqrh_cand_lds_bytes(nx, nu, 64) <= 160 * 1024, (nx, nu)
    assert driver.lqrh_lds_bytes(4, 1) < 2048                   # the cart-pole: many workgroups per compute unit


def test_no_accepted_shape_has_more_tiles_than_the_waves_hold(driver):
    """``lqr_gemm_tn`` / ``dare_gemm`` give each of the NW waves at most four 16 x 16 tiles and compute no tile beyond 4 NW, so every
    product of every accepted shape must fit: the products of the backward passes, of DARE and of the Lyapunov kernel are
    (nx or nu) x (nx or nu) with NW = lqr_waves(nx), the probe's is M x N with one wave for M <= 16 and four above (M, N <= 64 is what
    ``mjb_lqr_gemm_tn`` accepts).  The shapes that fill every slot - (16, 32) and (64, 32), the probe's (16, 64) and (64, 64) - are
    among those the exact-integer and restatement tests run."""
    tiles = lambda M, N: ((M + 15) // 16) * ((N + 15) // 16)
    full = set()
    for nx in range(1, 65):
        nw = driver.lqrh_waves(nx)
        assert nw == (1 if nx <= 16 else 4)
        for nu in range(1, 33):
            assert driver.lqrh_size_error(1, 1, nx, nu) == 0
            most = max(tiles(M, N) for M in (nx, nu) for N in (nx, nu))
            assert most <= 4 * nw, (nx, nu, most)
            if most == 4 * nw:
                full.add((nx, nu))
    assert (16, 32) in full and (64, 32) in full and (15, 16) not in full
    for M in range(1, 65):
        for N in range(1, 65):
            assert tiles(M, N) <= 4 * (1 if M <= 16 else 4), (M, N)
    assert driver.lqrh_size_error(1, 1, 65, 1) == 3 and driver.lqrh_size_error(1, 1, 4, 33) == 4      # beyond them the entry points refuse


# ---- 3. cross-compilation ---------------------------------------------------------------------------------------------------------------
def test_translation_unit_cross_compiles_with_the_f64_mfma(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is required: the kernels are HIP for gfx950")
    src = os.path.join(ROOT, "mujoco_template_amd", "csrc", "mjb_lqr.hip")
    asm = str(tmp_path / "mjb_lqr.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm, src])
    text = open(asm).read()
    assert "v_mfma_f64_16x16x4" in text
    for kernel in ("k_lqr_backward", "k_lqr_candidates", "k_lqr_gemm_probe"):
        assert kernel in text


def test_library_exports_the_entry_points():
    so = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    lib = ctypes.CDLL(so)
    for sym in ("mjb_lqr_backward", "mjb_lqr_candidates", "mjb_lqr_gemm_tn"):
        assert hasattr(lib, sym), sym
    import mujoco_template_amd as mt

    assert callable(mt.lqr_backward) and callable(mt.lqr_candidates)
