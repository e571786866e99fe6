"""The trajectory-cost and selection kernels (``mjb_traj_cost`` / ``mjb_traj_select``) without a GPU.

  1. the kernel source itself (``mjb_traj.hpp``) compiled for the host (``tests/traj_host.cpp``, g++ -DMJB_HOST_EMU: one thread per
     lane) against the numpy restatement of ``tests/traj_common.py`` (long double = truth, float64 = the measure of the bound), against
     the library's host ``mjb_differentiate_pos``, on exact integers, for position independence and for non-finite input;
  2. the extent and size arithmetic of the argument checks against enumeration;
  3. the translation unit cross-compiles for gfx950, and the library exports the entry points.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import lqr_common as lc
from tests import traj_common as tc
from tests.conftest import measured

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Strided(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("ss", ctypes.c_long), ("es", ctypes.c_long)]


class CostArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("T", "B", "nq", "nv", "nu", "njnt", "state_f32", "ctrl_f32")] + \
               [(n, Strided) for n in ("qpos0", "qvel0", "qpos", "qvel", "ctrl", "qref", "vref", "uref", "Q", "R", "Qf")] + \
               [(n, ctypes.c_void_p) for n in ("jnt_type", "jnt_qposadr", "jnt_dofadr", "cost", "cost_t", "lx", "lu", "VxT")]


class SelectArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("nprob", "T", "nu", "mode", "cand_f32", "out_f32")] + \
               [("ncand", ctypes.c_long), ("temperature", ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ("cost", "cand", "u_out", "best", "best_cost", "weights")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("traj") / "libtraj_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "traj_host.cpp")])
    lib = ctypes.CDLL(so)
    cl, ci = ctypes.c_long, ctypes.c_int
    lib.trajh_cost.argtypes = [ctypes.POINTER(CostArgs), ci]
    lib.trajh_select.argtypes = [ctypes.POINTER(SelectArgs)]
    lib.trajh_highest_element.argtypes = [cl] * 5 + [ctypes.POINTER(ctypes.c_longlong)]
    lib.trajh_cost_size_error.argtypes = [cl] * 5
    lib.trajh_select_size_error.argtypes = [cl] * 4 + [ci, ctypes.c_double]
    lib.trajh_cost_tiles.argtypes = [cl, cl]
    lib.trajh_cost_tiles.restype = cl
    lib.trajh_cost_lds_bytes.argtypes = [ci, ci]
    lib.trajh_cost_lds_bytes.restype = cl
    return lib


@pytest.fixture(scope="module")
def tables(compiled):
    from mujoco_template_amd.mjcf import compile_xml_string
    from tests import large_models

    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = compile_xml_string(large_models.two_free_xml()) if name == "two_free" else compiled(name)
        return cache[name]

    return get


def host_cost(lib, cm, case, layout="batch_major", gradients=True, grid=3):
    """The emulated kernels on a ``traj_common.generate`` case.  The states lie in a ring-like buffer (a time column in front, two pad
    columns behind) laid out [T, B, dim] (time_major) or [B, T, dim] (batch_major) and are read in place through (pointer, step stride,
    env stride); Q and R are passed once (both strides 0) when the case holds one matrix, per (t, e) otherwise."""
    nq, nv, nu = case["nq"], case["nv"], case["nu"]
    nx, ns = 2 * nv, nq + nv
    x, u = case["x"], case["u"]
    B, T = x.shape[0], x.shape[1] - 1
    jt, jq, jd = tc.joint_table(cm)
    dim = 1 + ns + 2
    tm = layout == "time_major"
    ring = np.full((T, B, dim) if tm else (B, T, dim), 7.5, dtype=x.dtype)
    ctrl = np.zeros((T, B, nu) if tm else (B, T, nu), dtype=u.dtype)
    if tm:
        ring[:, :, 1:1 + ns], ctrl[:] = x[:, 1:].transpose(1, 0, 2), u.transpose(1, 0, 2)
    else:
        ring[:, :, 1:1 + ns], ctrl[:] = x[:, 1:], u
    x0 = np.ascontiguousarray(np.concatenate([np.zeros((B, 1), dtype=x.dtype), x[:, 0]], axis=1))
    size = x.dtype.itemsize
    rs, re = (B * dim, dim) if tm else (dim, T * dim)
    us, ue = (B * nu, nu) if tm else (nu, T * nu)
    keep = {k: np.ascontiguousarray(case[k], dtype=np.float64) for k in ("x_ref", "Q", "R", "Qf")}
    uref = None if case.get("u_ref") is None else np.ascontiguousarray(np.broadcast_to(case["u_ref"], u.shape), dtype=np.float64)
    full_ref = keep["x_ref"].ndim == 3
    a = CostArgs(T=T, B=B, nq=nq, nv=nv, nu=nu, njnt=len(jt), state_f32=int(x.dtype == np.float32), ctrl_f32=int(u.dtype == np.float32))
    a.qpos0, a.qvel0 = Strided(x0.ctypes.data + size, 0, 1 + ns), Strided(x0.ctypes.data + size * (1 + nq), 0, 1 + ns)
    a.qpos, a.qvel = Strided(ring.ctypes.data + size, rs, re), Strided(ring.ctypes.data + size * (1 + nq), rs, re)
    a.ctrl = Strided(ctrl.ctypes.data, us, ue)
    a.qref = Strided(keep["x_ref"].ctypes.data, ns if full_ref else 0, (T + 1) * ns if full_ref else 0)
    a.vref = Strided(keep["x_ref"].ctypes.data + 8 * nq, a.qref.ss, a.qref.es)
    a.uref = Strided(None, 0, 0) if uref is None else Strided(uref.ctypes.data, nu, T * nu)
    a.Q = Strided(keep["Q"].ctypes.data, *((nx * nx, T * nx * nx) if keep["Q"].ndim == 4 else (0, 0)))
    a.R = Strided(keep["R"].ctypes.data, *((nu * nu, T * nu * nu) if keep["R"].ndim == 4 else (0, 0)))
    a.Qf = Strided(keep["Qf"].ctypes.data, 0, nx * nx if keep["Qf"].ndim == 3 else 0)
    a.jnt_type, a.jnt_qposadr, a.jnt_dofadr = jt.ctypes.data, jq.ctypes.data, jd.ctypes.data
    out = {"cost": np.full(B, np.nan), "cost_t": np.full((B, T + 1), np.nan)}
    if gradients:
        out.update({"lx": np.full((T, B, nx), np.nan), "lu": np.full((T, B, nu), np.nan), "VxT": np.full((B, nx), np.nan)})
    for k in tc.COST_OUTPUTS:
        setattr(a, k, out[k].ctypes.data if k in out else None)
    assert lib.trajh_cost(ctypes.byref(a), grid) == 0
    assert (ring[..., 0] == 7.5).all() and (ring[..., 1 + ns:] == 7.5).all()
    if gradients:
        out["lx"], out["lu"] = out["lx"].transpose(1, 0, 2), out["lu"].transpose(1, 0, 2)
    return out


def restated(cm, case, dtype):
    return tc.restate_cost(tc.joint_table(cm), case["nq"], case["nv"], case["nu"], case["x"], case["u"], case["x_ref"], case.get("u_ref"),
                           case["Q"], case["R"], case["Qf"], dtype)


def compare(tag, got, truth, f64, keys=tc.COST_OUTPUTS):
    for key in keys:
        mine, numpy64 = lc.rel_err(got[key], truth[key]), lc.rel_err(f64[key], truth[key])
        print(f"{tag} {key}: kernel {mine:.3e}  float64 numpy {numpy64:.3e}  bound {lc.bound(numpy64):.3e}")
        measured(f"traj/{tag}/{key}", mine, lc.bound(numpy64), f"(float64 numpy restatement: {numpy64:.3e})")


# ---- 1. cost and expansion against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["time_major", "batch_major"])
@pytest.mark.parametrize("per_point", [False, True], ids=["Q_broadcast", "Q_per_point"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,T,B", [("cartpole", 7, 3), ("humanoid", 5, 2), ("two_free", 2, 2)])
def test_cost_matches_the_restatement(driver, tables, name, T, B, dtype, per_point, layout):
    cm = tables(name)
    case = tc.generate(cm, T, B, seed=1, state_dtype=dtype, per_point_cost=per_point)
    case["u"] = case["u"].astype(dtype)
    truth, f64 = restated(cm, case, np.longdouble), restated(cm, case, np.float64)
    got = host_cost(driver, cm, case, layout=layout)
    assert np.array_equal(truth["dx"][0, 1, :case["nv"]], np.zeros(case["nv"]))              # the point with qpos == qref
    compare(f"host/{name}/{np.dtype(dtype).name}/{'pp' if per_point else 'bc'}/{layout}", got, truth, f64)
    nocost = host_cost(driver, cm, case, layout=layout, gradients=False)                       # the optional outputs left out
    assert np.array_equal(nocost["cost"], got["cost"]) and np.array_equal(nocost["cost_t"], got["cost_t"])


# ---- 2. the tangent-space difference against the library's host function -----------------------------------------------------------------
def test_dx_is_the_librarys_differentiate_pos(driver, tables):
    """Q = I makes lx = dx (the products with 0 and 1 are exact): the kernel's dx of the humanoid against mjb_differentiate_pos, a
    reference that shares nothing with the test's own numpy; the point with qpos == qref gives dx = 0 exactly."""
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    from mujoco_template_amd._capi import DeviceModel

    cm = tables("humanoid")
    T, B = 5, 2
    case = tc.generate(cm, T, B, seed=2)
    nq, nv = case["nq"], case["nv"]
    case["Q"], case["Qf"], case["x_ref"][..., nq:] = np.eye(2 * nv), np.eye(2 * nv), 0.0
    got = host_cost(driver, cm, case)
    dx = np.concatenate([got["lx"], got["VxT"][:, None]], axis=1)[:, 1:]                     # points 1 .. T
    dm = DeviceModel(cm)
    ref = np.zeros((B * T, nv))
    dm.differentiate_pos(ref, 1.0, np.ascontiguousarray(case["x_ref"][:, 1:, :nq]).reshape(B * T, nq), np.ascontiguousarray(case["x"][:, 1:, :nq]).reshape(B * T, nq))
    truth, f64 = restated(cm, case, np.longdouble), restated(cm, case, np.float64)
    numpy64 = lc.rel_err(f64["dx"], truth["dx"])
    mine = lc.rel_err(dx[..., :nv].reshape(B * T, nv), ref)
    print(f"dx vs mjb_differentiate_pos: {mine:.3e}  float64 numpy vs truth {numpy64:.3e}")
    measured("traj/host/humanoid/dx_vs_differentiate_pos", mine, lc.bound(numpy64))
    measured("traj/host/humanoid/dx_vs_truth", lc.rel_err(dx, truth["dx"][:, 1:]), lc.bound(numpy64))
    assert np.array_equal(dx[0, 0, :nv], np.zeros(nv))                                        # point (0, 1): qpos == qref
    assert np.abs(ref[0]).max() == 0.0


# ---- 3. exact integers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_point", [False, True], ids=["Q_broadcast", "Q_per_point"])
def test_exact_integers_are_bit_equal_to_numpy(driver, tables, per_point):
    """Cart-pole (a slide and a hinge): small-integer states, references, Q, R - every partial sum is exact, so the results equal
    numpy's bit for bit whatever the order, and any slip in indexing or transposition shows.  Q is symmetric with entries of very
    different magnitudes per position (1 .. 4 digits), so a permuted row or column changes the result."""
    cm = tables("cartpole")
    T, B, nq, nv, nu, nx = 5, 3, 2, 2, 1, 4
    rng = np.random.default_rng(3)
    lead = (B, T) if per_point else ()
    scale = np.array([[1, 10, 100, 1000], [10, 1, 1000, 100], [100, 1000, 1, 10], [1000, 100, 10, 1]], dtype=np.float64)
    G = rng.integers(1, 10, size=lead + (nx, nx)).astype(np.float64)
    Q = (G + np.swapaxes(G, -1, -2)) * scale
    Gf = rng.integers(1, 10, size=(nx, nx)).astype(np.float64)
    case = {"x": rng.integers(-9, 10, size=(B, T + 1, nq + nv)).astype(np.float64), "u": rng.integers(-9, 10, size=(B, T, nu)).astype(np.float64),
            "x_ref": rng.integers(-4, 5, size=(B, T + 1, nq + nv)).astype(np.float64), "u_ref": rng.integers(-4, 5, size=(B, T, nu)).astype(np.float64),
            "Q": Q, "R": rng.integers(1, 10, size=lead + (nu, nu)).astype(np.float64), "Qf": (Gf + Gf.T) * scale, "nq": nq, "nv": nv, "nu": nu}
    assert not np.array_equal(case["Qf"], case["Qf"][::-1, ::-1])
    ref = restated(cm, case, np.float64)
    for layout in ("time_major", "batch_major"):
        got = host_cost(driver, cm, case, layout=layout)
        for key in tc.COST_OUTPUTS:
            assert np.array_equal(got[key], ref[key]), (key, layout)


# ---- 4. position independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", [("cartpole", 7), ("humanoid", 5)])
def test_a_trajectory_gives_the_same_bits_anywhere(driver, tables, name, T):
    """One trajectory alone, and the same trajectory as element 5 of a batch of 7 (another tile slot, other neighbours, another grid)."""
    cm = tables(name)
    big = tc.generate(cm, T, 7, seed=4, per_point_cost=True)
    one = {k: (v[5:6] if isinstance(v, np.ndarray) and v.ndim >= 3 else v) for k, v in big.items()}
    a, b = host_cost(driver, cm, big, grid=3), host_cost(driver, cm, one, grid=1)
    for key in tc.COST_OUTPUTS:
        assert np.array_equal(a[key][5:6], b[key]), key


# ---- 5. non-finite input -------------------------------------------------------------------------------------------------------------------------
def test_a_nan_state_costs_inf_and_touches_nothing_else(driver, tables):
    cm = tables("humanoid")
    case = tc.generate(cm, 5, 3, seed=5)
    clean = host_cost(driver, cm, case)
    case["x"][1, 3, 9] = np.nan
    got = host_cost(driver, cm, case)
    assert got["cost"][1] == np.inf and np.isfinite(got["cost"][[0, 2]]).all()
    for key in tc.COST_OUTPUTS:
        assert np.array_equal(got[key][[0, 2]], clean[key][[0, 2]]), key
    case["x"][1, 3, 9] = np.inf                                                               # an infinite sum is +inf too, never NaN
    assert host_cost(driver, cm, case)["cost"][1] == np.inf


# ---- 6. select ---------------------------------------------------------------------------------------------------------------------------------------
def host_select(lib, cost, cand, mode, temperature=0.0, out_dtype=None, sentinel=-77.0):
    G, n, T, nu = cand.shape
    out_dtype = cand.dtype if out_dtype is None else np.dtype(out_dtype)
    cost, cand = np.ascontiguousarray(cost, dtype=np.float64), np.ascontiguousarray(cand)
    out = {"u": np.full((G, T, nu), sentinel, dtype=out_dtype), "best": np.full(G, -9, dtype=np.int32), "best_cost": np.full(G, np.nan),
           "weights": np.full((G, n), np.nan)}
    a = SelectArgs(nprob=G, T=T, nu=nu, mode=int(mode == "softmin"), cand_f32=int(cand.dtype == np.float32), out_f32=int(out_dtype == np.float32),
                   ncand=n, temperature=temperature)
    a.cost, a.cand, a.u_out = cost.ctypes.data, cand.ctypes.data, out["u"].ctypes.data
    a.best, a.best_cost, a.weights = out["best"].ctypes.data, out["best_cost"].ctypes.data, out["weights"].ctypes.data
    assert lib.trajh_select(ctypes.byref(a)) == 0
    return out


def test_argmin_ties_non_finite_costs_and_the_copy(driver):
    rng = np.random.default_rng(6)
    G, n, T, nu = 4, 9, 3, 2
    cand = rng.normal(size=(G, n, T, nu))
    cost = rng.integers(3, 9, size=(G, n)).astype(np.float64)
    cost[0, [6, 2, 4]] = 1.0                                      # ties: the lowest index
    cost[1, 0], cost[1, 1], cost[1, 5] = -np.inf, np.nan, 2.0     # non-finite costs are skipped (-inf included)
    cost[2, :] = [np.nan, np.inf, -np.inf] * 3                    # nothing finite
    cost[3, 8] = -5.0
    got = host_select(driver, cost, cand, "argmin")
    assert got["best"].tolist() == [2, 5, -1, 8]
    assert got["best_cost"].tolist() == [1.0, 2.0, np.inf, -5.0]
    for g, b in ((0, 2), (1, 5), (3, 8)):
        assert np.array_equal(got["u"][g], cand[g, b])
    assert (got["u"][2] == -77.0).all()                           # unwritten: the sentinel is intact
    got32 = host_select(driver, cost, cand, "argmin", out_dtype=np.float32)
    for g, b in ((0, 2), (1, 5), (3, 8)):
        assert np.array_equal(got32["u"][g], np.float32(cand[g, b]))
    assert (got32["u"][2] == np.float32(-77.0)).all()
    c32 = cand.astype(np.float32)
    assert np.array_equal(host_select(driver, cost, c32, "argmin")["u"][0], c32[0, 2])                     # float32 -> float32: a bit copy
    assert np.array_equal(host_select(driver, cost, c32, "argmin", out_dtype=np.float64)["u"][0], c32[0, 2].astype(np.float64))
    wide = rng.normal(size=(1, 3, 150, 3))                        # T * nu = 450: 29 chunks of 16 elements, the last one partial
    assert np.array_equal(host_select(driver, np.array([[2.0, 1.0, 3.0]]), wide, "argmin")["u"][0], wide[0, 1])


@pytest.mark.parametrize("ncand", [1, 5, 64, 1000])
def test_softmin_matches_the_restatement(driver, ncand):
    """Weights and the weighted controls against the restatement; one infinite cost (weight exactly 0) and, in the second problem, a
    temperature so small against the cost gaps that one weight is exactly 1."""
    rng = np.random.default_rng(7)
    G, T, nu = 2, 4, 3
    cand = rng.normal(size=(G, ncand, T, nu))
    cost = rng.uniform(1.0, 3.0, size=(G, ncand))
    cost[1] = 1.0 + 1e6 * np.arange(ncand)[rng.permutation(ncand)]
    if ncand > 1:
        cost[0, ncand // 2] = np.inf
    temperature = 0.7
    truth, f64 = tc.restate_select(cost, cand, "softmin", temperature, np.longdouble), tc.restate_select(cost, cand, "softmin", temperature, np.float64)
    got = host_select(driver, cost, cand, "softmin", temperature)
    assert np.array_equal(got["best"], truth["best"]) and np.array_equal(got["best_cost"], cost[np.arange(G), truth["best"]])
    for key in ("weights", "u"):
        mine, numpy64 = lc.rel_err(got[key], truth[key]), lc.rel_err(f64[key], truth[key])
        print(f"softmin n={ncand} {key}: kernel {mine:.3e}  float64 numpy {numpy64:.3e}")
        measured(f"traj/host/softmin/{ncand}/{key}", mine, lc.bound(numpy64))
    if ncand > 1:
        assert got["weights"][0, ncand // 2] == 0.0
    assert got["weights"][1].max() == 1.0 and np.count_nonzero(got["weights"][1]) == 1
    assert np.array_equal(got["u"][1], cand[1, truth["best"][1]])
    got32 = host_select(driver, cost, cand.astype(np.float32), "softmin", temperature, out_dtype=np.float32)
    t32 = tc.restate_select(cost, cand.astype(np.float32), "softmin", temperature, np.longdouble)
    assert tc.float32_ulp_error(got32["u"], t32["u"]) <= 1.0
    none = host_select(driver, np.full((1, ncand), np.nan), cand[:1], "softmin", temperature)
    assert none["best"][0] == -1 and none["best_cost"][0] == np.inf and (none["u"] == -77.0).all() and (none["weights"] == 0.0).all()


# ---- 7. host arithmetic ----------------------------------------------------------------------------------------------------------------------------
def test_extents_and_size_limits(driver):
    def hi(*a):
        out = ctypes.c_longlong(-7)
        return driver.trajh_highest_element(*a, ctypes.byref(out)), int(out.value)

    rng = np.random.default_rng(0)
    for _ in range(300):
        T, B, n = (int(x) for x in rng.integers(1, 6, 3))
        ss, es = (int(x) for x in rng.integers(0, 40, 2))
        assert hi(T, B, n, ss, es) == (0, max(t * ss + e * es + i for t in range(T) for e in range(B) for i in range(n)))
    T, B, nq, nv, dim = 5, 3, 28, 27, 60                          # the layouts the entry point meets: a ring's columns, T + 1 reference points
    assert hi(T, B, nq, B * dim, dim)[1] == (T - 1) * B * dim + (B - 1) * dim + nq - 1
    assert hi(T + 1, B, nq, nq + nv, (T + 1) * (nq + nv))[1] == (B * (T + 1) - 1) * (nq + nv) + nq - 1
    assert hi(1, B, nq, 0, dim)[1] == (B - 1) * dim + nq - 1 and hi(T, B, 16, 0, 0)[1] == 15
    for bad in ((0, 3, 2, 1, 1), (3, 0, 2, 1, 1), (3, 3, 0, 1, 1), (3, 3, 2, -1, 1), (3, 3, 2, 1, -1)):
        assert hi(*bad)[0] == 1, bad
    assert hi(1 << 20, 1 << 20, 8, (1 << 62) - 1, (1 << 62) - 1)[0] == 2
    ok = driver.trajh_cost_size_error
    assert ok(1, 1, 66, 64, 64) == 0 and ok(500, 4096, 28, 27, 21) == 0
    assert [ok(0, 1, 2, 2, 1), ok(1, 0, 2, 2, 1), ok(1, 1, 65, 65, 1), ok(1, 1, 2, 2, 65), ok(1, 1, 2, 2, 0), ok(1, 1, 1, 2, 1)] == [1, 2, 3, 4, 4, 5]
    sel = driver.trajh_select_size_error
    assert sel(1, 1 << 20, 50, 21, 0, 0.0) == 0 and sel(256, 16, 100, 1, 1, 0.5) == 0
    assert [sel(0, 4, 3, 1, 0, 0.0), sel(1, (1 << 20) + 1, 3, 1, 0, 0.0), sel(1, 0, 3, 1, 0, 0.0), sel(1, 4, 0, 1, 0, 0.0), sel(1, 4, 3, 1, 2, 0.0),
            sel(1, 4, 3, 1, 1, 0.0), sel(1, 4, 3, 1, 1, -1.0), sel(1, 4, 3, 1, 1, float("nan"))] == [1, 2, 2, 3, 4, 5, 5, 5]
    for T, B in ((1, 1), (7, 3), (5, 2), (50, 4096), (8, 1), (3, 8)):
        assert driver.trajh_cost_tiles(T, B) == -(-T * B // 8) + -(-B // 8)
    assert driver.trajh_cost_lds_bytes(64, 64) <= 64 * 1024


# ---- 8. cross-compilation, 9. exports ------------------------------------------------------------------------------------------------------------
def test_translation_unit_cross_compiles_for_gfx950(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is required: the kernels are HIP for gfx950")
    src = os.path.join(ROOT, "mujoco_template_amd", "csrc", "mjb_traj.hip")
    asm = str(tmp_path / "mjb_traj.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm, src])
    text = open(asm).read()
    for kernel in ("k_traj_cost", "k_traj_cost_sum", "k_traj_select"):
        assert kernel in text
    assert "v_fma_f64" in text and "amdgcn-amd-amdhsa--gfx950" in text


def test_library_exports_the_entry_points():
    so = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    lib = ctypes.CDLL(so)
    for sym in ("mjb_traj_cost", "mjb_traj_select"):
        assert hasattr(lib, sym), sym
    header = open(os.path.join(ROOT, "include", "mjbatch.h")).read()
    for text in ("int mjb_traj_cost(", "int mjb_traj_select(", "examples/humanoid/controllers/lqr.py:97-114", "examples/humanoid/controllers/lqr.py:153"):
        assert text in header
    import mujoco_template_amd as mt

    assert callable(mt.trajectory_cost) and callable(mt.select_candidates)
