"""Uniform record columns of the baked model (mjb::UniformCols in the generated translation units), the parts that need no GPU: the
emitted column sets against sets computed in numpy from the compiled model's arrays, signed zeros, batched fields, the shipped
models' kernels cross-compiled for gfx950, the host emulation on the small test models, and the oracle's word that the start
states of tests/test_gpu_uniform_columns.py make the rows they are for."""
import os
import re

import numpy as np
import pytest

from mujoco_template_amd import mjcf
from mujoco_template_amd._capi import ENV_PARAM_FIELDS, DeviceModel, compile_spec
from tests import uniform_columns_models as ucm
from tests.conftest import MODELS

_COLS = re.compile(r"// uniform columns of (\w+) \(stride (\d+)\)\ntemplate <> struct mjb::UniformCols<\d+> \{ static constexpr unsigned long long "
                   r"mask = 0x([0-9a-f]+)ull; static constexpr ([\w ]+) val\[(\d+)\] = \{([^}]*)\}; \};")


def emitted(source):
    """name -> (stride, set of uniform columns, {column: value as numpy scalar of the emitted type})"""
    out = {}
    for name, stride, mask, ctype, n, vals in _COLS.findall(source):
        assert int(n) == int(stride) and name not in out
        mask, vals = int(mask, 16), [v.strip() for v in vals.split(",")]
        cols = {k for k in range(int(stride)) if (mask >> k) & 1}
        val = {}
        for k in cols:
            if ctype == "int":
                val[k] = np.int32(int(vals[k]))
            elif ctype == "float":
                assert vals[k].endswith("f")
                val[k] = np.float32(float.fromhex(vals[k][:-1]))
            else:
                val[k] = np.float64(float.fromhex(vals[k]))
        out[name] = (int(stride), cols, val)
    return out


def uniform(records):
    """The same question asked of a [n, S] numpy array: columns whose bits are equal in every record (NaN: never)."""
    r = np.ascontiguousarray(records)
    bits = r.view({4: np.uint32, 8: np.uint64}[r.dtype.itemsize])
    cols = {k for k in range(r.shape[1]) if (bits[:, k] == bits[0, k]).all() and not (r.dtype.kind == "f" and np.isnan(r[0, k]))}
    return cols if r.shape[0] >= 2 else set()


def _clamp_solimp(si, T):
    s = si.astype(T)
    lo, hi = T(0.0001), T(0.9999)
    out = np.empty_like(s)
    for k in (0, 1, 3):
        out[:, k] = np.minimum(np.maximum(s[:, k], lo), hi)
    out[:, 2] = np.maximum(s[:, 2], T(0)); out[:, 4] = np.maximum(s[:, 4], T(1))
    return out


def _kb(solref, dmax_raw, timestep):
    dmax = np.clip(dmax_raw, 0.0001, 0.9999)
    assert (solref[:, 0] > 0).all()                               # (the models of this file use the time-constant form)
    tc = np.maximum(solref[:, 0], 2 * timestep); dr = solref[:, 1]
    return 1 / np.maximum(1e-15, dmax * dmax * tc * tc * dr * dr), 2 / np.maximum(1e-15, dmax * tc)


def records(cm, T):
    """pair_kb, lim_f, body_quat, actuator_ctrlrange as the kernels' record tables, rebuilt here from the compiled arrays."""
    a = cm.arrays
    gb, g1, g2 = a["geom_bodyid"], a["pair_geom1"], a["pair_geom2"]
    biw = a["body_invweight0"].reshape(-1, 2)
    kb = np.zeros((cm.npair, 12), dtype=T)
    if cm.npair:
        K, Bv = _kb(a["pair_solref"].reshape(-1, 2), a["pair_solimp"].reshape(-1, 5)[:, 1], cm.timestep)
        kb[:, 0] = (a["pair_margin"] - a["pair_gap"]).astype(T)
        kb[:, 1] = (biw[gb[g1], 0] + biw[gb[g2], 0]).astype(T)
        kb[:, 2] = K.astype(T); kb[:, 3] = Bv.astype(T)
        kb[:, 4:9] = _clamp_solimp(a["pair_solimp"].reshape(-1, 5), T)
    nobj = cm.njnt + cm.ntendon
    lf = np.zeros((nobj, 12), dtype=T)
    rng = np.concatenate([a["jnt_range"].reshape(-1, 2), a["tendon_range"].reshape(-1, 2)])
    mar = np.concatenate([a["jnt_margin"].ravel(), a["tendon_margin"].ravel()])
    diag = np.concatenate([a["dof_invweight0"][a["jnt_dofadr"]], a["tendon_invweight0"].ravel()])
    sr = np.concatenate([a["jnt_solref"].reshape(-1, 2), a["tendon_solref"].reshape(-1, 2)])
    si = np.concatenate([a["jnt_solimp"].reshape(-1, 5), a["tendon_solimp"].reshape(-1, 5)])
    K, Bv = _kb(sr, si[:, 1], cm.timestep)
    lf[:, 0:2] = rng.astype(T); lf[:, 2] = mar.astype(T); lf[:, 3] = diag.astype(T); lf[:, 4] = K.astype(T); lf[:, 5] = Bv.astype(T)
    lf[:, 6:11] = _clamp_solimp(si, T)
    return {"pair_kb": kb, "lim_f": lf, "body_quat": a["body_quat"].reshape(-1, 4).astype(T),
            "actuator_ctrlrange": a["actuator_ctrlrange"].reshape(-1, 2).astype(T)}


@pytest.fixture(scope="module")
def humanoid():
    cm = mjcf.compile_xml_path(MODELS["humanoid"])
    return cm, DeviceModel(cm)


@pytest.mark.parametrize("kind", ["step", "step2", "fd"])
def test_humanoid_uniform_columns_equal_numpy(humanoid, kind):
    """fp32 step kernels and the float64 finite-difference kernel: the emitted sets and values of pair_kb, lim_f, body_quat and
    actuator_ctrlrange are those of the arrays, bitwise per column at the record stride."""
    cm, dm = humanoid
    src = {"step": dm.spec_source, "step2": dm.step2_spec_source, "fd": dm.fd_spec_source}[kind]()
    T = np.float64 if kind == "fd" else np.float32
    got = emitted(src)
    want = records(cm, T)
    for name, rec in want.items():
        cols = uniform(rec)
        stride, gcols, gval = got.get(name, (rec.shape[1], set(), {}))
        assert stride == rec.shape[1] and gcols == cols, (name, sorted(gcols), sorted(cols))
        for k in cols:
            assert gval[k].dtype == rec.dtype and gval[k].tobytes() == rec[0, k].tobytes(), (name, k)
    # what the issue's table says of the shipped humanoid (a change of the model changes these on purpose)
    assert got["pair_kb"][1] == {0, 4, 7, 8, 9, 10, 11} and got["lim_f"][1] == {2, 9, 10, 11}
    assert got["body_quat"][1] == {0, 1, 2, 3} and got["actuator_ctrlrange"][1] == {0, 1}
    assert got["pair_kb"][2][7] == T(0.5) and got["pair_kb"][2][8] == T(2) and got["lim_f"][2][9] == T(0.5) and got["lim_f"][2][10] == T(2)


def test_every_table_is_still_emitted_in_full(humanoid):
    """Constants are emitted beside the tables, never instead of them: the tables of the translation unit are what they were."""
    cm, dm = humanoid
    src = dm.spec_source()
    tabs = re.findall(r"static const __constant__ \w[\w ]* mjb_tab_(\d+)\[\] = \{([^}]*)\};", src)
    assert [int(n) for n, _ in tabs] == list(range(len(tabs)))
    sizes = sorted(len(body.split(",")) for _, body in tabs)
    assert cm.npair * 12 in sizes and (cm.njnt + cm.ntendon) * 12 in sizes and cm.nbody * 4 in sizes


def test_signed_zeros_are_different_values():
    """ctrlrange (-0, 1) and (+0, 1): column 0 compares equal as numbers and is NOT uniform; column 1 is."""
    xml = ucm.arm_xml(ctrlrange1="-0 1", ctrlrange2="0 1")
    cm = mjcf.compile_xml_string(xml)
    cr = cm.arrays["actuator_ctrlrange"].reshape(-1, 2)
    assert cr[0, 0] == cr[1, 0] == 0 and np.signbit(cr[0, 0]) and not np.signbit(cr[1, 0])
    dm = DeviceModel(cm)
    for src in (dm.spec_source(), dm.fd_spec_source()):
        assert emitted(src)["actuator_ctrlrange"][1] == {1}
    same = DeviceModel(mjcf.compile_xml_string(ucm.arm_xml(ctrlrange1="0 1", ctrlrange2="0 1")))
    assert emitted(same.spec_source())["actuator_ctrlrange"][1] == {0, 1}


def test_small_models_columns():
    """The GPU test's models are what they say: everything uniform in the first, exactly the named columns not in the others."""
    import collections

    def get(xml):                                                  # (a table without a uniform column has no entry: the empty set)
        return collections.defaultdict(lambda: (0, set(), {}), emitted(DeviceModel(mjcf.compile_xml_string(xml)).spec_source()))

    u = get(ucm.ARM_CASES["uniform"])
    assert u["lim_f"][1] == set(range(12)) - {3} and u["actuator_ctrlrange"][1] == {0, 1} and u["dof_frec"][1] == {0, 1, 2, 3}
    assert u["body_quat"][1] == {0, 1, 2, 3}
    assert get(ucm.ARM_CASES["solimp_mid_power"])["lim_f"][1] == u["lim_f"][1] - {9, 10}
    assert get(ucm.ARM_CASES["ctrlrange"])["actuator_ctrlrange"][1] == set()
    for case in ("second_body_rotated", "first_body_rotated"):
        assert get(ucm.ARM_CASES[case])["body_quat"][1] == {1, 3}                 # w and y differ between the bodies
    s = get(ucm.SPHERE_CASES["uniform"])
    assert {0, 2, 3, 4, 5, 6, 7, 8} <= s["pair_kb"][1] and s["pair_friction"][1] == {0, 1, 2, 3, 4}
    t = get(ucm.SPHERE_CASES["margin_friction"])
    assert 0 not in t["pair_kb"][1] and 0 not in t["pair_friction"][1]


def test_batched_fields_get_no_constants(humanoid):
    cm, dm = humanoid
    plain = emitted(dm.spec_source())
    for name in ("actuator_gear", "actuator_gainprm", "actuator_biasprm", "pair_friction"):
        assert plain[name][1], name                                                 # (they do fold when nothing is batched)
    full = emitted(dm.spec_source(params=ENV_PARAM_FIELDS))
    for name in ("body_mass", "body_inertia", "dof_damping", "dof_armature", "actuator_gear", "actuator_gainprm", "actuator_biasprm",
                 "pair_friction", "body_subtreemass"):
        assert name not in full, name
    for name in ("pair_kb", "lim_f", "body_quat", "actuator_ctrlrange"):
        assert full[name] == plain[name], name
    # only damping batched: every other field folds as usual
    damp = emitted(dm.spec_source(params=("dof_damping",)))
    assert damp == plain or {k: v for k, v in damp.items() if k != "dof_frec"} == {k: v for k, v in plain.items() if k != "dof_frec"}
    # ... and the record column that holds a copy of the model's damping is not a constant then (the arm: one damping for both dofs)
    arm = DeviceModel(mjcf.compile_xml_string(ucm.ARM_CASES["uniform"]))
    assert 0 in emitted(arm.spec_source())["dof_frec"][1]
    assert emitted(arm.spec_source(params=("dof_damping",)))["dof_frec"][1] == {1, 2, 3}
    assert emitted(arm.fd_spec_source(params=("dof_damping",)))["dof_frec"][1] == {1, 2, 3}


def test_constants_are_keyed_to_table_pointers_only(humanoid):
    """Every UniformCols specialisation is keyed to a word of the baked DevModel image that is a TABLE POINTER (the image declares those
    as `p<word>`, every other word - sizes, the timestep, the run-time options disableactuator / iterations / tolerance - as a pair
    of unsigned): nothing but a record table can be folded, with or without batched fields, in either precision."""
    cm, dm = humanoid
    for src in (dm.spec_source(), dm.spec_source(params=ENV_PARAM_FIELDS), dm.step2_spec_source(), dm.fd_spec_source()):
        pointers = {int(w) for w in re.findall(r"const void MJB_CONST\* p(\d+);", src)}
        keys = [int(w) for w in re.findall(r"struct mjb::UniformCols<(\d+)>", src)]
        assert keys and len(keys) == len(set(keys)) and set(keys) <= pointers
        assert len(keys) == len(emitted(src))                          # (and every one of them is one the parser of this file saw)


def test_two_wave_kernel_exists_where_the_gpu_tests_compare_it():
    """The small models have a two-wave kernel at 64 lanes per environment and none at their default lanes: what
    tests/test_gpu_uniform_columns.py relies on when it requires that comparison."""
    for xml in list(ucm.ARM_CASES.values()) + list(ucm.SPHERE_CASES.values()):
        dm = DeviceModel(mjcf.compile_xml_string(xml))
        assert dm.step2_spec_source() is None
        two = dm.step2_spec_source(lanes=64)
        assert two is not None and emitted(two) == emitted(dm.spec_source(lanes=64))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("name", ["humanoid", "cartpole", "pendulum", "drone2"])
def test_shipped_kernels_cross_compile(name):
    """The step, two-wave and finite-difference translation units of a shipped model build for gfx950 (from the in-tree cache after
    build(), a few seconds each otherwise)."""
    dm = DeviceModel(mjcf.compile_xml_path(MODELS[name]))
    for src in (dm.spec_source(), dm.step2_spec_source(), dm.fd_spec_source(), dm.fd_spec_source(dtype="float64")):
        if src is not None:
            assert "mjb::UniformCols<" in src
            assert os.path.getsize(compile_spec(src)) > 0


def _oracle_counts(cm, q, v, steps, seed=5):
    from oracle import mjo

    om = mjo.OracleModel(cm)
    ncon, nefc = np.zeros((steps, len(q)), int), np.zeros((steps, len(q)), int)
    for e in range(len(q)):
        od = mjo.OracleData(om)
        od.qpos[:] = q[e]; od.qvel[:] = v[e]
        for s in range(steps):
            od.ctrl[:] = od.random_ctrl(seed, e, s, 1.0)
            od.step()
            c = od.counters()
            ncon[s, e], nefc[s, e] = c["ncon"], c["nefc"]
        assert np.isfinite(od.qpos).all()
    return ncon, nefc


def test_start_states_make_the_rows_the_gpu_cases_are_for():
    """The float64 oracle from the start states of tests/test_gpu_uniform_columns.py, 30 steps, 4 environments: limit rows for the arms,
    contacts for the spheres, more contacts than 8 lanes for the crowd - in every environment."""
    for xml in ucm.ARM_CASES.values():
        cm = mjcf.compile_xml_string(xml)
        ncon, nefc = _oracle_counts(cm, *ucm.arm_start(4), 30)
        assert (nefc[0] > 0).all() and ncon.sum() == 0
    for xml in ucm.SPHERE_CASES.values():
        cm = mjcf.compile_xml_string(xml)
        ncon, nefc = _oracle_counts(cm, *ucm.spheres_start(4, cm), 30)
        assert (ncon[0] >= 3).all() and (nefc[0] > 0).all()
    cm = mjcf.compile_xml_string(ucm.crowd_xml())
    ncon, nefc = _oracle_counts(cm, *ucm.crowd_start(4, cm), 30)
    assert (ncon[0] > 8).all()


@pytest.mark.parametrize("case", ["uniform", "solimp_mid_power"])
def test_host_emulation_of_the_accessor(case):
    """-DMJB_HOST_EMU: MJB_REC is the plain table read; the arm's limit rows and ten steps against the float64 oracle."""
    from oracle import mjo
    from tests.hostemu.emu import EmuEnv

    cm = mjcf.compile_xml_string(ucm.ARM_CASES[case])
    q, v = ucm.arm_start(2)
    om = mjo.OracleModel(cm)
    for env in range(2):
        od = mjo.OracleData(om)
        e = EmuEnv(cm, G=8, use_double=True)
        od.qpos[:] = q[env]; od.qvel[:] = v[env]
        e.qpos[:] = q[env]; e.qvel[:] = v[env]
        od.forward(); e.forward()
        n = od.counters()["nefc"]
        assert n > 0 and e.counters[1] == n
        assert np.abs(e.efc_D[:n] - od.efc_D).max() < 1e-9 * od.efc_D.max()
        assert np.abs(e.efc_aref[:n] - od.efc_aref).max() < 1e-9 * max(1.0, np.abs(od.efc_aref).max())
        for s in range(10):
            u = od.random_ctrl(5, env, s, 1.0)
            od.ctrl[:] = u; e.ctrl[:cm.nu] = u
            od.step(); e.step()
        assert np.abs(e.qpos - od.qpos).max() < 1e-10 and np.abs(e.qvel - od.qvel).max() < 1e-8
