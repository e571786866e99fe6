"""The one-pass constraint-row assembly (make_constraint: limit objects and contacts in one lane pass, one impedance instance, the second
trip for a limit with both sides active, the caps) executed from the kernel SOURCE on the host (tests/hostemu), against the float64
oracle.  Start states and controls are those of tests/golden/make_rows_bits.py (cases humanoid, humanoid_caps, both_sides) at two
environments and 10 steps; tolerances are the ones tests/test_kernel_hostemu.py uses for the float64 instantiation.  CPU only."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import mjo
from tests.hostemu.emu import EmuEnv

_spec = importlib.util.spec_from_file_location("make_rows_bits", os.path.join(os.path.dirname(__file__), "golden", "make_rows_bits.py"))
rows_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rows_bits)

STEPS = 10


def _run(case, envs, G, ncon_max=0, nefc_max=0):
    """Free-running float64 emulation against the oracle from the case's start states: rows of the first forward pass, the counters of
    every step (rows, contacts, drops), the final state.  Returns the set of row types seen and the total drops."""
    c = rows_bits.CASES[case]
    cm = rows_bits.compiled_model(c["model"])
    om = mjo.OracleModel(cm)
    if ncon_max:
        om.set_limits(ncon_max, nefc_max)
    q, v = rows_bits.start_state(case, cm)
    types, drops = set(), np.zeros(2, dtype=np.int64)
    for env in envs:
        od = mjo.OracleData(om)
        e = EmuEnv(cm, G=G, use_double=True, ncon_max=ncon_max, nefc_max=nefc_max)
        od.qpos[:] = q[env]; od.qvel[:] = v[env]
        e.qpos[:] = q[env]; e.qvel[:] = v[env]
        od.forward(); e.forward()
        n = od.counters()["nefc"]
        assert e.counters[1] == n and e.counters[0] == od.counters()["ncon"]
        if n:
            assert np.abs(e.efc_J[: n * cm.nv] - od.efc_J).max() < 1e-12
            assert np.abs(e.efc_pos[:n] - od.efc_pos).max() < 1e-12
            assert np.abs(e.efc_aref[:n] - od.efc_aref).max() < 1e-9 * max(1.0, np.abs(od.efc_aref).max())
            assert np.abs(e.efc_D[:n] - od.efc_D).max() < 1e-9 * od.efc_D.max()
            assert (e.efc_type[:n] & 0xff).tolist() == od.efc_type().tolist()
        types.update(od.efc_type().tolist())
        od.qpos[:] = q[env]; od.qvel[:] = v[env]
        e.qpos[:] = q[env]; e.qvel[:] = v[env]
        for s in range(STEPS):
            u = od.random_ctrl(c["ctrl"][1], env, s, c["ctrl"][2])
            od.ctrl[:] = u; e.ctrl[:cm.nu] = u
            od.step(); e.step()
            oc = od.counters()
            assert (e.counters[0], e.counters[1], e.counters[2]) == (oc["ncon"], oc["nefc"], oc["solver_niter"]), (env, s)
            types.update(od.efc_type().tolist())
        drops += (e.counters[3], e.counters[4])
        assert np.abs(e.qpos - od.qpos).max() < 1e-10 and np.abs(e.qvel - od.qvel).max() < 1e-8, env
    return types, drops


@pytest.mark.parametrize("G", [16, 64])
def test_humanoid_limits_tendon_limit_and_contacts(G):
    """Hamstring tendon limit (environment 1), joint limits and foot / body contacts (prone keyframe, environment 6).  G = 16: more items
    (24 limit objects + contacts) than lanes, the chunked pass with its carried row counts; G = 64: one chunk."""
    types, drops = _run("humanoid", (1, 6), G)
    assert {0, 1, 3} <= types and drops.sum() == 0


@pytest.mark.parametrize("G", [16, 64])
def test_humanoid_row_and_contact_caps(G):
    """nefcmax = 8, nconmax = 2: limit rows dropped one by one, contacts that do not fit whole, the recount at the tail: contacts, rows and
    solver iterations equal the oracle's at every step (the two count what they drop in different units, so the drop counters are
    only required to be non-zero here; tests/test_gpu_rows_one_pass.py pins their values)."""
    types, drops = _run("humanoid_caps", (1, 6), G, ncon_max=2, nefc_max=8)
    assert drops[0] > 0 and drops[1] > 0


def test_limit_with_both_sides_active():
    """range = +-0.01 degrees with margin 0.05: both sides of the hinge limit are rows at once, lower before upper (the second trip)."""
    types, drops = _run("both_sides", (0, 1), 8)
    assert types == {0} and drops.sum() == 0
    cm = rows_bits.compiled_model("both_sides")
    e = EmuEnv(cm, G=8, use_double=True)
    e.qpos[0] = 0.004
    e.forward()
    half = np.radians(0.01)                                      # the range is in degrees
    assert e.counters[1] == 2 and e.efc_J[:2].tolist() == [1.0, -1.0]
    assert e.efc_pos[:2] == pytest.approx([0.004 + half, half - 0.004], abs=1e-15)
