"""Open-loop control sequences (``CTRL_SEQUENCE``, ``mjb_rollout_ctrl``) without a GPU: the step kernel's ``env_run`` compiled for the host
(``tests/ctrl_seq_host.cpp``, g++ -DMJB_HOST_EMU, one thread per lane) over a small batch, recording the ring of ``rollout()``
(qpos | qvel | sensordata | time after every step).  Checked against the same driver stepping one step at a time with ``ctrl`` written
before each step (bitwise), against the float64 oracle, and for a broadcast step stride of 0."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import mjo

HERE = os.path.dirname(os.path.abspath(__file__))
CTRL_KEEP, CTRL_SEQUENCE = 0, 4


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ctrl_seq") / "libctrl_seq_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "ctrl_seq_host.cpp")])
    lib = ctypes.CDLL(so)
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.ctrlseq_run.argtypes = [ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, cl, cl] + [vp] * 9
    lib.ctrlseq_run.restype = ci
    lib.ctrlseq_last_error.restype = ctypes.c_char_p
    return lib


class Batch:
    """float64 state arrays of `batch` environments, advanced in place by the emulated kernel."""

    def __init__(self, lib, cm, batch, G, use_double):
        from mujoco_template_amd._pack import PackedTable

        self.lib, self.cm, self.packed, self.B, self.G, self.use_double = lib, cm, PackedTable(cm), batch, G, use_double
        self.dim = cm.nq + cm.nv + cm.nsensordata + 1
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

    def run(self, nstep, mode, table=None, step_stride=0, env_stride=0):
        ring = np.full((nstep, self.B, self.dim), np.nan)
        p = self.packed
        s = self.s
        rc = self.lib.ctrlseq_run(p.n, p.names, p.ptrs, p.dtypes, p.counts, self.G, int(self.use_double), 64, 160, self.B, nstep, mode,
                                  None if table is None else table.ctypes.data, step_stride, env_stride,
                                  *[s[k].ctypes.data for k in ("qpos", "qvel", "ctrl", "qacc", "qacc_warmstart", "time", "counters", "sensordata")],
                                  ring.ctypes.data)
        assert rc == 0, self.lib.ctrlseq_last_error().decode()
        return ring


def _table(cm, B, T, seed=3):
    """[B, T, nu] controls inside the ctrl range, fp32-representable (the fp32 kernel keeps ctrl in fp32 and stores it back)."""
    lo, hi = np.full(cm.nu, -1.0), np.full(cm.nu, 1.0)
    rng_ = np.reshape(np.asarray(cm.arrays["actuator_ctrlrange"], dtype=np.float64), (-1, 2))
    lim = np.asarray(cm.arrays["actuator_ctrllimited"]).astype(bool)
    lo[lim], hi[lim] = rng_[lim, 0], rng_[lim, 1]
    u = np.random.default_rng(seed).uniform(lo, hi, size=(B, T, cm.nu))
    return u.astype(np.float32).astype(np.float64)


CASES = [("cartpole", 24), ("pendulum", 24), ("humanoid", 5)]


@pytest.mark.parametrize("G", [16, 64])
@pytest.mark.parametrize("use_double", [True, False], ids=["float64", "float32"])
@pytest.mark.parametrize("name,T", CASES)
def test_sequence_equals_stepwise_keep(driver, compiled, name, T, use_double, G):
    """(a) one launch of T sequence steps == T launches of one KEEP step with ctrl written before each: ring and final state bitwise."""
    cm = compiled(name)
    B = 3
    a = Batch(driver, cm, B, G, use_double)
    b = a.copy()
    tab = _table(cm, B, T)
    ring = a.run(T, CTRL_SEQUENCE, np.ascontiguousarray(tab), step_stride=cm.nu, env_stride=T * cm.nu)
    rows = []
    for t in range(T):
        b.s["ctrl"][:, :cm.nu] = tab[:, t]
        rows.append(b.run(1, CTRL_KEEP)[0])
    assert np.array_equal(ring, np.stack(rows)), "ring rows differ from the step-wise run"
    for k in a.s:
        assert np.array_equal(a.s[k], b.s[k]), k
    assert np.array_equal(a.s["ctrl"][:, :cm.nu], tab[:, -1])                 # data.ctrl holds the last applied control
    assert np.array_equal(ring[-1, :, :cm.nq], a.s["qpos"]) and np.array_equal(ring[-1, :, -1], a.s["time"])


def test_sequence_strides_address_any_layout(driver, compiled):
    """The same controls laid out [T, B, nu] (env stride nu, step stride B nu) give the same trajectory as the [B, T, nu] layout."""
    cm = compiled("cartpole")
    B, T = 3, 16
    a = Batch(driver, cm, B, 16, True)
    b = a.copy()
    tab = _table(cm, B, T)
    ra = a.run(T, CTRL_SEQUENCE, np.ascontiguousarray(tab), step_stride=cm.nu, env_stride=T * cm.nu)
    rb = b.run(T, CTRL_SEQUENCE, np.ascontiguousarray(tab.transpose(1, 0, 2)), step_stride=B * cm.nu, env_stride=cm.nu)
    assert np.array_equal(ra, rb)
    assert not np.array_equal(ra[:, 0], ra[:, 1])                              # the environments did get different controls


@pytest.mark.parametrize("name,T,G", [("cartpole", 40, 16), ("pendulum", 40, 16), ("drone2", 30, 16), ("humanoid", 8, 64)])
def test_float64_sequence_tracks_oracle(driver, compiled, name, T, G):
    """(b) float64 ring vs the oracle with ctrl set before each step(1), at every step (tolerances of the host-emulation suite)."""
    cm = compiled(name)
    B = 2
    a = Batch(driver, cm, B, G, True)
    q0, v0 = a.s["qpos"].copy(), a.s["qvel"].copy()
    tab = _table(cm, B, T, seed=11)
    ring = a.run(T, CTRL_SEQUENCE, np.ascontiguousarray(tab), step_stride=cm.nu, env_stride=T * cm.nu)
    om = mjo.OracleModel(cm)
    nq, nv, ns = cm.nq, cm.nv, cm.nsensordata
    for e in range(B):
        od = mjo.OracleData(om)
        od.qpos[:] = q0[e]; od.qvel[:] = v0[e]
        for t in range(T):
            od.ctrl[:] = tab[e, t]
            od.step()
            row = ring[t, e]
            assert np.abs(row[:nq] - od.qpos).max() < 1e-10, (e, t)
            assert np.abs(row[nq:nq + nv] - od.qvel).max() < 1e-8, (e, t)
            if ns:
                assert np.abs(row[nq + nv:nq + nv + ns] - od.sensordata).max() < 1e-9, (e, t)
            assert row[-1] == pytest.approx(od.time)


@pytest.mark.parametrize("use_double", [True, False], ids=["float64", "float32"])
def test_step_stride_zero_is_a_constant_ctrl(driver, compiled, use_double):
    """(c) step stride 0: every step reads the same row == a KEEP rollout on that ctrl."""
    cm = compiled("humanoid")
    B, T = 2, 4
    a = Batch(driver, cm, B, 16, use_double)
    b = a.copy()
    row = _table(cm, B, 1)[:, 0]
    ring = a.run(T, CTRL_SEQUENCE, np.ascontiguousarray(row), step_stride=0, env_stride=cm.nu)
    b.s["ctrl"][:, :cm.nu] = row
    assert np.array_equal(ring, b.run(T, CTRL_KEEP))
    for k in a.s:
        assert np.array_equal(a.s[k], b.s[k]), k
