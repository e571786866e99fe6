"""Constraint rows and short rollouts, bit for bit against the recorded build (tests/golden/rows_bits.npz, written by
tests/golden/make_rows_bits.py on an MI355X before make_constraint became one pass over limit objects and contacts): the generic fp32
kernel, the specialised one, and the two-wave kernel where the model has one.  The existing bitwise tests compare instantiations of
the same source with each other; this one pins all of them to the bytes of the earlier source.  A pull request that changes upstream
arithmetic on purpose regenerates the fixture (see the generator's docstring)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_rows_bits", os.path.join(_HERE, "golden", "make_rows_bits.py"))
rows_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rows_bits)


@pytest.fixture(scope="module")
def golden():
    return np.load(rows_bits.OUT)


@pytest.fixture(scope="module")
def device_models():
    from mujoco_template_amd._capi import DeviceModel

    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = DeviceModel(rows_bits.compiled_model(model))
        return cache[model]

    return get


def _types(golden, case, tag):
    t, n = golden[f"{case}/{tag}_efc_type"], golden[f"{case}/{tag}_counters"][:, 1]
    return {int(x) & 0xff for e in range(len(n)) for x in t[e, : n[e]]}


def test_fixture_covers_what_the_cases_are_for(golden):
    """The recorded cases hold what they were chosen for: joint limits, the hamstring tendon limit and contacts on the humanoid; row and
    contact drops under the small caps; more items than lanes on the drone and the 64-dof chain; both sides of one limit."""
    assert {0, 1, 3} <= _types(golden, "humanoid", "start") | _types(golden, "humanoid", "end")
    caps = golden["humanoid_caps/roll_counters"]
    assert (caps[:, 3] > 0).any() and (caps[:, 4] > 0).any() and golden["humanoid_caps/start_counters"][:, 3:5].sum() > 0
    assert golden["drone2_drop/end_counters"][:, 0].min() >= 4                    # the drone rests on the floor
    assert golden["drone2_flipped/start_counters"][:, 0].max() + 1 > 16          # contacts + the free joint's limit object > G = 16 lanes
    assert 0 in _types(golden, "cartpole_limit", "end")
    both = golden["both_sides/start_efc_J"][:, :2].view(np.float32)               # nv = 1: lower side (+1), then upper side (-1)
    assert (golden["both_sides/start_counters"][:, 1] == 2).all() and (both == [1.0, -1.0]).all()
    assert 64 + golden["chain64/start_counters"][:, 0].min() > 64                  # 64 limit objects + contacts > 64 lanes
    assert 1 in _types(golden, "tree", "start") | _types(golden, "tree", "end")


@pytest.mark.parametrize("variant", rows_bits.VARIANTS)
@pytest.mark.parametrize("case", list(rows_bits.CASES))
def test_rows_and_rollout_bits_match_the_recorded_build(golden, device_models, case, variant):
    got = rows_bits.run_case(case, variant, device_models(rows_bits.CASES[case]["model"]))
    if got is None:
        assert variant == "two"                                                    # no two-wave kernel for this model: nothing to compare
        return
    for key, arr in got.items():
        want = golden[key]
        assert arr.dtype == want.dtype and arr.shape == want.shape, key
        assert arr.tobytes() == want.tobytes(), f"{key}: {int((arr != want).sum())} of {arr.size} words differ"
