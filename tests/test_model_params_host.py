"""Per-environment model parameters, the parts that need no GPU: the oracle helper's derivation against the MJCF compiler, the
specialised kernel sources with and without batched fields, the all-fields kernel cross-compiled for gfx950, and the sharded slice."""
import os
import re
import subprocess

import numpy as np
import pytest

from mujoco_template_amd import mjcf
from mujoco_template_amd._capi import ENV_PARAM_FIELDS, DeviceModel, compile_spec, env_param_shape
from mujoco_template_amd.distributed import ShardPlan
from tests.conftest import MODELS
from tests.model_params_oracle import FIELDS, env_compiled


def _humanoid_xml():
    with open(MODELS["humanoid"]) as f:
        return f.read()


def test_helper_fields_follow_the_library_order():
    assert FIELDS == ENV_PARAM_FIELDS


def test_helper_derivation_matches_the_compiler():
    """Edit one body's mass (an explicit geom mass) and one geom's friction in the humanoid's XML: the compiled body_subtreemass and
    pair_friction equal what the helper derives from the UNEDITED model given the edited body_mass / geom_friction."""
    xml = _humanoid_xml()
    base = mjcf.compile_xml_string(xml, os.path.dirname(MODELS["humanoid"]))
    m = re.search(r'<geom name="(thigh_right)"([^>]*)/>', xml)
    assert m, "humanoid.xml: the right thigh's geom"
    edited = xml.replace(m.group(0), f'<geom name="thigh_right" mass="7.25" friction="1.3 0.02 0.0004"{m.group(2)}/>')
    cm = mjcf.compile_xml_string(edited, os.path.dirname(MODELS["humanoid"]))
    assert not np.array_equal(cm.arrays["body_mass"], base.arrays["body_mass"])
    assert not np.array_equal(cm.arrays["geom_friction"], base.arrays["geom_friction"])
    c = env_compiled(base, body_mass=cm.arrays["body_mass"], geom_friction=cm.arrays["geom_friction"])
    assert np.array_equal(c.arrays["body_subtreemass"], cm.arrays["body_subtreemass"])
    assert np.array_equal(c.arrays["pair_friction"], cm.arrays["pair_friction"])
    assert not np.array_equal(c.arrays["pair_friction"], base.arrays["pair_friction"])
    # the unedited model is a fixed point of the derivation
    b2 = env_compiled(base)
    assert np.array_equal(b2.arrays["body_subtreemass"], base.arrays["body_subtreemass"])
    assert np.array_equal(b2.arrays["pair_friction"], base.arrays["pair_friction"])


def test_param_shapes():
    cm = mjcf.compile_xml_path(MODELS["humanoid"])
    for name in ENV_PARAM_FIELDS:
        want = (3,) if name == "gravity" else np.shape(cm.arrays[name])
        assert env_param_shape(cm, name) == tuple(want), name


@pytest.fixture(scope="module")
def humanoid_dm():
    return DeviceModel(mjcf.compile_xml_path(MODELS["humanoid"]))


def test_spec_source_empty_mask_unchanged(humanoid_dm):
    dm = humanoid_dm
    assert dm.spec_source(params=()) == dm.spec_source()
    assert dm.fd_spec_source(params=()) == dm.fd_spec_source()
    assert dm.step2_spec_source(params=()) == dm.step2_spec_source()
    assert "MJB_SPEC_PARAMS" not in dm.spec_source()
    full = dm.spec_source(params=ENV_PARAM_FIELDS)
    assert full != dm.spec_source()
    assert "#define MJB_SPEC_PARAMS 511" in full
    assert "mjb_spec_params = 511" in full
    one = dm.spec_source(params=("gravity",))
    assert "#define MJB_SPEC_PARAMS 256" in one
    with pytest.raises(Exception):
        dm.spec_source(params=("geom_size",))


def test_spec_source_batched_damping_takes_the_damping_path():
    """A model without damping: its kernel assumes has_damping == 0 until dof_damping is batched, then == 1 (and the baked image too)."""
    dm = DeviceModel(mjcf.compile_xml_path(MODELS["pendulum"]))
    cm = dm.compiled
    assert not np.any(np.asarray(cm.arrays["dof_damping"]) > 0)
    plain, damped = dm.spec_source(), dm.spec_source(params=("dof_damping",))
    assert "(m).has_damping == 0" in plain and "(m).has_damping == 1" in damped
    assert "(m).has_damping == 1" in dm.spec_source(params=ENV_PARAM_FIELDS)
    assert "(m).has_damping == 0" in dm.spec_source(params=("body_mass",))


def _readelf_notes(co: str) -> str:
    elf = co + ".elf"
    bundler = "/opt/rocm/llvm/bin/clang-offload-bundler"
    with open(co, "rb") as f:
        head = f.read(4)
    if head == b"\x7fELF":
        elf = co
    else:
        subprocess.check_call([bundler, "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={co}", f"--output={elf}", "--unbundle"])
    return subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", elf], capture_output=True, text=True, check=True).stdout


def _meta(notes: str, key: str) -> int:
    m = re.search(r"\.%s:\s+(\d+)" % re.escape(key), notes)
    assert m, key
    return int(m.group(1))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_all_fields_kernel_compiles(humanoid_dm):
    """humanoid's specialised step kernel with every field batched builds for gfx950 with the LDS (group segment) of the mask-0
    build; VGPR / scratch of both are printed (the PR reports them)."""
    plain = _readelf_notes(compile_spec(humanoid_dm.spec_source()))
    full = _readelf_notes(compile_spec(humanoid_dm.spec_source(params=ENV_PARAM_FIELDS)))
    assert _meta(full, "group_segment_fixed_size") == _meta(plain, "group_segment_fixed_size")
    for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size"):
        print(f"{k}: mask 0 {_meta(plain, k)}, all fields {_meta(full, k)}")
    assert _meta(full, "vgpr_count") <= 256


@pytest.mark.parametrize("world", [2, 3])
def test_shard_slices_global_params(world):
    G = 10
    glob = np.arange(G * 3, dtype=np.float64).reshape(G, 3)
    got = []
    for rank in range(world):
        plan = ShardPlan.from_environment(G, rank=rank, world_size=world, local_rank=rank)
        blk = plan.local_rows(glob, (3,))
        assert blk.shape == (plan.count, 3)
        assert np.array_equal(blk, glob[plan.env0:plan.env0 + plan.count])
        one = glob[0]
        assert plan.local_rows(one, (3,)) is one                    # one value for every environment: passed through
        got.append(blk)
    assert np.array_equal(np.concatenate(got), glob)
    with pytest.raises(ValueError):
        ShardPlan.from_environment(G, rank=0, world_size=world, local_rank=0).local_rows(glob[:5], (3,))
