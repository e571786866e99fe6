"""The C-ABI shared library: loads, exports every symbol include/mjbatch.h declares, rejects bad
model tables, and fails loudly (no CPU fallback) when no HIP device is present.  CPU only: no compute calls."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "mujoco_template_amd", "libmjbatch.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):
        import __graft_entry__ as g

        g.build()
    import torch  # noqa: F401  (shares one HIP runtime with the library, see _capi.load_library)

    return ctypes.CDLL(SO)


def test_every_declared_symbol_is_exported(lib):
    header = open(os.path.join(ROOT, "include", "mjbatch.h")).read()
    names = sorted(set(re.findall(r"\b(mjb_[a-z_0-9]+)\s*\(", header)))
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), n


def test_header_cites_reference_call_sites():
    header = open(os.path.join(ROOT, "include", "mjbatch.h")).read()
    for cite in ("model.py:56-57", "model.py:53-54", "linearization.py:16-35", "jacobians.py:44-79", "observations.py:98-174", "runtime.py:631-663"):
        assert cite in header


def test_model_create_validates_table(lib, compiled):
    from mujoco_template_amd._pack import PackedTable

    lib.mjb_last_error.restype = ctypes.c_char_p
    p = PackedTable(compiled("cartpole"))
    out = ctypes.c_void_p()
    rc = lib.mjb_model_create(p.n, p.names, p.ptrs, p.dtypes, p.counts, ctypes.byref(out))
    assert rc == 0 and out.value
    lib.mjb_model_free(out)
    # truncated table -> loud failure naming the missing field
    rc = lib.mjb_model_create(20, p.names, p.ptrs, p.dtypes, p.counts, ctypes.byref(out))
    assert rc == -2 and b"missing" in lib.mjb_last_error()


def test_no_cpu_fallback(compiled):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mujoco_template_amd import Env, TemplateError
    from tests.conftest import MODELS

    with pytest.raises(TemplateError, match="no HIP device"):
        Env.from_xml_path(MODELS["pendulum"])


def test_product_package_does_not_import_oracle():
    pkg = os.path.join(ROOT, "mujoco_template_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "from oracle" not in text and "import oracle" not in text and "mjo_" not in text, f


def test_specialised_kernel_source_and_cross_compile():
    """Per-model specialisation (include/mjbatch.h mjb_model_kernel_source): the generated translation unit pins the model's
    structural sizes and LDS offsets - never the run-time options - and cross-compiles for gfx950 without a GPU."""
    import torch  # noqa: F401  (one HIP runtime per process: torch first)

    from mujoco_template_amd import mjcf
    from mujoco_template_amd._capi import DeviceModel, compile_spec
    from tests.conftest import MODELS

    dm = DeviceModel(mjcf.compile_xml_path(MODELS["cartpole"]))
    src = dm.spec_source()
    assert "#define MJB_SPEC_G 8" in src and "(m).nv == 2" in src and "(m).nbody == 3" in src and "(L).qpos == 0" in src
    for runtime_option in ("disableactuator", "iterations", "tolerance", "timestep"):
        assert runtime_option not in src
    assert dm.spec_source(nefcmax=12, nconmax=3) != src and "(m).nefc_max == 12" in dm.spec_source(nefcmax=12, nconmax=3)
    path = compile_spec(src)
    blob = open(path, "rb").read()
    assert (blob[:4] == b"\x7fELF" or blob.startswith(b"__CLANG_OFFLOAD_BUNDLE__")) and b"mjb_k_step_spec" in blob and b"gfx950" in blob
    assert compile_spec(src) == path                      # cached


def test_model_level_kernel_source_rejects_what_data_create_rejects():
    """The model-level kernel sources derive the launch configuration in the same function as mjb_data_create: caps whose
    per-workgroup LDS slice cannot fit are refused with mjb_data_create's error, and the two-wave kernel does not apply where its
    flat layout exceeds 64 KiB, instead of yielding sources no data object will ever ask for."""
    import torch  # noqa: F401

    from mujoco_template_amd import mjcf
    from mujoco_template_amd._capi import DeviceModel
    from mujoco_template_amd.exceptions import ConfigError
    from tests.conftest import MODELS

    dm = DeviceModel(mjcf.compile_xml_path(MODELS["humanoid"]))
    for source in (dm.spec_source, dm.fd_spec_source, dm.step2_spec_source):
        assert source(lanes=64, nconmax=64, nefcmax=256) is not None
    for source in (dm.spec_source, dm.fd_spec_source):
        with pytest.raises(ConfigError, match="exceeds 160 KiB"):
            source(lanes=8, nconmax=64, nefcmax=256)          # eight environments of 49 KB each in one workgroup
    assert dm.step2_spec_source(lanes=8, nconmax=64, nefcmax=256) is None
    assert "(m).nefc_max == 384" in dm.spec_source(lanes=64, nconmax=96, nefcmax=384)
    assert dm.step2_spec_source(lanes=64, nconmax=96, nefcmax=384) is None             # flat layout above 64 KiB


def test_specialised_kernel_drops_powf_only_when_the_model_allows_it():
    """The impedance curve of a constraint row needs powf only for a solimp power other than 1 or 2 (2 is MuJoCo's default).  The
    generated translation unit says so (MJB_SPEC_SOLIMP_POWER_1_OR_2) exactly when every joint-limit, tendon-limit and contact-pair
    power of the model qualifies - the device code is then compiled without the library's powf, ~2 000 instructions of a branch
    that is never taken; a model with power 3 keeps it."""
    import torch  # noqa: F401

    from mujoco_template_amd import mjcf
    from mujoco_template_amd._capi import DeviceModel
    from tests.conftest import BASE_XML, MODELS

    for name in ("humanoid", "cartpole", "drone2", "pendulum"):
        assert "#define MJB_SPEC_SOLIMP_POWER_1_OR_2 1" in DeviceModel(mjcf.compile_xml_path(MODELS[name])).spec_source(), name
    assert "MJB_SPEC_SOLIMP_POWER_1_OR_2" in DeviceModel(mjcf.compile_xml_string(BASE_XML)).spec_source()
    cubic = BASE_XML.replace('<joint limited="true" range="-1 1"/>', '<joint limited="true" range="-1 1" solimplimit="0.9 0.95 0.001 0.5 3"/>')
    assert cubic != BASE_XML
    assert "MJB_SPEC_SOLIMP_POWER_1_OR_2" not in DeviceModel(mjcf.compile_xml_string(cubic)).spec_source()


def test_spec_scheduler_rule_and_private_cache(tmp_path, monkeypatch):
    """VERDICT r1 #7 / ADVICE r1: the scheduler of the specialised kernel follows a stated rule (iterative ILP for every model
    with a constraint-row cap >= 8 or one wave per environment; ROCm 7.2.0's clang crashes with it on the degenerate BASE_XML kernel,
    profiles/r02_hipcc_iterative_ilp_crash.txt), and the fallback cache of a read-only install is private."""
    import stat

    import torch  # noqa: F401

    from mujoco_template_amd import _capi, mjcf
    from mujoco_template_amd._capi import DeviceModel, compile_spec, spec_scheduler
    from tests.conftest import BASE_XML, MODELS

    for name in ("humanoid", "drone2", "cartpole"):               # models with real constraint rows: the scheduler that was measured to pay
        assert spec_scheduler(DeviceModel(mjcf.compile_xml_path(MODELS[name])).spec_source()) == "iterative-ilp"
    assert spec_scheduler(DeviceModel(mjcf.compile_xml_path(MODELS["pendulum"])).spec_source()) is None     # 2 rows at most: tiny kernel
    # the specialised translation units carry the model itself (tables + DevModel image) and the float64 / two-wave variants exist
    hum = DeviceModel(mjcf.compile_xml_path(MODELS["humanoid"]))
    for src, kind, ctype in ((hum.spec_source(), 1, "float"), (hum.fd_spec_source(), 2, "double"), (hum.step2_spec_source(), 3, "float")):
        assert f"#define MJB_SPEC_KERNEL {kind}" in src and "#define MJB_SPEC_BAKED" in src and f"static const __constant__ {ctype} mjb_tab_" in src
        assert "not baked" not in src
    assert DeviceModel(mjcf.compile_xml_path(MODELS["cartpole"])).step2_spec_source() is None            # packed kernels: one wave per several environments
    base_src = DeviceModel(mjcf.compile_xml_string(BASE_XML)).spec_source()
    assert "#define MJB_SPEC_G 8" in base_src and spec_scheduler(base_src) is None
    assert os.path.exists(compile_spec(base_src))                 # the crashing case compiles under the rule (cross-compile only)
    # read-only install: the cache moves to a 0700 directory under the user's cache home; a planted world-writable one is refused
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path))
    d = _capi._private_cache_dir()
    assert d.startswith(str(tmp_path)) and stat.S_IMODE(os.lstat(d).st_mode) == 0o700
    os.chmod(d, 0o777)
    with pytest.raises(_capi.TemplateError, match="refusing"):
        _capi._private_cache_dir()
    os.chmod(d, 0o700)
    planted = os.path.join(d, "k_step_spec_x.hsaco")
    with open(planted, "wb") as fh:
        fh.write(b"x")
    os.chmod(planted, 0o666)
    with pytest.raises(_capi.TemplateError, match="refusing"):
        _capi._read_private(planted)
    link = os.path.join(d, "link.hsaco")
    os.symlink(planted, link)
    with pytest.raises(OSError):
        _capi._read_private(link)
