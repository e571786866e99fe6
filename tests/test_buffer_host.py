"""The two owner types of the C ABI's device / pinned memory (``csrc/mjb_buffer.hpp``) without a GPU: ``tests/buffer_host.cpp`` is a
stand-alone program that supplies the four allocator entry points itself (over malloc / free, with a table of the live blocks) and
runs under AddressSanitizer and UndefinedBehaviorSanitizer as a child process."""

from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_buffer_and_arena_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "buffer_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__", "-Wno-unused-result",
                           "-I" + HIP_INCLUDE, "-o", exe, os.path.join(HERE, "buffer_host.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr                       # a sanitizer report goes to stderr, whatever the exit status
    assert run.stdout.strip() == "buffer_host: ok"


def test_only_the_c_abi_translation_unit_depends_on_the_header():
    """The header has no device code and the kernel translation units do not see it (their dependency list is HDRS)."""
    csrc = os.path.join(ROOT, "mujoco_template_amd", "csrc")
    text = open(os.path.join(csrc, "mjb_buffer.hpp")).read()
    assert "__device__" not in text.replace("no __device__", "") and "__global__" not in text
    assert [ln for ln in text.splitlines() if ln.startswith("#include <hip")] == ["#include <hip/hip_runtime_api.h>"]
    make = open(os.path.join(csrc, "Makefile")).read()
    hdrs = next(ln for ln in make.splitlines() if ln.startswith("HDRS ="))
    assert "mjb_buffer.hpp" not in hdrs
    assert "build/mjb_api.o build/prof_mjb_api.o: mjb_buffer.hpp" in make
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".hpp", ".cpp")) and name not in ("mjb_api.hip", "mjb_buffer.hpp"):
            assert "mjb_buffer.hpp" not in open(os.path.join(csrc, name)).read(), name
