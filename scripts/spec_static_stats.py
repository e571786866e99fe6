"""Static side of the specialised kernels of the shipped models: for every (model, kernel kind) the code object that
``compile_spec`` builds for this tree, read with the LLVM tools of ROCm - no GPU needed.

    python scripts/spec_static_stats.py [--out stats.json]

Per kernel: instructions, VALU / SALU instructions, v_div_fixup (one per correctly rounded division), global / scalar loads
(model tables are read with both; the state in HBM only at the ends of a launch), code length in bytes, VGPRs, SGPRs, scratch per
lane and LDS of the kernel descriptor.  Run it in two checkouts to compare two revisions."""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = ("humanoid.xml", "cartpole.xml", "pendulum.xml", os.path.join("drone2", "scene.xml"))


def _tool(name: str) -> str:
    for cand in (shutil.which(name), f"/opt/rocm/llvm/bin/{name}", f"/opt/rocm/lib/llvm/bin/{name}"):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit(f"{name} not found")


def stats(bundle: str) -> dict:
    import tempfile

    # hipcc --genco writes an offload bundle: take the gfx950 code object out of it
    with tempfile.TemporaryDirectory() as tmp:
        hsaco = os.path.join(tmp, "k.co")
        subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={bundle}",
                        f"--output={hsaco}"], check=True)
        return _stats(hsaco)


def _stats(hsaco: str) -> dict:
    dis = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", hsaco], capture_output=True, text=True, check=True).stdout
    ops = [ln.split()[0] for ln in dis.splitlines() if ln.startswith("\t") and ln.split()]
    note = subprocess.run([_tool("llvm-readelf"), "--notes", hsaco], capture_output=True, text=True, check=True).stdout
    size = subprocess.run([_tool("llvm-readelf"), "-S", "-W", hsaco], capture_output=True, text=True, check=True).stdout
    text = re.search(r"\.text\s+PROGBITS\s+\S+\s+\S+\s+([0-9a-f]+)", size)

    def meta(key: str) -> int:
        m = re.search(rf"\.{key}:\s+(\d+)", note)
        return int(m.group(1)) if m else -1

    return {
        "instructions": len(ops),
        "valu": sum(o.startswith("v_") for o in ops),
        "salu": sum(o.startswith("s_") and not o.startswith(("s_load", "s_buffer_load", "s_waitcnt", "s_nop", "s_barrier")) for o in ops),
        "v_div_fixup": sum(o.startswith("v_div_fixup") for o in ops),
        "global_load": sum(o.startswith("global_load") for o in ops),
        "scalar_load": sum(o.startswith(("s_load", "s_buffer_load")) for o in ops),
        "scratch_ops": sum(o.startswith("scratch_") for o in ops),
        "code_bytes": int(text.group(1), 16) if text else -1,
        "vgprs": meta("vgpr_count"),
        "sgprs": meta("sgpr_count"),
        "scratch_bytes_per_lane": meta("private_segment_fixed_size"),
        "lds_bytes": meta("group_segment_fixed_size"),
    }


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mujoco_template_amd._capi import DeviceModel, compile_spec
    from mujoco_template_amd.mjcf import compile_xml_path

    res = {}
    for name in MODELS:
        dm = DeviceModel(compile_xml_path(os.path.join(ROOT, "models", name)))
        for kind, src in (("step", dm.spec_source()), ("step2", dm.step2_spec_source()), ("fd", dm.fd_spec_source())):
            if src is None:
                continue
            res[f"{os.path.splitext(os.path.basename(name))[0]}/{kind}"] = stats(compile_spec(src))
    for k, v in res.items():
        print(k, json.dumps(v))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
