"""Cost of per-environment model parameters: humanoid B = 4096, fp32, 1000-step random-ctrl rollouts with no field batched and with
all nine batched (``BatchSim.set_env_params``, every row a different draw), each through its specialised step kernel.  The two data
objects take turns for --rounds windows (alternated, after a warm-up of both); each window is one 1000-step launch from the same
standing state, timed on the host clock around a device synchronise.  Reports the median env-steps/s of each and their ratio.

    python scripts/gpu_model_params_timing.py [--batch 4096] [--steps 1000] [--rounds 5] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mujoco_template_amd import mjcf  # noqa: E402
from mujoco_template_amd._capi import CTRL_RANDOM, ENV_PARAM_FIELDS, BatchSim, DeviceModel  # noqa: E402


def params(cm, B, seed=0):
    rng = np.random.default_rng(seed)
    out = {}
    for k in ENV_PARAM_FIELDS:
        own = np.array(cm.gravity if k == "gravity" else cm.arrays[k], dtype=np.float64)
        v = np.broadcast_to(own, (B, *own.shape)).copy()
        if k == "gravity":
            v[:, 2] = rng.uniform(-11.0, -8.5, B)
        elif k == "geom_friction":
            v[..., 0] = rng.uniform(0.5, 1.5, v.shape[:-1])
        else:
            v *= rng.uniform(0.8, 1.2, v.shape)
        out[k] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cm = mjcf.compile_xml_path(os.path.join(ROOT, "models", "humanoid.xml"))
    dm = DeviceModel(cm)
    key = cm.name2id(mjcf.OBJ_KEY, "stand_on_left_leg")
    sims = {"none": BatchSim(dm, args.batch, dtype="float32"), "all9": BatchSim(dm, args.batch, dtype="float32")}
    sims["all9"].set_env_params(**params(cm, args.batch))
    for s in sims.values():
        assert s.specialized, "the specialised kernel is what is measured"

    def window(sim):
        sim.reset(key)
        sim.sync()
        t0 = time.perf_counter()
        sim.rollout(args.steps, CTRL_RANDOM, seed=1, ctrl_scale=0.3)
        sim.sync()
        return args.batch * args.steps / (time.perf_counter() - t0)

    for s in sims.values():                                    # warm-up
        window(s)
    rates = {k: [] for k in sims}
    for _ in range(args.rounds):
        for k, s in sims.items():
            rates[k].append(window(s))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    res = {"workload": f"humanoid B={args.batch} fp32, {args.steps}-step random-ctrl rollout, specialised kernel",
           "env_steps_per_s_median": med, "all_windows": rates, "cost_all9_vs_none": 1.0 - med["all9"] / med["none"],
           "map": sims["none"].schedule_info()["map"]}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
