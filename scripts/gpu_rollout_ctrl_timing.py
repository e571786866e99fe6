"""Open-loop rollouts from a control tensor, three ways, in ONE process and alternated:

  seq       ``BatchSim.rollout_ctrl`` - the whole [B, T, nu] control tensor in one launch (``mjb_rollout_ctrl``);
  loop      the per-step torch loop - ``DeviceData.ctrl.copy_(u[:, t])`` + ``step(1)``, one launch per step;
  random    ``mjb_rollout(MJB_CTRL_RANDOM)`` - the fused ceiling (controls made inside the kernel).

Workloads (fp32, T = 100 steps per rollout): humanoid B = 4096, cart-pole B = 1024, humanoid B = 512 (two-wave kernel).  Every number:
env-steps/s from the host clock around a window that ends in a device synchronise, after a warm-up of every shape; the three ways take
turns for --rounds rounds and the median is reported with the min..max spread.

    python scripts/gpu_rollout_ctrl_timing.py [--steps 100] [--rounds 5] [--min-seconds 0.5] [--out FILE.json]
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

from mujoco_template_amd._capi import CTRL_RANDOM, BatchSim, DeviceModel  # noqa: E402
from mujoco_template_amd.mjcf import compile_xml_path  # noqa: E402

WORKLOADS = [("humanoid", 4096), ("cartpole", 1024), ("humanoid", 512)]


def make(name, B):
    dm = DeviceModel(compile_xml_path(os.path.join(ROOT, "models", f"{name}.xml")))
    sim = BatchSim(dm, B, dtype="float32")
    sim.use_torch_stream()
    return sim, dm.compiled.nu


def run_way(way, sim, u, T, ctrl_view):
    if way == "seq":
        sim.rollout_ctrl(T, u)
    elif way == "loop":
        for t in range(T):
            ctrl_view.copy_(u[:, t])
            sim.step(1)
    else:
        sim.rollout(T, CTRL_RANDOM, seed=1, ctrl_scale=0.1)


def timed(way, sim, u, T, ctrl_view, min_seconds):
    """env-steps/s of repeated rollouts from the current state (reset between windows keeps the state physical)."""
    n = 0
    sim.reset(-1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while True:
        run_way(way, sim, u, T, ctrl_view)
        n += 1
        if n % 4 == 0:
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= min_seconds:
                return n * T * sim.batch / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures the MI355X and has no CPU fallback")
    T = args.steps
    results = []
    for name, B in WORKLOADS:
        sim, nu = make(name, B)
        g = torch.Generator(device="cuda").manual_seed(0)
        u = (torch.rand((B, T, nu), device="cuda", generator=g) * 2 - 1) * 0.1   # small controls: the humanoid stays physical over a window
        ctrl_view = sim.torch_view("ctrl")
        for way in ("seq", "loop", "random"):                                       # warm-up of every shape (code objects, allocator)
            run_way(way, sim, u, T, ctrl_view)
        torch.cuda.synchronize()
        rates = {w: [] for w in ("seq", "loop", "random")}
        for _ in range(args.rounds):
            for way in rates:
                rates[way].append(timed(way, sim, u, T, ctrl_view, args.min_seconds))
        sim.rollout_ctrl(T, u)
        sim.sync()
        seq_info = sim.schedule_info()
        row = {"model": name, "batch": B, "steps": T, "seq_schedule": seq_info,
               **{f"{w}_Msteps_per_s": {"median": float(np.median(r)) / 1e6, "min": min(r) / 1e6, "max": max(r) / 1e6} for w, r in rates.items()}}
        row["seq_over_loop"] = row["seq_Msteps_per_s"]["median"] / row["loop_Msteps_per_s"]["median"]
        row["seq_over_random"] = row["seq_Msteps_per_s"]["median"] / row["random_Msteps_per_s"]["median"]
        results.append(row)
        print(json.dumps(row), flush=True)
        del sim
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
