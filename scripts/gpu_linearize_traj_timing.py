"""Linearising a whole trajectory: ``linearize_rollout`` (two submissions: the rollout launch, then ``mjb_transition_fd_points`` over its
T x B points) against the per-step host loop that was the only way before it,

    for t: data.ctrl <- u[:, t];  (A_t, B_t) <- transition_fd();  step(1)

(T synchronisations, T pinned host results), in ONE process and alternated.  Humanoid, float32 data, (B, T) in (1, 100), (1, 500),
(16, 100), (512, 8).  Every number: after a warm-up of both ways, the median (min..max) of --rounds alternated windows, HIP-event time
and host wall time around a window that ends in a device synchronise.  ``--profile-shape B,T`` runs each way once for that shape and
nothing else (for a ``rocprofv3 --kernel-trace --stats`` run of its own).

    python scripts/gpu_linearize_traj_timing.py [--rounds 5] [--out FILE.json]
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

from mujoco_template_amd import linearize_rollout, mj  # noqa: E402

SHAPES = [(1, 100), (1, 500), (16, 100), (512, 8)]


def host_loop(sim, ctrl_view, u, T):
    out = None
    for t in range(T):
        ctrl_view.copy_(u[:, t])
        out = sim.transition_fd(1e-6, True, copy=False)
        sim.step(1)
    return out


def window(fn):
    """(HIP-event ms, wall ms, ms until fn returned) of one call of fn, ended by a device synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    t1 = time.perf_counter()                                       # the call has returned: everything is enqueued, nothing waited for
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile-shape", default=None, help="B,T: run each way once for this shape only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures the MI355X and has no CPU fallback")
    model = mj.MjModel.from_xml_path(os.path.join(ROOT, "models", "humanoid.xml"))
    shapes = [tuple(int(x) for x in args.profile_shape.split(","))] if args.profile_shape else SHAPES
    results = []
    for B, T in shapes:
        fused, loop = mj.MjData(model, batch=B, dtype="float32"), mj.MjData(model, batch=B, dtype="float32")
        g = torch.Generator(device="cuda").manual_seed(0)
        u = (torch.rand((B, T, model.nu), device="cuda", generator=g) * 2 - 1) * 0.3
        x0 = torch.cat([torch.zeros(1), torch.as_tensor(np.ravel(model.compiled.qpos0)), torch.zeros(model.nv)]).double()
        loop.sim.use_torch_stream()
        ctrl_view = loop.sim.torch_view("ctrl")

        def run_fused():
            return linearize_rollout(model, fused, u, initial_state=x0)

        def run_loop():
            loop.sim.reset(-1)
            return host_loop(loop.sim, ctrl_view, u, T)

        ways = {"linearize_rollout": run_fused, "host_loop": run_loop}
        for fn in ways.values():                                    # warm-up: code objects, scratch, allocator
            fn()
        torch.cuda.synchronize()
        if args.profile_shape:
            continue
        ms = {w: [] for w in ways}
        for _ in range(args.rounds):
            for w, fn in ways.items():
                ms[w].append(window(fn))
        row = {"model": "humanoid", "dtype": "float32", "batch": B, "steps": T, "points": B * T, "fd_slabs": fused.sim.fd_points_slabs()}
        for w, v in ms.items():
            ev, wall, ret = np.array(v).T
            row[w] = {"returns_after_ms": float(np.median(ret)), "event_ms": {"median": float(np.median(ev)), "min": float(ev.min()), "max": float(ev.max())},
                      "wall_ms": {"median": float(np.median(wall)), "min": float(wall.min()), "max": float(wall.max())}}
        row["loop_over_fused_wall"] = row["host_loop"]["wall_ms"]["median"] / row["linearize_rollout"]["wall_ms"]["median"]
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out and results:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
