"""Predictive sampling on the cart-pole with ``mujoco_template_amd.rollout``: the open-loop rollout API end to end.

Every control step, K noisy control sequences around the nominal plan (sample 0 is the plan itself) are rolled out over H steps from
the current state of the controlled system in ONE launch; a torch cost over the returned states picks the best sequence; its first
control is applied to the system (a separate one-environment data object) and the plan shifts by one step.  The pole starts tilted by
--tilt rad; the script reports whether it stays up (|hinge| < 0.5 rad throughout) and the tilt over the last second.

    python scripts/gpu_predictive_sampling.py [--samples 256] [--horizon 50] [--steps 300] [--tilt 0.2] [--out FILE.json]
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

from mujoco_template_amd import mj, rollout  # noqa: E402

XML = os.path.join(ROOT, "models", "cartpole.xml")
U_MAX = 2.0          # |ctrl| used by the planner (gear 50: 100 N on a ~5 kg cart)


def cost(state: torch.Tensor, ctrl: torch.Tensor) -> torch.Tensor:
    """[K] cost of [K, H, 1 + nq + nv] states (time, slider, hinge, slider vel, hinge vel) under [K, H, nu] controls."""
    x, th, xd, thd = state[..., 1], state[..., 2], state[..., 3], state[..., 4]
    run = 10.0 * th ** 2 + 0.5 * x ** 2 + 0.1 * thd ** 2 + 0.05 * xd ** 2 + 0.01 * ctrl[..., 0] ** 2
    return run.sum(dim=1) + 20.0 * (th[:, -1] ** 2 + 0.1 * thd[:, -1] ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--tilt", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the planner's rollouts run on the MI355X")
    K, H = args.samples, args.horizon
    model = mj.MjModel.from_xml_path(XML)
    plant = mj.MjData(model, batch=1, dtype="float64")                         # the controlled system
    planner = mj.MjData(model, batch=K, dtype="float32")                       # K sampled futures per control step
    plant.qpos[1] = args.tilt
    mj.mj_forward(model, plant)
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    plan = torch.zeros((H, model.nu), device="cuda")
    hinge, t0 = [], time.perf_counter()
    for _ in range(args.steps):
        x0 = np.concatenate([[plant.time], np.ravel(plant.qpos), np.ravel(plant.qvel)])
        noise = torch.randn((K, H, model.nu), device="cuda", generator=g) * args.sigma
        noise[0] = 0                                                           # keep the nominal plan among the candidates
        u = (plan.unsqueeze(0) + noise).clamp_(-U_MAX, U_MAX)
        state, _ = rollout(model, planner, u, initial_state=x0)
        best = int(torch.argmin(cost(state, u)))
        plan = torch.cat([u[best, 1:], u[best, -1:]])                          # shift: the tail repeats the last control
        plant.ctrl[:] = float(u[best, 0, 0])
        mj.mj_step(model, plant)
        hinge.append(float(np.ravel(plant.qpos)[1]))
    wall = time.perf_counter() - t0
    h = np.abs(np.array(hinge))
    last = h[-int(round(1.0 / model.opt.timestep)):]
    res = {"samples": K, "horizon": H, "control_steps": args.steps, "tilt0_rad": args.tilt, "max_abs_hinge_rad": float(h.max()),
           "last_second_max_abs_hinge_rad": float(last.max()), "stays_up": bool(h.max() < 0.5),
           "final_slider_m": float(np.ravel(plant.qpos)[0]), "wall_s": wall, "planner_env_steps_per_s": K * H * args.steps / wall}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
