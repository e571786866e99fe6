"""Device-resident control loop (torch controller on DeviceData, Env.step on the GPU state) next to the host-driven loop and the fused
rollout, in ONE process: humanoid, B = 4096, fp32.

    python scripts/gpu_device_loop.py [--batch 4096] [--min-seconds 0.5] [--out profiles/device_loop_<tag>.log]
    python scripts/gpu_device_loop.py --loops random --fixed-steps 200 --no-log     (the shape to run under rocprofv3 --kernel-trace)

Loops: (a) ``random``  torch uniform ctrl written in place, (b) ``mlp``  a 2 x 64 tanh MLP policy on [qpos, qvel], (c) ``reset``
random ctrl with ``reset_done=True`` and a torso-height done_fn; ``host``  the reference-shaped host loop (numpy controller, state
block over PCIe every step), ``fused``  the one-launch rollout (RandomCtrlController, 20 steps per launch).  Every number: env-steps/s
from the host clock around a synchronised window of at least --min-seconds after a warm-up.
"""
from __future__ import annotations

import argparse
import datetime
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mujoco_template_amd as mt  # noqa: E402

XML = os.path.join(ROOT, "models", "humanoid.xml")


class TorchRandom:
    device_arrays = True

    def __init__(self, seed=0):
        self.capabilities = mt.ControllerCapabilities()
        self.gen = None
        self.seed = seed

    def prepare(self, model, data):
        pass

    def __call__(self, model, data, t):
        if self.gen is None:
            self.gen = torch.Generator(device=data.device).manual_seed(self.seed)
        data.ctrl.uniform_(-1.0, 1.0, generator=self.gen)


class TorchMLP:
    device_arrays = True

    def __init__(self, nq, nv, nu, hidden=64, seed=0):
        self.capabilities = mt.ControllerCapabilities()
        g = torch.Generator().manual_seed(seed)
        self.net = torch.nn.Sequential(torch.nn.Linear(nq + nv, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, hidden), torch.nn.Tanh(),
                                       torch.nn.Linear(hidden, nu), torch.nn.Tanh())
        with torch.no_grad():
            for p in self.net.parameters():
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
        self.moved = False

    def prepare(self, model, data):
        pass

    @torch.no_grad()
    def __call__(self, model, data, t):
        if not self.moved:
            self.net = self.net.to(device=data.device, dtype=data.qpos.dtype)
            self.moved = True
        data.ctrl.copy_(self.net(torch.cat([data.qpos, data.qvel], dim=1)))


class HostRandom:
    def __init__(self, seed=0):
        self.capabilities = mt.ControllerCapabilities()
        self.rng = np.random.default_rng(seed)

    def prepare(self, model, data):
        pass

    def __call__(self, model, data, t):
        data.ctrl[...] = self.rng.uniform(-1.0, 1.0, np.shape(data.ctrl))


def timed(step_fn, batch, warmup, min_seconds, fixed_steps=0, chunk=50):
    """env-steps/s from the host clock around a synchronised window (>= min_seconds, or exactly fixed_steps steps)."""
    for _ in range(warmup):
        step_fn()
    torch.cuda.synchronize()
    n = 0
    t0 = time.perf_counter()
    while True:
        for _ in range(chunk if not fixed_steps else fixed_steps):
            step_fn()
        n += chunk if not fixed_steps else fixed_steps
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if fixed_steps or dt >= min_seconds:
            break
    return {"env_steps_per_s": batch * n / dt, "us_per_step": 1e6 * dt / n, "steps": n, "seconds": dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--fixed-steps", type=int, default=0)
    ap.add_argument("--loops", default="random,mlp,reset,host,fused")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-log", action="store_true")
    args = ap.parse_args()
    B = args.batch
    loops = args.loops.split(",")
    lines = [f"# scripts/gpu_device_loop.py  {datetime.datetime.now().isoformat(timespec='seconds')}  humanoid B={B} fp32  "
             f"torch {torch.__version__}  device {torch.cuda.get_device_name(0)}",
             "# env-steps/s = B x steps / host-clock window (synchronised at both ends, after warm-up)"]
    res = {}

    def report(name, r, extra=""):
        res[name] = r
        line = f"{name:8s} {r['env_steps_per_s'] / 1e6:8.2f} M env-steps/s   {r['us_per_step']:8.1f} us/step   ({r['steps']} steps, {r['seconds']:.3f} s){extra}"
        lines.append(line)
        print(line, flush=True)

    obs_spec = mt.ObservationSpec(as_dict=False)
    for name in loops:
        if name in ("random", "mlp", "reset"):
            if name == "mlp":
                probe = mt.ModelHandle.from_xml_path(XML, batch=1)
                ctl = TorchMLP(probe.model.nq, probe.model.nv, probe.model.nu)
                del probe
            else:
                ctl = TorchRandom(seed=1)
            kw = {}
            if name == "reset":
                kw = dict(done_fn=lambda m, d, o: d.qpos[:, 2] < 1.0, reset_done=True, reset_noise=(0.01, 0.01), reset_seed=3)
            env = mt.Env.from_xml_path(XML, obs_spec=obs_spec, controller=ctl, batch=B, dtype="float32", **kw)
            r = timed(lambda: env.step(), B, args.warmup, args.min_seconds, args.fixed_steps)
            extra = ""
            if name == "reset":
                torch.cuda.synchronize()
                extra = f"   resets so far: {int(env.device_data.episode.sum())}"
            report(name, r, extra)
            del env
        elif name == "host":
            env = mt.Env.from_xml_path(XML, obs_spec=obs_spec, controller=HostRandom(), batch=B, dtype="float32")
            report(name, timed(lambda: env.step(), B, 10, args.min_seconds, args.fixed_steps, chunk=10))
            del env
        elif name == "fused":
            env = mt.Env.from_xml_path(XML, obs_spec=obs_spec, controller=mt.RandomCtrlController(seed=0), batch=B, dtype="float32")
            r = timed(lambda: env.rollout(20), B, 3, args.min_seconds, args.fixed_steps, chunk=5)
            r = dict(r, env_steps_per_s=r["env_steps_per_s"] * 20, steps=r["steps"] * 20, us_per_step=r["us_per_step"] / 20)   # launches -> steps
            report(name + "/20", r)
            del env
    if "host" in res:
        for k in ("random", "mlp", "reset"):
            if k in res:
                lines.append(f"# {k} / host = {res[k]['env_steps_per_s'] / res['host']['env_steps_per_s']:.2f}x")
    if not args.no_log:
        out = args.out or os.path.join(ROOT, "profiles", f"device_loop_{datetime.date.today().isoformat()}.log")
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print("wrote", out)


if __name__ == "__main__":
    main()
