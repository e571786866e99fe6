"""Times ``mt.feedback_ctrl`` (``mjb_feedback_law``) against the torch expression a user writes on ``DeviceData`` today, and
``mt.rollout_feedback`` per step against ``mjb_step(d, 1)`` alone.

    python scripts/gpu_feedback_timing.py [--out FILE.json] [--reps 20]

  * the law call at B = 4096 for cart-pole, drone2 and humanoid (float32 data), ``K`` in float64 and in float32, shared ``[nu, 2nv]``
    and per environment ``[B, nu, 2nv]``: HIP events around a window of back-to-back calls that lasts at least 30 ms, warm-up excluded,
    per call, the median of ``--reps`` (>= 10) such windows - MEASURED.  This is the whole Python call at its sustained rate; where
    the kernel is shorter than the enqueue, it is the enqueue rate;
  * the torch route: ``u0 - einsum(K, dx)`` and the clip on the same device tensors, with the quaternion difference of the free joint
    written in torch (one gather per joint kind, no Python loop over environments) - MEASURED the same way;
  * each figure also as bytes moved (K + u0 + q0 + v0 + state + ctrl) over 6.3 TB/s, the achievable HBM rate: the time the traffic alone
    would take.  A 4096-humanoid float64 ``K`` is 37 MB and lives in the 256 MiB Infinity Cache between calls, so one more
    per-environment float64 humanoid case has B = 32768 (``K``: 297 MB, more than the cache holds) - the rows say which is which;
  * ``rollout_feedback`` (20 steps per call) per step against ``step(1)``: the difference is the price of the law and the record.
Prints one JSON object per row.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WINDOW_MS = 30.0  # a timed window lasts at least this long: a window of a fraction of a millisecond measures the clock and the scheduler
HBM_BYTES_PER_MS = 6.3e9


def event_median_ms(torch, fn, reps, warmup=3):
    """Per-call milliseconds: the median, minimum and maximum over ``reps`` windows of back-to-back calls, and the calls per window
    (chosen from a first window of 10 calls so that a window lasts at least ``WINDOW_MS``)."""
    def window(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    inner = max(1, int(np.ceil(WINDOW_MS / max(window(10), 1e-4))))
    times = [window(inner) for _ in range(reps)]
    return {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times)), "reps": reps, "calls_per_window": inner,
            "how": "measured, HIP events"}


def torch_law(torch, cm):
    """The law in torch on DeviceData, as a user writes it today: float64 arithmetic, the free joint's quaternion difference by hand."""
    jt, jq, jd = (np.asarray(x) for x in (cm.jnt_type, cm.jnt_qposadr, cm.jnt_dofadr))
    nv, nu = int(cm.nv), int(cm.nu)
    free = [(int(jq[j]), int(jd[j])) for j in range(len(jt)) if jt[j] == 0]
    sq = torch.as_tensor([int(jq[j]) for j in range(len(jt)) if jt[j] != 0], dtype=torch.long, device="cuda")
    sd = torch.as_tensor([int(jd[j]) for j in range(len(jt)) if jt[j] != 0], dtype=torch.long, device="cuda")
    rg = torch.as_tensor(np.asarray(cm.actuator_ctrlrange, dtype=np.float64).reshape(nu, 2), device="cuda")
    lim = torch.as_tensor(np.asarray(cm.actuator_ctrllimited).reshape(nu) != 0, device="cuda")
    inf = torch.full((nu,), float("inf"), dtype=torch.float64, device="cuda")
    lo, hi = torch.where(lim, rg[:, 0], -inf), torch.where(lim, rg[:, 1], inf)

    def law(dd, K, u0, q0):
        qpos, qvel, q0 = dd.qpos.double(), dd.qvel.double(), q0.double().expand(dd.qpos.shape)
        dx = torch.empty((qpos.shape[0], 2 * nv), dtype=torch.float64, device=qpos.device)
        dx[:, sd] = qpos[:, sq] - q0[:, sq]
        for qa, da in free:
            dx[:, da:da + 3] = qpos[:, qa:qa + 3] - q0[:, qa:qa + 3]
            a, b = q0[:, qa + 3:qa + 7], qpos[:, qa + 3:qa + 7]
            a0, a1, a2, a3 = a[:, 0], -a[:, 1], -a[:, 2], -a[:, 3]
            w = a0 * b[:, 0] - a1 * b[:, 1] - a2 * b[:, 2] - a3 * b[:, 3]
            v = torch.stack([a0 * b[:, 1] + a1 * b[:, 0] + a2 * b[:, 3] - a3 * b[:, 2], a0 * b[:, 2] - a1 * b[:, 3] + a2 * b[:, 0] + a3 * b[:, 1],
                             a0 * b[:, 3] + a1 * b[:, 2] - a2 * b[:, 1] + a3 * b[:, 0]], dim=1)
            sn = v.norm(dim=1)
            ang = 2 * torch.atan2(sn, w)
            ang = torch.where(ang > np.pi, ang - 2 * np.pi, ang)
            dx[:, da + 3:da + 6] = torch.where((sn < 1e-15)[:, None], torch.zeros_like(v), v * (ang / sn.clamp_min(1e-300))[:, None])
        dx[:, nv:] = qvel
        s = torch.einsum("ak,bk->ba", K.double(), dx) if K.ndim == 2 else torch.einsum("bak,bk->ba", K.double(), dx)
        dd.ctrl.copy_(torch.minimum(torch.maximum(u0.double() - s, lo), hi))

    return law


def main():
    import torch

    import mujoco_template_amd as mt
    from mujoco_template_amd import mj

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    reps = max(10, args.reps)
    rng = np.random.default_rng(0)
    rows = []
    paths = {"cartpole": "cartpole.xml", "drone2": os.path.join("drone2", "scene.xml"), "humanoid": "humanoid.xml"}
    for name, nb in (("cartpole", 4096), ("drone2", 4096), ("humanoid", 4096), ("humanoid", 32768)):
        model = mj.MjModel.from_xml_path(os.path.join(ROOT, "models", paths[name]))
        data = mj.MjData(model, batch=nb, dtype="float32")
        sim = data.sim
        cm = sim.model.compiled
        nq, nv, nu = int(cm.nq), int(cm.nv), int(cm.nu)
        dd = mt.DeviceData(data)
        sim.use_torch_stream()
        dd.qvel.copy_(torch.as_tensor(rng.normal(size=(nb, nv)) * 0.05, dtype=torch.float32, device="cuda"))
        q0 = torch.as_tensor(np.asarray(cm.qpos0, dtype=np.float64).reshape(nq), device="cuda")
        u0 = torch.zeros((nb, nu), dtype=torch.float64, device="cuda")
        law = torch_law(torch, cm)
        state_bytes = nb * (nq + nv + nu) * 4 + u0.numel() * 8 + q0.numel() * 8
        for kdt in (torch.float64, torch.float32):
            for per_env in (False, True):
                if nb > 4096 and not (per_env and kdt == torch.float64):
                    continue
                amp = 0.01 * float(np.abs(np.asarray(cm.actuator_ctrlrange)).max())
                K = torch.as_tensor(rng.normal(size=((nb,) if per_env else ()) + (nu, 2 * nv)) * amp, dtype=kdt, device="cuda")
                st = mt.feedback_ctrl(data, K, u0, q0)
                mine = dd.ctrl.double().clone()
                law(dd, K, u0, q0)
                torch.cuda.synchronize()
                agree = float((dd.ctrl.double() - mine).abs().max())
                kbytes = K.numel() * K.element_size()
                row = {"model": name, "batch": nb, "K_dtype": str(kdt).replace("torch.", ""), "K": "per environment" if per_env else "shared",
                       "K_bytes": kbytes, "K_fits_infinity_cache": bool(kbytes < 256 * 2 ** 20), "status_max": int(st.max()),
                       "max_abs_difference_from_torch": agree,
                       "hbm_floor_ms": (kbytes + state_bytes) / HBM_BYTES_PER_MS,
                       "feedback_ctrl_ms": event_median_ms(torch, lambda: mt.feedback_ctrl(data, K, u0, q0, status=st), reps),
                       "torch_ms": event_median_ms(torch, lambda: law(dd, K, u0, q0), reps)}
                rows.append(row)
                print(json.dumps(row), flush=True)
        if nb == 4096:                                              # the closed-loop rollout per step against the step alone
            K = torch.as_tensor(rng.normal(size=(nb, nu, 2 * nv)) * amp, dtype=torch.float64, device="cuda")
            x0 = torch.cat([dd.time[:, None].double(), dd.qpos.double(), dd.qvel.double()], dim=1).clone()
            nstep = 20
            roll = event_median_ms(torch, lambda: mt.rollout_feedback(model, data, K, u0, q0, nstep=nstep, initial_state=x0), reps)
            sim.torch_view("qpos").copy_(x0[:, 1:1 + nq])
            sim.torch_view("qvel").copy_(x0[:, 1 + nq:])
            dd.ctrl.zero_()
            step = event_median_ms(torch, lambda: sim.step(1), reps)
            row = {"model": name, "batch": nb, "rollout_feedback_per_step_ms": {**roll, "median": roll["median"] / nstep, "min": roll["min"] / nstep,
                                                                                  "max": roll["max"] / nstep, "steps_per_call": nstep},
                   "step_1_ms": step, "law_and_record_per_step_ms": roll["median"] / nstep - step["median"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del data, dd
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
