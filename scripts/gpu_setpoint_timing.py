"""Times ``mt.solve_setpoint`` (``mjb_setpoint_ctrl``) against the two routes it replaces, on 4096 cart-pole-sized (1 x 2), drone-sized
(4 x 6) and humanoid-sized (21 x 27) problems and on a single humanoid-sized one.  The humanoid-sized moment matrix is a gear-scaled
selection matrix with an unactuated 6-dof root and three tendon-like couplings; the others are Gaussian with rows scaled by
exp(N(0, 1)).

    python scripts/gpu_setpoint_timing.py [--out FILE.json] [--reps 20]

  * solve_setpoint: HIP events around a window of back-to-back calls that lasts at least 30 ms (hundreds of calls), warm-up
    excluded, per call, the median of ``--reps`` (>= 10) such windows - MEASURED.  This is the time of the whole Python call at its
    sustained rate; where the kernel is shorter than the enqueue, it is the enqueue rate;
  * the host path it replaces: the device -> host copy of (moment, qfrc), then the stacked-numpy ``_solve_for_ctrl`` of
    ``setpoints.py`` (numpy.linalg.svd, pinv, einsum) - MEASURED, wall clock, the median of ``--reps`` runs;
  * ``torch.linalg.pinv`` + ``einsum`` in float64 on the same device tensors (no conditioning guard, so no singular values are
    computed twice and nothing is copied to the host: the torch route at its best) - MEASURED with HIP events.
Prints one JSON object per row.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


WINDOW_MS = 30.0  # a timed window lasts at least this long: a window of a fraction of a millisecond measures the clock and the scheduler


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
    return float(np.median(times)), float(np.min(times)), float(np.max(times)), inner


def problems(nu, nv, nb, rng):
    if (nu, nv) == (21, 27):
        m = np.zeros((nb, nu, nv))
        gear = rng.uniform(20.0, 120.0, size=(nb, nu))
        m[:, np.arange(nu), 6 + np.arange(nu)] = gear
        for a, d, f in ((2, 11, 0.5), (9, 20, -0.3), (15, 7, 0.25)):
            m[:, a, d] = f * gear[:, a]
    else:
        m = rng.normal(size=(nb, nu, nv)) * np.exp(rng.normal(size=(nb, nu, 1)))
    return m, rng.normal(size=(nb, nv))


def main():
    import torch

    import mujoco_template_amd as mt
    from mujoco_template_amd import mj
    from mujoco_template_amd.setpoints import _solve_for_ctrl

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    reps = max(10, args.reps)
    dev = "cuda"
    model = mj.MjModel.from_xml_path(os.path.join(ROOT, "models", "cartpole.xml"))
    data = mj.MjData(model, batch=1, dtype="float64")
    rng = np.random.default_rng(0)
    rows = []
    for name, nu, nv, nb in (("cartpole_1x2", 1, 2, 4096), ("drone_4x6", 4, 6, 4096), ("humanoid_21x27", 21, 27, 4096), ("humanoid_21x27", 21, 27, 1)):
        mh, qh = problems(nu, nv, nb, rng)
        m, q = torch.as_tensor(mh, dtype=torch.float64, device=dev), torch.as_tensor(qh, dtype=torch.float64, device=dev)
        res = mt.solve_setpoint(data, m, q)
        torch.cuda.synchronize()
        assert bool((res.status == 0).all()), res.status
        med, lo, hi, inner = event_median_ms(torch, lambda: mt.solve_setpoint(data, m, q), reps)
        row = {"design": name, "nb": nb, "sweeps_max": int(res.sweeps.max()), "rcond_min": float(res.rcond.min()),
               "solve_setpoint_ms": {"median": med, "min": lo, "max": hi, "reps": reps, "calls_per_window": inner, "how": "measured, HIP events"}}
        # the host path: device -> host copy, stacked numpy svd + pinv + einsum
        host = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            u_host = _solve_for_ctrl(m.cpu().numpy(), q.cpu().numpy())
            host.append((time.perf_counter() - t0) * 1e3)
        row["numpy_host_ms"] = {"median": float(np.median(host)), "min": float(np.min(host)), "max": float(np.max(host)), "reps": reps,
                                "how": "measured, wall clock, copy included"}
        u = res.ctrl.cpu().numpy()
        row["ctrl_vs_numpy"] = float((np.abs(u - u_host).max(axis=1) / np.abs(u_host).max(axis=1) * res.rcond.cpu().numpy()).max())
        # torch on the device
        route = lambda: torch.einsum("bv,bvu->bu", q, torch.linalg.pinv(m))
        ut = route()
        m2, l2, h2, inner2 = event_median_ms(torch, route, reps)
        row["torch_float64_ms"] = {"median": m2, "min": l2, "max": h2, "reps": reps, "calls_per_window": inner2, "how": "measured, HIP events; pinv + einsum, no guard"}
        row["ctrl_vs_torch"] = float(((res.ctrl - ut).abs().amax(dim=1) / ut.abs().amax(dim=1) * res.rcond).max())
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
