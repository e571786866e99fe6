"""Times ``mt.solve_dare`` (``mjb_lqr_dare``) against the two routes it replaces, on the cart-pole (4 x 1) and on the tutorial's humanoid
balance design (54 x 21, tests/golden/dare_humanoid.npz), for nb = 1, 256, 4096 systems (copies with Q scaled per problem).

    python scripts/gpu_dare_timing.py [--out FILE.json] [--reps 20]

  * solve_dare: HIP events around one call, warm-up excluded, the median of ``--reps`` (>= 10) calls - MEASURED;
  * the host loop it replaces: the device -> host copy of (A, B, Q), then scipy.linalg.solve_discrete_are and the gain solve per
    system - MEASURED on min(nb, 16) systems and EXTRAPOLATED linearly to nb where nb > 16 (said so in the output);
  * the only device route available before: ``lqr_backward`` on ``expand``-ed constant (A, B) at the shortest horizon, among powers of
    two, whose V0xx is within 1e-10 (relative) of solve_dare's X - cart-pole only, MEASURED with its horizon reported.  On the
    humanoid design no horizon up to 20 000 reaches it (the plain recursion is still 5.5e-4 away there, measured on the CPU), so
    that route is not timed.
Prints one JSON object; every number says whether it is measured or extrapolated.
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


def event_median_ms(torch, fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    import torch
    from scipy.linalg import solve_discrete_are

    import mujoco_template_amd as mt
    from mujoco_template_amd import mj

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    reps = max(10, args.reps)
    dev = "cuda"
    model = mj.MjModel.from_xml_path(os.path.join(ROOT, "models", "cartpole.xml"))
    data = mj.MjData(model, batch=1, dtype="float64")
    cm = data.sim.model.compiled
    x0 = torch.zeros(1 + cm.nq + cm.nv, dtype=torch.float64, device=dev)
    _, _, A, B = mt.linearize_rollout(model, data, torch.zeros((1, 1, cm.nu), dtype=torch.float64, device=dev), initial_state=x0)
    z = np.load(os.path.join(ROOT, "tests", "golden", "dare_humanoid.npz"))
    t64 = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
    designs = {
        "cartpole_4x1": (A[0, 0].contiguous(), B[0, 0].contiguous(), torch.diag(t64([0.5, 10.0, 0.05, 0.1])), 0.01 * torch.eye(1, dtype=torch.float64, device=dev)),
        "humanoid_54x21": tuple(t64(z[k]) for k in "ABQR"),
    }
    rows, horizon = [], {}
    for name, (A1, B1, Q1, R1) in designs.items():
        nx, nu = int(A1.shape[0]), int(B1.shape[1])
        for nb in (1, 256, 4096):
            scale = torch.linspace(0.5, 2.0, nb, dtype=torch.float64, device=dev) if nb > 1 else torch.ones(1, dtype=torch.float64, device=dev)
            Q = (scale[:, None, None] * Q1[None]).contiguous()
            Ab, Bb = A1[None].expand(nb, nx, nx).contiguous(), B1[None].expand(nb, nx, nu).contiguous()
            res = mt.solve_dare(data, Ab, Bb, Q, R1)
            torch.cuda.synchronize()
            assert bool((res.status == 0).all()), res.status
            med, lo, hi = event_median_ms(torch, lambda: mt.solve_dare(data, Ab, Bb, Q, R1), reps)
            row = {"design": name, "nb": nb, "iters_max": int(res.iters.max()), "solve_dare_ms": {"median": med, "min": lo, "max": hi, "reps": reps, "how": "measured, HIP events"}}
            # the host loop: device -> host copy, scipy's DARE and the gain solve per system
            ns = min(nb, 16)
            t0 = time.perf_counter()
            Ah, Bh, Qh, Rh = Ab[:ns].cpu().numpy(), Bb[:ns].cpu().numpy(), Q[:ns].cpu().numpy(), R1.cpu().numpy()
            worst = 0.0
            for e in range(ns):
                P = solve_discrete_are(Ah[e], Bh[e], Qh[e], Rh)
                K = np.linalg.solve(Rh + Bh[e].T @ P @ Bh[e], Bh[e].T @ P @ Ah[e])
                worst = max(worst, float(np.abs(res.K[e].cpu().numpy() - K).max() / np.abs(K).max())) if e < 2 else worst
            dt = (time.perf_counter() - t0) * 1e3
            row["scipy_host_loop_ms"] = {"value": dt * nb / ns, "systems_timed": ns,
                                         "how": "measured" if ns == nb else f"EXTRAPOLATED from {ns} systems ({dt:.1f} ms measured)"}
            row["K_vs_scipy"] = worst
            if name.startswith("cartpole"):
                T = horizon.get(name, 64)                        # the horizon found at a smaller nb is where the search starts
                while T <= 1 << 14:
                    sol = mt.lqr_backward(data, Ab[:, None].expand(nb, T, nx, nx), Bb[:, None].expand(nb, T, nx, nu), lxx=Q[:, None].expand(nb, T, nx, nx),
                                          luu=R1, VxxT=Q, mu=0.0)
                    err = float(((sol.V0xx - res.X).abs().amax(dim=(1, 2)) / res.X.abs().amax(dim=(1, 2))).max())
                    if err <= 1e-10:
                        break
                    T *= 2
                del sol
                if err <= 1e-10:
                    horizon[name] = T
                    At, Bt, Qt = Ab[:, None].expand(nb, T, nx, nx), Bb[:, None].expand(nb, T, nx, nu), Q[:, None].expand(nb, T, nx, nx)
                    m2, l2, h2 = event_median_ms(torch, lambda: mt.lqr_backward(data, At, Bt, lxx=Qt, luu=R1, VxxT=Q, mu=0.0), reps)
                    row["lqr_backward_ms"] = {"median": m2, "min": l2, "max": h2, "horizon": T, "V0xx_vs_X": err, "how": "measured, HIP events"}
                else:
                    row["lqr_backward_ms"] = {"how": f"no power-of-two horizon up to {T // 2} is within 1e-10 (reached {err:.1e})"}
            else:
                row["lqr_backward_ms"] = {"how": "not timed: no horizon up to 20000 reaches the solution (5.5e-4 away, measured on the CPU)"}
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
