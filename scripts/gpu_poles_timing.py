"""Times ``mt.closed_loop_poles`` (``mjb_lqr_eig``) against the routes it replaces, on cart-pole closed loops (4 x 1) and on
humanoid-sized ones (54 x 21, the tutorial's balance design of tests/golden/dare_humanoid.npz), every system with its own gain
(``solve_dare`` with Q scaled per problem): 4096 cart-poles, 4096 humanoids and a single humanoid.

    python scripts/gpu_poles_timing.py [--out FILE.json] [--reps 20]

  * closed_loop_poles: HIP events around one call, warm-up excluded, the median of ``--reps`` (>= 10) calls - MEASURED;
  * the host loop it replaces: the device -> host copy of (A, B, K), then ``A - B @ K`` and ``numpy.linalg.eigvals`` per system -
    MEASURED on min(nb, 16) systems and EXTRAPOLATED linearly to nb where nb > 16 (said so in the output);
  * ``torch.linalg.eigvals(A - B @ K)`` on the same device tensors, if it runs: wall clock around the call and a synchronisation (it
    synchronises by itself), the median of 3 calls after one warm-up - MEASURED.
Prints one JSON object per case; every number says whether it is measured or extrapolated.
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
    rows = []
    for name, nb in (("cartpole_4x1", 4096), ("humanoid_54x21", 4096), ("humanoid_54x21", 1)):
        A1, B1, Q1, R1 = designs[name]
        nx, nu = int(A1.shape[0]), int(B1.shape[1])
        scale = torch.linspace(0.5, 2.0, nb, dtype=torch.float64, device=dev) if nb > 1 else torch.ones(1, dtype=torch.float64, device=dev)
        Ab, Bb = A1[None].expand(nb, nx, nx).contiguous(), B1[None].expand(nb, nx, nu).contiguous()
        sol = mt.solve_dare(data, Ab, Bb, (scale[:, None, None] * Q1[None]).contiguous(), R1)
        K = sol.K
        res = mt.closed_loop_poles(data, Ab, Bb, K)
        torch.cuda.synchronize()
        assert bool((sol.status == 0).all()) and bool((res.status == 0).all()), (sol.status, res.status)
        med, lo, hi = event_median_ms(torch, lambda: mt.closed_loop_poles(data, Ab, Bb, K), reps)
        row = {"design": name, "nb": nb, "sweeps_max": int(res.sweeps.max()), "rho_max": float(res.rho.max()),
               "closed_loop_poles_ms": {"median": med, "min": lo, "max": hi, "reps": reps, "how": "measured, HIP events"}}
        # the host loop: device -> host copy, A - B K and numpy's eigvals per system
        ns = min(nb, 16)
        t0 = time.perf_counter()
        Ah, Bh, Kh = Ab[:ns].cpu().numpy(), Bb[:ns].cpu().numpy(), K[:ns].cpu().numpy()
        rho_host = [float(np.abs(np.linalg.eigvals(Ah[e] - Bh[e] @ Kh[e])).max()) for e in range(ns)]
        dt = (time.perf_counter() - t0) * 1e3
        row["numpy_host_loop_ms"] = {"value": dt * nb / ns, "systems_timed": ns,
                                     "how": "measured" if ns == nb else f"EXTRAPOLATED from {ns} systems ({dt:.2f} ms measured)"}
        row["rho_vs_numpy"] = float(np.abs(res.rho[:ns].cpu().numpy() - np.array(rho_host)).max())
        try:
            route = lambda: torch.linalg.eigvals(Ab - Bb @ K).abs().amax(dim=1)
            rho_t = route()
            torch.cuda.synchronize()
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                route()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            row["torch_linalg_eigvals_ms"] = {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times)), "reps": 3,
                                              "how": "measured, wall clock with a synchronisation",
                                              "rho_vs_kernel": float((rho_t - res.rho).abs().max())}
        except Exception as exc:  # noqa: BLE001  (whatever the ROCm build of torch answers: reported, not hidden)
            row["torch_linalg_eigvals_ms"] = {"how": f"did not run: {type(exc).__name__}: {str(exc)[:200]}"}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
