"""Times ``mt.closed_loop_cost`` (``mjb_lqr_dlyap``) against the two routes it replaces, on cart-pole closed loops (4 x 1) and on
humanoid-sized ones (54 x 21, tests/golden/dare_humanoid.npz), for nb = 1 and 4096 systems (copies with Q scaled per problem, each
with its own gain from ``mt.solve_dare``).

    python scripts/gpu_dlyap_timing.py [--out FILE.json] [--reps 20]

  * closed_loop_cost: HIP events around one call, warm-up excluded, the median of ``--reps`` (>= 10) calls - MEASURED;
  * the host loop it replaces: the device -> host copy of (A, B, K, Q), then M, S and scipy.linalg.solve_discrete_lyapunov per system
    - MEASURED on min(nb, 16) systems and EXTRAPOLATED linearly to nb where nb > 16 (said so in the output);
  * the same iteration written in torch float64 on the device (batched matmul, the kernel's largest iteration count for every
    problem, no convergence test and therefore no host synchronisation: the torch route at its best) - MEASURED with HIP events.
Prints one JSON object per row; every number says whether it is measured or extrapolated.
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


def torch_smith(A, B, K, Q, R, iters):
    """The iteration of include/mjbatch.h in batched torch float64: `iters` doublings for every problem."""
    M = A - B @ K
    V = Q + K.transpose(1, 2) @ (R @ K)
    P = 0.5 * (V + V.transpose(1, 2))
    for _ in range(iters):
        T = M.transpose(1, 2) @ (P @ M)
        P = P + 0.5 * (T + T.transpose(1, 2))
        M = M @ M
    return P


def main():
    import torch
    from scipy.linalg import solve_discrete_lyapunov

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
    for name, (A1, B1, Q1, R1) in designs.items():
        nx, nu = int(A1.shape[0]), int(B1.shape[1])
        for nb in (1, 4096):
            scale = torch.linspace(0.5, 2.0, nb, dtype=torch.float64, device=dev) if nb > 1 else torch.ones(1, dtype=torch.float64, device=dev)
            Q = (scale[:, None, None] * Q1[None]).contiguous()
            Ab, Bb = A1[None].expand(nb, nx, nx).contiguous(), B1[None].expand(nb, nx, nu).contiguous()
            sol = mt.solve_dare(data, Ab, Bb, Q, R1)
            K = sol.K
            xs = torch.ones((nx,), dtype=torch.float64, device=dev)
            res = mt.closed_loop_cost(data, Ab, Bb, K, Q=Q, R=R1, x0=xs)
            torch.cuda.synchronize()
            assert bool((sol.status == 0).all()) and bool((res.status == 0).all()), (sol.status, res.status)
            med, lo, hi = event_median_ms(torch, lambda: mt.closed_loop_cost(data, Ab, Bb, K, Q=Q, R=R1, x0=xs), reps)
            iters = int(res.iters.max())
            row = {"design": name, "nb": nb, "iters_max": iters,
                   "P_vs_dare_X": float(((res.P - sol.X).abs().amax(dim=(1, 2)) / sol.X.abs().amax(dim=(1, 2))).max()),
                   "closed_loop_cost_ms": {"median": med, "min": lo, "max": hi, "reps": reps, "how": "measured, HIP events"}}
            # the host loop: device -> host copy, M, S and scipy's Lyapunov solve per system
            ns = min(nb, 16)
            t0 = time.perf_counter()
            Ah, Bh, Kh, Qh, Rh = Ab[:ns].cpu().numpy(), Bb[:ns].cpu().numpy(), K[:ns].cpu().numpy(), Q[:ns].cpu().numpy(), R1.cpu().numpy()
            Ps = []
            for e in range(ns):
                M = Ah[e] - Bh[e] @ Kh[e]
                Ps.append(solve_discrete_lyapunov(M.T, Qh[e] + Kh[e].T @ Rh @ Kh[e]))
            dt = (time.perf_counter() - t0) * 1e3
            row["scipy_host_loop_ms"] = {"value": dt * nb / ns, "systems_timed": ns,
                                         "how": "measured" if ns == nb else f"EXTRAPOLATED from {ns} systems ({dt:.1f} ms measured)"}
            Pk = res.P[:ns].cpu().numpy()
            row["P_vs_scipy"] = float(max(np.abs(Pk[e] - Ps[e]).max() / np.abs(Ps[e]).max() for e in range(ns)))
            # the same iteration in torch on the device
            Rb = R1[None]
            Pt = torch_smith(Ab, Bb, K, Q, Rb, iters)
            m2, l2, h2 = event_median_ms(torch, lambda: torch_smith(Ab, Bb, K, Q, Rb, iters), reps)
            row["torch_float64_ms"] = {"median": m2, "min": l2, "max": h2, "iters": iters, "how": "measured, HIP events; fixed iteration count, no host sync"}
            row["P_vs_torch"] = float(((res.P - Pt).abs().amax(dim=(1, 2)) / Pt.abs().amax(dim=(1, 2))).max())
            del Pt
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
