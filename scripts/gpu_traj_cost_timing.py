"""``trajectory_cost`` / ``select_candidates`` against the torch expressions they replace, on identical inputs, in one process.

The torch side of the cost is what ``scripts/gpu_ilqr_cartpole.py --cost torch`` and the planners of INTEGRATION.md write: the
``einsum`` cost plus ``xs @ Q``, ``u @ R`` and ``Qf @ xs[T]``; for the humanoid (``nq != nv``) it needs a torch ``differentiatePos``,
written below.  The torch side of the selection is ``argmin`` + gather, and ``softmax`` + ``einsum``.  Each cell is the median of
--windows alternated windows (kernel, torch, kernel, ...), every window closed by a device synchronise, after one warm-up of each;
min..max are kept.  Random states of the model's sizes: the time does not depend on the values.  Prints one JSON line; --out also
writes it to a file.

    python scripts/gpu_traj_cost_timing.py [--windows 5] [--out profiles/traj_cost_timing.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mujoco_template_amd import mj, select_candidates, trajectory_cost  # noqa: E402

# model, B, T, state dtype, gradients
COST_ROWS = [("cartpole", 1, 100, "float64", True), ("humanoid", 1, 500, "float64", True), ("humanoid", 4096, 50, "float32", False),
             ("cartpole", 4096, 50, "float64", True)]
# nprob, ncand, T, nu, candidate dtype
SELECT_ROWS = [(256, 16, 100, 1, "float64"), (1, 4096, 50, 21, "float32")]


def torch_diff_scalar(x, x_ref, nq):
    return x - x_ref


def torch_diff_free_root(x, x_ref, nq):
    """differentiatePos(x_ref -> x) for a model whose first joint is free and whose others are scalar (the humanoid): [.., nq + nv] -> [.., 2 nv]"""
    q1, q2 = x_ref[..., 3:7], x[..., 3:7]
    a0, a1, a2, a3 = q1[..., 0], -q1[..., 1], -q1[..., 2], -q1[..., 3]
    b0, b1, b2, b3 = q2[..., 0], q2[..., 1], q2[..., 2], q2[..., 3]
    w = a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3
    v = torch.stack([a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2, a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], dim=-1)
    sn = v.norm(dim=-1)
    ang = 2 * torch.atan2(sn, w)
    ang = torch.where(ang > torch.pi, ang - 2 * torch.pi, ang)
    rot = v * torch.where(sn < 1e-15, torch.zeros_like(sn), ang / sn.clamp_min(1e-300))[..., None]
    return torch.cat([x[..., :3] - x_ref[..., :3], rot, x[..., 7:] - x_ref[..., 7:]], dim=-1)


def torch_cost(diff, x, u, x_ref, Q, R, Qf, nq, gradients):
    """x [B, T + 1, nq + nv], u [B, T, nu] in their own dtype (widened here, as a float64 cost of a float32 rollout has to)"""
    dx, du = diff(x.double(), x_ref, nq), u.double()
    run = 0.5 * torch.einsum("bti,ij,btj->b", dx[:, :-1], Q, dx[:, :-1]) + 0.5 * torch.einsum("bti,ij,btj->b", du, R, du)
    cost = run + 0.5 * torch.einsum("bi,ij,bj->b", dx[:, -1], Qf, dx[:, -1])
    if not gradients:
        return cost, None, None, None
    return cost, dx[:, :-1] @ Q, du @ R, dx[:, -1] @ Qf


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def compare(kernel, loop, windows):
    kernel(); loop()                                             # warm-up of both
    a, b = [], []
    for _ in range(windows):
        a.append(window(kernel)); b.append(window(loop))
    cell = lambda v: {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v)}
    return {"kernel": cell(a), "torch": cell(b), "speedup": statistics.median(b) / statistics.median(a)}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the kernels run on the MI355X")
    dev, f64 = torch.device("cuda"), torch.float64
    datas = {}
    cost_rows, select_rows = [], []
    for name, B, T, dtype, gradients in COST_ROWS:
        if name not in datas:
            xml = os.path.join(ROOT, "models", name + ".xml")
            datas[name] = mj.MjData(mj.MjModel.from_xml_path(xml), batch=1, dtype="float64")
        data = datas[name]
        cm = data.sim.model.compiled
        nq, nv, nu = int(cm.nq), int(cm.nv), int(cm.nu)
        nx, ns = 2 * nv, nq + nv
        tdt = torch.float32 if dtype == "float32" else f64
        g = torch.Generator(device="cpu").manual_seed(0)
        rnd = lambda *s: torch.randn(s, generator=g, dtype=f64).to(dev)
        x_ref = torch.cat([torch.as_tensor(cm.qpos0, dtype=f64).reshape(-1), torch.zeros(nv, dtype=f64)]).to(dev)
        full = torch.zeros((B, T + 1, 1 + ns), dtype=f64, device=dev)
        full[..., 1:] = x_ref + 0.3 * rnd(B, T + 1, ns)
        if nq != nv:                                             # the free root joint: a unit quaternion some way from the reference's
            q = rnd(B, T + 1, 4) + torch.tensor([2.0, 0, 0, 0], dtype=f64, device=dev)
            full[..., 4:8] = q / q.norm(dim=-1, keepdim=True)
        full = full.to(tdt)
        state, x0, x = full[:, 1:], full[:, 0], full[..., 1:]
        u = (0.3 * rnd(B, T, nu)).to(tdt)
        Gq, Gr = rnd(nx, nx), rnd(nu, nu)
        Q, R = Gq @ Gq.T / nx + torch.eye(nx, dtype=f64, device=dev), Gr @ Gr.T / nu + 0.01 * torch.eye(nu, dtype=f64, device=dev)
        Q, R = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
        Qf = 20.0 * Q
        diff = torch_diff_free_root if nq != nv else torch_diff_scalar
        kern = lambda: trajectory_cost(data, state, u, initial_state=x0, Q=Q, R=R, Qf=Qf, x_ref=x_ref, gradients=gradients)
        loop = lambda: torch_cost(diff, x, u, x_ref, Q, R, Qf, nq, gradients)
        k, t = kern(), loop()
        agree = {"cost": rel(k.cost, t[0])}
        if gradients:
            agree.update(lx=rel(k.lx, t[1]), lu=rel(k.lu, t[2]), VxT=rel(k.VxT, t[3]))
        cell = compare(kern, loop, args.windows)
        cost_rows.append({"model": name, "nx": nx, "nu": nu, "B": B, "T": T, "state_dtype": dtype, "gradients": gradients, **cell, "kernel_vs_torch_rel": agree})
        print(f"cost {name} B={B} T={T} {dtype}{'' if gradients else ' (cost only)'}: kernel {cell['kernel']['median_ms']:.3f} ms vs torch "
              f"{cell['torch']['median_ms']:.3f} ms (x{cell['speedup']:.2f}); agreement {agree}", file=sys.stderr, flush=True)
    data = datas["cartpole"]
    for G, n, T, nu, dtype in SELECT_ROWS:
        tdt = torch.float32 if dtype == "float32" else f64
        g = torch.Generator(device="cpu").manual_seed(1)
        cand = torch.randn((G, n, T, nu), generator=g, dtype=f64).to(dev, tdt)
        cost = (torch.rand((G, n), generator=g, dtype=f64) * 5.0 + 1.0).to(dev)
        temperature = 0.5
        rows = torch.arange(G, device=dev)
        modes = {
            "argmin": (lambda: select_candidates(data, cost, cand).u, lambda: cand[rows, torch.argmin(cost, dim=1)]),
            "softmin": (lambda: select_candidates(data, cost, cand, mode="softmin", temperature=temperature).u,
                        lambda: torch.einsum("gn,gntu->gtu", torch.softmax(-cost / temperature, dim=1), cand.double()).to(tdt)),
        }
        row = {"nprob": G, "ncand": n, "T": T, "nu": nu, "cand_dtype": dtype}
        for mode, (kern, loop) in modes.items():
            agree = rel(kern().double(), loop().double())
            cell = compare(kern, loop, args.windows)
            row[mode] = {**cell, "kernel_vs_torch_rel": agree}
            print(f"select {mode} nprob={G} ncand={n} T={T} nu={nu} {dtype}: kernel {cell['kernel']['median_ms']:.3f} ms vs torch "
                  f"{cell['torch']['median_ms']:.3f} ms (x{cell['speedup']:.2f}); agreement {agree:.2e}", file=sys.stderr, flush=True)
        select_rows.append(row)
    res = {"windows": args.windows, "cost": cost_rows, "select": select_rows}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
