"""``lqr_backward`` / ``lqr_candidates`` against the torch float64 loops they replace, on identical inputs, in one process.

The torch side is the loop of ``scripts/gpu_ilqr_cartpole.py --backward torch`` batched over the B trajectories
(``torch.linalg.solve`` / ``@`` on ``[B, ...]`` tensors): the best the library offered before the kernels.  Each cell is the median of
--windows alternated windows (kernel, torch, kernel, ...), every window closed by a device synchronise, after one warm-up of each;
min..max are kept.  Random benign systems of the model's sizes (cart-pole 4 / 1, humanoid 54 / 21): the time does not depend on the
values.  Prints one JSON line; --out also writes it to a file.

    python scripts/gpu_lqr_timing.py [--windows 5] [--alphas 16] [--out profiles/lqr_timing.json]
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

from mujoco_template_amd import lqr_backward, lqr_candidates, mj  # noqa: E402

ROWS = [("cartpole", 4, 1, 1, 100), ("humanoid", 54, 21, 1, 100), ("humanoid", 54, 21, 1, 500), ("humanoid", 54, 21, 256, 50), ("cartpole", 4, 1, 4096, 50)]


def flops_per_step(nx, nu):
    """Multiply-adds x 2 of one step of the recursion: Vxx A, A' (Vxx A): 2 x 2 nx^3; Vxx B, B' (Vxx A), and the two rank-nu terms of the
    Vxx update: 4 x 2 nx^2 nu; B' (Vxx B), Quu K and the substitutions for nx + 1 right-hand sides: 2 nx nu^2 x 3; Cholesky nu^3 / 3."""
    return 4 * nx ** 3 + 8 * nx * nx * nu + 6 * nx * nu * nu + nu ** 3 // 3


def torch_backward(A, Bm, lx, lu, Q, R, Qf, mu):
    B, T, nx, nu = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]
    Vx, Vxx = torch.zeros((B, nx, 1), dtype=A.dtype, device=A.device), Qf.expand(B, nx, nx).clone()
    ks, Ks = torch.zeros((B, T, nu, 1), dtype=A.dtype, device=A.device), torch.zeros((B, T, nu, nx), dtype=A.dtype, device=A.device)
    eye = mu * torch.eye(nu, dtype=A.dtype, device=A.device)
    for t in range(T - 1, -1, -1):
        At, Bt = A[:, t], Bm[:, t]
        AT, BT = At.transpose(1, 2), Bt.transpose(1, 2)
        Qx, Qu = lx[:, t, :, None] + AT @ Vx, lu[:, t, :, None] + BT @ Vx
        Qxx, Quu, Qux = Q + AT @ Vxx @ At, R + BT @ Vxx @ Bt + eye, BT @ Vxx @ At
        k, K = -torch.linalg.solve(Quu, Qu), -torch.linalg.solve(Quu, Qux)
        ks[:, t], Ks[:, t] = k, K
        KT = K.transpose(1, 2)
        Vx = Qx + KT @ Quu @ k + KT @ Qu + Qux.transpose(1, 2) @ k
        Vxx = Qxx + KT @ Quu @ K + KT @ Qux + Qux.transpose(1, 2) @ K
        Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
    return ks[..., 0], Ks


def torch_candidates(A, Bm, k, K, u, alphas, lo, hi):
    B, T, nx, nu, na = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3], alphas.shape[0]
    dx = torch.zeros((B, na, nx), dtype=A.dtype, device=A.device)
    cand = torch.empty((B, na, T, nu), dtype=A.dtype, device=A.device)
    for t in range(T):
        du = alphas[None, :, None] * k[:, t][:, None] + dx @ K[:, t].transpose(1, 2)
        cand[:, :, t] = (u[:, t][:, None] + du).clamp(lo, hi)
        dx = dx @ A[:, t].transpose(1, 2) + (cand[:, :, t] - u[:, t][:, None]) @ Bm[:, t].transpose(1, 2)
    return cand


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--alphas", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the kernels run on the MI355X")
    dev, f64 = torch.device("cuda"), torch.float64
    data = mj.MjData(mj.MjModel.from_xml_path(os.path.join(ROOT, "models", "cartpole.xml")), batch=1, dtype="float64")
    alphas = torch.cat([torch.tensor([0.0]), torch.logspace(0, -3, args.alphas - 1)]).to(dev, f64)
    rows = []
    for name, nx, nu, B, T in ROWS:
        g = torch.Generator(device="cpu").manual_seed(0)
        rnd = lambda *s: torch.randn(s, generator=g, dtype=f64).to(dev)
        A = torch.eye(nx, dtype=f64, device=dev) + 0.02 * rnd(B, 1, nx, nx) / nx ** 0.5 + 0.005 * rnd(B, T, nx, nx) / nx ** 0.5
        Bm = (0.05 * rnd(B, 1, nx, nu)).expand(B, T, nx, nu).contiguous()
        lx, lu, u = rnd(B, T, nx), 0.1 * rnd(B, T, nu), 0.1 * rnd(B, T, nu)
        Q, R = torch.diag(torch.rand(nx, generator=g, dtype=f64) * 9.9 + 0.1).to(dev), 0.01 * torch.eye(nu, dtype=f64, device=dev)
        Qf = 20.0 * Q
        sol = lqr_backward(data, A, Bm, lx=lx, lu=lu, lxx=Q, luu=R, VxxT=Qf, mu=1e-6)
        assert int(sol.status.abs().max()) == 0
        kt, Kt = torch_backward(A, Bm, lx, lu, Q, R, Qf, 1e-6)
        agree = float((sol.K - Kt).abs().max() / Kt.abs().max())
        back = compare(lambda: lqr_backward(data, A, Bm, lx=lx, lu=lu, lxx=Q, luu=R, VxxT=Qf, mu=1e-6), lambda: torch_backward(A, Bm, lx, lu, Q, R, Qf, 1e-6), args.windows)
        cnd = compare(lambda: lqr_candidates(data, A, Bm, sol.k, sol.K, u, alphas, lo=-4.0, hi=4.0), lambda: torch_candidates(A, Bm, sol.k, sol.K, u, alphas, -4.0, 4.0), args.windows)
        flop = flops_per_step(nx, nu) * T * B
        rows.append({"model": name, "nx": nx, "nu": nu, "B": B, "T": T, "backward": back, "candidates": cnd, "K_kernel_vs_torch_rel": agree,
                     "backward_flop": flop, "backward_gflops": flop / (back["kernel"]["median_ms"] * 1e-3) / 1e9})
        print(f"{name} B={B} T={T}: backward {back['kernel']['median_ms']:.3f} ms vs torch {back['torch']['median_ms']:.1f} ms (x{back['speedup']:.0f}); "
              f"candidates {cnd['kernel']['median_ms']:.3f} ms vs {cnd['torch']['median_ms']:.1f} ms (x{cnd['speedup']:.0f})", file=sys.stderr, flush=True)
    res = {"windows": args.windows, "alphas": args.alphas, "rows": rows}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
