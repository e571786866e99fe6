"""``lqr_backward`` / ``lqr_candidates`` against the torch float64 loops they replace, on identical inputs, in one process.

The torch side is the loop of ``scripts/gpu_ilqr_cartpole.py --backward torch`` batched over the B trajectories
(``torch.linalg.solve`` / ``@`` on ``[B, ...]`` tensors): the best the library offered before the kernels.  Each cell is the median of
--windows alternated windows (kernel, torch, kernel, ...), every window closed by a device synchronise, after one warm-up of each;
min..max are kept.  Random benign systems of the model's sizes (cart-pole 4 / 1, humanoid 54 / 21): the time does not depend on the
values.  Prints one JSON line; --out also writes it to a file.

Each row also times the control-limited pass (``lqr_backward(..., u=, lo=, hi=)``): against ``torch_backward_box``, a torch float64
restatement of the same per-step QP loop, with a box that binds (--bound), and against the unconstrained kernel with a box that never binds.

    python scripts/gpu_lqr_timing.py [--windows 5] [--box-windows 3] [--bound 0.5] [--alphas 16] [--out profiles/lqr_timing.json]
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


def torch_box_qp(Quu, Qu, lob, hib, max_iter=64, max_trials=64):
    """The box QP of every trajectory at one step, min x' Quu x / 2 + Qu' x on [lob, hib], by the projected Newton iteration of
    ``mjb_lqr_backward_box`` written with batched torch operations: what a user of the library would write without the kernel.
    Returns the iterate and its clamped set [B, nu]."""
    B, nu = Qu.shape
    eye = torch.eye(nu, dtype=Qu.dtype, device=Qu.device).expand(B, nu, nu)
    mv = lambda M, v: (M @ v[..., None])[..., 0]
    f = lambda y: (y * (Qu + 0.5 * mv(Quu, y))).sum(-1)
    x = torch.zeros_like(Qu).clamp(lob, hib)
    done = torch.zeros(B, dtype=torch.bool, device=Qu.device)
    g = Qu + mv(Quu, x)
    c = ((x == lob) & (g > 0)) | ((x == hib) & (g < 0))
    for _ in range(max_iter):
        done = done | c.all(-1)
        if bool(done.all()):
            break
        H = torch.where(c[:, :, None] | c[:, None, :], eye, Quu)
        rhs = torch.where(c, torch.zeros_like(Qu), Qu + mv(Quu, torch.where(c, x, torch.zeros_like(x))))
        xs = torch.where(c, x, -torch.linalg.solve(H, rhs[..., None])[..., 0])
        inside = (xs.clamp(lob, hib) == xs).all(-1)
        d, fold = xs - x, f(x)
        sdotg = (g * d).sum(-1)
        accepted, xn = inside | done, torch.where(inside[:, None], xs, x)
        step = torch.ones(B, dtype=Qu.dtype, device=Qu.device)
        for _ in range(max_trials):                              # Armijo on the projected segment, for the trajectories that need it
            if bool(accepted.all()):
                break
            y = (x + step[:, None] * d).clamp(lob, hib)
            ok = ~accepted & (sdotg < 0) & (f(y) - fold <= 0.1 * step * sdotg)
            xn, accepted, step = torch.where(ok[:, None], y, xn), accepted | ok, step * 0.6
        xn = torch.where(done[:, None], x, xn)
        g2 = Qu + mv(Quu, xn)
        c2 = ((xn == lob) & (g2 > 0)) | ((xn == hib) & (g2 < 0))
        done = done | (inside & (c2 == c).all(-1)) | ~accepted
        x, g, c = xn, g2, c2                                     # (a trajectory that is done keeps its x, hence its set)
    return x, c


def torch_backward_box(A, Bm, lx, lu, Q, R, Qf, mu, u, lo, hi):
    B, T, nx, nu = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]
    Vx, Vxx = torch.zeros((B, nx, 1), dtype=A.dtype, device=A.device), Qf.expand(B, nx, nx).clone()
    ks, Ks = torch.zeros((B, T, nu, 1), dtype=A.dtype, device=A.device), torch.zeros((B, T, nu, nx), dtype=A.dtype, device=A.device)
    cs = torch.zeros((B, T, nu), dtype=torch.bool, device=A.device)
    eye, eyeb = mu * torch.eye(nu, dtype=A.dtype, device=A.device), torch.eye(nu, dtype=A.dtype, device=A.device).expand(B, nu, nu)
    for t in range(T - 1, -1, -1):
        At, Bt = A[:, t], Bm[:, t]
        AT, BT = At.transpose(1, 2), Bt.transpose(1, 2)
        Qx, Qu = lx[:, t, :, None] + AT @ Vx, lu[:, t, :, None] + BT @ Vx
        Qxx, Quu, Qux = Q + AT @ Vxx @ At, R + BT @ Vxx @ Bt + eye, BT @ Vxx @ At
        lob, hib = lo - u[:, t], hi - u[:, t]
        x, c = torch_box_qp(Quu, Qu[..., 0], lob, hib)
        H = torch.where(c[:, :, None] | c[:, None, :], eyeb, Quu)    # the polish on the final set
        xc = torch.where(c, x, torch.zeros_like(x))[..., None]
        rhs = torch.where(c[:, :, None], torch.zeros((B, nu, nx + 1), dtype=A.dtype, device=A.device), torch.cat([Qux, Qu + Quu @ xc], dim=2))
        X = -torch.linalg.solve(H, rhs)
        K = X[:, :, :nx]
        k = torch.where(c, x, X[:, :, nx]).clamp(lob, hib)[..., None]
        ks[:, t], Ks[:, t], cs[:, t] = k, K, c
        KT = K.transpose(1, 2)
        Vx = Qx + KT @ Quu @ k + KT @ Qu + Qux.transpose(1, 2) @ k
        Vxx = Qxx + KT @ Quu @ K + KT @ Qux + Qux.transpose(1, 2) @ K
        Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
    return ks[..., 0], Ks, cs


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
    ap.add_argument("--box-windows", type=int, default=3, help="windows of the control-limited rows (their torch loop is slow)")
    ap.add_argument("--bound", type=float, default=0.5, help="the box of the control-limited rows: lo = -bound, hi = 1.25 bound")
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
        # the control-limited pass: against its torch restatement with a box that binds, and against the unconstrained kernel with one that never does
        lo, hi = -args.bound, 1.25 * args.bound
        ub = u.clamp(lo, hi)
        box_call = lambda lo, hi: lqr_backward(data, A, Bm, lx=lx, lu=lu, lxx=Q, luu=R, VxxT=Qf, mu=1e-6, u=ub, lo=lo, hi=hi)
        bsol = box_call(lo, hi)
        kb, Kb, cb = torch_backward_box(A, Bm, lx, lu, Q, R, Qf, 1e-6, ub, lo, hi)
        bits = ((bsol.clamped[..., None] >> torch.arange(nu, device=dev, dtype=torch.int32)) & 1).bool()
        box = compare(lambda: box_call(lo, hi), lambda: torch_backward_box(A, Bm, lx, lu, Q, R, Qf, 1e-6, ub, lo, hi), args.box_windows)
        free = compare(lambda: box_call(-1e30, 1e30), lambda: lqr_backward(data, A, Bm, lx=lx, lu=lu, lxx=Q, luu=R, VxxT=Qf, mu=1e-6), args.windows)
        box_row = {"bound": args.bound, "box": box, "status_nonzero": int((bsol.status != 0).sum()), "qp_iters_max": int(bsol.qp_iters.max()),
                   "clamped_fraction": float(bits.double().mean()), "clamped_sets_equal_torch": bool((bits == cb).all()),
                   "K_kernel_vs_torch_rel": float((bsol.K - Kb).abs().max() / Kb.abs().max()),
                   "never_binding_vs_unconstrained": {"box_kernel": free["kernel"], "unconstrained_kernel": free["torch"], "ratio": 1.0 / free["speedup"]}}
        print(f"{name} B={B} T={T}: box backward {box['kernel']['median_ms']:.3f} ms vs torch {box['torch']['median_ms']:.1f} ms; never-binding box "
              f"{free['kernel']['median_ms']:.3f} ms vs unconstrained {free['torch']['median_ms']:.3f} ms", file=sys.stderr, flush=True)
        flop = flops_per_step(nx, nu) * T * B
        rows.append({"model": name, "nx": nx, "nu": nu, "B": B, "T": T, "backward": back, "candidates": cnd, "backward_box": box_row, "K_kernel_vs_torch_rel": agree,
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
