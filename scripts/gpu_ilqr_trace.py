"""One iLQR iteration of the cart-pole with nothing read back in between, for a ``rocprofv3 --kernel-trace --memory-copy-trace`` run,
and the digest of that run's CSV files.

The iteration is ``linearize_rollout`` -> cost expansion (torch) -> ``lqr_backward`` -> ``lqr_candidates`` -> ``rollout`` (one environment
per step size) -> cost of every candidate and the choice of the best one (torch, on the device).  Two warm-up iterations run first;
the traced one is separated from them and from the final read-back by a device synchronise and a pause of --gap seconds, so that
the digest finds it as the last burst of kernels that holds a ``k_lqr_backward`` dispatch.  With ``--cost kernel`` the cost, its
expansion and the choice come from ``trajectory_cost`` / ``select_candidates`` (the nominal controls updated in place) instead of torch.

    rocprofv3 --kernel-trace --memory-copy-trace --hip-runtime-trace -d DIR -o ilqr --output-format csv -- python scripts/gpu_ilqr_trace.py
    python scripts/gpu_ilqr_trace.py --digest DIR > profiles/lqr_ilqr_iteration_trace.log
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U_MAX = 4.0


def run(args):
    import torch

    from mujoco_template_amd import linearize_rollout, lqr_backward, lqr_candidates, mj, rollout, select_candidates, trajectory_cost

    T, K = args.horizon, args.alphas
    dev, f64 = torch.device("cuda"), torch.float64
    model = mj.MjModel.from_xml_path(os.path.join(ROOT, "models", "cartpole.xml"))
    nq, nv, nu = model.nq, model.nv, model.nu
    nx = 2 * nv
    nominal, search = mj.MjData(model, batch=1, dtype="float64"), mj.MjData(model, batch=K, dtype="float64")
    x0 = torch.zeros(1 + nq + nv, dtype=f64, device=dev)
    x0[2] = 0.3
    Q = torch.diag(torch.tensor([0.5, 10.0, 0.05, 0.1], dtype=f64)).to(dev)
    Qf, R = 20.0 * Q, 0.01 * torch.eye(nu, dtype=f64, device=dev)
    alphas = torch.cat([torch.tensor([0.0]), torch.logspace(0, -3, K - 1)]).to(dev, f64)
    lo, hi = torch.full((nu,), -U_MAX, dtype=f64, device=dev), torch.full((nu,), U_MAX, dtype=f64, device=dev)
    mu = torch.full((1,), 1e-6, dtype=f64, device=dev)
    lxx = Q.expand(T, nx, nx).clone()
    lxx[0] = 0
    lxx = lxx[None]

    def cost(state, u):
        x = state[..., 1:]
        run_ = 0.5 * torch.einsum("bti,ij,btj->b", x[:, :-1], Q, x[:, :-1]) + 0.5 * torch.einsum("bti,ij,btj->b", u, R, u)
        return run_ + 0.5 * torch.einsum("bi,ij,bj->b", x[:, -1], Qf, x[:, -1])

    def iteration(u):
        """Everything stays on the device: returns the next nominal controls, the candidates' costs and the status word as tensors."""
        state, _, A, Bm = linearize_rollout(model, nominal, u, initial_state=x0)
        xs = torch.cat([x0[None, 1:], state[0, :, 1:]])
        lx = xs[:T] @ Q
        lx[0] = 0
        sol = lqr_backward(nominal, A, Bm, lx=lx[None], lu=u @ R, lxx=lxx, luu=R, VxT=Qf @ xs[T], VxxT=Qf, mu=mu)
        cand = lqr_candidates(nominal, A, Bm, sol.k, sol.K, u, alphas, lo=lo, hi=hi)[0]
        st, _ = rollout(model, search, cand, initial_state=x0)
        c = cost(st, cand)
        best = torch.argmin(torch.nan_to_num(c, nan=float("inf")))
        return cand.index_select(0, best[None]), c, sol.status

    x_goal = torch.zeros(nq + nv, dtype=f64, device=dev)
    lxxK = lxx.expand(K, T, nx, nx)

    def iteration_kernel(u):
        """The same iteration on trajectory_cost / select_candidates: u is updated in place."""
        state, _, A, Bm = linearize_rollout(model, nominal, u, initial_state=x0)
        c0 = trajectory_cost(nominal, state, u, initial_state=x0, Q=lxx, R=R, Qf=Qf, x_ref=x_goal)
        sol = lqr_backward(nominal, A, Bm, lx=c0.lx, lu=c0.lu, lxx=lxx, luu=R, VxT=c0.VxT, VxxT=Qf, mu=mu)
        cand = lqr_candidates(nominal, A, Bm, sol.k, sol.K, u, alphas, lo=lo, hi=hi)
        st, _ = rollout(model, search, cand[0], initial_state=x0)
        cc = trajectory_cost(search, st, cand[0], initial_state=x0, Q=lxxK, R=R, Qf=Qf, x_ref=x_goal, gradients=False)
        select_candidates(nominal, cc.cost[None], cand, out=u)
        return u, cc.cost, sol.status

    if args.cost == "kernel":
        iteration = iteration_kernel
    u = torch.zeros((1, T, nu), dtype=f64, device=dev)
    for _ in range(2):                                           # warm-up: allocations, kernel loading, the FD scratch
        u, c, status = iteration(u)
    torch.cuda.synchronize()
    time.sleep(args.gap)
    u, c, status = iteration(u)                                  # the traced iteration: enqueued back to back, nothing read
    torch.cuda.synchronize()
    time.sleep(args.gap)
    print(f"traced iteration: best cost {float(c.min()):.6f}, status {int(status[0])}", flush=True)       # the read-back, after the pause


def _rows(path_glob):
    out = []
    for path in glob.glob(path_glob, recursive=True):
        with open(path, newline="") as fh:
            out += list(csv.DictReader(fh))
    return out


def digest(d, gap_s):
    kern = sorted(_rows(os.path.join(d, "**", "*kernel_trace.csv")), key=lambda r: int(r["Start_Timestamp"]))
    copies = _rows(os.path.join(d, "**", "*memory_copy_trace.csv"))
    if not kern:
        raise SystemExit(f"no kernel trace under {d}")
    bursts, cur = [], [kern[0]]
    for r in kern[1:]:
        if int(r["Start_Timestamp"]) - int(cur[-1]["End_Timestamp"]) > gap_s * 0.5e9:
            bursts.append(cur); cur = [r]
        else:
            cur.append(r)
    bursts.append(cur)
    with_lqr = [b for b in bursts if any("k_lqr_backward" in r["Kernel_Name"] for r in b)]
    win = with_lqr[-1]
    t0, t1 = int(win[0]["Start_Timestamp"]), max(int(r["End_Timestamp"]) for r in win)
    print("# rocprofv3 --kernel-trace --memory-copy-trace --hip-runtime-trace -- python scripts/gpu_ilqr_trace.py   (its own run, no counters)")
    if any("k_traj_cost" in r["Kernel_Name"] for r in win):
        print("# --cost kernel: the cost, its expansion and the choice are trajectory_cost / select_candidates (k_traj_*)")
    print("# cart-pole iLQR, T = 100, 16 step sizes, float64: ONE iteration (linearize_rollout -> lqr_backward -> lqr_candidates -> rollout -> choice of")
    print("# the best candidate), enqueued back to back after two warm-up iterations; window = first to last kernel of that iteration")
    print()
    print(f"kernel bursts in the run: {len(bursts)}, of which {len(with_lqr)} hold a k_lqr_backward dispatch (2 warm-up iterations in one burst + the traced one)")
    print(f"window: {len(win)} dispatches, {(t1 - t0) / 1e3:.1f} us from the first kernel's start to the last kernel's end")
    print()
    print("dispatches in the window, in order (torch's own kernels folded into one line per run of them):")
    ours, run_n, run_t = ("mjb_k", "k_fd", "k_lqr", "k_traj", "k_obs", "k_step", "k_prm", "k_reset"), 0, 0.0

    def flush():
        nonlocal run_n, run_t
        if run_n:
            print(f"   {run_n:3d} x torch kernels                                    {run_t:9.1f} us")
        run_n, run_t = 0, 0.0

    for r in win:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if any(k in name for k in ours) or "copyBuffer" in name:
            flush()
            short = name.split("(")[0].replace("void ", "").replace("mjb::", "")
            print(f"     1 x {short[:52]:52s} {us:9.1f} us   +{(int(r['Start_Timestamp']) - t0) / 1e3:9.1f} us")
        else:
            run_n += 1; run_t += us
    flush()
    print()
    inside = [c for c in copies if int(c["End_Timestamp"]) >= t0 and int(c["Start_Timestamp"]) <= t1]
    by_dir = {}
    for c in copies:
        by_dir[c["Direction"]] = by_dir.get(c["Direction"], 0) + 1
    print(f"memory copies in the whole run, by direction: {by_dir if by_dir else 'none'}")
    print(f"memory copies inside the window: {len(inside)}")
    for c in inside:
        print(f"   {c['Direction']}  +{(int(c['Start_Timestamp']) - t0) / 1e3:.1f} us  {(int(c['End_Timestamp']) - int(c['Start_Timestamp'])) / 1e3:.1f} us")
    d2h = [c for c in inside if "DEVICE_TO_HOST" in c["Direction"].upper() or c["Direction"].upper().endswith("DTOH")]
    print(f"device-to-host copies between the first and the last kernel of the iteration: {len(d2h)}")
    after = [c for c in copies if int(c["Start_Timestamp"]) > t1 and "DEVICE_TO_HOST" in c["Direction"].upper()]
    print(f"device-to-host copies after the window (the read-back of the cost and the status word, after the pause): {len(after)}")
    later = [r for b in bursts for r in b if int(r["Start_Timestamp"]) > t1]
    print(f"kernels after the window (the read-back): {[r['Kernel_Name'].split('(')[0][:40] for r in later]}")
    # the host side of the same span: HIP runtime calls from the end of the synchronise that closed the warm-up to the end of the window's last kernel
    api = sorted(_rows(os.path.join(d, "**", "*hip_api_trace.csv")), key=lambda r: int(r["Start_Timestamp"]))
    if api:
        syncs = [r for r in api if "Synchronize" in r["Function"] and int(r["End_Timestamp"]) <= t0]
        a = int(syncs[-1]["End_Timestamp"]) if syncs else int(api[0]["Start_Timestamp"])
        hist = {}
        for r in api:
            if a <= int(r["Start_Timestamp"]) <= t1:
                hist[r["Function"]] = hist.get(r["Function"], 0) + 1
        print()
        print("HIP runtime calls of the host between the synchronise that closed the warm-up and the end of the window's last kernel:")
        for fnc, n in sorted(hist.items(), key=lambda kv: -kv[1]):
            print(f"   {n:4d} x {fnc}")
        blocking = {f: n for f, n in hist.items() if "Synchronize" in f or ("Memcpy" in f and "Async" not in f) or "EventQuery" in f}
        print(f"calls that wait for the device or copy synchronously: {blocking if blocking else 'none'}"
              "   (the one hipDeviceSynchronize, if listed, is the script's own: it closes the iteration and is entered while the last kernels still run)")
        after_api = {}
        for r in api:
            if int(r["Start_Timestamp"]) > t1 and ("Memcpy" in r["Function"] or "Synchronize" in r["Function"]):
                after_api[r["Function"]] = after_api.get(r["Function"], 0) + 1
        print(f"after the window (the read-back): {after_api}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--alphas", type=int, default=16)
    ap.add_argument("--gap", type=float, default=0.5)
    ap.add_argument("--cost", choices=("kernel", "torch"), default="torch")
    ap.add_argument("--digest", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.digest:
        digest(args.digest, args.gap)
    else:
        run(args)


if __name__ == "__main__":
    main()
