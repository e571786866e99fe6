"""iLQR on the cart-pole with ``linearize_rollout``: trajectory optimisation that never leaves the GPU between its three phases.

Each iteration (horizon T, one nominal control sequence):
  linearise  ``linearize_rollout`` - the nominal rollout and (A_t, B_t) at every step of it, two submissions;
  backward   the Riccati recursion -> feed-forward k_t and gains K_t: ``lqr_backward``, one kernel launch (--backward kernel, the
             default), or the loop of small torch float64 operations it replaces (--backward torch);
  forward    a line search over --alphas step sizes as ONE ``rollout`` (one environment per alpha).  The rollout is open loop, so
             the candidate controls come from the closed loop run on the LINEARISED dynamics: dx' = A dx + B du,
             du = alpha k + K dx (``lqr_candidates``, one launch; with --backward torch a second torch loop); the true cost of each
             candidate is evaluated on the simulated states and the best one is kept.
  cost       --cost kernel (the default with --backward kernel): the trajectory cost, its expansion lx / lu / VxT and the choice of the
             step come from ``trajectory_cost`` and ``select_candidates``; the nominal controls are updated in place through ``out=``,
             the per-iteration costs stay on the GPU and are read once at the end - apart from the synchronises that close the timed
             phases, an iteration never waits for the GPU.  --cost torch: the einsum cost, ``xs @ Q`` / ``u @ R`` / ``Qf @ xs[T]`` and
             a host ``argmin``, as before.
  limits     --limits clamp (the default): the backward pass does not know the actuator limit U_MAX, only the candidates are clamped
             to it; --limits box: ``lqr_backward(..., u=u, lo=-U_MAX, hi=U_MAX)``, the control-limited pass (zero gains and the bound
             itself as feed-forward for a saturated control), and the same clamped candidates.
The pole starts tilted by --tilt rad; the cost asks for the upright pole at the origin.  Prints one JSON line: cost per iteration,
the tilt at the end of the final trajectory and the wall time of each phase (each closed by a device synchronise).

    python scripts/gpu_ilqr_cartpole.py [--horizon 100] [--iters 15] [--alphas 16] [--tilt 0.3] [--backward kernel|torch] [--cost kernel|torch] [--limits clamp|box] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mujoco_template_amd import linearize_rollout, lqr_backward, lqr_candidates, mj, rollout, select_candidates, trajectory_cost  # noqa: E402

XML = os.path.join(ROOT, "models", "cartpole.xml")
U_MAX = 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--alphas", type=int, default=16)
    ap.add_argument("--tilt", type=float, default=0.3)
    ap.add_argument("--backward", choices=("kernel", "torch"), default="kernel")
    ap.add_argument("--cost", choices=("kernel", "torch"), default=None, help="default: kernel with --backward kernel, torch otherwise")
    ap.add_argument("--limits", choices=("clamp", "box"), default="clamp",
                    help="clamp: the backward pass ignores U_MAX and the candidates are clamped to it; box: the control-limited backward pass "
                         "(lqr_backward with u, lo, hi) as well; needs --backward kernel")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.limits == "box" and args.backward != "kernel":
        raise SystemExit("--limits box is the kernel's control-limited pass: it needs --backward kernel")
    if args.cost is None:
        args.cost = "kernel" if args.backward == "kernel" else "torch"
    if args.cost == "kernel" and args.backward != "kernel":
        raise SystemExit("--cost kernel feeds lqr_backward: it needs --backward kernel")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the rollouts and linearisations run on the MI355X")
    T, K = args.horizon, args.alphas
    dev, f64 = torch.device("cuda"), torch.float64
    model = mj.MjModel.from_xml_path(XML)
    nq, nv, nu = model.nq, model.nv, model.nu
    nx = 2 * nv
    nominal = mj.MjData(model, batch=1, dtype="float64")
    search = mj.MjData(model, batch=K, dtype="float64")
    x0 = torch.zeros(1 + nq + nv, dtype=f64)
    x0[2] = args.tilt                                                          # time, slider, hinge, slider vel, hinge vel
    Q = torch.diag(torch.tensor([0.5, 10.0, 0.05, 0.1], dtype=f64, device=dev))
    Qf = 20.0 * Q
    R = 0.01 * torch.eye(nu, dtype=f64, device=dev)
    alphas = torch.cat([torch.tensor([0.0]), torch.logspace(0, -3, K - 1)]).to(dev, f64)   # alpha 0: the nominal itself

    def cost(state, u):
        """[B] cost of states [B, T, 1+nq+nv] (after each step) under controls [B, T, nu]; the goal is the origin."""
        x = state[..., 1:]
        run = 0.5 * torch.einsum("bti,ij,btj->b", x[:, :-1], Q, x[:, :-1]) + 0.5 * torch.einsum("bti,ij,btj->b", u, R, u)
        return run + 0.5 * torch.einsum("bi,ij,bj->b", x[:, -1], Qf, x[:, -1])

    u = torch.zeros((1, T, nu), dtype=f64, device=dev)
    costs, split = [], {"linearise": 0.0, "backward": 0.0, "forward": 0.0}
    reg = 1e-6
    # --cost kernel: the script's cost has no state term at t = 0, so Q is passed per step with Q_0 = 0; the goal is the origin
    x0_dev, x_goal = x0.to(dev), torch.zeros(nq + nv, dtype=f64, device=dev)
    Qt = Q.expand(T, nx, nx).clone()
    Qt[0] = 0
    Qt1, QtK = Qt[None], Qt[None].expand(K, T, nx, nx)
    cost_dev = torch.zeros(args.iters + 1, dtype=f64, device=dev)
    limits = dict(u=None, lo=-U_MAX, hi=U_MAX) if args.limits == "box" else {}
    clamped_steps = []                                                         # --limits box: per iteration, the steps whose control is clamped (a device tensor each)
    for it in range(args.iters):
        t0 = time.perf_counter()
        state, _, A, Bm = linearize_rollout(model, nominal, u, initial_state=x0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if args.cost == "kernel":
            c0 = trajectory_cost(nominal, state, u, initial_state=x0_dev, Q=Qt1, R=R, Qf=Qf, x_ref=x_goal)
            cost_dev[it:it + 1].copy_(c0.cost)
            if limits:
                limits["u"] = u
            sol = lqr_backward(nominal, A, Bm, lx=c0.lx, lu=c0.lu, lxx=Qt1, luu=R, VxT=c0.VxT, VxxT=Qf, mu=reg, **limits)
            if limits:
                clamped_steps.append((sol.clamped != 0).sum())
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            cand = lqr_candidates(nominal, A, Bm, sol.k, sol.K, u, alphas, lo=-U_MAX, hi=U_MAX)
            st, _ = rollout(model, search, cand[0], initial_state=x0)
            cc = trajectory_cost(search, st, cand[0], initial_state=x0_dev, Q=QtK, R=R, Qf=Qf, x_ref=x_goal, gradients=False)
            select_candidates(nominal, cc.cost[None], cand, out=u)             # u <- the best candidate (a NaN rollout costs +inf)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            split["linearise"] += t1 - t0; split["backward"] += t2 - t1; split["forward"] += t3 - t2
            continue
        costs.append(float(cost(state, u)[0]))
        xs = torch.cat([x0[1:].to(dev)[None], state[0, :, 1:]])                # [T + 1, nx]: x_t before step t, x_T the last state
        if args.backward == "kernel":
            lx = (xs[:T] @ Q).clone()
            lx[0] = 0                                                          # the script's cost has no state term at t = 0
            lxx = Q.expand(T, nx, nx).clone()
            lxx[0] = 0
            if limits:
                limits["u"] = u
            sol = lqr_backward(nominal, A, Bm, lx=lx[None], lu=u @ R, lxx=lxx[None], luu=R, VxT=Qf @ xs[T], VxxT=Qf, mu=reg, **limits)
            if limits:
                clamped_steps.append((sol.clamped != 0).sum())
        else:
            A, Bm = A[0], Bm[0]
            Vx, Vxx = Qf @ xs[T], Qf.clone()
            ks, Ks = torch.zeros((T, nu), dtype=f64, device=dev), torch.zeros((T, nu, nx), dtype=f64, device=dev)
            for t in range(T - 1, -1, -1):
                lx = Q @ xs[t] if t > 0 else torch.zeros(nx, dtype=f64, device=dev)
                Qx, Qu = lx + A[t].T @ Vx, R @ u[0, t] + Bm[t].T @ Vx
                Qxx, Quu, Qux = (Q if t > 0 else 0 * Q) + A[t].T @ Vxx @ A[t], R + Bm[t].T @ Vxx @ Bm[t] + reg * torch.eye(nu, dtype=f64, device=dev), Bm[t].T @ Vxx @ A[t]
                ks[t], Ks[t] = -torch.linalg.solve(Quu, Qu), -torch.linalg.solve(Quu, Qux)
                Vx = Qx + Ks[t].T @ Quu @ ks[t] + Ks[t].T @ Qu + Qux.T @ ks[t]
                Vxx = Qxx + Ks[t].T @ Quu @ Ks[t] + Ks[t].T @ Qux + Qux.T @ Ks[t]
                Vxx = 0.5 * (Vxx + Vxx.T)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if args.backward == "kernel":
            cand = lqr_candidates(nominal, A, Bm, sol.k, sol.K, u, alphas, lo=-U_MAX, hi=U_MAX)[0]
        else:
            dx = torch.zeros((K, nx), dtype=f64, device=dev)                       # closed loop on the linearised dynamics, all alphas at once
            cand = torch.empty((K, T, nu), dtype=f64, device=dev)
            for t in range(T):
                du = alphas[:, None] * ks[t][None] + dx @ Ks[t].T
                cand[:, t] = (u[0, t][None] + du).clamp(-U_MAX, U_MAX)
                dx = dx @ A[t].T + (cand[:, t] - u[0, t][None]) @ Bm[t].T
        st, _ = rollout(model, search, cand, initial_state=x0)
        c = cost(st, cand)
        best = int(torch.argmin(torch.nan_to_num(c, nan=float("inf"))))
        u = cand[best:best + 1].clone()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        split["linearise"] += t1 - t0; split["backward"] += t2 - t1; split["forward"] += t3 - t2
    state, _ = rollout(model, nominal, u, initial_state=x0)
    if args.cost == "kernel":
        cost_dev[args.iters:].copy_(trajectory_cost(nominal, state, u, initial_state=x0_dev, Q=Qt1, R=R, Qf=Qf, x_ref=x_goal, gradients=False).cost)
        costs = cost_dev.tolist()                                              # the one host read of the costs
    else:
        costs.append(float(cost(state, u)[0]))
    res = {"backward": args.backward, "cost": args.cost, "limits": args.limits, "u_max": U_MAX, "clamped_steps_per_iteration": [int(c) for c in clamped_steps],
           "iterations_to_within_1e-3_of_final": next(i for i, c in enumerate(costs) if c <= costs[-1] * (1 + 1e-3)), "horizon": T, "iterations": args.iters, "alphas": K, "tilt0_rad": args.tilt, "cost_per_iteration": costs,
           "final_tilt_rad": float(state[0, -1, 2]), "final_slider_m": float(state[0, -1, 1]),
           "wall_s": {k: v for k, v in split.items()}, "wall_share": {k: v / sum(split.values()) for k, v in split.items()}}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
