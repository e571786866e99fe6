"""``mjb_lqr_backward`` / ``mjb_lqr_candidates`` on the GPU (``mt.lqr_backward`` / ``mt.lqr_candidates``).

The yardstick is never the kernel: the numpy restatement of ``tests/lqr_common.py`` in long double is the truth, the same restatement
in float64 measures what float64 arithmetic alone loses, and every bound is 8 x that measure (floor 1e-13; 1e-11 against scipy's
``solve_discrete_are``).  Both values of every comparison go through ``tests.conftest.measured`` (profiles/lqr_parity_measured.json
keeps the recorded pairs)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import lqr_common as lc
from tests.conftest import MODELS, measured

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch

    from mujoco_template_amd import mj

    model = mj.MjModel.from_xml_path(MODELS["cartpole"])
    data = mj.MjData(model, batch=1, dtype="float64")
    return torch, model, data


def _dev(torch, x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


def _np(res):
    return {"k": res.k.cpu().numpy(), "K": res.K.cpu().numpy(), "dV": res.dV.cpu().numpy(), "V0x": res.V0x.cpu().numpy(),
            "V0xx": res.V0xx.cpu().numpy(), "status": res.status.cpu().numpy()}


def _compare(tag, got, truth, f64, floor=lc.FLOOR):
    for key in lc.OUTPUTS:
        mine, numpy64 = lc.rel_err(got[key], truth[key]), lc.rel_err(f64[key], truth[key])
        print(f"{tag} {key}: kernel {mine:.3e}  float64 numpy {numpy64:.3e}  bound {lc.bound(numpy64, floor):.3e}")
        measured(f"lqr/{tag}/{key}", mine, lc.bound(numpy64, floor), f"(float64 numpy restatement: {numpy64:.3e})")


# ---- 1. the fragment maps of the f64 MFMA ---------------------------------------------------------------------------------------------
# Both variants of the probe at their edges: M = 1 / 15 / 16 with one wave (N <= 64 stays within its four tiles), 17 / 33 / 48 / 49 /
# 64 with four; N and K below, at and above a tile (16) and a k-step (4).
PROBE_FIRST = [(54, 21, 54), (7, 3, 7), (64, 32, 64), (16, 64, 5), (3, 17, 1)]
PROBE_ALL = PROBE_FIRST + [s for s in ((M, N, K) for M in (1, 15, 16, 17, 33, 48, 49, 64) for N in (1, 16, 17, 33, 64) for K in (1, 3, 4, 5, 64))
                           if s not in PROBE_FIRST]


@pytest.mark.parametrize("M,N,K", PROBE_ALL)
def test_mfma_map_on_exact_integers(ctx, M, N, K):
    """(M x K)(K x N) of small integers through the kernels' tile product equals numpy's bit for bit; asymmetric operands."""
    torch, _, data = ctx
    rng = np.random.default_rng(1)
    a = rng.integers(-9, 10, size=(K, M)).astype(np.float64)
    b = rng.integers(-9, 10, size=(K, N)).astype(np.float64)
    c = data.sim.lqr_gemm_tn(_dev(torch, a), _dev(torch, b)).cpu().numpy()
    assert np.array_equal(c, a.T @ b)


def test_probe_refuses_what_its_tile_slots_do_not_hold(ctx):
    """One wave holds four tiles and four waves sixteen; no tile beyond them is computed, so the entry point must refuse M or N above
    64 (tests/test_lqr_host.py enumerates that every shape up to there fits)."""
    from mujoco_template_amd.exceptions import ConfigError, TemplateError

    torch, _, data = ctx
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    for a, b in ((z(4, 65), z(4, 1)), (z(4, 1), z(4, 65)), (z(4, 16), z(4, 80))):
        with pytest.raises((ConfigError, TemplateError), match="must lie in"):
            data.sim.lqr_gemm_tn(a, b)


# ---- 2. the recursion against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense_TB", "permuted_BT"])
@pytest.mark.parametrize("nx,nu,T", lc.SIZES + lc.EDGE_BACKWARD)
def test_recursion_matches_the_restatement(ctx, nx, nu, T, layout):
    """B = 5 distinct systems per launch; from dense [T, B, ...] arrays, and from the permuted [B, T, ...] views of them (what
    linearize_rollout returns) with Q, R broadcast (one system's cost for all: both strides 0).  With ``lqr_common.EDGE_BACKWARD``
    every launch variant runs: k_lqr_backward<1, 8>, <1, 32> (nx <= 16 with nu > 8) and <4, 32>, and the horizons T = 1 and 2."""
    import mujoco_template_amd as mt

    torch, _, data = ctx
    B = 5
    p = lc.generate(nx, nu, T, B)
    if layout == "permuted_BT":                                  # Q, R shared: passed once
        p["Q"] = np.broadcast_to(p["Q"][0], p["Q"].shape).copy()
        p["VxxT"] = 20.0 * p["Q"]
    truth, f64 = lc.restate_batch(p, np.longdouble), lc.restate_batch(p, np.float64)
    assert (truth["status"] == 0).all()                          # every Quu positive definite: the inputs are benign
    A, Bm, lx, lu = (_dev(torch, p[k]) for k in ("A", "B", "lx", "lu"))
    if layout == "dense_TB":
        Q = _dev(torch, p["Q"]).unsqueeze(0).expand(T, B, nx, nx)
        R = _dev(torch, p["R"]).unsqueeze(0).expand(T, B, nu, nu)
        res = mt.lqr_backward(data, A, Bm, lx=lx, lu=lu, lxx=Q, luu=R, VxT=_dev(torch, p["VxT"]), VxxT=_dev(torch, p["VxxT"]), mu=p["mu"], time_major=True)
        assert res.K.shape == (T, B, nu, nx) and res.k.shape == (T, B, nu)
        got = _np(res)
        got["k"], got["K"] = got["k"].transpose(1, 0, 2), got["K"].transpose(1, 0, 2, 3)
    else:
        res = mt.lqr_backward(data, A.permute(1, 0, 2, 3), Bm.permute(1, 0, 2, 3), lx=lx.permute(1, 0, 2), lu=lu.permute(1, 0, 2),
                              lxx=_dev(torch, p["Q"][0]), luu=_dev(torch, p["R"][0]), VxT=_dev(torch, p["VxT"]), VxxT=_dev(torch, p["VxxT"][0]),
                              mu=torch.full((B,), p["mu"], dtype=torch.float64, device="cuda"))
        assert res.K.shape == (B, T, nu, nx) and res.k.shape == (B, T, nu)
        got = _np(res)
    assert got["status"].tolist() == [0] * B and got["V0xx"].shape == (B, nx, nx) and got["dV"].shape == (B, 2)
    _compare(f"{layout}/{nx}x{nu}x{T}", got, truth, f64)


@pytest.mark.parametrize("nx,nu", [(12, 4), (16, 9), (17, 9)])
def test_results_do_not_depend_on_the_batch_position(ctx, nx, nu):
    """One size per launch variant (<1, 8>, <1, 32>, <4, 32>): five systems in one launch against each system launched alone, every
    output bit for bit."""
    import mujoco_template_amd as mt

    torch, _, data = ctx
    T, B = 20, 5
    p = lc.generate(nx, nu, T, B)

    def run(keep):
        args = {k: _dev(torch, p[k][:, keep]).permute(1, 0, *range(2, p[k].ndim)) for k in ("A", "B", "lx", "lu")}
        n = len(keep)
        return _np(mt.lqr_backward(data, args["A"], args["B"], lx=args["lx"], lu=args["lu"], lxx=_dev(torch, p["Q"][keep]).unsqueeze(1).expand(n, T, nx, nx),
                                   luu=_dev(torch, p["R"][keep]).unsqueeze(1).expand(n, T, nu, nu), VxT=_dev(torch, p["VxT"][keep]),
                                   VxxT=_dev(torch, p["VxxT"][keep]), mu=p["mu"]))

    got = run(list(range(B)))
    assert got["status"].tolist() == [0] * B and np.isfinite(got["K"]).all() and np.abs(got["K"]).max() > 0
    for e in range(B):
        alone = run([e])
        for key in lc.OUTPUTS + ("status",):
            assert np.array_equal(got[key][e:e + 1], alone[key]), (e, key)


# ---- 3. the reference's DARE ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", [(4, 1), (12, 4)])
def test_riccati_limit_is_scipys_dare(ctx, nx, nu):
    import mujoco_template_amd as mt
    from scipy.linalg import solve_discrete_are

    torch, _, data = ctx
    T = 3200        # the closed-loop spectral radii of these systems are 0.9957 / 0.9936: at 1600 steps the recursion is still 1e-7 / 1e-9 from its limit
    p = lc.generate(nx, nu, T, 1, constant=True)
    p["lx"][:] = 0; p["lu"][:] = 0; p["VxxT"] = p["Q"].copy(); p["mu"] = 0.0
    A, Bm, Q, R = p["A"][0, 0], p["B"][0, 0], p["Q"][0], p["R"][0]
    P = solve_discrete_are(A, Bm, Q, R)
    Kd = -np.linalg.solve(R + Bm.T @ P @ Bm, Bm.T @ P @ A)
    f64 = lc.restate_batch(p, np.float64)
    At, Bt = _dev(torch, A).expand(1, T, nx, nx), _dev(torch, Bm).expand(1, T, nx, nu)          # constant (A, B): strides 0
    got = _np(mt.lqr_backward(data, At, Bt, lxx=_dev(torch, Q), luu=_dev(torch, R), VxxT=_dev(torch, Q), mu=0.0))
    assert got["status"][0] == 0
    for key, ref, mine, np64 in (("K_0", Kd, got["K"][0, 0], f64["K"][0, 0]), ("P", P, got["V0xx"][0], f64["V0xx"][0])):
        e_mine, e_np = lc.rel_err(mine, ref), lc.rel_err(np64, ref)
        print(f"DARE {(nx, nu)} {key}: kernel {e_mine:.3e}  float64 numpy recursion {e_np:.3e}")
        measured(f"lqr/dare/{nx}x{nu}/{key}", e_mine, lc.bound(e_np, lc.FLOOR_DARE), f"(float64 numpy recursion: {e_np:.3e})")


# ---- 4. on real linearisations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T,B,dtype", [("cartpole", 100, 1, "float64"), ("humanoid", 20, 4, "float32")])
def test_on_real_linearisations(name, T, B, dtype):
    """linearize_rollout's (A, B) views passed in place; the same bound against the restatement fed the same tensors."""
    import torch

    import mujoco_template_amd as mt
    from mujoco_template_amd import mj

    model = mj.MjModel.from_xml_path(MODELS[name])
    data = mj.MjData(model, batch=B, dtype=dtype)
    nu, nx = model.nu, 2 * model.nv
    gen = torch.Generator(device="cpu").manual_seed(3)
    u = (0.05 * torch.randn((B, T, nu), generator=gen, dtype=torch.float64)).to("cuda", torch.float32 if dtype == "float32" else torch.float64)
    _, _, A, Bm = mt.linearize_rollout(model, data, u)
    assert A.shape == (B, T, nx, nx) and (B == 1 or not A.is_contiguous())      # the permuted view of the [T, B, ...] blocks, read in place
    rng = np.random.default_rng(4)
    p = {"A": A.permute(1, 0, 2, 3).cpu().numpy(), "B": Bm.permute(1, 0, 2, 3).cpu().numpy(), "lx": rng.normal(size=(T, B, nx)),
         "lu": 0.1 * rng.normal(size=(T, B, nu)), "Q": np.broadcast_to(np.eye(nx), (B, nx, nx)).copy(), "R": np.broadcast_to(0.01 * np.eye(nu), (B, nu, nu)).copy(),
         "VxT": np.zeros((B, nx))}
    p["VxxT"] = 20.0 * p["Q"]
    if name == "cartpole":
        p["mu"] = 1e-6                                           # the iLQR script's value
        truth = lc.restate_batch(p, np.longdouble)
    else:                                                        # the smallest power of ten for which the long-double restatement finds every Quu positive definite
        for e10 in range(-12, 4):
            p["mu"] = 10.0 ** e10
            truth = lc.restate_batch(p, np.longdouble)
            if (truth["status"] == 0).all():
                break
        print(f"humanoid: mu = {p['mu']:g}")
    assert (truth["status"] == 0).all()
    f64 = lc.restate_batch(p, np.float64)
    res = mt.lqr_backward(data, A, Bm, lx=_dev(torch, p["lx"]).permute(1, 0, 2), lu=_dev(torch, p["lu"]).permute(1, 0, 2), lxx=_dev(torch, p["Q"][0]),
                          luu=_dev(torch, p["R"][0]), VxxT=_dev(torch, p["VxxT"][0]), mu=p["mu"])
    got = _np(res)
    assert (got["status"] == 0).all()
    _compare(f"linearised/{name}", got, truth, f64)


# ---- 5. an indefinite Quu ---------------------------------------------------------------------------------------------------------------------
def test_indefinite_quu_is_reported_not_propagated(ctx):
    import mujoco_template_amd as mt

    torch, _, data = ctx
    nx, nu, T, B, badenv = 7, 3, 12, 5, 2
    p = lc.generate(nx, nu, T, B)
    luu = p["R"].copy(); luu[badenv] = -np.eye(nu)
    mu = np.full(B, p["mu"]); mu[badenv] = 0.0
    q = dict(p); q["R"], q["mu"] = luu, mu
    assert lc.restate_batch(q, np.longdouble)["status"][badenv] == T

    def run(keep):
        args = {k: _dev(torch, p[k][:, keep]).permute(1, 0, *range(2, p[k].ndim)) for k in ("A", "B", "lx", "lu")}
        n = len(keep)
        return _np(mt.lqr_backward(data, args["A"], args["B"], lx=args["lx"], lu=args["lu"], lxx=_dev(torch, p["Q"][keep]).unsqueeze(1).expand(n, T, nx, nx),
                                   luu=_dev(torch, luu[keep]).unsqueeze(1).expand(n, T, nu, nu), VxxT=_dev(torch, p["VxxT"][keep]), mu=_dev(torch, mu[keep])))

    got = run(list(range(B)))
    assert got["status"].tolist() == [0, 0, T, 0, 0]
    for key in lc.OUTPUTS:
        assert np.array_equal(got[key][badenv], np.zeros_like(got[key][badenv])), key
        assert np.isfinite(got[key]).all(), key
    keep = [e for e in range(B) if e != badenv]
    alone = run(keep)
    for key in lc.OUTPUTS + ("status",):
        assert np.array_equal(got[key][keep], alone[key]), key


# ---- 6. candidates ------------------------------------------------------------------------------------------------------------------------------
def test_candidates(ctx):
    """Against the torch loop of scripts/gpu_ilqr_cartpole.py in float64 (the comparison) with the long-double restatement as truth;
    alpha = 0 with dx0 = 0 returns clamp(u) bitwise; the float32 output is the float64 output rounded once."""
    import mujoco_template_amd as mt

    torch, _, data = ctx
    nx, nu, T, B, na = 12, 4, 60, 3, 16
    p = lc.generate(nx, nu, T, B)
    sol = lc.restate_batch(p, np.float64)
    lo, hi = -0.8, 0.9
    u = np.clip(np.random.default_rng(5).normal(size=(B, T, nu)), lo, hi)                  # a nominal inside its bounds, some entries on them
    alphas = np.concatenate([[0.0], np.logspace(0, -3, na - 1)])
    A, Bm = _dev(torch, p["A"]).permute(1, 0, 2, 3), _dev(torch, p["B"]).permute(1, 0, 2, 3)
    k, K, ud, al = _dev(torch, sol["k"]), _dev(torch, sol["K"]), _dev(torch, u), _dev(torch, alphas)
    got = mt.lqr_candidates(data, A, Bm, k, K, ud, al, lo=lo, hi=hi)
    got32 = mt.lqr_candidates(data, A, Bm, k, K, ud, al, lo=lo, hi=hi, dtype=torch.float32)
    assert got.shape == (B, na, T, nu) and got32.dtype == torch.float32
    for e in range(B):
        dx = torch.zeros((na, nx), dtype=torch.float64, device="cuda")                      # the script's loop
        cand = torch.empty((na, T, nu), dtype=torch.float64, device="cuda")
        for t in range(T):
            du = al[:, None] * k[e, t][None] + dx @ K[e, t].T
            cand[:, t] = (ud[e, t][None] + du).clamp(lo, hi)
            dx = dx @ A[e, t].T + (cand[:, t] - ud[e, t][None]) @ Bm[e, t].T
        truth = lc.restate_candidates(p["A"][:, e], p["B"][:, e], sol["k"][e], sol["K"][e], u[e], alphas, None, np.full(nu, lo), np.full(nu, hi), np.longdouble)
        mine, loop = lc.rel_err(got[e].cpu().numpy(), truth), lc.rel_err(cand.cpu().numpy(), truth)
        print(f"candidates env {e}: kernel {mine:.3e}  torch float64 loop {loop:.3e}")
        measured(f"lqr/candidates/env{e}", mine, lc.bound(loop), f"(torch float64 loop: {loop:.3e})")
    assert torch.equal(got[:, 0], ud.clamp(lo, hi))
    assert torch.equal(got32, got.to(torch.float32))


def _candidates(torch, data, c, alphas, dx0, lo, hi, time_major=False, **kw):
    """``mt.lqr_candidates`` on a ``lqr_common.candidate_case``: the permuted [B, T, ...] views of its time-major arrays, or with
    ``time_major`` those arrays themselves.  lo / hi: None, a number or an array [nu]."""
    import mujoco_template_amd as mt

    perm = lambda x: x if time_major else x.permute(1, 0, *range(2, x.ndim))
    A, Bm, k, K, u = (perm(_dev(torch, c[key])) for key in ("A", "B", "k", "K", "u"))
    dev = lambda x: x if x is None or np.ndim(x) == 0 else _dev(torch, x)
    return mt.lqr_candidates(data, A, Bm, k, K, u, _dev(torch, alphas), dx0=None if dx0 is None else _dev(torch, dx0), lo=dev(lo), hi=dev(hi),
                             time_major=time_major, **kw)


@pytest.mark.parametrize("dx0_kind,bounds_kind", lc.CAND_VARIANTS)
@pytest.mark.parametrize("nx,nu,T,B,na", lc.CAND_SIZES)
def test_candidates_at_the_edge_sizes(ctx, nx, nu, T, B, na, dx0_kind, bounds_kind):
    """``lqr_common.CAND_SIZES`` x ``CAND_VARIANTS`` against the long-double restatement within 8 x the float64 restatement's own error
    (``lqr_common.judge_candidates``, which also asserts on the restatement that the variant clamps what it says).  A dx0, per
    trajectory or shared, changes the kernel's result; bounds that are all one number give the same bits passed as that number and
    as an array; ``time_major=True`` on the [T, B, ...] arrays is bitwise the call on their permuted views; the float32 output is the
    float64 one rounded once."""
    torch, _, data = ctx
    c = lc.candidate_case(nx, nu, T, B, na)
    dx0, lo, hi = lc.candidate_variant(c, dx0_kind, bounds_kind)
    res = _candidates(torch, data, c, c["alphas"], dx0, lo, hi)
    assert res.shape == (B, na, T, nu) and res.dtype == torch.float64
    lc.judge_candidates(c, res.cpu().numpy(), dx0_kind, bounds_kind, f"lqr/candidates/{nx}x{nu}x{T}x{B}x{na}/{dx0_kind}/{bounds_kind}", record=measured)
    if dx0 is not None:
        assert not torch.equal(res, _candidates(torch, data, c, c["alphas"], None, lo, hi))
    if bounds_kind != "per_actuator":
        number = lambda x: None if x is None else float(x[0])
        assert torch.equal(res, _candidates(torch, data, c, c["alphas"], dx0, number(lo), number(hi)))
    assert torch.equal(res, _candidates(torch, data, c, c["alphas"], dx0, lo, hi, time_major=True))
    res32 = _candidates(torch, data, c, c["alphas"], dx0, lo, hi, dtype=torch.float32)
    assert res32.dtype == torch.float32 and torch.equal(res32, res.to(torch.float32))


@pytest.mark.parametrize("nx,nu,T,B,na", lc.CAND_SIZES)
def test_candidates_zero_step_returns_the_clamped_nominal(ctx, nx, nu, T, B, na):
    """alpha = 0 with dx0 = 0 (absent, and given as zeros) and a nominal inside its bounds, some entries on them: clamp(u) = u bit for
    bit - dx stays 0."""
    torch, _, data = ctx
    c = lc.candidate_case(nx, nu, T, B, na)
    alphas = np.array([0.0]) if na == 1 else c["alphas"]
    want = _dev(torch, c["u"]).permute(1, 0, 2).clamp(lc.CAND_LO, lc.CAND_HI)
    assert alphas[0] == 0.0 and bool((want == lc.CAND_LO).any()) and bool((want == lc.CAND_HI).any())
    for dx0 in (None, np.zeros((B, nx)), np.zeros(nx)):
        got = _candidates(torch, data, c, alphas, dx0, lc.CAND_LO, lc.CAND_HI)
        assert torch.equal(got[:, 0], want)


# ---- 7. stream order, no host round trip ------------------------------------------------------------------------------------------------------
def test_chain_on_a_side_stream_needs_no_synchronise(ctx):
    """linearize_rollout -> lqr_backward -> lqr_candidates -> rollout enqueued back to back on a non-default stream equals, bitwise,
    the same chain with a synchronise after every call."""
    import mujoco_template_amd as mt
    from mujoco_template_amd import mj

    torch, model, nominal = ctx
    T, na = 50, 8
    nx, nu = 2 * model.nv, model.nu
    search = mj.MjData(model, batch=na, dtype="float64")
    x0 = torch.zeros(1 + model.nq + model.nv, dtype=torch.float64); x0[2] = 0.3
    Q = torch.diag(torch.tensor([0.5, 10.0, 0.05, 0.1], dtype=torch.float64, device="cuda"))
    R = 0.01 * torch.eye(nu, dtype=torch.float64, device="cuda")
    alphas = torch.cat([torch.tensor([0.0]), torch.logspace(0, -3, na - 1)]).to("cuda", torch.float64)
    u = 0.1 * torch.ones((1, T, nu), dtype=torch.float64, device="cuda")

    def chain(sync):
        wait = torch.cuda.synchronize if sync else (lambda: None)
        state, _, A, Bm = mt.linearize_rollout(model, nominal, u, initial_state=x0); wait()
        xs = torch.cat([x0[1:].to("cuda")[None], state[0, :-1, 1:]])
        sol = mt.lqr_backward(nominal, A, Bm, lx=(xs @ Q)[None], lu=u @ R, lxx=Q, luu=R, VxT=(state[0, -1, 1:] @ (20 * Q)), VxxT=20 * Q, mu=1e-6); wait()
        cand = mt.lqr_candidates(nominal, A, Bm, sol.k, sol.K, u, alphas, lo=-4.0, hi=4.0); wait()
        st, _ = mt.rollout(model, search, cand[0], initial_state=x0); wait()
        return st.clone(), sol.status.clone(), cand.clone()

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fast = chain(False)
    side.synchronize()
    with torch.cuda.stream(side):
        slow = chain(True)
    torch.cuda.synchronize()
    assert int(fast[1][0]) == 0 and torch.isfinite(fast[0]).all()
    assert float((fast[2][0, 1] - fast[2][0, 0]).abs().max()) > 0            # the gains did something
    for a, b in zip(fast, slow):
        assert torch.equal(a, b)


# ---- 8. argument checks ---------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_untouched(ctx):
    from mujoco_template_amd.exceptions import ConfigError, TemplateError

    torch, _, data = ctx
    sim = data.sim
    T, B, nx, nu = 3, 2, 4, 1
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    A, Bm, lx, lu, Q, R = z(T, B, nx, nx), z(T, B, nx, nu), z(T, B, nx), z(T, B, nu), torch.eye(nx, dtype=torch.float64, device="cuda"), torch.eye(nu, dtype=torch.float64, device="cuda")
    outs = {"k": torch.full((T, B, nu), 7.0, dtype=torch.float64, device="cuda"), "K": torch.full((T, B, nu, nx), 7.0, dtype=torch.float64, device="cuda"),
            "dV": torch.full((B, 2), 7.0, dtype=torch.float64, device="cuda"), "V0x": torch.full((B, nx), 7.0, dtype=torch.float64, device="cuda"),
            "V0xx": torch.full((B, nx, nx), 7.0, dtype=torch.float64, device="cuda"), "status": torch.full((B,), 7, dtype=torch.int32, device="cuda")}
    mu = z(1)
    host = np.zeros(T * B * nx * nx)

    def call(sizes=None, **override):
        arrays = {"A": (A.data_ptr(), B * nx * nx, nx * nx), "B": (Bm.data_ptr(), B * nx * nu, nx * nu), "lx": (lx.data_ptr(), B * nx, nx),
                  "lu": (lu.data_ptr(), B * nu, nu), "lxx": (Q.data_ptr(), 0, 0), "luu": (R.data_ptr(), 0, 0), "lux": (0, 0, 0),
                  "VxT": (lx.data_ptr(), 0, nx), "VxxT": (Q.data_ptr(), 0, 0), "mu": (mu.data_ptr(), 0, 0)}
        arrays.update(override)
        s = {"T": T, "batch": B, "nx": nx, "nu": nu}
        s.update(sizes or {})
        sim.lqr_backward(s, arrays, {k: v.data_ptr() for k, v in outs.items()})

    call()                                                       # the well-formed call goes through
    torch.cuda.synchronize()
    assert outs["status"].tolist() == [0, 0]
    for v in outs.values():
        v.fill_(7)
    # an A one element too short: the extent is measured against what hipMemGetAddressRange reports behind the pointer (torch's
    # caching allocator hands out pieces of larger blocks), so A is placed to end one element past that block
    from tests.test_gpu_rollout_ctrl import _hip_runtime

    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert _hip_runtime().hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(A.data_ptr())) == 0
    a_ok = (base.value + size.value - A.data_ptr()) // 8
    short = A.data_ptr() + 8 * (a_ok - T * B * nx * nx + 1)
    call(A=(short - 8, B * nx * nx, nx * nx))                    # ending exactly at the end of the block: accepted
    torch.cuda.synchronize()
    for v in outs.values():
        v.fill_(7)
    bad = [("nx must lie in", dict(sizes={"nx": 65})), ("nu must lie in", dict(sizes={"nu": 33})), ("T must be", dict(sizes={"T": 0})),
           ("not device-accessible", dict(A=(host.ctypes.data, B * nx * nx, nx * nx))), ("strides must be", dict(A=(A.data_ptr(), -1, nx * nx))),
           ("beyond its allocation", dict(A=(short, B * nx * nx, nx * nx))), ("lxx is NULL", dict(lxx=(0, 0, 0)))]
    for msg, kw in bad:
        with pytest.raises((ConfigError, TemplateError), match=msg):
            call(**kw)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == 7).all()), k
