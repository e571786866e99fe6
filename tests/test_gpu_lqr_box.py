"""``mjb_lqr_backward_box`` on the GPU, through ``mt.lqr_backward(..., u=, lo=, hi=)``.

The yardstick is never the kernel: the numpy restatement of ``tests/lqr_box_common.py`` in long double is the truth, the same
restatement in float64 measures what float64 arithmetic alone loses, every bound is 8 x that measure (floor 1e-13) and goes through
``tests.conftest.measured``.  Before a test looks at the kernel it asserts on the restatement that both precisions find the same
clamped sets with no decision closer than 1e-6 to flipping (``lqr_box_common.preconditions``)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import lqr_box_common as bc
from tests import lqr_common as lc
from tests.conftest import MODELS, measured

pytestmark = pytest.mark.gpu

# the last three: nu > nx in k_lqr_backward_box<1, 32>, that variant with every tile slot of its wave used, and the smallest system
# (<1, 8>).  Their long-double references keep every active-set decision at least 5e-6 from its threshold (MARGIN_MIN is 1e-6) with
# the seeds and horizons as they stand: nothing had to be changed for the module's rule.
SIZES = [(4, 1, 200), (7, 3, 64), (12, 4, 200), (16, 12, 40), (54, 21, 30), (64, 32, 12), (3, 9, 40), (16, 32, 12), (1, 1, 20)]
B = 3


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
    return {k: getattr(res, k).cpu().numpy() for k in res._fields}


def _run(torch, data, p, layout, lo="p", hi="p", luu=None, mu=None, keep=None):
    """The kernel on a ``box_inputs`` dict, outputs as numpy [B, T, ...].  dense_TB: [T, B, ...] tensors, Q, R expanded per step;
    permuted_BT: the permuted [B, T, ...] views of them, with Q, R passed once when the dict's systems share them."""
    import mujoco_template_amd as mt

    keep = list(range(p["A"].shape[1])) if keep is None else keep
    n, T, nx, nu = len(keep), p["A"].shape[0], p["A"].shape[2], p["B"].shape[3]
    lo = p["lo"] if isinstance(lo, str) else lo
    hi = p["hi"] if isinstance(hi, str) else hi
    lo, hi = (None if x is None else _dev(torch, x) for x in (lo, hi))
    luu = p["R"] if luu is None else luu
    mu = np.broadcast_to(np.asarray(p["mu"] if mu is None else mu, dtype=np.float64), (p["A"].shape[1],))[keep]
    A, Bm, lx, lu, u = (_dev(torch, p[k][:, keep]) for k in ("A", "B", "lx", "lu", "u"))
    kw = dict(VxT=_dev(torch, p["VxT"][keep]), mu=_dev(torch, mu), lo=lo, hi=hi)
    if layout == "dense_TB":
        Q = _dev(torch, p["Q"][keep]).unsqueeze(0).expand(T, n, nx, nx)
        R = _dev(torch, luu[keep]).unsqueeze(0).expand(T, n, nu, nu)
        got = _np(mt.lqr_backward(data, A, Bm, lx=lx, lu=lu, lxx=Q, luu=R, VxxT=_dev(torch, p["VxxT"][keep]), u=u, time_major=True, **kw))
        got["k"], got["K"] = got["k"].transpose(1, 0, 2), got["K"].transpose(1, 0, 2, 3)
        if "clamped" in got:
            got["clamped"] = got["clamped"].T
        return got
    perm = lambda x: x.permute(1, 0, *range(2, x.ndim))
    shared = all(np.array_equal(p["Q"][e], p["Q"][keep[0]]) and np.array_equal(luu[e], luu[keep[0]]) for e in keep)
    if shared:                                                   # one cost for all: passed once, both strides 0
        Q, R, Vf = _dev(torch, p["Q"][keep[0]]), _dev(torch, luu[keep[0]]), _dev(torch, p["VxxT"][keep[0]])
    else:
        Q, R = _dev(torch, p["Q"][keep]).unsqueeze(1).expand(n, T, nx, nx), _dev(torch, luu[keep]).unsqueeze(1).expand(n, T, nu, nu)
        Vf = _dev(torch, p["VxxT"][keep])
    res = mt.lqr_backward(data, perm(A), perm(Bm), lx=perm(lx), lu=perm(lu), lxx=Q, luu=R, VxxT=Vf, u=perm(u), **kw)
    if lo is not None or hi is not None:
        assert isinstance(res, mt.LqrBoxResult) and res.K.shape == (n, T, nu, nx) and res.clamped.shape == (n, T) and res.qp_iters.shape == (n,)
    return _np(res)


def _structure(got, p, lo, hi):
    """k bitwise the bound where clamped and inside the box everywhere; the clamped rows of K zero.  Returns the mask [B, T, nu]."""
    nu = lo.shape[0]
    u = p["u"].transpose(1, 0, 2)
    lob, hib = lo[None, None] - u, hi[None, None] - u
    cm = ((np.ascontiguousarray(got["clamped"])[..., None].view(np.uint32) >> np.arange(nu, dtype=np.uint32)) & 1).astype(bool)
    assert cm.any() and not cm.all()
    assert ((got["k"] == lob) | (got["k"] == hib))[cm].all()
    assert (got["k"] >= lob).all() and (got["k"] <= hib).all()
    assert (got["K"][cm] == 0).all() and (np.abs(got["K"][~cm]).max(axis=-1) > 0).all()
    return cm


def _compare(tag, got, truth, f64):
    for key in lc.OUTPUTS:
        mine, numpy64 = lc.rel_err(got[key], truth[key]), lc.rel_err(f64[key], truth[key])
        print(f"{tag} {key}: kernel {mine:.3e}  float64 numpy {numpy64:.3e}  bound {lc.bound(numpy64):.3e}")
        measured(f"lqr_box/{tag}/{key}", mine, lc.bound(numpy64), f"(float64 numpy restatement: {numpy64:.3e})")


# ---- 1, 2. the recursion against the restatement, and its exact structure ---------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense_TB", "permuted_BT"])
@pytest.mark.parametrize("b", bc.BOUNDS)
@pytest.mark.parametrize("nx,nu,T", SIZES)
def test_box_recursion_matches_the_restatement(ctx, nx, nu, T, b, layout):
    torch, _, data = ctx
    p, truth, f64 = bc.case(nx, nu, T, b, B, shared_cost=layout == "permuted_BT")
    bc.preconditions(truth, f64)
    got = _run(torch, data, p, layout)
    print(f"{(nx, nu, T, b)} qp_iters {got['qp_iters'].tolist()}  clamped {truth['cmask'].mean():.2f}  margin {truth['margin']:.2e}")
    assert (got["status"] == 0).all()
    assert np.array_equal(got["clamped"], truth["clamped"])
    assert ((got["qp_iters"] >= 1) & (got["qp_iters"] <= bc.QP_MAX_ITER)).all()
    assert np.array_equal(_structure(got, p, p["lo"], p["hi"]), truth["cmask"])
    _compare(f"{layout}/{nx}x{nu}x{T}/b{b}", got, truth, f64)


# ---- 3. unbounded is unconstrained --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["one_side_none", "inf"])
@pytest.mark.parametrize("layout", ["dense_TB", "permuted_BT"])
@pytest.mark.parametrize("nx,nu,T", SIZES)
def test_unbounded_is_the_unconstrained_kernel_bitwise(ctx, nx, nu, T, layout, how):
    """Bounds that cannot bind (lo = -inf with hi None, or +-inf arrays) through the box kernel against the unconstrained kernel
    (both bounds None): every output equal bit for bit, nothing clamped, one QP iteration per step."""
    torch, _, data = ctx
    p = bc.case(nx, nu, T, 0.5, B, shared_cost=layout == "permuted_BT")[0]
    lo, hi = (np.full(nu, -np.inf), None) if how == "one_side_none" else (np.full(nu, -np.inf), np.full(nu, np.inf))
    got, ref = _run(torch, data, p, layout, lo=lo, hi=hi), _run(torch, data, p, layout, lo=None, hi=None)
    assert set(ref) == set(lc.OUTPUTS) | {"status"} and (ref["status"] == 0).all() and np.isfinite(ref["K"]).all()
    for key in lc.OUTPUTS + ("status",):
        assert np.array_equal(got[key], ref[key]), key
    assert (got["clamped"] == 0).all() and (got["qp_iters"] == 1).all()


def test_bounds_none_is_todays_call(ctx):
    """Without bounds the keywords change nothing: an LqrBackwardResult, bitwise that of the call without them (u is then ignored)."""
    import mujoco_template_amd as mt

    torch, _, data = ctx
    nx, nu, T = 12, 4, 30
    p = bc.box_inputs(nx, nu, T, B, 0.5)
    perm = lambda x: x.permute(1, 0, *range(2, x.ndim))
    A, Bm, lx, lu, u = (perm(_dev(torch, p[k])) for k in ("A", "B", "lx", "lu", "u"))
    kw = dict(lx=lx, lu=lu, lxx=_dev(torch, p["Q"][0]), luu=_dev(torch, p["R"][0]), VxxT=_dev(torch, p["VxxT"][0]), mu=p["mu"])
    old, new = mt.lqr_backward(data, A, Bm, **kw), mt.lqr_backward(data, A, Bm, u=u, lo=None, hi=None, **kw)
    assert type(new) is mt.LqrBackwardResult and type(old) is mt.LqrBackwardResult
    for a, b in zip(old, new):
        assert torch.equal(a, b) and a.shape == b.shape and a.stride() == b.stride()


# ---- 4. on real linearisations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T,nb,dtype", [("cartpole", 100, 1, "float64"), ("humanoid", 20, 4, "float32")])
def test_on_real_linearisations(name, T, nb, dtype):
    """linearize_rollout's (A, B) and the nominal controls passed in place; lo / hi are the model's ctrlrange scaled by a factor taken
    from the UNCONSTRAINED long-double restatement (the median |k| over the range's half width, then halved or doubled if needed) so
    that the box restatement clamps some controls but not all - asserted, with the usual preconditions, before the kernel is read."""
    import torch

    import mujoco_template_amd as mt
    from mujoco_template_amd import mj

    model = mj.MjModel.from_xml_path(MODELS[name])
    data = mj.MjData(model, batch=nb, dtype=dtype)
    nu, nx = model.nu, 2 * model.nv
    gen = torch.Generator(device="cpu").manual_seed(3)
    u = (0.05 * torch.randn((nb, T, nu), generator=gen, dtype=torch.float64)).to("cuda", torch.float32 if dtype == "float32" else torch.float64)
    _, _, A, Bm = mt.linearize_rollout(model, data, u)
    u64 = u.to(torch.float64)                                    # the kernel reads float64 controls; exact for float32 values
    rng = np.random.default_rng(4)
    p = {"A": A.permute(1, 0, 2, 3).cpu().numpy(), "B": Bm.permute(1, 0, 2, 3).cpu().numpy(), "lx": rng.normal(size=(T, nb, nx)),
         "lu": 0.1 * rng.normal(size=(T, nb, nu)), "Q": np.broadcast_to(np.eye(nx), (nb, nx, nx)).copy(),
         "R": np.broadcast_to(0.01 * np.eye(nu), (nb, nu, nu)).copy(), "VxT": np.zeros((nb, nx)), "u": u64.permute(1, 0, 2).cpu().numpy()}
    p["VxxT"] = 20.0 * p["Q"]
    if name == "cartpole":
        p["mu"] = 1e-6
        free = lc.restate_batch(p, np.longdouble)
    else:                                                        # as tests/test_gpu_lqr.py: the smallest power of ten that makes every Quu positive definite
        for e10 in range(-12, 4):
            p["mu"] = 10.0 ** e10
            free = lc.restate_batch(p, np.longdouble)
            if (free["status"] == 0).all():
                break
    assert (free["status"] == 0).all()
    rng_ = np.asarray(model.actuator_ctrlrange, dtype=np.float64).reshape(nu, 2)
    assert (rng_[:, 0] < 0).all() and (rng_[:, 1] > 0).all()
    base = float(np.median(np.abs(free["k"]).astype(np.float64))) / float(np.abs(rng_).max())
    chosen = None
    for factor in (1.0, 0.5, 2.0):
        p["lo"], p["hi"] = base * factor * rng_[:, 0], base * factor * rng_[:, 1]
        if (p["u"] < p["lo"]).any() or (p["u"] > p["hi"]).any():
            continue                                             # the nominal controls must lie inside the box
        truth, f64 = bc.restate_box_batch(p, np.longdouble), bc.restate_box_batch(p, np.float64)
        frac = truth["cmask"].mean()
        print(f"{name}: mu {p['mu']:g}  scale {base * factor:.3e}  clamped {frac:.2f}  margin {truth['margin']:.2e} / {f64['margin']:.2e}  qp_iters {truth['qp_iters'].tolist()}")
        if 0.05 < frac < 0.95 and np.array_equal(truth["cmask"], f64["cmask"]) and min(truth["margin"], f64["margin"]) >= bc.MARGIN_MIN \
                and (truth["status"] == 0).all() and (f64["status"] == 0).all():
            chosen = factor
            break
    assert chosen is not None, "no scaling of ctrlrange met the preconditions"
    bc.preconditions(truth, f64)
    res = mt.lqr_backward(data, A, Bm, lx=_dev(torch, p["lx"]).permute(1, 0, 2), lu=_dev(torch, p["lu"]).permute(1, 0, 2), lxx=_dev(torch, p["Q"][0]),
                          luu=_dev(torch, p["R"][0]), VxxT=_dev(torch, p["VxxT"][0]), mu=p["mu"], u=u64, lo=_dev(torch, p["lo"]), hi=_dev(torch, p["hi"]))
    got = _np(res)
    assert (got["status"] == 0).all()
    assert np.array_equal(got["clamped"], truth["clamped"])
    assert np.array_equal(_structure(got, p, p["lo"], p["hi"]), truth["cmask"])
    _compare(f"linearised/{name}", got, truth, f64)


# ---- 5. an indefinite Quu -------------------------------------------------------------------------------------------------------------------
def test_indefinite_quu_is_reported_as_before(ctx):
    torch, _, data = ctx
    nx, nu, T, nb, badenv = 7, 3, 12, 5, 2
    p = bc.box_inputs(nx, nu, T, nb, 0.5)
    luu = p["R"].copy(); luu[badenv] = -np.eye(nu)
    mu = np.full(nb, p["mu"]); mu[badenv] = 0.0
    got = _run(torch, data, p, "permuted_BT", luu=luu, mu=mu)
    assert got["status"].tolist() == [0, 0, T, 0, 0]
    for key in lc.OUTPUTS + ("clamped",):
        assert np.array_equal(got[key][badenv], np.zeros_like(got[key][badenv])), key
        assert np.isfinite(got[key]).all(), key
    keep = [e for e in range(nb) if e != badenv]
    alone = _run(torch, data, p, "permuted_BT", luu=luu, mu=mu, keep=keep)
    for key in lc.OUTPUTS + ("status", "clamped", "qp_iters"):
        assert np.array_equal(got[key][keep], alone[key]), key
    assert (alone["clamped"] != 0).any()


# ---- 6. stream order ------------------------------------------------------------------------------------------------------------------------
def test_chain_with_the_box_pass_on_a_side_stream_needs_no_synchronise(ctx):
    """The chain of tests/test_gpu_lqr.py with the control-limited pass in it: back to back on a non-default stream equals, bitwise, the
    same chain with a synchronise after every call - ``clamped`` included, and some control is clamped."""
    import mujoco_template_amd as mt
    from mujoco_template_amd import mj

    torch, model, nominal = ctx
    T, na, umax = 50, 8, 4.0
    nu = model.nu
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
        sol = mt.lqr_backward(nominal, A, Bm, lx=(xs @ Q)[None], lu=u @ R, lxx=Q, luu=R, VxT=(state[0, -1, 1:] @ (20 * Q)), VxxT=20 * Q, mu=1e-6,
                              u=u, lo=-umax, hi=umax); wait()
        cand = mt.lqr_candidates(nominal, A, Bm, sol.k, sol.K, u, alphas, lo=-umax, hi=umax); wait()
        st, _ = mt.rollout(model, search, cand[0], initial_state=x0); wait()
        return st.clone(), sol.status.clone(), cand.clone(), sol.clamped.clone(), sol.qp_iters.clone(), sol.k.clone()

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fast = chain(False)
    side.synchronize()
    with torch.cuda.stream(side):
        slow = chain(True)
    torch.cuda.synchronize()
    assert int(fast[1][0]) == 0 and torch.isfinite(fast[0]).all()
    assert int((fast[3] != 0).sum()) > 0 and float(fast[5].abs().max()) <= umax + 0.1
    for a, b in zip(fast, slow):
        assert torch.equal(a, b)


# ---- 7. argument checks -----------------------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_untouched(ctx):
    import mujoco_template_amd as mt
    from mujoco_template_amd.exceptions import ConfigError, TemplateError

    torch, _, data = ctx
    sim = data.sim
    T, nb, nx, nu = 3, 2, 4, 1
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    eye = lambda n: torch.eye(n, dtype=torch.float64, device="cuda")
    A, Bm, lx, lu, u, Q, R = z(T, nb, nx, nx), z(T, nb, nx, nu), z(T, nb, nx), z(T, nb, nu), z(T, nb, nu), eye(nx), eye(nu)
    lo, hi, mu = torch.full((nu,), -1.0, dtype=torch.float64, device="cuda"), torch.full((nu,), 1.0, dtype=torch.float64, device="cuda"), z(1)
    f = lambda shape, dt=torch.float64: torch.full(shape, 7, dtype=dt, device="cuda")
    outs = {"k": f((T, nb, nu)), "K": f((T, nb, nu, nx)), "dV": f((nb, 2)), "V0x": f((nb, nx)), "V0xx": f((nb, nx, nx)),
            "status": f((nb,), torch.int32), "clamped": f((T, nb), torch.int32), "qp_iters": f((nb,), torch.int32)}
    host = np.zeros(T * nb * nu)

    def call(sizes=None, ptrs=None, **override):
        arrays = {"A": (A.data_ptr(), nb * nx * nx, nx * nx), "B": (Bm.data_ptr(), nb * nx * nu, nx * nu), "lx": (lx.data_ptr(), nb * nx, nx),
                  "lu": (lu.data_ptr(), nb * nu, nu), "lxx": (Q.data_ptr(), 0, 0), "luu": (R.data_ptr(), 0, 0), "lux": (0, 0, 0),
                  "VxT": (lx.data_ptr(), 0, nx), "VxxT": (Q.data_ptr(), 0, 0), "mu": (mu.data_ptr(), 0, 0), "u": (u.data_ptr(), nb * nu, nu)}
        arrays.update(override)
        s = {"T": T, "batch": nb, "nx": nx, "nu": nu}
        s.update(sizes or {})
        pt = {k: v.data_ptr() for k, v in outs.items()}
        pt.update(lo=lo.data_ptr(), hi=hi.data_ptr())
        pt.update(ptrs or {})
        sim.lqr_backward_box(s, arrays, pt)

    call()                                                       # the well-formed call goes through
    torch.cuda.synchronize()
    assert outs["status"].tolist() == [0, 0] and outs["qp_iters"].tolist() == [1, 1] and not bool(outs["clamped"].any())
    for v in outs.values():
        v.fill_(7)
    bad = [("u is NULL", dict(u=(0, 0, 0))), ("u is not device-accessible", dict(u=(host.ctypes.data, nb * nu, nu))),
           ("lo is not device-accessible", dict(ptrs={"lo": host.ctypes.data})), ("strides must be", dict(u=(u.data_ptr(), -1, nu))),
           ("strides must be", dict(A=(A.data_ptr(), nb * nx * nx, -1))), ("nu must lie in", dict(sizes={"nu": 33})),
           ("clamped is NULL", dict(ptrs={"clamped": 0})), ("qp_iters is NULL", dict(ptrs={"qp_iters": 0}))]
    for msg, kw in bad:
        with pytest.raises((ConfigError, TemplateError), match=msg):
            call(**kw)
    with pytest.raises(ConfigError, match="u is required"):     # the tensor interface: a bound without the nominal controls
        mt.lqr_backward(data, A, Bm, lxx=Q, luu=R, VxxT=Q, lo=-1.0, time_major=True)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == 7).all()), k
