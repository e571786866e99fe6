"""Trajectory optimisation on the GPU: the backward pass of a batched time-varying LQR / iLQR and the candidate controls of its line
search, as one kernel launch each (``mjb_lqr_backward`` / ``mjb_lqr_candidates``, float64).

With ``rollout`` and ``linearize_rollout`` these are the phases of an iLQR iteration, none of which leaves the GPU::

    state, _, A, B = linearize_rollout(model, data, u, initial_state=x0)       # A [B, T, nx, nx], B [B, T, nx, nu]
    sol = lqr_backward(data, A, B, lx=lx, lu=lu, lxx=Q, luu=R, VxT=VxT, VxxT=Qf, mu=1e-6)
    cand = lqr_candidates(data, A, B, sol.k, sol.K, u, alphas, lo=-u_max, hi=u_max)        # [B, nalpha, T, nu]

The reference designs its controllers from one ``(A, B)`` with ``scipy.linalg.solve_discrete_are``; with ``lx = lu = 0`` the backward
pass is the finite-horizon, time-varying form of that recursion and ``K[:, t]`` the LQR gain of step ``t``.

Tensors are float64 on the data's GPU, addressed ``[B, T, ...]`` (``time_major=True``: ``[T, B, ...]``) through their own strides:
the permuted views ``linearize_rollout`` returns, dense tensors of either order and ``expand``-ed ones are read in place.  A tensor of
the trailing shape alone (``Q [nx, nx]``) is the same for every step and trajectory.  Only the two leading axes may be strided: the
trailing block of every (step, trajectory) must be dense and row-major, and a tensor whose block is not (a transposed ``Q``) is copied
once with ``.contiguous()`` before the launch - the one case in which an input is not read in place.  Everything is enqueued on torch's current
stream; nothing waits for the GPU and nothing is copied to the host.
"""
from __future__ import annotations

from typing import NamedTuple

from .exceptions import ConfigError


class LqrBackwardResult(NamedTuple):
    k: object        # [B, T, nu] feed-forward terms
    K: object        # [B, T, nu, nx] gains
    dV: object       # [B, 2]: sum_t k' Qu and sum_t k' Quu k / 2 (the expected cost change of step size a is a dV[0] + a^2 dV[1])
    V0x: object      # [B, nx]
    V0xx: object     # [B, nx, nx]
    status: object   # [B] int32: 0, or 1 + t for the first (highest) step whose Quu was not positive definite (results zeroed)


def _sim(data):
    return getattr(data, "sim", data)


def _strided(fn, name, x, trail, B, T, dev, time_major, optional=False):
    """(address, step stride, env stride, tensor kept alive) of one input: full ``[B, T, *trail]`` / ``[T, B, *trail]`` or ``trail`` alone"""
    import torch

    if x is None:
        if optional:
            return 0, 0, 0, None
        raise ConfigError(f"{fn}: {name} is required")
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device != dev:
        raise ConfigError(f"{fn}: {name} must be a float64 torch tensor on {dev}")
    trail = tuple(trail)
    lead = (T, B) if time_major else (B, T)
    if tuple(x.shape) == trail:
        full = False
    elif tuple(x.shape) == lead + trail:
        full = True
    else:
        raise ConfigError(f"{fn}: {name} must have shape {list(lead + trail)} or {list(trail)}, got {list(x.shape)}")
    if x.numel() and not (x[0, 0] if full else x).is_contiguous():     # the trailing block must be dense, row-major
        x = x.contiguous()
    if not full:
        return x.data_ptr(), 0, 0, x
    s0, s1 = x.stride(0), x.stride(1)
    ss, es = (s0, s1) if time_major else (s1, s0)
    return x.data_ptr(), ss, es, x


def lqr_backward(data, A, B, *, lx=None, lu=None, lxx, luu, lux=None, VxT=None, VxxT, mu=1e-6, time_major: bool = False) -> LqrBackwardResult:
    """The Riccati / iLQR backward recursion for every trajectory, one kernel launch.  For ``t = T-1 .. 0`` from ``Vx = VxT, Vxx = VxxT``::

        Qx = lx + A' Vx    Qu = lu + B' Vx    Qxx = lxx + A' Vxx A    Quu = luu + B' Vxx B + mu I    Qux = lux + B' Vxx A
        k = -Quu^-1 Qu     K = -Quu^-1 Qux    (Cholesky)              dV += (k' Qu, k' Quu k / 2)
        Vx = Qx + K' Quu k + K' Qu + Qux' k   Vxx = sym(Qxx + K' Quu K + K' Qux + Qux' K)

    ``A [B, T, nx, nx]``, ``B [B, T, nx, nu]`` (``nx <= 64``, ``nu <= 32``; an augmented state is fine: the sizes come from the tensors),
    ``lx [.., nx]``, ``lu [.., nu]`` (``None`` = 0), ``lxx [.., nx, nx]``, ``luu [.., nu, nu]``, ``lux [.., nu, nx]`` (``None`` = 0);
    ``VxT [B, nx]`` or ``[nx]`` (``None`` = 0), ``VxxT [B, nx, nx]`` or ``[nx, nx]``; ``mu`` a number or a ``[B]`` tensor (a
    per-trajectory Levenberg-Marquardt schedule stays on the GPU).  ``data`` (an ``MjData`` or ``BatchSim``) supplies the GPU; the
    number of trajectories is ``A``'s and need not be the data's batch.

    A trajectory whose ``Quu`` is not positive definite at some step stops there: ``status`` holds ``1 + t``, its ``k``, ``K`` of the
    steps ``<= t``, ``dV``, ``V0x``, ``V0xx`` are zeros and the other trajectories are unaffected (raise ``mu`` and call again)."""
    import torch

    fn = "lqr_backward"
    sim = _sim(data)
    dev = torch.device(f"cuda:{sim.device}")
    if not isinstance(A, torch.Tensor) or A.ndim != 4 or A.shape[2] != A.shape[3]:
        raise ConfigError(f"{fn}: A must be a [B, T, nx, nx] tensor")
    if not isinstance(B, torch.Tensor) or B.ndim != 4:
        raise ConfigError(f"{fn}: B must be a [B, T, nx, nu] tensor")
    (T, nb) = (A.shape[0], A.shape[1]) if time_major else (A.shape[1], A.shape[0])
    nx, nu = int(A.shape[2]), int(B.shape[3])
    T, nb = int(T), int(nb)
    zeros = None

    def zero(n):
        nonlocal zeros
        if zeros is None:
            zeros = torch.zeros(max(nx, nu), dtype=torch.float64, device=dev)
        return zeros[:n]

    arrays, keep = {}, []
    for name, x, trail in (("A", A, (nx, nx)), ("B", B, (nx, nu)), ("lx", zero(nx) if lx is None else lx, (nx,)),
                           ("lu", zero(nu) if lu is None else lu, (nu,)), ("lxx", lxx, (nx, nx)), ("luu", luu, (nu, nu)), ("lux", lux, (nu, nx))):
        p, ss, es, t = _strided(fn, name, x, trail, nb, T, dev, time_major, optional=name == "lux")
        arrays[name] = (p, ss, es); keep.append(t)
    for name, x, trail in (("VxT", zero(nx) if VxT is None else VxT, (nx,)), ("VxxT", VxxT, (nx, nx))):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device != dev or tuple(x.shape) not in (trail, (nb,) + trail):
            raise ConfigError(f"{fn}: {name} must be a float64 tensor {list((nb,) + trail)} or {list(trail)} on {dev}")
        if not (x if x.ndim == len(trail) else x[0]).is_contiguous():
            x = x.contiguous()
        arrays[name] = (x.data_ptr(), 0, 0 if x.ndim == len(trail) else x.stride(0)); keep.append(x)
    if isinstance(mu, torch.Tensor):
        if mu.dtype != torch.float64 or mu.device != dev or tuple(mu.shape) != (nb,):
            raise ConfigError(f"{fn}: mu must be a number or a float64 tensor [{nb}] on {dev}")
        arrays["mu"] = (mu.data_ptr(), 0, mu.stride(0))
    else:
        mu = torch.full((1,), float(mu), dtype=torch.float64, device=dev)
        arrays["mu"] = (mu.data_ptr(), 0, 0)
    keep.append(mu)
    opt = dict(dtype=torch.float64, device=dev)
    k = torch.empty((T, nb, nu), **opt)
    K = torch.empty((T, nb, nu, nx), **opt)
    dV, V0x, V0xx = torch.empty((nb, 2), **opt), torch.empty((nb, nx), **opt), torch.empty((nb, nx, nx), **opt)
    status = torch.empty((nb,), dtype=torch.int32, device=dev)
    sim.lqr_backward({"T": T, "batch": nb, "nx": nx, "nu": nu}, arrays,
                     {"k": k.data_ptr(), "K": K.data_ptr(), "dV": dV.data_ptr(), "V0x": V0x.data_ptr(), "V0xx": V0xx.data_ptr(),
                      "status": status.data_ptr()}, keep=keep)
    if not time_major:
        k, K = k.permute(1, 0, 2), K.permute(1, 0, 2, 3)
    return LqrBackwardResult(k, K, dV, V0x, V0xx, status)


def lqr_candidates(data, A, B, k, K, u, alphas, *, dx0=None, lo=None, hi=None, dtype=None, time_major: bool = False):
    """The candidate controls of a line search, every step size at once: for trajectory ``e`` and ``alphas[j]``, from ``dx = dx0[e]``
    (``None`` = 0), ``c_t = clamp(u_t + alphas[j] k_t + K_t dx, lo, hi)`` and ``dx = A_t dx + B_t (c_t - u_t)`` - the closed loop on
    the linearised dynamics.  Returns ``cand [B, nalpha, T, nu]`` in ``dtype`` (``torch.float64``, the default, or ``torch.float32`` =
    the float64 value rounded once: what ``rollout`` of a float32 data object takes).  ``k [B, T, nu]``, ``K [B, T, nu, nx]`` as
    ``lqr_backward`` returns them, ``u [B, T, nu]``, ``alphas [nalpha]`` (at most 64) float64 on the GPU; ``lo`` / ``hi``: a number, a
    ``[nu]`` tensor or ``None`` (unbounded)."""
    import torch

    fn = "lqr_candidates"
    sim = _sim(data)
    dev = torch.device(f"cuda:{sim.device}")
    if not isinstance(A, torch.Tensor) or A.ndim != 4 or A.shape[2] != A.shape[3] or not isinstance(B, torch.Tensor) or B.ndim != 4:
        raise ConfigError(f"{fn}: A must be a [B, T, nx, nx] and B a [B, T, nx, nu] tensor")
    (T, nb) = (A.shape[0], A.shape[1]) if time_major else (A.shape[1], A.shape[0])
    nx, nu, T, nb = int(A.shape[2]), int(B.shape[3]), int(T), int(nb)
    dtype = torch.float64 if dtype is None else dtype
    if dtype not in (torch.float64, torch.float32):
        raise ConfigError(f"{fn}: dtype must be torch.float64 or torch.float32")
    if not isinstance(alphas, torch.Tensor) or alphas.dtype != torch.float64 or alphas.device != dev or alphas.ndim != 1:
        raise ConfigError(f"{fn}: alphas must be a float64 tensor [nalpha] on {dev}")
    alphas = alphas.contiguous()
    na = int(alphas.shape[0])
    arrays, keep = {}, [alphas]
    for name, x, trail in (("A", A, (nx, nx)), ("B", B, (nx, nu)), ("k", k, (nu,)), ("K", K, (nu, nx)), ("u", u, (nu,))):
        p, ss, es, t = _strided(fn, name, x, trail, nb, T, dev, time_major)
        arrays[name] = (p, ss, es); keep.append(t)
    if dx0 is None:
        arrays["dx0"] = (0, 0, 0)
    else:
        if not isinstance(dx0, torch.Tensor) or dx0.dtype != torch.float64 or dx0.device != dev or tuple(dx0.shape) not in ((nx,), (nb, nx)):
            raise ConfigError(f"{fn}: dx0 must be a float64 tensor [{nb}, {nx}] or [{nx}] on {dev}")
        dx0 = dx0.contiguous()
        arrays["dx0"] = (dx0.data_ptr(), 0, nx if dx0.ndim == 2 else 0); keep.append(dx0)
    ptrs = {"alphas": alphas.data_ptr()}
    for name, x in (("lo", lo), ("hi", hi)):
        if x is None:
            ptrs[name] = 0
            continue
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.float64 or x.device != dev or tuple(x.shape) != (nu,):
                raise ConfigError(f"{fn}: {name} must be a number or a float64 tensor [{nu}] on {dev}")
            x = x.contiguous()
        else:
            x = torch.full((nu,), float(x), dtype=torch.float64, device=dev)
        ptrs[name] = x.data_ptr(); keep.append(x)
    cand = torch.empty((nb, na, T, nu), dtype=dtype, device=dev)
    ptrs["cand"] = cand.data_ptr()
    sim.lqr_candidates({"T": T, "batch": nb, "nx": nx, "nu": nu, "nalpha": na, "out_f32": int(dtype == torch.float32)}, arrays, ptrs,
                       keep=keep)
    return cand


__all__ = ["LqrBackwardResult", "lqr_backward", "lqr_candidates"]
