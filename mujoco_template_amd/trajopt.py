"""Trajectory optimisation on the GPU: the backward pass of a batched time-varying LQR / iLQR and the candidate controls of its line
search, as one kernel launch each (``mjb_lqr_backward`` / ``mjb_lqr_candidates``, float64), the quadratic trajectory cost with its
first-order expansion (``mjb_traj_cost``) and the choice or softmin update over candidates (``mjb_traj_select``).

With ``rollout`` and ``linearize_rollout`` these are the phases of an iLQR iteration, none of which leaves the GPU::

    state, _, A, B = linearize_rollout(model, data, u, initial_state=x0)       # A [B, T, nx, nx], B [B, T, nx, nu]
    c = trajectory_cost(data, state, u, initial_state=x0, Q=Q, R=R, Qf=Qf, x_ref=x_ref)       # cost [B], lx, lu, VxT
    sol = lqr_backward(data, A, B, lx=c.lx, lu=c.lu, lxx=Q, luu=R, VxT=c.VxT, VxxT=Qf, mu=1e-6)
    # (with actuator limits: lqr_backward(..., u=u, lo=-u_max, hi=u_max) - the control-limited pass, an LqrBoxResult)
    cand = lqr_candidates(data, A, B, sol.k, sol.K, u, alphas, lo=-u_max, hi=u_max)        # [B, nalpha, T, nu]
    st, _ = rollout(model, search, cand[0], initial_state=x0)
    cc = trajectory_cost(search, st, cand[0], initial_state=x0, Q=Q, R=R, Qf=Qf, x_ref=x_ref, gradients=False)
    select_candidates(data, cc.cost[None], cand, out=u)                        # u <- the best candidate, no host read

The reference designs its controllers from one ``(A, B)`` with ``scipy.linalg.solve_discrete_are``; with ``lx = lu = 0`` the backward
pass is the finite-horizon, time-varying form of that recursion and ``K[:, t]`` the LQR gain of step ``t``.  The equation itself -
the infinite-horizon design - is ``solve_dare`` (``mjb_lqr_dare``, a doubling algorithm: one launch for every system of a batch), so
that a per-environment LQR design under domain randomisation never leaves the GPU either::

    data.set_env_params(body_mass=mass)                                          # every environment its own model
    _, _, A, B = linearize_rollout(model, data, u0[:, None], initial_state=x0)   # T = 1: A [B, 1, nx, nx], B [B, 1, nx, nu]
    sol = solve_dare(data, A[:, 0], B[:, 0], Q, R)                               # the views are read in place; sol.K [B, nu, nx]
    # a torch controller on DeviceData: ctrl = u0 - (sol.K @ dx[..., None])[..., 0]   (K has the reference's sign, not lqr_backward's)

The reference's next line after every design is ``np.max(np.abs(np.linalg.eigvals(A - B @ K)))``: it refuses a gain whose closed-loop
spectral radius is not below 1.  ``closed_loop_poles`` (``mjb_lqr_eig``) is that check for the whole batch in one launch - LAPACK's
method for eigenvalues alone (power-of-two balancing, Householder reduction to Hessenberg form, Francis double-shift QR with dlahqr's
deflation tests), one wavefront per system - so the chain is ``... -> solve_dare -> closed_loop_poles -> (rho < 1) mask``::

    poles = closed_loop_poles(data, A[:, 0], B[:, 0], sol.K)                     # wr, wi [B, nx] by descending modulus; rho [B]
    stable = poles.rho < 1                                                       # False for a failed problem too: its rho is +inf
    # one nominal gain against every randomised model (K [nu, nx] is read once, no copy): closed_loop_poles(data, A[:, 0], B[:, 0], K_nominal)

What a gain costs where it is stable is ``closed_loop_cost`` (``mjb_lqr_dlyap``): the solution ``P`` of the discrete Lyapunov equation
``P = M' P M + Q + K' R K`` of the closed loop ``M = A - B K`` by the squared Smith (doubling) iteration, and ``J = x0' P x0``, one
workgroup per system.  For the gain of ``solve_dare`` ``P`` is its ``X``; for the nominal gain on a randomised model it is what
``scipy.linalg.solve_discrete_lyapunov`` gives on the host, so the chain goes on
``... -> closed_loop_poles -> closed_loop_cost -> J_nominal / J_optimal per environment``::

    nominal = closed_loop_cost(data, A[:, 0], B[:, 0], K_nominal, Q=Q, R=R, x0=dx0)        # P [B, nx, nx], J [B]; +inf where it failed
    optimal = closed_loop_cost(data, A[:, 0], B[:, 0], sol.K, Q=Q, R=R, x0=dx0)            # P is sol.X to rounding
    price = nominal.J / optimal.J                                                          # >= 1: what the nominal gain costs on model e

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


class LqrBoxResult(NamedTuple):
    k: object        # [B, T, nu] feed-forward terms, inside [lo - u, hi - u]; bitwise the bound where clamped
    K: object        # [B, T, nu, nx] gains; the rows of clamped controls are zero
    dV: object       # [B, 2]
    V0x: object      # [B, nx]
    V0xx: object     # [B, nx, nx]
    status: object   # [B] int32: 0; 1 + t as LqrBackwardResult; -(1 + t) for the highest step whose QP did not converge (results usable)
    clamped: object  # [B, T] int32: bit a set when control a is clamped at that step
    qp_iters: object  # [B] int32: the largest QP iteration count of any step


def _sim(data):
    return getattr(data, "sim", data)


def _strided(fn, name, x, trail, B, T, dev, time_major, optional=False, dtypes=None):
    """(address, step stride, env stride, tensor kept alive) of one input: full ``[B, T, *trail]`` / ``[T, B, *trail]`` or ``trail`` alone.
    ``dtypes``: the element types accepted (float64 alone by default); the tensor returned tells which one it is."""
    import torch

    if x is None:
        if optional:
            return 0, 0, 0, None
        raise ConfigError(f"{fn}: {name} is required")
    dtypes = (torch.float64,) if dtypes is None else tuple(dtypes)
    if not isinstance(x, torch.Tensor) or x.dtype not in dtypes or x.device != dev:
        raise ConfigError(f"{fn}: {name} must be a {' or '.join(str(d).replace('torch.', '') for d in dtypes)} torch tensor on {dev}")
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


def _bound(fn, name, x, nu, dev, keep):
    """Device address of one side of a control box: a number, a float64 ``[nu]`` tensor, or ``None`` (0: unbounded on that side)."""
    import torch

    if x is None:
        return 0
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float64 or x.device != dev or tuple(x.shape) != (nu,):
            raise ConfigError(f"{fn}: {name} must be a number or a float64 tensor [{nu}] on {dev}")
        x = x.contiguous()
    else:
        x = torch.full((nu,), float(x), dtype=torch.float64, device=dev)
    keep.append(x)
    return x.data_ptr()


def lqr_backward(data, A, B, *, lx=None, lu=None, lxx, luu, lux=None, VxT=None, VxxT, mu=1e-6, time_major: bool = False,
                 u=None, lo=None, hi=None):
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
    steps ``<= t``, ``dV``, ``V0x``, ``V0xx`` are zeros and the other trajectories are unaffected (raise ``mu`` and call again).

    **Control limits.**  With ``lo`` and / or ``hi`` (a number, a ``[nu]`` tensor or ``None`` = unbounded on that side, as
    ``lqr_candidates`` takes them) and the nominal controls ``u [B, T, nu]`` (required then, read in place), the pass is control-limited
    DDP (Tassa, Mansard, Todorov 2014; ``mjb_lqr_backward_box``): per step the box QP ``min dk' Quu dk / 2 + Qu' dk`` subject to
    ``lo - u_t <= dk <= hi - u_t`` by projected Newton, ``k`` its solution (bitwise the bound where clamped), the rows of ``K`` of the
    clamped controls zero, the value update unchanged.  Returns an ``LqrBoxResult``: the fields above plus ``clamped [B, T]`` (bit
    masks) and ``qp_iters [B]``; ``status`` may also be ``-(1 + t)``: the QP of step ``t`` hit its iteration cap (64) or its line search
    failed, the results are still inside the box.  With both bounds ``None`` the call is the unconstrained one above."""
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
    box = lo is not None or hi is not None
    bounds = {}
    if box:
        p, ss, es, t = _strided(fn, "u", u, (nu,), nb, T, dev, time_major)
        if tuple(t.shape) == (nu,):
            raise ConfigError(f"{fn}: u must have shape {[T, nb, nu] if time_major else [nb, T, nu]}")
        arrays["u"] = (p, ss, es); keep.append(t)
        bounds = {"lo": _bound(fn, "lo", lo, nu, dev, keep), "hi": _bound(fn, "hi", hi, nu, dev, keep)}
    opt = dict(dtype=torch.float64, device=dev)
    k = torch.empty((T, nb, nu), **opt)
    K = torch.empty((T, nb, nu, nx), **opt)
    dV, V0x, V0xx = torch.empty((nb, 2), **opt), torch.empty((nb, nx), **opt), torch.empty((nb, nx, nx), **opt)
    status = torch.empty((nb,), dtype=torch.int32, device=dev)
    sizes = {"T": T, "batch": nb, "nx": nx, "nu": nu}
    ptrs = {"k": k.data_ptr(), "K": K.data_ptr(), "dV": dV.data_ptr(), "V0x": V0x.data_ptr(), "V0xx": V0xx.data_ptr(), "status": status.data_ptr()}
    if not box:
        sim.lqr_backward(sizes, arrays, ptrs, keep=keep)
        if not time_major:
            k, K = k.permute(1, 0, 2), K.permute(1, 0, 2, 3)
        return LqrBackwardResult(k, K, dV, V0x, V0xx, status)
    clamped = torch.empty((T, nb), dtype=torch.int32, device=dev)
    qp_iters = torch.empty((nb,), dtype=torch.int32, device=dev)
    ptrs.update(bounds, clamped=clamped.data_ptr(), qp_iters=qp_iters.data_ptr())
    sim.lqr_backward_box(sizes, arrays, ptrs, keep=keep)
    if not time_major:
        k, K, clamped = k.permute(1, 0, 2), K.permute(1, 0, 2, 3), clamped.permute(1, 0)
    return LqrBoxResult(k, K, dV, V0x, V0xx, status, clamped, qp_iters)


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
    ptrs = {"alphas": alphas.data_ptr(), "lo": _bound(fn, "lo", lo, nu, dev, keep), "hi": _bound(fn, "hi", hi, nu, dev, keep)}
    cand = torch.empty((nb, na, T, nu), dtype=dtype, device=dev)
    ptrs["cand"] = cand.data_ptr()
    sim.lqr_candidates({"T": T, "batch": nb, "nx": nx, "nu": nu, "nalpha": na, "out_f32": int(dtype == torch.float32)}, arrays, ptrs,
                       keep=keep)
    return cand


class DareResult(NamedTuple):
    X: object        # [nb, nx, nx] the stabilising solution of the Riccati equation, bitwise symmetric (zeros where status != 0)
    K: object        # [nb, nu, nx] the gain of u = u0 - K dx (zeros where status != 0)
    status: object   # [nb] int32: 0 converged, 1 a Cholesky pivot (R or R + B'XB), 2 an LU pivot or an iterate not finite, 3 max_iter reached
    iters: object    # [nb] int32 doubling iterations done
    change: object   # [nb] max|H_{k+1} - H_k| / max|H_{k+1}| of the last iteration (+inf when not finite)


def solve_dare(data, A, B, Q, R, *, tol: float = 1e-12, max_iter: int = 32) -> DareResult:
    """Infinite-horizon LQR design for ``nb`` systems in one kernel launch (``mjb_lqr_dare``): the stabilising solution ``X`` of

        A' X A - X - A' X B (R + B' X B)^-1 B' X A + Q = 0        and        K = (R + B' X B)^-1 B' X A

    - what the reference gets from ``scipy.linalg.solve_discrete_are`` for one system on the host.  The structure-preserving doubling
    algorithm in float64 (include/mjbatch.h states it): iteration ``k`` holds ``2^k`` steps of the Riccati recursion, so a dozen
    iterations (19 on the humanoid balance design, whose closed loop keeps marginal modes) reach what ``lqr_backward`` on a constant
    ``(A, B)`` needs thousands of steps for.  It stops when ``max|H_{k+1} - H_k| / max|H_{k+1}| <= tol`` or after ``max_iter`` (1..64).

    **Sign.**  ``K`` is the gain of the reference and of ``set_feedback`` (``u = u0 - K dx``): the NEGATIVE of ``lqr_backward``'s ``K``.

    ``A [nb, nx, nx]``, ``B [nb, nx, nu]``, ``Q [nb, nx, nx]``, ``R [nb, nu, nu]`` (``nx <= 64``, ``nu <= 32``), float64 on the data's
    GPU; each may also be its trailing block alone, shared by all problems.  ``nb`` is the leading size of those that have one (they
    must agree; 1 if none has) and need not be the data's batch.  The leading axis may be strided: the ``A[:, 0]``, ``B[:, 0]`` views
    of ``linearize_rollout(..., T=1)`` are read in place; a trailing block that is not dense and row-major is copied once with
    ``.contiguous()``.  ``Q`` and ``R`` are taken as symmetric and not checked: only their lower triangles are read.  No cross term.

    ``status`` (per problem): 0 converged; 1 a Cholesky pivot of ``R`` or ``R + B'XB`` was ``<= 0`` or not finite; 2 an LU pivot was
    zero or not finite or an iterate was not finite (a system that is not stabilisable ends this way); 3 ``max_iter`` reached.  Where it
    is not 0, ``X`` and ``K`` are zeros, ``iters`` and ``change`` hold what was reached, and no other problem is affected.  A problem's
    results are bitwise the same at any position of any batch.  Enqueued on torch's current stream; nothing waits for the GPU and
    nothing is copied to the host."""
    import torch

    fn = "solve_dare"
    sim = _sim(data)
    dev = torch.device(f"cuda:{sim.device}")
    for name, x in (("A", A), ("B", B), ("Q", Q), ("R", R)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device != dev or x.ndim not in (2, 3):
            raise ConfigError(f"{fn}: {name} must be a float64 torch tensor [nb, n, m] or [n, m] on {dev}")
    nx, nu = int(A.shape[-1]), int(B.shape[-1])
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or not (tol >= 0):
        raise ConfigError(f"{fn}: max_iter must be an integer and tol >= 0")
    lead = {name: int(x.shape[0]) for name, x in (("A", A), ("B", B), ("Q", Q), ("R", R)) if x.ndim == 3}
    if len(set(lead.values())) > 1:
        raise ConfigError(f"{fn}: the leading sizes differ: {lead}")
    nb = next(iter(lead.values())) if lead else 1
    if nb < 1:
        raise ConfigError(f"{fn}: at least one problem is required")
    arrays, keep = {}, []
    for name, x, trail in (("A", A, (nx, nx)), ("B", B, (nx, nu)), ("Q", Q, (nx, nx)), ("R", R, (nu, nu))):
        if tuple(x.shape[-2:]) != trail:
            raise ConfigError(f"{fn}: {name} must have shape {[nb, *trail]} or {list(trail)}, got {list(x.shape)}")
        if x.numel() and not (x[0] if x.ndim == 3 else x).is_contiguous():     # the trailing block must be dense, row-major
            x = x.contiguous()
        es = x.stride(0) if x.ndim == 3 else 0
        if es < 0:
            raise ConfigError(f"{fn}: {name} has a negative stride")
        arrays[name] = (x.data_ptr(), 0, es); keep.append(x)
    opt = dict(dtype=torch.float64, device=dev)
    X, K, change = torch.empty((nb, nx, nx), **opt), torch.empty((nb, nu, nx), **opt), torch.empty((nb,), **opt)
    iters, status = torch.empty((nb,), dtype=torch.int32, device=dev), torch.empty((nb,), dtype=torch.int32, device=dev)
    sim.lqr_dare({"batch": nb, "nx": nx, "nu": nu, "max_iter": int(max_iter), "tol": float(tol)}, arrays,
                 {"X": X.data_ptr(), "K": K.data_ptr(), "change": change.data_ptr(), "iters": iters.data_ptr(), "status": status.data_ptr()}, keep=keep)
    return DareResult(X, K, status, iters, change)


class KalmanResult(NamedTuple):
    P: object        # [nb, nx, nx] the steady-state a-priori error covariance, bitwise symmetric (zeros where status != 0)
    L: object        # [nb, nx, ny] the gain of the one-step predictor (zeros where status != 0)
    status: object   # [nb] int32, solve_dare's: 0 converged, 1 a Cholesky pivot (V or C P C' + V), 2 an LU pivot or an iterate not finite, 3 max_iter reached
    iters: object    # [nb] int32 doubling iterations done
    change: object   # [nb] relative change of the last iteration (+inf when not finite)


def solve_kalman(data, A, C, W, V, *, tol: float = 1e-12, max_iter: int = 32) -> KalmanResult:
    """Steady-state Kalman gain for ``nb`` systems ``x+ = A x + B u + w``, ``y = C x + D u + v`` with ``cov w = W``, ``cov v = V``, in
    one kernel launch: the stabilising solution ``P`` (the steady-state a-priori error covariance) of

        P = A P A' - A P C' (C P C' + V)^-1 C P A' + W        and        L = A P C' (C P C' + V)^-1

    ``L`` is the gain of the one-step predictor ``xhat+ = A xhat + B du + L (dy - C xhat - D du)``, whose error dynamics are
    ``A - L C``.  ``(A, B, C, D)`` are what ``linearize_rollout(..., sensor_derivatives=True)`` returns (the reference leaves ``C`` and
    ``D`` of ``mjd_transitionFD`` out, mujoco_template/linearization.py:28-34).

    The filter equation is the dual of the regulator's: this is ``solve_dare(data, A', C', W, V)`` with ``P = X`` and ``L = K'``, on the
    same kernel (``mjb_lqr_dare``) - no new solver, nothing on the host.  The transposes cost one ``.transpose(-1, -2).contiguous()``
    each; a block without a leading axis, shared by all systems, stays shared.

    - The filter (measurement-update) gain:  ``M = torch.linalg.solve(C @ P @ C.mT + V, C @ P).mT``  ``= P C' (C P C' + V)^-1``.
    - The stability check:  ``closed_loop_poles(data, A.mT, C.mT, L.mT).rho < 1``  (the poles of ``A' - C' L'``, those of ``A - L C``).

    ``A [nb, nx, nx]``, ``C [nb, ny, nx]``, ``W [nb, nx, nx]``, ``V [nb, ny, ny]`` (``nx <= 64``, ``ny <= 32``), float64 on the data's GPU,
    each optionally its trailing block alone; ``nb``, ``tol``, ``max_iter`` and ``status`` as in ``solve_dare``.  A pair ``(A, C)`` that is
    not detectable ends with ``status != 0`` and zeros in ``P`` and ``L``, as ``solve_dare`` documents for a system that is not
    stabilisable; no other system is affected."""
    import torch

    fn = "solve_kalman"
    for name, x in (("A", A), ("C", C)):
        if not isinstance(x, torch.Tensor) or x.ndim not in (2, 3):
            raise ConfigError(f"{fn}: {name} must be a float64 torch tensor [nb, n, m] or [n, m]")
    if A.shape[-1] != A.shape[-2] or C.shape[-1] != A.shape[-1]:
        raise ConfigError(f"{fn}: A must be [nb, nx, nx] and C [nb, ny, nx], got {list(A.shape)} and {list(C.shape)}")
    sol = solve_dare(data, A.transpose(-1, -2).contiguous(), C.transpose(-1, -2).contiguous(), W, V, tol=tol, max_iter=max_iter)
    return KalmanResult(sol.X, sol.K.transpose(-1, -2), sol.status, sol.iters, sol.change)


class PolesResult(NamedTuple):
    wr: object       # [nb, nx] real parts, by descending modulus, ties by descending wr, then descending wi (NaN where status != 0)
    wi: object       # [nb, nx] imaginary parts; a complex pair is two neighbours with equal wr and wi bitwise negated, the positive one first
    rho: object      # [nb] the spectral radius: the correctly rounded sqrt(wr[:, 0]^2 + wi[:, 0]^2) (+inf where status != 0)
    status: object   # [nb] int32: 0 ok, 1 an entry of A, B, K or M is not finite, 2 max_sweeps reached before every eigenvalue had deflated
    sweeps: object   # [nb] int32 Francis sweeps done
    scale: object    # [nb, nx] the balancing diagonal D (powers of two; ones with balance=False): the spectrum computed is that of D^-1 M D


def closed_loop_poles(data, A, B=None, K=None, *, feedback_sign: int = -1, balance: bool = True, max_sweeps=None) -> PolesResult:
    """Every eigenvalue of ``M = A + feedback_sign * B K`` and the spectral radius ``rho = max |lambda|`` for ``nb`` systems in one
    kernel launch (``mjb_lqr_eig``) - what the reference computes with ``np.max(np.abs(np.linalg.eigvals(A - B @ K)))`` after every
    design, to refuse a gain that does not stabilise.  ``rho < 1`` is the mask of the stabilised environments.

    **Sign.**  ``feedback_sign=-1`` (the default) is the convention of ``solve_dare`` and ``set_feedback`` (``u = u0 - K dx``); ``+1``
    is ``lqr_backward``'s.  The sign is applied to ``K`` exactly: ``+1`` with ``-K`` gives the bits of ``-1`` with ``K``.  With ``B``
    and ``K`` both ``None`` the matrix is ``A`` itself (open-loop poles); exactly one of them is a ``ConfigError``.

    **Method**: LAPACK's for eigenvalues only, in float64, one wavefront per system with the iterate in LDS (include/mjbatch.h states
    it): ``M`` on the f64 MFMA; with ``balance`` Parlett-Reinsch scaling by powers of two (exact, no permutation; ``scale`` returns the
    diagonal ``D``, the spectrum computed is that of ``D^-1 M D``); Householder reduction to Hessenberg form; Francis implicit
    double-shift QR with ``dlahqr``'s deflation tests and exceptional shifts and ``dlanv2``'s 2 x 2 blocks.  ``max_sweeps`` caps the total
    number of sweeps of a system: ``None`` = LAPACK's ``30 * max(10, nx)``, else 1 .. that number.

    ``A [nb, nx, nx]``, ``B [nb, nx, nu]``, ``K [nb, nu, nx]`` (``nx <= 64``, ``nu <= 32``), float64 on the data's GPU; each may also
    be its trailing block alone, shared by all problems - one nominal ``K [nu, nx]`` against per-environment ``A``, ``B`` is the
    robustness sweep and costs no copy.  ``nb`` is taken and checked as in ``solve_dare``.  The leading axis may be strided (``A[:, 0]``
    of ``linearize_rollout`` and ``sol.K`` are read in place); a trailing block that is not dense and row-major is copied once with
    ``.contiguous()``; a negative stride is rejected.

    **Order.**  ``wr, wi [nb, nx]`` by descending modulus, ties by descending ``wr``, then descending ``wi``; a complex pair comes as
    exact conjugates (equal ``wr``, ``wi`` bitwise negated, the positive one first).  ``rho [nb]`` is the modulus of the first.

    **Failures.**  ``status`` 1: an entry is not finite; 2: ``max_sweeps`` reached.  There ``wr``, ``wi`` are NaN and ``rho`` is
    ``+inf``, so that ``rho < 1`` is false - deliberately not the zeros of ``solve_dare``, which would read as stable.  No other problem
    is affected; a problem's results are bitwise the same at any position of any batch.  Enqueued on torch's current stream; nothing
    waits for the GPU and nothing is copied to the host."""
    import torch

    fn = "closed_loop_poles"
    sim = _sim(data)
    dev = torch.device(f"cuda:{sim.device}")
    if (B is None) != (K is None):
        raise ConfigError(f"{fn}: B and K must be given together (both None: the poles of A)")
    given = (("A", A),) if B is None else (("A", A), ("B", B), ("K", K))
    for name, x in given:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device != dev or x.ndim not in (2, 3):
            raise ConfigError(f"{fn}: {name} must be a float64 torch tensor [nb, n, m] or [n, m] on {dev}")
    nx = int(A.shape[-1])
    nu = 0 if B is None else int(B.shape[-1])
    if feedback_sign not in (-1, 1) or isinstance(feedback_sign, bool):
        raise ConfigError(f"{fn}: feedback_sign must be -1 or +1")
    if max_sweeps is not None and (isinstance(max_sweeps, bool) or int(max_sweeps) != max_sweeps or not 1 <= max_sweeps <= 30 * max(10, nx)):
        raise ConfigError(f"{fn}: max_sweeps must be None or an integer in [1, {30 * max(10, nx)}]")
    lead = {name: int(x.shape[0]) for name, x in given if x.ndim == 3}
    if len(set(lead.values())) > 1:
        raise ConfigError(f"{fn}: the leading sizes differ: {lead}")
    nb = next(iter(lead.values())) if lead else 1
    if nb < 1:
        raise ConfigError(f"{fn}: at least one problem is required")
    arrays, keep = {}, []
    for (name, x), trail in zip(given, ((nx, nx), (nx, nu), (nu, nx))):
        if tuple(x.shape[-2:]) != trail:
            raise ConfigError(f"{fn}: {name} must have shape {[nb, *trail]} or {list(trail)}, got {list(x.shape)}")
        if x.numel() and not (x[0] if x.ndim == 3 else x).is_contiguous():     # the trailing block must be dense, row-major
            x = x.contiguous()
        es = x.stride(0) if x.ndim == 3 else 0
        if es < 0:
            raise ConfigError(f"{fn}: {name} has a negative stride")
        arrays[name] = (x.data_ptr(), 0, es); keep.append(x)
    opt = dict(dtype=torch.float64, device=dev)
    wr, wi, scale, rho = torch.empty((nb, nx), **opt), torch.empty((nb, nx), **opt), torch.empty((nb, nx), **opt), torch.empty((nb,), **opt)
    sweeps, status = torch.empty((nb,), dtype=torch.int32, device=dev), torch.empty((nb,), dtype=torch.int32, device=dev)
    sim.lqr_eig({"batch": nb, "nx": nx, "nu": nu, "feedback_sign": int(feedback_sign), "balance": int(bool(balance)),
                 "max_sweeps": 0 if max_sweeps is None else int(max_sweeps)}, arrays,
                {"wr": wr.data_ptr(), "wi": wi.data_ptr(), "rho": rho.data_ptr(), "scale": scale.data_ptr(), "sweeps": sweeps.data_ptr(),
                 "status": status.data_ptr()}, keep=keep)
    return PolesResult(wr, wi, rho, status, sweeps, scale)


class LyapResult(NamedTuple):
    P: object        # [nb, nx, nx] the solution of P = M' P M + Q + K' R K, bitwise symmetric (NaN where status != 0)
    J: object        # [nb] x0' P x0 (+inf where status != 0), or None without x0
    status: object   # [nb] int32: 0 converged, 1 an entry of M or S is not finite, 2 an iterate not finite (rho > 1), 3 max_iter reached
    iters: object    # [nb] int32 doubling iterations done
    change: object   # [nb] max|P_{k+1} - P_k| / max|P_{k+1}| of the last iteration (+inf when not finite)


def closed_loop_cost(data, A, B=None, K=None, *, Q, R=None, x0=None, feedback_sign: int = -1, transpose: bool = False,
                     tol: float = 1e-12, max_iter: int = 64) -> LyapResult:
    """The infinite-horizon quadratic cost of running the gain ``K`` on ``(A, B)`` for ``nb`` systems in one kernel launch
    (``mjb_lqr_dlyap``): the solution ``P`` of the discrete Lyapunov equation

        P = M' P M + Q + K' R K,        M = A + feedback_sign * B K

    and, with ``x0``, ``J = x0' P x0`` - what ``scipy.linalg.solve_discrete_lyapunov`` gives for one system on the host.  For the
    gain of ``solve_dare`` ``P`` is its ``X`` (the ``P`` the reference's ``_solve_lqr_gains`` returns beside ``K``); for any other gain
    - a nominal one on a randomised model, a hand-tuned one - ``J / J_optimal`` says what that gain costs there.  The squared Smith
    (doubling) iteration in float64 (include/mjbatch.h states it): ``P <- sym(P + M' P M)``, ``M <- M M``, so iterate ``k`` holds
    ``2^k`` steps of the cost sum; it stops at the FIRST ``max|P_{k+1} - P_k| / max|P_{k+1}| <= tol`` or after ``max_iter`` (1..64).

    **Sign.**  As in ``closed_loop_poles``: ``-1`` (the default) for the gains of ``solve_dare`` and ``set_feedback``, ``+1`` for
    ``lqr_backward``'s; applied to ``K`` exactly.  With ``B`` and ``K`` both ``None``, ``M = A``; exactly one of them is a
    ``ConfigError``, and so is ``R`` without ``K``.  ``R=None`` leaves the cost term ``K' R K`` out.

    **Gramian form.**  ``transpose=True`` solves ``P = M P M' + S`` with the same ``S = sym(Q + K' R K)``: ``Q = B B'`` gives the
    controllability Gramian of ``M``.

    ``A [nb, nx, nx]``, ``B [nb, nx, nu]``, ``K [nb, nu, nx]``, ``Q [nb, nx, nx]``, ``R [nb, nu, nu]``, ``x0 [nb, nx]`` (``nx <= 64``,
    ``nu <= 32``), float64 on the data's GPU; each may also be its trailing block alone, shared by all problems - one nominal ``K``,
    ``Q``, ``R`` against per-environment ``A``, ``B`` is the robustness sweep and costs no copy.  ``nb`` is taken and checked as in
    ``solve_dare``.  The leading axis may be strided (``A[:, 0]`` of ``linearize_rollout``, ``expand``-ed tensors and ``sol.K`` are read
    in place); a trailing block that is not dense and row-major is copied once with ``.contiguous()``.  ``Q`` and ``R`` are taken as
    symmetric and not checked: only their lower triangles are read.

    **Failures.**  ``status`` 1: an entry of ``M`` or ``S`` is not finite; 2: an iterate is not finite (a closed loop with
    ``rho > 1`` ends this way); 3: ``max_iter`` reached (``rho == 1`` with a marginal mode the cost sees).  There ``P`` is NaN and
    ``J`` is ``+inf``, so that ``J < bound`` is false - the convention of ``closed_loop_poles``, not the zeros of ``solve_dare``;
    ``iters`` and ``change`` hold what was reached.  No other problem is affected; a problem's results are bitwise the same at any
    position of any batch.  Enqueued on torch's current stream; nothing waits for the GPU and nothing is copied to the host."""
    import torch

    fn = "closed_loop_cost"
    sim = _sim(data)
    dev = torch.device(f"cuda:{sim.device}")
    if (B is None) != (K is None):
        raise ConfigError(f"{fn}: B and K must be given together (both None: M = A)")
    if R is not None and K is None:
        raise ConfigError(f"{fn}: R needs K (the cost term is K' R K)")
    for name, x in (("A", A), ("B", B), ("K", K), ("Q", Q), ("R", R)):
        if x is not None and (not isinstance(x, torch.Tensor) or x.ndim not in (2, 3)):
            raise ConfigError(f"{fn}: {name} must be a float64 torch tensor [nb, n, m] or [n, m] on {dev}")
    if x0 is not None and (not isinstance(x0, torch.Tensor) or x0.ndim not in (1, 2)):
        raise ConfigError(f"{fn}: x0 must be a float64 torch tensor [nb, nx] or [nx] on {dev}")
    nx = int(A.shape[-1])
    nu = 0 if B is None else int(B.shape[-1])
    if feedback_sign not in (-1, 1) or isinstance(feedback_sign, bool):
        raise ConfigError(f"{fn}: feedback_sign must be -1 or +1")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= max_iter <= 64 or not (tol >= 0):
        raise ConfigError(f"{fn}: max_iter must be an integer in [1, 64] and tol >= 0")
    given = [("A", A, (nx, nx)), ("B", B, (nx, nu)), ("K", K, (nu, nx)), ("Q", Q, (nx, nx)), ("R", R, (nu, nu)), ("x0", x0, (nx,))]
    lead = {name: int(x.shape[0]) for name, x, trail in given if x is not None and x.ndim == len(trail) + 1}
    if len(set(lead.values())) > 1:
        raise ConfigError(f"{fn}: the leading sizes differ: {lead}")
    nb = next(iter(lead.values())) if lead else 1
    if nb < 1:
        raise ConfigError(f"{fn}: at least one problem is required")
    arrays, keep = {}, []
    for name, x, trail in given:                                   # one step per problem: [nb, 1, *trail] views through _strided
        if x is not None and x.ndim == len(trail) + 1:
            x = x.unsqueeze(1)
        p, _, es, t = _strided(fn, name, x, trail, nb, 1, dev, False, optional=name in ("B", "K", "R", "x0"))
        arrays[name] = (p, 0, es); keep.append(t)
    opt = dict(dtype=torch.float64, device=dev)
    P, change = torch.empty((nb, nx, nx), **opt), torch.empty((nb,), **opt)
    J = None if x0 is None else torch.empty((nb,), **opt)
    iters, status = torch.empty((nb,), dtype=torch.int32, device=dev), torch.empty((nb,), dtype=torch.int32, device=dev)
    sim.lqr_dlyap({"batch": nb, "nx": nx, "nu": nu, "feedback_sign": int(feedback_sign), "transpose": int(bool(transpose)),
                   "max_iter": int(max_iter), "tol": float(tol)}, arrays,
                  {"P": P.data_ptr(), "J": 0 if J is None else J.data_ptr(), "change": change.data_ptr(), "iters": iters.data_ptr(),
                   "status": status.data_ptr()}, keep=keep)
    return LyapResult(P, J, status, iters, change)


class TrajCostResult(NamedTuple):
    cost: object     # [B] float64; +inf where the sum is not finite
    cost_t: object   # [B, T + 1]
    lx: object       # [B, T, nx] (a permuted view of the [T, B, nx] block lqr_backward reads in place), or None
    lu: object       # [B, T, nu], or None
    VxT: object      # [B, nx], or None


class TrajSelectResult(NamedTuple):
    u: object          # [nprob, T, nu] (``out`` itself when given)
    best: object       # [nprob] int32: lowest index among the candidates of minimal finite cost, -1 when none is finite
    best_cost: object  # [nprob] float64 (+inf when none is finite)
    weights: object    # [nprob, ncand] float64 (softmin), or None


def _dtype_code(t):
    import torch

    return 0 if t.dtype == torch.float32 else 1


def trajectory_cost(data, state, control, *, initial_state, Q, R, Qf, x_ref=None, u_ref=None, gradients: bool = True) -> TrajCostResult:
    """The quadratic cost of ``B`` trajectories of ``T + 1`` points and its first-order expansion, on the GPU (``mjb_traj_cost``)::

        dx_t = [differentiatePos(qref_t -> qpos_t) ; qvel_t - vref_t]     du_t = u_t - uref_t          (2nv tangent space, float64)
        cost = sum_{t<T} (dx_t' Q_t dx_t + du_t' R_t du_t) / 2 + dx_T' Qf dx_T / 2
        lx[:, t] = Q_t dx_t     lu[:, t] = R_t du_t     VxT = Qf dx_T

    ``state [B, T, 1+nq+nv]`` as ``rollout`` / ``linearize_rollout`` return it (float32 or float64, read in place: row ``t`` is the
    state after step ``t``, the time column is skipped), ``control [B, T, nu]`` or ``[T, nu]`` (float32 or float64),
    ``initial_state [B, 1+nq+nv]`` or ``[1+nq+nv]`` (converted to ``state``'s dtype if it differs - the rounding the rollout applied
    to it).  ``x_ref [nq+nv]`` or ``[B, T+1, nq+nv]`` float64 (``None``: the model's ``qpos0`` at zero velocity), ``u_ref [nu]`` or
    ``[B, T, nu]`` (``None``: 0); ``Q [nx, nx]`` or ``[B, T, nx, nx]`` with ``nx = 2 nv``, ``R [nu, nu]`` or ``[B, T, nu, nu]``,
    ``Qf [nx, nx]`` or ``[B, nx, nx]``, float64, taken as symmetric.  ``B`` is ``state``'s and need not be the data's batch; the model
    (``nq, nv, nu``, the joint table) is the data's.  ``gradients=False`` leaves ``lx, lu, VxT`` out (a line search needs the cost only).

    A trajectory whose cost is NaN or infinite gets ``cost = +inf``; the others are unaffected.  A trajectory's results are bitwise
    the same at any position of any batch.  Enqueued on torch's current stream; nothing waits for the GPU."""
    import torch

    fn = "trajectory_cost"
    sim = _sim(data)
    dev = torch.device(f"cuda:{sim.device}")
    m = sim.model.compiled
    nq, nv, nu = int(m.nq), int(m.nv), int(m.nu)
    nx, ns = 2 * nv, 1 + nq + nv
    both = (torch.float32, torch.float64)
    if not isinstance(state, torch.Tensor) or state.ndim != 3 or state.shape[2] != ns:
        raise ConfigError(f"{fn}: state must be a [B, T, {ns}] tensor (time, qpos, qvel)")
    nb, T = int(state.shape[0]), int(state.shape[1])
    if nb < 1 or T < 1:
        raise ConfigError(f"{fn}: state must hold at least one trajectory of one step")
    arrays, keep = {}, []
    p, ss, es, state = _strided(fn, "state", state, (ns,), nb, T, dev, False, dtypes=both)
    size, code = state.element_size(), _dtype_code(state)
    arrays["qpos"] = (p + size, ss, es, code); arrays["qvel"] = (p + size * (1 + nq), ss, es, code); keep.append(state)
    if isinstance(control, torch.Tensor) and control.ndim == 2 and tuple(control.shape) == (T, nu):
        control = control.unsqueeze(0).expand(nb, T, nu)
    if not isinstance(control, torch.Tensor) or tuple(control.shape) != (nb, T, nu):
        raise ConfigError(f"{fn}: control must be a tensor [{nb}, {T}, {nu}] or [{T}, {nu}]")
    p, ss, es, control = _strided(fn, "control", control, (nu,), nb, T, dev, False, dtypes=both)
    arrays["ctrl"] = (p, ss, es, _dtype_code(control)); keep.append(control)
    x0 = initial_state
    if not isinstance(x0, torch.Tensor) or x0.dtype not in both or x0.device != dev or tuple(x0.shape) not in ((ns,), (nb, ns)):
        raise ConfigError(f"{fn}: initial_state must be a float32 or float64 tensor [{nb}, {ns}] or [{ns}] on {dev}")
    if x0.dtype != state.dtype:
        x0 = x0.to(state.dtype)
    if x0.stride(-1) != 1:
        x0 = x0.contiguous()
    es0 = x0.stride(0) if x0.ndim == 2 else 0
    arrays["qpos0"] = (x0.data_ptr() + size, 0, es0, code); arrays["qvel0"] = (x0.data_ptr() + size * (1 + nq), 0, es0, code); keep.append(x0)
    if x_ref is None:
        x_ref = sim.__dict__.get("_traj_x_ref0")                 # the model's qpos0 at rest, uploaded once per data object
        if x_ref is None or x_ref.device != dev:
            import numpy as np

            x_ref = torch.as_tensor(np.concatenate([np.asarray(m.qpos0, dtype=np.float64).reshape(-1), np.zeros(nv)])).to(dev)
            sim.__dict__["_traj_x_ref0"] = x_ref
    if not isinstance(x_ref, torch.Tensor) or x_ref.dtype != torch.float64 or x_ref.device != dev or \
            tuple(x_ref.shape) not in ((nq + nv,), (nb, T + 1, nq + nv)):
        raise ConfigError(f"{fn}: x_ref must be a float64 tensor [{nq + nv}] or [{nb}, {T + 1}, {nq + nv}] on {dev}")
    if x_ref.stride(-1) != 1:
        x_ref = x_ref.contiguous()
    rs, re = (x_ref.stride(1), x_ref.stride(0)) if x_ref.ndim == 3 else (0, 0)
    arrays["qref"] = (x_ref.data_ptr(), rs, re); arrays["vref"] = (x_ref.data_ptr() + 8 * nq, rs, re); keep.append(x_ref)
    for name, x, trail, opt in (("uref", u_ref, (nu,), True), ("Q", Q, (nx, nx), False), ("R", R, (nu, nu), False)):
        p, ss, es, t = _strided(fn, "u_ref" if name == "uref" else name, x, trail, nb, T, dev, False, optional=opt)
        arrays[name] = (p, ss, es); keep.append(t)
    if not isinstance(Qf, torch.Tensor) or Qf.dtype != torch.float64 or Qf.device != dev or tuple(Qf.shape) not in ((nx, nx), (nb, nx, nx)):
        raise ConfigError(f"{fn}: Qf must be a float64 tensor [{nb}, {nx}, {nx}] or [{nx}, {nx}] on {dev}")
    if not (Qf if Qf.ndim == 2 else Qf[0]).is_contiguous():
        Qf = Qf.contiguous()
    arrays["Qf"] = (Qf.data_ptr(), 0, 0 if Qf.ndim == 2 else Qf.stride(0)); keep.append(Qf)
    for name, v in arrays.items():
        if v[1] < 0 or v[2] < 0:
            raise ConfigError(f"{fn}: {name} has a negative stride")
    opt = dict(dtype=torch.float64, device=dev)
    cost, cost_t = torch.empty((nb,), **opt), torch.empty((nb, T + 1), **opt)
    lx = lu = VxT = None
    if gradients:
        lx, lu, VxT = torch.empty((T, nb, nx), **opt), torch.empty((T, nb, nu), **opt), torch.empty((nb, nx), **opt)
    sim.traj_cost({"T": T, "batch": nb}, arrays,
                  {"cost": cost.data_ptr(), "cost_t": cost_t.data_ptr(), "lx": lx.data_ptr() if gradients else 0,
                   "lu": lu.data_ptr() if gradients else 0, "VxT": VxT.data_ptr() if gradients else 0}, keep=keep)
    if gradients:
        lx, lu = lx.permute(1, 0, 2), lu.permute(1, 0, 2)
    return TrajCostResult(cost, cost_t, lx, lu, VxT)


def select_candidates(data, cost, cand, *, mode: str = "argmin", temperature=None, out=None, dtype=None) -> TrajSelectResult:
    """Choose among, or blend, ``ncand`` candidate control sequences for each of ``nprob`` problems on the GPU (``mjb_traj_select``).
    ``cost [nprob, ncand]`` float64, ``cand [nprob, ncand, T, nu]`` float32 or float64 (what ``lqr_candidates`` returns; for a
    sampling planner the control tensor itself with a leading axis of 1).

    ``mode="argmin"``: ``u[g] = cand[g, best[g]]`` with ``best`` the lowest index among the candidates of minimal finite cost.
    ``mode="softmin"`` (the MPPI update): ``u[g] = sum_j w_j cand[g, j]`` with ``w_j = exp(-(c_j - c_min) / temperature)`` over the
    finite costs (0 for the others), normalised; accumulated in float64 and rounded once; ``weights`` holds the ``w_j``.
    A problem without any finite cost gets ``best = -1``, ``best_cost = +inf`` and its ``u`` is NOT written: pass the nominal controls
    as ``out [nprob, T, nu]`` and they are updated in place or kept (without ``out`` the result starts as zeros).  ``dtype``: the
    result's (``out``'s when given; ``cand``'s by default).  Enqueued on torch's current stream; nothing waits for the GPU."""
    import torch

    fn = "select_candidates"
    sim = _sim(data)
    dev = torch.device(f"cuda:{sim.device}")
    both = (torch.float32, torch.float64)
    if mode not in ("argmin", "softmin"):
        raise ConfigError(f"{fn}: mode must be 'argmin' or 'softmin', got {mode!r}")
    if mode == "softmin" and temperature is None:
        raise ConfigError(f"{fn}: mode 'softmin' needs a temperature")
    if not isinstance(cand, torch.Tensor) or cand.ndim != 4 or cand.dtype not in both or cand.device != dev:
        raise ConfigError(f"{fn}: cand must be a float32 or float64 tensor [nprob, ncand, T, nu] on {dev}")
    G, n, T, nu = (int(v) for v in cand.shape)
    if not isinstance(cost, torch.Tensor) or cost.dtype != torch.float64 or cost.device != dev or tuple(cost.shape) != (G, n):
        raise ConfigError(f"{fn}: cost must be a float64 tensor [{G}, {n}] on {dev}")
    cost, cand = cost.contiguous(), cand.contiguous()
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype not in both or out.device != dev or tuple(out.shape) != (G, T, nu) or not out.is_contiguous():
            raise ConfigError(f"{fn}: out must be a contiguous float32 or float64 tensor [{G}, {T}, {nu}] on {dev}")
        if dtype is not None and dtype != out.dtype:
            raise ConfigError(f"{fn}: dtype {dtype} differs from out's {out.dtype}")
        u = out
    else:
        dtype = cand.dtype if dtype is None else dtype
        if dtype not in both:
            raise ConfigError(f"{fn}: dtype must be torch.float64 or torch.float32")
        u = torch.zeros((G, T, nu), dtype=dtype, device=dev)
    best = torch.empty((G,), dtype=torch.int32, device=dev)
    best_cost = torch.empty((G,), dtype=torch.float64, device=dev)
    weights = torch.empty((G, n), dtype=torch.float64, device=dev) if mode == "softmin" else None
    sim.traj_select({"nprob": G, "ncand": n, "T": T, "nu": nu, "mode": int(mode == "softmin"), "cand_dtype": _dtype_code(cand),
                     "out_dtype": _dtype_code(u), "temperature": 0.0 if temperature is None else float(temperature)},
                    {"cost": cost.data_ptr(), "cand": cand.data_ptr(), "u_out": u.data_ptr(), "best": best.data_ptr(),
                     "best_cost": best_cost.data_ptr(), "weights": weights.data_ptr() if weights is not None else 0}, keep=[cost, cand, u])
    return TrajSelectResult(u, best, best_cost, weights)


__all__ = ["LqrBackwardResult", "LqrBoxResult", "lqr_backward", "lqr_candidates", "DareResult", "solve_dare", "KalmanResult", "solve_kalman", "PolesResult", "closed_loop_poles", "TrajCostResult", "TrajSelectResult", "trajectory_cost", "select_candidates"]
