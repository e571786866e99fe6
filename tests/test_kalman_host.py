"""``solve_kalman`` without a GPU: the wrapper's transposition and sign, with ``solve_dare`` replaced by a scipy stand-in."""
import numpy as np
import pytest

from tests import kalman_common as kc


def _stand_in(calls):
    import torch
    from scipy.linalg import solve_discrete_are

    from mujoco_template_amd.trajopt import DareResult

    def solve_dare(data, A, B, Q, R, *, tol=1e-12, max_iter=32):
        calls.append((A, B, Q, R))
        for x in (A, B):
            assert (x[0] if x.ndim == 3 else x).is_contiguous()        # what the kernel needs of a trailing block
        nb = max(x.shape[0] if x.ndim == 3 else 1 for x in (A, B, Q, R))
        pick = lambda x, e: (x[e] if x.ndim == 3 else x).numpy()        # noqa: E731
        X, K = [], []
        for e in range(nb):
            a, b, q, r = (pick(x, e) for x in (A, B, Q, R))
            x = solve_discrete_are(a, b, q, r)
            X.append(x); K.append(np.linalg.solve(r + b.T @ x @ b, b.T @ x @ a))
        z = torch.zeros(nb, dtype=torch.int32)
        return DareResult(torch.from_numpy(np.stack(X)), torch.from_numpy(np.stack(K)), z, z.clone(), torch.zeros(nb, dtype=torch.float64))

    return solve_dare


@pytest.mark.parametrize("shared_c", [False, True], ids=["per_system_C", "shared_C"])
@pytest.mark.parametrize("nx,ny", kc.SIZES[:3])
def test_solve_kalman_is_the_dual_dare(monkeypatch, nx, ny, shared_c):
    import torch

    from mujoco_template_amd import trajopt

    calls = []
    monkeypatch.setattr(trajopt, "solve_dare", _stand_in(calls))
    s = kc.systems(nx, ny)
    if shared_c:
        s["C"] = s["C"][0]
    t = {k: torch.from_numpy(v) for k, v in s.items()}
    res = trajopt.solve_kalman(None, t["A"], t["C"], t["W"], t["V"])
    assert isinstance(res, trajopt.KalmanResult) and tuple(res.L.shape) == (kc.NB, nx, ny) and tuple(res.P.shape) == (kc.NB, nx, nx)
    assert calls[0][1].ndim == (2 if shared_c else 3)                  # a shared block stays shared
    for e in range(kc.NB):
        C = s["C"] if shared_c else s["C"][e]
        P, L = kc.scipy_kalman(s["A"][e], C, s["W"][e], s["V"][e])
        assert np.abs(res.P[e].numpy() - P).max() <= 1e-9 * np.abs(P).max()
        assert np.abs(res.L[e].numpy() - L).max() <= 1e-9 * max(1.0, np.abs(L).max())
        # the predictor's error dynamics A - L C are stable, and P solves the filter Riccati equation
        Ln = res.L[e].numpy()
        assert np.abs(np.linalg.eigvals(s["A"][e] - Ln @ C)).max() < 1.0
        A, W, V = s["A"][e], s["W"][e], s["V"][e]
        rhs = A @ P @ A.T - A @ P @ C.T @ np.linalg.solve(C @ P @ C.T + V, C @ P @ A.T) + W
        assert np.abs(rhs - res.P[e].numpy()).max() <= 1e-8 * np.abs(P).max()


def test_solve_kalman_rejects_mismatched_shapes():
    import torch

    from mujoco_template_amd import ConfigError, solve_kalman

    A, C = torch.eye(3, dtype=torch.float64), torch.ones((2, 4), dtype=torch.float64)
    with pytest.raises(ConfigError):
        solve_kalman(None, A, C, A, torch.eye(2, dtype=torch.float64))
    with pytest.raises(ConfigError):
        solve_kalman(None, A.numpy(), C, A, A)
