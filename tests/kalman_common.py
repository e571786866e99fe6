"""Shared by tests/test_kalman_host.py and tests/test_gpu_kalman.py: seeded estimation problems and their scipy solution.  Not a test module."""
import numpy as np

SIZES = [(1, 1), (4, 2), (12, 10), (54, 32)]
NB = 3


def systems(nx, ny, nb=NB, seed=0):
    """nb random systems: A with spectral radius spread over 0.9 .. 1.05, a full C, W and V positive definite."""
    rng = np.random.default_rng(7000 + 100 * nx + ny + seed)
    A, C, W, V = [], [], [], []
    for e in range(nb):
        M = rng.normal(size=(nx, nx))
        A.append(M * (np.linspace(0.9, 1.05, nb)[e] / np.abs(np.linalg.eigvals(M)).max()))
        C.append(rng.normal(size=(ny, nx)))
        G, H = rng.normal(size=(nx, nx)) / np.sqrt(nx), rng.normal(size=(ny, ny)) / np.sqrt(ny)
        W.append(0.1 * np.eye(nx) + G @ G.T)
        V.append(0.1 * np.eye(ny) + H @ H.T)
    return {k: np.stack(v) for k, v in (("A", A), ("C", C), ("W", W), ("V", V))}


def scipy_kalman(A, C, W, V):
    """(P, L) of one system: P from scipy's DARE of the dual problem, L = A P C' (C P C' + V)^-1 written out."""
    from scipy.linalg import solve_discrete_are

    P = solve_discrete_are(A.T, C.T, W, V)
    L = A @ P @ C.T @ np.linalg.inv(C @ P @ C.T + V)
    return P, L
