"""Shared by tests/test_eig_host.py and tests/test_gpu_eig.py: the yardstick of ``mjb_lqr_eig``.  Not a test module.

The yardstick is never the kernel: LAPACK through ``numpy.linalg.eigvals``.  The measure is a backward error that does not depend on
the conditioning of the eigenvalues, ``be(Mb, w) = max_i sigma_min(Mb - w_i I) / ||Mb||_2`` with ``Mb = D^-1 M D`` formed here from
``M`` and the returned ``scale``; the kernel's figure must lie within ``lqr_common.bound`` (8 x, floor 1e-13) of LAPACK's own on the
same matrix.

A solver is ``solve(A, B=None, K=None, feedback_sign=-1, balance=True, max_sweeps=None)`` on numpy arrays (``A [n, nx, nx]``,
``B [n, nx, nu]``, ``K [n, nu, nx]`` or the shared ``[nu, nx]``) returning a dict of numpy arrays wr, wi, scale [n, nx], rho, status,
sweeps [n]."""
from __future__ import annotations

from decimal import Decimal, localcontext

import numpy as np

from tests import dare_common as dc
from tests.lqr_common import bound

GAUSS_SIZES = [1, 2, 3, 4, 7, 16, 17, 33, 64]
KEYS = ("wr", "wi", "rho", "status", "sweeps", "scale")


def exact_hypot(x, y):
    """The correctly rounded sqrt(x^2 + y^2) (200 decimal digits, rounded once to float64): what the kernel's modulus is specified as."""
    with localcontext() as c:
        c.prec = 200
        return float((Decimal(float(x)) ** 2 + Decimal(float(y)) ** 2).sqrt())


def backward_error(M, w):
    """max_i sigma_min(M - w_i I) / ||M||_2 (the denominator 1 for the zero matrix)."""
    n = M.shape[0]
    den = np.linalg.norm(M, 2) if n else 0.0
    den = den if den > 0 else 1.0
    eye = np.eye(n)
    return max(np.linalg.svd(M - wi * eye, compute_uv=False)[-1] for wi in w) / den


def balanced(M, scale):
    return M * scale[None, :] / scale[:, None]


def check_properties(got, label):
    """What holds for every problem that ended with status 0: scale exact powers of two, the order, exact conjugate pairs, rho."""
    wr, wi, rho, scale = (np.asarray(got[k]) for k in ("wr", "wi", "rho", "scale"))
    for e in range(wr.shape[0]):
        assert int(got["status"][e]) == 0, (label, e, got["status"])
        n = wr.shape[1]
        mant, _ = np.frexp(scale[e])
        assert (scale[e] > 0).all() and (mant == 0.5).all(), (label, e, scale[e])
        mod = [exact_hypot(wr[e, i], wi[e, i]) for i in range(n)]
        key = [(-mod[i], -wr[e, i], -wi[e, i]) for i in range(n)]
        assert key == sorted(key), (label, e, "order", list(zip(wr[e], wi[e])))
        assert rho[e].tobytes() == np.float64(mod[0]).tobytes(), (label, e, rho[e], mod[0])
        i = 0
        while i < n:
            if wi[e, i] == 0.0:
                i += 1
                continue
            assert i + 1 < n and wi[e, i] > 0 and wr[e, i].tobytes() == wr[e, i + 1].tobytes() and \
                (-wi[e, i]).tobytes() == wi[e, i + 1].tobytes(), (label, e, i, "conjugate pair", wr[e], wi[e])
            i += 2


def judge(M, got, label, record=None, balance=True):
    """The comparison every test makes, per launch: M [n, nx, nx] (formed here, in numpy), got = the solver's outputs.  Returns the
    kernel's eigenvalues as complex [n, nx]."""
    n = M.shape[0]
    assert np.asarray(got["status"]).tolist() == [0] * n, (label, got["status"])
    check_properties(got, label)
    if not balance:
        assert np.array_equal(got["scale"], np.ones_like(got["scale"])), label
    w = np.asarray(got["wr"]) + 1j * np.asarray(got["wi"])
    mine, ref = 0.0, 0.0
    for e in range(n):
        Mb = balanced(M[e], got["scale"][e])
        mine = max(mine, backward_error(Mb, w[e]))
        ref = max(ref, backward_error(Mb, np.linalg.eigvals(Mb)))
    print(f"{label} backward error: kernel {mine:.2e}  LAPACK {ref:.2e}  bound {bound(ref):.2e}")
    if record:
        record(f"{label}/backward_error", mine, bound(ref))
    assert mine <= bound(ref), (label, mine, ref)
    return w


# ---- the cases, all seeded ------------------------------------------------------------------------------------------------------------
def gauss_case(nx, n, seed=0):
    return np.random.default_rng(7000 + 100 * seed + nx).normal(size=(n, nx, nx)) / np.sqrt(nx)


_LOOPS = {}


def closed_loop_case(kind, nx, nu, n):
    """A, B of dare_common's generators and K from its float64 restatement (computed once per size, left unchanged)."""
    key = (kind, nx, nu, n)
    if key not in _LOOPS:
        c = (dc.mechanical_case if kind == "mech" else dc.generator_case)(nx, nu, n)
        K = []
        for e in range(n):
            r = dc.restate(c["A"][e], c["B"][e], c["Q"][e], c["R"][e], np.float64)
            assert r["status"] == 0
            K.append(r["K"])
        _LOOPS[key] = (c["A"], c["B"], np.stack(K))
    return tuple(x.copy() for x in _LOOPS[key])


LOOP_SIZES = [("mech", 6, 2), ("mech", 54, 21), ("gen", 64, 32)]


def humanoid_loop():
    key = "humanoid"
    if key not in _LOOPS:
        c = dc.humanoid_case()
        r = dc.restate(c["A"][0], c["B"][0], c["Q"][0], c["R"][0], np.float64)
        assert r["status"] == 0
        _LOOPS[key] = (c["A"], c["B"], r["K"][None])
    return tuple(x.copy() for x in _LOOPS[key])


def normal_case():
    """Q diag(blocks) Q' with Q orthogonal, n = 17: eight rotation-scaled 2 x 2 blocks and one real pole, moduli in 0.2 .. 1.1.
    Returns (M [1, 17, 17], the known eigenvalues [17])."""
    rng = np.random.default_rng(4242)
    n = 17
    mod, ang = np.linspace(0.2, 1.1, 9), rng.uniform(0.2, 2.9, size=8)
    D = np.zeros((n, n))
    w = []
    for b in range(8):
        c, s = mod[b] * np.cos(ang[b]), mod[b] * np.sin(ang[b])
        D[2 * b:2 * b + 2, 2 * b:2 * b + 2] = [[c, -s], [s, c]]
        w += [c + 1j * s, c - 1j * s]
    D[16, 16] = -mod[8]
    w.append(-mod[8] + 0j)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return (Q @ D @ Q.T)[None], np.array(w)


def matching_error(w, known):
    """The largest distance in the best one-to-one matching of w to the known eigenvalues."""
    from scipy.optimize import linear_sum_assignment

    cost = np.abs(np.asarray(w)[:, None] - np.asarray(known)[None, :])
    r, c = linear_sum_assignment(cost)
    return float(cost[r, c].max())


def degenerate_cases():
    """(name, M, the eigenvalues where they can be read off the matrix, else None)"""
    rng = np.random.default_rng(99)
    g = rng.normal(size=(7, 7)) / np.sqrt(7)
    zc = g.copy()
    zc[:, 2] = 0.0
    d, t = np.diag(rng.normal(size=7)), np.triu(rng.normal(size=(7, 7)))
    return [("zero", np.zeros((5, 5)), np.zeros(5)), ("identity", np.eye(6), np.ones(6)), ("diagonal", d, np.diag(d).copy()),
            ("triangular", t, np.diag(t).copy()), ("hessenberg", np.triu(rng.normal(size=(9, 9)), -1), None), ("zerocol7", zc, None)]


# ---- the checks both suites run, given a solver ---------------------------------------------------------------------------------------
def check_gauss(solve, nx, label, record=None, n=2):
    M = gauss_case(nx, n)
    judge(M, solve(M), f"{label}/gauss{nx}", record)


def check_closed_loop(solve, kind, nx, nu, label, record=None, n=2):
    """K per problem, then ONE K (the first) shared by every problem."""
    A, B, K = closed_loop_case(kind, nx, nu, n)
    judge(A - B @ K, solve(A, B, K), f"{label}/{kind}{nx}x{nu}", record)
    judge(A - B @ K[0], solve(A, B, K[0]), f"{label}/{kind}{nx}x{nu}_sharedK", record)


def check_humanoid(solve, label, record=None):
    """The humanoid balance design, balanced and not; rho against numpy's to 1e-6."""
    A, B, K = humanoid_loop()
    M = A - B @ K
    ref = np.abs(np.linalg.eigvals(M[0])).max()
    for bal in (True, False):
        got = solve(A, B, K, balance=bal)
        judge(M, got, f"{label}/humanoid_{'balanced' if bal else 'plain'}", record, balance=bal)
        print(f"{label} humanoid balance={bal}: rho {got['rho'][0]:.12f}  numpy {ref:.12f}  sweeps {got['sweeps'][0]}  "
              f"scale {got['scale'][0].min()} .. {got['scale'][0].max()}")
        if record:
            record(f"{label}/humanoid_{'balanced' if bal else 'plain'}/rho", abs(got["rho"][0] - ref), 1e-6)
        assert abs(got["rho"][0] - ref) <= 1e-6, (bal, got["rho"][0], ref)


def check_normal(solve, label, record=None):
    M, known = normal_case()
    w = judge(M, solve(M), f"{label}/normal17", record)
    mine, ref = matching_error(w[0], known), matching_error(np.linalg.eigvals(M[0]), known)
    print(f"{label} normal17 matching error: kernel {mine:.2e}  LAPACK {ref:.2e}  bound {bound(ref):.2e}")
    if record:
        record(f"{label}/normal17/matching", mine, bound(ref))
    assert mine <= bound(ref), (mine, ref)


def check_degenerate(solve, label, record=None):
    """Each against LAPACK by the backward error; where the spectrum can be read off the matrix, also matched to it within ``bound`` of
    LAPACK's own matching error.  The zero-column matrix must report a zero eigenvalue exactly as LAPACK does: to within the bound."""
    for name, M, known in degenerate_cases():
        w = judge(M[None], solve(M[None]), f"{label}/{name}", record)
        if known is not None:
            mine, ref = matching_error(w[0], known), matching_error(np.linalg.eigvals(M), known)
            print(f"{label} {name} matching error: kernel {mine:.2e}  LAPACK {ref:.2e}  bound {bound(ref):.2e}")
            if record:
                record(f"{label}/{name}/matching", mine, bound(ref))
            assert mine <= bound(ref), (name, mine, ref)


def check_sign(solve, label):
    """feedback_sign = +1 with -K is bitwise feedback_sign = -1 with K."""
    A, B, K = closed_loop_case("mech", 6, 2, 2)
    a, b = solve(A, B, K, feedback_sign=-1), solve(A, B, -K, feedback_sign=1)
    for k in KEYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (label, k)
    assert np.asarray(a["status"]).tolist() == [0, 0]


def check_statuses(solve, label):
    """Five 7 x 7 Gaussian problems: a NaN in A[2]; max_sweeps = 1; the isolation and the independence of the batch position."""
    M = gauss_case(7, 5, seed=3)
    good = solve(M)
    assert np.asarray(good["status"]).tolist() == [0] * 5 and (np.asarray(good["sweeps"]) > 1).all(), (label, good["status"], good["sweeps"])
    bad = M.copy()
    bad[2, 3, 4] = np.nan
    got = solve(bad)
    assert np.asarray(got["status"]).tolist() == [0, 0, 1, 0, 0], (label, got["status"])
    assert np.isnan(got["wr"][2]).all() and np.isnan(got["wi"][2]).all() and got["rho"][2] == np.inf and not (got["rho"][2] < 1), label
    assert got["sweeps"][2] == 0 and np.array_equal(got["scale"][2], np.ones(7))
    keep = [0, 1, 3, 4]
    alone = solve(bad[keep])
    for k in KEYS:
        assert np.asarray(got[k])[keep].tobytes() == np.asarray(alone[k]).tobytes(), (label, "isolation", k)
        assert np.asarray(got[k])[keep].tobytes() == np.asarray(good[k])[keep].tobytes(), (label, "neighbour", k)
    capped = solve(M, max_sweeps=1)
    assert np.asarray(capped["status"]).tolist() == [2] * 5 and np.asarray(capped["sweeps"]).tolist() == [1] * 5, (label, capped["status"], capped["sweeps"])
    assert np.isnan(capped["wr"]).all() and np.isnan(capped["wi"]).all() and (capped["rho"] == np.inf).all(), label
    mant, _ = np.frexp(capped["scale"])
    assert (mant == 0.5).all()
    # one problem at positions 0 and 4 of a batch of five, and alone
    first, last, one = solve(M[[0, 1, 2, 3, 4]]), solve(M[[4, 1, 2, 3, 0]]), solve(M[[0]])
    for k in KEYS:
        assert np.asarray(first[k])[0].tobytes() == np.asarray(last[k])[4].tobytes() == np.asarray(one[k])[0].tobytes(), (label, "position", k)
