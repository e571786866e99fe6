// mjb_dare.hpp — the infinite-horizon LQR design (mjb_lqr_dare): the stabilising solution X of the discrete algebraic Riccati equation
//   A' X A - X - A' X B (R + B' X B)^-1 B' X A + Q = 0
// and the gain K = (R + B' X B)^-1 B' X A, for a batch of systems, as workgroup-cooperative float64 device code.  It is what the
// reference gets from scipy.linalg.solve_discrete_are, one system at a time on the host (reference
// examples/humanoid/controllers/lqr.py:114, examples/drone/controllers/lqr.py:358-369).
//
// The structure-preserving doubling algorithm (SDA): iteration k holds the data of 2^k steps of the Riccati recursion, so a dozen
// iterations reach what the plain recursion (mjb_lqr_backward) needs thousands of steps for, marginal closed-loop modes included.
//   R = L L' (Cholesky),  G_0 = sym(B R^-1 B'),  H_0 = Q,  A_0 = A
//   W = I + G_k H_k;  LU of W with partial pivoting (the pivot row: the LOWEST index among the rows of largest |.|)
//   X_A = W^-1 A_k,  X_G = W^-1 G_k
//   H_{k+1} = sym(H_k + A_k' (H_k X_A)),  G_{k+1} = sym(G_k + A_k X_G A_k'),  A_{k+1} = A_k X_A
//   change = max|H_{k+1} - H_k| / max|H_{k+1}|;  stop on change <= tol or after max_iter iterations - never on stagnation
//   X = H (bitwise symmetric),  K = (R + B' X B)^-1 B' X A (Cholesky)
// K has the sign of the reference and of mjb_set_feedback (u = u0 - K dx): the NEGATIVE of lqr_backward_env's K.  Q and R are taken
// as symmetric: only their LOWER triangles are read.
//
// One workgroup per problem, lqr_waves(nx) waves, every iterate resident in LDS, every nx x nx product on v_mfma_f64_16x16x4_f64
// through the fragment maps of lqr_gemm_tn (dare_gemm: the same tile loop with the operands given as accessors, so that a packed or a
// transposed operand costs no copy).  G and H share one nx x (nx + 1) buffer, H in the lower triangle and G in the upper one.
// The same source compiles in the host emulation of mjb_lqr.hpp (MJB_HOST_EMU), which only the CPU test-suite uses.
#pragma once
#include "mjb_lqr.hpp"

namespace mjb {

static const int kDareMaxIter = 64;

struct DareArgs {
  int B, nx, nu, max_iter;
  double tol;
  LqrStrided A, Bm, Q, R;                           // per problem e: p + e * es (ss unused)
  double *X, *K, *change;                           // [B, nx, nx], [B, nu, nx], [B] (change may be null)
  int *iters, *status;                              // [B]
};

// ---- LDS layout (offsets in doubles) --------------------------------------------------------------------------------------------
// S: the packed G / H pair, row stride nx + 1.  A, W, X: nx x nx with row stride ld = nx | 1 (odd: the products that read a left
// operand down its rows meet no bank conflict).  perm: the row permutation of the LU.  red: two partial maxima per thread.  XL: the
// low parts of X during a substitution, nx x ld floats.  W, X and XL are one region with the nu-sized blocks of the start (G_0) and of
// the end (K), when no iterate but S and A is live: Bm [nx, nu], Z [nu, nx] (B' solved in place into R^-1 B'; at the end B' X A), XB [nx, nu], M [nu, nu], L [nu, kLqrMaxNu].
struct DareLay { int S, A, perm, red, W, X, XL, Bm, Z, XB, M, L, ld, lds, total; };
MJB_LQR_HD DareLay dare_layout(int nx, int nu) {
  DareLay l;
  l.ld = nx | 1; l.lds = nx + 1;
  const int nt = 64 * lqr_waves(nx);
  int o = 0;
  l.S = o; o += nx * l.lds;
  l.A = o; o += nx * l.ld;
  l.perm = o; o += nx;
  l.red = o; o += 2 * nt;
  const int u0 = o;
  l.W = o; o += nx * l.ld;
  l.X = o; o += nx * l.ld;
  l.XL = o; o += (nx * l.ld + 1) / 2;
  const int end1 = o;
  o = u0;
  l.Bm = o; o += nx * nu;
  l.Z = o; o += nu * nx;
  l.XB = o; o += nx * nu;
  l.M = o; o += nu * nu;
  l.L = o; o += nu * kLqrMaxNu;
  l.total = o > end1 ? o : end1;
  return l;
}
// the packed pair: H(i, j) at the lower triangle of S, G(i, j) one column to the right of the upper one
MJB_LQR_HD int dare_h_index(int i, int j, int lds) { return i >= j ? i * lds + j : j * lds + i; }
MJB_LQR_HD int dare_g_index(int i, int j, int lds) { return i <= j ? i * lds + j + 1 : j * lds + i + 1; }

// 0 ok; otherwise which limit is broken (the entry point turns it into the message)
inline int dare_size_error(long B, long nx, long nu, long max_iter, double tol) {
  if (B < 1) return 1;
  if (nx < 1 || nx > kLqrMaxNx) return 2;
  if (nu < 1 || nu > kLqrMaxNu) return 3;
  if (max_iter < 1 || max_iter > kDareMaxIter) return 4;
  if (!(tol >= 0.0)) return 5;
  if ((__int128)B * nx * nx > ((__int128)1 << 40)) return 6;
  return 0;
}

MJB_LQR_DEV bool dare_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// C [M, N] = init + sum_k la(k, i) lb(k, j): the tile loop of lqr_gemm_tn (same fragment maps, same tile-to-wave order, at most four
// tiles per wave) with the operands as accessors.  The whole result sits in the accumulators before the first store, so with SYNC a
// barrier separates the last operand read from it and the product may overwrite one of its own operands.
template <int NW, bool SYNC, class LA, class LB, class Init, class Store>
MJB_LQR_DEV void dare_gemm(int M, int N, int K, int tid, LA la, LB lb, Init init, Store store) {
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int nt = (N + 15) >> 4, ntile = ((M + 15) >> 4) * nt;
  lqr_d4 acc[4];
  int ti[4], tj[4];
  bool on[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int q = wave + NW * s;
    on[s] = q < ntile;
    ti[s] = 16 * (q / nt); tj[s] = 16 * (q % nt);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = ti[s] + lk + 4 * r, col = tj[s] + li;
      acc[s][r] = (on[s] && row < M && col < N) ? init(row, col) : 0.0;
    }
  }
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + lk;
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if (!on[s]) continue;                                      // wave-uniform
      const int i = ti[s] + li, j = tj[s] + li;
      const double av = (k < K && i < M) ? la(k, i) : 0.0, bv = (k < K && j < N) ? lb(k, j) : 0.0;
      acc[s] = MJB_MFMA_F64(av, bv, acc[s]);
    }
  }
  if (SYNC) lqr_sync();
#pragma unroll
  for (int s = 0; s < 4; s++) {
    if (!on[s]) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = ti[s] + lk + 4 * r, col = tj[s] + li;
      if (row < M && col < N) store(row, col, acc[s][r]);
    }
  }
}

// Element passes over an n x n block: thread (rg, c) = (tid / CW, tid % CW) owns column c of the rows rg, rg + RG, ...: lanes run
// along a row (no bank conflict), no integer division.  CW = 16 with one wave (nx <= 16), 64 with four.
template <int NW> struct DareMap { static const int CW = NW == 4 ? 64 : 16, RG = 64 * NW / CW; };

// LU of W (row stride ld) in place with partial pivoting: unit L below the diagonal, U on and above it, the rows physically swapped,
// perm[i] = the original row now in place i.  false at a pivot that is zero or not finite - uniform: every thread scans the same column.
template <int NW>
MJB_LQR_DEV bool dare_lu(double* W, int ld, double* perm, int n, int tid) {
  constexpr int CW = DareMap<NW>::CW, RG = DareMap<NW>::RG;
  const int c = tid % CW, rg = tid / CW;
  for (int i = tid; i < n; i += 64 * NW) perm[i] = (double)i;
  lqr_sync();
  for (int j = 0; j < n; j++) {
    const double dj = W[j * ld + j];
    double best = fabs(dj), pv = dj;
    int p = j;
    for (int i = j + 1; i < n; i++) {
      const double w = W[i * ld + j], v = fabs(w);
      if (v > best) { best = v; pv = w; p = i; }
    }
    if (!(best > 0.0) || !dare_finite(best)) return false;
    lqr_sync();
    // the swap of rows j and p (column j: from the values every thread holds) and the multipliers of column j
    if (tid < n) {
      if (tid != j && p != j) { const double a = W[j * ld + tid], b = W[p * ld + tid]; W[j * ld + tid] = b; W[p * ld + tid] = a; }
      if (tid == j) W[j * ld + j] = pv;
      else if (tid > j) W[tid * ld + j] = (tid == p ? dj : W[tid * ld + j]) / pv;
      if (tid == 0 && p != j) { const double a = perm[j]; perm[j] = perm[p]; perm[p] = a; }
    }
    lqr_sync();
    if (c > j && c < n)
      for (int i = j + 1 + rg; i < n; i += RG) W[i * ld + c] = fma(-W[i * ld + j], W[j * ld + c], W[i * ld + c]);
    lqr_sync();
  }
  return true;
}

// The substitutions carry every entry as an unevaluated sum hi + lo (hi in X, lo as a float in XL: 24 more bits are all the
// correction needs).  W = I + G H is ill-conditioned on designs with marginal modes, and there the rounding of the running sums of a
// plain float64 substitution is what limits X: on the humanoid balance design it is 40 x the error of everything else together.
// (hi, lo) -= a (xh + xl): the product and the sum error-free (fma, TwoSum), renormalised so that lo stays a correction of hi
MJB_LQR_DEV void dare_dd_sub(double& hi, double& lo, double a, double xh, double xl) {
  const double p = fma(-a, xh, 0.0), e = fma(-a, xh, -p);        // p + e = -a xh exactly; no bare product: nothing to contract
  const double s = hi + p, bb = s - hi, err = (hi - (s - bb)) + (p - bb);
  const double t = lo + (err + fma(-a, xl, e));
  hi = s + t; lo = t - (hi - s);
}
// (hi, lo) <- (hi + lo) / u
MJB_LQR_DEV void dare_dd_div(double& hi, double& lo, double u) {
  const double q = (hi + lo) / u, r = fma(-q, u, hi) + lo, ql = r / u;
  hi = q + ql; lo = ql - (hi - q);
}
MJB_LQR_DEV float dare_lo(double lo) { return fabs(lo) < 3.0e38 ? (float)lo : 0.0f; }     // a correction no float holds is dropped

// X <- W^-1 X for the factors of dare_lu, X [n, n] (row stride ld) holding the right-hand sides with their rows already permuted:
// column-oriented substitutions, one barrier per column; the division by U's diagonal is done by the thread that finishes a row,
// and the row it finishes holds the rounded sum hi + lo.
template <int NW>
MJB_LQR_DEV void dare_lu_solve(const double* W, double* X, float* XL, int ld, int n, int tid) {
  constexpr int CW = DareMap<NW>::CW, RG = DareMap<NW>::RG;
  const int c = tid % CW, rg = tid / CW;
  if (c < n) for (int i = rg; i < n; i += RG) XL[i * ld + c] = 0.0f;
  lqr_sync();
  for (int j = 0; j + 1 < n; j++) {
    if (c < n) {
      const double xh = X[j * ld + c], xl = (double)XL[j * ld + c];
      for (int i = j + 1 + rg; i < n; i += RG) {
        double hi = X[i * ld + c], lo = (double)XL[i * ld + c];
        dare_dd_sub(hi, lo, W[i * ld + j], xh, xl);
        X[i * ld + c] = hi; XL[i * ld + c] = dare_lo(lo);
      }
    }
    lqr_sync();
  }
  if (rg == 0 && c < n) {
    double hi = X[(n - 1) * ld + c], lo = (double)XL[(n - 1) * ld + c];
    dare_dd_div(hi, lo, W[(n - 1) * ld + n - 1]);
    X[(n - 1) * ld + c] = hi; XL[(n - 1) * ld + c] = dare_lo(lo);
  }
  lqr_sync();
  for (int j = n - 1; j >= 1; j--) {
    if (c < n) {
      const double xh = X[j * ld + c], xl = (double)XL[j * ld + c];
      for (int i = j - 1 - rg; i >= 0; i -= RG) {
        double hi = X[i * ld + c], lo = (double)XL[i * ld + c];
        dare_dd_sub(hi, lo, W[i * ld + j], xh, xl);
        if (i == j - 1) dare_dd_div(hi, lo, W[i * ld + i]);
        X[i * ld + c] = hi; XL[i * ld + c] = dare_lo(lo);
      }
    }
    lqr_sync();
  }
}

// a problem that did not converge: zeros for X and K, what was reached for the rest
template <int NT>
MJB_LQR_DEV void dare_report(const DareArgs& p, int e, int tid, int status, int iters, double change) {
  const int nx = p.nx, nu = p.nu;
  for (int i = tid; i < nx * nx; i += NT) p.X[(long)e * nx * nx + i] = 0.0;
  for (int i = tid; i < nu * nx; i += NT) p.K[(long)e * nu * nx + i] = 0.0;
  if (tid == 0) {
    p.status[e] = status; p.iters[e] = iters;
    if (p.change) p.change[e] = dare_finite(change) ? change : __builtin_huge_val();
  }
}

// ---- problem e -----------------------------------------------------------------------------------------------------------------
// NW waves (64 NW threads, tid), nu <= MU (the unroll bound of the Cholesky substitutions), w: dare_layout(nx, nu).total doubles of LDS.
// Every decision that encloses a barrier (a bad pivot, convergence) is read by every thread from the same LDS words: workgroup-uniform.
template <int NW, int MU>
MJB_LQR_DEV void dare_env(const DareArgs& p, int e, int tid, double* w) {
  constexpr int NT = 64 * NW, CW = DareMap<NW>::CW, RG = DareMap<NW>::RG;
  const int nx = p.nx, nu = p.nu, c = tid % CW, rg = tid / CW;
  const DareLay l = dare_layout(nx, nu);
  const int ld = l.ld, lds = l.lds;
  double *S = w + l.S, *A = w + l.A, *perm = w + l.perm, *red = w + l.red, *W = w + l.W, *X = w + l.X;
  float* XL = (float*)(w + l.XL);
  double *Bm = w + l.Bm, *Z = w + l.Z, *XB = w + l.XB, *M = w + l.M, *Lf = w + l.L;
  const double* Ag = p.A.p + (long)e * p.A.es;
  const double* Bg = p.Bm.p + (long)e * p.Bm.es;
  const double* Qg = p.Q.p + (long)e * p.Q.es;
  const double* Rg = p.R.p + (long)e * p.R.es;
  auto H = [&](int i, int j) -> double& { return S[dare_h_index(i, j, lds)]; };
  auto G = [&](int i, int j) -> double& { return S[dare_g_index(i, j, lds)]; };
  const double inf = __builtin_huge_val();

  // G_0 = sym(B R^-1 B') through Z = R^-1 B' and the product B Z (parked in A's buffer), H_0 = Q
  for (int i = tid; i < nx * nu; i += NT) { Bm[i] = Bg[i]; Z[(i % nu) * nx + i / nu] = Bg[i]; }
  for (int i = tid; i < nu * nu; i += NT) M[i] = Rg[i];
  if (c < nx) for (int i = rg; i < nx; i += RG) if (c <= i) H(i, c) = Qg[i * nx + c];
  lqr_sync();
  if (!lqr_cholesky<NT>(M, Lf, nu, tid)) { dare_report<NT>(p, e, tid, 1, 0, inf); return; }
  for (int cc = tid; cc < nx; cc += NT) lqr_solve_column<MU>(Z, nx, Lf, nu, cc, [&](int i, double v) { Z[i * nx + cc] = -v; });
  lqr_sync();
  dare_gemm<NW, false>(nx, nx, nu, tid, [&](int k, int i) { return Bm[i * nu + k]; }, [&](int k, int j) { return Z[k * nx + j]; },
                       [](int, int) { return 0.0; }, [&](int r, int cc, double v) { A[r * ld + cc] = v; });
  lqr_sync();
  if (c < nx) for (int i = rg; i < nx; i += RG) if (i <= c) G(i, c) = 0.5 * (A[i * ld + c] + A[c * ld + i]);
  lqr_sync();
  if (c < nx) for (int i = rg; i < nx; i += RG) A[i * ld + c] = Ag[i * nx + c];
  lqr_sync();

  int iters = 0;
  double change = inf;
  for (;;) {
    // W = I + G H and its LU
    dare_gemm<NW, false>(nx, nx, nx, tid, [&](int k, int i) { return G(i, k); }, [&](int k, int j) { return H(k, j); },
                         [](int r, int cc) { return r == cc ? 1.0 : 0.0; }, [&](int r, int cc, double v) { W[r * ld + cc] = v; });
    lqr_sync();
    if (!dare_lu<NW>(W, ld, perm, nx, tid)) { dare_report<NT>(p, e, tid, 2, iters, change); return; }
    double dmax = 0.0, hmax = 0.0;                               // this thread's part of max|dH|, max|H|; dmax = inf at a value that is not finite

    // X = W^-1 G, X <- X A', then A X (parked in X): G += sym(A X_G A')
    if (c < nx) for (int i = rg; i < nx; i += RG) X[i * ld + c] = G((int)perm[i], c);
    lqr_sync();
    dare_lu_solve<NW>(W, X, XL, ld, nx, tid);
    dare_gemm<NW, true>(nx, nx, nx, tid, [&](int k, int i) { return X[i * ld + k]; }, [&](int k, int j) { return A[j * ld + k]; },
                        [](int, int) { return 0.0; }, [&](int r, int cc, double v) { X[r * ld + cc] = v; });
    lqr_sync();
    dare_gemm<NW, true>(nx, nx, nx, tid, [&](int k, int i) { return A[i * ld + k]; }, [&](int k, int j) { return X[k * ld + j]; },
                        [](int, int) { return 0.0; }, [&](int r, int cc, double v) { X[r * ld + cc] = v; });
    lqr_sync();
    if (c < nx)
      for (int i = rg; i < nx; i += RG)
        if (i <= c) {
          const double v = G(i, c) + 0.5 * (X[i * ld + c] + X[c * ld + i]);
          if (!dare_finite(v)) dmax = inf;
          G(i, c) = v;
        }
    lqr_sync();

    // X = W^-1 A, W <- H X, then A' W (parked in W): H += sym(A' H X_A); A <- A X
    if (c < nx) for (int i = rg; i < nx; i += RG) X[i * ld + c] = A[(int)perm[i] * ld + c];
    lqr_sync();
    dare_lu_solve<NW>(W, X, XL, ld, nx, tid);
    dare_gemm<NW, false>(nx, nx, nx, tid, [&](int k, int i) { return H(i, k); }, [&](int k, int j) { return X[k * ld + j]; },
                         [](int, int) { return 0.0; }, [&](int r, int cc, double v) { W[r * ld + cc] = v; });
    lqr_sync();
    dare_gemm<NW, true>(nx, nx, nx, tid, [&](int k, int i) { return A[k * ld + i]; }, [&](int k, int j) { return W[k * ld + j]; },
                        [](int, int) { return 0.0; }, [&](int r, int cc, double v) { W[r * ld + cc] = v; });
    lqr_sync();
    if (c < nx)
      for (int i = rg; i < nx; i += RG)
        if (c <= i) {
          const double h = H(i, c), v = h + 0.5 * (W[i * ld + c] + W[c * ld + i]), d = fabs(v - h);
          if (!dare_finite(v)) dmax = inf;
          if (d > dmax) dmax = d;
          if (fabs(v) > hmax) hmax = fabs(v);
          H(i, c) = v;
        }
    dare_gemm<NW, true>(nx, nx, nx, tid, [&](int k, int i) { return A[i * ld + k]; }, [&](int k, int j) { return X[k * ld + j]; },
                        [](int, int) { return 0.0; }, [&](int r, int cc, double v) { if (!dare_finite(v)) dmax = inf; A[r * ld + cc] = v; });
    red[2 * tid] = dmax; red[2 * tid + 1] = hmax;
    lqr_sync();
    double dall = 0.0, hall = 0.0;
    for (int t = 0; t < NT; t++) { if (red[2 * t] > dall) dall = red[2 * t]; if (red[2 * t + 1] > hall) hall = red[2 * t + 1]; }
    lqr_sync();                                                  // red is rewritten in the next iteration
    iters++;
    change = dall / hall;
    if (!dare_finite(dall) || !dare_finite(hall)) { dare_report<NT>(p, e, tid, 2, iters, inf); return; }
    if (change <= p.tol) break;
    if (iters == p.max_iter) { dare_report<NT>(p, e, tid, 3, iters, change); return; }
  }

  // K = (R + B' X B)^-1 B' X A with the A and B of the problem: XB = X B, M = R + B' XB, Z = XB' A
  for (int i = tid; i < nx * nu; i += NT) Bm[i] = Bg[i];
  if (c < nx) for (int i = rg; i < nx; i += RG) A[i * ld + c] = Ag[i * nx + c];
  lqr_sync();
  dare_gemm<NW, false>(nx, nu, nx, tid, [&](int k, int i) { return H(i, k); }, [&](int k, int j) { return Bm[k * nu + j]; },
                       [](int, int) { return 0.0; }, [&](int r, int cc, double v) { XB[r * nu + cc] = v; });
  lqr_sync();
  dare_gemm<NW, false>(nu, nu, nx, tid, [&](int k, int i) { return Bm[k * nu + i]; }, [&](int k, int j) { return XB[k * nu + j]; },
                       [&](int r, int cc) { return r >= cc ? Rg[r * nu + cc] : Rg[cc * nu + r]; }, [&](int r, int cc, double v) { M[r * nu + cc] = v; });
  dare_gemm<NW, false>(nu, nx, nx, tid, [&](int k, int i) { return XB[k * nu + i]; }, [&](int k, int j) { return A[k * ld + j]; },
                       [](int, int) { return 0.0; }, [&](int r, int cc, double v) { Z[r * nx + cc] = v; });
  lqr_sync();
  if (!lqr_cholesky<NT>(M, Lf, nu, tid)) { dare_report<NT>(p, e, tid, 1, iters, change); return; }
  double* Ko = p.K + (long)e * nu * nx;
  for (int cc = tid; cc < nx; cc += NT) lqr_solve_column<MU>(Z, nx, Lf, nu, cc, [&](int i, double v) { Ko[i * nx + cc] = -v; });
  double* Xo = p.X + (long)e * nx * nx;
  if (c < nx) for (int i = rg; i < nx; i += RG) Xo[i * nx + c] = H(i, c);
  if (tid == 0) { p.status[e] = 0; p.iters[e] = iters; if (p.change) p.change[e] = change; }
}

#ifndef MJB_HOST_EMU
// enqueue only (mjb_dare.hip); the entry point (mjb_api.hip) has checked every pointer and extent
hipError_t dare_launch(const DareArgs& p, hipStream_t stream);
#endif

}  // namespace mjb
