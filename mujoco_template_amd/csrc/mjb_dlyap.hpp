// mjb_dlyap.hpp — the infinite-horizon quadratic cost of running a gain on a system (mjb_lqr_dlyap): the solution P of the discrete
// Lyapunov equation
//   P = M' P M + S,      M = A + s B K,      S = sym(Q + K' R K)
// and J = x0' P x0, for a batch of systems, as workgroup-cooperative float64 device code.  For the optimal gain P is the X of
// mjb_lqr_dare, the P the reference's _solve_lqr_gains hands back beside K (reference examples/drone/controllers/lqr.py:350-360); for
// any other gain (a nominal one on a randomised model, a hand-tuned one) it is what scipy.linalg.solve_discrete_lyapunov gives on the
// host, one system at a time.  The closed loop is the one whose spectral radius the reference checks (examples/drone/controllers/lqr.py:133-137).
//
// Squared Smith (doubling) iteration: iterate k holds 2^k steps of the cost sum.
//   M = A + s B K (s K staged: the sign is an exact negation; no B, K: M = A),  S = sym(Q + K' (R K)) (no R or no K: sym(Q))
//   an entry of M or S that is not finite: status 1
//   P_0 = S, M_0 = M;  repeat:
//     T = M_k' (P_k M_k)            (transpose: T = M_k (P_k M_k'), the Gramian form P = M P M' + S)
//     P_{k+1} = sym(P_k + T),  M_{k+1} = M_k M_k
//     change = max|P_{k+1} - P_k| / max|P_{k+1}| (0 / 0 = 0);  iters += 1
//     an iterate that is not finite: status 2 (rho > 1 ends this way);  the FIRST change <= tol: status 0;  iters == max_iter: status 3
//   P = P_k (bitwise symmetric),  J = x0' P x0: y = P x0 row by row, then sum_i x0_i y_i in index order.
// The stop is on change alone and at its first crossing, never on stagnation: with marginal modes that S does not see, change
// collapses, then doubles every iteration as M^(2^k) drifts.  Q and R are taken as symmetric: only their LOWER triangles are read.
// A failed problem has NaN in P and +inf in J (J < bound is false for it), and touches no other problem.
//
// One workgroup per problem, lqr_waves(nx) waves, P, M and the product temporary resident in LDS with the odd row stride nx | 1 (a
// product may read either operand down its rows or along them without a bank conflict, so the transpose form costs no copy), every
// nx x nx product on v_mfma_f64_16x16x4_f64 in the tile loop of dare_gemm.  P M and M M run in ONE pass over k (eight independent
// accumulator chains per wave), M M waiting in registers until the second product has read M: five barriers per iteration.
// The same source compiles in the host emulation of mjb_lqr.hpp (MJB_HOST_EMU), which only the CPU test-suite uses.
#pragma once
#include "mjb_dare.hpp"

namespace mjb {

static const int kDlyapMaxIter = 64;

struct DlyapArgs {
  int B, nx, nu, transpose, max_iter;               // nu = 0: no B K term (Bm.p, K.p, R.p unused)
  double sign, tol;                                 // sign: -1.0 or +1.0
  LqrStrided A, Bm, K, Q, R, x0;                    // per problem e: p + e * es (ss unused); R.p, x0.p may be null
  double *P, *J, *change;                           // [B, nx, nx], [B] (null exactly when x0.p is), [B] (may be null)
  int *iters, *status;                              // [B]
};

// ---- LDS layout (offsets in doubles) --------------------------------------------------------------------------------------------
// M, W (the product temporary; S before it is symmetrised), P: nx x nx with row stride ld = nx | 1.  red: two partial maxima per
// thread (later the terms of J), red2: those of the 16 groups of threads.  Ks [nu, nx], the staged s K, and RK [nu, nx] = R Ks are
// dead once M and W are formed and lie under P.
struct DlyapLay { int M, W, red, red2, P, Ks, RK, ld, total; };
MJB_LQR_HD DlyapLay dlyap_layout(int nx, int nu) {
  DlyapLay l;
  l.ld = nx | 1;
  const int nt = 64 * lqr_waves(nx);
  int o = 0;
  l.M = o; o += nx * l.ld;
  l.W = o; o += nx * l.ld;
  l.red = o; o += 2 * nt;
  l.red2 = o; o += 32;
  const int u0 = o;
  l.P = o; o += nx * l.ld;
  const int end1 = o;
  o = u0;
  l.Ks = o; o += nu * nx;
  l.RK = o; o += nu * nx;
  l.total = o > end1 ? o : end1;
  return l;
}

// 0 ok; otherwise which limit is broken (the entry point turns it into the message).  has_bk: the B K term is present
inline int dlyap_size_error(long B, long nx, long nu, int has_bk, long max_iter, double tol, long feedback_sign) {
  if (B < 1) return 1;
  if (nx < 1 || nx > kLqrMaxNx) return 2;
  if (has_bk && (nu < 1 || nu > kLqrMaxNu)) return 3;
  if (max_iter < 1 || max_iter > kDlyapMaxIter) return 4;
  if (!(tol >= 0.0)) return 5;
  if (feedback_sign != 1 && feedback_sign != -1) return 6;
  if ((__int128)B * nx * nx > ((__int128)1 << 40)) return 7;
  return 0;
}

// Two independent products of the same shape in one pass over k, C1 [n, n] = sum_k la1(k, i) lb1(k, j) stored at once and
// C2 = sum_k la2(k, i) lb2(k, j) left in the accumulators acc2 (dlyap_store writes them): the tile loop and fragment maps of
// dare_gemm, every tile with the operation order it has there.  Eight independent MFMA chains per wave instead of four hide the
// latency of the LDS reads, and C2 may overwrite an operand once every reader is past a later barrier.
template <int NW, class LA1, class LB1, class LA2, class LB2, class Store>
MJB_LQR_DEV void dlyap_gemm_pair(int n, int tid, LA1 la1, LB1 lb1, LA2 la2, LB2 lb2, Store store1, lqr_d4 (&acc2)[4]) {
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int nt = (n + 15) >> 4, ntile = nt * nt;
  lqr_d4 acc1[4];
  int ti[4], tj[4];
  bool on[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int q = wave + NW * s;
    on[s] = q < ntile;
    ti[s] = 16 * (q / nt); tj[s] = 16 * (q % nt);
#pragma unroll
    for (int r = 0; r < 4; r++) { acc1[s][r] = 0.0; acc2[s][r] = 0.0; }
  }
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int k = k0 + lk;
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if (!on[s]) continue;                                      // wave-uniform
      const int i = ti[s] + li, j = tj[s] + li;
      const bool ia = k < n && i < n, ja = k < n && j < n;
      const double a1 = ia ? la1(k, i) : 0.0, b1 = ja ? lb1(k, j) : 0.0, a2 = ia ? la2(k, i) : 0.0, b2 = ja ? lb2(k, j) : 0.0;
      acc1[s] = MJB_MFMA_F64(a1, b1, acc1[s]);
      acc2[s] = MJB_MFMA_F64(a2, b2, acc2[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < 4; s++) {
    if (!on[s]) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = ti[s] + lk + 4 * r, col = tj[s] + li;
      if (row < n && col < n) store1(row, col, acc1[s][r]);
    }
  }
}
template <int NW, class Store>
MJB_LQR_DEV void dlyap_store(int n, int tid, const lqr_d4 (&acc)[4], Store store) {
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int nt = (n + 15) >> 4, ntile = nt * nt;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int q = wave + NW * s;
    if (q >= ntile) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * (q / nt) + lk + 4 * r, col = 16 * (q % nt) + li;
      if (row < n && col < n) store(row, col, acc[s][r]);
    }
  }
}

// The maxima of the (a, b) pairs every thread gives, the same in every thread: through red (one pair per thread), then red2 (one pair
// per group of NT / 16 threads) - 16 + NT / 16 dependent LDS reads instead of NT.  A maximum does not depend on the order: the result
// is that of any other reduction.  The caller keeps a barrier between two calls.
template <int NT>
MJB_LQR_DEV void dlyap_max2(double* red, double* red2, int tid, double& a, double& b) {
  constexpr int G = NT / 16;
  red[2 * tid] = a; red[2 * tid + 1] = b;
  lqr_sync();
  if (tid < 16) {
    double x = 0.0, y = 0.0;
    for (int t = tid * G; t < (tid + 1) * G; t++) { if (red[2 * t] > x) x = red[2 * t]; if (red[2 * t + 1] > y) y = red[2 * t + 1]; }
    red2[2 * tid] = x; red2[2 * tid + 1] = y;
  }
  lqr_sync();
  a = 0.0; b = 0.0;
  for (int t = 0; t < 16; t++) { if (red2[2 * t] > a) a = red2[2 * t]; if (red2[2 * t + 1] > b) b = red2[2 * t + 1]; }
}

// a failed problem: NaN for P, +inf for J, what was reached for the rest
template <int NT>
MJB_LQR_DEV void dlyap_report(const DlyapArgs& p, int e, int tid, int status, int iters, double change) {
  const int nx = p.nx;
  for (int i = tid; i < nx * nx; i += NT) p.P[(long)e * nx * nx + i] = __builtin_nan("");
  if (tid == 0) {
    if (p.J) p.J[e] = __builtin_huge_val();
    p.status[e] = status; p.iters[e] = iters;
    if (p.change) p.change[e] = dare_finite(change) ? change : __builtin_huge_val();
  }
}

// ---- problem e -----------------------------------------------------------------------------------------------------------------
// NW waves (64 NW threads, tid), w: dlyap_layout(nx, nu).total doubles of LDS.  Every decision that encloses a barrier (a value that
// is not finite, convergence) is read by every thread from the same LDS words: workgroup-uniform.
template <int NW>
MJB_LQR_DEV void dlyap_env(const DlyapArgs& p, int e, int tid, double* w) {
  constexpr int NT = 64 * NW, CW = DareMap<NW>::CW, RG = DareMap<NW>::RG;
  const int nx = p.nx, nu = p.nu, c = tid % CW, rg = tid / CW;
  const DlyapLay l = dlyap_layout(nx, nu);
  const int ld = l.ld;
  double *M = w + l.M, *W = w + l.W, *red = w + l.red, *red2 = w + l.red2, *P = w + l.P, *Ks = w + l.Ks, *RK = w + l.RK;
  const double* Ag = p.A.p + (long)e * p.A.es;
  const double* Qg = p.Q.p + (long)e * p.Q.es;
  const double inf = __builtin_huge_val();
  auto Qs = [&](int r, int cc) { return r >= cc ? Qg[r * nx + cc] : Qg[cc * nx + r]; };

  // M = A + s B K into M, Q + K' (R K) into W
  if (nu > 0) {
    const double* Bg = p.Bm.p + (long)e * p.Bm.es;
    const double* Kg = p.K.p + (long)e * p.K.es;
    const double sg = p.sign;
    for (int i = tid; i < nu * nx; i += NT) Ks[i] = sg * Kg[i];
    lqr_sync();
    dare_gemm<NW, false>(nx, nx, nu, tid, [&](int k, int i) { return Bg[i * nu + k]; }, [&](int k, int j) { return Ks[k * nx + j]; },
                         [&](int r, int cc) { return Ag[r * nx + cc]; }, [&](int r, int cc, double v) { M[r * ld + cc] = v; });
    if (p.R.p) {
      const double* Rg = p.R.p + (long)e * p.R.es;
      dare_gemm<NW, false>(nu, nx, nu, tid, [&](int k, int i) { return i >= k ? Rg[i * nu + k] : Rg[k * nu + i]; },
                           [&](int k, int j) { return Ks[k * nx + j]; }, [](int, int) { return 0.0; },
                           [&](int r, int cc, double v) { RK[r * nx + cc] = v; });
      lqr_sync();
      dare_gemm<NW, false>(nx, nx, nu, tid, [&](int k, int i) { return Ks[k * nx + i]; }, [&](int k, int j) { return RK[k * nx + j]; },
                           Qs, [&](int r, int cc, double v) { W[r * ld + cc] = v; });
    } else {
      if (c < nx) for (int i = rg; i < nx; i += RG) W[i * ld + c] = Qs(i, c);
    }
  } else {
    if (c < nx) for (int i = rg; i < nx; i += RG) { M[i * ld + c] = Ag[i * nx + c]; W[i * ld + c] = Qs(i, c); }
  }
  lqr_sync();                                                    // Ks and RK are dead from here on: P lies over them
  {
    double bad = 0.0, none = 0.0;
    if (c < nx)
      for (int i = rg; i < nx; i += RG) {
        const double s = 0.5 * (W[i * ld + c] + W[c * ld + i]);
        if (!dare_finite(s) || !dare_finite(M[i * ld + c])) bad = 1.0;
        P[i * ld + c] = s;
      }
    dlyap_max2<NT>(red, red2, tid, bad, none);
    if (bad != 0.0) { dlyap_report<NT>(p, e, tid, 1, 0, inf); return; }
  }

  // entry (k, i) of M read as the left factor M' or the right factor M is M[k * sk + i * si]; the transpose form swaps the strides
  const int sk = p.transpose ? 1 : ld, si = p.transpose ? ld : 1;
  int iters = 0;
  double change = inf;
  for (;;) {
    // W = P M (P M') and, left in registers, M M;  then W <- M' W (M W): the second product overwrites its own right operand behind
    // its barrier, behind which nobody reads M any more either, so M M goes into M
    lqr_d4 mm[4];
    dlyap_gemm_pair<NW>(nx, tid, [&](int k, int i) { return P[i * ld + k]; }, [&](int k, int j) { return M[k * sk + j * si]; },
                        [&](int k, int i) { return M[i * ld + k]; }, [&](int k, int j) { return M[k * ld + j]; },
                        [&](int r, int cc, double v) { W[r * ld + cc] = v; }, mm);
    lqr_sync();
    dare_gemm<NW, true>(nx, nx, nx, tid, [&](int k, int i) { return M[k * sk + i * si]; }, [&](int k, int j) { return W[k * ld + j]; },
                        [](int, int) { return 0.0; }, [&](int r, int cc, double v) { W[r * ld + cc] = v; });
    double dmax = 0.0, hmax = 0.0;                               // this thread's part of max|dP|, max|P|; dmax = inf at a value that is not finite
    dlyap_store<NW>(nx, tid, mm, [&](int r, int cc, double v) { if (!dare_finite(v)) dmax = inf; M[r * ld + cc] = v; });
    lqr_sync();
    if (c < nx)
      for (int i = rg; i < nx; i += RG)
        if (c <= i) {                                            // the lower triangle decides, both halves are written: bitwise symmetric
          const double h = P[i * ld + c], v = h + 0.5 * (W[i * ld + c] + W[c * ld + i]), d = fabs(v - h);
          if (!dare_finite(v)) dmax = inf;
          if (d > dmax) dmax = d;
          if (fabs(v) > hmax) hmax = fabs(v);
          P[i * ld + c] = v; P[c * ld + i] = v;
        }
    dlyap_max2<NT>(red, red2, tid, dmax, hmax);                  // its first barrier also ends the iteration's writes of P and M
    iters++;
    if (!dare_finite(dmax) || !dare_finite(hmax)) { dlyap_report<NT>(p, e, tid, 2, iters, inf); return; }
    change = (dmax == 0.0 && hmax == 0.0) ? 0.0 : dmax / hmax;
    if (change <= p.tol) break;
    if (iters == p.max_iter) { dlyap_report<NT>(p, e, tid, 3, iters, change); return; }
  }

  double* Po = p.P + (long)e * nx * nx;
  if (c < nx) for (int i = rg; i < nx; i += RG) Po[i * nx + c] = P[i * ld + c];
  if (p.x0.p) {                                                  // J = sum_i x0_i (P x0)_i: one row per thread, then thread 0 in index order
    const double* xg = p.x0.p + (long)e * p.x0.es;
    if (tid < nx) {
      double y = 0.0;
      for (int j = 0; j < nx; j++) y = fma(P[tid * ld + j], xg[j], y);
      red[tid] = xg[tid] * y;
    }
    lqr_sync();
    if (tid == 0) {
      double s = 0.0;
      for (int i = 0; i < nx; i++) s += red[i];
      p.J[e] = s;
    }
  }
  if (tid == 0) { p.status[e] = 0; p.iters[e] = iters; if (p.change) p.change[e] = change; }
}

#ifndef MJB_HOST_EMU
// enqueue only (mjb_dlyap.hip); the entry point (mjb_api.hip) has checked every pointer and extent
hipError_t dlyap_launch(const DlyapArgs& p, hipStream_t stream);
#endif

}  // namespace mjb
