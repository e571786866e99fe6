// mjb_eig.hpp — the poles of a batch of (closed-loop) systems (mjb_lqr_eig): every eigenvalue of M = A + s B K (s = -1 or +1; or of A
// alone) and the spectral radius rho = max |lambda|, as wavefront-cooperative float64 device code.  It is what the reference computes on
// the host right after every design, np.max(np.abs(np.linalg.eigvals(A - B @ K))), to refuse or rescale a gain whose closed loop is not
// inside the unit circle (reference examples/drone/controllers/lqr.py:134-137, examples/drone2/main.py:317-318).
//
// The method is LAPACK's for eigenvalues only (dgebal 'S', dgehd2, dlahqr with wantt = wantz = false, dlanv2), per problem:
//   1. M = A + s B K on v_mfma_f64_16x16x4_f64 (dare_gemm: the operands are accessors).  K is staged in LDS with the sign applied (an
//      exact negation: s = +1 with -K is bitwise s = -1 with K); B and A are read in place, band after band of 16 rows (one wave holds
//      four 16 x 16 tiles: the product LOOPS over the row bands).  An entry of M that is not finite ends the problem with status 1.
//   2. Balancing (optional): Parlett-Reinsch scaling alone, no permutation, radix 2 (exact), the loop of dgebal on the 1-norms of the
//      off-diagonal row and column parts with its 0.95 acceptance factor; rows in index order until a full pass changes nothing; a zero
//      row or column norm leaves that index alone.  scale = D, the iterate is D^-1 M D.
//   3. Householder reduction to upper Hessenberg form, one lane per column (left update) and per row (right update); a reflector whose
//      tail is zero is the identity and is skipped: no division by zero on a zero, diagonal, triangular or Hessenberg matrix.
//   4. Francis implicit double-shift QR on the active block only: dlahqr's two-stage small-subdiagonal test, its search for two
//      consecutive small subdiagonals, exceptional shifts at every 10th (from the top of the block) and 20th (from its bottom) sweep
//      since the last deflation, 2 x 2 blocks standardised as dlanv2 does (a pair comes out as exact conjugates).  `max_sweeps` caps the
//      TOTAL number of sweeps (LAPACK's 30 max(10, nx) by default): reaching it is status 2.
//   5. Rank sort, one lane per eigenvalue: descending modulus, ties by descending real part, then descending imaginary part (so the
//      member of a pair with the positive imaginary part comes first).  The modulus is eig_hypot, a correctly rounded hypot from
//      IEEE operations alone (the same bits on the GPU and in the host emulation); rho is the modulus of the first.
// A failed problem has NaN in wr, wi and +inf in rho (rho < 1 is false for it), and touches no other problem.
//
// Mapping: ONE wavefront per problem for every stage, the iterate resident in LDS with the odd row stride nx | 1 (a lane per row and a
// lane per column are both conflict-free).  The bulge chase is serial in its position: a 3 x 3 reflector touches at most 64 columns,
// then at most 64 rows, so one wave covers each half in one pass and more waves would only add workgroup barriers to a chain of ~2 nx
// dependent steps per sweep; with 64 threads the barrier between the halves is wave-scope (no s_barrier is emitted for a workgroup of
// one wave).  The two searches of a sweep (the negligible subdiagonal entry, the two consecutive small ones) test one position per lane
// and agree through one flag word per lane in LDS (the highest flagged position wins, as in the serial loops); the other scalar
// decisions (shifts, reflectors, 2 x 2 blocks) are computed redundantly by every lane from broadcast LDS reads, so they are uniform
// without any reduction.  Occupancy comes from the batch: under 1 KB of LDS for a cart-pole, 49 KB at (64, 32).
// The kernel takes 92 VGPRs and no scratch; the measured times are in INTEGRATION.md.
// The same source compiles in the host emulation of mjb_lqr.hpp (MJB_HOST_EMU), which only the CPU test-suite uses.
#pragma once
#include "mjb_dare.hpp"

namespace mjb {

struct EigArgs {
  int B, nx, nu, max_sweeps, balance;               // nu = 0: no B K term (Bm.p, K.p unused)
  double sign;                                      // -1.0 or +1.0
  LqrStrided A, Bm, K;                              // per problem e: p + e * es (ss unused)
  double *wr, *wi, *scale, *rho;                    // [B, nx] x 3, [B]
  int *sweeps, *status;                             // [B]
};

MJB_LQR_HD int eig_default_sweeps(int nx) { return 30 * (nx > 10 ? nx : 10); }

// ---- LDS layout (offsets in doubles) --------------------------------------------------------------------------------------------
// H: the iterate, row stride ld = nx | 1.  sc: the balancing diagonal.  After M is formed: wr, wi (the eigenvalues as they deflate),
// v (the Householder vector; the moduli during the sort), red (one word per lane).  Ks [nu, nx], the staged s K, is dead once M is
// formed and lies under them.
struct EigLay { int H, sc, wr, wi, v, red, Ks, ld, total; };
MJB_LQR_HD EigLay eig_layout(int nx, int nu) {
  EigLay l;
  l.ld = nx | 1;
  int o = 0;
  l.H = o; o += nx * l.ld;
  l.sc = o; o += nx;
  const int u0 = o;
  l.wr = o; o += nx;
  l.wi = o; o += nx;
  l.v = o; o += nx;
  l.red = o; o += 64;
  const int end1 = o;
  o = u0;
  l.Ks = o; o += nu * nx;
  l.total = o > end1 ? o : end1;
  return l;
}

// 0 ok; otherwise which limit is broken (the entry point turns it into the message).  has_bk: the B K term is present;
// max_sweeps 0 = the default
inline int eig_size_error(long B, long nx, long nu, int has_bk, long max_sweeps, long feedback_sign) {
  if (B < 1) return 1;
  if (nx < 1 || nx > kLqrMaxNx) return 2;
  if (has_bk && (nu < 1 || nu > kLqrMaxNu)) return 3;
  if (max_sweeps < 0 || max_sweeps > eig_default_sweeps((int)nx)) return 4;
  if (feedback_sign != 1 && feedback_sign != -1) return 5;
  if ((__int128)B * nx * nx > ((__int128)1 << 40)) return 6;
  return 0;
}

// sqrt(x^2 + y^2) correctly rounded from IEEE operations alone: the square root of the rounded sum, then one correction by the exactly
// evaluated residual h^2 - x^2 - y^2 (every product is a statement of its own: nothing for the compiler to contract)
MJB_LQR_DEV double eig_hypot(double x, double y) {
  double ax = fabs(x), ay = fabs(y);
  if (ax < ay) { const double t = ax; ax = ay; ay = t; }
  if (ay <= ax * 0x1p-30 || !dare_finite(ax)) return ax;         // (y / x)^2 / 2 < 2^-60: x is the rounded result
  double back = 1.0;
  if (ax > 0x1p500) { ax *= 0x1p-600; ay *= 0x1p-600; back = 0x1p600; }
  else if (ax < 0x1p-500) { ax *= 0x1p600; ay *= 0x1p600; back = 0x1p-600; }
  const double ay2 = ay * ay;
  double h = sqrt(fma(ax, ax, ay2));
  const double h2 = h * h;
  const double ax2 = ax * ax;
  const double d = h2 - ax2;
  const double r0 = fma(-ay, ay, d);
  const double r1 = fma(h, h, -h2);
  const double r2 = fma(ax, ax, -ax2);
  const double r = (r0 + r1) - r2;
  const double c = r / (2.0 * h);
  h = h - c;
  return h * back;
}

// dlapy2 for finite arguments
MJB_LQR_DEV double eig_lapy2(double x, double y) {
  const double ax = fabs(x), ay = fabs(y), w = ax > ay ? ax : ay, z = ax > ay ? ay : ax;
  if (z == 0.0) return w;
  const double q = z / w;
  return w * sqrt(1.0 + q * q);
}

// dlarfg for a vector of nr = 2 or 3 entries (v0; v1, v2): v0 <- beta, (v1, v2) <- the tail of the reflector, returns tau (0: identity)
MJB_LQR_DEV double eig_larfg(int nr, double& v0, double& v1, double& v2) {
  if (nr < 3) v2 = 0.0;
  double xnorm = eig_lapy2(v1, v2);
  if (xnorm == 0.0) return 0.0;
  const double safmin = 2.2250738585072014e-308 / 1.1102230246251565e-16, rsafmn = 1.0 / safmin;
  double alpha = v0, beta = -copysign(eig_lapy2(alpha, xnorm), alpha);
  int knt = 0;
  if (fabs(beta) < safmin) {
    do { knt++; v1 *= rsafmn; v2 *= rsafmn; beta *= rsafmn; alpha *= rsafmn; } while (fabs(beta) < safmin && knt < 20);
    xnorm = eig_lapy2(v1, v2);
    beta = -copysign(eig_lapy2(alpha, xnorm), alpha);
  }
  const double tau = (beta - alpha) / beta, s = 1.0 / (alpha - beta);
  v1 *= s; v2 *= s;
  for (int j = 0; j < knt; j++) beta *= safmin;
  v0 = beta;
  return tau;
}

// dlanv2 for the eigenvalues alone: those of [a b; c d], a complex pair as (re, +im), (re, -im) with one re
MJB_LQR_DEV void eig_lanv2(double a, double b, double c, double d, double& rt1r, double& rt1i, double& rt2r, double& rt2i) {
  const double eps = 2.220446049250313e-16, multpl = 4.0;
  auto sgn = [](double x) { return copysign(1.0, x); };
  if (c == 0.0) {
  } else if (b == 0.0) {
    const double t = d; d = a; a = t; b = -c; c = 0.0;
  } else if ((a - d) == 0.0 && sgn(b) != sgn(c)) {
  } else {
    const double temp = a - d;
    double p = 0.5 * temp;
    const double bcmax = fabs(b) > fabs(c) ? fabs(b) : fabs(c);
    const double bcmis = (fabs(b) > fabs(c) ? fabs(c) : fabs(b)) * sgn(b) * sgn(c);
    const double scale = fabs(p) > bcmax ? fabs(p) : bcmax;
    double z = (p / scale) * p + (bcmax / scale) * bcmis;
    if (z >= multpl * eps) {                                      // real eigenvalues
      z = p + copysign(sqrt(scale) * sqrt(z), p);
      a = d + z;
      d = d - (bcmax / z) * bcmis;
      b = b - c; c = 0.0;
    } else {                                                      // complex, or real and (almost) equal: make the diagonal equal
      const double sigma = b + c, tau = eig_lapy2(sigma, temp);
      const double cs = sqrt(0.5 * (1.0 + fabs(sigma) / tau)), sn = -(p / (tau * cs)) * sgn(sigma);
      const double aa = a * cs + b * sn, bb = -a * sn + b * cs, cc = c * cs + d * sn, dd = -c * sn + d * cs;
      a = aa * cs + cc * sn; b = bb * cs + dd * sn; c = -aa * sn + cc * cs; d = -bb * sn + dd * cs;
      const double mid = 0.5 * (a + d);
      a = mid; d = mid;
      if (c != 0.0) {
        if (b != 0.0) {
          if (sgn(b) == sgn(c)) {                                 // real: reduce to upper triangular form
            p = copysign(sqrt(fabs(b)) * sqrt(fabs(c)), c);
            a = mid + p; d = mid - p;
            b = b - c; c = 0.0;
          }
        } else { b = -c; c = 0.0; }
      }
    }
  }
  rt1r = a; rt2r = d;
  if (c == 0.0) { rt1i = 0.0; rt2i = 0.0; }
  else { rt1i = sqrt(fabs(b)) * sqrt(fabs(c)); rt2i = -rt1i; }
}

// the highest index flagged: flag[t] != 0 stands for index top - t, t < count; `none` when no flag is set.  Every lane reads every flag.
MJB_LQR_DEV int eig_first(const double* flag, int count, int top, int none) {
  int first = count;
  for (int t = count - 1; t >= 0; t--) if (flag[t] != 0.0) first = t;
  return first < count ? top - first : none;
}

// a failed problem: NaN eigenvalues, rho = +inf, the scaling reached (sc; null = ones)
MJB_LQR_DEV void eig_report(const EigArgs& p, int e, int tid, int status, int sweeps, const double* sc) {
  const int n = p.nx;
  if (tid < n) {
    p.wr[(long)e * n + tid] = __builtin_nan("");
    p.wi[(long)e * n + tid] = __builtin_nan("");
    p.scale[(long)e * n + tid] = sc ? sc[tid] : 1.0;
  }
  if (tid == 0) { p.rho[e] = __builtin_huge_val(); p.status[e] = status; p.sweeps[e] = sweeps; }
}

// ---- problem e -----------------------------------------------------------------------------------------------------------------
// One wave (64 threads, tid), w: eig_layout(nx, nu).total doubles of LDS.  Every decision that encloses a barrier is computed by every
// thread from the same LDS words, read between two barriers in which nobody writes them: uniform.
MJB_LQR_DEV void eig_env(const EigArgs& p, int e, int tid, double* w) {
  const int n = p.nx, nu = p.nu;
  const EigLay l = eig_layout(n, nu);
  const int ld = l.ld;
  double *H = w + l.H, *sc = w + l.sc, *wr = w + l.wr, *wi = w + l.wi, *v = w + l.v, *red = w + l.red, *Ks = w + l.Ks;
  auto h = [&](int i, int j) -> double& { return H[i * ld + j]; };
  const double* Ag = p.A.p + (long)e * p.A.es;

  // 1. M = A + s B K
  if (nu > 0) {
    const double* Bg = p.Bm.p + (long)e * p.Bm.es;
    const double* Kg = p.K.p + (long)e * p.K.es;
    const double sg = p.sign;
    for (int i = tid; i < nu * n; i += 64) Ks[i] = sg * Kg[i];
    lqr_sync();
    for (int i0 = 0; i0 < n; i0 += 16) {
      const int mb = n - i0 < 16 ? n - i0 : 16;
      dare_gemm<1, false>(mb, n, nu, tid, [&](int k, int i) { return Bg[(i0 + i) * nu + k]; }, [&](int k, int j) { return Ks[k * n + j]; },
                          [&](int r, int c) { return Ag[(i0 + r) * n + c]; }, [&](int r, int c, double x) { h(i0 + r, c) = x; });
    }
  } else {
    for (int i = tid; i < n * n; i += 64) h(i / n, i % n) = Ag[i];
  }
  lqr_sync();                                                    // Ks is dead from here on
  {
    double bad = 0.0;
    if (tid < n) for (int i = 0; i < n; i++) if (!dare_finite(h(i, tid))) bad = 1.0;
    red[tid] = bad;
    if (tid < n) sc[tid] = 1.0;
    lqr_sync();
    double any = 0.0;
    for (int t = 0; t < 64; t++) any += red[t];
    if (any != 0.0) { eig_report(p, e, tid, 1, 0, nullptr); return; }
  }

  // 2. balancing: D^-1 M D, D powers of two
  if (p.balance) {
    const double sfmin1 = 2.2250738585072014e-308 / 2.220446049250313e-16, sfmax1 = 1.0 / sfmin1, sfmin2 = sfmin1 * 2.0, sfmax2 = 1.0 / sfmin2;
    for (int pass = 0; pass < 128; pass++) {                      // the cap is never reached by a convergent scaling; it bounds the time
      bool changed = false;
      for (int i = 0; i < n; i++) {
        double c = 0.0, r = 0.0;
        for (int j = 0; j < n; j++) if (j != i) { c += fabs(h(j, i)); r += fabs(h(i, j)); }
        if (c == 0.0 || r == 0.0) continue;
        double g = r * 0.5, f = 1.0;
        const double s = c + r;
        for (int it = 0; it < 1100 && c < g && (f > c ? f : c) < sfmax2 && (r < g ? r : g) > sfmin2; it++) { f *= 2.0; c *= 2.0; r *= 0.5; g *= 0.5; }
        g = c * 0.5;
        for (int it = 0; it < 1100 && g >= r && r < sfmax2 && (f < g ? f : g) > sfmin2; it++) { f *= 0.5; c *= 0.5; g *= 0.5; r *= 2.0; }
        if (c + r >= 0.95 * s) continue;
        const double si = sc[i];
        if (f < 1.0 && si < 1.0 && f * si <= sfmin1) continue;
        if (f > 1.0 && si > 1.0 && si >= sfmax1 / f) continue;
        lqr_sync();                                              // everybody has read row and column i (and sc[i])
        const double gi = 1.0 / f;
        if (tid < n && tid != i) { h(i, tid) *= gi; h(tid, i) *= f; }
        if (tid == 0) sc[i] = si * f;
        changed = true;
        lqr_sync();
      }
      if (!changed) break;
    }
  }

  // 3. Householder reduction to upper Hessenberg form
  for (int k = 0; k + 2 < n; k++) {
    double xmax = 0.0;
    for (int i = k + 2; i < n; i++) { const double a = fabs(h(i, k)); if (a > xmax) xmax = a; }
    if (xmax == 0.0) continue;                                   // the identity: nothing is written, no barrier is needed
    double ssq = 0.0;
    for (int i = k + 2; i < n; i++) { const double q = h(i, k) / xmax; ssq += q * q; }
    const double xnorm = xmax * sqrt(ssq), alpha = h(k + 1, k), beta = -copysign(eig_lapy2(alpha, xnorm), alpha);
    const double tau = (beta - alpha) / beta, s = 1.0 / (alpha - beta);
    if (tid < n) v[tid] = tid <= k ? 0.0 : tid == k + 1 ? 1.0 : h(tid, k) * s;
    lqr_sync();
    if (tid > k && tid < n) {
      h(tid, k) = tid == k + 1 ? beta : 0.0;
      double t = 0.0;                                            // column tid: (I - tau v v') H
      for (int i = k + 1; i < n; i++) t += v[i] * h(i, tid);
      t *= tau;
      int i = k + 1;
      for (; i + 3 < n; i += 4) {                                // four entries in flight: the loads before the stores
        const double a0 = h(i, tid), a1 = h(i + 1, tid), a2 = h(i + 2, tid), a3 = h(i + 3, tid), u0 = v[i], u1 = v[i + 1], u2 = v[i + 2], u3 = v[i + 3];
        h(i, tid) = a0 - u0 * t; h(i + 1, tid) = a1 - u1 * t; h(i + 2, tid) = a2 - u2 * t; h(i + 3, tid) = a3 - u3 * t;
      }
      for (; i < n; i++) h(i, tid) -= v[i] * t;
    }
    lqr_sync();
    if (tid < n) {
      double t = 0.0;                                            // row tid: H (I - tau v v')
      for (int j = k + 1; j < n; j++) t += h(tid, j) * v[j];
      t *= tau;
      int j = k + 1;
      for (; j + 3 < n; j += 4) {
        const double a0 = h(tid, j), a1 = h(tid, j + 1), a2 = h(tid, j + 2), a3 = h(tid, j + 3), u0 = v[j], u1 = v[j + 1], u2 = v[j + 2], u3 = v[j + 3];
        h(tid, j) = a0 - t * u0; h(tid, j + 1) = a1 - t * u1; h(tid, j + 2) = a2 - t * u2; h(tid, j + 3) = a3 - t * u3;
      }
      for (; j < n; j++) h(tid, j) -= t * v[j];
    }
    lqr_sync();
  }

  // 4. Francis double-shift QR on the active block H[l..i, l..i], deflating from the bottom
  const double safmin = 2.2250738585072014e-308, ulp = 2.220446049250313e-16, smlnum = safmin * ((double)n / ulp);
  const int cap = p.max_sweeps > 0 ? p.max_sweeps : eig_default_sweeps(n);
  int sweeps = 0, status = 0, i = n - 1;
  while (i >= 0) {
    int l = 0, its = 0;
    for (;;) {
      lqr_sync();                                                // the last sweep's writes are visible
      {                                                          // a negligible subdiagonal entry: lane t tests k = i - t, the highest k wins
        const int k = i - tid;
        double hit = 0.0;
        if (k > l) {
          const double sub = fabs(h(k, k - 1));
          if (sub <= smlnum) hit = 1.0;
          else {
            double tst = fabs(h(k - 1, k - 1)) + fabs(h(k, k));
            if (tst == 0.0) {
              if (k - 2 >= 0) tst += fabs(h(k - 1, k - 2));
              if (k + 1 <= n - 1) tst += fabs(h(k + 1, k));
            }
            if (sub <= ulp * tst) {
              const double up = fabs(h(k - 1, k)), dk = fabs(h(k, k)), dd = fabs(h(k - 1, k - 1) - h(k, k));
              const double ab = sub > up ? sub : up, ba = sub > up ? up : sub, aa = dk > dd ? dk : dd, bb = dk > dd ? dd : dk;
              const double s = aa + ab, rhs = ulp * (bb * (aa / s));
              if (ba * (ab / s) <= (smlnum > rhs ? smlnum : rhs)) hit = 1.0;
            }
          }
        }
        red[tid] = hit;
        lqr_sync();
        l = eig_first(red, i - l, i, l);
        if (l > 0 && tid == 0) h(l, l - 1) = 0.0;                // nobody reads H before the next barrier but at other entries
      }
      if (l >= i - 1) break;                                     // one or two eigenvalues have split off
      if (sweeps == cap) { status = 2; break; }
      sweeps++; its++;

      double h11, h21, h12, h22;
      if (its % 20 == 10) {                                      // exceptional shift from the top of the block
        const double s = fabs(h(l + 1, l)) + fabs(h(l + 2, l + 1));
        h11 = 0.75 * s + h(l, l); h12 = -0.4375 * s; h21 = s; h22 = h11;
      } else if (its % 20 == 0) {                                // ... from its bottom
        const double s = fabs(h(i, i - 1)) + fabs(h(i - 1, i - 2));
        h11 = 0.75 * s + h(i, i); h12 = -0.4375 * s; h21 = s; h22 = h11;
      } else {
        h11 = h(i - 1, i - 1); h21 = h(i, i - 1); h12 = h(i - 1, i); h22 = h(i, i);
      }
      double rt1r, rt1i, rt2r, rt2i;
      {
        const double s = fabs(h11) + fabs(h12) + fabs(h21) + fabs(h22);
        if (s == 0.0) { rt1r = rt1i = rt2r = rt2i = 0.0; }
        else {
          h11 /= s; h21 /= s; h12 /= s; h22 /= s;
          const double tr = (h11 + h22) * 0.5, det = (h11 - tr) * (h22 - tr) - h12 * h21, rtdisc = sqrt(fabs(det));
          if (det >= 0.0) { rt1r = tr * s; rt2r = rt1r; rt1i = rtdisc * s; rt2i = -rt1i; }
          else {
            rt1r = tr + rtdisc; rt2r = tr - rtdisc;
            if (fabs(rt1r - h22) <= fabs(rt2r - h22)) { rt1r *= s; rt2r = rt1r; } else { rt2r *= s; rt1r = rt2r; }
            rt1i = rt2i = 0.0;
          }
        }
      }
      // two consecutive small subdiagonal entries: lane t tests m = i - 2 - t (m > l), the highest m wins, else m = l
      auto start = [&](int m, double& v0, double& v1, double& v2) {
        const double hmm = h(m, m), h21a = fabs(h(m + 1, m));
        double s = fabs(hmm - rt2r) + fabs(rt2i) + h21a;
        const double h21s = h(m + 1, m) / s;
        v0 = h21s * h(m, m + 1) + (hmm - rt1r) * ((hmm - rt2r) / s) - rt1i * (rt2i / s);
        v1 = h21s * (hmm + h(m + 1, m + 1) - rt1r - rt2r);
        v2 = h21s * h(m + 2, m + 1);
        s = fabs(v0) + fabs(v1) + fabs(v2);
        v0 /= s; v1 /= s; v2 /= s;
      };
      double v0 = 0.0, v1 = 0.0, v2 = 0.0;
      double hit = 0.0;
      {
        const int mm = i - 2 - tid;
        if (mm > l) {
          start(mm, v0, v1, v2);
          const double h00 = fabs(h(mm - 1, mm - 1)), h11a = fabs(h(mm, mm)), h22a = fabs(h(mm + 1, mm + 1));
          if (fabs(h(mm, mm - 1)) * (fabs(v1) + fabs(v2)) <= ulp * fabs(v0) * (h00 + h11a + h22a)) hit = 1.0;
        }
      }
      lqr_sync();                                                // everybody has read the flags of the search above
      red[tid] = hit;
      lqr_sync();
      const int m = eig_first(red, i - 2 - l, i - 2, l);
      start(m, v0, v1, v2);
      for (int k = m; k < i; k++) {                              // the bulge chase
        const int nr = i - k + 1 < 3 ? i - k + 1 : 3;
        lqr_sync();                                              // column k - 1 is written; at k = m: all reads above are done
        if (k > m) { v0 = h(k, k - 1); v1 = h(k + 1, k - 1); v2 = nr == 3 ? h(k + 2, k - 1) : 0.0; }
        const double t1 = eig_larfg(nr, v0, v1, v2), t2 = t1 * v1, t3 = t1 * v2;
        const int j = k + tid;                                   // column j of the rows k .. k + nr - 1
        if (j <= i) {
          if (nr == 3) {
            const double a = h(k, j), b = h(k + 1, j), c = h(k + 2, j), sum = a + v1 * b + v2 * c;
            h(k, j) = a - sum * t1; h(k + 1, j) = b - sum * t2; h(k + 2, j) = c - sum * t3;
          } else {
            const double a = h(k, j), b = h(k + 1, j), sum = a + v1 * b;
            h(k, j) = a - sum * t1; h(k + 1, j) = b - sum * t2;
          }
        }
        lqr_sync();
        if (tid == 0) {
          if (k > m) { h(k, k - 1) = v0; h(k + 1, k - 1) = 0.0; if (k < i - 1) h(k + 2, k - 1) = 0.0; }
          else if (m > l) h(k, k - 1) *= 1.0 - t1;
        }
        const int r = l + tid, rmax = k + 3 < i ? k + 3 : i;     // row r of the columns k .. k + nr - 1
        if (r <= rmax) {
          if (nr == 3) {
            const double a = h(r, k), b = h(r, k + 1), c = h(r, k + 2), sum = a + v1 * b + v2 * c;
            h(r, k) = a - sum * t1; h(r, k + 1) = b - sum * t2; h(r, k + 2) = c - sum * t3;
          } else {
            const double a = h(r, k), b = h(r, k + 1), sum = a + v1 * b;
            h(r, k) = a - sum * t1; h(r, k + 1) = b - sum * t2;
          }
        }
      }
    }
    if (status) break;
    if (l == i) {
      if (tid == 0) { wr[i] = h(i, i); wi[i] = 0.0; }
    } else {
      double rt1r, rt1i, rt2r, rt2i;
      eig_lanv2(h(i - 1, i - 1), h(i - 1, i), h(i, i - 1), h(i, i), rt1r, rt1i, rt2r, rt2i);
      if (tid == 0) { wr[i - 1] = rt1r; wi[i - 1] = rt1i; wr[i] = rt2r; wi[i] = rt2i; }
    }
    i = l - 1;
  }
  lqr_sync();
  if (status) { eig_report(p, e, tid, status, sweeps, sc); return; }

  // 5. rank sort: descending modulus, then descending real part, then descending imaginary part (then the index: a total order)
  if (tid < n) v[tid] = eig_hypot(wr[tid], wi[tid]);
  lqr_sync();
  if (tid < n) {
    const double a = wr[tid], b = wi[tid], md = v[tid];
    int rank = 0;
    for (int k = 0; k < n; k++) {
      const double ak = wr[k], bk = wi[k], mk = v[k];
      if (mk > md || (mk == md && (ak > a || (ak == a && (bk > b || (bk == b && k < tid)))))) rank++;
    }
    p.wr[(long)e * n + rank] = a; p.wi[(long)e * n + rank] = b;
    p.scale[(long)e * n + tid] = sc[tid];
    if (rank == 0) p.rho[e] = md;
  }
  if (tid == 0) { p.status[e] = 0; p.sweeps[e] = sweeps; }
}

#ifndef MJB_HOST_EMU
// enqueue only (mjb_eig.hip); the entry point (mjb_api.hip) has checked every pointer and extent
hipError_t eig_launch(const EigArgs& p, hipStream_t stream);
#endif

}  // namespace mjb
