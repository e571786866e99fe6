// mjb_setpoint.hpp — the equilibrium controls of a batch of operating points (mjb_setpoint_ctrl): the minimum-norm u of
//   min_u | u @ moment - qfrc |_2,      moment [nu, nv] the actuator moment matrix,  qfrc [nv] the force inverse dynamics asks for,
// with the singular values of moment and a conditioning verdict, as wavefront-cooperative float64 device code.  It is what the reference
// computes on the host before every design, ctrl0 = qfrc0 @ pinv(actuator_moment) behind an SVD guard against a singular moment matrix
// (reference mujoco_template/setpoints.py:50-51, examples/humanoid/controllers/lqr.py:83); mjb_inverse leaves both operands in device memory.
//
// One-sided (Hestenes) Jacobi SVD of G = moment' [nv, nu] itself, never an eigen-solve of G'G (that squares the condition number the
// guard tests); Jacobi also keeps high relative accuracy when actuator rows differ by orders of magnitude (gear ratios).  Per problem:
//   1. G [nv, nu], column a = row a of moment; V = I [nu, nu].  An entry of moment or qfrc that is not finite, or a sum(G^2) that is
//      not (finite entries above 1e154, whose squares overflow): status 1.
//   2. tol = 2^-52, floor = tol^2 sum(G^2): a column whose squared norm is <= floor is rounding noise and is never rotated (the nu - nv
//      null columns of a wide problem, nu > nv, would otherwise rotate for ever).
//   3. Sweeps of the round-robin schedule below.  For a pair i < j: a = |g_i|^2, b = |g_j|^2, c = g_i . g_j; skipped if c == 0 or
//      |c| <= tol sqrt(a) sqrt(b) or min(a, b) <= floor; otherwise z = (b - a) / (2 c), t = sign(z) / (|z| + hypot(1, z)) (z == 0: t = 1),
//      cs = 1 / sqrt(1 + t^2), sn = cs t, (g_i, g_j) <- (cs g_i - sn g_j, sn g_i + cs g_j) and the same for the columns of V.
//   4. A sweep without a rotation ends the iteration (it is counted in `sweeps`); max_sweeps sweeps that each rotated: status 2.
//   5. sigma_j = sqrt(|g_j|^2), sorted descending, ties by lower index; r = min(nu, nv); sv = the first r; rcond = sigma_r / sigma_1
//      (0 when sigma_1 == 0); rank = the count of sigma_j > rcond_min sigma_1 among them; rcond < rcond_min: status 3.
//   6. ctrl = sum_j v_j (g_j . qfrc) / |g_j|^2 over the first r columns in sorted order, terms with sigma_j == 0 skipped;
//      residual = max_i |(ctrl @ moment - qfrc)_i| with moment re-read from global memory; optionally pinv [nv, nu] = sum_j g_j v_j' / |g_j|^2.
// A failed problem has NaN in ctrl and pinv and +inf in residual; sv, rcond, rank and sweeps hold what was reached (status 1: NaN, NaN,
// 0, 0); it touches no other problem.
//
// The schedule.  n' = nu rounded up to even; a sweep has n' - 1 rounds of n' / 2 pairs (the circle method: index n' - 1 stays, the
// others go round).  In round rd (0 .. n' - 2), pair 0 is (n' - 1, rd) and pair k (1 .. n' / 2 - 1) is ((rd + k) mod (n' - 1),
// (rd - k) mod (n' - 1)); each is taken as (i, j) = (min, max), and a pair with j >= nu (odd nu: the partner of the padding index)
// is idle.  The pairs of a round are disjoint, so they run concurrently and their order cannot matter; over a sweep every pair i < j
// is met exactly once.
//
// Mapping: ONE wavefront per problem, G and V resident in LDS by column with the odd leading dimensions nv | 1 and nu | 1.  The up to
// 16 pairs of a round take four lanes each (lane = 4 pair + s): lane s sums the rows s, s + 4, ... of the three dot products, the four
// partial sums go through LDS and every lane of the pair adds them in the order s = 0 .. 3 (so the four agree bitwise on the
// rotation), then lane s rotates the rows s, s + 4, ... of G and of V.  Two wave-scope barriers per round (no s_barrier is emitted for a
// workgroup of one wave).  With few actuators most lanes idle (a cart-pole uses none: nu = 1 has no pair); occupancy comes from the
// batch: 28.3 KB of LDS at 32 x 64, 2.1 KB for a 1 x 2 problem.  Every reduction runs in a fixed order, so a problem gives the same
// bits at any position of any batch.  There is no matrix product here worth the f64 MFMA.  The measured times are in INTEGRATION.md.
// The same source compiles in the host emulation of mjb_lqr.hpp (MJB_HOST_EMU), which only the CPU test-suite uses.
#pragma once
#include "mjb_eig.hpp"

namespace mjb {

static const int kSetpointMaxNu = 32, kSetpointMaxNv = 64, kSetpointMaxSweeps = 64, kSetpointDefaultSweeps = 30;

struct SetpointArgs {
  int B, nu, nv, max_sweeps, m_f32, q_f32;          // max_sweeps 0 = the default; *_f32: the elements are float (widened exactly)
  double rcond_min;
  const void *moment, *qfrc;                        // per problem e: element e * m_es (e * q_es) onwards, [nu, nv] and [nv] dense
  long m_es, q_es;
  double *ctrl, *sv, *rcond, *residual, *pinv;      // [B, nu], [B, min(nu, nv)], [B], [B], [B, nv, nu] (may be null)
  int *rank, *sweeps, *status;                      // [B]
};

// ---- LDS layout (offsets in doubles) --------------------------------------------------------------------------------------------
// G [nv, nu] and V [nu, nu] by column, leading dimensions ldg = nv | 1, ldv = nu | 1.  q: qfrc widened.  red: three partial sums per
// lane (later |residual_i|).  flg: one word per lane.  s2, sg: |g_j|^2 and its root.  perm: the column of each sorted position.
// wq: (g_j . qfrc) / |g_j|^2.  u: ctrl.
struct SetpointLay { int G, V, q, red, flg, s2, sg, perm, wq, u, ldg, ldv, total; };
MJB_LQR_HD SetpointLay setpoint_layout(int nu, int nv) {
  SetpointLay l;
  l.ldg = nv | 1; l.ldv = nu | 1;
  int o = 0;
  l.G = o; o += nu * l.ldg;
  l.V = o; o += nu * l.ldv;
  l.q = o; o += nv;
  l.red = o; o += 3 * 64;
  l.flg = o; o += 64;
  l.s2 = o; o += nu;
  l.sg = o; o += nu;
  l.perm = o; o += nu;
  l.wq = o; o += nu;
  l.u = o; o += nu;
  l.total = o;
  return l;
}

// 0 ok; otherwise which limit is broken (the entry point turns it into the message).  max_sweeps 0 = the default
inline int setpoint_size_error(long B, long nu, long nv, long max_sweeps, double rcond_min) {
  if (B < 1) return 1;
  if (nu < 1 || nu > kSetpointMaxNu) return 2;
  if (nv < 1 || nv > kSetpointMaxNv) return 3;
  if (max_sweeps < 0 || max_sweeps > kSetpointMaxSweeps) return 4;
  if (!(rcond_min >= 0.0) || !(rcond_min <= 1.7976931348623157e308)) return 5;
  if ((__int128)B * nu * nv > ((__int128)1 << 40)) return 6;
  return 0;
}

// pair k of round rd of the schedule above as (i, j), i < j; n2 = n' (even, >= 2)
MJB_LQR_HD void setpoint_pair(int n2, int rd, int k, int& i, int& j) {
  const int m = n2 - 1;
  const int a = k == 0 ? m : (rd + k) % m, b = k == 0 ? rd : (rd - k + m) % m;
  i = a < b ? a : b; j = a < b ? b : a;
}

MJB_LQR_DEV double setpoint_in(const void* base, int f32, long i) {
  return f32 ? (double)((const float*)base)[i] : ((const double*)base)[i];
}

// ---- problem e -----------------------------------------------------------------------------------------------------------------
// One wave (64 threads, tid), w: setpoint_layout(nu, nv).total doubles of LDS.  Every decision that encloses a barrier is computed by
// every thread from the same LDS words, read between two barriers in which nobody writes them: uniform.
MJB_LQR_DEV void setpoint_env(const SetpointArgs& p, int e, int tid, double* w) {
  const int nu = p.nu, nv = p.nv, r = nu < nv ? nu : nv;
  const SetpointLay l = setpoint_layout(nu, nv);
  const int ldg = l.ldg, ldv = l.ldv;
  double *G = w + l.G, *V = w + l.V, *q = w + l.q, *red = w + l.red, *flg = w + l.flg, *s2 = w + l.s2, *sg = w + l.sg, *perm = w + l.perm,
         *wq = w + l.wq, *u = w + l.u;
  const double inf = __builtin_huge_val(), nan = __builtin_nan(""), tol = 0x1p-52;
  const long m0 = (long)e * p.m_es, q0 = (long)e * p.q_es;

  // status 1: nothing was reached
  auto not_finite = [&]() {
    if (tid < r) p.sv[(long)e * r + tid] = nan;
    if (tid < nu) p.ctrl[(long)e * nu + tid] = nan;
    if (p.pinv) for (int i = tid; i < nv * nu; i += 64) p.pinv[(long)e * nv * nu + i] = nan;
    if (tid == 0) { p.rcond[e] = nan; p.residual[e] = inf; p.rank[e] = 0; p.sweeps[e] = 0; p.status[e] = 1; }
  };

  // 1. G = moment', V = I, q = qfrc
  {
    double bad = 0.0;
    for (int i = tid; i < nu * nv; i += 64) {
      const double x = setpoint_in(p.moment, p.m_f32, m0 + i);
      if (!dare_finite(x)) bad = 1.0;
      G[(i % nv) + (i / nv) * ldg] = x;
    }
    for (int i = tid; i < nv; i += 64) {
      const double x = setpoint_in(p.qfrc, p.q_f32, q0 + i);
      if (!dare_finite(x)) bad = 1.0;
      q[i] = x;
    }
    for (int i = tid; i < nu * nu; i += 64) V[(i % nu) + (i / nu) * ldv] = i % nu == i / nu ? 1.0 : 0.0;
    flg[tid] = bad;
    lqr_sync();
    double any = 0.0;
    for (int t = 0; t < 64; t++) any += flg[t];
    if (any != 0.0) { not_finite(); return; }
  }

  // 2. the noise floor
  if (tid < nu) {
    double s = 0.0;
    for (int k = 0; k < nv; k++) { const double x = G[k + tid * ldg]; s += x * x; }
    s2[tid] = s;
  }
  lqr_sync();
  double floor2 = 0.0;
  for (int j = 0; j < nu; j++) floor2 += s2[j];
  if (!dare_finite(floor2)) { not_finite(); return; }             // finite entries whose squares overflow: no norm, no verdict (uniform)
  floor2 *= tol * tol;

  // 3., 4. the sweeps
  const int np = (nu + 1) >> 1, n2 = 2 * np, pr = tid >> 2, sub = tid & 3;
  const int cap = p.max_sweeps > 0 ? p.max_sweeps : kSetpointDefaultSweeps;
  int sweeps = 0;
  bool converged = false;
  while (sweeps < cap) {
    double rot = 0.0;
    for (int rd = 0; rd < n2 - 1; rd++) {
      int i = 0, j = nu;
      if (pr < np) setpoint_pair(n2, rd, pr, i, j);
      const bool on = pr < np && j < nu;
      double *gi = G + i * ldg, *gj = G + (on ? j : 0) * ldg;
      if (on) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int k = sub; k < nv; k += 4) { const double x = gi[k], y = gj[k]; a += x * x; b += y * y; c += x * y; }
        red[3 * tid] = a; red[3 * tid + 1] = b; red[3 * tid + 2] = c;
      }
      lqr_sync();
      if (on) {
        const double* h = red + 12 * pr;
        const double a = ((h[0] + h[3]) + h[6]) + h[9], b = ((h[1] + h[4]) + h[7]) + h[10], c = ((h[2] + h[5]) + h[8]) + h[11];
        const bool skip = c == 0.0 || fabs(c) <= tol * sqrt(a) * sqrt(b) || (a < b ? a : b) <= floor2;
        if (!skip) {
          const double z = (b - a) / (2.0 * c);
          const double t = z == 0.0 ? 1.0 : copysign(1.0, z) / (fabs(z) + eig_hypot(1.0, z));
          const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
          for (int k = sub; k < nv; k += 4) { const double x = gi[k], y = gj[k]; gi[k] = cs * x - sn * y; gj[k] = sn * x + cs * y; }
          double *vi = V + i * ldv, *vj = V + j * ldv;
          for (int k = sub; k < nu; k += 4) { const double x = vi[k], y = vj[k]; vi[k] = cs * x - sn * y; vj[k] = sn * x + cs * y; }
          rot = 1.0;
        }
      }
      lqr_sync();
    }
    sweeps++;
    flg[tid] = rot;
    lqr_sync();
    double any = 0.0;
    for (int t = 0; t < 64; t++) any += flg[t];
    if (any == 0.0) { converged = true; break; }
  }

  // 5. the singular values, their order, the verdict
  if (tid < nu) {
    double s = 0.0, d = 0.0;
    for (int k = 0; k < nv; k++) { const double x = G[k + tid * ldg]; s += x * x; d += x * q[k]; }
    s2[tid] = s; sg[tid] = sqrt(s); wq[tid] = s > 0.0 ? d / s : 0.0;
    perm[tid] = (double)tid;                                     // a norm that is not a number has no rank: every position still names a column
  }
  lqr_sync();
  if (tid < nu) {
    const double mine = sg[tid];
    int pos = 0;
    for (int k = 0; k < nu; k++) { const double o = sg[k]; if (o > mine || (o == mine && k < tid)) pos++; }
    perm[pos] = (double)tid;
  }
  lqr_sync();
  const double s1 = sg[(int)perm[0]], sr = sg[(int)perm[r - 1]], rcond = s1 == 0.0 ? 0.0 : sr / s1;
  int rank = 0;
  for (int t = 0; t < r; t++) if (sg[(int)perm[t]] > p.rcond_min * s1) rank++;
  const int status = !converged ? 2 : !(rcond >= p.rcond_min) ? 3 : 0;   // a rcond that is not a number is no pass
  if (tid < r) p.sv[(long)e * r + tid] = sg[(int)perm[tid]];
  if (tid == 0) { p.rcond[e] = rcond; p.rank[e] = rank; p.sweeps[e] = sweeps; p.status[e] = status; }
  if (status) {
    if (tid < nu) p.ctrl[(long)e * nu + tid] = nan;
    if (p.pinv) for (int i = tid; i < nv * nu; i += 64) p.pinv[(long)e * nv * nu + i] = nan;
    if (tid == 0) p.residual[e] = inf;
    return;
  }

  // 6. the solution, what no actuator can supply, the pseudo-inverse
  if (tid < nu) {
    double s = 0.0;
    for (int t = 0; t < r; t++) { const int j = (int)perm[t]; if (sg[j] != 0.0) s += V[tid + j * ldv] * wq[j]; }
    u[tid] = s;
    p.ctrl[(long)e * nu + tid] = s;
  }
  lqr_sync();
  if (tid < nv) {
    double s = 0.0;
    for (int a = 0; a < nu; a++) s += u[a] * setpoint_in(p.moment, p.m_f32, m0 + (long)a * nv + tid);
    red[tid] = fabs(s - q[tid]);
  }
  lqr_sync();
  if (tid == 0) {
    double m = 0.0;
    for (int i = 0; i < nv; i++) if (red[i] > m) m = red[i];
    p.residual[e] = m;
  }
  if (p.pinv)
    for (int i = tid; i < nv * nu; i += 64) {
      const int k = i / nu, a = i % nu;
      double s = 0.0;
      for (int t = 0; t < r; t++) { const int j = (int)perm[t]; if (sg[j] != 0.0) s += G[k + j * ldg] * V[a + j * ldv] / s2[j]; }
      p.pinv[(long)e * nv * nu + i] = s;
    }
}

#ifndef MJB_HOST_EMU
// enqueue only (mjb_setpoint.hip); the entry point (mjb_api.hip) has checked every pointer and extent
hipError_t setpoint_launch(const SetpointArgs& p, hipStream_t stream);
#endif

}  // namespace mjb
