// mjb_traj.hpp — the quadratic trajectory cost with its first-order expansion (mjb_traj_cost) and the selection / softmin update over
// candidate controls (mjb_traj_select) as float64 device code.  Formulas: include/mjbatch.h.
//
// Cost: the (T + 1) x B points of a call are independent.  One wavefront takes a tile of kTrajTile points: it forms their tangent-space
// deviations dx (the quaternion rule of mjb_differentiate_pos) and du in LDS, then every lane accumulates its row(s) of Q dx for all
// points of the tile at once - each element of Q is loaded once per tile, as Q[j, lane] (Q is taken as symmetric, so the lanes of
// one load are consecutive in memory), and multiplied into kTrajTile accumulators.  The arithmetic of a point never depends on which
// tile or lane group it lands in: j ascends, the lanes' partial costs meet in a fixed 64-leaf tree.  A second kernel sums cost_t
// over t in an order fixed by T alone.
//
// Select: one workgroup per (problem, chunk of 16 elements of u_out).  Every workgroup of a problem finds the same (minimal finite
// cost, lowest index) and, for SOFTMIN, the same normaliser; it then copies its chunk, or accumulates it with the candidates dealt
// round-robin to 16 slices of threads (the weights staged in LDS tiles) whose partial sums meet in a fixed tree.
//
// The same source compiles in a host emulation (MJB_HOST_EMU: one std::thread per lane, a pthread barrier per workgroup) that only the
// CPU test-suite uses; the product library never contains that build.
#pragma once
#include <cmath>
#include <cstddef>

#ifdef MJB_HOST_EMU
#include <pthread.h>
#define MJB_TRAJ_DEV static inline
#else
#include <hip/hip_runtime.h>
#define MJB_TRAJ_DEV __device__ __forceinline__
#endif

namespace mjb {

static const int kTrajMaxNv = 64, kTrajMaxNu = 64;
static const int kTrajTile = 8;                        // points per wavefront pass
static const int kTrajSelThreads = 256, kTrajSelTile = 1024;      // select: threads per workgroup, weights per LDS tile
static const int kTrajSelElems = 16, kTrajSelSlices = kTrajSelThreads / kTrajSelElems;       // elements of u_out per workgroup x slices of candidates
static const long kTrajMaxCand = 1L << 20, kTrajMaxSelElems = 1L << 22;
static const int kTrajJntFree = 0;                     // mjtJoint: free = 0; slide and hinge are scalar joints
static const int kTrajArgmin = 0, kTrajSoftmin = 1;    // MJB_SELECT_ARGMIN / MJB_SELECT_SOFTMIN
static const double kTrajDblMax = 1.7976931348623157e308;

struct TrajIn { const void* p; long ss, es; };         // float32 or float64 (the call's flag): block (t, e) at p + t * ss + e * es, in elements
struct TrajRef { const double* p; long ss, es; };

struct TrajCostArgs {
  int T, B, nq, nv, nu, njnt, state_f32, ctrl_f32;
  TrajIn qpos0, qvel0, qpos, qvel, ctrl;               // qpos0 / qvel0: env stride only; qpos / qvel (t, e): the state AFTER step t
  TrajRef qref, vref, uref, Q, R, Qf;                  // qref / vref per point 0 .. T (vref.p null = 0), uref (null = 0), Q, R per (t, e), Qf per e
  const int *jnt_type, *jnt_qposadr, *jnt_dofadr;
  double *cost, *cost_t, *lx, *lu, *VxT;               // cost [B], cost_t [B, T + 1]; lx [T, B, 2nv], lu [T, B, nu], VxT [B, 2nv] may be null
};

struct TrajSelectArgs {
  int nprob, T, nu, mode, cand_f32, out_f32;
  long ncand;
  double temperature;
  const double* cost;                                  // [nprob, ncand]
  const void* cand;                                    // [nprob, ncand, T, nu]
  void* u_out;                                         // [nprob, T, nu]
  int* best; double* best_cost; double* weights;       // [nprob], [nprob], [nprob, ncand]; each may be null
};

// ---- host arithmetic of the argument checks (no HIP: tested without a GPU) -----------------------------------------------------------
// Highest element a strided array of `nstep` x B blocks of n elements touches; false: an empty extent or a negative stride.
inline bool traj_highest_element(long nstep, long B, long n, long ss, long es, __int128& hi) {
  hi = -1;
  if (nstep < 1 || B < 1 || n < 1 || ss < 0 || es < 0) return false;
  hi = (__int128)(nstep - 1) * ss + (__int128)(B - 1) * es + (n - 1);
  return true;
}
// 0 ok; otherwise which limit the sizes break (the entry points turn it into the message)
inline int traj_cost_size_error(long T, long B, long nq, long nv, long nu) {
  if (T < 1) return 1;
  if (B < 1) return 2;
  if (nv < 1 || nv > kTrajMaxNv) return 3;
  if (nu < 1 || nu > kTrajMaxNu) return 4;
  if (nq < nv || nq > 2 * nv) return 5;
  if ((__int128)(T + 1) * B * 2 * nv > ((__int128)1 << 40)) return 6;
  return 0;
}
inline int traj_select_size_error(long nprob, long ncand, long T, long nu, int mode, double temperature) {
  if (nprob < 1 || nprob > (1L << 30)) return 1;
  if (ncand < 1 || ncand > kTrajMaxCand) return 2;
  if (T < 1 || nu < 1 || (__int128)T * nu > kTrajMaxSelElems) return 3;
  if (mode != kTrajArgmin && mode != kTrajSoftmin) return 4;
  if (mode == kTrajSoftmin && !(temperature > 0.0 && temperature <= kTrajDblMax)) return 5;
  if ((__int128)nprob * ncand * T * nu > ((__int128)1 << 44)) return 6;
  return 0;
}
// tiles of kTrajTile points: the T * B stage points (index t * B + e) first, then the B terminal points - no tile holds both kinds
inline long traj_cost_tiles(long T, long B) { return (T * B + kTrajTile - 1) / kTrajTile + (B + kTrajTile - 1) / kTrajTile; }
// LDS of one wavefront of the cost kernel, in doubles: dx, du of the tile and the 64 leaves of every point's cost tree
inline int traj_cost_lds(int nv, int nu) { return kTrajTile * (2 * nv + nu + 64); }
// LDS of the select kernel, in doubles: (cost, index) per thread and one tile of weights
inline int traj_select_lds() { return 2 * kTrajSelThreads + kTrajSelTile; }

// ---- workgroup primitives --------------------------------------------------------------------------------------------------------------
#ifdef MJB_HOST_EMU
namespace trajemu {
struct Block {
  pthread_barrier_t bar;
  explicit Block(int n) { pthread_barrier_init(&bar, nullptr, (unsigned)n); }
  ~Block() { pthread_barrier_destroy(&bar); }
};
inline thread_local Block* tl_block = nullptr;
}  // namespace trajemu
static inline void traj_sync() { pthread_barrier_wait(&trajemu::tl_block->bar); }
#else
MJB_TRAJ_DEV void traj_sync() { __syncthreads(); }
#endif

MJB_TRAJ_DEV double traj_ld(const void* p, long i, int f32) { return f32 ? (double)((const float*)p)[i] : ((const double*)p)[i]; }
MJB_TRAJ_DEV bool traj_finite(double v) { return fabs(v) <= kTrajDblMax; }

// res [3] = the rotation from q1 to q2 as a tangent vector (mjb_differentiate_pos with dt = 1).  No contraction into fused
// multiply-adds here: with q2 == q1 every component of the vector part is then exactly 0.
MJB_TRAJ_DEV void traj_quat_diff(double* res, const double* q1, const double* q2) {
#ifndef MJB_HOST_EMU
#pragma clang fp contract(off)
#endif
  const double a0 = q1[0], a1 = -q1[1], a2 = -q1[2], a3 = -q1[3];
  const double w = a0 * q2[0] - a1 * q2[1] - a2 * q2[2] - a3 * q2[3], x = a0 * q2[1] + a1 * q2[0] + a2 * q2[3] - a3 * q2[2];
  const double y = a0 * q2[2] - a1 * q2[3] + a2 * q2[0] + a3 * q2[1], z = a0 * q2[3] + a1 * q2[2] - a2 * q2[1] + a3 * q2[0];
  const double sn = sqrt(x * x + y * y + z * z);
  if (sn < 1e-15) { res[0] = res[1] = res[2] = 0.0; return; }
  const double PI = 3.14159265358979323846;
  double ang = 2 * atan2(sn, w);
  if (ang > PI) ang -= 2 * PI;
  const double k = ang / sn;
  res[0] = x * k; res[1] = y * k; res[2] = z * k;
}

// ---- the cost of one tile of points: one wavefront (lane 0 .. 63), w = traj_cost_lds(nv, nu) doubles of LDS ------------------------------
MJB_TRAJ_DEV void traj_cost_tile(const TrajCostArgs& a, long tile, int lane, double* w) {
  constexpr int P = kTrajTile;
  const int nv = a.nv, nx = 2 * a.nv, nu = a.nu, T = a.T;
  const long B = a.B, nstage = (long)T * B, stage_tiles = (nstage + P - 1) / P;
  const bool term = tile >= stage_tiles;
  const long first = term ? (tile - stage_tiles) * P : tile * P, count = term ? B : nstage;
  const int np = count - first < P ? (int)(count - first) : P;
  double *dx = w, *du = w + P * nx, *red = du + P * nu;

  // dx, du of the tile's points (zeros for the slots beyond the last point)
  for (int p = 0; p < P; p++) {
    double* dxp = dx + p * nx;
    double* dup = du + p * nu;
    if (p >= np) {
      for (int i = lane; i < nx; i += 64) dxp[i] = 0.0;
      if (lane < nu) dup[lane] = 0.0;
      continue;
    }
    const long idx = first + p;
    const int t = term ? T : (int)(idx / B);
    const long e = term ? idx : idx % B;
    const void *qp, *qv;
    if (t == 0) {
      qp = (const char*)a.qpos0.p + (e * a.qpos0.es) * (a.state_f32 ? 4 : 8);
      qv = (const char*)a.qvel0.p + (e * a.qvel0.es) * (a.state_f32 ? 4 : 8);
    } else {
      qp = (const char*)a.qpos.p + ((long)(t - 1) * a.qpos.ss + e * a.qpos.es) * (a.state_f32 ? 4 : 8);
      qv = (const char*)a.qvel.p + ((long)(t - 1) * a.qvel.ss + e * a.qvel.es) * (a.state_f32 ? 4 : 8);
    }
    const double* qr = a.qref.p + (long)t * a.qref.ss + e * a.qref.es;
    const double* vr = a.vref.p ? a.vref.p + (long)t * a.vref.ss + e * a.vref.es : nullptr;
    if (lane < a.njnt) {
      const int qa = a.jnt_qposadr[lane], da = a.jnt_dofadr[lane];
      if (a.jnt_type[lane] == kTrajJntFree) {
        for (int k = 0; k < 3; k++) dxp[da + k] = traj_ld(qp, qa + k, a.state_f32) - qr[qa + k];
        double q1[4], q2[4];
        for (int k = 0; k < 4; k++) { q1[k] = qr[qa + 3 + k]; q2[k] = traj_ld(qp, qa + 3 + k, a.state_f32); }
        traj_quat_diff(dxp + da + 3, q1, q2);
      } else {
        dxp[da] = traj_ld(qp, qa, a.state_f32) - qr[qa];
      }
    }
    if (lane < nv) dxp[nv + lane] = traj_ld(qv, lane, a.state_f32) - (vr ? vr[lane] : 0.0);
    if (!term && lane < nu) {
      const void* up = (const char*)a.ctrl.p + ((long)t * a.ctrl.ss + e * a.ctrl.es) * (a.ctrl_f32 ? 4 : 8);
      const double ur = a.uref.p ? a.uref.p[(long)t * a.uref.ss + e * a.uref.es + lane] : 0.0;
      dup[lane] = traj_ld(up, lane, a.ctrl_f32) - ur;
    } else if (lane < nu) {
      dup[lane] = 0.0;
    }
  }
  traj_sync();

  // lx = Q dx (VxT = Qf dx): lane l owns rows l and l + 64; Q[j, l] for Q[l, j] - symmetric - so that a load is one run of memory
  const double* M[P];
  long et[P]; int tt[P];
#pragma unroll
  for (int p = 0; p < P; p++) {
    const long idx = first + (p < np ? p : 0);
    tt[p] = term ? T : (int)(idx / B);
    et[p] = term ? idx : idx % B;
    M[p] = term ? a.Qf.p + et[p] * a.Qf.es : a.Q.p + (long)tt[p] * a.Q.ss + et[p] * a.Q.es;
  }
  const bool shared_q = term ? a.Qf.es == 0 : (a.Q.ss == 0 && a.Q.es == 0);
  const int r0 = lane, r1 = lane + 64;
  const bool on0 = r0 < nx, on1 = r1 < nx;
  double acc0[P], acc1[P];
#pragma unroll
  for (int p = 0; p < P; p++) { acc0[p] = 0.0; acc1[p] = 0.0; }
  if (shared_q) {
    const double* Mq = M[0];
    for (int j = 0; j < nx; j++) {
      const double m0 = on0 ? Mq[(long)j * nx + r0] : 0.0, m1 = on1 ? Mq[(long)j * nx + r1] : 0.0;
#pragma unroll
      for (int p = 0; p < P; p++) { const double x = dx[p * nx + j]; acc0[p] = fma(m0, x, acc0[p]); acc1[p] = fma(m1, x, acc1[p]); }
    }
  } else {
    for (int j = 0; j < nx; j++) {
#pragma unroll
      for (int p = 0; p < P; p++) {
        const double m0 = on0 ? M[p][(long)j * nx + r0] : 0.0, m1 = on1 ? M[p][(long)j * nx + r1] : 0.0;
        const double x = dx[p * nx + j];
        acc0[p] = fma(m0, x, acc0[p]); acc1[p] = fma(m1, x, acc1[p]);
      }
    }
  }
  double part[P];
#pragma unroll
  for (int p = 0; p < P; p++) {
    part[p] = (on0 ? dx[p * nx + r0] * acc0[p] : 0.0) + (on1 ? dx[p * nx + r1] * acc1[p] : 0.0);
    if (p < np) {
      double* out = term ? (a.VxT ? a.VxT + et[p] * nx : nullptr) : (a.lx ? a.lx + ((long)tt[p] * B + et[p]) * nx : nullptr);
      if (out) { if (on0) out[r0] = acc0[p]; if (on1) out[r1] = acc1[p]; }
    }
  }

  // lu = R du and its share of the cost (stage points only; nu <= 64: one row per lane)
  if (!term) {
    const bool shared_r = a.R.ss == 0 && a.R.es == 0, onu = lane < nu;
    double accu[P];
#pragma unroll
    for (int p = 0; p < P; p++) accu[p] = 0.0;
    for (int b = 0; b < nu; b++) {
      const double ms = (shared_r && onu) ? a.R.p[(long)b * nu + lane] : 0.0;
#pragma unroll
      for (int p = 0; p < P; p++) {
        const double m = shared_r ? ms : (onu ? a.R.p[(long)tt[p] * a.R.ss + et[p] * a.R.es + (long)b * nu + lane] : 0.0);
        accu[p] = fma(m, du[p * nu + b], accu[p]);
      }
    }
#pragma unroll
    for (int p = 0; p < P; p++) {
      if (onu) {
        part[p] += du[p * nu + lane] * accu[p];
        if (p < np && a.lu) a.lu[((long)tt[p] * B + et[p]) * nu + lane] = accu[p];
      }
    }
  }

  // the lanes' parts of every point's cost: a fixed 64-leaf tree
#pragma unroll
  for (int p = 0; p < P; p++) red[p * 64 + lane] = part[p];
  traj_sync();
  for (int s = 32; s >= 1; s >>= 1) {
    if (lane < s)
      for (int p = 0; p < P; p++) red[p * 64 + lane] += red[p * 64 + lane + s];
    traj_sync();
  }
#pragma unroll
  for (int p = 0; p < P; p++)
    if (lane == p && p < np) a.cost_t[et[p] * (T + 1) + tt[p]] = 0.5 * red[p * 64];
  traj_sync();                                                   // the next tile of this wavefront reuses the LDS
}

// cost[e] = sum_t cost_t[e, t]: lane l adds t = l, l + 64, ... in ascending order, then the 64-leaf tree; not finite -> +inf.  w: 64 doubles
MJB_TRAJ_DEV void traj_cost_sum(const TrajCostArgs& a, long e, int lane, double* w) {
  const double* c = a.cost_t + e * (a.T + 1);
  double s = 0.0;
  for (int t = lane; t <= a.T; t += 64) s += c[t];
  w[lane] = s;
  traj_sync();
  for (int k = 32; k >= 1; k >>= 1) {
    if (lane < k) w[lane] += w[lane + k];
    traj_sync();
  }
  if (lane == 0) a.cost[e] = traj_finite(w[0]) ? w[0] : INFINITY;
  traj_sync();
}

inline long traj_select_chunks(long T, long nu) { return (T * nu + kTrajSelElems - 1) / kTrajSelElems; }

// ---- select: workgroup (problem g, chunk) of kTrajSelThreads threads, w = traj_select_lds() doubles of LDS -------------------------------
MJB_TRAJ_DEV void traj_select_block(const TrajSelectArgs& a, long g, long chunk, int tid, double* w) {
  constexpr int NT = kTrajSelThreads, WT = kTrajSelTile, ES = kTrajSelElems, NS = kTrajSelSlices;
  const int el = tid % ES, sl = tid / ES;
  const long n = a.ncand, M = (long)a.T * a.nu;
  const double* c = a.cost + g * n;
  double *rc = w, *ri = w + NT, *wt = w + 2 * NT;                // indices < 2^20 are exact in a double
  double bc = INFINITY, bi = -1.0;
  for (long j = tid; j < n; j += NT) {                           // ascending j: a thread keeps the lowest index among equals
    const double v = c[j];
    if (traj_finite(v) && (bi < 0.0 || v < bc)) { bc = v; bi = (double)j; }
  }
  rc[tid] = bc; ri[tid] = bi;
  traj_sync();
  for (int s = NT / 2; s >= 1; s >>= 1) {
    if (tid < s) {
      const double oc = rc[tid + s], oi = ri[tid + s];
      if (oi >= 0.0 && (ri[tid] < 0.0 || oc < rc[tid] || (oc == rc[tid] && oi < ri[tid]))) { rc[tid] = oc; ri[tid] = oi; }
    }
    traj_sync();
  }
  const long best = (long)ri[0];
  const double cmin = rc[0];
  traj_sync();
  if (chunk == 0 && tid == 0) {
    if (a.best) a.best[g] = (int)best;
    if (a.best_cost) a.best_cost[g] = best < 0 ? INFINITY : cmin;
  }
  const long i = chunk * ES + el;                                // this thread's element of u_out[g]; slice sl of the candidates
  if (best < 0) {                                                // no finite cost: u_out keeps what the caller put there
    if (a.mode == kTrajSoftmin && a.weights && chunk == 0) for (long j = tid; j < n; j += NT) a.weights[g * n + j] = 0.0;
    return;
  }
  if (a.mode == kTrajArgmin) {
    if (i < M && sl == 0) {
      const long src = (g * n + best) * M + i, dst = g * M + i;
      if (a.cand_f32 && a.out_f32) ((float*)a.u_out)[dst] = ((const float*)a.cand)[src];
      else if (a.cand_f32) ((double*)a.u_out)[dst] = (double)((const float*)a.cand)[src];
      else if (a.out_f32) ((float*)a.u_out)[dst] = (float)((const double*)a.cand)[src];
      else ((double*)a.u_out)[dst] = ((const double*)a.cand)[src];
    }
    return;
  }
  // SOFTMIN.  The normaliser: per-thread sums in ascending j, then the tree
  double z = 0.0;
  for (long j = tid; j < n; j += NT) { const double v = c[j]; if (traj_finite(v)) z += exp(-(v - cmin) / a.temperature); }
  rc[tid] = z;
  traj_sync();
  for (int s = NT / 2; s >= 1; s >>= 1) {
    if (tid < s) rc[tid] += rc[tid + s];
    traj_sync();
  }
  const double Z = rc[0];                                        // >= 1: the best candidate contributes exp(0)
  double acc = 0.0;
  for (long j0 = 0; j0 < n; j0 += WT) {
    const int m = n - j0 < WT ? (int)(n - j0) : WT;
    for (int k = tid; k < m; k += NT) {
      const double v = c[j0 + k];
      const double wj = traj_finite(v) ? exp(-(v - cmin) / a.temperature) / Z : 0.0;
      wt[k] = wj;
      if (a.weights && chunk == 0) a.weights[g * n + j0 + k] = wj;
    }
    traj_sync();
    if (i < M) {
      const long base = (g * n + j0) * M + i;
      if (a.cand_f32) for (int k = sl; k < m; k += NS) acc = fma(wt[k], (double)((const float*)a.cand)[base + (long)k * M], acc);
      else for (int k = sl; k < m; k += NS) acc = fma(wt[k], ((const double*)a.cand)[base + (long)k * M], acc);
    }
    traj_sync();
  }
  rc[tid] = acc;                                                 // the slices' partial sums of an element: a fixed tree
  traj_sync();
  for (int s = NS / 2; s >= 1; s >>= 1) {
    if (sl < s) rc[tid] += rc[tid + s * ES];
    traj_sync();
  }
  if (i < M && sl == 0) {
    if (a.out_f32) ((float*)a.u_out)[g * M + i] = (float)rc[tid]; else ((double*)a.u_out)[g * M + i] = rc[tid];
  }
  traj_sync();
}

#ifndef MJB_HOST_EMU
// enqueue only (mjb_traj.hip); the entry points (mjb_api.hip) have checked every pointer and extent
hipError_t traj_launch_cost(const TrajCostArgs& p, hipStream_t stream);
hipError_t traj_launch_select(const TrajSelectArgs& p, hipStream_t stream);
#endif

}  // namespace mjb
