// mjb_feedback.hpp — the linear feedback law from device tensors (mjb_feedback_law, the law kernel of mjb_rollout_feedback) as float64
// device code.  For environment e of the data object at step index t, all arithmetic in float64, float32 inputs widened exactly:
//   dx  = [ differentiatePos(q0 -> qpos_e, dt = 1) ; qvel_e - v0 ]      # 2nv
//   s_a = sum_k K[a, k] dx[k]
//   u_a = u0[a] + feedback_sign * s_a
//   if clip and actuator a is ctrl-limited: u_a = min(max(u_a, lo_a), hi_a)
//   ctrl_e[a] = u_a                                                     # rounded once to the data's dtype
// K, u0, q0, v0 are strided inputs: the block of (t, e) sits at ptr + t * step_stride + e * env_stride (elements, stride 0 = broadcast),
// float32 or float64 per array; v0.p null = zeros.  The sign and quaternion rule of dx are those of mjb_differentiate_pos(qvel_out, 1,
// q0, qpos).  Formulas, statuses and the record: include/mjbatch.h.
//
// Mapping: ONE wavefront per environment, feedback_waves(nu, nv) of them per workgroup and no workgroup barrier - a wave orders its own
// LDS traffic with a wavefront-scope fence.  dx is built once per environment in LDS, lanes over joints (and over dofs for the velocity
// half).  K is the only large operand (nu * 2nv * 8 B: 9 KB per humanoid environment) and is read exactly once, as a flat sweep over
// its nu * nx elements: 16 bytes per lane where the block's address is 16-byte aligned (two float64 or four float32, four such loads in
// flight per lane; the up to three elements behind the last whole vector one per lane), one element per lane otherwise.  Which lane loads an element decides nothing: its
// product K[a, k] * dx[k] is rounded once and goes to LDS at p[a * (nx | 1) + k], and lane a adds row a in the order k = 0 .. nx - 1.
// So an environment's ctrl is bitwise the same at any position of any batch, for any batch size, any alignment of its K block and any
// broadcast layout of the inputs.  No scratch memory, no allocation, no atomics: status[e] is a plain load, OR and store by lane 0 of the
// wave that owns e.  The measured times are in INTEGRATION.md.
//
// The same source compiles in a host emulation (MJB_HOST_EMU: one std::thread per lane, a pthread barrier per wavefront) that only the
// CPU test-suite uses; the product library never contains that build.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef MJB_HOST_EMU
#include <pthread.h>
#define MJB_FB_DEV static inline
#else
#include <hip/hip_runtime.h>
#define MJB_FB_DEV __device__ __forceinline__
#endif

namespace mjb {

// the 16-byte loads of the sweep
#ifdef MJB_HOST_EMU
struct alignas(16) fb_f4 { float x, y, z, w; };
struct alignas(16) fb_d2 { double x, y; };
#else
typedef float4 fb_f4;
typedef double2 fb_d2;
#endif

static const int kFbMaxNv = 64, kFbMaxNu = 32;         // the limits of mjb_lqr_dare
static const int kFbJntFree = 0;                       // mjtJoint: free = 0; slide and hinge are scalar joints
static const int kFbNotFinite = 1, kFbClipped = 2;     // bits of status
static const int kFbLoads = 4;                         // 16-byte loads of the K sweep a lane has in flight at once
static const double kFbDblMax = 1.7976931348623157e308;

struct FbIn { const void* p; long ss, es; int f32; };  // block (t, e) at p + t * ss + e * es, in elements of float (f32) or double

struct FeedbackLawArgs {
  int B, nq, nv, nu, njnt, data_f32, clip, t;
  double sign;                                         // -1: u = u0 - K dx (mjb_lqr_dare, mjb_set_feedback); +1: mjb_lqr_backward
  FbIn K, u0, q0, v0;                                  // [nu, 2nv], [nu], [nq], [nv] per (t, e); v0.p null = zeros
  const void *qpos, *qvel;                             // the data object's [B, nq], [B, nv] (float when data_f32)
  void* ctrl;                                          // the data object's [B, nu]
  const int *jnt_type, *jnt_qposadr, *jnt_dofadr, *ctrllimited;   // [njnt] x 3, [nu]
  const double* ctrlrange;                             // [nu, 2]
  const unsigned char* mask;                           // [B] or null: 0 = the environment is not touched
  int* status;                                         // [B] or null: bits ORed in
  void* u_rec; long ur_ss, ur_es;                      // null, or the record: the ctrl row also goes to u_rec + t * ur_ss + e * ur_es (data's dtype)
};

// ---- host arithmetic of the argument checks (no HIP: tested without a GPU) -----------------------------------------------------------
// 0 ok; otherwise which argument is wrong (the entry points turn it into the message).  nstep: the steps t .. t + nstep - 1 will run.
inline int feedback_arg_error(const FeedbackLawArgs& a, long nstep) {
  if (a.B < 1) return 1;
  if (a.nv < 1 || a.nv > kFbMaxNv) return 2;
  if (a.nu < 1 || a.nu > kFbMaxNu) return 3;
  if (a.nq < a.nv || a.nq > 2 * a.nv || a.njnt < 1 || a.njnt > a.nv) return 4;
  if (!(a.sign == 1.0 || a.sign == -1.0)) return 5;
  if (a.t < 0) return 6;
  if (nstep < 1 || (long)a.t + nstep > (1L << 30)) return 7;
  const FbIn* in[4] = {&a.K, &a.u0, &a.q0, &a.v0};
  for (const FbIn* s : in) if (s->ss < 0 || s->es < 0) return 8;
  if (a.ur_ss < 0 || a.ur_es < 0) return 8;
  if (!a.K.p || !a.u0.p || !a.q0.p) return 9;
  return 0;
}
// wavefronts per workgroup: four where their LDS fits the 64 KiB a launch gets without asking, else two, else one (32 x 64: 34 KB a wave)
inline int feedback_lds_doubles(int nu, int nv) { return (2 * nv + nu * ((2 * nv) | 1) + 32 + 1) & ~1; }    // dx | p | 64 flag words, even
inline int feedback_waves(int nu, int nv) {
  const long bytes = (long)feedback_lds_doubles(nu, nv) * 8;
  return 4 * bytes <= 64 * 1024 ? 4 : 2 * bytes <= 64 * 1024 ? 2 : 1;
}

// ---- wavefront primitives -----------------------------------------------------------------------------------------------------------
#ifdef MJB_HOST_EMU
namespace fbemu {
struct Block {
  pthread_barrier_t bar;
  explicit Block(int n) { pthread_barrier_init(&bar, nullptr, (unsigned)n); }
  ~Block() { pthread_barrier_destroy(&bar); }
};
inline thread_local Block* tl_block = nullptr;
}  // namespace fbemu
static inline void fb_wave_sync() { pthread_barrier_wait(&fbemu::tl_block->bar); }
#else
// DS instructions of a wave execute in issue order: a wavefront-scope fence (a compiler ordering point, no s_barrier) orders the
// wave's own LDS traffic, and the other waves of the workgroup share nothing with it
MJB_FB_DEV void fb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

MJB_FB_DEV double fb_ld(const void* p, long i, int f32) { return f32 ? (double)((const float*)p)[i] : ((const double*)p)[i]; }
MJB_FB_DEV bool fb_finite(double v) { return fabs(v) <= kFbDblMax; }

// res [3] = the rotation from q1 to q2 as a tangent vector (mjb_differentiate_pos with dt = 1).  No contraction into fused
// multiply-adds here: with q2 == q1 every component of the vector part is then exactly 0.
MJB_FB_DEV void fb_quat_diff(double* res, const double* q1, const double* q2) {
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

// one product of the sweep: element i = a * nx + k of the K block
MJB_FB_DEV void fb_product(double kv, int i, int nx, int ldp, const double* dx, double* p, int& bad) {
  const int a = i / nx, k = i - a * nx;
  if (!fb_finite(kv)) bad = 1;
  p[a * ldp + k] = kv * dx[k];
}

// ---- environment e: one wavefront (lane 0 .. 63), w = feedback_lds_doubles(nu, nv) doubles of LDS that no other wave touches ------------
MJB_FB_DEV void feedback_env(const FeedbackLawArgs& a, int e, int lane, double* w) {
  if (a.mask && !a.mask[e]) return;                              // the whole wave: ctrl, status and the record row keep what they hold
  const int nv = a.nv, nq = a.nq, nu = a.nu, nx = 2 * nv, ldp = nx | 1, n = nu * nx;
  double *dx = w, *p = w + nx;
  int* flg = (int*)(p + nu * ldp);
  const long t = a.t;
  const size_t ds = a.data_f32 ? 4 : 8;
  const void* qp = (const char*)a.qpos + (size_t)e * nq * ds;
  const void* qv = (const char*)a.qvel + (size_t)e * nv * ds;
  const void* q0 = (const char*)a.q0.p + (size_t)(t * a.q0.ss + (long)e * a.q0.es) * (a.q0.f32 ? 4 : 8);
  const void* v0 = a.v0.p ? (const char*)a.v0.p + (size_t)(t * a.v0.ss + (long)e * a.v0.es) * (a.v0.f32 ? 4 : 8) : nullptr;
  const void* u0 = (const char*)a.u0.p + (size_t)(t * a.u0.ss + (long)e * a.u0.es) * (a.u0.f32 ? 4 : 8);
  const char* Kb = (const char*)a.K.p + (size_t)(t * a.K.ss + (long)e * a.K.es) * (a.K.f32 ? 4 : 8);
  int bad = 0;

  // dx: lanes over joints for the position half, over dofs for the velocity half
  if (lane < a.njnt) {
    const int qa = a.jnt_qposadr[lane], da = a.jnt_dofadr[lane];
    if (a.jnt_type[lane] == kFbJntFree) {
      double q1[7], q2[7];
      for (int k = 0; k < 7; k++) {
        q1[k] = fb_ld(q0, qa + k, a.q0.f32); q2[k] = fb_ld(qp, qa + k, a.data_f32);
        if (!fb_finite(q1[k]) || !fb_finite(q2[k])) bad = 1;
      }
      for (int k = 0; k < 3; k++) dx[da + k] = q2[k] - q1[k];
      fb_quat_diff(dx + da + 3, q1 + 3, q2 + 3);
    } else {
      const double r = fb_ld(q0, qa, a.q0.f32), q = fb_ld(qp, qa, a.data_f32);
      if (!fb_finite(r) || !fb_finite(q)) bad = 1;
      dx[da] = q - r;
    }
  }
  if (lane < nv) {
    const double v = fb_ld(qv, lane, a.data_f32), r = v0 ? fb_ld(v0, lane, a.v0.f32) : 0.0;
    if (!fb_finite(v) || !fb_finite(r)) bad = 1;
    dx[nv + lane] = v - r;
  }
  fb_wave_sync();

  // the sweep over K: every element once
  if (((uintptr_t)Kb & 15) == 0) {
    if (a.K.f32) {
      const int nvec = n >> 2;
      for (int j0 = lane; j0 < nvec; j0 += 64 * kFbLoads) {        // kFbLoads loads in flight per lane before the first product
        fb_f4 v[kFbLoads];
#pragma unroll
        for (int r = 0; r < kFbLoads; r++) if (j0 + 64 * r < nvec) v[r] = ((const fb_f4*)Kb)[j0 + 64 * r];
#pragma unroll
        for (int r = 0; r < kFbLoads; r++) {
          const int j = j0 + 64 * r;
          if (j >= nvec) break;
          fb_product((double)v[r].x, 4 * j, nx, ldp, dx, p, bad); fb_product((double)v[r].y, 4 * j + 1, nx, ldp, dx, p, bad);
          fb_product((double)v[r].z, 4 * j + 2, nx, ldp, dx, p, bad); fb_product((double)v[r].w, 4 * j + 3, nx, ldp, dx, p, bad);
        }
      }
      const int i = 4 * nvec + lane;
      if (lane < 3 && i < n) fb_product((double)((const float*)Kb)[i], i, nx, ldp, dx, p, bad);
    } else {
      const int nvec = n >> 1;
      for (int j0 = lane; j0 < nvec; j0 += 64 * kFbLoads) {
        fb_d2 v[kFbLoads];
#pragma unroll
        for (int r = 0; r < kFbLoads; r++) if (j0 + 64 * r < nvec) v[r] = ((const fb_d2*)Kb)[j0 + 64 * r];
#pragma unroll
        for (int r = 0; r < kFbLoads; r++) {
          const int j = j0 + 64 * r;
          if (j >= nvec) break;
          fb_product(v[r].x, 2 * j, nx, ldp, dx, p, bad); fb_product(v[r].y, 2 * j + 1, nx, ldp, dx, p, bad);
        }
      }
      const int i = 2 * nvec + lane;
      if (lane < 1 && i < n) fb_product(((const double*)Kb)[i], i, nx, ldp, dx, p, bad);
    }
  } else {
    for (int i = lane; i < n; i += 64) fb_product(fb_ld(Kb, i, a.K.f32), i, nx, ldp, dx, p, bad);
  }
  fb_wave_sync();

  // row a on lane a, k ascending; the clip; what the wave has to report
  double u = 0.0;
  int clipped = 0;
  if (lane < nu) {
    const double* row = p + lane * ldp;
    double s = 0.0;
    for (int k = 0; k < nx; k++) s += row[k];
    const double ub = fb_ld(u0, lane, a.u0.f32);
    u = ub + a.sign * s;
    if (!fb_finite(ub) || !fb_finite(u)) bad = 1;
    if (a.clip && a.ctrllimited[lane]) {
      const double lo = a.ctrlrange[2 * lane], hi = a.ctrlrange[2 * lane + 1];
      if (u < lo) { u = lo; clipped = 1; }
      if (u > hi) { u = hi; clipped = 1; }
    }
  }
  flg[lane] = bad | (clipped << 1);
  fb_wave_sync();
  int any = 0;
  for (int l = 0; l < 64; l++) any |= flg[l];
  const int bits = (any & 1) ? kFbNotFinite : (any & 2) ? kFbClipped : 0;  // a step that is not finite has no clip to report
  if (bits & kFbNotFinite) u = 0.0;                              // zeros for the whole environment: a bad law is not applied
  if (lane < nu) {
    if (a.data_f32) ((float*)a.ctrl)[(size_t)e * nu + lane] = (float)u; else ((double*)a.ctrl)[(size_t)e * nu + lane] = u;
    if (a.u_rec) {
      const size_t o = (size_t)(t * a.ur_ss + (long)e * a.ur_es) + lane;
      if (a.data_f32) ((float*)a.u_rec)[o] = (float)u; else ((double*)a.u_rec)[o] = u;
    }
  }
  if (lane == 0 && a.status && bits) a.status[e] = a.status[e] | bits;
}

#ifndef MJB_HOST_EMU
// enqueue only (mjb_feedback.hip); the entry points (mjb_api.hip) have checked every pointer and extent
hipError_t feedback_launch(const FeedbackLawArgs& p, hipStream_t stream);
#endif

}  // namespace mjb
