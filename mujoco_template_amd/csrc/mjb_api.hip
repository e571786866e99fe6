// mjb_api.hip — host side of the C ABI declared in include/mjbatch.h.
// Owns device memory (SoA [batch, dof] state in HBM, model constants), launches the
// kernels of mjb_kernels.hpp on the caller's HIP stream.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/mjbatch.h"
#include "mjb_buffer.hpp"
#include "mjb_host.hpp"
#include "mjb_kernels.hpp"
#include "mjb_lqr.hpp"
#include "mjb_dare.hpp"
#include "mjb_eig.hpp"
#include "mjb_dlyap.hpp"
#include "mjb_setpoint.hpp"
#include "mjb_traj.hpp"
#include "mjb_feedback.hpp"

using namespace mjb;

namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(expr)                                                                                           \
  do {                                                                                                         \
    hipError_t e_ = (expr);                                                                                    \
    if (e_ != hipSuccess) return fail(MJB_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

struct DevAlloc {                                           // the model tables of fill_dev_model as blocks of the data object's arena
  Arena& arena;
  template <typename X> const X* put(const std::vector<X>& v) {
    X* p = arena.alloc<X>(v.size());
    if (p && v.size() && hipMemcpy(p, v.data(), v.size() * sizeof(X), hipMemcpyHostToDevice) != hipSuccess) arena.ok = false;
    return p;
  }
  const float* putf(const std::vector<float>& v) { return put(v); }
  const double* putf(const std::vector<double>& v) { return put(v); }
  const int* puti(const std::vector<int>& v) { return put(v); }
  const unsigned long long* putu(const std::vector<unsigned long long>& v) { return put(v); }
};
// every block of a group that is allocated together: a failed call leaves the whole group empty, and the next call allocates again
template <typename... B> void reset_all(B&... b) { (b.reset(), ...); }
// the zero fill dev_alloc (below) gives an arena block, for a Buffer that has just been made or has grown
template <typename X> hipError_t reserve_zeroed(Buffer<X>& b, size_t n) {
  if (n <= b.count()) return hipSuccess;
  hipError_t e = b.reserve(n);
  if (e == hipSuccess && b.kind() != Mem::Device) std::memset(b.get(), 0, n * sizeof(X));
  else if (e == hipSuccess && (e = hipMemset(b.get(), 0, n * sizeof(X))) != hipSuccess) b.reset();
  return e;
}

struct ArrayInfo { void* ptr; long per_env; int kind; };  // kind: 0 = data dtype, 1 = float64, 2 = int32, 3 = uint32 (int32 to mjb_array_ptr, widened by mjb_get_array)
}  // namespace

struct mjbModel {
  HostModel h;
  int disableactuator;
  int iterations;
  double tolerance;
  std::vector<char> blob;                                   // the table this model was created from, serialised (mjb_model_save / mjb_model_field)
  struct Field { std::string name; int dtype; long count; size_t off; };
  std::vector<Field> fields;
  std::map<int, std::vector<std::string>> names;            // object names by mjtObj code (table fields "names_<code>", dtype 2)
};

struct mjbObsSpec {
  ObsSpecDev dev;
  Arena arena;                                              // the id tables dev points at
};

// Launch configuration of a data object (derive_config): lane-group widths, caps on contacts / constraint rows, LDS layouts
struct Config {
  int G, G_fd, ncon_max, nefc_max;        // G: lanes per environment of the step kernel; G_fd: of the float64 FD / Jacobian kernels
  Lay Lf, Ld;                             // fp32 / float64 layouts of one environment's LDS slice
  Lay Lf2;                                // flat fp32 layout of the two-wave step kernel (k_step2); bytes == 0: that kernel does not apply
};

struct mjbData {
  mjbModel* model;
  int batch, dtype, device, env0;
  Config cfg;
  hipStream_t stream;
  Arena arena;                          // blocks of the object's whole life: model tables, descriptors, state and debug arrays
  DevModel<float> mf;
  DevModel<double> md;
  DevModel<float>* mf_dev = nullptr;    // device copies of the structs above and of the layouts (read through the constant address space)
  DevModel<double>* md_dev = nullptr;
  Lay *Lf_dev = nullptr, *Ld_dev = nullptr, *Lf2_dev = nullptr;
  // per-model specialised kernels (mjb_kernel_load), indexed by MJB_KERNEL_*; a null function = the generic kernel
  struct { hipModule_t mod; hipFunction_t fn; } spec[4] = {};
  int ncu = 0;                              // CUs of the device (queried once, by mjb_data_create)
  int two_wave = -1;                        // MJB_TWO_WAVE: 0 never, 1 whenever it applies, -1 (default) the policy in launch()
  int up_disable = -1, up_iter = -1; double up_tol = -1;
  DevData<float> df;
  DevData<double> dd;
  std::map<std::string, ArrayInfo> arrays;
  // debug dumps
  bool dbg_ready = false;
  DevDebug<float> dbgf;
  DevDebug<double> dbgd;
  std::map<std::string, ArrayInfo> dbg_arrays;
  // device-side feedback controller gains (float and double copies): K [nu, 2nv], u0 [nu], q0 [nq], v0 [nv]
  Buffer<float> fbf[4];
  Buffer<double> fbd[4];
  // work scheduling of k_step (launch()): resident workgroups of the kernel in use on this device; < 0 = not yet queried
  long step_slots = -1;
  int sched_chunk = -1, fair_bit = -1;     // experiment overrides (MJB_CHUNK_STEPS, MJB_FAIR_BIT); -1 = policy below
  unsigned launch_seq = 0;                 // ticket launches so far (tags of the hand-over buffer)
  unsigned long long ticket_next = 0;      // value of the device ticket counter when the next ticket launch starts
  int last_sched[6] = {0, 0, 0, 0, 0, 0};  // of the last mode-0 launch: steps, environment blocks, resident slots, chunk_steps, fair_bit, two waves per environment
  // fd / jac scratch
  Buffer<double> fd_y, fd_A, fd_B; Buffer<int> fd_valid;       // fd_y / fd_valid: per-column scratch (fd_scratch), grown on demand
  hipEvent_t fd_done = nullptr;                                // recorded behind the last FD launch: a call on ANOTHER stream waits for it before it reuses the scratch
  hipStream_t fd_stream = nullptr; bool fd_pending = false;
  int last_fd_slabs = 0;                                       // slabs of the last mjb_transition_fd_points (mjb_fd_points_slabs)
  Buffer<double> fd_A_host{Mem::Pinned}, fd_B_host{Mem::Pinned};   // the (A, B) blocks leave the device in one async copy each
  // the sensor half (mjb_transition_fd_sensors / _points_sensors), made by the first call that asks for it: fd_s [npoint, ncol, ns] = the
  // per-column sensordata beside fd_y, (C, D) result blocks as (A, B)
  Buffer<double> fd_s, fd_C, fd_D, fd_C_host{Mem::Pinned}, fd_D_host{Mem::Pinned};
  bool spec_fd_sensors = false;                                // the loaded MJB_KERNEL_FD code object knows FdPoints::sens_out (mjb_kernel_load)
  // mjb_jac: persistent buffers (grown on demand) - the request (kinds | ids) in pinned memory the kernel reads directly, the result
  // blocks pinned (small requests: written by the kernel itself) and on the device (large requests: one async copy each)
  Buffer<unsigned char> io_pin{Mem::Pinned};                   // pinned staging of mjb_get_array / mjb_set_array (grown on demand, with slack)
  Buffer<int> jac_req_pin{Mem::Pinned};
  Buffer<double> jac_pin[2] = {Buffer<double>(Mem::Pinned), Buffer<double>(Mem::Pinned)}, jac_dev[2];
  // standalone feedback law (mjb_feedback_ctrl): optional noise (std [nu], table [nsteps, nu]) in both precisions, dx scratch for float64
  Buffer<float> fb_noise_f[2];
  Buffer<double> fb_noise_d[2], fb_dx;
  int fb_nsteps = 0, fb_env_stride = 0;
  // host mirror (mjb_host_view): ONE pinned float64 block  qpos | qvel | ctrl | qacc | qacc_warmstart | time , each [batch, n],
  // and its device staging twin; filled by one pack kernel + one D2H per mjb_sync_to_host
  Buffer<double> mirror_host{Mem::PinnedCoherent}, mirror_dev;
  std::vector<double> mirror_shadow;      // host copy of the block as last refreshed / uploaded: what in-place edits are detected against
  unsigned long long mirror_seq = 0;      // sequence number of the last polled host-driven step (completion words behind the flags word)
  size_t mirror_off[7] = {0, 0, 0, 0, 0, 0, 0};             // element offsets of the six fields, [6] = total
  Buffer<int> flags_pin{Mem::Pinned};     // the four engine-flag bits as words the kernels set (DevData::flags_pin)
  Buffer<unsigned> episode;               // [batch] resets per environment by mjb_reset_envs (the episode counter of its noise streams)
  Buffer<unsigned long long> xfer;        // hand-over buffer of the ticket map (DevData<float>::xfer), made by the first launch that needs it
  unsigned xfer_timeout = 0;             // ticks of the 100 MHz clock a wave waits for a hand-over (0 = not yet read from MJB_XFER_TIMEOUT_MS)
  int xfer_poison_env = -1;               // test hook MJB_XFER_POISON_ENV (-1 = not yet read)
  // per-environment model parameters (mjb_set_env_param): rows of slot k (PRM_*, mjb_types.hpp) in float64 and, for float32 data, fp32;
  // the same pointers sit in df.prm / dd.prm, which the kernels receive (prm_publish)
  Buffer<double> prm_d[PRM_NSLOT];
  Buffer<float> prm_f[PRM_NSLOT];
  int prm_mask = 0;                       // bit k = field k batched
  int spec_prm[4] = {0, 0, 0, 0};         // the batched fields each loaded specialised kernel was built for
  Buffer<double> prm_stage;               // device staging of host-memory sources (float64)
};

namespace {
// ---- serialised model table: "MJBM0001", int32 nfield, then per field: int32 name length, name, int32 dtype (0 f64, 1 i32,
// 2 bytes), int64 count, payload padded to 8 bytes.  Written by mjb_model_save, read by mjb_model_load; also what
// mjb_model_field serves pointers into. ----
size_t elem_size(int dtype) { return dtype == 0 ? 8 : (dtype == 1 ? 4 : 1); }
bool keep_table(mjbModel* m, const Table& t, std::string& err) {
  std::vector<char>& b = m->blob;
  b.clear(); m->fields.clear(); m->names.clear();
  auto put = [&](const void* p, size_t n) { const char* c = (const char*)p; b.insert(b.end(), c, c + n); };
  put("MJBM0001", 8);
  int32_t nf = t.n; put(&nf, 4);
  for (int i = 0; i < t.n; i++) {
    if (t.dtypes[i] < 0 || t.dtypes[i] > 2 || t.counts[i] < 0) { err = std::string("model field '") + t.names[i] + "': bad dtype/count"; return false; }
    int32_t nl = (int32_t)std::strlen(t.names[i]), dt = t.dtypes[i]; int64_t cnt = t.counts[i];
    put(&nl, 4); put(t.names[i], nl); put(&dt, 4); put(&cnt, 8);
    while (b.size() % 8) b.push_back(0);
    size_t off = b.size(), nb = (size_t)cnt * elem_size(dt);
    if (nb) put(t.ptrs[i], nb);
    while (b.size() % 8) b.push_back(0);
    m->fields.push_back({t.names[i], dt, (long)cnt, off});
    if (dt == 2 && !std::strncmp(t.names[i], "names_", 6)) {           // NUL-terminated names of one object type, in id order
      std::vector<std::string>& v = m->names[std::atoi(t.names[i] + 6)];
      const char* c = (const char*)t.ptrs[i];
      for (long k = 0; k < cnt;) { size_t l = strnlen(c + k, (size_t)(cnt - k)); v.emplace_back(c + k, l); k += (long)l + 1; }
    }
  }
  return true;
}
// parse a blob back into a Table (pointers into `b`)
bool parse_blob(const std::vector<char>& b, std::vector<std::string>& names, std::vector<const void*>& ptrs, std::vector<int>& dts, std::vector<long>& cnts, std::string& err) {
  size_t o = 0;
  auto need = [&](size_t n) { return o + n <= b.size(); };
  if (!need(12) || std::memcmp(b.data(), "MJBM0001", 8)) { err = "not a mjbatch model file (bad magic)"; return false; }
  int32_t nf; std::memcpy(&nf, b.data() + 8, 4); o = 12;
  if (nf < 0 || nf > 100000) { err = "corrupt model file (field count)"; return false; }
  for (int i = 0; i < nf; i++) {
    int32_t nl, dt; int64_t cnt;
    if (!need(4)) { err = "truncated model file"; return false; }
    std::memcpy(&nl, b.data() + o, 4); o += 4;
    if (nl < 0 || nl > 256 || !need((size_t)nl + 12)) { err = "corrupt model file (field name)"; return false; }
    names.emplace_back(b.data() + o, (size_t)nl); o += nl;
    std::memcpy(&dt, b.data() + o, 4); o += 4; std::memcpy(&cnt, b.data() + o, 8); o += 8;
    if (dt < 0 || dt > 2 || cnt < 0) { err = "corrupt model file (dtype/count)"; return false; }
    o = (o + 7) / 8 * 8;
    // count is checked against what is left of the file BEFORE it is multiplied: a crafted int64 count must not wrap the byte size
    if (o > b.size() || (uint64_t)cnt > (uint64_t)(b.size() - o) / elem_size(dt)) { err = "truncated model file"; return false; }
    size_t nb = (size_t)cnt * elem_size(dt);
    ptrs.push_back(b.data() + o); dts.push_back(dt); cnts.push_back((long)cnt);
    o = (o + nb + 7) / 8 * 8;
  }
  return true;
}

// the joints of one environment on the host, float64 (mj_integratePos / mj_differentiatePos act on caller-owned host vectors)
void h_quat_mul(double* r, const double* a, const double* b) {
  double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  double y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}

template <typename X> int dev_alloc(mjbData* d, X** out, size_t n) {
  if (n == 0) n = 1;
  *out = d->arena.alloc<X>(n);
  return *out && hipMemset(*out, 0, n * sizeof(X)) == hipSuccess ? 0 : -1;
}

template <typename TS> int alloc_state(mjbData* d, DevData<TS>& s) {
  const HostModel& h = d->model->h;
  size_t B = (size_t)d->batch;
  s.batch = d->batch;
  int rc = 0;
  rc |= dev_alloc(d, &s.qpos, B * h.nq); rc |= dev_alloc(d, &s.qvel, B * h.nv); rc |= dev_alloc(d, &s.ctrl, B * h.nu);
  rc |= dev_alloc(d, &s.qacc, B * h.nv); rc |= dev_alloc(d, &s.qacc_warmstart, B * h.nv); rc |= dev_alloc(d, &s.time, B);
  rc |= dev_alloc(d, &s.xpos, B * h.nbody * 3); rc |= dev_alloc(d, &s.xquat, B * h.nbody * 4); rc |= dev_alloc(d, &s.xipos, B * h.nbody * 3);
  rc |= dev_alloc(d, &s.site_xpos, B * h.nsite * 3); rc |= dev_alloc(d, &s.geom_xpos, B * h.ngeom * 3);
  rc |= dev_alloc(d, &s.subtree_com, B * h.nbody * 3); rc |= dev_alloc(d, &s.sensordata, B * h.nsensordata);
  rc |= dev_alloc(d, &s.qfrc_inverse, B * h.nv); rc |= dev_alloc(d, &s.actuator_moment, B * h.nu * h.nv);
  rc |= dev_alloc(d, &s.counters, B * CNT_N); rc |= dev_alloc(d, &s.flags, 1);
  rc |= dev_alloc(d, &s.sched, 1);
  if (reserve_zeroed(d->flags_pin, 4) != hipSuccess) return -1;   // the engine flags as four words of pinned host memory (raise_engine_flags)
  s.flags_pin = d->flags_pin.get();
  s.xfer = nullptr;                                             // hand-over buffer of the ticket map: allocated by the first launch that needs it
  rc |= dev_alloc(d, &s.prof, (size_t)PH_N + 4 * B);        // + per-environment timeline records of the -DMJB_TIMELINE diagnostic kernel
  if (rc) return -1;
  auto& A = d->arrays;
  A["qpos"] = {s.qpos, h.nq, 0}; A["qvel"] = {s.qvel, h.nv, 0}; A["ctrl"] = {s.ctrl, h.nu, 0}; A["qacc"] = {s.qacc, h.nv, 0};
  A["qacc_warmstart"] = {s.qacc_warmstart, h.nv, 0}; A["time"] = {s.time, 1, 1};
  A["xpos"] = {s.xpos, h.nbody * 3L, 0}; A["xquat"] = {s.xquat, h.nbody * 4L, 0}; A["xipos"] = {s.xipos, h.nbody * 3L, 0};
  A["site_xpos"] = {s.site_xpos, h.nsite * 3L, 0}; A["geom_xpos"] = {s.geom_xpos, h.ngeom * 3L, 0};
  A["subtree_com"] = {s.subtree_com, h.nbody * 3L, 0}; A["sensordata"] = {s.sensordata, h.nsensordata, 0};
  A["qfrc_inverse"] = {s.qfrc_inverse, h.nv, 0}; A["actuator_moment"] = {s.actuator_moment, (long)h.nu * h.nv, 0};
  A["counters"] = {s.counters, CNT_N, 2};
  if (reserve_zeroed(d->episode, B) != hipSuccess) return -1;
  A["episode"] = {d->episode.get(), 1, 3};
  return 0;
}

template <typename TS> int alloc_debug(mjbData* d, DevDebug<TS>& g) {
  const HostModel& h = d->model->h;
  size_t B = (size_t)d->batch, nv = h.nv, ne = d->cfg.nefc_max, nc = d->cfg.ncon_max;
  int rc = 0;
  rc |= dev_alloc(d, &g.qM, B * nv * nv); rc |= dev_alloc(d, &g.qfrc_bias, B * nv); rc |= dev_alloc(d, &g.qfrc_passive, B * nv);
  rc |= dev_alloc(d, &g.qfrc_actuator, B * nv); rc |= dev_alloc(d, &g.qacc_smooth, B * nv); rc |= dev_alloc(d, &g.qfrc_constraint, B * nv);
  rc |= dev_alloc(d, &g.efc_J, B * ne * nv); rc |= dev_alloc(d, &g.efc_aref, B * ne); rc |= dev_alloc(d, &g.efc_D, B * ne);
  rc |= dev_alloc(d, &g.efc_pos, B * ne); rc |= dev_alloc(d, &g.efc_force, B * ne); rc |= dev_alloc(d, &g.con, B * nc * CON_STRIDE);
  rc |= dev_alloc(d, &g.cdof, B * 6 * nv); rc |= dev_alloc(d, &g.cinert, B * 10 * h.nbody); rc |= dev_alloc(d, &g.cvel, B * 6 * h.nbody);
  rc |= dev_alloc(d, &g.efc_type, B * ne);
  if (rc) return -1;
  auto& A = d->dbg_arrays;
  A["qM"] = {g.qM, (long)(nv * nv), 0}; A["qfrc_bias"] = {g.qfrc_bias, (long)nv, 0}; A["qfrc_passive"] = {g.qfrc_passive, (long)nv, 0};
  A["qfrc_actuator"] = {g.qfrc_actuator, (long)nv, 0}; A["qacc_smooth"] = {g.qacc_smooth, (long)nv, 0}; A["qfrc_constraint"] = {g.qfrc_constraint, (long)nv, 0};
  A["efc_J"] = {g.efc_J, (long)(ne * nv), 0}; A["efc_aref"] = {g.efc_aref, (long)ne, 0}; A["efc_D"] = {g.efc_D, (long)ne, 0};
  A["efc_pos"] = {g.efc_pos, (long)ne, 0}; A["efc_force"] = {g.efc_force, (long)ne, 0}; A["con"] = {g.con, (long)(nc * CON_STRIDE), 0};
  A["cdof"] = {g.cdof, (long)(6 * nv), 0}; A["cinert"] = {g.cinert, 10L * h.nbody, 0}; A["cvel"] = {g.cvel, 6L * h.nbody, 0};
  A["efc_type"] = {g.efc_type, (long)ne, 2};
  return 0;
}

int refresh_options(mjbData* d) {
  const mjbModel* mm = d->model;
  if (d->up_disable == mm->disableactuator && d->up_iter == mm->iterations && d->up_tol == mm->tolerance) return MJB_OK;
  d->mf.disableactuator = d->md.disableactuator = mm->disableactuator;
  d->mf.iterations = d->md.iterations = mm->iterations;
  d->md.tolerance = mm->tolerance;
  // fp32 floor of the solver tolerance: 1e-7 / 1e-8 were measured (profiles/r02_humanoid_phase_errors.log): +0.6 / +0.8 Newton
  // iterations per step, -3 % / -4.5 % throughput, no change of the humanoid drift curve (the error enters through M and the bias force)
  float tol = (float)mm->tolerance;
  d->mf.tolerance = tol < 1e-6f ? 1e-6f : tol;
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(d->mf_dev, &d->mf, sizeof(d->mf), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d->md_dev, &d->md, sizeof(d->md), hipMemcpyHostToDevice));
  d->up_disable = mm->disableactuator; d->up_iter = mm->iterations; d->up_tol = mm->tolerance;
  return MJB_OK;
}


// Caps on contacts / constraint rows held in LDS per environment.  Explicit values are taken as given.  Default: the model's own
// worst case when that is small (<= 96 rows, <= 32 contacts); otherwise the largest (rows <= 96, contacts = 3/8 rows) that still
// lets 8 fp32 (4 fp64) wavefronts share one CU's 160 KiB — the occupancy step that matters most for throughput (profiles/).
// Overflow drops rows and is COUNTED.
void choose_caps(const HostModel& h, int dtype, int lanes, int nconmax, int nefcmax, int& nc_out, int& ne_out) {
  int ne, nc;
  if (nconmax > 0 || nefcmax > 0) {
    nc = nconmax > 0 ? nconmax : (h.ncon_alloc < 32 ? h.ncon_alloc : 32);
    ne = nefcmax > 0 ? nefcmax : (h.nefc_alloc < 96 ? h.nefc_alloc : 96);
  } else {
    const size_t budget = (size_t)160 * 1024 / (dtype == MJB_F32 ? 8 : 4);
    ne = h.nefc_alloc < 96 ? h.nefc_alloc : 96; nc = 0;
    if (h.nefc_alloc <= 96 && h.ncon_alloc <= 32) {
      // the model's own worst case (every candidate pair in contact, every limit active) is small: hold all of it, nothing
      // can ever be dropped (drone2: 20 contacts / 80+ rows when it lands flat); occupancy is not traded against that
      ne = h.nefc_alloc; nc = h.ncon_alloc;
    } else for (;; ne -= 8) {
      // rows bind first (a frictional contact is four rows): for each row cap try 3/8 of it as contact cap and shave that down to a
      // third before giving up rows (humanoid fp32: 64 rows / 23 contacts = 20 448 B, eight slices in 160 KB; 64 / 24 misses by 16 B)
      int hi = ne * 3 / 8; if (hi < 8) hi = 8; if (hi > h.ncon_alloc) hi = h.ncon_alloc;
      int lo = ne / 3; if (lo < 8) lo = 8; if (lo > hi) lo = hi;
      bool fits = false;
      for (nc = hi; nc >= lo; nc--) {
        Lay t = make_layout(h, nc > 0 ? nc : 1, ne > 0 ? ne : 1, dtype == MJB_F32 ? sizeof(float) : sizeof(double));
        if ((size_t)(64 / lanes) * (size_t)t.bytes <= budget) { fits = true; break; }
      }
      if (fits) break;
      if (ne <= 32) { nc = hi; break; }
    }
  }
  if (nc < 1) nc = 1;
  if (ne < 1) ne = 1;
  nc_out = nc; ne_out = ne;
}
int auto_lanes(const HostModel& h, int lanes) { return lanes == 0 ? (h.nv <= 4 ? 8 : (h.nv <= 16 ? 16 : 64)) : lanes; }

// The launch configuration of a data object of model h created with these arguments: mjb_data_create keeps it, and the model-level
// kernel sources derive it here too, so a kernel built from the model alone is the one a data object later asks for.
bool derive_config(const HostModel& h, int dtype, int lanes, int nconmax, int nefcmax, Config& c, std::string& err) {
  c.G = auto_lanes(h, lanes);
  if (c.G != 8 && c.G != 16 && c.G != 64) { err = "lanes must be 8, 16 or 64"; return false; }
  choose_caps(h, dtype, c.G, nconmax, nefcmax, c.ncon_max, c.nefc_max);
  c.Lf = make_layout(h, c.ncon_max, c.nefc_max, sizeof(float));
  c.Ld = make_layout(h, c.ncon_max, c.nefc_max, sizeof(double));
  // the float64 FD / Jacobian kernels may need more lanes per environment than the step kernel to fit LDS
  c.G_fd = c.G;
  while (c.G_fd < 64 && (size_t)(64 / c.G_fd) * (size_t)c.Ld.bytes > 160 * 1024) c.G_fd = c.G_fd == 8 ? 16 : 64;
  const size_t lds = (size_t)(64 / c.G) * (size_t)(dtype == MJB_F32 ? c.Lf.bytes : c.Ld.bytes);
  if (lds > 160 * 1024 || (size_t)(64 / c.G_fd) * (size_t)c.Ld.bytes > 160 * 1024) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "per-workgroup LDS %zu B exceeds 160 KiB (lower nconmax/nefcmax or use more lanes)", lds);
    err = buf;
    return false;
  }
  std::memset(&c.Lf2, 0, sizeof(Lay));
  if (dtype == MJB_F32 && c.G == 64 && h.nv <= 32 && h.integrator != INT_RK4) {
    c.Lf2 = make_layout(h, c.ncon_max, c.nefc_max, sizeof(float), true);
    if ((size_t)c.Lf2.bytes > 64 * 1024) std::memset(&c.Lf2, 0, sizeof(Lay));       // (never for the models this path is for)
  }
  return true;
}

// The per-model specialised kernels, indexed by MJB_KERNEL_*: the kernel's symbol in its code object, the first line of its generated
// source (it names the entry points of an earlier ABI: kept as it is, because the source text keys the in-tree cache of code objects),
// and why it may not apply to a configuration
struct KernelKind { const char* symbol; const char* banner; const char* not_applicable; };
const KernelKind kKinds[4] = {
    {nullptr, nullptr, nullptr},
    {"mjb_k_step_spec", "// generated by mjb_model_spec_source(): size- and layout-specialised k_step<float, float, G> of ONE compiled model\n",
     "only the float32 step kernel is specialised"},
    {"mjb_k_fd_spec", "// generated by mjb_fd_spec_source(): size- and layout-specialised k_fd<double, TS, G> of ONE compiled model\n", ""},
    {"mjb_k_step2_spec", "// generated by mjb_step2_spec_source(): size- and (flat) layout-specialised two-wave step kernel k_step2<float, float> of ONE compiled model\n",
     "the two-wave step kernel does not apply to this configuration (fp32, one wave per environment, nv <= 32, Euler)"},
};
bool valid_kind(int kind) { return kind == MJB_KERNEL_STEP || kind == MJB_KERNEL_FD || kind == MJB_KERNEL_STEP2; }

// What a kernel kind is built for under configuration c: its LDS layout, lanes per environment, the state type TS of the data object
struct KernelTarget { const Lay* L; int G; const char* ts; bool applies; };
KernelTarget kernel_target(const Config& c, int dtype, int kind) {
  switch (kind) {
    case MJB_KERNEL_STEP: return {&c.Lf, c.G, "float", dtype == MJB_F32};
    case MJB_KERNEL_FD: return {&c.Ld, c.G_fd, dtype == MJB_F32 ? "float" : "double", true};
    default: return {&c.Lf2, 64, "float", c.Lf2.bytes > 0};                              // MJB_KERNEL_STEP2
  }
}
int check_kind(const Config& c, int dtype, int kind) {
  if (!valid_kind(kind)) return fail(MJB_ERR_ARG, "unknown kernel kind (MJB_KERNEL_STEP, MJB_KERNEL_FD or MJB_KERNEL_STEP2)");
  if (!kernel_target(c, dtype, kind).applies) return fail(MJB_ERR_ARG, kKinds[kind].not_applicable);
  return MJB_OK;
}

// The model itself as `__constant__` data of the specialised translation unit (MJB_SPEC_BAKED, mjb_device.hpp): fill_dev_model runs
// against an allocator that EMITS every table as a C array and hands out recognisable tokens instead of addresses; the filled
// DevModel<float> is then written out word by word as a struct of the same layout (pointer words -> the emitted arrays, everything
// else -> the bit pattern), so the image cannot fall out of step with fill_dev_model or with the struct's member list.
struct EmitAlloc {
  // One `static const __constant__` array per table - its own symbol, so a lane-indexed read is global_load(table address + lane
  // offset) with no further address arithmetic.  Measured (scripts/gpu_spec_check.py, same box, B = 4096, M env-steps/s; pointer
  // hops / one struct of all tables / arrays): humanoid 41.7 / 43.1 / 43.4, drone2 178 / 193 / 218, cart-pole 215 / 230 / 248.  The
  // humanoid kernel (256 VGPRs) spills 61 VGPRs to scratch with the array form (spill stores around the ticket loop, ~7 KB per
  // environment and chunk switch: HBM write traffic 0.15 -> 1.2 GB per 1000-step launch) and far fewer with the struct form; it is
  // still 2 % faster with the arrays (4 % on the two-wave kernel).  The struct form is at commit a705124.
  // Tables of records (stride S > 1, at least two records): the columns whose value is bitwise the same in every record become
  // constants of the translation unit (mjb::UniformCols, mjb_types.hpp) - most solref / solimp / margin / range columns of a real
  // model are defaults, and LLVM folds `tab[S * i + k]` only when the WHOLE table is one value.  Compared as emitted (after
  // fill_dev_model's casts and clamps), bit for bit: +0.0 and -0.0 differ, a NaN column is never uniform.
  struct Cols { int stride = 1; unsigned long long mask = 0; const char* ctype = ""; std::vector<std::string> val; };
  std::string text;
  std::vector<Cols> cols;                                    // one per table, in emission order
  int n = 0;
  static constexpr unsigned long long TOKEN = 0x7E57AB1Eull << 32;
  template <typename X, typename F> const X* emit(const std::vector<X>& v, const char* ctype, int stride, F fmt) {
    std::string body;
    if (v.empty()) body = "0";
    for (size_t i = 0; i < v.size(); i++) { if (i) body += (i % 16 == 0 ? ",\n " : ","); body += fmt(v[i]); }
    text += std::string("static const __constant__ ") + ctype + " mjb_tab_" + std::to_string(n) + "[] = {" + body + "};\n";
    Cols c;
    c.ctype = ctype;
    const size_t S = stride > 1 ? (size_t)stride : 1;
    if (S > 1 && S <= 64 && v.size() % S == 0 && v.size() >= 2 * S) {
      c.stride = (int)S;
      c.val.assign(S, "0");
      for (size_t k = 0; k < S; k++) {
        bool same = v[k] == v[k];                            // false for a NaN
        for (size_t r = 1; r * S < v.size() && same; r++) same = std::memcmp(&v[r * S + k], &v[k], sizeof(X)) == 0;
        if (same) { c.mask |= 1ull << k; c.val[k] = fmt(v[k]); }
      }
    }
    cols.push_back(c);
    return (const X*)(uintptr_t)(TOKEN + (unsigned long long)(n++) * 16ull + 16ull);
  }
  const float* putf(const std::vector<float>& v, int stride = 1) {
    return emit(v, "float", stride, [](float x) {
      if (std::isnan(x)) return std::string("__builtin_nanf(\"\")");
      if (std::isinf(x)) return std::string(x > 0 ? "__builtin_inff()" : "-__builtin_inff()");
      char b[48]; std::snprintf(b, sizeof(b), "%af", (double)x); return std::string(b);             // hex float: exact
    });
  }
  const double* putf(const std::vector<double>& v, int stride = 1) {
    return emit(v, "double", stride, [](double x) {
      if (std::isnan(x)) return std::string("__builtin_nan(\"\")");
      if (std::isinf(x)) return std::string(x > 0 ? "__builtin_inf()" : "-__builtin_inf()");
      char b[48]; std::snprintf(b, sizeof(b), "%a", x); return std::string(b);
    });
  }
  const int* puti(const std::vector<int>& v, int stride = 1) { return emit(v, "int", stride, [](int x) { return std::to_string(x); }); }
  const unsigned long long* putu(const std::vector<unsigned long long>& v, int stride = 1) {
    return emit(v, "unsigned long long", stride, [](unsigned long long x) { char b[40]; std::snprintf(b, sizeof(b), "0x%llxull", x); return std::string(b); });
  }
};

template <typename T>
std::string baked_model_source(const HostModel& h, int ncon_max, int nefc_max, int prm_mask) {
  static_assert(sizeof(DevModel<T>) % 8 == 0, "DevModel<T> is written out in 8-byte words");
  const char* tname = sizeof(T) == 4 ? "float" : "double";
  EmitAlloc ea;
  DevModel<T> m;
  fill_dev_model<T>(h, ea, ncon_max, nefc_max, m);
  const size_t nw = sizeof(m) / 8;
  std::vector<unsigned long long> wv(nw);
  std::memcpy(wv.data(), (const void*)&m, sizeof(m));
  std::string decl = "struct MjbBakedModel {", init = "static const __constant__ MjbBakedModel mjb_baked_model = {";
  for (size_t i = 0; i < nw; i++) {
    const unsigned long long v = wv[i];
    if ((v >> 32) == (EmitAlloc::TOKEN >> 32)) {
      decl += " const void MJB_CONST* p" + std::to_string(i) + ";";
      init += " (const void MJB_CONST*)mjb_tab_" + std::to_string((int)((v - EmitAlloc::TOKEN) / 16 - 1)) + ",";
    } else {
      char b[64];
      decl += " unsigned a" + std::to_string(i) + ", b" + std::to_string(i) + ";";
      std::snprintf(b, sizeof(b), " 0x%xu, 0x%xu,", (unsigned)(v & 0xffffffffull), (unsigned)(v >> 32));
      init += b;
    }
    if (i % 8 == 7) init += "\n ";
  }
  decl += " };\n"; init += " };\n";
  {
    // every emitted table must be referenced by exactly one pointer word of the image (a data word that happens to look like a token,
    // or a table the struct does not point at, would make the image wrong): otherwise no baked model - the kernel reads the device copy
    std::vector<int> seen((size_t)ea.n, 0);
    bool ok = true;
    for (size_t i = 0; i < nw && ok; i++)
      if ((wv[i] >> 32) == (EmitAlloc::TOKEN >> 32)) {
        const unsigned long long k = (wv[i] - EmitAlloc::TOKEN) / 16 - 1;
        if (k >= (unsigned long long)ea.n || (wv[i] - EmitAlloc::TOKEN) % 16 != 0 || seen[(size_t)k]++) ok = false;
      }
    for (int k = 0; k < ea.n && ok; k++) if (seen[(size_t)k] != 1) ok = false;
    if (!ok) return std::string("// (model not baked in: the DevModel image did not map one-to-one onto the emitted tables)\n");
  }
  std::string s = "#include \"mjb_types.hpp\"\n// the model as constant data of this translation unit (tables, then the DevModel image)\n";
  s += ea.text + decl + init;
  {
    // the uniform columns of the record tables the kernels read through MJB_REC (mjb_device.hpp), keyed by the pointer word of the
    // table in DevModel, so that MJB_REC finds them from the member it reads.  This list names those tables: a table that is not in
    // it gets no constants and is read as before (a missing entry costs a fold, never a wrong value).  A field that is batched per
    // environment in this kernel (prm_mask) is read from the environment's rows: no constants for its table, for the tables derived
    // from it, or for the record column that holds a copy of it.
    struct Named { size_t off; const char* name; int prm; unsigned long long drop; };
#define NM(f, prm, drop) {offsetof(DevModel<T>, f), #f, prm, drop}
    const Named named[] = {
        NM(body_pos, -1, 0), NM(body_quat, -1, 0), NM(body_ipos, -1, 0), NM(body_iquat, -1, 0), NM(geom_size, -1, 0), NM(actuator_trnid, -1, 0),
        NM(actuator_gear, PRM_ACT_GEAR, ~0ull), NM(actuator_gainprm, PRM_ACT_GAINPRM, ~0ull), NM(actuator_biasprm, PRM_ACT_BIASPRM, ~0ull),
        NM(actuator_ctrlrange, -1, 0), NM(actuator_forcerange, -1, 0), NM(pair_friction, PRM_GEOM_FRICTION, ~0ull),
        NM(pair_kb, -1, 0), NM(lim_f, -1, 0), NM(jnt_rec, -1, 0), NM(jnt_irec, -1, 0), NM(dof_irec, -1, 0),
        NM(dof_frec, PRM_DOF_DAMPING, 1ull), NM(body_irec, -1, 0), NM(pair_body, -1, 0), NM(lim_i, -1, 0)};
#undef NM
    for (size_t i = 0; i < nw; i++) {
      if ((wv[i] >> 32) != (EmitAlloc::TOKEN >> 32)) continue;
      const EmitAlloc::Cols& c = ea.cols[(size_t)((wv[i] - EmitAlloc::TOKEN) / 16 - 1)];
      const Named* nm = nullptr;
      for (const Named& x : named) if (x.off == 8 * i) nm = &x;
      if (!nm) continue;
      unsigned long long mask = c.mask;
      if (nm->prm >= 0 && ((prm_mask >> nm->prm) & 1)) mask &= ~nm->drop;
      if (!mask) continue;
      char hex[24];
      std::snprintf(hex, sizeof(hex), "0x%llxull", mask);
      s += std::string("// uniform columns of ") + nm->name + " (stride " + std::to_string(c.stride) + ")\ntemplate <> struct mjb::UniformCols<" + std::to_string(i) +
           "> { static constexpr unsigned long long mask = " + hex + ";";
      s += std::string(" static constexpr ") + c.ctype + " val[" + std::to_string(c.stride) + "] = {";
      for (int k = 0; k < c.stride; k++) s += (k ? ", " : "") + ((mask >> k) & 1 ? c.val[(size_t)k] : std::string("0"));
      s += "}; };\n";
    }
  }
  s += std::string("static_assert(sizeof(MjbBakedModel) == sizeof(mjb::DevModel<") + tname + ">), \"baked model image\");\n";
  s += std::string("#define MJB_SPEC_BAKED (*(const mjb::DevModel<") + tname + "> MJB_CONST*)&mjb_baked_model)\n";
  return s;
}

// Translation unit of a per-model specialised kernel (kind: MJB_KERNEL_*) under configuration c: the structural sizes of DevModel
// (never the run-time options: disableactuator, iterations, tolerance) and every offset of the kernel's LDS layout become
// __builtin_assume()s, and the model itself becomes constant data of the translation unit.
std::string spec_source(const HostModel& h_model, const Config& c, int dtype, int kind, int prm_mask) {
  // per-environment damping makes the implicit-damping path part of the step (mjb_device.hpp has_damping): the kernel is built, and the
  // model baked, as for a model with damping
  HostModel h_damped;
  if ((prm_mask >> PRM_DOF_DAMPING) & 1) { h_damped = h_model; h_damped.has_damping = 1; }
  const HostModel& h = (prm_mask >> PRM_DOF_DAMPING) & 1 ? h_damped : h_model;
  const KernelTarget t = kernel_target(c, dtype, kind);
  const Lay& L = *t.L;
  const int ncon_max = c.ncon_max, nefc_max = c.nefc_max;
  std::string s = kKinds[kind].banner;
  s += "#define MJB_SPEC_KERNEL " + std::to_string(kind) + "\n#define MJB_SPEC_TS " + t.ts + "\n#define MJB_SPEC_G " + std::to_string(t.G) + "\n#define MJB_SPEC_ASSUME(m)";
  auto A = [&](const char* obj, const char* f, long v) { s += std::string(" __builtin_assume((") + obj + ")." + f + " == " + std::to_string(v) + ");"; };
#define SM(f, v) A("m", #f, (long)(v))
  SM(nq, h.nq); SM(nv, h.nv); SM(nu, h.nu); SM(nbody, h.nbody); SM(njnt, h.njnt); SM(ngeom, h.ngeom); SM(nsite, h.nsite);
  SM(ntendon, h.ntendon); SM(nwrap, h.nwrap); SM(nsensor, h.nsensor); SM(nsensordata, h.nsensordata); SM(nkey, h.nkey); SM(npair, h.npair);
  SM(nlevel, h.nlevel); SM(integrator, h.integrator); SM(has_damping, h.has_damping); SM(has_fluid, h.has_fluid); SM(has_accel, h.has_accel);
  SM(nvp, h.nvp); SM(nvshift, h.nvshift); SM(ncon_max, ncon_max); SM(nefc_max, nefc_max); SM(nsiteact, h.siteact.size()); SM(nmpair, h.mpair.size());
  SM(nround, h.nround); SM(nround_inner, h.nround_inner); SM(max_nsub, h.max_nsub); SM(dfs_ok, h.dfs_ok);
#undef SM
  s += "\n";
  if (prm_mask) s += "#define MJB_SPEC_PARAMS " + std::to_string(prm_mask) + "   // per-environment model parameters: bit k = field MJB_PRM_k\n";
  s += "#define MJB_SPEC_ASSUME_LAY(L)";
#define SL(f) A("L", #f, (long)L.f)
  SL(qpos); SL(qvel); SL(ctrl); SL(qacc); SL(qacc_ws); SL(qacc_smooth); SL(qfrc_bias); SL(qfrc_passive); SL(qfrc_actuator); SL(qfrc_smooth);
  SL(qfrc_constraint); SL(xpos); SL(xquat); SL(xmat); SL(xipos); SL(ximat); SL(xanchor); SL(xaxis); SL(geom_xpos); SL(geom_xmat); SL(site_xpos);
  SL(site_xmat); SL(subtree_com); SL(cinert); SL(crb); SL(cdof); SL(cdof_dot); SL(cvel); SL(cacc); SL(cfrc); SL(dofbuf); SL(bfrc); SL(M); SL(W);
  SL(ten_length); SL(ten_J); SL(act_force); SL(sens); SL(con); SL(efc_J); SL(efc_pos); SL(efc_D); SL(efc_aref); SL(efc_jar); SL(efc_jv);
  SL(efc_force); SL(efc_KBI); SL(Ma); SL(grad); SL(search); SL(Mv); SL(tmp); SL(cholcol); SL(rk); SL(nT); SL(i_efc_type); SL(i_efc_id);
  SL(i_con_pair); SL(i_scal); SL(i_mail); SL(nI); SL(bytes);
#undef SL
  s += "\n";
  {
    // solimp powers of the model (joint limits, tendon limits, contact pairs): when every one is 1 or 2 (2 is MuJoCo's default) the
    // impedance curve needs no powf, and the specialised kernel is compiled without that code (~2 000 instructions of a cold branch)
    bool le2 = true;
    for (const char* name : {"jnt_solimp", "tendon_solimp", "pair_solimp"}) {
      const auto& v = h.D(name);
      for (size_t k = 4; k < v.size(); k += 5) { const double pw = v[k] > 1.0 ? v[k] : 1.0; if (pw != 1.0 && pw != 2.0) le2 = false; }
    }
    if (le2) s += "#define MJB_SPEC_SOLIMP_POWER_1_OR_2 1\n";       // (model fields are read-only after compilation: only the solver options change at run time)
  }
  s += kind != MJB_KERNEL_FD ? baked_model_source<float>(h, ncon_max, nefc_max, prm_mask) : baked_model_source<double>(h, ncon_max, nefc_max, prm_mask);
  s += "#include \"mjb_kernels.hpp\"\n";
  if (prm_mask) s += "extern \"C\" __constant__ int mjb_spec_params = " + std::to_string(prm_mask) + ";   // checked by mjb_kernel_load\n";
  // the point table's layout the kernel was compiled against, from the header itself: read by mjb_kernel_load
  if (kind == MJB_KERNEL_FD) s += "extern \"C\" __constant__ int mjb_spec_fd_points = MJB_FD_POINTS_ABI;\n";
  return s;
}

// How k_step's work is mapped to workgroups (mjb_kernels.hpp).  With no more environment blocks than the chip holds at once every
// block keeps its workgroup for the whole launch; beyond that the resident workgroups draw (block, chunk-of-steps) tickets, which
// removes the "rounds" of the static map and their tails (profiles/r02_wave_timeline.log: -20 % launch time at 20 steps per launch,
// -9 % at 100, humanoid B = 4096).  Chunk length ~ sqrt(steps)/2: per-chunk cost (state through memory, one ticket) ~2 us against
// a tail of half a chunk.  The priority hand-over (StepArgs::fair_bit) matters where the launch waits for its slowest wave.
static void choose_schedule(mjbData* d, StepArgs& a) {
  a.chunk_steps = 0; a.fair_bit = 0; a.nblk = 0; a.grid_blocks = 0; a.nuniform = 0; a.nchunk = 0;
  if (a.mode != 0) return;
  if (d->sched_chunk == -1) {
    const char* e1 = std::getenv("MJB_CHUNK_STEPS"); const char* e2 = std::getenv("MJB_FAIR_BIT");
    d->sched_chunk = e1 ? std::atoi(e1) : -2; d->fair_bit = e2 ? std::atoi(e2) : -2;
  }
  const int epb = 64 / d->cfg.G;
  const long nblk = (d->batch + epb - 1) / epb;
  if (d->step_slots < 0) {
    int nb = 0;
    if (hipFunction_t fn = d->spec[MJB_KERNEL_STEP].fn) {
      if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 64, (size_t)epb * d->cfg.Lf.bytes) != hipSuccess) nb = 0;
    } else nb = d->dtype == MJB_F32 ? step_blocks_per_cu<float, float>(d->cfg.G, d->cfg.Lf) : step_blocks_per_cu<double, double>(d->cfg.G, d->cfg.Ld);
    d->step_slots = nb > 0 ? (long)nb * d->ncu : 0;           // 0 = unknown: keep the static map
  }
  a.fair_bit = d->fair_bit >= 0 ? d->fair_bit : 15;            // 2^15 x 10 ns = 0.33 ms per turn
  a.nblk = (int)nblk; a.grid_blocks = d->step_slots > 0 && d->step_slots < nblk ? (int)d->step_slots : (int)nblk;
  if (d->sched_chunk >= 0) {
    a.chunk_steps = a.nstep > 1 ? d->sched_chunk : 0;
    if (std::getenv("MJB_SCHED_DEBUG")) std::fprintf(stderr, "[mjb] schedule (override): blocks %ld, resident slots %ld, steps %d -> chunk_steps %d, fair_bit %d\n", nblk, d->step_slots, a.nstep, a.chunk_steps, a.fair_bit);
    return;
  }
  if (d->step_slots > 0 && nblk > d->step_slots && a.nstep >= 4) {
    // uniform chunks of c steps, then a guided taper (every further chunk = half of what is left, chunk_plan): the tail of the launch
    // is half of the LAST chunk (one step), so c only trades switches (~2.7 us each: hand-over out, one ticket, hand-over in)
    // against how early imbalance starts to be evened out.  c ~ sqrt(3 N): 8 at N = 20, 17 at N = 100 (measured flat optimum
    // 6..12 and 12..16, profiles/r02_schedule.log), at most 32
    int c = (int)std::lround(std::sqrt(3.0 * (double)a.nstep));
    a.chunk_steps = c < 1 ? 1 : (c > 32 ? 32 : c);
  }
  if (std::getenv("MJB_SCHED_DEBUG")) std::fprintf(stderr, "[mjb] schedule: blocks %ld, resident slots %ld, steps %d -> chunk_steps %d, fair_bit %d\n", nblk, d->step_slots, a.nstep, a.chunk_steps, a.fair_bit);
}

// Bit 3 of the engine flags: a wave of a ticket-mode launch gave up waiting for a hand-over and left its environment where the launch
// found it - the results of that launch are incomplete.  The kernels set the word in pinned host memory, so after any stream
// synchronisation (and at the entry of the next launch) the host sees it without a copy: every entry point that synchronises
// returns MJB_ERR_DEVICE from then on, until mjb_reset clears the flags.
int engine_check(const mjbData* d) {
  if (d->flags_pin.get() && __atomic_load_n(d->flags_pin.get() + 3, __ATOMIC_ACQUIRE) != 0)
    return fail(MJB_ERR_DEVICE, "a ticket-mode launch timed out waiting for a state hand-over (engine flag 8): the environments concerned were not "
                                "advanced; mjb_reset() clears the condition");
  return MJB_OK;
}

// A per-model specialised step kernel (MJB_KERNEL_STEP or MJB_KERNEL_STEP2): the arguments of the generic fp32 kernel, lg = its layout
hipError_t launch_spec_step(mjbData* d, int kind, const Lay* lg, const DevDebug<float>& dbg, const StepArgs& a, const ObsSpecDev& obs,
                            void* obs_out, unsigned grid, unsigned block, size_t lds) {
  const DevModel<float>* mg = d->mf_dev;
  DevData<float> dv = d->df; DevDebug<float> dbgarg = dbg; StepArgs av = a; ObsSpecDev ov = obs; float* oo = (float*)obs_out;
  void* args[] = {(void*)&mg, (void*)&lg, (void*)&dv, (void*)&dbgarg, (void*)&av, (void*)&ov, (void*)&oo};
  return hipModuleLaunchKernel(d->spec[kind].fn, grid, 1, 1, block, 1, 1, (unsigned)lds, d->stream, args, nullptr);
}

int launch(mjbData* d, const StepArgs& a_in, const ObsSpecDev& obs, void* obs_out, bool debug) {
  int rc = engine_check(d);                                    // no further launches on top of a failed one
  if (rc != MJB_OK) return rc;
  rc = refresh_options(d);
  if (rc != MJB_OK) return rc;
  hipError_t e;
  StepArgs a = a_in;
  choose_schedule(d, a);
  if (a.chunk_steps > 0) {
    if (d->dtype != MJB_F32 || a.nstep >= (1 << 20) - 2) a.chunk_steps = 0;     // hand-over words are (fp32, tag) pairs; 20 bits of step index in the tag
  }
  if (a.chunk_steps > 0 && !d->df.xfer) {
    const HostModel& hm = d->model->h;
    if (reserve_zeroed(d->xfer, (size_t)d->batch * (size_t)(hm.nq + 3 * hm.nv + 2)) != hipSuccess) a.chunk_steps = 0;   // no memory: static map
    d->df.xfer = d->xfer.get();
  }
  if (a.chunk_steps > 0) chunk_plan_counts(a.nstep, a.chunk_steps, a.nuniform, a.nchunk);
  if (a.mode == 0) {
    const int epb = 64 / d->cfg.G;
    d->last_sched[0] = a.nstep; d->last_sched[1] = (d->batch + epb - 1) / epb; d->last_sched[2] = (int)(d->step_slots > 0 ? d->step_slots : 0);
    d->last_sched[3] = a.chunk_steps; d->last_sched[4] = a.fair_bit;
  }
  // host-side bookkeeping of the ticket counter and the tag sequence: COMMITTED only after the launch succeeded (a failed launch must
  // not leave the host counter ahead of the device's: every later ticket would then underflow and no step would run)
  unsigned seq_next = d->launch_seq;
  unsigned long long ticket_after = d->ticket_next;
  if (a.chunk_steps > 0) {
    do { seq_next++; } while ((seq_next & 0xFFFu) == 0);
    a.tagbase = (seq_next & 0xFFFu) << 20;
    // the ticket counter is never reset on the hot path: every launched workgroup draws tickets until one is past the end, so a
    // launch advances the counter by exactly (tickets + workgroups) and the next launch starts from there (32-bit: rewound long before it wraps)
    const unsigned long long adv = (unsigned long long)a.nblk * (unsigned)a.nchunk + (unsigned long long)a.grid_blocks;
    if (d->ticket_next + adv > 0xF0000000ull) { HIPCHK(hipMemsetAsync(d->df.sched, 0, sizeof(unsigned), d->stream)); d->ticket_next = 0; }
    a.ticket_base = (unsigned)d->ticket_next;
    ticket_after = d->ticket_next + adv;
    if (d->xfer_timeout == 0) {                                  // default 5 s of wall clock; MJB_XFER_TIMEOUT_MS for tests
      const char* e1 = std::getenv("MJB_XFER_TIMEOUT_MS");
      double ms = e1 ? std::atof(e1) : 5000.0;
      if (!(ms > 0)) ms = 5000.0;
      if (ms > 40000.0) ms = 40000.0;
      d->xfer_timeout = (unsigned)(ms * 1e5);
      if (d->xfer_timeout == 0) d->xfer_timeout = 1;
    }
    if (d->xfer_poison_env < 0) { const char* e2 = std::getenv("MJB_XFER_POISON_ENV"); d->xfer_poison_env = e2 ? std::atoi(e2) + 1 : 0; if (d->xfer_poison_env < 0) d->xfer_poison_env = 0; }
    a.xfer_timeout = d->xfer_timeout; a.xfer_poison_env = d->xfer_poison_env;
  }
  // Two waves per environment (env_run2) when the batch leaves at least half of the step kernel's resident slots empty: stepping
  // launches only (mode 0, no debug dumps), fp32, one wave per environment, nv <= 32, Euler.
  bool two = false;
  if (a.mode == 0 && !debug && d->dtype == MJB_F32 && d->cfg.Lf2.bytes > 0 && a.chunk_steps == 0) {
    if (d->two_wave == -1) { const char* e2 = std::getenv("MJB_TWO_WAVE"); d->two_wave = e2 ? (std::atoi(e2) ? 1 : 0) : 2; }
    // every environment must be resident at once: the kernel is built for two waves per SIMD (__launch_bounds__(128, 2)), i.e. four
    // workgroups per CU.  Measured on the humanoid (profiles/r02_two_wave.log): x1.15 .. 1.18 up to 512 environments (two SIMDs per
    // environment), x1.12 at 768, x1.09 at 1024, x0.7 beyond (two rounds)
    long wg_per_cu = d->cfg.Lf2.bytes > 0 ? (160L * 1024) / d->cfg.Lf2.bytes : 0;
    if (wg_per_cu > 4) wg_per_cu = 4;
    two = d->two_wave == 1 || (d->two_wave == 2 && (long)d->batch <= wg_per_cu * d->ncu);
  }
  d->last_sched[5] = two ? 1 : 0;
  DevDebug<float> nodbg; std::memset(&nodbg, 0, sizeof(nodbg));
  if (two) {
    a.fair_bit = 0;
    if (d->spec[MJB_KERNEL_STEP2].fn)
      e = launch_spec_step(d, MJB_KERNEL_STEP2, d->Lf2_dev, nodbg, a, obs, obs_out, (unsigned)d->batch, 128, (size_t)d->cfg.Lf2.bytes);
    else e = launch_step2<float, float>(d->mf_dev, d->Lf2_dev, d->cfg.Lf2, d->df, a, obs, (float*)obs_out, d->stream);
  } else if (d->spec[MJB_KERNEL_STEP].fn) {                  // per-model specialised kernel: same arguments, same grid
    const int epb = 64 / d->cfg.G;
    const unsigned grid = a.chunk_steps > 0 ? (unsigned)a.grid_blocks : (unsigned)((d->batch + epb - 1) / epb);
    e = launch_spec_step(d, MJB_KERNEL_STEP, d->Lf_dev, debug ? d->dbgf : nodbg, a, obs, obs_out, grid, 64, (size_t)epb * d->cfg.Lf.bytes);
  } else if (d->dtype == MJB_F32) {
    e = launch_step<float, float>(d->cfg.G, d->mf_dev, d->Lf_dev, d->cfg.Lf, d->df, debug ? d->dbgf : nodbg, a, obs, (float*)obs_out, d->stream);
  } else {
    DevDebug<double> none; std::memset(&none, 0, sizeof(none));
    e = launch_step<double, double>(d->cfg.G, d->md_dev, d->Ld_dev, d->cfg.Ld, d->dd, debug ? d->dbgd : none, a, obs, (double*)obs_out, d->stream);
  }
  if (e != hipSuccess) {
    // the device counter may or may not have been rewound above and no workgroup drew a ticket: start the next ticket launch from a
    // known state (counter zeroed in stream order, host count zero)
    if (a.chunk_steps > 0) { (void)hipMemsetAsync(d->df.sched, 0, sizeof(unsigned), d->stream); d->ticket_next = 0; }
    return fail(MJB_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
  }
  d->launch_seq = seq_next; d->ticket_next = ticket_after;
  return MJB_OK;
}

// pinned staging block of the array getters / setters: the copies run on the data's stream straight to / from pinned memory (no pageable
// staging inside the runtime, no per-call temporary), the widening / narrowing conversion happens between it and the caller's array
int copy_out(mjbData* d, const ArrayInfo& ai, double* host_out) {
  size_t n = (size_t)d->batch * ai.per_env;
  if (n == 0) return MJB_OK;
  const bool wide = ai.kind == 1 || (ai.kind == 0 && d->dtype == MJB_F64);
  if (!wide && ai.kind != 0 && ai.kind != 3) return fail(MJB_ERR_ARG, "integer array requested as float64");
  const size_t bytes = n * (wide ? sizeof(double) : sizeof(float));
  HIPCHK(d->io_pin.reserve(bytes, true));
  HIPCHK(hipMemcpyAsync(d->io_pin.get(), ai.ptr, bytes, hipMemcpyDeviceToHost, d->stream));   // ordered behind whatever the stream still runs
  HIPCHK(hipStreamSynchronize(d->stream));
  { int ec = engine_check(d); if (ec != MJB_OK) return ec; }
  if (ai.kind == 3) { const unsigned* src = (const unsigned*)d->io_pin.get(); for (size_t i = 0; i < n; i++) host_out[i] = (double)src[i]; }
  else if (wide) std::memcpy(host_out, d->io_pin.get(), bytes);
  else { const float* src = (const float*)d->io_pin.get(); for (size_t i = 0; i < n; i++) host_out[i] = (double)src[i]; }
  return MJB_OK;
}
}  // namespace

extern "C" {

const char* mjb_last_error(void) { return g_err.c_str(); }
// for the other translation units of the library (mjb_mjcf.cpp): set the error string, return the code
int mjb_set_error_(int code, const char* msg) { return fail(code, msg ? msg : ""); }

int mjb_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mjb_model_create(int nfield, const char* const* names, const void* const* ptrs, const int* dtypes, const long* counts, mjbModel** out) {
  if (!out) return fail(MJB_ERR_ARG, "out is NULL");
  Table t{nfield, names, ptrs, dtypes, counts};
  mjbModel* m = new mjbModel();
  std::string err;
  if (!m->h.load(t, err)) { delete m; return fail(MJB_ERR_MODEL, err); }
  if (!keep_table(m, t, err)) { delete m; return fail(MJB_ERR_MODEL, err); }
  m->disableactuator = m->h.disableactuator;
  m->iterations = m->h.iterations;
  m->tolerance = m->h.tolerance;
  *out = m;
  return MJB_OK;
}

void mjb_model_free(mjbModel* m) { delete m; }

int mjb_model_set_disableactuator(mjbModel* m, int mask) { if (!m) return fail(MJB_ERR_ARG, "model is NULL"); m->disableactuator = mask; return MJB_OK; }
int mjb_model_set_solver(mjbModel* m, int iterations, double tolerance) {
  if (!m || iterations < 1 || !(tolerance >= 0)) return fail(MJB_ERR_ARG, "bad solver options");
  m->iterations = iterations; m->tolerance = tolerance;
  return MJB_OK;
}

int mjb_data_create(mjbModel* m, int batch, int dtype, int lanes, int nconmax, int nefcmax, int device, int env0, mjbData** out) {
  if (!m || !out) return fail(MJB_ERR_ARG, "model/out is NULL");
  if (batch < 1) return fail(MJB_ERR_ARG, "batch must be >= 1");
  if (dtype != MJB_F32 && dtype != MJB_F64) return fail(MJB_ERR_ARG, "dtype must be MJB_F32 or MJB_F64");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(MJB_ERR_DEVICE, "no HIP device: the batched engine has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(MJB_ERR_ARG, "device index out of range");
  HIPCHK(hipSetDevice(device));
  const HostModel& h = m->h;
  Config cfg;
  std::string err;
  if (!derive_config(h, dtype, lanes, nconmax, nefcmax, cfg, err)) return fail(MJB_ERR_ARG, err);
  mjbData* d = new mjbData();
  d->model = m; d->batch = batch; d->dtype = dtype; d->cfg = cfg; d->device = device; d->env0 = env0; d->stream = nullptr;
  if (hipDeviceGetAttribute(&d->ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || d->ncu < 1) d->ncu = 256;
  DevAlloc tables{d->arena};
  fill_dev_model<float>(h, tables, cfg.ncon_max, cfg.nefc_max, d->mf);
  fill_dev_model<double>(h, tables, cfg.ncon_max, cfg.nefc_max, d->md);
  if (!d->arena.ok) { mjb_data_free(d); return fail(MJB_ERR_DEVICE, "device allocation of the model failed"); }
  if (dev_alloc(d, &d->mf_dev, 1) || dev_alloc(d, &d->md_dev, 1) || dev_alloc(d, &d->Lf_dev, 1) || dev_alloc(d, &d->Ld_dev, 1) || dev_alloc(d, &d->Lf2_dev, 1) ||
      hipMemcpy(d->Lf2_dev, &d->cfg.Lf2, sizeof(Lay), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d->Lf_dev, &d->cfg.Lf, sizeof(Lay), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d->Ld_dev, &d->cfg.Ld, sizeof(Lay), hipMemcpyHostToDevice) != hipSuccess) {
    mjb_data_free(d);
    return fail(MJB_ERR_DEVICE, "device allocation of the model descriptors failed");
  }
  std::memset(&d->df, 0, sizeof(d->df)); std::memset(&d->dd, 0, sizeof(d->dd));
  int rc = dtype == MJB_F32 ? alloc_state(d, d->df) : alloc_state(d, d->dd);
  if (rc) { mjb_data_free(d); return fail(MJB_ERR_DEVICE, "device allocation of the state failed"); }
  *out = d;
  int r = mjb_reset(d, -1);
  if (r != MJB_OK) { mjb_data_free(d); *out = nullptr; return r; }
  return MJB_OK;
}

void mjb_data_free(mjbData* d) {
  if (!d) return;
  (void)hipSetDevice(d->device);
  for (auto& k : d->spec) if (k.mod) (void)hipModuleUnload(k.mod);
  if (d->fd_done) (void)hipEventDestroy(d->fd_done);
  delete d;                                                    // the arena and every Buffer member release their memory
}

int mjb_set_stream(mjbData* d, void* hip_stream) { if (!d) return fail(MJB_ERR_ARG, "data is NULL"); d->stream = (hipStream_t)hip_stream; return MJB_OK; }
int mjb_sync(mjbData* d) { if (!d) return fail(MJB_ERR_ARG, "data is NULL"); HIPCHK(hipStreamSynchronize(d->stream)); return engine_check(d); }

int mjb_engine_flags(mjbData* d, int* flags_out) {
  if (!d || !flags_out) return fail(MJB_ERR_ARG, "NULL argument");
  HIPCHK(hipStreamSynchronize(d->stream));
  return mjb_engine_flags_peek(d, flags_out);
}

int mjb_engine_flags_peek(mjbData* d, int* flags_out) {
  if (!d || !flags_out) return fail(MJB_ERR_ARG, "NULL argument");
  int fl = 0;
  for (int k = 0; k < 4; k++) if (d->flags_pin.get() && __atomic_load_n(d->flags_pin.get() + k, __ATOMIC_ACQUIRE) != 0) fl |= 1 << k;
  *flags_out = fl;
  return MJB_OK;
}

int mjb_data_info(mjbData* d, int* batch, int* dtype, int* lanes, int* nconmax, int* nefcmax, int* lds_bytes_per_env) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  if (batch) *batch = d->batch;
  if (dtype) *dtype = d->dtype;
  if (lanes) *lanes = d->cfg.G;
  if (nconmax) *nconmax = d->cfg.ncon_max;
  if (nefcmax) *nefcmax = d->cfg.nefc_max;
  if (lds_bytes_per_env) *lds_bytes_per_env = d->dtype == MJB_F32 ? d->cfg.Lf.bytes : d->cfg.Ld.bytes;
  return MJB_OK;
}

int mjb_array_ptr(mjbData* d, const char* name, void** dev_ptr, long* per_env, int* dtype) {
  if (!d || !name) return fail(MJB_ERR_ARG, "data/name is NULL");
  auto it = d->arrays.find(name);
  if (it == d->arrays.end()) return fail(MJB_ERR_ARG, std::string("unknown array: ") + name);
  if (dev_ptr) *dev_ptr = it->second.ptr;
  if (per_env) *per_env = it->second.per_env;
  if (dtype) *dtype = it->second.kind == 0 ? d->dtype : (it->second.kind == 1 ? MJB_F64 : 2);      // (uint32 "episode": int32 bits)
  return MJB_OK;
}

int mjb_get_array(mjbData* d, const char* name, double* host_out) {
  if (!d || !name || !host_out) return fail(MJB_ERR_ARG, "NULL argument");
  auto it = d->arrays.find(name);
  if (it == d->arrays.end()) return fail(MJB_ERR_ARG, std::string("unknown array: ") + name);
  HIPCHK(hipSetDevice(d->device));
  return copy_out(d, it->second, host_out);
}

int mjb_set_array(mjbData* d, const char* name, const double* host_in) {
  if (!d || !name || !host_in) return fail(MJB_ERR_ARG, "NULL argument");
  auto it = d->arrays.find(name);
  if (it == d->arrays.end()) return fail(MJB_ERR_ARG, std::string("unknown array: ") + name);
  const ArrayInfo& ai = it->second;
  size_t n = (size_t)d->batch * ai.per_env;
  if (n == 0) return MJB_OK;
  HIPCHK(hipSetDevice(d->device));
  const bool wide = ai.kind == 1 || (ai.kind == 0 && d->dtype == MJB_F64);
  if (!wide && ai.kind != 0) return fail(MJB_ERR_ARG, "integer arrays are read-only");   // (counters, episode)
  const size_t bytes = n * (wide ? sizeof(double) : sizeof(float));
  HIPCHK(d->io_pin.reserve(bytes, true));
  if (wide) std::memcpy(d->io_pin.get(), host_in, bytes);
  else { float* dst = (float*)d->io_pin.get(); for (size_t i = 0; i < n; i++) dst[i] = (float)host_in[i]; }
  HIPCHK(hipMemcpyAsync(ai.ptr, d->io_pin.get(), bytes, hipMemcpyHostToDevice, d->stream));    // ordered behind the launches already queued
  HIPCHK(hipStreamSynchronize(d->stream));                                               // the staging block is free again on return
  return MJB_OK;
}

int mjb_get_counters(mjbData* d, int* host_out) {
  if (!d || !host_out) return fail(MJB_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(host_out, d->arrays["counters"].ptr, (size_t)d->batch * CNT_N * sizeof(int), hipMemcpyDeviceToHost));
  return engine_check(d);
}

int mjb_reset(mjbData* d, int key) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  const HostModel& h = d->model->h;
  if (key >= h.nkey) return fail(MJB_ERR_LOOKUP, "keyframe index out of range");
  HIPCHK(hipSetDevice(d->device));
  int threads = 256, grid = (d->batch + threads - 1) / threads;
  double time = key >= 0 ? h.D("key_time")[key] : 0.0;
  if (d->dtype == MJB_F32) {
    const float* qp = key >= 0 ? d->mf.key_qpos + (size_t)key * h.nq : d->mf.qpos0;
    const float* qv = key >= 0 ? d->mf.key_qvel + (size_t)key * h.nv : nullptr;
    const float* cu = key >= 0 ? d->mf.key_ctrl + (size_t)key * h.nu : nullptr;
    hipLaunchKernelGGL(k_reset<float>, dim3(grid), dim3(threads), 0, d->stream, d->df, h.nq, h.nv, h.nu, qp, qv, cu, time);
  } else {
    const double* qp = key >= 0 ? d->md.key_qpos + (size_t)key * h.nq : d->md.qpos0;
    const double* qv = key >= 0 ? d->md.key_qvel + (size_t)key * h.nv : nullptr;
    const double* cu = key >= 0 ? d->md.key_ctrl + (size_t)key * h.nu : nullptr;
    hipLaunchKernelGGL(k_reset<double>, dim3(grid), dim3(threads), 0, d->stream, d->dd, h.nq, h.nv, h.nu, qp, qv, cu, time);
  }
  HIPCHK(hipGetLastError());
  // a reset also clears the sticky engine flags (k_reset, in stream order); after a failed ticket launch the host-visible word must be
  // clear before the next launch's entry check reads it: wait for the reset in that (rare) case
  if (d->flags_pin.get() && __atomic_load_n(d->flags_pin.get() + 3, __ATOMIC_ACQUIRE) != 0) HIPCHK(hipStreamSynchronize(d->stream));
  return MJB_OK;
}

int mjb_reset_envs(mjbData* d, int key, const unsigned char* mask_dev, unsigned seed, double qpos_noise, double qvel_noise) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  const HostModel& h = d->model->h;
  if (key >= h.nkey) return fail(MJB_ERR_LOOKUP, "keyframe index out of range");
  if (!(qpos_noise >= 0) || !(qvel_noise >= 0) || std::isinf(qpos_noise) || std::isinf(qvel_noise)) return fail(MJB_ERR_ARG, "reset noise must be finite and >= 0");
  HIPCHK(hipSetDevice(d->device));
  // float64 tables whatever the data dtype: the noise is computed in float64 and rounded once (without noise: the fp32 tables' values)
  ResetSpec r;
  r.nq = h.nq; r.nv = h.nv; r.nu = h.nu; r.njnt = h.njnt;
  r.jnt_type = d->md.jnt_type; r.jnt_qposadr = d->md.jnt_qposadr; r.jnt_dofadr = d->md.jnt_dofadr;
  r.qpos = key >= 0 ? d->md.key_qpos + (size_t)key * h.nq : d->md.qpos0;
  r.qvel = key >= 0 ? d->md.key_qvel + (size_t)key * h.nv : nullptr;
  r.ctrl = key >= 0 ? d->md.key_ctrl + (size_t)key * h.nu : nullptr;
  r.time = key >= 0 ? h.D("key_time")[key] : 0.0;
  r.seed = seed; r.qpos_noise = qpos_noise; r.qvel_noise = qvel_noise;
  const int threads = 64, grid = (d->batch + threads - 1) / threads;
  if (d->dtype == MJB_F32) hipLaunchKernelGGL(k_reset_envs<float>, dim3(grid), dim3(threads), 0, d->stream, d->df, r, mask_dev, (unsigned)d->env0, d->episode.get());
  else hipLaunchKernelGGL(k_reset_envs<double>, dim3(grid), dim3(threads), 0, d->stream, d->dd, r, mask_dev, (unsigned)d->env0, d->episode.get());
  HIPCHK(hipGetLastError());
  return MJB_OK;
}

static StepArgs make_args(mjbData* d, int nstep, int ctrl_mode, unsigned seed, unsigned step0, double scale, int mode) {
  StepArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nstep = nstep; a.ctrl_mode = ctrl_mode; a.seed = seed; a.step0 = step0; a.env0 = (unsigned)d->env0;
  a.ctrl_scale = scale; a.dt = d->model->h.timestep; a.mode = mode; a.write_kin = 1; a.obs_every = 0;
  static const int rep = std::getenv("MJB_REPEAT_PHASE") ? std::atoi(std::getenv("MJB_REPEAT_PHASE")) : -1;   // diagnostic kernels only (-DMJB_PHASE_REPEAT)
  a.repeat_phase = rep;
  return a;
}

// the specialised kernels: model-level and data-level sources come from the same configuration (derive_config) and the same target
static long kernel_source(const HostModel& h, const Config& c, int dtype, int kind, int prm_mask, char* buf, long cap) {
  if (check_kind(c, dtype, kind) != MJB_OK) return -1;
  if (prm_mask < 0 || prm_mask >= (1 << PRM_NFIELD)) { fail(MJB_ERR_ARG, "params_mask has bits beyond MJB_PRM_N"); return -1; }
  const std::string src = spec_source(h, c, dtype, kind, prm_mask);
  if (buf && cap > (long)src.size()) std::memcpy(buf, src.c_str(), src.size() + 1);
  return (long)src.size();
}

long mjb_model_kernel_source_params(mjbModel* m, int kind, int dtype, int lanes, int nconmax, int nefcmax, int params_mask, char* buf, long cap) {
  if (!m) { fail(MJB_ERR_ARG, "model is NULL"); return -1; }
  if (dtype != MJB_F32 && dtype != MJB_F64) { fail(MJB_ERR_ARG, "dtype must be MJB_F32 or MJB_F64"); return -1; }
  Config c;
  std::string err;
  if (!derive_config(m->h, dtype, lanes, nconmax, nefcmax, c, err)) { fail(MJB_ERR_ARG, err); return -1; }
  return kernel_source(m->h, c, dtype, kind, params_mask, buf, cap);
}

long mjb_model_kernel_source(mjbModel* m, int kind, int dtype, int lanes, int nconmax, int nefcmax, char* buf, long cap) {
  return mjb_model_kernel_source_params(m, kind, dtype, lanes, nconmax, nefcmax, 0, buf, cap);
}

long mjb_kernel_source(mjbData* d, int kind, char* buf, long cap) {
  if (!d) { fail(MJB_ERR_ARG, "data is NULL"); return -1; }
  return kernel_source(d->model->h, d->cfg, d->dtype, kind, d->prm_mask, buf, cap);
}

// Unload a kind's module (after the stream has drained).  The step kernel's occupancy decides the ticket map's grid: re-query it.
static void drop_kernel(mjbData* d, int kind) {
  if (!d->spec[kind].mod) return;
  (void)hipModuleUnload(d->spec[kind].mod);
  d->spec[kind].mod = nullptr; d->spec[kind].fn = nullptr;
  if (kind == MJB_KERNEL_STEP) d->step_slots = -1;
}

int mjb_kernel_load(mjbData* d, int kind, const void* image, long nbytes) {
  if (!d || !image || nbytes <= 0) return fail(MJB_ERR_ARG, "NULL argument");
  int rc = check_kind(d->cfg, d->dtype, kind);
  if (rc != MJB_OK) return rc;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipStreamSynchronize(d->stream));
  drop_kernel(d, kind);
  hipModule_t mod; hipFunction_t fn;
  hipError_t e = hipModuleLoadData(&mod, image);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("hipModuleLoadData: ") + hipGetErrorString(e));
  e = hipModuleGetFunction(&fn, mod, kKinds[kind].symbol);
  if (e != hipSuccess) { (void)hipModuleUnload(mod); return fail(MJB_ERR_DEVICE, std::string("code object has no ") + kKinds[kind].symbol + " kernel"); }
  // the batched fields the kernel was built for (spec_source: the symbol exists when the set is not empty) must be this data's: a
  // kernel built for a field reads only that field's rows, one built without it reads only the model table
  int built_for = 0;
  hipDeviceptr_t sym = nullptr; size_t symsize = 0;
  if (hipModuleGetGlobal(&sym, &symsize, mod, "mjb_spec_params") == hipSuccess && symsize == sizeof(int)) {
    if (hipMemcpyDtoH(&built_for, sym, sizeof(int)) != hipSuccess) { (void)hipModuleUnload(mod); return fail(MJB_ERR_DEVICE, "reading mjb_spec_params of the code object failed"); }
  } else (void)hipGetLastError();
  if (built_for != d->prm_mask) {
    (void)hipModuleUnload(mod);
    return fail(MJB_ERR_ARG, "the specialised kernel was built for per-environment parameters " + std::to_string(built_for) + ", this data object has " +
                                 std::to_string(d->prm_mask) + " (take the source from mjb_kernel_source after mjb_set_env_param)");
  }
  if (kind == MJB_KERNEL_FD) {
    // a code object from a header whose point table had no sensor output carries no such record (or an older one): it still serves
    // the plain calls (the members it reads kept their offsets), and a sensor request takes the generic kernel instead (fd_run_slab)
    int abi = 0;
    if (hipModuleGetGlobal(&sym, &symsize, mod, "mjb_spec_fd_points") == hipSuccess && symsize == sizeof(int)) {
      if (hipMemcpyDtoH(&abi, sym, sizeof(int)) != hipSuccess) { (void)hipModuleUnload(mod); return fail(MJB_ERR_DEVICE, "reading mjb_spec_fd_points of the code object failed"); }
    } else (void)hipGetLastError();
    d->spec_fd_sensors = abi == MJB_FD_POINTS_ABI;
  }
  d->spec[kind].mod = mod; d->spec[kind].fn = fn; d->spec_prm[kind] = built_for;
  if (kind == MJB_KERNEL_STEP) d->step_slots = -1;
  return MJB_OK;
}

int mjb_kernel_unload(mjbData* d, int kind) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  if (!valid_kind(kind)) return fail(MJB_ERR_ARG, "unknown kernel kind (MJB_KERNEL_STEP, MJB_KERNEL_FD or MJB_KERNEL_STEP2)");
  if (d->spec[kind].mod) { HIPCHK(hipStreamSynchronize(d->stream)); drop_kernel(d, kind); }
  return MJB_OK;
}

int mjb_forward(mjbData* d) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  HIPCHK(hipSetDevice(d->device));
  ObsSpecDev none; std::memset(&none, 0, sizeof(none));
  return launch(d, make_args(d, 1, MJB_CTRL_KEEP, 0, 0, 1.0, 1), none, nullptr, false);
}

int mjb_forward_envs(mjbData* d, const unsigned char* mask_dev) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  HIPCHK(hipSetDevice(d->device));
  ObsSpecDev none; std::memset(&none, 0, sizeof(none));
  StepArgs a = make_args(d, 1, MJB_CTRL_KEEP, 0, 0, 1.0, 1);
  a.env_mask = mask_dev;
  return launch(d, a, none, nullptr, false);
}

int mjb_inverse(mjbData* d) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  HIPCHK(hipSetDevice(d->device));
  ObsSpecDev none; std::memset(&none, 0, sizeof(none));
  return launch(d, make_args(d, 1, MJB_CTRL_KEEP, 0, 0, 1.0, 2), none, nullptr, false);
}

int mjb_step(mjbData* d, int nstep) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  if (nstep < 1) return fail(MJB_ERR_ARG, "nstep must be >= 1");
  HIPCHK(hipSetDevice(d->device));
  ObsSpecDev none; std::memset(&none, 0, sizeof(none));
  return launch(d, make_args(d, nstep, MJB_CTRL_KEEP, 0, 0, 1.0, 0), none, nullptr, false);
}

int mjb_rollout(mjbData* d, int nstep, int ctrl_mode, unsigned seed, unsigned step0, double ctrl_scale,
                const mjbObsSpec* spec, void* obs_out_dev, int obs_every) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  if (nstep < 1) return fail(MJB_ERR_ARG, "nstep must be >= 1");
  if (ctrl_mode < 0 || ctrl_mode > 3) return fail(MJB_ERR_ARG, "bad ctrl_mode");
  if (ctrl_mode == 3 && !d->fbd[0].get()) return fail(MJB_ERR_ARG, "MJB_CTRL_FEEDBACK needs mjb_set_feedback() first");
  HIPCHK(hipSetDevice(d->device));
  StepArgs a = make_args(d, nstep, ctrl_mode, seed, step0, ctrl_scale, 0);
  if (ctrl_mode == 3) {
    if (d->dtype == MJB_F32) { a.fb_K = d->fbf[0].get(); a.fb_u0 = d->fbf[1].get(); a.fb_q0 = d->fbf[2].get(); a.fb_v0 = d->fbf[3].get(); }
    else { a.fb_K = d->fbd[0].get(); a.fb_u0 = d->fbd[1].get(); a.fb_q0 = d->fbd[2].get(); a.fb_v0 = d->fbd[3].get(); }
    if (d->fb_nsteps > 0) {
      a.fb_nsteps = d->fb_nsteps; a.fb_env_stride = d->fb_env_stride;
      a.fb_noise_std = d->dtype == MJB_F32 ? (const void*)d->fb_noise_f[0].get() : (const void*)d->fb_noise_d[0].get();
      a.fb_noise_tab = d->dtype == MJB_F32 ? (const void*)d->fb_noise_f[1].get() : (const void*)d->fb_noise_d[1].get();
    }
  }
  ObsSpecDev obs; std::memset(&obs, 0, sizeof(obs));
  if (spec && obs_out_dev && obs_every > 0) { obs = spec->dev; a.obs_every = obs_every; }
  return launch(d, a, obs, obs_out_dev, false);
}

// The control table of mjb_rollout_ctrl is read by the step kernel at caller-chosen offsets: everything it could touch is checked
// here, before anything is launched, so that a bad pointer or extent comes back as MJB_ERR_ARG instead of a page fault on the device.
static int check_ctrl_table(mjbData* d, int nstep, const void* ctrl_dev, long step_stride, long env_stride) {
  const int nu = d->model->h.nu;
  if (nu == 0) return MJB_OK;                                  // nothing is read: NULL allowed
  if (!ctrl_dev) return fail(MJB_ERR_ARG, "mjb_rollout_ctrl: ctrl_dev is NULL");
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  hipError_t e = hipPointerGetAttributes(&at, ctrl_dev);
  if (e != hipSuccess) (void)hipGetLastError();                // pageable host memory: an error on some runtimes, "unregistered" on others
  const bool dev_mem = e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == d->device;
  const bool pinned = e == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer == ctrl_dev;
  if (!dev_mem && !pinned)
    return fail(MJB_ERR_ARG, "mjb_rollout_ctrl: ctrl_dev is not device-accessible memory of this data object's device");
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ctrl_dev);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(MJB_ERR_ARG, "mjb_rollout_ctrl: no allocation found behind ctrl_dev"); }
  // highest element read: (nstep-1) step_stride + (batch-1) env_stride + nu-1, in 128-bit arithmetic (no overflow whatever the strides)
  const __int128 hi = (__int128)(nstep - 1) * step_stride + (__int128)(d->batch - 1) * env_stride + (nu - 1);
  const __int128 esize = d->dtype == MJB_F32 ? 4 : 8;
  const __int128 end = (__int128)(uintptr_t)ctrl_dev + (hi + 1) * esize, limit = (__int128)(uintptr_t)base + (__int128)size;
  if ((uintptr_t)ctrl_dev < (uintptr_t)base || end > limit)
    return fail(MJB_ERR_ARG, "mjb_rollout_ctrl: the control table's extent (nstep, batch, strides) lies beyond its allocation");
  return MJB_OK;
}

int mjb_rollout_ctrl(mjbData* d, int nstep, const void* ctrl_dev, long step_stride, long env_stride,
                     const mjbObsSpec* spec, void* obs_out_dev, int obs_every) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  if (nstep < 1) return fail(MJB_ERR_ARG, "nstep must be >= 1");
  if (step_stride < 0 || env_stride < 0) return fail(MJB_ERR_ARG, "mjb_rollout_ctrl: strides must be >= 0");
  HIPCHK(hipSetDevice(d->device));
  int rc = check_ctrl_table(d, nstep, ctrl_dev, step_stride, env_stride);
  if (rc != MJB_OK) return rc;
  StepArgs a = make_args(d, nstep, CTRL_SEQUENCE, 0, 0, 1.0, 0);
  a.ctrl_seq = ctrl_dev; a.ctrl_step_stride = step_stride; a.ctrl_env_stride = env_stride;
  ObsSpecDev obs; std::memset(&obs, 0, sizeof(obs));
  if (spec && obs_out_dev && obs_every > 0) { obs = spec->dev; a.obs_every = obs_every; }
  return launch(d, a, obs, obs_out_dev, false);
}

}  // extern "C"

// ---- per-environment model parameters (mjb_set_env_param) ----
namespace {
static_assert(PRM_BODY_MASS == MJB_PRM_BODY_MASS && PRM_BODY_INERTIA == MJB_PRM_BODY_INERTIA && PRM_DOF_DAMPING == MJB_PRM_DOF_DAMPING &&
              PRM_DOF_ARMATURE == MJB_PRM_DOF_ARMATURE && PRM_ACT_GEAR == MJB_PRM_ACTUATOR_GEAR && PRM_ACT_GAINPRM == MJB_PRM_ACTUATOR_GAINPRM &&
              PRM_ACT_BIASPRM == MJB_PRM_ACTUATOR_BIASPRM && PRM_GEOM_FRICTION == MJB_PRM_GEOM_FRICTION && PRM_GRAVITY == MJB_PRM_GRAVITY &&
              PRM_NFIELD == MJB_PRM_N, "mjbatch.h and mjb_types.hpp number the per-environment fields alike");
const char* const kPrmNames[PRM_NFIELD] = {"body_mass", "body_inertia", "dof_damping", "dof_armature", "actuator_gear", "actuator_gainprm",
                                           "actuator_biasprm", "geom_friction", "gravity"};

int prm_index(const char* name) {
  if (name) for (int k = 0; k < PRM_NFIELD; k++) if (!std::strcmp(name, kPrmNames[k])) return k;
  return -1;
}
// values per environment of slot k (the derived slots included)
long prm_count(const HostModel& h, int k) {
  switch (k) {
    case PRM_BODY_MASS: case PRM_SUBTREEMASS: return h.nbody;
    case PRM_BODY_INERTIA: return 3L * h.nbody;
    case PRM_DOF_DAMPING: case PRM_DOF_ARMATURE: return h.nv;
    case PRM_ACT_GEAR: return 6L * h.nu;
    case PRM_ACT_GAINPRM: case PRM_ACT_BIASPRM: return 3L * h.nu;
    case PRM_GEOM_FRICTION: return 3L * h.ngeom;
    case PRM_GRAVITY: return 3;
    default: return 5L * h.npair;                                      // PRM_PAIR_FRICTION
  }
}
// the compiled model's values of slot k (geom_friction only lives in the model table: the kernels read the pairs' friction)
bool prm_model_values(const mjbModel* m, int k, std::vector<double>& out, std::string& err) {
  const HostModel& h = m->h;
  const long n = prm_count(h, k);
  static const char* const derived[2] = {"body_subtreemass", "pair_friction"};
  if (k == PRM_GRAVITY) { out.assign(h.gravity, h.gravity + 3); return true; }
  if (k == PRM_GEOM_FRICTION) {
    for (const auto& f : m->fields)
      if (f.name == "geom_friction" && f.dtype == 0 && f.count == n) {
        const double* p = (const double*)(m->blob.data() + f.off);
        out.assign(p, p + n);
        return true;
      }
    err = "geom_friction: the model table has no float64 geom_friction [ngeom, 3]";
    return false;
  }
  out = h.D(k >= PRM_NFIELD ? derived[k - PRM_NFIELD] : kPrmNames[k]);
  if ((long)out.size() != n) { err = std::string("model field ") + kPrmNames[k < PRM_NFIELD ? k : 0] + " has the wrong size"; return false; }
  return true;
}

// Device memory the kernels will read at ptr[0 .. bytes): 0 = device memory of the data's device (or pinned host memory mapped for it)
// with an allocation behind it that covers the extent, 1 = not such memory, 2 = no allocation found, 3 = the extent lies beyond it.
// The checks of mjb_rollout_ctrl's control table.
int device_extent(const mjbData* d, const void* ptr, size_t bytes) {
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  hipError_t e = hipPointerGetAttributes(&at, ptr);
  if (e != hipSuccess) (void)hipGetLastError();
  const bool dev_mem = e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == d->device;
  const bool pinned = e == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer == ptr;
  if (!dev_mem && !pinned) return 1;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr);
  if (e != hipSuccess) { (void)hipGetLastError(); return 2; }
  const __int128 end = (__int128)(uintptr_t)ptr + (__int128)bytes, limit = (__int128)(uintptr_t)base + (__int128)size;
  if ((uintptr_t)ptr < (uintptr_t)base || end > limit) return 3;
  return 0;
}
int extent_error(int why, const std::string& what) {
  static const char* const msg[4] = {"", " is not device-accessible memory of this data object's device", ": no allocation found behind it",
                                     ": the allocation behind it is shorter than the data read"};
  return fail(MJB_ERR_ARG, "mjb_set_env_param: " + what + msg[why]);
}

// The masked rows of one field from the caller's [batch, n] block (float32 or float64) into the float64 master and the fp32 copy
// (rounded once from the float64 value, as fill_dev_model rounds the model tables).
__global__ void k_prm_set(const void* src, int src_f32, long n, int batch, const unsigned char* mask, double* dst, float* dstf) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)batch * n) return;
  if (mask && !mask[t / n]) return;
  const double v = src_f32 ? (double)((const float*)src)[t] : ((const double*)src)[t];
  dst[t] = v;
  if (dstf) dstf[t] = (float)v;
}
// body_subtreemass of the masked environments: one thread per environment, the compiler's order (leaves to the root, ids descending)
__global__ void k_prm_subtreemass(const double* mass, const int* parent, int nbody, int batch, const unsigned char* mask, double* sub, float* subf) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= batch || (mask && !mask[e])) return;
  const double* ms = mass + (size_t)e * nbody;
  double* s = sub + (size_t)e * nbody;
  for (int b = 0; b < nbody; b++) s[b] = ms[b];
  for (int b = nbody - 1; b > 0; b--) s[parent[b]] += s[b];
  if (subf) for (int b = 0; b < nbody; b++) subf[(size_t)e * nbody + b] = (float)s[b];
}
// friction of every collision pair of the masked environments: element-wise max of its two geoms', stored [f0, f0, f1, f2, f2]
__global__ void k_prm_pair_friction(const double* gf, const int* g1, const int* g2, int ngeom, int npair, int batch, const unsigned char* mask,
                                    double* pf, float* pff) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)batch * npair) return;
  const int e = (int)(t / npair), p = (int)(t - (long)e * npair);
  if (mask && !mask[e]) return;
  const double* a = gf + ((size_t)e * ngeom + g1[p]) * 3;
  const double* b = gf + ((size_t)e * ngeom + g2[p]) * 3;
  double f[3];
  for (int k = 0; k < 3; k++) f[k] = a[k] > b[k] ? a[k] : b[k];
  const double v[5] = {f[0], f[0], f[1], f[2], f[2]};
  for (int k = 0; k < 5; k++) {
    pf[(size_t)t * 5 + k] = v[k];
    if (pff) pff[(size_t)t * 5 + k] = (float)v[k];
  }
}

// the kernels' view of the rows (both DevData, so that a float32 data object's float64 FD kernel finds the masters)
void prm_publish(mjbData* d) {
  for (int k = 0; k < PRM_NSLOT; k++) {
    d->df.prm.d[k] = d->dd.prm.d[k] = (const double MJB_CONST*)d->prm_d[k].get();
    d->df.prm.f[k] = d->dd.prm.f[k] = (const float MJB_CONST*)d->prm_f[k].get();
  }
}
// After the set of batched fields changed: the specialised kernels built for another set are unloaded (the generic kernels read the
// rows of whatever is batched; a specialised one reads the rows of exactly its own fields and would fault on a missing row).
int prm_mask_changed(mjbData* d) {
  bool drain = false;
  for (int kind = 1; kind < 4; kind++) if (d->spec[kind].mod && d->spec_prm[kind] != d->prm_mask) drain = true;
  if (!drain) return MJB_OK;
  HIPCHK(hipStreamSynchronize(d->stream));
  for (int kind = 1; kind < 4; kind++) if (d->spec[kind].mod && d->spec_prm[kind] != d->prm_mask) drop_kernel(d, kind);
  return MJB_OK;
}
void prm_free(mjbData* d, int k) { reset_all(d->prm_d[k], d->prm_f[k]); }
// rows of slot k, allocated and filled with the model's values for every environment: both blocks of the slot, or neither
int prm_alloc(mjbData* d, int k) {
  const bool f32 = d->dtype == MJB_F32;
  if (d->prm_d[k].get() && (!f32 || d->prm_f[k].get())) return MJB_OK;
  std::vector<double> v;
  std::string err;
  if (!prm_model_values(d->model, k, v, err)) return fail(MJB_ERR_ARG, err);
  const size_t n = v.size(), total = (size_t)d->batch * n;
  std::vector<double> rows(total ? total : 1);
  for (size_t e = 0; e < (size_t)d->batch; e++) std::memcpy(rows.data() + e * n, v.data(), n * sizeof(double));
  const std::vector<float> rf(rows.begin(), rows.end());
  if (d->prm_d[k].reserve(rows.size()) != hipSuccess || (f32 && d->prm_f[k].reserve(rf.size()) != hipSuccess)) {
    prm_free(d, k);
    return fail(MJB_ERR_DEVICE, "device allocation of parameter rows failed");
  }
  HIPCHK(hipMemcpy(d->prm_d[k].get(), rows.data(), total * sizeof(double), hipMemcpyHostToDevice));
  if (f32) HIPCHK(hipMemcpy(d->prm_f[k].get(), rf.data(), total * sizeof(float), hipMemcpyHostToDevice));
  return MJB_OK;
}
int prm_derived(int k) { return k == PRM_BODY_MASS ? PRM_SUBTREEMASS : (k == PRM_GEOM_FRICTION ? PRM_PAIR_FRICTION : -1); }
}  // namespace

extern "C" {

int mjb_set_env_param(mjbData* d, const char* name, const void* src, int src_dtype, int src_on_device, const unsigned char* env_mask) {
  if (!d || !src) return fail(MJB_ERR_ARG, "NULL argument");
  const int k = prm_index(name);
  if (k < 0) return fail(MJB_ERR_ARG, std::string("mjb_set_env_param: unknown per-environment field '") + (name ? name : "") + "'");
  if (src_dtype != MJB_F32 && src_dtype != MJB_F64) return fail(MJB_ERR_ARG, "mjb_set_env_param: src_dtype must be MJB_F32 or MJB_F64");
  const HostModel& h = d->model->h;
  const long n = prm_count(h, k);
  const size_t total = (size_t)d->batch * (size_t)n, esize = src_dtype == MJB_F32 ? 4 : 8;
  HIPCHK(hipSetDevice(d->device));
  if (env_mask) { int why = device_extent(d, env_mask, (size_t)d->batch); if (why) return extent_error(why, "env_mask"); }
  if (src_on_device) {
    if (total) { int why = device_extent(d, src, total * esize); if (why) return extent_error(why, "src"); }
  } else {
    for (size_t i = 0; i < total; i++) {
      const double v = src_dtype == MJB_F32 ? (double)((const float*)src)[i] : ((const double*)src)[i];
      if (!std::isfinite(v)) return fail(MJB_ERR_ARG, std::string("mjb_set_env_param: ") + name + " has a value that is not finite");
    }
  }
  const int dk = prm_derived(k);
  int rc = prm_alloc(d, k);
  if (rc == MJB_OK && dk >= 0) rc = prm_alloc(d, dk);
  if (rc != MJB_OK) { prm_free(d, k); if (dk >= 0) prm_free(d, dk); return rc; }
  if (total == 0) { d->prm_mask |= 1 << k; prm_publish(d); return prm_mask_changed(d); }
  const void* from = src;
  int from_f32 = src_dtype == MJB_F32;
  if (!src_on_device) {                                        // host memory: through the pinned block to a device stage, read before return
    const size_t bytes = total * sizeof(double);
    HIPCHK(d->io_pin.reserve(bytes, true));
    if (d->prm_stage.count() < total) {
      if (d->prm_stage.get()) HIPCHK(hipStreamSynchronize(d->stream));   // kernels already queued may still read the old stage
      HIPCHK(d->prm_stage.reserve(total));
    }
    double* pin = (double*)d->io_pin.get();
    for (size_t i = 0; i < total; i++) pin[i] = src_dtype == MJB_F32 ? (double)((const float*)src)[i] : ((const double*)src)[i];
    HIPCHK(hipMemcpyAsync(d->prm_stage.get(), pin, bytes, hipMemcpyHostToDevice, d->stream));
    from = d->prm_stage.get(); from_f32 = 0;
  }
  const int threads = 256;
  hipLaunchKernelGGL(k_prm_set, dim3((unsigned)((total + threads - 1) / threads)), dim3(threads), 0, d->stream, from, from_f32, n, d->batch,
                     env_mask, d->prm_d[k].get(), d->prm_f[k].get());
  HIPCHK(hipGetLastError());
  if (k == PRM_BODY_MASS)
    hipLaunchKernelGGL(k_prm_subtreemass, dim3((unsigned)((d->batch + 63) / 64)), dim3(64), 0, d->stream, d->prm_d[k].get(), d->md.body_parentid, h.nbody,
                       d->batch, env_mask, d->prm_d[PRM_SUBTREEMASS].get(), d->prm_f[PRM_SUBTREEMASS].get());
  else if (k == PRM_GEOM_FRICTION && h.npair > 0) {
    const size_t np = (size_t)d->batch * h.npair;
    hipLaunchKernelGGL(k_prm_pair_friction, dim3((unsigned)((np + threads - 1) / threads)), dim3(threads), 0, d->stream, d->prm_d[k].get(), d->md.pair_geom1,
                       d->md.pair_geom2, h.ngeom, h.npair, d->batch, env_mask, d->prm_d[PRM_PAIR_FRICTION].get(), d->prm_f[PRM_PAIR_FRICTION].get());
  }
  HIPCHK(hipGetLastError());
  if (!src_on_device) HIPCHK(hipStreamSynchronize(d->stream));            // the pinned block is free again on return
  const int before = d->prm_mask;
  d->prm_mask |= 1 << k;
  prm_publish(d);
  return d->prm_mask != before ? prm_mask_changed(d) : MJB_OK;
}

int mjb_get_env_param(mjbData* d, const char* name, double* host_out) {
  if (!d || !host_out) return fail(MJB_ERR_ARG, "NULL argument");
  const int k = prm_index(name);
  if (k < 0) return fail(MJB_ERR_ARG, std::string("mjb_get_env_param: unknown per-environment field '") + (name ? name : "") + "'");
  const long n = prm_count(d->model->h, k);
  if (!d->prm_d[k].get()) {
    std::vector<double> v;
    std::string err;
    if (!prm_model_values(d->model, k, v, err)) return fail(MJB_ERR_ARG, err);
    for (size_t e = 0; e < (size_t)d->batch; e++) std::memcpy(host_out + e * n, v.data(), n * sizeof(double));
    return MJB_OK;
  }
  HIPCHK(hipSetDevice(d->device));
  return copy_out(d, ArrayInfo{d->prm_d[k].get(), n, 1}, host_out);
}

int mjb_clear_env_param(mjbData* d, const char* name) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  const int k = prm_index(name);
  if (k < 0) return fail(MJB_ERR_ARG, std::string("mjb_clear_env_param: unknown per-environment field '") + (name ? name : "") + "'");
  if (!d->prm_d[k].get()) return MJB_OK;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipStreamSynchronize(d->stream));                     // launches already queued read these rows
  prm_free(d, k);
  if (prm_derived(k) >= 0) prm_free(d, prm_derived(k));
  d->prm_mask &= ~(1 << k);
  prm_publish(d);
  return prm_mask_changed(d);
}

int mjb_env_param_mask(mjbData* d, int* mask) {
  if (!d || !mask) return fail(MJB_ERR_ARG, "NULL argument");
  *mask = d->prm_mask;
  return MJB_OK;
}

int mjb_set_feedback(mjbData* d, const double* K, const double* u0, const double* q0, const double* v0) {
  if (!d || !K || !u0 || !q0) return fail(MJB_ERR_ARG, "NULL argument");
  const HostModel& h = d->model->h;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipStreamSynchronize(d->stream));
  const size_t n[4] = {(size_t)h.nu * 2 * h.nv, (size_t)h.nu, (size_t)h.nq, (size_t)h.nv};
  const double* src[4] = {K, u0, q0, v0};
  for (int k = 0; k < 4; k++) {
    if (reserve_zeroed(d->fbd[k], n[k] ? n[k] : 1) != hipSuccess || reserve_zeroed(d->fbf[k], n[k] ? n[k] : 1) != hipSuccess) {
      for (int j = 0; j < 4; j++) reset_all(d->fbd[j], d->fbf[j]);   // all eight blocks or none (an empty array still gets one element)
      return fail(MJB_ERR_DEVICE, "device allocation of feedback gains failed");
    }
    std::vector<double> vd(n[k], 0.0);
    if (src[k]) vd.assign(src[k], src[k] + n[k]);
    std::vector<float> vf(vd.begin(), vd.end());
    if (n[k]) {
      HIPCHK(hipMemcpy(d->fbd[k].get(), vd.data(), n[k] * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d->fbf[k].get(), vf.data(), n[k] * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  return MJB_OK;
}


int mjb_set_feedback_noise(mjbData* d, const double* noise_std, const double* noise_table, int nsteps, int env_stride) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  d->fb_env_stride = env_stride;
  if (!noise_std || !noise_table || nsteps < 1) { d->fb_nsteps = 0; return MJB_OK; }      // switch the noise term off
  const HostModel& h = d->model->h;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipStreamSynchronize(d->stream));
  const size_t n[2] = {(size_t)h.nu, (size_t)nsteps * h.nu};
  const double* src[2] = {noise_std, noise_table};
  d->fb_nsteps = 0;                                            // until the new table is complete
  for (int k = 0; k < 2; k++) {
    // the previous table's blocks are reused when large enough, else replaced (the stream has drained: no kernel still reads them)
    if (d->fb_noise_d[k].reserve(n[k] ? n[k] : 1) != hipSuccess || d->fb_noise_f[k].reserve(n[k] ? n[k] : 1) != hipSuccess) {
      reset_all(d->fb_noise_d[0], d->fb_noise_f[0], d->fb_noise_d[1], d->fb_noise_f[1]);
      return fail(MJB_ERR_DEVICE, "device allocation of the feedback noise failed");
    }
    std::vector<float> vf(src[k], src[k] + n[k]);
    HIPCHK(hipMemcpy(d->fb_noise_d[k].get(), src[k], n[k] * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d->fb_noise_f[k].get(), vf.data(), n[k] * sizeof(float), hipMemcpyHostToDevice));
  }
  d->fb_nsteps = nsteps;
  return MJB_OK;
}

int mjb_feedback_ctrl(mjbData* d, int step) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  if (!d->fbd[0].get()) return fail(MJB_ERR_ARG, "mjb_feedback_ctrl needs mjb_set_feedback() first");
  const HostModel& h = d->model->h;
  if (h.nu == 0) return MJB_OK;
  HIPCHK(hipSetDevice(d->device));
  { int rc0 = refresh_options(d); if (rc0 != MJB_OK) return rc0; }
  FeedbackArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nsteps = d->fb_nsteps; a.step = step; a.env_stride = d->fb_env_stride;
  if (d->dtype == MJB_F32) {
    a.K = d->fbf[0].get(); a.u0 = d->fbf[1].get(); a.q0 = d->fbf[2].get(); a.v0 = d->fbf[3].get();
    if (d->fb_nsteps > 0) { a.noise_std = d->fb_noise_f[0].get(); a.noise_tab = d->fb_noise_f[1].get(); }
    const int kpad = (2 * h.nv + 1) & ~1;
    const size_t shmem = (size_t)32 * kpad * sizeof(float);
    if (shmem > 64 * 1024) return fail(MJB_ERR_ARG, "mjb_feedback_ctrl: 2 nv too large for the LDS tile");
    hipLaunchKernelGGL(k_feedback_mfma<0>, dim3((unsigned)((d->batch + 31) / 32)), dim3(64), shmem, d->stream, (const DevModel<float>*)d->mf_dev, d->df, a);
  } else {
    a.K = d->fbd[0].get(); a.u0 = d->fbd[1].get(); a.q0 = d->fbd[2].get(); a.v0 = d->fbd[3].get();
    if (d->fb_nsteps > 0) { a.noise_std = d->fb_noise_d[0].get(); a.noise_tab = d->fb_noise_d[1].get(); }
    if (reserve_zeroed(d->fb_dx, (size_t)d->batch * 2 * h.nv) != hipSuccess) return fail(MJB_ERR_DEVICE, "device allocation of the feedback scratch failed");
    hipLaunchKernelGGL(k_feedback_simple<double>, dim3((unsigned)d->batch), dim3(64), 0, d->stream, (const DevModel<double>*)d->md_dev, d->dd, a, d->fb_dx.get());
  }
  HIPCHK(hipGetLastError());
  return MJB_OK;
}

int mjb_obs_spec_create(mjbData* d, int flags, int nsite, const int* site_ids, int nbody, const int* body_ids,
                        int ngeom, const int* geom_ids, int nsubtree, const int* subtree_ids, mjbObsSpec** out) {
  if (!d || !out) return fail(MJB_ERR_ARG, "NULL argument");
  const HostModel& h = d->model->h;
  for (int i = 0; i < nsite; i++) if (site_ids[i] < 0 || site_ids[i] >= h.nsite) return fail(MJB_ERR_LOOKUP, "site id out of range");
  for (int i = 0; i < nbody; i++) if (body_ids[i] < 0 || body_ids[i] >= h.nbody) return fail(MJB_ERR_LOOKUP, "body id out of range");
  for (int i = 0; i < ngeom; i++) if (geom_ids[i] < 0 || geom_ids[i] >= h.ngeom) return fail(MJB_ERR_LOOKUP, "geom id out of range");
  for (int i = 0; i < nsubtree; i++) if (subtree_ids[i] < 0 || subtree_ids[i] >= h.nbody) return fail(MJB_ERR_LOOKUP, "subtree body id out of range");
  HIPCHK(hipSetDevice(d->device));
  mjbObsSpec* s = new mjbObsSpec();
  std::memset(&s->dev, 0, sizeof(s->dev));
  auto up = [&](const int* ids, int n) -> const int* {
    int* p = s->arena.alloc<int>(n > 0 ? n : 0);
    if (p && n > 0 && hipMemcpy(p, ids, sizeof(int) * n, hipMemcpyHostToDevice) != hipSuccess) s->arena.ok = false;
    return p;
  };
  s->dev.flags = flags; s->dev.nsite = nsite; s->dev.nbody = nbody; s->dev.ngeom = ngeom; s->dev.nsubtree = nsubtree;
  s->dev.site_ids = up(site_ids, nsite); s->dev.body_ids = up(body_ids, nbody); s->dev.geom_ids = up(geom_ids, ngeom); s->dev.subtree_ids = up(subtree_ids, nsubtree);
  if (!s->arena.ok) { delete s; return fail(MJB_ERR_DEVICE, "device upload of the observation id tables failed"); }
  int dim = 3 * (nsite + nbody + ngeom + nsubtree);
  if (flags & 1) dim += h.nq;
  if (flags & 2) dim += h.nv;
  if (flags & 4) dim += h.nu;
  if (flags & 8) dim += h.nsensordata;
  if (flags & 16) dim += 1;
  if (flags & 128) dim += h.nv;
  s->dev.dim = dim;
  *out = s;
  return MJB_OK;
}

void mjb_obs_spec_free(mjbObsSpec* s) { delete s; }

int mjb_obs_dim(const mjbObsSpec* s) { return s ? s->dev.dim : -1; }

int mjb_obs_gather(mjbData* d, const mjbObsSpec* s, void* out_dev) {
  if (!d || !s || !out_dev) return fail(MJB_ERR_ARG, "NULL argument");
  const HostModel& h = d->model->h;
  HIPCHK(hipSetDevice(d->device));
  if (d->dtype == MJB_F32)
    hipLaunchKernelGGL(k_obs<float>, dim3(d->batch), dim3(64), 0, d->stream, d->df, h.nq, h.nv, h.nu, h.nbody, h.ngeom, h.nsite, h.nsensordata, s->dev, (float*)out_dev);
  else
    hipLaunchKernelGGL(k_obs<double>, dim3(d->batch), dim3(64), 0, d->stream, d->dd, h.nq, h.nv, h.nu, h.nbody, h.ngeom, h.nsite, h.nsensordata, s->dev, (double*)out_dev);
  HIPCHK(hipGetLastError());
  return MJB_OK;
}

// Scratch budget of one slab of mjb_transition_fd_points (the per-column next states, fd_y): 66 KB per humanoid point, so ~2 000 points
// per launch - several times what fills the chip.  MJB_FD_SLAB_BYTES overrides it (tests).
static const unsigned long long kFdSlabBytes = 128ull << 20;

// fd_y / fd_valid for `npoint` points: allocated once per data object and grown only when a larger slab comes
// (fd_s, the per-column sensordata, only for a call that asks for the sensor Jacobians)
static int fd_scratch(mjbData* d, size_t npoint, int ncol, bool sensors = false) {
  const HostModel& h = d->model->h;
  const size_t ny = npoint * ncol * (size_t)(h.nq + h.nv), nvalid = npoint * ncol, ns = sensors ? npoint * ncol * (size_t)h.nsensordata : 0;
  if (ny <= d->fd_y.count() && nvalid <= d->fd_valid.count() && ns <= d->fd_s.count()) return MJB_OK;
  // reserve releases the old blocks through hipFree, which waits for the kernels that may still read them
  if (d->fd_y.reserve(ny) != hipSuccess || d->fd_valid.reserve(nvalid) != hipSuccess || (ns > 0 && d->fd_s.reserve(ns) != hipSuccess)) {
    (void)hipGetLastError(); reset_all(d->fd_y, d->fd_valid, d->fd_s);
    return fail(MJB_ERR_DEVICE, "device allocation of FD scratch failed");
  }
  return MJB_OK;
}

// The scratch is one block per data object and mjb_transition_fd_points does not synchronise: when the data's stream has changed
// since the last FD launch (mjb_set_stream), the new stream first waits for that launch's event, so two calls never share the scratch.
static int fd_order_begin(mjbData* d) {
  if (d->fd_pending && d->fd_stream != d->stream) HIPCHK(hipStreamWaitEvent(d->stream, d->fd_done, 0));
  return MJB_OK;
}
static int fd_order_end(mjbData* d) {
  if (!d->fd_done) HIPCHK(hipEventCreateWithFlags(&d->fd_done, hipEventDisableTiming));
  HIPCHK(hipEventRecord(d->fd_done, d->stream));
  d->fd_stream = d->stream; d->fd_pending = true;
  return MJB_OK;
}

// One slab of points (pt.p0, pt.npoint set): the column kernel, then the combine kernel into the slab's (A, B) blocks; enqueued only.
// C non-null (nsensordata > 0): the column kernel also keeps every column's sensordata, and a second combine kernel writes the slab's (C, D).
static int fd_run_slab(mjbData* d, const FdPoints& pt_in, double eps, int centered, double* A, double* B, double* C = nullptr, double* D = nullptr) {
  const HostModel& h = d->model->h;
  const int nin = 2 * h.nv + h.nu, ncol = 1 + 2 * nin;
  const bool sensors = C != nullptr && h.nsensordata > 0;
  { int rc = fd_scratch(d, (size_t)pt_in.npoint, ncol, sensors); if (rc != MJB_OK) return rc; }
  FdPoints pt = pt_in;
  pt.sens_out = sensors ? d->fd_s.get() : nullptr;
  // columns per job (k_fd shares the stages a chunk of columns cannot change), sized by the points of THIS launch
  int chunk;
  {
    const size_t per_wg = (size_t)(64 / d->cfg.G_fd) * (size_t)d->cfg.Ld.bytes;
    size_t wg_per_cu = per_wg ? (size_t)160 * 1024 / per_wg : 8;
    if (wg_per_cu > 32) wg_per_cu = 32;
    if (wg_per_cu < 1) wg_per_cu = 1;
    const long slots = (long)wg_per_cu * d->ncu * (64 / d->cfg.G_fd);
    if (const char* e = std::getenv("MJB_FD_CHUNK")) chunk = std::atoi(e);        // experiments (scripts/gpu_fd_timing.py)
    else chunk = fd_chunk_rule(pt.npoint, ncol, slots);
    if (chunk < 1) chunk = 1;
  }
  hipError_t e;
  // per-model specialised kernel: same arguments, same grid as launch_fd_g.  A code object compiled before the point table had a sensor
  // output (mjb_kernel_load) would not store the sensors: such a request runs on the generic kernel, whose results are the same
  if (d->spec[MJB_KERNEL_FD].fn && (!sensors || d->spec_fd_sensors)) {
    const int epb = 64 / d->cfg.G_fd;
    const int njob = (1 + 2 * h.nu + chunk - 1) / chunk + (2 * h.nv + chunk - 1) / chunk + 2 * h.nv;
    const long ngroups = (long)pt.npoint * njob;
    const DevModel<double>* mg = d->md_dev; const Lay* lg = d->Ld_dev;
    DevData<float> dvf = d->df; DevData<double> dvd = d->dd;
    int ncol_ = ncol, cv = chunk, cc = chunk; double eps_ = eps; double* yy = d->fd_y.get(); int* vv = d->fd_valid.get(); FdPoints pp = pt;
    void* args[] = {(void*)&mg, (void*)&lg, d->dtype == MJB_F32 ? (void*)&dvf : (void*)&dvd, (void*)&ncol_, (void*)&eps_, (void*)&yy, (void*)&vv, (void*)&cv, (void*)&cc, (void*)&pp};
    e = hipModuleLaunchKernel(d->spec[MJB_KERNEL_FD].fn, (unsigned)((ngroups + epb - 1) / epb), 1, 1, 64, 1, 1, (unsigned)((size_t)epb * d->cfg.Ld.bytes), d->stream, args, nullptr);
  } else
  e = d->dtype == MJB_F32 ? launch_fd<double, float>(d->cfg.G_fd, d->md_dev, d->Ld_dev, d->cfg.Ld, d->df, pt, ncol, h.nv, h.nu, chunk, eps, d->fd_y.get(), d->fd_valid.get(), d->stream)
                          : launch_fd<double, double>(d->cfg.G_fd, d->md_dev, d->Ld_dev, d->cfg.Ld, d->dd, pt, ncol, h.nv, h.nu, chunk, eps, d->fd_y.get(), d->fd_valid.get(), d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("fd launch: ") + hipGetErrorString(e));
  const long nthreads = (long)pt.npoint * nin;
  hipLaunchKernelGGL(k_fd_combine<double>, dim3((unsigned)((nthreads + 127) / 128)), dim3(128), 0, d->stream, (const DevModel<double>*)d->md_dev, pt.npoint, ncol, centered, eps,
                     (const double*)d->fd_y.get(), (const int*)d->fd_valid.get(), A, B);
  HIPCHK(hipGetLastError());
  if (sensors) {
    hipLaunchKernelGGL(k_fd_combine_sensors<double>, dim3((unsigned)((nthreads + 127) / 128)), dim3(128), 0, d->stream, (const DevModel<double>*)d->md_dev, pt.npoint, ncol, centered,
                       eps, (const double*)d->fd_s.get(), (const int*)d->fd_valid.get(), C, D);
    HIPCHK(hipGetLastError());
  }
  return MJB_OK;
}

static int transition_fd_impl(mjbData* d, double eps, int centered, bool sensors = false) {
  if (!d) return fail(MJB_ERR_ARG, "NULL argument");
  if (!(eps > 0)) return fail(MJB_ERR_ARG, "eps must be > 0");
  const HostModel& h = d->model->h;
  HIPCHK(hipSetDevice(d->device));
  { int rc0 = refresh_options(d); if (rc0 != MJB_OK) return rc0; }
  const int nx = 2 * h.nv;
  size_t B = (size_t)d->batch;
  const size_t nA = B * nx * nx, nB = B * nx * (h.nu > 0 ? h.nu : 1);
  if (reserve_zeroed(d->fd_A, nA) != hipSuccess || reserve_zeroed(d->fd_B, nB) != hipSuccess ||          // the four result blocks together
      d->fd_A_host.reserve(nA) != hipSuccess || d->fd_B_host.reserve(nB) != hipSuccess) {
    reset_all(d->fd_A, d->fd_B, d->fd_A_host, d->fd_B_host);
    return fail(MJB_ERR_DEVICE, "device allocation of FD scratch failed");
  }
  const size_t ns = (size_t)h.nsensordata, nC = B * ns * nx, nD = B * ns * (h.nu > 0 ? h.nu : 1);
  sensors = sensors && ns > 0;
  if (sensors && (reserve_zeroed(d->fd_C, nC) != hipSuccess || reserve_zeroed(d->fd_D, nD) != hipSuccess ||
                  d->fd_C_host.reserve(nC) != hipSuccess || d->fd_D_host.reserve(nD) != hipSuccess)) {
    reset_all(d->fd_C, d->fd_D, d->fd_C_host, d->fd_D_host);
    return fail(MJB_ERR_DEVICE, "device allocation of FD scratch failed");
  }
  // the point table of T = 1 over the data's own arrays: point e = environment e, one slab
  FdPoints pt;
  std::memset(&pt, 0, sizeof(pt));
  if (d->dtype == MJB_F32) { pt.qpos = d->df.qpos; pt.qvel = d->df.qvel; pt.ctrl = d->df.ctrl; pt.warmstart = d->df.qacc_warmstart; }
  else { pt.qpos = d->dd.qpos; pt.qvel = d->dd.qvel; pt.ctrl = d->dd.ctrl; pt.warmstart = d->dd.qacc_warmstart; }
  pt.qpos_es = h.nq; pt.qvel_es = h.nv; pt.ctrl_es = h.nu; pt.ws_es = h.nv;
  pt.p0 = 0; pt.npoint = d->batch;
  // a few environments (the reference's batch-1 loops with needs_linearization controllers): the combine kernel writes (A, B) straight
  // into the pinned result blocks (device-visible) - no staging copies; larger batches keep the device blocks + one async copy each
  // (the rule looks at (A, B) alone, so that asking for the sensors does not move them)
  const bool zero_copy = B * nx * (nx + (size_t)h.nu) * sizeof(double) <= (size_t)256 * 1024;
  { int rc = fd_order_begin(d); if (rc != MJB_OK) return rc; }
  { int rc = fd_run_slab(d, pt, eps, centered, zero_copy ? d->fd_A_host.get() : d->fd_A.get(), zero_copy ? d->fd_B_host.get() : d->fd_B.get(),
                         !sensors ? nullptr : zero_copy ? d->fd_C_host.get() : d->fd_C.get(), !sensors ? nullptr : zero_copy ? d->fd_D_host.get() : d->fd_D.get());
    if (rc != MJB_OK) return rc; }
  if (!zero_copy) {
    HIPCHK(hipMemcpyAsync(d->fd_A_host.get(), d->fd_A.get(), B * nx * nx * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if (h.nu > 0) HIPCHK(hipMemcpyAsync(d->fd_B_host.get(), d->fd_B.get(), B * nx * h.nu * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if (sensors) HIPCHK(hipMemcpyAsync(d->fd_C_host.get(), d->fd_C.get(), B * ns * nx * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if (sensors && h.nu > 0) HIPCHK(hipMemcpyAsync(d->fd_D_host.get(), d->fd_D.get(), B * ns * h.nu * sizeof(double), hipMemcpyDeviceToHost, d->stream));
  }
  HIPCHK(hipStreamSynchronize(d->stream));
  d->fd_pending = false;                                       // this stream has drained, and every earlier FD launch was ordered before it
  return MJB_OK;
}

// One strided [T, batch, n] input or output of mjb_transition_fd_points, checked as mjb_rollout_ctrl checks its control table
static int check_fd_array(const mjbData* d, const char* what, const void* ptr, bool may_be_null, long T, long n, long ss, long es, size_t esize) {
  const std::string pre = std::string("mjb_transition_fd_points: ") + what;
  if (ss < 0 || es < 0) return fail(MJB_ERR_ARG, pre + ": strides must be >= 0");
  if (n == 0) return MJB_OK;                                    // nothing is read: NULL allowed
  if (!ptr) return may_be_null ? MJB_OK : fail(MJB_ERR_ARG, pre + " is NULL");
  __int128 hi;
  if (!fd_highest_element(T, d->batch, n, ss, es, hi)) return fail(MJB_ERR_ARG, pre + ": bad extent");
  if (hi + 1 > ((__int128)1 << 60)) return fail(MJB_ERR_ARG, pre + ": the extent (T, batch, strides) lies beyond its allocation");
  const int why = device_extent(d, ptr, (size_t)(hi + 1) * esize);
  static const char* const msg[4] = {"", " is not device-accessible memory of this data object's device", ": no allocation found behind it",
                                     ": the extent (T, batch, strides) lies beyond its allocation"};
  return why ? fail(MJB_ERR_ARG, pre + msg[why]) : MJB_OK;
}

static int transition_fd_points_impl(mjbData* d, int T, const void* qpos, long qpos_step_stride, long qpos_env_stride,
                                     const void* qvel, long qvel_step_stride, long qvel_env_stride,
                                     const void* ctrl, long ctrl_step_stride, long ctrl_env_stride,
                                     const void* qacc_warmstart, long ws_step_stride, long ws_env_stride,
                                     double eps, int centered, double* A_dev, double* B_dev, bool sensors, double* C_dev, double* D_dev) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  if (T < 1) return fail(MJB_ERR_ARG, "mjb_transition_fd_points: T must be >= 1");
  if (!(eps > 0)) return fail(MJB_ERR_ARG, "eps must be > 0");
  const HostModel& h = d->model->h;
  const long npoint = (long)T * d->batch;
  if (npoint > 0x7fffffffL) return fail(MJB_ERR_ARG, "mjb_transition_fd_points: T * batch must fit 31 bits");
  HIPCHK(hipSetDevice(d->device));
  const size_t es = d->dtype == MJB_F32 ? 4 : 8;
  const long nx = 2L * h.nv;
  int rc;
  if ((rc = check_fd_array(d, "qpos", qpos, false, T, h.nq, qpos_step_stride, qpos_env_stride, es)) != MJB_OK) return rc;
  if ((rc = check_fd_array(d, "qvel", qvel, false, T, h.nv, qvel_step_stride, qvel_env_stride, es)) != MJB_OK) return rc;
  if ((rc = check_fd_array(d, "ctrl", ctrl, false, T, h.nu, ctrl_step_stride, ctrl_env_stride, es)) != MJB_OK) return rc;
  if ((rc = check_fd_array(d, "qacc_warmstart", qacc_warmstart, true, T, h.nv, ws_step_stride, ws_env_stride, es)) != MJB_OK) return rc;
  if ((rc = check_fd_array(d, "A_dev", A_dev, false, T, nx * nx, (long)d->batch * nx * nx, nx * nx, 8)) != MJB_OK) return rc;
  if ((rc = check_fd_array(d, "B_dev", B_dev, false, T, nx * h.nu, (long)d->batch * nx * h.nu, nx * h.nu, 8)) != MJB_OK) return rc;
  const long ns = h.nsensordata;
  if (sensors) {
    if ((rc = check_fd_array(d, "C_dev", C_dev, false, T, ns * nx, (long)d->batch * ns * nx, ns * nx, 8)) != MJB_OK) return rc;
    if ((rc = check_fd_array(d, "D_dev", D_dev, false, T, ns * h.nu, (long)d->batch * ns * h.nu, ns * h.nu, 8)) != MJB_OK) return rc;
    sensors = ns > 0;                                           // no sensors in the model: nothing to write, the plain call
  }
  if ((rc = refresh_options(d)) != MJB_OK) return rc;
  FdPoints pt;
  std::memset(&pt, 0, sizeof(pt));
  pt.qpos = qpos; pt.qvel = qvel; pt.ctrl = ctrl; pt.warmstart = qacc_warmstart;
  pt.qpos_ss = qpos_step_stride; pt.qpos_es = qpos_env_stride; pt.qvel_ss = qvel_step_stride; pt.qvel_es = qvel_env_stride;
  pt.ctrl_ss = ctrl_step_stride; pt.ctrl_es = ctrl_env_stride; pt.ws_ss = ws_step_stride; pt.ws_es = ws_env_stride;
  unsigned long long budget = kFdSlabBytes;
  if (const char* e = std::getenv("MJB_FD_SLAB_BYTES")) { const long long v = std::atoll(e); if (v > 0) budget = (unsigned long long)v; }
  const long per_slab = fd_slab_points(fd_point_scratch_bytes(h.nq, h.nv, h.nu, sensors ? h.nsensordata : 0), budget);
  const long nslab = fd_slab_count(npoint, per_slab);
  // the scratch of the largest slab, once, before anything is launched: growing it (the first call included) frees the old block, and
  // hipFree waits for the device - the one case in which this call synchronises
  if ((rc = fd_scratch(d, (size_t)(npoint < per_slab ? npoint : per_slab), 1 + 2 * (2 * h.nv + h.nu), sensors)) != MJB_OK) return rc;
  if ((rc = fd_order_begin(d)) != MJB_OK) return rc;
  for (long k = 0; k < nslab; k++) {                            // slab after slab on the stream: the scratch is reused in stream order
    long p0 = 0, n = 0;
    fd_slab(npoint, per_slab, k, p0, n);
    pt.p0 = (int)p0; pt.npoint = (int)n;
    rc = fd_run_slab(d, pt, eps, centered, A_dev + (size_t)p0 * nx * nx, B_dev ? B_dev + (size_t)p0 * nx * h.nu : nullptr,
                     sensors ? C_dev + (size_t)p0 * ns * nx : nullptr, sensors && D_dev ? D_dev + (size_t)p0 * ns * h.nu : nullptr);
    if (rc != MJB_OK) return rc;
  }
  d->last_fd_slabs = (int)nslab;
  return fd_order_end(d);
}

int mjb_transition_fd_points(mjbData* d, int T, const void* qpos, long qpos_step_stride, long qpos_env_stride,
                             const void* qvel, long qvel_step_stride, long qvel_env_stride,
                             const void* ctrl, long ctrl_step_stride, long ctrl_env_stride,
                             const void* qacc_warmstart, long ws_step_stride, long ws_env_stride,
                             double eps, int centered, double* A_dev, double* B_dev) {
  return transition_fd_points_impl(d, T, qpos, qpos_step_stride, qpos_env_stride, qvel, qvel_step_stride, qvel_env_stride, ctrl, ctrl_step_stride, ctrl_env_stride,
                                   qacc_warmstart, ws_step_stride, ws_env_stride, eps, centered, A_dev, B_dev, false, nullptr, nullptr);
}

int mjb_transition_fd_points_sensors(mjbData* d, int T, const void* qpos, long qpos_step_stride, long qpos_env_stride,
                                     const void* qvel, long qvel_step_stride, long qvel_env_stride,
                                     const void* ctrl, long ctrl_step_stride, long ctrl_env_stride,
                                     const void* qacc_warmstart, long ws_step_stride, long ws_env_stride,
                                     double eps, int centered, double* A_dev, double* B_dev, double* C_dev, double* D_dev) {
  return transition_fd_points_impl(d, T, qpos, qpos_step_stride, qpos_env_stride, qvel, qvel_step_stride, qvel_env_stride, ctrl, ctrl_step_stride, ctrl_env_stride,
                                   qacc_warmstart, ws_step_stride, ws_env_stride, eps, centered, A_dev, B_dev, true, C_dev, D_dev);
}

int mjb_fd_points_slabs(const mjbData* d) { return d ? d->last_fd_slabs : -1; }

// ---- mjb_lqr_backward / mjb_lqr_backward_box / mjb_lqr_candidates: the checks; the kernels and their launches are in mjb_lqr.hip ----
// One strided float64 (or esize-byte) array of `n` elements per (t, e), T x B blocks: pointer, strides, extent
static int check_lqr_array(const mjbData* d, const char* fn, const char* what, const void* ptr, bool may_be_null, long T, long B, long n,
                           long ss, long es, size_t esize = 8) {
  const std::string pre = std::string(fn) + ": " + what;
  if (ss < 0 || es < 0) return fail(MJB_ERR_ARG, pre + ": strides must be >= 0");
  if (!ptr) return may_be_null ? MJB_OK : fail(MJB_ERR_ARG, pre + " is NULL");
  __int128 hi;
  if (!lqr_highest_element(T, B, n, ss, es, hi)) return fail(MJB_ERR_ARG, pre + ": bad extent");
  if (hi + 1 > ((__int128)1 << 60)) return fail(MJB_ERR_ARG, pre + ": the extent (T, batch, strides) lies beyond its allocation");
  const int why = device_extent(d, ptr, (size_t)(hi + 1) * esize);
  static const char* const msg[4] = {"", " is not device-accessible memory of this data object's device", ": no allocation found behind it",
                                     ": the extent (T, batch, strides) lies beyond its allocation"};
  return why ? fail(MJB_ERR_ARG, pre + msg[why]) : MJB_OK;
}
static int check_lqr_sizes(const char* fn, long T, long B, long nx, long nu) {
  static const char* const msg[6] = {"", ": T must be >= 1", ": batch must be >= 1", ": nx must lie in [1, 64] (the state the kernel keeps in LDS)",
                                     ": nu must lie in [1, 32]", ": T * batch * nu * nx is too large"};
  const int why = lqr_size_error(T, B, nx, nu);
  return why ? fail(MJB_ERR_ARG, std::string(fn) + msg[why]) : MJB_OK;
}
static LqrStrided lqr_arr(const mjbStrided& s) { LqrStrided r; r.p = s.ptr; r.ss = s.step_stride; r.es = s.env_stride; return r; }

int mjb_lqr_backward(mjbData* d, const mjbLqrBackward* p) {
  static const char* fn = "mjb_lqr_backward";
  if (!d || !p) return fail(MJB_ERR_ARG, "mjb_lqr_backward: NULL argument");
  int rc;
  if ((rc = check_lqr_sizes(fn, p->T, p->batch, p->nx, p->nu)) != MJB_OK) return rc;
  HIPCHK(hipSetDevice(d->device));
  const long T = p->T, B = p->batch, nx = p->nx, nu = p->nu;
  const struct { const char* what; const mjbStrided* s; long n; bool opt; } in[] = {
      {"A", &p->A, nx * nx, false}, {"B", &p->B, nx * nu, false}, {"lx", &p->lx, nx, false}, {"lu", &p->lu, nu, false},
      {"lxx", &p->lxx, nx * nx, false}, {"luu", &p->luu, nu * nu, false}, {"lux", &p->lux, nu * nx, true}};
  for (const auto& a : in)
    if ((rc = check_lqr_array(d, fn, a.what, a.s->ptr, a.opt, T, B, a.n, a.s->step_stride, a.s->env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "VxT", p->VxT.ptr, false, 1, B, nx, 0, p->VxT.env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "VxxT", p->VxxT.ptr, false, 1, B, nx * nx, 0, p->VxxT.env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "mu", p->mu.ptr, false, 1, B, 1, 0, p->mu.env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "k", p->k, false, T, B, nu, B * nu, nu)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "K", p->K, false, T, B, nu * nx, B * nu * nx, nu * nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "dV", p->dV, false, 1, B, 2, 0, 2)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "V0x", p->V0x, true, 1, B, nx, 0, nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "V0xx", p->V0xx, true, 1, B, nx * nx, 0, nx * nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "status", p->status, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  LqrBackwardArgs a;
  a.T = p->T; a.B = p->batch; a.nx = p->nx; a.nu = p->nu;
  a.A = lqr_arr(p->A); a.Bm = lqr_arr(p->B); a.lx = lqr_arr(p->lx); a.lu = lqr_arr(p->lu); a.lxx = lqr_arr(p->lxx); a.luu = lqr_arr(p->luu);
  a.lux = lqr_arr(p->lux); a.VxT = lqr_arr(p->VxT); a.VxxT = lqr_arr(p->VxxT); a.mu = lqr_arr(p->mu);
  a.k = p->k; a.K = p->K; a.dV = p->dV; a.V0x = p->V0x; a.V0xx = p->V0xx; a.status = p->status;
  const hipError_t e = lqr_launch_backward(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_lqr_backward launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

int mjb_lqr_backward_box(mjbData* d, const mjbLqrBackwardBox* q) {
  static const char* fn = "mjb_lqr_backward_box";
  if (!d || !q) return fail(MJB_ERR_ARG, "mjb_lqr_backward_box: NULL argument");
  const mjbLqrBackward* p = &q->base;
  int rc;
  if ((rc = check_lqr_sizes(fn, p->T, p->batch, p->nx, p->nu)) != MJB_OK) return rc;
  HIPCHK(hipSetDevice(d->device));
  const long T = p->T, B = p->batch, nx = p->nx, nu = p->nu;
  const struct { const char* what; const mjbStrided* s; long n; bool opt; } in[] = {
      {"A", &p->A, nx * nx, false}, {"B", &p->B, nx * nu, false}, {"lx", &p->lx, nx, false}, {"lu", &p->lu, nu, false},
      {"lxx", &p->lxx, nx * nx, false}, {"luu", &p->luu, nu * nu, false}, {"lux", &p->lux, nu * nx, true}, {"u", &q->u, nu, false}};
  for (const auto& a : in)
    if ((rc = check_lqr_array(d, fn, a.what, a.s->ptr, a.opt, T, B, a.n, a.s->step_stride, a.s->env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "VxT", p->VxT.ptr, false, 1, B, nx, 0, p->VxT.env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "VxxT", p->VxxT.ptr, false, 1, B, nx * nx, 0, p->VxxT.env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "mu", p->mu.ptr, false, 1, B, 1, 0, p->mu.env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "lo", q->lo, true, 1, 1, nu, 0, 0)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "hi", q->hi, true, 1, 1, nu, 0, 0)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "k", p->k, false, T, B, nu, B * nu, nu)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "K", p->K, false, T, B, nu * nx, B * nu * nx, nu * nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "dV", p->dV, false, 1, B, 2, 0, 2)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "V0x", p->V0x, true, 1, B, nx, 0, nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "V0xx", p->V0xx, true, 1, B, nx * nx, 0, nx * nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "status", p->status, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "clamped", q->clamped, false, T, B, 1, B, 1, 4)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "qp_iters", q->qp_iters, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  LqrBoxArgs a;
  a.b.T = p->T; a.b.B = p->batch; a.b.nx = p->nx; a.b.nu = p->nu;
  a.b.A = lqr_arr(p->A); a.b.Bm = lqr_arr(p->B); a.b.lx = lqr_arr(p->lx); a.b.lu = lqr_arr(p->lu); a.b.lxx = lqr_arr(p->lxx); a.b.luu = lqr_arr(p->luu);
  a.b.lux = lqr_arr(p->lux); a.b.VxT = lqr_arr(p->VxT); a.b.VxxT = lqr_arr(p->VxxT); a.b.mu = lqr_arr(p->mu);
  a.b.k = p->k; a.b.K = p->K; a.b.dV = p->dV; a.b.V0x = p->V0x; a.b.V0xx = p->V0xx; a.b.status = p->status;
  a.u = lqr_arr(q->u); a.lo = q->lo; a.hi = q->hi; a.clamped = q->clamped; a.qp_iters = q->qp_iters;
  const hipError_t e = lqr_launch_backward_box(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_lqr_backward_box launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

int mjb_lqr_candidates(mjbData* d, const mjbLqrCandidates* p) {
  static const char* fn = "mjb_lqr_candidates";
  if (!d || !p) return fail(MJB_ERR_ARG, "mjb_lqr_candidates: NULL argument");
  int rc;
  if ((rc = check_lqr_sizes(fn, p->T, p->batch, p->nx, p->nu)) != MJB_OK) return rc;
  if (p->nalpha < 1 || p->nalpha > kLqrMaxAlpha) return fail(MJB_ERR_ARG, "mjb_lqr_candidates: nalpha must lie in [1, 64]");
  HIPCHK(hipSetDevice(d->device));
  const long T = p->T, B = p->batch, nx = p->nx, nu = p->nu, na = p->nalpha;
  const struct { const char* what; const mjbStrided* s; long n; } in[] = {
      {"A", &p->A, nx * nx}, {"B", &p->B, nx * nu}, {"k", &p->k, nu}, {"K", &p->K, nu * nx}, {"u", &p->u, nu}};
  for (const auto& a : in)
    if ((rc = check_lqr_array(d, fn, a.what, a.s->ptr, false, T, B, a.n, a.s->step_stride, a.s->env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "dx0", p->dx0.ptr, true, 1, B, nx, 0, p->dx0.env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "alphas", p->alphas, false, 1, 1, na, 0, 0)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "lo", p->lo, true, 1, 1, nu, 0, 0)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "hi", p->hi, true, 1, 1, nu, 0, 0)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "cand", p->cand, false, 1, B, na * T * nu, 0, na * T * nu, p->out_f32 ? 4 : 8)) != MJB_OK) return rc;
  LqrCandArgs a;
  a.T = p->T; a.B = p->batch; a.nx = p->nx; a.nu = p->nu; a.nalpha = p->nalpha; a.out_f32 = p->out_f32 ? 1 : 0;
  a.A = lqr_arr(p->A); a.Bm = lqr_arr(p->B); a.k = lqr_arr(p->k); a.K = lqr_arr(p->K); a.u = lqr_arr(p->u); a.dx0 = lqr_arr(p->dx0);
  a.alphas = p->alphas; a.lo = p->lo; a.hi = p->hi; a.cand = p->cand;
  const hipError_t e = lqr_launch_candidates(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_lqr_candidates launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

int mjb_lqr_gemm_tn(mjbData* d, int M, int N, int K, const double* a, const double* b, double* c) {
  static const char* fn = "mjb_lqr_gemm_tn";
  if (!d) return fail(MJB_ERR_ARG, "mjb_lqr_gemm_tn: data is NULL");
  if (M < 1 || N < 1 || K < 1 || M > kLqrMaxNx || N > kLqrMaxNx || K > (1 << 20)) return fail(MJB_ERR_ARG, "mjb_lqr_gemm_tn: M, N must lie in [1, 64], K in [1, 2^20]");
  HIPCHK(hipSetDevice(d->device));
  int rc;
  if ((rc = check_lqr_array(d, fn, "a", a, false, 1, 1, (long)K * M, 0, 0)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "b", b, false, 1, 1, (long)K * N, 0, 0)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "c", c, false, 1, 1, (long)M * N, 0, 0)) != MJB_OK) return rc;
  const hipError_t e = lqr_launch_gemm_probe(M, N, K, a, b, c, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_lqr_gemm_tn launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

// ---- mjb_lqr_dare: the checks (those of mjb_lqr_backward); the kernel and its launch are in mjb_dare.hip ----
int mjb_lqr_dare(mjbData* d, const mjbLqrDare* p) {
  static const char* fn = "mjb_lqr_dare";
  if (!d || !p) return fail(MJB_ERR_ARG, "mjb_lqr_dare: NULL argument");
  static const char* const msg[7] = {"", ": batch must be >= 1", ": nx must lie in [1, 64] (the state the kernel keeps in LDS)", ": nu must lie in [1, 32]",
                                     ": max_iter must lie in [1, 64]", ": tol must be >= 0", ": batch * nx * nx is too large"};
  const int why = dare_size_error(p->batch, p->nx, p->nu, p->max_iter, p->tol);
  if (why) return fail(MJB_ERR_ARG, std::string(fn) + msg[why]);
  HIPCHK(hipSetDevice(d->device));
  const long B = p->batch, nx = p->nx, nu = p->nu;
  int rc;
  const struct { const char* what; const mjbStrided* s; long n; } in[] = {
      {"A", &p->A, nx * nx}, {"B", &p->B, nx * nu}, {"Q", &p->Q, nx * nx}, {"R", &p->R, nu * nu}};
  for (const auto& a : in)
    if ((rc = check_lqr_array(d, fn, a.what, a.s->ptr, false, 1, B, a.n, 0, a.s->env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "X", p->X, false, 1, B, nx * nx, 0, nx * nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "K", p->K, false, 1, B, nu * nx, 0, nu * nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "change", p->change, true, 1, B, 1, 0, 1)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "iters", p->iters, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "status", p->status, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  DareArgs a;
  a.B = p->batch; a.nx = p->nx; a.nu = p->nu; a.max_iter = p->max_iter; a.tol = p->tol;
  a.A = lqr_arr(p->A); a.Bm = lqr_arr(p->B); a.Q = lqr_arr(p->Q); a.R = lqr_arr(p->R);
  a.X = p->X; a.K = p->K; a.change = p->change; a.iters = p->iters; a.status = p->status;
  const hipError_t e = dare_launch(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_lqr_dare launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

// ---- mjb_lqr_eig: the checks (those of mjb_lqr_dare); the kernel and its launch are in mjb_eig.hip ----
int mjb_lqr_eig(mjbData* d, const mjbLqrEig* p) {
  static const char* fn = "mjb_lqr_eig";
  if (!d || !p) return fail(MJB_ERR_ARG, "mjb_lqr_eig: NULL argument");
  static const char* const msg[7] = {"", ": batch must be >= 1", ": nx must lie in [1, 64] (the matrix the kernel keeps in LDS)", ": nu must lie in [1, 32]",
                                     ": max_sweeps must be 0 (the default) or lie in [1, 30 * max(10, nx)]", ": feedback_sign must be -1 or +1",
                                     ": batch * nx * nx is too large"};
  if ((p->B.ptr == nullptr) != (p->K.ptr == nullptr)) return fail(MJB_ERR_ARG, "mjb_lqr_eig: B and K must be given together (both NULL: the poles of A)");
  const bool has_bk = p->B.ptr != nullptr;
  const int why = eig_size_error(p->batch, p->nx, p->nu, has_bk, p->max_sweeps, p->feedback_sign);
  if (why) return fail(MJB_ERR_ARG, std::string(fn) + msg[why]);
  HIPCHK(hipSetDevice(d->device));
  const long B = p->batch, nx = p->nx, nu = has_bk ? p->nu : 0;
  int rc;
  if ((rc = check_lqr_array(d, fn, "A", p->A.ptr, false, 1, B, nx * nx, 0, p->A.env_stride)) != MJB_OK) return rc;
  if (has_bk) {
    if ((rc = check_lqr_array(d, fn, "B", p->B.ptr, false, 1, B, nx * nu, 0, p->B.env_stride)) != MJB_OK) return rc;
    if ((rc = check_lqr_array(d, fn, "K", p->K.ptr, false, 1, B, nu * nx, 0, p->K.env_stride)) != MJB_OK) return rc;
  }
  if ((rc = check_lqr_array(d, fn, "wr", p->wr, false, 1, B, nx, 0, nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "wi", p->wi, false, 1, B, nx, 0, nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "rho", p->rho, false, 1, B, 1, 0, 1)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "scale", p->scale, false, 1, B, nx, 0, nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "sweeps", p->sweeps, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "status", p->status, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  EigArgs a;
  a.B = p->batch; a.nx = p->nx; a.nu = (int)nu; a.max_sweeps = p->max_sweeps; a.balance = p->balance ? 1 : 0; a.sign = (double)p->feedback_sign;
  a.A = lqr_arr(p->A); a.Bm = lqr_arr(p->B); a.K = lqr_arr(p->K);
  a.wr = p->wr; a.wi = p->wi; a.rho = p->rho; a.scale = p->scale; a.sweeps = p->sweeps; a.status = p->status;
  const hipError_t e = eig_launch(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_lqr_eig launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

// ---- mjb_lqr_dlyap: the checks (those of mjb_lqr_dare / mjb_lqr_eig); the kernels and their launch are in mjb_dlyap.hip ----
int mjb_lqr_dlyap(mjbData* d, const mjbLqrDlyap* p) {
  static const char* fn = "mjb_lqr_dlyap";
  if (!d || !p) return fail(MJB_ERR_ARG, "mjb_lqr_dlyap: NULL argument");
  static const char* const msg[8] = {"", ": batch must be >= 1", ": nx must lie in [1, 64] (the state the kernel keeps in LDS)", ": nu must lie in [1, 32]",
                                     ": max_iter must lie in [1, 64]", ": tol must be >= 0", ": feedback_sign must be -1 or +1",
                                     ": batch * nx * nx is too large"};
  if ((p->B.ptr == nullptr) != (p->K.ptr == nullptr)) return fail(MJB_ERR_ARG, "mjb_lqr_dlyap: B and K must be given together (both NULL: M = A)");
  const bool has_bk = p->B.ptr != nullptr;
  if (p->R.ptr && !has_bk) return fail(MJB_ERR_ARG, "mjb_lqr_dlyap: R needs K (the cost term is K' R K)");
  if ((p->x0.ptr == nullptr) != (p->J == nullptr)) return fail(MJB_ERR_ARG, "mjb_lqr_dlyap: x0 and J must be given together");
  const int why = dlyap_size_error(p->batch, p->nx, p->nu, has_bk, p->max_iter, p->tol, p->feedback_sign);
  if (why) return fail(MJB_ERR_ARG, std::string(fn) + msg[why]);
  HIPCHK(hipSetDevice(d->device));
  const long B = p->batch, nx = p->nx, nu = has_bk ? p->nu : 0;
  int rc;
  if ((rc = check_lqr_array(d, fn, "A", p->A.ptr, false, 1, B, nx * nx, 0, p->A.env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "Q", p->Q.ptr, false, 1, B, nx * nx, 0, p->Q.env_stride)) != MJB_OK) return rc;
  if (has_bk) {
    if ((rc = check_lqr_array(d, fn, "B", p->B.ptr, false, 1, B, nx * nu, 0, p->B.env_stride)) != MJB_OK) return rc;
    if ((rc = check_lqr_array(d, fn, "K", p->K.ptr, false, 1, B, nu * nx, 0, p->K.env_stride)) != MJB_OK) return rc;
    if ((rc = check_lqr_array(d, fn, "R", p->R.ptr, true, 1, B, nu * nu, 0, p->R.env_stride)) != MJB_OK) return rc;
  }
  if ((rc = check_lqr_array(d, fn, "x0", p->x0.ptr, true, 1, B, nx, 0, p->x0.env_stride)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "P", p->P, false, 1, B, nx * nx, 0, nx * nx)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "J", p->J, true, 1, B, 1, 0, 1)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "change", p->change, true, 1, B, 1, 0, 1)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "iters", p->iters, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "status", p->status, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  DlyapArgs a;
  a.B = p->batch; a.nx = p->nx; a.nu = (int)nu; a.transpose = p->transpose ? 1 : 0; a.max_iter = p->max_iter;
  a.sign = (double)p->feedback_sign; a.tol = p->tol;
  a.A = lqr_arr(p->A); a.Bm = lqr_arr(p->B); a.K = lqr_arr(p->K); a.Q = lqr_arr(p->Q); a.R = lqr_arr(p->R); a.x0 = lqr_arr(p->x0);
  a.P = p->P; a.J = p->J; a.change = p->change; a.iters = p->iters; a.status = p->status;
  const hipError_t e = dlyap_launch(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_lqr_dlyap launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

// ---- mjb_setpoint_ctrl: the checks (those of mjb_lqr_dlyap); the kernel and its launch are in mjb_setpoint.hip ----
int mjb_setpoint_ctrl(mjbData* d, const mjbSetpoint* p) {
  static const char* fn = "mjb_setpoint_ctrl";
  if (!d || !p) return fail(MJB_ERR_ARG, "mjb_setpoint_ctrl: NULL argument");
  static const char* const msg[7] = {"", ": batch must be >= 1", ": nu must lie in [1, 32]", ": nv must lie in [1, 64] (the matrix the kernel keeps in LDS)",
                                     ": max_sweeps must be 0 (the default, 30) or lie in [1, 64]", ": rcond_min must be finite and >= 0",
                                     ": batch * nu * nv is too large"};
  const int why = setpoint_size_error(p->batch, p->nu, p->nv, p->max_sweeps, p->rcond_min);
  if (why) return fail(MJB_ERR_ARG, std::string(fn) + msg[why]);
  if ((p->moment.dtype != MJB_F32 && p->moment.dtype != MJB_F64) || (p->qfrc.dtype != MJB_F32 && p->qfrc.dtype != MJB_F64))
    return fail(MJB_ERR_ARG, "mjb_setpoint_ctrl: the dtype of moment and of qfrc must be MJB_F32 or MJB_F64");
  HIPCHK(hipSetDevice(d->device));
  const long B = p->batch, nu = p->nu, nv = p->nv, r = nu < nv ? nu : nv;
  int rc;
  if ((rc = check_lqr_array(d, fn, "moment", p->moment.ptr, false, 1, B, nu * nv, 0, p->moment.env_stride, p->moment.dtype == MJB_F32 ? 4 : 8)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "qfrc", p->qfrc.ptr, false, 1, B, nv, 0, p->qfrc.env_stride, p->qfrc.dtype == MJB_F32 ? 4 : 8)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "ctrl", p->ctrl, false, 1, B, nu, 0, nu)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "sv", p->sv, false, 1, B, r, 0, r)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "rcond", p->rcond, false, 1, B, 1, 0, 1)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "residual", p->residual, false, 1, B, 1, 0, 1)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "pinv", p->pinv, true, 1, B, nv * nu, 0, nv * nu)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "rank", p->rank, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "sweeps", p->sweeps, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  if ((rc = check_lqr_array(d, fn, "status", p->status, false, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  SetpointArgs a;
  a.B = p->batch; a.nu = p->nu; a.nv = p->nv; a.max_sweeps = p->max_sweeps; a.rcond_min = p->rcond_min;
  a.m_f32 = p->moment.dtype == MJB_F32; a.q_f32 = p->qfrc.dtype == MJB_F32;
  a.moment = p->moment.ptr; a.qfrc = p->qfrc.ptr; a.m_es = p->moment.env_stride; a.q_es = p->qfrc.env_stride;
  a.ctrl = p->ctrl; a.sv = p->sv; a.rcond = p->rcond; a.residual = p->residual; a.pinv = p->pinv;
  a.rank = p->rank; a.sweeps = p->sweeps; a.status = p->status;
  const hipError_t e = setpoint_launch(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_setpoint_ctrl launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

// ---- mjb_traj_cost / mjb_traj_select: the checks; the kernels and their launches are in mjb_traj.hip ----
static int check_traj_array(const mjbData* d, const char* fn, const char* what, const void* ptr, bool may_be_null, long nstep, long B, long n,
                            long ss, long es, size_t esize = 8) {
  const std::string pre = std::string(fn) + ": " + what;
  if (ss < 0 || es < 0) return fail(MJB_ERR_ARG, pre + ": strides must be >= 0");
  if (!ptr) return may_be_null ? MJB_OK : fail(MJB_ERR_ARG, pre + " is NULL");
  __int128 hi;
  if (!traj_highest_element(nstep, B, n, ss, es, hi)) return fail(MJB_ERR_ARG, pre + ": bad extent");
  if (hi + 1 > ((__int128)1 << 60)) return fail(MJB_ERR_ARG, pre + ": the extent (T, batch, strides) lies beyond its allocation");
  const int why = device_extent(d, ptr, (size_t)(hi + 1) * esize);
  static const char* const msg[4] = {"", " is not device-accessible memory of this data object's device", ": no allocation found behind it",
                                     ": the extent (T, batch, strides) lies beyond its allocation"};
  return why ? fail(MJB_ERR_ARG, pre + msg[why]) : MJB_OK;
}

int mjb_traj_cost(mjbData* d, const mjbTrajCost* p) {
  static const char* fn = "mjb_traj_cost";
  if (!d || !p) return fail(MJB_ERR_ARG, "mjb_traj_cost: NULL argument");
  const HostModel& h = d->model->h;
  const long T = p->T, B = p->batch, nq = h.nq, nv = h.nv, nu = h.nu, nx = 2 * nv;
  static const char* const msg[7] = {"", ": T must be >= 1", ": batch must be >= 1", ": nv must lie in [1, 64]", ": nu must lie in [1, 64]",
                                     ": nq must lie in [nv, 2 nv]", ": (T + 1) * batch * 2 nv is too large"};
  if (const int why = traj_cost_size_error(T, B, nq, nv, nu)) return fail(MJB_ERR_ARG, std::string(fn) + msg[why]);
  const mjbStridedIn* st[4] = {&p->qpos0, &p->qvel0, &p->qpos, &p->qvel};
  for (const mjbStridedIn* s : st)
    if ((s->dtype != MJB_F32 && s->dtype != MJB_F64) || s->dtype != p->qpos0.dtype)
      return fail(MJB_ERR_ARG, "mjb_traj_cost: qpos0, qvel0, qpos, qvel must share one dtype, MJB_F32 or MJB_F64");
  if (p->ctrl.dtype != MJB_F32 && p->ctrl.dtype != MJB_F64) return fail(MJB_ERR_ARG, "mjb_traj_cost: ctrl dtype must be MJB_F32 or MJB_F64");
  HIPCHK(hipSetDevice(d->device));
  const size_t ss = p->qpos0.dtype == MJB_F32 ? 4 : 8, su = p->ctrl.dtype == MJB_F32 ? 4 : 8;
  int rc;
  if ((rc = check_traj_array(d, fn, "qpos0", p->qpos0.ptr, false, 1, B, nq, 0, p->qpos0.env_stride, ss)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "qvel0", p->qvel0.ptr, false, 1, B, nv, 0, p->qvel0.env_stride, ss)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "qpos", p->qpos.ptr, false, T, B, nq, p->qpos.step_stride, p->qpos.env_stride, ss)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "qvel", p->qvel.ptr, false, T, B, nv, p->qvel.step_stride, p->qvel.env_stride, ss)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "ctrl", p->ctrl.ptr, false, T, B, nu, p->ctrl.step_stride, p->ctrl.env_stride, su)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "qref", p->qref.ptr, false, T + 1, B, nq, p->qref.step_stride, p->qref.env_stride)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "vref", p->vref.ptr, true, T + 1, B, nv, p->vref.step_stride, p->vref.env_stride)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "uref", p->uref.ptr, true, T, B, nu, p->uref.step_stride, p->uref.env_stride)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "Q", p->Q.ptr, false, T, B, nx * nx, p->Q.step_stride, p->Q.env_stride)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "R", p->R.ptr, false, T, B, nu * nu, p->R.step_stride, p->R.env_stride)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "Qf", p->Qf.ptr, false, 1, B, nx * nx, 0, p->Qf.env_stride)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "cost", p->cost, false, 1, B, 1, 0, 1)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "cost_t", p->cost_t, false, 1, B, T + 1, 0, T + 1)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "lx", p->lx, true, T, B, nx, B * nx, nx)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "lu", p->lu, true, T, B, nu, B * nu, nu)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "VxT", p->VxT, true, 1, B, nx, 0, nx)) != MJB_OK) return rc;
  TrajCostArgs a;
  a.T = p->T; a.B = p->batch; a.nq = h.nq; a.nv = h.nv; a.nu = h.nu; a.njnt = h.njnt;
  a.state_f32 = p->qpos0.dtype == MJB_F32; a.ctrl_f32 = p->ctrl.dtype == MJB_F32;
  auto in = [](const mjbStridedIn& s, bool per_env) { TrajIn r; r.p = s.ptr; r.ss = per_env ? 0 : s.step_stride; r.es = s.env_stride; return r; };
  auto ref = [](const mjbStrided& s, bool per_env) { TrajRef r; r.p = s.ptr; r.ss = per_env ? 0 : s.step_stride; r.es = s.env_stride; return r; };
  a.qpos0 = in(p->qpos0, true); a.qvel0 = in(p->qvel0, true); a.qpos = in(p->qpos, false); a.qvel = in(p->qvel, false); a.ctrl = in(p->ctrl, false);
  a.qref = ref(p->qref, false); a.vref = ref(p->vref, false); a.uref = ref(p->uref, false);
  a.Q = ref(p->Q, false); a.R = ref(p->R, false); a.Qf = ref(p->Qf, true);
  a.jnt_type = d->md.jnt_type; a.jnt_qposadr = d->md.jnt_qposadr; a.jnt_dofadr = d->md.jnt_dofadr;
  a.cost = p->cost; a.cost_t = p->cost_t; a.lx = p->lx; a.lu = p->lu; a.VxT = p->VxT;
  const hipError_t e = traj_launch_cost(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_traj_cost launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

int mjb_traj_select(mjbData* d, const mjbTrajSelect* p) {
  static const char* fn = "mjb_traj_select";
  if (!d || !p) return fail(MJB_ERR_ARG, "mjb_traj_select: NULL argument");
  static const char* const msg[7] = {"", ": nprob must lie in [1, 2^30]", ": ncand must lie in [1, 2^20]", ": T, nu must be >= 1 and T * nu <= 2^22",
                                     ": mode must be MJB_SELECT_ARGMIN or MJB_SELECT_SOFTMIN", ": temperature must be finite and > 0",
                                     ": nprob * ncand * T * nu is too large"};
  if (const int why = traj_select_size_error(p->nprob, p->ncand, p->T, p->nu, p->mode, p->temperature)) return fail(MJB_ERR_ARG, std::string(fn) + msg[why]);
  if ((p->cand_dtype != MJB_F32 && p->cand_dtype != MJB_F64) || (p->out_dtype != MJB_F32 && p->out_dtype != MJB_F64))
    return fail(MJB_ERR_ARG, "mjb_traj_select: cand_dtype and out_dtype must be MJB_F32 or MJB_F64");
  HIPCHK(hipSetDevice(d->device));
  const long G = p->nprob, n = p->ncand, M = (long)p->T * p->nu;
  int rc;
  if ((rc = check_traj_array(d, fn, "cost", p->cost, false, 1, G, n, 0, n)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "cand", p->cand, false, 1, G, n * M, 0, n * M, p->cand_dtype == MJB_F32 ? 4 : 8)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "u_out", p->u_out, false, 1, G, M, 0, M, p->out_dtype == MJB_F32 ? 4 : 8)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "best", p->best, true, 1, G, 1, 0, 1, 4)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "best_cost", p->best_cost, true, 1, G, 1, 0, 1)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "weights", p->weights, true, 1, G, n, 0, n)) != MJB_OK) return rc;
  TrajSelectArgs a;
  a.nprob = p->nprob; a.T = p->T; a.nu = p->nu; a.mode = p->mode; a.cand_f32 = p->cand_dtype == MJB_F32; a.out_f32 = p->out_dtype == MJB_F32;
  a.ncand = p->ncand; a.temperature = p->temperature;
  a.cost = p->cost; a.cand = p->cand; a.u_out = p->u_out; a.best = p->best; a.best_cost = p->best_cost; a.weights = p->weights;
  const hipError_t e = traj_launch_select(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_traj_select launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

// ---- mjb_feedback_law / mjb_rollout_feedback: the checks; the kernel and its launch are in mjb_feedback.hip ----
// Everything both entry points check, for the steps t0 .. t0 + nstep - 1, and the kernel's arguments (t left to the caller).
static int feedback_args(mjbData* d, const char* fn, const mjbFeedbackLaw* p, int t0, int nstep, FeedbackLawArgs& a) {
  if (!d || !p) return fail(MJB_ERR_ARG, std::string(fn) + ": NULL argument");
  const HostModel& h = d->model->h;
  std::memset(&a, 0, sizeof(a));
  a.B = d->batch; a.nq = h.nq; a.nv = h.nv; a.nu = h.nu; a.njnt = h.njnt; a.data_f32 = d->dtype == MJB_F32; a.clip = p->clip ? 1 : 0; a.t = t0;
  a.sign = (double)p->feedback_sign;
  const mjbStridedIn* src[4] = {&p->K, &p->u0, &p->q0, &p->v0};
  FbIn* dst[4] = {&a.K, &a.u0, &a.q0, &a.v0};
  static const char* const names[4] = {"K", "u0", "q0", "v0"};
  for (int k = 0; k < 4; k++) {
    if (src[k]->ptr && src[k]->dtype != MJB_F32 && src[k]->dtype != MJB_F64)
      return fail(MJB_ERR_ARG, std::string(fn) + ": the dtype of " + names[k] + " must be MJB_F32 or MJB_F64");
    dst[k]->p = src[k]->ptr; dst[k]->ss = src[k]->step_stride; dst[k]->es = src[k]->env_stride; dst[k]->f32 = src[k]->dtype == MJB_F32;
  }
  a.ur_ss = p->u_rec_step_stride; a.ur_es = p->u_rec_env_stride;
  static const char* const msg[10] = {"", ": the data object has no environment", ": nv must lie in [1, 64]", ": nu must lie in [1, 32]",
                                      ": the model's joint table does not fit nq, nv", ": feedback_sign must be -1 or +1", ": t must be >= 0",
                                      ": nstep must be >= 1 (and t + nstep <= 2^30)", ": strides must be >= 0", ": K, u0 and q0 are required"};
  if (const int why = feedback_arg_error(a, nstep)) return fail(MJB_ERR_ARG, std::string(fn) + msg[why]);
  HIPCHK(hipSetDevice(d->device));
  const long B = d->batch, last = (long)t0 + nstep - 1, nx = 2L * h.nv;
  const long n[4] = {(long)h.nu * nx, h.nu, h.nq, h.nv};
  int rc;
  for (int k = 0; k < 4; k++)
    if ((rc = check_traj_array(d, fn, names[k], src[k]->ptr, k == 3, last + 1, B, n[k], src[k]->step_stride, src[k]->env_stride,
                               src[k]->dtype == MJB_F32 ? 4 : 8)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "u_rec", p->u_rec, true, last + 1, B, h.nu, p->u_rec_step_stride, p->u_rec_env_stride, a.data_f32 ? 4 : 8)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "status", p->status, true, 1, B, 1, 0, 1, 4)) != MJB_OK) return rc;
  if ((rc = check_traj_array(d, fn, "env_mask", p->env_mask, true, 1, B, 1, 0, 1, 1)) != MJB_OK) return rc;
  if (a.data_f32) { a.qpos = d->df.qpos; a.qvel = d->df.qvel; a.ctrl = d->df.ctrl; }
  else { a.qpos = d->dd.qpos; a.qvel = d->dd.qvel; a.ctrl = d->dd.ctrl; }
  a.jnt_type = d->md.jnt_type; a.jnt_qposadr = d->md.jnt_qposadr; a.jnt_dofadr = d->md.jnt_dofadr;
  a.ctrllimited = d->md.actuator_ctrllimited; a.ctrlrange = d->md.actuator_ctrlrange;
  a.mask = p->env_mask; a.status = p->status; a.u_rec = p->u_rec;
  return MJB_OK;
}

int mjb_feedback_law(mjbData* d, const mjbFeedbackLaw* p, int t) {
  FeedbackLawArgs a;
  int rc = feedback_args(d, "mjb_feedback_law", p, t, 1, a);
  if (rc != MJB_OK) return rc;
  const hipError_t e = feedback_launch(a, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_feedback_law launch: ") + hipGetErrorString(e));
  return MJB_OK;
}

int mjb_rollout_feedback(mjbData* d, const mjbFeedbackLaw* p, int nstep, const mjbObsSpec* spec, void* obs_out_dev, int obs_every) {
  static const char* fn = "mjb_rollout_feedback";
  FeedbackLawArgs a;
  int rc = feedback_args(d, fn, p, 0, nstep, a);
  if (rc != MJB_OK) return rc;
  const bool ring = spec && obs_out_dev && obs_every > 0;
  const long rows = ring ? nstep / obs_every : 0;
  const size_t esize = d->dtype == MJB_F32 ? 4 : 8;
  if (ring && rows > 0 && (rc = check_traj_array(d, fn, "obs_out_dev", obs_out_dev, false, rows, d->batch, spec->dev.dim, (long)d->batch * spec->dev.dim,
                                                   spec->dev.dim, esize)) != MJB_OK) return rc;
  if ((rc = engine_check(d)) != MJB_OK) return rc;               // what the first step's launch would refuse, before the first law kernel
  ObsSpecDev none; std::memset(&none, 0, sizeof(none));
  for (int t = 0; t < nstep; t++) {
    a.t = t;
    const hipError_t e = feedback_launch(a, d->stream);
    if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("mjb_rollout_feedback launch: ") + hipGetErrorString(e));
    if ((rc = launch(d, make_args(d, 1, MJB_CTRL_KEEP, 0, 0, 1.0, 0), none, nullptr, false)) != MJB_OK) return rc;   // mjb_step(d, 1)
    if (ring && (t + 1) % obs_every == 0 &&
        (rc = mjb_obs_gather(d, spec, (char*)obs_out_dev + (size_t)(t / obs_every) * d->batch * spec->dev.dim * esize)) != MJB_OK) return rc;
  }
  return MJB_OK;
}

int mjb_transition_fd(mjbData* d, double eps, int centered, double* A_host, double* B_host) {
  if (!d || !A_host || !B_host) return fail(MJB_ERR_ARG, "NULL argument");
  int rc = transition_fd_impl(d, eps, centered);
  if (rc != MJB_OK) return rc;
  const HostModel& h = d->model->h;
  const size_t B = (size_t)d->batch, nx = 2 * (size_t)h.nv;
  std::memcpy(A_host, d->fd_A_host.get(), B * nx * nx * sizeof(double));
  if (h.nu > 0) std::memcpy(B_host, d->fd_B_host.get(), B * nx * h.nu * sizeof(double));
  return MJB_OK;
}

int mjb_transition_fd_pinned(mjbData* d, double eps, int centered, const double** A_pinned, const double** B_pinned) {
  if (!d || !A_pinned || !B_pinned) return fail(MJB_ERR_ARG, "NULL argument");
  int rc = transition_fd_impl(d, eps, centered);
  if (rc != MJB_OK) return rc;
  *A_pinned = d->fd_A_host.get(); *B_pinned = d->fd_B_host.get();
  return MJB_OK;
}

int mjb_transition_fd_sensors(mjbData* d, double eps, int centered, const double** A_pinned, const double** B_pinned, const double** C_pinned, const double** D_pinned) {
  if (!d || !A_pinned || !B_pinned || !C_pinned || !D_pinned) return fail(MJB_ERR_ARG, "NULL argument");
  int rc = transition_fd_impl(d, eps, centered, true);
  if (rc != MJB_OK) return rc;
  const bool any = d->model->h.nsensordata > 0;                // a model without sensors: empty blocks, NULL
  *A_pinned = d->fd_A_host.get(); *B_pinned = d->fd_B_host.get();
  *C_pinned = any ? d->fd_C_host.get() : nullptr; *D_pinned = any ? d->fd_D_host.get() : nullptr;
  return MJB_OK;
}



int mjb_jac(mjbData* d, int nreq, const int* kinds, const int* ids, double* jacp_host, double* jacr_host) {
  if (!d || !kinds || !ids || !jacp_host || nreq < 1) return fail(MJB_ERR_ARG, "bad argument");
  const HostModel& h = d->model->h;
  for (int i = 0; i < nreq; i++) {
    if (kinds[i] < 0 || kinds[i] > 3) return fail(MJB_ERR_ARG, "jacobian kind must be 0..3");
    int lim = kinds[i] == 0 ? h.nsite : h.nbody;
    if (ids[i] < 0 || ids[i] >= lim) return fail(MJB_ERR_LOOKUP, "jacobian object id out of range");
  }
  HIPCHK(hipSetDevice(d->device));
  { int rc0 = refresh_options(d); if (rc0 != MJB_OK) return rc0; }
  const size_t n = (size_t)d->batch * nreq * 3 * h.nv;
  if (n == 0) return MJB_OK;
  // persistent buffers instead of four hipMalloc / hipFree and four blocking copies per call (a controller with needs_jacobians calls this
  // once per Env.step): request in pinned memory read by the kernel, results pinned, device staging only for large requests
  HIPCHK(d->jac_req_pin.reserve(2 * (size_t)nreq));
  const bool zero_copy = 2 * n * sizeof(double) <= (size_t)256 * 1024;
  if (d->jac_pin[0].reserve(n) != hipSuccess || d->jac_pin[1].reserve(n) != hipSuccess ||            // each pair to exactly n
      (!zero_copy && (d->jac_dev[0].reserve(n) != hipSuccess || d->jac_dev[1].reserve(n) != hipSuccess))) {
    reset_all(d->jac_pin[0], d->jac_pin[1], d->jac_dev[0], d->jac_dev[1]);
    return fail(MJB_ERR_DEVICE, "mjb_jac: allocation of the result blocks failed");
  }
  HIPCHK(hipStreamSynchronize(d->stream));                       // nothing queued may still be reading the previous request
  std::memcpy(d->jac_req_pin.get(), kinds, sizeof(int) * nreq);
  std::memcpy(d->jac_req_pin.get() + nreq, ids, sizeof(int) * nreq);
  double *op = zero_copy ? d->jac_pin[0].get() : d->jac_dev[0].get(), *orr = zero_copy ? d->jac_pin[1].get() : d->jac_dev[1].get();
  const int *dk = d->jac_req_pin.get(), *di = d->jac_req_pin.get() + nreq;
  hipError_t e = d->dtype == MJB_F32 ? launch_jac<double, float>(d->cfg.G_fd, d->md_dev, d->Ld_dev, d->cfg.Ld, d->df, nreq, dk, di, op, orr, d->stream)
                                     : launch_jac<double, double>(d->cfg.G_fd, d->md_dev, d->Ld_dev, d->cfg.Ld, d->dd, nreq, dk, di, op, orr, d->stream);
  if (e != hipSuccess) return fail(MJB_ERR_DEVICE, std::string("jac launch: ") + hipGetErrorString(e));
  if (!zero_copy) {
    HIPCHK(hipMemcpyAsync(d->jac_pin[0].get(), d->jac_dev[0].get(), n * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if (jacr_host) HIPCHK(hipMemcpyAsync(d->jac_pin[1].get(), d->jac_dev[1].get(), n * sizeof(double), hipMemcpyDeviceToHost, d->stream));
  }
  if (hipStreamSynchronize(d->stream) != hipSuccess) return fail(MJB_ERR_DEVICE, "jac sync failed");
  std::memcpy(jacp_host, d->jac_pin[0].get(), n * sizeof(double));
  if (jacr_host) std::memcpy(jacr_host, d->jac_pin[1].get(), n * sizeof(double));
  return MJB_OK;
}


// ---------------------------------------------------------------------------------------------------------------------
// model: names, fields, binary save / load
// ---------------------------------------------------------------------------------------------------------------------
int mjb_model_name2id(const mjbModel* m, int objtype, const char* name) {
  if (!m || !name) { fail(MJB_ERR_ARG, "model/name is NULL"); return -1; }
  if (objtype == 2) objtype = 1;                                       // mjOBJ_XBODY aliases mjOBJ_BODY
  auto it = m->names.find(objtype);
  if (it == m->names.end()) return -1;
  for (size_t i = 0; i < it->second.size(); i++) if (!it->second[i].empty() && it->second[i] == name) return (int)i;
  return -1;
}

const char* mjb_model_id2name(const mjbModel* m, int objtype, int id) {
  if (!m) { fail(MJB_ERR_ARG, "model is NULL"); return nullptr; }
  if (objtype == 2) objtype = 1;
  auto it = m->names.find(objtype);
  if (it == m->names.end() || id < 0 || id >= (int)it->second.size() || it->second[id].empty()) return nullptr;
  return it->second[id].c_str();
}

int mjb_model_field(const mjbModel* m, const char* name, const void** ptr, long* count, int* dtype) {
  if (!m || !name) return fail(MJB_ERR_ARG, "model/name is NULL");
  for (const auto& f : m->fields) if (f.name == name) {
    if (ptr) *ptr = m->blob.data() + f.off;
    if (count) *count = f.count;
    if (dtype) *dtype = f.dtype;
    return MJB_OK;
  }
  return fail(MJB_ERR_ARG, std::string("unknown model field: ") + name);
}

int mjb_model_field_at(const mjbModel* m, int index, const char** name, const void** ptr, long* count, int* dtype) {
  if (!m) { fail(MJB_ERR_ARG, "model is NULL"); return -1; }
  if (index < 0 || index >= (int)m->fields.size()) return (int)m->fields.size();     // out of range: returns the field count
  const auto& f = m->fields[index];
  if (name) *name = f.name.c_str();
  if (ptr) *ptr = m->blob.data() + f.off;
  if (count) *count = f.count;
  if (dtype) *dtype = f.dtype;
  return MJB_OK;
}

int mjb_model_save(const mjbModel* m, const char* path) {
  if (!m || !path) return fail(MJB_ERR_ARG, "model/path is NULL");
  // like mj_saveModel the file carries the options as they are NOW (disableactuator / iterations / tolerance may have been edited
  // since the table was compiled): they are patched into a copy of the creation-time blob
  std::vector<char> blob = m->blob;
  for (const auto& fl : m->fields) {
    if (fl.count != 1) continue;
    if (fl.dtype == 1 && fl.name == "disableactuator") { int32_t v = m->disableactuator; std::memcpy(blob.data() + fl.off, &v, 4); }
    else if (fl.dtype == 1 && fl.name == "iterations") { int32_t v = m->iterations; std::memcpy(blob.data() + fl.off, &v, 4); }
    else if (fl.dtype == 0 && fl.name == "tolerance") { double v = m->tolerance; std::memcpy(blob.data() + fl.off, &v, 8); }
  }
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(MJB_ERR_ARG, std::string("cannot open for writing: ") + path);
  size_t n = std::fwrite(blob.data(), 1, blob.size(), f);
  int rc = std::fclose(f);
  if (n != blob.size() || rc != 0) return fail(MJB_ERR_ARG, std::string("short write: ") + path);
  return MJB_OK;
}

int mjb_model_load(const char* path, mjbModel** out) {
  if (!path || !out) return fail(MJB_ERR_ARG, "path/out is NULL");
  FILE* f = std::fopen(path, "rb");
  if (!f) return fail(MJB_ERR_ARG, std::string("cannot open: ") + path);
  std::vector<char> b;
  char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
  std::fclose(f);
  std::vector<std::string> names; std::vector<const void*> ptrs; std::vector<int> dts; std::vector<long> cnts;
  std::string err;
  if (!parse_blob(b, names, ptrs, dts, cnts, err)) return fail(MJB_ERR_MODEL, err + ": " + path);
  std::vector<const char*> cn;
  for (auto& s : names) cn.push_back(s.c_str());
  return mjb_model_create((int)cn.size(), cn.data(), ptrs.data(), dts.data(), cnts.data(), out);
}

// ---------------------------------------------------------------------------------------------------------------------
// mj_integratePos / mj_differentiatePos on caller-owned HOST vectors, float64, batched [batch, nq] / [batch, nv]
// ---------------------------------------------------------------------------------------------------------------------
int mjb_integrate_pos(const mjbModel* m, int batch, double* qpos, const double* qvel, double dt) {
  if (!m || !qpos || !qvel || batch < 1) return fail(MJB_ERR_ARG, "bad argument");
  const HostModel& h = m->h;
  const auto& jt = h.I("jnt_type"); const auto& jq = h.I("jnt_qposadr"); const auto& jd = h.I("jnt_dofadr");
  for (int e = 0; e < batch; e++) {
    double* q = qpos + (size_t)e * h.nq; const double* v = qvel + (size_t)e * h.nv;
    for (int j = 0; j < h.njnt; j++) {
      const int qa = jq[j], da = jd[j];
      if (jt[j] == JNT_FREE) {
        for (int k = 0; k < 3; k++) q[qa + k] += dt * v[da + k];
        double ax[3] = {v[da + 3], v[da + 4], v[da + 5]};
        const double nrm = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        if (nrm < 1e-15) continue;
        const double ang = dt * nrm, sn = std::sin(0.5 * ang) / nrm;
        double qr[4] = {std::cos(0.5 * ang), ax[0] * sn, ax[1] * sn, ax[2] * sn}, out[4];
        h_quat_mul(out, q + qa + 3, qr);
        const double on = std::sqrt(out[0] * out[0] + out[1] * out[1] + out[2] * out[2] + out[3] * out[3]);
        if (on < 1e-15) { q[qa + 3] = 1; q[qa + 4] = q[qa + 5] = q[qa + 6] = 0; }
        else for (int k = 0; k < 4; k++) q[qa + 3 + k] = out[k] / on;
      } else q[qa] += dt * v[da];
    }
  }
  return MJB_OK;
}

int mjb_differentiate_pos(const mjbModel* m, int batch, double* qvel_out, double dt, const double* qpos1, const double* qpos2) {
  if (!m || !qvel_out || !qpos1 || !qpos2 || batch < 1) return fail(MJB_ERR_ARG, "bad argument");
  if (dt == 0) return fail(MJB_ERR_ARG, "dt must be non-zero");
  const HostModel& h = m->h;
  const auto& jt = h.I("jnt_type"); const auto& jq = h.I("jnt_qposadr"); const auto& jd = h.I("jnt_dofadr");
  const double PI = 3.14159265358979323846;
  for (int e = 0; e < batch; e++) {
    const double *q1 = qpos1 + (size_t)e * h.nq, *q2 = qpos2 + (size_t)e * h.nq; double* v = qvel_out + (size_t)e * h.nv;
    for (int j = 0; j < h.njnt; j++) {
      const int qa = jq[j], da = jd[j];
      if (jt[j] == JNT_FREE) {
        for (int k = 0; k < 3; k++) v[da + k] = (q2[qa + k] - q1[qa + k]) / dt;
        const double qn[4] = {q1[qa + 3], -q1[qa + 4], -q1[qa + 5], -q1[qa + 6]};
        double qd[4];
        h_quat_mul(qd, qn, q2 + qa + 3);
        const double sn = std::sqrt(qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3]);
        if (sn < 1e-15) { v[da + 3] = v[da + 4] = v[da + 5] = 0; continue; }
        double ang = 2 * std::atan2(sn, qd[0]);
        if (ang > PI) ang -= 2 * PI;
        const double k = ang / sn / dt;
        v[da + 3] = qd[1] * k; v[da + 4] = qd[2] * k; v[da + 5] = qd[3] * k;
      } else v[da] = (q2[qa] - q1[qa]) / dt;
    }
  }
  return MJB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// host mirror: ONE pinned float64 block per data object, one pack kernel + ONE copy per direction
// ---------------------------------------------------------------------------------------------------------------------
static int ensure_mirror(mjbData* d) {
  if (d->mirror_host.get() && d->mirror_dev.get()) return MJB_OK;
  const HostModel& h = d->model->h;
  const size_t B = (size_t)d->batch, n[6] = {(size_t)h.nq, (size_t)h.nv, (size_t)h.nu, (size_t)h.nv, (size_t)h.nv, 1};
  size_t o = 0;
  for (int k = 0; k < 6; k++) { d->mirror_off[k] = o; o += B * n[k]; }
  d->mirror_off[6] = o;
  HIPCHK(hipSetDevice(d->device));
  // + the engine-flags word + one completion word per environment (polled by mjb_step_host on the zero-copy path: coherent memory, the
  // device's stores must be visible to the host while the kernel is still running)
  if (reserve_zeroed(d->mirror_host, o + 1 + B) != hipSuccess || reserve_zeroed(d->mirror_dev, o + 1) != hipSuccess) {   // both or neither
    reset_all(d->mirror_host, d->mirror_dev);
    return fail(MJB_ERR_DEVICE, "device allocation of the mirror staging block failed");
  }
  return MJB_OK;
}
static const char* const kMirrorNames[6] = {"qpos", "qvel", "ctrl", "qacc", "qacc_warmstart", "time"};

int mjb_host_view(mjbData* d, const char* name, double** host_ptr, long* per_env) {
  if (!d || !name || !host_ptr) return fail(MJB_ERR_ARG, "NULL argument");
  int rc = ensure_mirror(d);
  if (rc != MJB_OK) return rc;
  const HostModel& h = d->model->h;
  const long n[6] = {h.nq, h.nv, h.nu, h.nv, h.nv, 1};
  if (!std::strcmp(name, "engine_flags")) { *host_ptr = d->mirror_host.get() + d->mirror_off[6]; if (per_env) *per_env = 0; return MJB_OK; }
  for (int k = 0; k < 6; k++) if (!std::strcmp(name, kMirrorNames[k])) {
    *host_ptr = d->mirror_host.get() + d->mirror_off[k];
    if (per_env) *per_env = n[k];
    return MJB_OK;
  }
  return fail(MJB_ERR_ARG, std::string("no host mirror for array: ") + name);
}

// Small blocks (a few environments: the reference's batch-1 loops) skip the staging copy: the pack / unpack kernels read and write
// the pinned host block itself (device-visible, unified addressing) - two runtime calls less per host-driven step.
static bool mirror_zero_copy(const mjbData* d) { return d->mirror_off[6] + 1 <= 8192; }

static int mirror_pull(mjbData* d) {
  const HostModel& h = d->model->h;
  const long total = (long)d->mirror_off[6];
  const unsigned grid = (unsigned)((total + 255) / 256);
  double* dst = mirror_zero_copy(d) ? d->mirror_host.get() : d->mirror_dev.get();
  if (d->dtype == MJB_F32) hipLaunchKernelGGL(k_mirror_pack<float>, dim3(grid), dim3(256), 0, d->stream, d->df, h.nq, h.nv, h.nu, dst, total);
  else hipLaunchKernelGGL(k_mirror_pack<double>, dim3(grid), dim3(256), 0, d->stream, d->dd, h.nq, h.nv, h.nu, dst, total);
  HIPCHK(hipGetLastError());
  if (dst == d->mirror_dev.get()) HIPCHK(hipMemcpyAsync(d->mirror_host.get(), d->mirror_dev.get(), (size_t)(total + 1) * sizeof(double), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  return engine_check(d);
}

static int mirror_push(mjbData* d, int mask) {
  mask &= 63;
  if (!mask) return MJB_OK;
  const HostModel& h = d->model->h;
  int lo = 0, hi = 5;
  while (!((mask >> lo) & 1)) lo++;
  while (!((mask >> hi) & 1)) hi--;
  const size_t a = d->mirror_off[lo], b = d->mirror_off[hi + 1];       // one contiguous span covering the edited fields
  const double* src = mirror_zero_copy(d) ? d->mirror_host.get() : d->mirror_dev.get();
  if (src == d->mirror_dev.get()) HIPCHK(hipMemcpyAsync(d->mirror_dev.get() + a, d->mirror_host.get() + a, (b - a) * sizeof(double), hipMemcpyHostToDevice, d->stream));
  const long total = (long)d->mirror_off[6];
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (d->dtype == MJB_F32) hipLaunchKernelGGL(k_mirror_unpack<float>, dim3(grid), dim3(256), 0, d->stream, d->df, h.nq, h.nv, h.nu, src, total, mask);
  else hipLaunchKernelGGL(k_mirror_unpack<double>, dim3(grid), dim3(256), 0, d->stream, d->dd, h.nq, h.nv, h.nu, src, total, mask);
  HIPCHK(hipGetLastError());
  return MJB_OK;
}

int mjb_sync_to_host(mjbData* d) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  int rc = ensure_mirror(d);
  if (rc != MJB_OK) return rc;
  HIPCHK(hipSetDevice(d->device));
  return mirror_pull(d);
}

int mjb_sync_to_device(mjbData* d, int field_mask) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  int rc = ensure_mirror(d);
  if (rc != MJB_OK) return rc;
  HIPCHK(hipSetDevice(d->device));
  return mirror_push(d, field_mask);
}

int mjb_step_host(mjbData* d, int nstep, int field_mask) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  if (nstep < 0) return fail(MJB_ERR_ARG, "nstep must be >= 0");
  int rc = ensure_mirror(d);
  if (rc != MJB_OK) return rc;
  HIPCHK(hipSetDevice(d->device));
  ObsSpecDev none; std::memset(&none, 0, sizeof(none));
  if (nstep > 0 && mirror_zero_copy(d) && d->dtype == MJB_F32) {
    // small batches: ONE launch - the step kernel reads the edited fields from the pinned block and writes the new state back into it
    StepArgs a = make_args(d, nstep, MJB_CTRL_KEEP, 0, 0, 1.0, 0);
    a.mirror = d->mirror_host.get(); a.mirror_mask = field_mask & 63;
    double* flagword = d->mirror_host.get() + d->mirror_off[6];
    // short launches: poll the environments' completion words in the pinned block instead of waiting for the end-of-kernel signal
    // (the state words are published before them; whatever else the kernel's epilogue writes is ordered by the stream for later calls)
    static const bool poll_ok = !(std::getenv("MJB_HOST_POLL") && std::atoi(std::getenv("MJB_HOST_POLL")) == 0);
    const bool poll = poll_ok && nstep <= 64;
    if (poll) a.mirror_seq = ++d->mirror_seq;
    if ((rc = launch(d, a, none, nullptr, false)) != MJB_OK) return rc;
    bool done = false;
    if (poll) {
      const unsigned long long* words = (const unsigned long long*)(flagword + 1);
      const auto t0 = std::chrono::steady_clock::now();
      for (unsigned long spins = 0;; spins++) {
        int e = 0;
        while (e < d->batch && __atomic_load_n(words + e, __ATOMIC_ACQUIRE) == a.mirror_seq) e++;
        if (e == d->batch) { done = true; break; }
        __builtin_ia32_pause();
        // a launch that has not finished after 20 ms is not the short step this path is for (or has faulted): let the runtime wait and report
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
      }
    }
    if (!done) HIPCHK(hipStreamSynchronize(d->stream));
    if (*flagword < 0) {                                       // some environment raised an engine flag: fetch the sticky word
      int fl = 0;
      if (done) HIPCHK(hipStreamSynchronize(d->stream));        // (rare) the polled return left the kernel's epilogue in flight: the copy below must not overtake it
      HIPCHK(hipMemcpy(&fl, d->df.flags, sizeof(int), hipMemcpyDeviceToHost));
      *flagword = (double)fl;
    }
    return MJB_OK;
  }
  if ((rc = mirror_push(d, field_mask)) != MJB_OK) return rc;
  if (nstep > 0 && (rc = launch(d, make_args(d, nstep, MJB_CTRL_KEEP, 0, 0, 1.0, 0), none, nullptr, false)) != MJB_OK) return rc;
  if (nstep == 0 && (rc = launch(d, make_args(d, 1, MJB_CTRL_KEEP, 0, 0, 1.0, 1), none, nullptr, false)) != MJB_OK) return rc;   // mj_forward
  return mirror_pull(d);
}

static int ensure_shadow(mjbData* d) {
  int rc = ensure_mirror(d);
  if (rc != MJB_OK) return rc;
  if (d->mirror_shadow.empty()) d->mirror_shadow.assign(d->mirror_host.get(), d->mirror_host.get() + d->mirror_off[6]);
  return MJB_OK;
}

int mjb_mirror_edited_mask(mjbData* d, int* mask_out) {
  if (!d || !mask_out) return fail(MJB_ERR_ARG, "NULL argument");
  int rc = ensure_shadow(d);
  if (rc != MJB_OK) return rc;
  int mask = 0;
  for (int k = 0; k < 6; k++) {
    const size_t a = d->mirror_off[k], b = d->mirror_off[k + 1];
    if (b > a && std::memcmp(d->mirror_host.get() + a, d->mirror_shadow.data() + a, (b - a) * sizeof(double)) != 0) mask |= 1 << k;   // bitwise: -0.0 / NaN payload edits count
  }
  *mask_out = mask;
  return MJB_OK;
}

int mjb_mirror_commit(mjbData* d, int field_mask) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  int rc = ensure_shadow(d);
  if (rc != MJB_OK) return rc;
  for (int k = 0; k < 6; k++) if ((field_mask >> k) & 1) {
    const size_t a = d->mirror_off[k], b = d->mirror_off[k + 1];
    std::memcpy(d->mirror_shadow.data() + a, d->mirror_host.get() + a, (b - a) * sizeof(double));
  }
  return MJB_OK;
}

int mjb_step_host_auto(mjbData* d, int nstep, int compare, int* mask_out) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  int mask = 0, rc;
  if (compare && (rc = mjb_mirror_edited_mask(d, &mask)) != MJB_OK) return rc;
  if (mask_out) *mask_out = mask;
  if ((rc = mjb_step_host(d, nstep, mask)) != MJB_OK) return rc;
  return mjb_mirror_commit(d, 63);
}

// ---------------------------------------------------------------------------------------------------------------------
// observation all-gather over RCCL for a host that owns an ncclComm_t (SURVEY.md §8(b) "allgather_obs", §8(e)): the ONE
// collective of the path.  The library does not link RCCL: the symbol is taken from the RCCL the process already loaded
// (torch's bundled one, or the host's), else from librccl.so.1.
// ---------------------------------------------------------------------------------------------------------------------
int mjb_allgather_obs(void* nccl_comm, const void* send_dev, void* recv_dev, long count_per_rank, int dtype, void* hip_stream) {
  if (!nccl_comm || !send_dev || !recv_dev || count_per_rank < 0) return fail(MJB_ERR_ARG, "mjb_allgather_obs: NULL / negative argument");
  if (dtype != MJB_F32 && dtype != MJB_F64) return fail(MJB_ERR_ARG, "dtype must be MJB_F32 or MJB_F64");
  typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
  static allgather_fn fn = nullptr;
  if (!fn) {
    fn = (allgather_fn)dlsym(RTLD_DEFAULT, "ncclAllGather");
    if (!fn) {
      void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
      if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
      if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
      if (h) fn = (allgather_fn)dlsym(h, "ncclAllGather");
    }
    if (!fn) return fail(MJB_ERR_DEVICE, "ncclAllGather not found: no RCCL in this process and librccl.so.1 is not loadable");
  }
  const int nccl_dtype = dtype == MJB_F32 ? 7 /* ncclFloat32 */ : 8 /* ncclFloat64 */;
  const int rc = fn(send_dev, recv_dev, (size_t)count_per_rank, nccl_dtype, nccl_comm, (hipStream_t)hip_stream);
  if (rc != 0) return fail(MJB_ERR_DEVICE, "ncclAllGather failed with ncclResult " + std::to_string(rc));
  return MJB_OK;
}

int mjb_profile_get(mjbData* d, unsigned long long* host_out /* [24] per-phase cycle sums; zero unless built with -DMJB_PROFILE */) {
  if (!d || !host_out) return fail(MJB_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipStreamSynchronize(d->stream));
  void* p = d->dtype == MJB_F32 ? (void*)d->df.prof : (void*)d->dd.prof;
  HIPCHK(hipMemcpy(host_out, p, sizeof(unsigned long long) * PH_N, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(p, 0, sizeof(unsigned long long) * PH_N));
  return MJB_OK;
}

int mjb_step_schedule(mjbData* d, int* out6) {
  if (!d || !out6) return fail(MJB_ERR_ARG, "NULL argument");
  for (int i = 0; i < 6; i++) out6[i] = d->last_sched[i];
  return MJB_OK;
}

int mjb_profile_env_get(mjbData* d, unsigned long long* host_out /* [batch, 4]: start, end (100 MHz), HW_ID, XCC_ID; zeros unless the kernel was built with -DMJB_TIMELINE */) {
  if (!d || !host_out) return fail(MJB_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipStreamSynchronize(d->stream));
  unsigned long long* p = (d->dtype == MJB_F32 ? d->df.prof : d->dd.prof) + PH_N;
  HIPCHK(hipMemcpy(host_out, p, sizeof(unsigned long long) * 4 * (size_t)d->batch, hipMemcpyDeviceToHost));
  return MJB_OK;
}

int mjb_debug_forward(mjbData* d) {
  if (!d) return fail(MJB_ERR_ARG, "data is NULL");
  HIPCHK(hipSetDevice(d->device));
  if (!d->dbg_ready) {
    std::memset(&d->dbgf, 0, sizeof(d->dbgf)); std::memset(&d->dbgd, 0, sizeof(d->dbgd));
    int rc = d->dtype == MJB_F32 ? alloc_debug(d, d->dbgf) : alloc_debug(d, d->dbgd);
    if (rc) return fail(MJB_ERR_DEVICE, "device allocation of debug buffers failed");
    d->dbg_ready = true;
  }
  ObsSpecDev none; std::memset(&none, 0, sizeof(none));
  return launch(d, make_args(d, 1, MJB_CTRL_KEEP, 0, 0, 1.0, 1), none, nullptr, true);
}

int mjb_debug_get(mjbData* d, const char* name, void* host_out, long capacity_elems) {
  if (!d || !name || !host_out) return fail(MJB_ERR_ARG, "NULL argument");
  if (!d->dbg_ready) return fail(MJB_ERR_ARG, "call mjb_debug_forward first");
  auto it = d->dbg_arrays.find(name);
  if (it == d->dbg_arrays.end()) return fail(MJB_ERR_ARG, std::string("unknown debug array: ") + name);
  const ArrayInfo& ai = it->second;
  long n = (long)d->batch * ai.per_env;
  if (capacity_elems < n) return fail(MJB_ERR_ARG, "output buffer too small");
  HIPCHK(hipSetDevice(d->device));
  if (ai.kind == 2) {
    HIPCHK(hipStreamSynchronize(d->stream));
    HIPCHK(hipMemcpy(host_out, ai.ptr, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return MJB_OK;
  }
  return copy_out(d, ai, (double*)host_out);
}

}  // extern "C"
