// TEST-ONLY, used by tests/test_fd_points_host.py; not part of the product library.
//  (a) fdp_run: the step kernel's per-environment driver env_run (mjb_device.hpp) compiled for the host with g++ -DMJB_HOST_EMU (one
//      std::thread per lane, mjb_hostemu.hpp) over a small batch, recording the observation ring of the caller's flag word every step:
//      qpos | qvel | sensordata | time (flags 27, the ring of mjb_rollout_ctrl) and, with flag 128, qacc_warmstart behind them.
//  (b) the host arithmetic of mjb_transition_fd_points (mjb_host.hpp): highest element of a strided array, the extent check, the slab
//      plan and the columns-per-job rule, exported for ctypes.
#define MJB_HOST_EMU 1
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../mujoco_template_amd/csrc/mjb_device.hpp"
#include "../mujoco_template_amd/csrc/mjb_host.hpp"

using namespace mjb;

namespace {
std::string g_err;

template <typename T> struct HostAlloc {
  std::vector<std::vector<T>> f; std::vector<std::vector<int>> i; std::vector<std::vector<unsigned long long>> u;
  const T* putf(const std::vector<T>& v) { f.push_back(v); if (f.back().empty()) f.back().resize(1); return f.back().data(); }
  const int* puti(const std::vector<int>& v) { i.push_back(v); if (i.back().empty()) i.back().resize(1); return i.back().data(); }
  const unsigned long long* putu(const std::vector<unsigned long long>& v) { u.push_back(v); return u.back().data(); }
};

template <typename T, int G>
void run_batch(const DevModel<T>& m, const Lay& L, const DevData<double>& d, const StepArgs& a, const ObsSpecDev& obs, double* ring) {
  DevDebug<double> dbg;
  std::memset(&dbg, 0, sizeof(dbg));
  for (int env = 0; env < d.batch; env++) {
    std::vector<char> lds((size_t)L.bytes + 64, 0);
    T* w = (T*)lds.data();
    int* wi = (int*)(w + L.nT);
    emu::Group grp(G);
    std::vector<std::thread> th;
    for (int lane = 0; lane < G; lane++) {
      th.emplace_back([&, lane]() {
        emu::tl_group = &grp; emu::tl_lane = lane;
        env_run<T, double, G>(&m, &L, d, dbg, a, obs, ring, w, wi, env, lane, 0, a.nstep, 0u);
      });
    }
    for (auto& t : th) t.join();
  }
}

template <typename T>
int run_typed(const HostModel& h, int G, int ncon_max, int nefc_max, const DevData<double>& d, const StepArgs& a, const ObsSpecDev& obs,
              double* ring) {
  HostAlloc<T> alloc;
  DevModel<T> m;
  fill_dev_model<T>(h, alloc, ncon_max, nefc_max, m);
  Lay L = make_layout(h, ncon_max, nefc_max, sizeof(T));
  switch (G) {
    case 16: run_batch<T, 16>(m, L, d, a, obs, ring); break;
    case 64: run_batch<T, 64>(m, L, d, a, obs, ring); break;
    default: g_err = "unsupported G"; return -1;
  }
  return 0;
}
}  // namespace

extern "C" {
const char* fdp_last_error() { return g_err.c_str(); }

// state arrays [batch, n] float64 (time [batch], counters int [batch, 8], sensordata [batch, nsensordata]) advanced in place;
// ring [nstep, batch, nq + nv + nsensordata + 1 (+ nv with flag 128)]
int fdp_run(int obs_flags, int nfield, const char* const* names, const void* const* ptrs, const int* dtypes, const long* counts,
                int G, int use_double, int ncon_max, int nefc_max, int batch, int nstep, int ctrl_mode,
                const double* ctrl_seq, long step_stride, long env_stride,
                double* qpos, double* qvel, double* ctrl, double* qacc, double* qacc_ws, double* time, int* counters, double* sensordata,
                double* ring) {
  Table t{nfield, names, ptrs, dtypes, counts};
  HostModel h;
  if (!h.load(t, g_err)) return -1;
  if (ncon_max <= 0) ncon_max = h.ncon_alloc;
  if (nefc_max <= 0) nefc_max = h.nefc_alloc;
  std::vector<double> xpos((size_t)batch * 3 * h.nbody + 1), xquat((size_t)batch * 4 * h.nbody + 1), xipos((size_t)batch * 3 * h.nbody + 1),
      sub((size_t)batch * 3 * h.nbody + 1), site((size_t)batch * 3 * h.nsite + 1), geom((size_t)batch * 3 * h.ngeom + 1);
  DevData<double> d;
  std::memset(&d, 0, sizeof(d));
  d.batch = batch;
  d.qpos = qpos; d.qvel = qvel; d.ctrl = ctrl; d.qacc = qacc; d.qacc_warmstart = qacc_ws; d.time = time; d.counters = counters;
  d.sensordata = sensordata; d.xpos = xpos.data(); d.xquat = xquat.data(); d.xipos = xipos.data(); d.subtree_com = sub.data();
  d.site_xpos = site.data(); d.geom_xpos = geom.data();
  StepArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nstep = nstep; a.ctrl_mode = ctrl_mode; a.dt = h.timestep; a.mode = 0; a.write_kin = 1; a.obs_every = 1;
  a.ctrl_seq = ctrl_seq; a.ctrl_step_stride = step_stride; a.ctrl_env_stride = env_stride;
  ObsSpecDev obs;
  std::memset(&obs, 0, sizeof(obs));
  if ((obs_flags & ~128) != (1 | 2 | 8 | 16)) { g_err = "obs_flags must be 27 or 27 | 128"; return -1; }
  obs.flags = obs_flags;                                        // qpos, qvel, sensordata, time [, qacc_warmstart]
  obs.dim = h.nq + h.nv + h.nsensordata + 1 + ((obs_flags & 128) ? h.nv : 0);
  return use_double ? run_typed<double>(h, G, ncon_max, nefc_max, d, a, obs, ring)
                    : run_typed<float>(h, G, ncon_max, nefc_max, d, a, obs, ring);
}

// ---- (b) ----
// hi_out: the highest element index (-1: nothing touched); returns 0 ok, 1 rejected (negative stride / empty extent), 2 hi beyond 63 bits
int fdp_highest_element(long T, long B, long n, long step_stride, long env_stride, long long* hi_out) {
  __int128 hi;
  if (!fd_highest_element(T, B, n, step_stride, env_stride, hi)) return 1;
  if (hi > (__int128)0x7fffffffffffffffLL) return 2;
  *hi_out = (long long)hi;
  return 0;
}
int fdp_extent_inside(unsigned long long ptr, long long hi, unsigned long long esize, unsigned long long base, unsigned long long size) {
  return fd_extent_inside(ptr, (__int128)hi, esize, base, size) ? 1 : 0;
}
unsigned long long fdp_point_scratch_bytes(int nq, int nv, int nu) { return fd_point_scratch_bytes(nq, nv, nu); }
long fdp_slab_points(unsigned long long bytes_per_point, unsigned long long budget) { return fd_slab_points(bytes_per_point, budget); }
long fdp_slab_count(long npoint, long per_slab) { return fd_slab_count(npoint, per_slab); }
int fdp_slab(long npoint, long per_slab, long k, long* p0, long* n) { return fd_slab(npoint, per_slab, k, *p0, *n) ? 1 : 0; }
int fdp_chunk_rule(long npoint, int ncol, long slots) { return fd_chunk_rule(npoint, ncol, slots); }
}
