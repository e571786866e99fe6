// TEST-ONLY: the step kernel's per-environment driver env_run (mjb_device.hpp) compiled for the host with g++ -DMJB_HOST_EMU
// (one std::thread per lane, mjb_hostemu.hpp) and run over a small batch the way k_step runs it, with the observation ring of
// mjb_rollout_ctrl (qpos | qvel | sensordata | time every step).  ctrl_mode CTRL_SEQUENCE reads the control table at
// (step * step_stride + env * env_stride); CTRL_KEEP steps on the ctrl array as it is.  Used by tests/test_ctrl_sequence_host.py;
// not part of the product library.
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
const char* ctrlseq_last_error() { return g_err.c_str(); }

// state arrays [batch, n] float64 (time [batch], counters int [batch, 8], sensordata [batch, nsensordata]) advanced in place;
// ring [nstep, batch, nq + nv + nsensordata + 1]
int ctrlseq_run(int nfield, const char* const* names, const void* const* ptrs, const int* dtypes, const long* counts,
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
  obs.flags = 1 | 2 | 8 | 16;                                   // qpos, qvel, sensordata, time
  obs.dim = h.nq + h.nv + h.nsensordata + 1;
  return use_double ? run_typed<double>(h, G, ncon_max, nefc_max, d, a, obs, ring)
                    : run_typed<float>(h, G, ncon_max, nefc_max, d, a, obs, ring);
}
}
