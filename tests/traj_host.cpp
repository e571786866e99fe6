// TEST-ONLY, used by tests/test_traj_cost_host.py; not part of the product library.
// The source of the trajectory-cost and selection kernels (mjb_traj.hpp) compiled for the host with g++ -DMJB_HOST_EMU: one std::thread
// per lane, a pthread barrier for the workgroup - the tiles, the cost sum and the selection run as the very code the GPU runs, in the
// launch shapes of mjb_traj.hip.  Also exports the host arithmetic of the argument checks.
#define MJB_HOST_EMU 1
#include <thread>
#include <vector>

#include "../mujoco_template_amd/csrc/mjb_traj.hpp"

using namespace mjb;

namespace {
template <class F> void run_block(int nthreads, F body) {
  trajemu::Block blk(nthreads);
  std::vector<std::thread> th;
  for (int tid = 0; tid < nthreads; tid++)
    th.emplace_back([&, tid]() { trajemu::tl_block = &blk; body(tid); });
  for (auto& t : th) t.join();
}
}  // namespace

extern "C" {
// k_traj_cost with a grid of `grid` workgroups (each takes the tiles blockIdx, blockIdx + grid, ...), then k_traj_cost_sum
int trajh_cost(const TrajCostArgs* p, int grid) {
  if (traj_cost_size_error(p->T, p->B, p->nq, p->nv, p->nu) || grid < 1) return -1;
  const long ntile = traj_cost_tiles(p->T, p->B);
  for (int b = 0; b < grid; b++) {
    std::vector<double> lds((size_t)traj_cost_lds(p->nv, p->nu));
    run_block(64, [&](int lane) { for (long tile = b; tile < ntile; tile += grid) traj_cost_tile(*p, tile, lane, lds.data()); });
  }
  std::vector<double> lds(64);
  run_block(64, [&](int lane) { for (long e = 0; e < p->B; e++) traj_cost_sum(*p, e, lane, lds.data()); });
  return 0;
}
int trajh_select(const TrajSelectArgs* p) {
  if (traj_select_size_error(p->nprob, p->ncand, p->T, p->nu, p->mode, p->temperature)) return -1;
  const long chunks = traj_select_chunks(p->T, p->nu);
  std::vector<double> lds((size_t)traj_select_lds());
  for (long chunk = 0; chunk < chunks; chunk++)
    run_block(kTrajSelThreads, [&](int tid) { for (long g = 0; g < p->nprob; g++) traj_select_block(*p, g, chunk, tid, lds.data()); });
  return 0;
}
// 0 ok and *hi_out set, 1 rejected, 2 beyond 63 bits
int trajh_highest_element(long nstep, long B, long n, long ss, long es, long long* hi_out) {
  __int128 hi;
  if (!traj_highest_element(nstep, B, n, ss, es, hi)) return 1;
  if (hi > (__int128)0x7fffffffffffffffLL) return 2;
  *hi_out = (long long)hi;
  return 0;
}
int trajh_cost_size_error(long T, long B, long nq, long nv, long nu) { return traj_cost_size_error(T, B, nq, nv, nu); }
int trajh_select_size_error(long nprob, long ncand, long T, long nu, int mode, double temperature) {
  return traj_select_size_error(nprob, ncand, T, nu, mode, temperature);
}
long trajh_cost_tiles(long T, long B) { return traj_cost_tiles(T, B); }
long trajh_cost_lds_bytes(int nv, int nu) { return (long)traj_cost_lds(nv, nu) * 8; }
}
