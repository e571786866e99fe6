// TEST-ONLY, used by tests/test_setpoint_host.py; not part of the product library.
// The source of the set-point kernel (mjb_setpoint.hpp) compiled for the host with g++ -DMJB_HOST_EMU: one std::thread per lane,
// pthread barriers for the wavefront - the Jacobi sweeps run as the very code the GPU runs.  Also exports the LDS layout, the
// schedule and the size-error function.
#define MJB_HOST_EMU 1
#include <thread>
#include <vector>

#include "../mujoco_template_amd/csrc/mjb_setpoint.hpp"

using namespace mjb;

namespace {
template <class F> void run_block(int nthreads, F body) {
  lqremu::Block blk(nthreads);
  std::vector<std::thread> th;
  for (int tid = 0; tid < nthreads; tid++)
    th.emplace_back([&, tid]() { lqremu::tl_block = &blk; lqremu::tl_tid = tid; body(tid); });
  for (auto& t : th) t.join();
}
}  // namespace

extern "C" {
// the dispatch of setpoint_launch (mjb_setpoint.hip), one problem after the other
int setpointh_solve(const SetpointArgs* p) {
  if (setpoint_size_error(p->B, p->nu, p->nv, p->max_sweeps, p->rcond_min)) return -1;
  std::vector<double> lds((size_t)setpoint_layout(p->nu, p->nv).total + 2);
  for (int e = 0; e < p->B; e++) run_block(64, [&](int tid) { setpoint_env(*p, e, tid, lds.data()); });
  return 0;
}
int setpointh_size_error(long B, long nu, long nv, long max_sweeps, double rcond_min) { return setpoint_size_error(B, nu, nv, max_sweeps, rcond_min); }
long setpointh_lds_bytes(int nu, int nv) { return (long)setpoint_layout(nu, nv).total * 8; }
// 1 when no two blocks overlap, everything lies inside `total` and both leading dimensions are odd and large enough
int setpointh_layout_ok(int nu, int nv) {
  const SetpointLay l = setpoint_layout(nu, nv);
  if (l.ldg != (nv | 1) || l.ldv != (nu | 1)) return 0;
  struct Seg { int o, n; };
  const Seg s[] = {{l.G, nu * l.ldg}, {l.V, nu * l.ldv}, {l.q, nv}, {l.red, 192}, {l.flg, 64}, {l.s2, nu}, {l.sg, nu}, {l.perm, nu}, {l.wq, nu}, {l.u, nu}};
  const int ns = (int)(sizeof(s) / sizeof(s[0]));
  for (int i = 0; i < ns; i++) {
    if (s[i].o < 0 || s[i].o + s[i].n > l.total) return 0;
    for (int j = i + 1; j < ns; j++) if (!(s[i].o + s[i].n <= s[j].o || s[j].o + s[j].n <= s[i].o)) return 0;
  }
  return 1;
}
// pair k of round rd for nu columns: out2 = (i, j); returns 1 when the pair is active (j < nu)
int setpointh_pair(int nu, int rd, int k, int* out2) {
  const int n2 = 2 * ((nu + 1) >> 1);
  setpoint_pair(n2, rd, k, out2[0], out2[1]);
  return out2[1] < nu ? 1 : 0;
}
}
