// TEST-ONLY, used by tests/test_lqr_box_host.py; not part of the product library.
// The control-limited backward pass of mjb_lqr.hpp compiled for the host with g++ -DMJB_HOST_EMU, by the emulation of lqr_host.cpp
// (one std::thread per lane, pthread barriers, the emulated f64 MFMA), next to the unconstrained recursion it must reduce to.
#define MJB_HOST_EMU 1
#include <thread>
#include <vector>

#include "../mujoco_template_amd/csrc/mjb_lqr.hpp"

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
// the dispatch of lqr_launch_backward_box (mjb_lqr.hip), one environment after the other
int lqrbh_backward_box(const LqrBoxArgs* p) {
  const int nx = p->b.nx, nu = p->b.nu;
  if (lqr_size_error(p->b.T, p->b.B, nx, nu)) return -1;
  std::vector<double> lds((size_t)lqr_box_layout(nx, nu).total + 2);
  for (int e = 0; e < p->b.B; e++) {
    if (lqr_waves(nx) == 1 && nu <= 8) run_block(64, [&](int tid) { lqr_backward_box_env<1, 8>(*p, e, tid, lds.data()); });
    else if (lqr_waves(nx) == 1) run_block(64, [&](int tid) { lqr_backward_box_env<1, kLqrMaxNu>(*p, e, tid, lds.data()); });
    else run_block(256, [&](int tid) { lqr_backward_box_env<4, kLqrMaxNu>(*p, e, tid, lds.data()); });
  }
  return 0;
}
int lqrbh_backward(const LqrBackwardArgs* p) {
  if (lqr_size_error(p->T, p->B, p->nx, p->nu)) return -1;
  std::vector<double> lds((size_t)lqr_layout(p->nx, p->nu).total + 2);
  for (int e = 0; e < p->B; e++) {
    if (lqr_waves(p->nx) == 1 && p->nu <= 8) run_block(64, [&](int tid) { lqr_backward_env<1, 8>(*p, e, tid, lds.data()); });
    else if (lqr_waves(p->nx) == 1) run_block(64, [&](int tid) { lqr_backward_env<1, kLqrMaxNu>(*p, e, tid, lds.data()); });
    else run_block(256, [&](int tid) { lqr_backward_env<4, kLqrMaxNu>(*p, e, tid, lds.data()); });
  }
  return 0;
}
long lqrbh_lds_bytes(int nx, int nu) { return (long)lqr_box_layout(nx, nu).total * 8; }
// 1 when no two arrays that are live in the same half of a step overlap and everything lies inside `total`
int lqrbh_layout_ok(int nx, int nu) {
  const LqrBoxLay b = lqr_box_layout(nx, nu);
  const LqrLay& l = b.l;
  struct Seg { int o, n; };
  const Seg keep[] = {{l.Vxx, nx * nx}, {l.Qux, nu * nx}, {l.Quu, nu * nu}, {l.Vx, nx}, {l.Qx, nx}, {l.Qu, nu}, {l.wq, nu}};
  const Seg half1[] = {{l.A, nx * nx}, {l.VA, nx * nx}, {l.B, nx * nu}, {l.VB, nx * nu}};
  const Seg half2[] = {{l.Qw, nu * nu}, {l.L, nu * kLqrMaxNu}, {l.R, nu * (nx + 1)}, {l.S, nu * nx}, {b.x, nu}, {b.xs, nu}, {b.g, nu},
                       {b.lob, nu}, {b.hib, nu}, {b.cf, nu}, {b.fe, nu}, {b.pass, kLqrQpTrials}};
  auto disjoint = [](const Seg& a, const Seg& c) { return a.o + a.n <= c.o || c.o + c.n <= a.o; };
  std::vector<Seg> s1(keep, keep + 7), s2(keep, keep + 7);
  s1.insert(s1.end(), half1, half1 + 4); s2.insert(s2.end(), half2, half2 + 12);
  if (b.total < l.total) return 0;
  for (auto* v : {&s1, &s2})
    for (size_t i = 0; i < v->size(); i++) {
      if ((*v)[i].o < 0 || (*v)[i].o + (*v)[i].n > b.total) return 0;
      for (size_t j = i + 1; j < v->size(); j++) if (!disjoint((*v)[i], (*v)[j])) return 0;
    }
  return 1;
}
}
