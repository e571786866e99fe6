// TEST-ONLY, used by tests/test_dlyap_host.py; not part of the product library.
// The source of the Lyapunov kernel (mjb_dlyap.hpp) compiled for the host with g++ -DMJB_HOST_EMU: one std::thread per lane, pthread
// barriers for the workgroup, the f64 MFMA emulated in its hardware fragment layout - the squared Smith iteration runs as the very
// code the GPU runs.  Also exports the LDS layout.
#define MJB_HOST_EMU 1
#include <thread>
#include <vector>

#include "../mujoco_template_amd/csrc/mjb_dlyap.hpp"

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
// the dispatch of dlyap_launch (mjb_dlyap.hip), one problem after the other
int dlyaph_solve(const DlyapArgs* p) {
  if (dlyap_size_error(p->B, p->nx, p->nu, p->nu > 0, p->max_iter, p->tol, (long)p->sign)) return -1;
  std::vector<double> lds((size_t)dlyap_layout(p->nx, p->nu).total + 2);
  for (int e = 0; e < p->B; e++) {
    if (lqr_waves(p->nx) == 1) run_block(64, [&](int tid) { dlyap_env<1>(*p, e, tid, lds.data()); });
    else run_block(256, [&](int tid) { dlyap_env<4>(*p, e, tid, lds.data()); });
  }
  return 0;
}
int dlyaph_size_error(long B, long nx, long nu, int has_bk, long max_iter, double tol, long sign) {
  return dlyap_size_error(B, nx, nu, has_bk, max_iter, tol, sign);
}
long dlyaph_lds_bytes(int nx, int nu) { return (long)dlyap_layout(nx, nu).total * 8; }
// 1 when no two blocks that are live together overlap and everything lies inside `total`
int dlyaph_layout_ok(int nx, int nu) {
  const DlyapLay l = dlyap_layout(nx, nu);
  const int nt = 64 * lqr_waves(nx);
  if (l.ld != (nx | 1)) return 0;
  struct Seg { int o, n; };
  const Seg keep[] = {{l.M, nx * l.ld}, {l.W, nx * l.ld}, {l.red, 2 * nt}, {l.red2, 32}};
  const Seg half1[] = {{l.P, nx * l.ld}};
  const Seg half2[] = {{l.Ks, nu * nx}, {l.RK, nu * nx}};
  auto disjoint = [](const Seg& a, const Seg& b) { return a.o + a.n <= b.o || b.o + b.n <= a.o; };
  std::vector<Seg> s1(keep, keep + 4), s2(keep, keep + 4);
  s1.insert(s1.end(), half1, half1 + 1); s2.insert(s2.end(), half2, half2 + 2);
  for (auto* v : {&s1, &s2})
    for (size_t i = 0; i < v->size(); i++) {
      if ((*v)[i].o < 0 || (*v)[i].o + (*v)[i].n > l.total) return 0;
      for (size_t j = i + 1; j < v->size(); j++) if (!disjoint((*v)[i], (*v)[j])) return 0;
    }
  return 1;
}
}
