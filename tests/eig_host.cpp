// TEST-ONLY, used by tests/test_eig_host.py; not part of the product library.
// The source of the eigenvalue kernel (mjb_eig.hpp) compiled for the host with g++ -DMJB_HOST_EMU: one std::thread per lane, pthread
// barriers for the wavefront, the f64 MFMA emulated in its hardware fragment layout - balancing, the Hessenberg reduction and the
// Francis iteration run as the very code the GPU runs.  Also exports the LDS layout, the size check and eig_hypot.
#define MJB_HOST_EMU 1
#include <thread>
#include <vector>

#include "../mujoco_template_amd/csrc/mjb_eig.hpp"

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
// the dispatch of eig_launch (mjb_eig.hip), one problem after the other
int eigh_solve(const EigArgs* p) {
  if (eig_size_error(p->B, p->nx, p->nu, p->nu > 0, p->max_sweeps, (long)p->sign)) return -1;
  std::vector<double> lds((size_t)eig_layout(p->nx, p->nu).total + 2);
  for (int e = 0; e < p->B; e++) run_block(64, [&](int tid) { eig_env(*p, e, tid, lds.data()); });
  return 0;
}
int eigh_size_error(long B, long nx, long nu, int has_bk, long max_sweeps, long sign) { return eig_size_error(B, nx, nu, has_bk, max_sweeps, sign); }
int eigh_default_sweeps(int nx) { return eig_default_sweeps(nx); }
long eigh_lds_bytes(int nx, int nu) { return (long)eig_layout(nx, nu).total * 8; }
double eigh_hypot(double x, double y) { return eig_hypot(x, y); }
// 1 when no two blocks that are live together overlap and everything lies inside `total`
int eigh_layout_ok(int nx, int nu) {
  const EigLay l = eig_layout(nx, nu);
  struct Seg { int o, n; };
  const Seg keep[] = {{l.H, nx * l.ld}, {l.sc, nx}};
  const Seg half1[] = {{l.wr, nx}, {l.wi, nx}, {l.v, nx}, {l.red, 64}};
  const Seg half2[] = {{l.Ks, nu * nx}};
  auto disjoint = [](const Seg& a, const Seg& b) { return a.n == 0 || b.n == 0 || a.o + a.n <= b.o || b.o + b.n <= a.o; };
  std::vector<Seg> s1(keep, keep + 2), s2(keep, keep + 2);
  s1.insert(s1.end(), half1, half1 + 4); s2.insert(s2.end(), half2, half2 + 1);
  if (l.ld != (nx | 1)) return 0;
  for (auto* v : {&s1, &s2})
    for (size_t i = 0; i < v->size(); i++) {
      if ((*v)[i].o < 0 || (*v)[i].o + (*v)[i].n > l.total) return 0;
      for (size_t j = i + 1; j < v->size(); j++) if (!disjoint((*v)[i], (*v)[j])) return 0;
    }
  return 1;
}
}
