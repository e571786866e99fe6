// TEST-ONLY, used by tests/test_lqr_host.py; not part of the product library.
// The source of the LQR kernels (mjb_lqr.hpp) compiled for the host with g++ -DMJB_HOST_EMU: one std::thread per lane, pthread
// barriers for the workgroup, the f64 MFMA emulated in its hardware fragment layout - the recursion, the candidate loop and the tile
// product run as the very code the GPU runs.  Also exports the host arithmetic of the argument checks and the LDS layouts.
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
// the dispatch of lqr_launch_backward (mjb_lqr.hip), one environment after the other
int lqrh_backward(const LqrBackwardArgs* p) {
  if (lqr_size_error(p->T, p->B, p->nx, p->nu)) return -1;
  std::vector<double> lds((size_t)lqr_layout(p->nx, p->nu).total + 2);
  for (int e = 0; e < p->B; e++) {
    if (lqr_waves(p->nx) == 1 && p->nu <= 8) run_block(64, [&](int tid) { lqr_backward_env<1, 8>(*p, e, tid, lds.data()); });
    else if (lqr_waves(p->nx) == 1) run_block(64, [&](int tid) { lqr_backward_env<1, kLqrMaxNu>(*p, e, tid, lds.data()); });
    else run_block(256, [&](int tid) { lqr_backward_env<4, kLqrMaxNu>(*p, e, tid, lds.data()); });
  }
  return 0;
}
int lqrh_candidates(const LqrCandArgs* p) {
  if (lqr_size_error(p->T, p->B, p->nx, p->nu) || p->nalpha < 1 || p->nalpha > kLqrMaxAlpha) return -1;
  std::vector<double> lds((size_t)lqr_cand_layout(p->nx, p->nu, p->nalpha).total + 2);
  for (int e = 0; e < p->B; e++) run_block(256, [&](int tid) { lqr_candidates_env<256>(*p, e, tid, lds.data()); });
  return 0;
}
int lqrh_gemm_tn(int M, int N, int K, const double* a, const double* b, double* c) {
  if (M <= 16) run_block(64, [&](int tid) { lqr_gemm_probe<1>(M, N, K, a, b, c, tid); });
  else run_block(256, [&](int tid) { lqr_gemm_probe<4>(M, N, K, a, b, c, tid); });
  return 0;
}
// 0 ok and *hi_out set, 1 rejected, 2 beyond 63 bits
int lqrh_highest_element(long T, long B, long n, long ss, long es, long long* hi_out) {
  __int128 hi;
  if (!lqr_highest_element(T, B, n, ss, es, hi)) return 1;
  if (hi > (__int128)0x7fffffffffffffffLL) return 2;
  *hi_out = (long long)hi;
  return 0;
}
int lqrh_size_error(long T, long B, long nx, long nu) { return lqr_size_error(T, B, nx, nu); }
int lqrh_waves(int nx) { return lqr_waves(nx); }
long lqrh_lds_bytes(int nx, int nu) { return (long)lqr_layout(nx, nu).total * 8; }
long lqrh_cand_lds_bytes(int nx, int nu, int nalpha) { return (long)lqr_cand_layout(nx, nu, nalpha).total * 8; }
// 1 when no two arrays that are live in the same half of a step overlap and everything lies inside `total`
int lqrh_layout_ok(int nx, int nu) {
  const LqrLay l = lqr_layout(nx, nu);
  struct Seg { int o, n; };
  const Seg keep[] = {{l.Vxx, nx * nx}, {l.Qux, nu * nx}, {l.Quu, nu * nu}, {l.Vx, nx}, {l.Qx, nx}, {l.Qu, nu}, {l.wq, nu}};
  const Seg half1[] = {{l.A, nx * nx}, {l.VA, nx * nx}, {l.B, nx * nu}, {l.VB, nx * nu}};
  const Seg half2[] = {{l.Qw, nu * nu}, {l.L, nu * kLqrMaxNu}, {l.R, nu * (nx + 1)}, {l.S, nu * nx}};
  auto disjoint = [](const Seg& a, const Seg& b) { return a.o + a.n <= b.o || b.o + b.n <= a.o; };
  std::vector<Seg> s1(keep, keep + 7), s2(keep, keep + 7);
  s1.insert(s1.end(), half1, half1 + 4); s2.insert(s2.end(), half2, half2 + 4);
  for (auto* v : {&s1, &s2})
    for (size_t i = 0; i < v->size(); i++) {
      if ((*v)[i].o < 0 || (*v)[i].o + (*v)[i].n > l.total) return 0;
      for (size_t j = i + 1; j < v->size(); j++) if (!disjoint((*v)[i], (*v)[j])) return 0;
    }
  return 1;
}
}
