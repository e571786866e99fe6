// TEST-ONLY, used by tests/test_dare_host.py; not part of the product library.
// The source of the DARE kernel (mjb_dare.hpp) compiled for the host with g++ -DMJB_HOST_EMU: one std::thread per lane, pthread
// barriers for the workgroup, the f64 MFMA emulated in its hardware fragment layout - the doubling iteration runs as the very code
// the GPU runs.  Also exports the LDS layout and the packed G / H accessors.
#define MJB_HOST_EMU 1
#include <thread>
#include <vector>

#include "../mujoco_template_amd/csrc/mjb_dare.hpp"

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
// the dispatch of dare_launch (mjb_dare.hip), one problem after the other
int dareh_solve(const DareArgs* p) {
  if (dare_size_error(p->B, p->nx, p->nu, p->max_iter, p->tol)) return -1;
  std::vector<double> lds((size_t)dare_layout(p->nx, p->nu).total + 2);
  for (int e = 0; e < p->B; e++) {
    if (lqr_waves(p->nx) == 1 && p->nu <= 8) run_block(64, [&](int tid) { dare_env<1, 8>(*p, e, tid, lds.data()); });
    else if (lqr_waves(p->nx) == 1) run_block(64, [&](int tid) { dare_env<1, kLqrMaxNu>(*p, e, tid, lds.data()); });
    else run_block(256, [&](int tid) { dare_env<4, kLqrMaxNu>(*p, e, tid, lds.data()); });
  }
  return 0;
}
int dareh_size_error(long B, long nx, long nu, long max_iter, double tol) { return dare_size_error(B, nx, nu, max_iter, tol); }
long dareh_lds_bytes(int nx, int nu) { return (long)dare_layout(nx, nu).total * 8; }
// 1 when no two blocks that are live together overlap and everything lies inside `total`
int dareh_layout_ok(int nx, int nu) {
  const DareLay l = dare_layout(nx, nu);
  const int nt = 64 * lqr_waves(nx);
  struct Seg { int o, n; };
  const Seg keep[] = {{l.S, nx * l.lds}, {l.A, nx * l.ld}, {l.perm, nx}, {l.red, 2 * nt}};
  const Seg half1[] = {{l.W, nx * l.ld}, {l.X, nx * l.ld}, {l.XL, (nx * l.ld + 1) / 2}};
  const Seg half2[] = {{l.Bm, nx * nu}, {l.Z, nu * nx}, {l.XB, nx * nu}, {l.M, nu * nu}, {l.L, nu * kLqrMaxNu}};
  auto disjoint = [](const Seg& a, const Seg& b) { return a.o + a.n <= b.o || b.o + b.n <= a.o; };
  std::vector<Seg> s1(keep, keep + 4), s2(keep, keep + 4);
  s1.insert(s1.end(), half1, half1 + 3); s2.insert(s2.end(), half2, half2 + 5);
  for (auto* v : {&s1, &s2})
    for (size_t i = 0; i < v->size(); i++) {
      if ((*v)[i].o < 0 || (*v)[i].o + (*v)[i].n > l.total) return 0;
      for (size_t j = i + 1; j < v->size(); j++) if (!disjoint((*v)[i], (*v)[j])) return 0;
    }
  return 1;
}
// The packed pair: writes h(i, j) = 1000 i + j (i >= j) and g(i, j) = -(1000 i + j) - 1 (i <= j) through the accessors into a buffer of
// nx (nx + 1) doubles, then reads every (i, j) back both ways round.  1 when nothing collides, every word is used once and g, h are symmetric.
int dareh_packed_roundtrip(int nx) {
  const int lds = nx + 1;
  std::vector<double> S((size_t)nx * lds, 0.0);
  std::vector<int> used((size_t)nx * lds, 0);
  for (int i = 0; i < nx; i++)
    for (int j = 0; j <= i; j++) {
      const int h = dare_h_index(i, j, lds), g = dare_g_index(j, i, lds);
      if (h < 0 || h >= nx * lds || g < 0 || g >= nx * lds) return 0;
      used[h]++; used[g]++;
      S[h] = 1000.0 * i + j; S[g] = -(1000.0 * j + i) - 1.0;
    }
  for (int v : used) if (v != 1) return 0;
  for (int i = 0; i < nx; i++)
    for (int j = 0; j < nx; j++) {
      const int hi = i > j ? i : j, lo = i > j ? j : i;
      if (S[dare_h_index(i, j, lds)] != 1000.0 * hi + lo) return 0;
      if (S[dare_g_index(i, j, lds)] != -(1000.0 * lo + hi) - 1.0) return 0;
    }
  return 1;
}
}
