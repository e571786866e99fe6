// TEST-ONLY, used by tests/test_feedback_host.py; not part of the product library.
// The source of the feedback-law kernel (mjb_feedback.hpp) compiled for the host with g++ -DMJB_HOST_EMU: one std::thread per lane, a
// pthread barrier for the wavefront - the sweep over K, the products in LDS and the row sums run as the very code the GPU runs.  Also
// exports the argument checker and the LDS sizes.
#define MJB_HOST_EMU 1
#include <thread>
#include <vector>

#include "../mujoco_template_amd/csrc/mjb_feedback.hpp"

using namespace mjb;

extern "C" {
// the dispatch of feedback_launch (mjb_feedback.hip), one environment after the other; the checker's code when it refuses
int fbh_law(const FeedbackLawArgs* p) {
  if (const int why = feedback_arg_error(*p, 1)) return why;
  std::vector<double> lds((size_t)feedback_lds_doubles(p->nu, p->nv) + 2);
  double* w = lds.data() + (((uintptr_t)lds.data() & 15) ? 1 : 0);          // 16-byte aligned, as the dynamic LDS base is
  for (int e = 0; e < p->B; e++) {
    fbemu::Block blk(64);
    std::vector<std::thread> th;
    for (int lane = 0; lane < 64; lane++)
      th.emplace_back([&, lane]() { fbemu::tl_block = &blk; feedback_env(*p, e, lane, w); });
    for (auto& t : th) t.join();
  }
  return 0;
}
int fbh_arg_error(const FeedbackLawArgs* p, long nstep) { return feedback_arg_error(*p, nstep); }
int fbh_lds_doubles(int nu, int nv) { return feedback_lds_doubles(nu, nv); }
int fbh_waves(int nu, int nv) { return feedback_waves(nu, nv); }
}
