// The kernel of mjb_feedback_law / mjb_rollout_feedback (mjb_feedback.hpp) and its launch.  One wavefront per environment,
// feedback_waves(nu, nv) wavefronts per workgroup, no workgroup barrier.
#include "mjb_feedback.hpp"

namespace mjb {

extern __shared__ __attribute__((aligned(16))) double feedback_lds[];

__global__ __launch_bounds__(256) void k_feedback_law(FeedbackLawArgs p, int per_wave) {
  const int wave = (int)threadIdx.x >> 6, waves = (int)blockDim.x >> 6;
  const long e = (long)blockIdx.x * waves + wave;
  if (e >= p.B) return;                                          // whole waves only: no barrier follows
  feedback_env(p, (int)e, (int)threadIdx.x & 63, feedback_lds + (size_t)wave * per_wave);
}

hipError_t feedback_launch(const FeedbackLawArgs& p, hipStream_t stream) {
  const int per_wave = feedback_lds_doubles(p.nu, p.nv), waves = feedback_waves(p.nu, p.nv);
  const size_t bytes = (size_t)per_wave * waves * sizeof(double);
  if (bytes > 64 * 1024) return hipErrorInvalidValue;             // never at nu <= 32, nv <= 64: feedback_waves sees to it
  hipLaunchKernelGGL(k_feedback_law, dim3((unsigned)((p.B + waves - 1) / waves)), dim3(64 * waves), bytes, stream, p, per_wave);
  return hipGetLastError();
}

}  // namespace mjb
