// The kernel of mjb_lqr_eig (mjb_eig.hpp) and its launch.  One workgroup of one wavefront per problem.
#include "mjb_eig.hpp"

namespace mjb {

extern __shared__ double eig_lds[];

__global__ __launch_bounds__(64) void k_lqr_eig(EigArgs p) { eig_env(p, (int)blockIdx.x, (int)threadIdx.x, eig_lds); }

hipError_t eig_launch(const EigArgs& p, hipStream_t stream) {
  const size_t bytes = (size_t)eig_layout(p.nx, p.nu).total * sizeof(double);
  if (bytes > 64 * 1024) return hipErrorInvalidValue;             // never at nx <= 64, nu <= 32: 49.7 KB at the limit
  hipLaunchKernelGGL(k_lqr_eig, dim3((unsigned)p.B), dim3(64), bytes, stream, p);
  return hipGetLastError();
}

}  // namespace mjb
