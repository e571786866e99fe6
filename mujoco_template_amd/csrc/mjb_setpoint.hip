// The kernel of mjb_setpoint_ctrl (mjb_setpoint.hpp) and its launch.  One workgroup of one wavefront per problem.
#include "mjb_setpoint.hpp"

namespace mjb {

extern __shared__ double setpoint_lds[];

__global__ __launch_bounds__(64) void k_setpoint(SetpointArgs p) { setpoint_env(p, (int)blockIdx.x, (int)threadIdx.x, setpoint_lds); }

hipError_t setpoint_launch(const SetpointArgs& p, hipStream_t stream) {
  const size_t bytes = (size_t)setpoint_layout(p.nu, p.nv).total * sizeof(double);
  if (bytes > 64 * 1024) return hipErrorInvalidValue;             // never at nu <= 32, nv <= 64: 28.3 KB at the limit
  hipLaunchKernelGGL(k_setpoint, dim3((unsigned)p.B), dim3(64), bytes, stream, p);
  return hipGetLastError();
}

}  // namespace mjb
