// The kernels of mjb_lqr_dare (mjb_dare.hpp) and their launch.  One workgroup per problem.
#include "mjb_dare.hpp"

namespace mjb {

extern __shared__ double dare_lds[];

template <int NW, int MU> __global__ __launch_bounds__(64 * NW) void k_lqr_dare(DareArgs p) {
  dare_env<NW, MU>(p, (int)blockIdx.x, (int)threadIdx.x, dare_lds);
}

// Dynamic LDS above the default limit is allowed once per kernel variant and device, for the 160 KB the LQR launches request
// (the layout is checked against it before a launch).
static const size_t kDareLdsMax = 160 * 1024;
template <auto kern> static hipError_t dare_lds_limit(size_t bytes) {
  static bool done[64] = {};
  if (bytes > kDareLdsMax) return hipErrorInvalidValue;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
  e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDareLdsMax);
  if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
  return e;
}

hipError_t dare_launch(const DareArgs& p, hipStream_t stream) {                   // the dispatch of lqr_launch_backward
  const size_t bytes = (size_t)dare_layout(p.nx, p.nu).total * sizeof(double);
  hipError_t e;
  if (lqr_waves(p.nx) == 1 && p.nu <= 8) {
    if ((e = dare_lds_limit<k_lqr_dare<1, 8>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_dare<1, 8>), dim3((unsigned)p.B), dim3(64), bytes, stream, p);
  } else if (lqr_waves(p.nx) == 1) {
    if ((e = dare_lds_limit<k_lqr_dare<1, kLqrMaxNu>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_dare<1, kLqrMaxNu>), dim3((unsigned)p.B), dim3(64), bytes, stream, p);
  } else {
    if ((e = dare_lds_limit<k_lqr_dare<4, kLqrMaxNu>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_dare<4, kLqrMaxNu>), dim3((unsigned)p.B), dim3(256), bytes, stream, p);
  }
  return hipGetLastError();
}

}  // namespace mjb
