// The kernels of mjb_lqr_dlyap (mjb_dlyap.hpp) and their launch.  One workgroup per problem.
#include "mjb_dlyap.hpp"

namespace mjb {

extern __shared__ double dlyap_lds[];

template <int NW> __global__ __launch_bounds__(64 * NW) void k_lqr_dlyap(DlyapArgs p) {
  dlyap_env<NW>(p, (int)blockIdx.x, (int)threadIdx.x, dlyap_lds);
}

// Dynamic LDS above the default limit is allowed once per kernel variant and device, for the 160 KB the LQR launches request
// (the layout is checked against it before a launch).
static const size_t kDlyapLdsMax = 160 * 1024;
template <auto kern> static hipError_t dlyap_lds_limit(size_t bytes) {
  static bool done[64] = {};
  if (bytes > kDlyapLdsMax) return hipErrorInvalidValue;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
  e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDlyapLdsMax);
  if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
  return e;
}

hipError_t dlyap_launch(const DlyapArgs& p, hipStream_t stream) {
  const size_t bytes = (size_t)dlyap_layout(p.nx, p.nu).total * sizeof(double);
  hipError_t e;
  if (lqr_waves(p.nx) == 1) {
    if ((e = dlyap_lds_limit<k_lqr_dlyap<1>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_dlyap<1>), dim3((unsigned)p.B), dim3(64), bytes, stream, p);
  } else {
    if ((e = dlyap_lds_limit<k_lqr_dlyap<4>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_dlyap<4>), dim3((unsigned)p.B), dim3(256), bytes, stream, p);
  }
  return hipGetLastError();
}

}  // namespace mjb
