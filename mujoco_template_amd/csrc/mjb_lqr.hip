// The kernels of mjb_lqr_backward / mjb_lqr_backward_box / mjb_lqr_candidates (mjb_lqr.hpp) and their launches.  One workgroup per trajectory.
#include "mjb_lqr.hpp"

namespace mjb {

extern __shared__ double lqr_lds[];

template <int NW, int MU> __global__ __launch_bounds__(64 * NW) void k_lqr_backward(LqrBackwardArgs p) {
  lqr_backward_env<NW, MU>(p, (int)blockIdx.x, (int)threadIdx.x, lqr_lds);
}
template <int NW, int MU> __global__ __launch_bounds__(64 * NW) void k_lqr_backward_box(LqrBoxArgs p) {
  lqr_backward_box_env<NW, MU>(p, (int)blockIdx.x, (int)threadIdx.x, lqr_lds);
}
__global__ __launch_bounds__(256) void k_lqr_candidates(LqrCandArgs p) {
  lqr_candidates_env<256>(p, (int)blockIdx.x, (int)threadIdx.x, lqr_lds);
}
template <int NW> __global__ __launch_bounds__(64 * NW) void k_lqr_gemm_probe(int M, int N, int K, const double* a, const double* b, double* c) {
  lqr_gemm_probe<NW>(M, N, K, a, b, c, (int)threadIdx.x);
}

// Dynamic LDS above the default limit has to be allowed per kernel: done ONCE per kernel variant and device, for the whole 160 KB of a
// CU (every layout is checked against it before a launch), not on every launch.
static const size_t kLqrLdsMax = 160 * 1024;
template <auto kern> static hipError_t lqr_lds_limit(size_t bytes) {             // one instantiation, one flag set, per kernel variant
  static bool done[64] = {};
  if (bytes > kLqrLdsMax) return hipErrorInvalidValue;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
  e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLqrLdsMax);
  if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
  return e;
}

hipError_t lqr_launch_backward(const LqrBackwardArgs& p, hipStream_t stream) {
  const size_t bytes = (size_t)lqr_layout(p.nx, p.nu).total * sizeof(double);
  hipError_t e;
  if (lqr_waves(p.nx) == 1 && p.nu <= 8) {                       // small systems: short substitutions, many workgroups per CU
    if ((e = lqr_lds_limit<k_lqr_backward<1, 8>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_backward<1, 8>), dim3((unsigned)p.B), dim3(64), bytes, stream, p);
  } else if (lqr_waves(p.nx) == 1) {
    if ((e = lqr_lds_limit<k_lqr_backward<1, kLqrMaxNu>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_backward<1, kLqrMaxNu>), dim3((unsigned)p.B), dim3(64), bytes, stream, p);
  } else {
    if ((e = lqr_lds_limit<k_lqr_backward<4, kLqrMaxNu>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_backward<4, kLqrMaxNu>), dim3((unsigned)p.B), dim3(256), bytes, stream, p);
  }
  return hipGetLastError();
}

hipError_t lqr_launch_backward_box(const LqrBoxArgs& p, hipStream_t stream) {      // the dispatch of lqr_launch_backward
  const int nx = p.b.nx, nu = p.b.nu;
  const size_t bytes = (size_t)lqr_box_layout(nx, nu).total * sizeof(double);
  const unsigned B = (unsigned)p.b.B;
  hipError_t e;
  if (lqr_waves(nx) == 1 && nu <= 8) {
    if ((e = lqr_lds_limit<k_lqr_backward_box<1, 8>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_backward_box<1, 8>), dim3(B), dim3(64), bytes, stream, p);
  } else if (lqr_waves(nx) == 1) {
    if ((e = lqr_lds_limit<k_lqr_backward_box<1, kLqrMaxNu>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_backward_box<1, kLqrMaxNu>), dim3(B), dim3(64), bytes, stream, p);
  } else {
    if ((e = lqr_lds_limit<k_lqr_backward_box<4, kLqrMaxNu>>(bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_lqr_backward_box<4, kLqrMaxNu>), dim3(B), dim3(256), bytes, stream, p);
  }
  return hipGetLastError();
}

hipError_t lqr_launch_candidates(const LqrCandArgs& p, hipStream_t stream) {
  const size_t bytes = (size_t)lqr_cand_layout(p.nx, p.nu, p.nalpha).total * sizeof(double);
  hipError_t e = lqr_lds_limit<k_lqr_candidates>(bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_lqr_candidates, dim3((unsigned)p.B), dim3(256), bytes, stream, p);
  return hipGetLastError();
}

hipError_t lqr_launch_gemm_probe(int M, int N, int K, const double* a, const double* b, double* c, hipStream_t stream) {
  if (M <= 16) hipLaunchKernelGGL(k_lqr_gemm_probe<1>, dim3(1), dim3(64), 0, stream, M, N, K, a, b, c);
  else hipLaunchKernelGGL(k_lqr_gemm_probe<4>, dim3(1), dim3(256), 0, stream, M, N, K, a, b, c);
  return hipGetLastError();
}

}  // namespace mjb
