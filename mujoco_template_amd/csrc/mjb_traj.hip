// The kernels of mjb_traj_cost / mjb_traj_select (mjb_traj.hpp) and their launches.
#include "mjb_traj.hpp"

namespace mjb {

extern __shared__ double traj_lds[];

// one wavefront per workgroup, tiles of points drawn grid-stride
__global__ __launch_bounds__(64) void k_traj_cost(TrajCostArgs p, long ntile) {
  for (long tile = blockIdx.x; tile < ntile; tile += gridDim.x) traj_cost_tile(p, tile, (int)threadIdx.x, traj_lds);
}
__global__ __launch_bounds__(64) void k_traj_cost_sum(TrajCostArgs p) {
  for (long e = blockIdx.x; e < p.B; e += gridDim.x) traj_cost_sum(p, e, (int)threadIdx.x, traj_lds);
}
__global__ __launch_bounds__(kTrajSelThreads) void k_traj_select(TrajSelectArgs p, long chunks) {
  for (long b = blockIdx.x; b < p.nprob * chunks; b += gridDim.x) traj_select_block(p, b / chunks, b % chunks, (int)threadIdx.x, traj_lds);
}

static const long kTrajMaxGrid = 1L << 16;             // workgroups of one launch; beyond it a workgroup takes several tiles

hipError_t traj_launch_cost(const TrajCostArgs& p, hipStream_t stream) {
  const long ntile = traj_cost_tiles(p.T, p.B);
  const size_t bytes = (size_t)traj_cost_lds(p.nv, p.nu) * sizeof(double);            // at most 8 * (128 + 64 + 64) * 8 = 16 KiB
  hipLaunchKernelGGL(k_traj_cost, dim3((unsigned)(ntile < kTrajMaxGrid ? ntile : kTrajMaxGrid)), dim3(64), bytes, stream, p, ntile);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_traj_cost_sum, dim3((unsigned)(p.B < kTrajMaxGrid ? p.B : kTrajMaxGrid)), dim3(64), 64 * sizeof(double), stream, p);
  return hipGetLastError();
}

hipError_t traj_launch_select(const TrajSelectArgs& p, hipStream_t stream) {
  const long chunks = traj_select_chunks(p.T, p.nu), total = p.nprob * chunks;                  // <= 2^30 * 2^18
  hipLaunchKernelGGL(k_traj_select, dim3((unsigned)(total < kTrajMaxGrid ? total : kTrajMaxGrid)), dim3(kTrajSelThreads),
                     (size_t)traj_select_lds() * sizeof(double), stream, p, chunks);
  return hipGetLastError();
}

}  // namespace mjb
