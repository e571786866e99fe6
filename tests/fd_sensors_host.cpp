// Host driver of tests/test_fd_sensors_host.py: the slab arithmetic of mjb_transition_fd_points_sensors (mjb_host.hpp, no HIP), with and
// without the sensor block of the per-point scratch.
#define MJB_HOST_EMU 1
#include <cstring>
#include <string>
#include <vector>

#include "../mujoco_template_amd/csrc/mjb_device.hpp"
#include "../mujoco_template_amd/csrc/mjb_host.hpp"

using namespace mjb;

extern "C" {
unsigned long long fds_point_scratch_bytes3(int nq, int nv, int nu) { return fd_point_scratch_bytes(nq, nv, nu); }
unsigned long long fds_point_scratch_bytes(int nq, int nv, int nu, int nsens) { return fd_point_scratch_bytes(nq, nv, nu, nsens); }
long fds_slab_points(unsigned long long bytes_per_point, unsigned long long budget) { return fd_slab_points(bytes_per_point, budget); }
long fds_slab_count(long npoint, long per_slab) { return fd_slab_count(npoint, per_slab); }
int fds_slab(long npoint, long per_slab, long k, long* p0, long* n) { return fd_slab(npoint, per_slab, k, *p0, *n) ? 1 : 0; }
}
