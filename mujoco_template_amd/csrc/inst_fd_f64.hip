// finite-difference linearisation columns: float64 arithmetic over a float64 state.
#include "mjb_kernels.hpp"
namespace mjb {
template <>
hipError_t launch_fd<double, double>(int G, const DevModel<double>* m, const Lay* Ldev, const Lay& L, const DevData<double>& d, const FdPoints& pt, int ncol, int nv, int nu, int chunk, double eps, double* y, int* valid, hipStream_t stream) {
  MJB_DISPATCH_G(G, return (launch_fd_g<double, double, GG>(m, Ldev, L, d, pt, ncol, nv, nu, chunk, eps, y, valid, stream)));
  return hipErrorInvalidValue;
}
template <>
hipError_t launch_jac<double, double>(int G, const DevModel<double>* m, const Lay* Ldev, const Lay& L, const DevData<double>& d, int nreq, const int* kinds, const int* ids, double* out_p, double* out_r, hipStream_t stream) {
  MJB_DISPATCH_G(G, return (launch_jac_g<double, double, GG>(m, Ldev, L, d, nreq, kinds, ids, out_p, out_r, stream)));
  return hipErrorInvalidValue;
}
}  // namespace mjb
