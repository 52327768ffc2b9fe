// srbd_backward.hip -- fourth translation unit of libsrbd_mpc.so: the backward pass of the MPC QP
// (pdipm_backward.hpp: adjoint KKT solve + QP-data gradients; qp_former_backward.hpp: the former's
// vector-Jacobian product). The forward kernels' units do not include these kernels, so their code
// does not change with this unit. Launch geometry as in srbd_mpc.hip.
#define SRBD_NO_GENERAL_KERNEL
#include "pdipm_backward.hpp"
#include "qp_former_backward.hpp"

namespace srbd {
namespace bwd {

constexpr int kFormerWaves = 4;

const void* adjoint_kernel() { return (const void*)pdipm_backward_kernel<0>; }

void launch_adjoint(const BackwardArgs& a, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL(pdipm_backward_kernel<0>, dim3(a.batch), dim3(64), lds, s, a);
}

const void* adjoint_multi_kernel() { return (const void*)pdipm_backward_multi_kernel<0>; }

void launch_adjoint_multi(const BackwardMultiArgs& a, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL(pdipm_backward_multi_kernel<0>, dim3(a.batch), dim3(64), lds, s, a);
}

void launch_former_backward(const FormerBackwardArgs& a, hipStream_t s) {
  const int rows = a.batch * a.n_seeds;  // the host entry checks that it fits an int
  const int grid = (rows + kFormerWaves - 1) / kFormerWaves;
  hipLaunchKernelGGL(qp_former_backward_kernel<kFormerWaves>, dim3(grid), dim3(64 * kFormerWaves), 0, s, a);
}

}  // namespace bwd
}  // namespace srbd
