// srbd_backward.hip -- fourth translation unit of libsrbd_mpc.so: the backward pass of the MPC QP
// (pdipm_backward.hpp: adjoint KKT solve + QP-data gradients; qp_former_backward.hpp: the former's
// vector-Jacobian product; mpc_io_backward.hpp: the VJPs of the controller step's FP32 input preparation and
// wrench / torque epilogue). The forward kernels' units do not include these kernels, so their code
// does not change with this unit. Launch geometry as in srbd_mpc.hip.
#define SRBD_NO_GENERAL_KERNEL
#include "pdipm_backward.hpp"
#include "qp_former_backward.hpp"
#include "mpc_io_backward.hpp"

namespace srbd {
namespace bwd {

constexpr int kFormerWaves = 4;

const void* adjoint_kernel(bool full) {
  return full ? (const void*)pdipm_backward_kernel<0, true> : (const void*)pdipm_backward_kernel<0, false>;
}

const void* adjoint_multi_kernel(bool full) {
  return full ? (const void*)pdipm_backward_multi_kernel<0, true> : (const void*)pdipm_backward_multi_kernel<0, false>;
}

void launch_former_backward(const FormerBackwardArgs& a, hipStream_t s) {
  const int rows = a.batch * a.n_seeds;  // the host entry checks that it fits an int
  const int grid = (rows + kFormerWaves - 1) / kFormerWaves;
  hipLaunchKernelGGL(qp_former_backward_kernel<kFormerWaves>, dim3(grid), dim3(64 * kFormerWaves), 0, s, a);
}

void launch_prepare_backward(const PrepArgs& prep, const double* const* g, const float* gwpd, const float* gyaw,
                             const double* gR, float* const* out, hipStream_t s) {
  PrepBackwardArgs a{};
  a.prep = prep;
  for (int i = 0; i < 17; ++i) a.g[i] = g ? g[i] : nullptr;
  a.gwpd = gwpd;
  a.gyaw = gyaw;
  a.gR = gR;
  for (int i = 0; i < SRBD_PREP_GRAD_COUNT; ++i) a.out[i] = out[i];
  hipLaunchKernelGGL(prepare_inputs_backward_kernel, dim3((prep.batch + 3) / 4), dim3(256), 0, s, a);
}

void launch_wrench_backward(int N, int batch, const double* x, const float* rotation_body, const float* grad_wrench,
                            int ndof, const float* J, const float* contact, const float* grad_tau, double* grad_x,
                            double* grad_R, hipStream_t s) {
  hipLaunchKernelGGL(u0_wrench_backward_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, N, batch, x,
                     rotation_body, grad_wrench, ndof, J, contact, grad_tau, grad_x, grad_R);
}

void launch_widen(int n, const float* src, double* dst, hipStream_t s) {
  hipLaunchKernelGGL(widen_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, src, dst);
}

}  // namespace bwd
}  // namespace srbd
