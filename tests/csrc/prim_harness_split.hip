// prim_harness_split.hip -- test-only launchers for the column-split chain primitives
// (tests/test_gpu_primitives_split.py). Built by biped_pympc_amd/build.py build_prim_harness_split()
// into tests/libprim_harness_split.so; never linked into the product libraries.
//
// Same conventions as prim_harness.hip: the product headers unchanged, every kernel loads its
// operands, calls ONE primitive and stores the result; one wavefront per block, thread
// t = 64 * blockIdx.x + lane reads `in + NIN * t` and writes `out + NOUT * t`; the lanes that call the
// primitive are the set bits of `mask` (a runtime, lane-dependent branch, as at the call sites in
// RegCtx::factor_chain / solve_chain, where `act` is per twisted group). The split
// primitives exchange values between lanes i and i + 32, so a mask must hold both or neither: the
// launchers refuse any other.
#define SRBD_NO_GENERAL_KERNEL
#include "pdipm_srbd_reg.hpp"

#ifndef SRBD_PRIM_ID
#define SRBD_PRIM_ID "unset"
#endif

using namespace srbd;

namespace {

__device__ __forceinline__ bool ph_active(unsigned long long mask) { return (mask >> (threadIdx.x & 63)) & 1ull; }
__device__ __forceinline__ size_t ph_tid() { return (size_t)blockIdx.x * 64 + threadIdx.x; }

// inverse_rows12_split. in: the whole row Sr[12] of the lane's group and row (lanes i and i + 32 hold
// the same row); the lane takes its half's six columns. out: Dr[6]
__global__ void k_inverse_split(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const int h = (threadIdx.x & 63) >> 5;
    double Sr[6], Dr[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) Sr[j] = in[12 * ph_tid() + (j < 3 ? j : j + 3) + 3 * h];
    inverse_rows12_split(Sr, Dr);
#pragma unroll
    for (int j = 0; j < 6; ++j) out[6 * ph_tid() + j] = Dr[j];
  }
}
// v_rows_split. in: Dl[6], d, x0, x1, x2
__global__ void k_v_rows_split(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 10 * ph_tid();
    double Dl[6], V[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) Dl[j] = p[j];
    v_rows_split(V, Dl, SplitCoef{p[6], p[7], p[8], p[9]});
#pragma unroll
    for (int j = 0; j < 6; ++j) out[6 * ph_tid() + j] = V[j];
  }
}
// fmac_rows678_6. in: x[6], v[6], c6, c7, c8
template <bool kNeg>
__global__ void k_rows678_6(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 15 * ph_tid();
    double x[6], v[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      x[j] = p[j];
      v[j] = p[6 + j];
    }
    fmac_rows678_6<kNeg>(x, v, p[12], p[13], p[14]);
#pragma unroll
    for (int j = 0; j < 6; ++j) out[6 * ph_tid() + j] = x[j];
  }
}
// dot_bc12_split. in: c[6], v
__global__ void k_dot_split(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 7 * ph_tid();
    double c[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) c[j] = p[j];
    out[ph_tid()] = dot_bc12_split(c, p[6]);
  }
}
// dot_bc12_sub_split. in: c[6], v, init
__global__ void k_dot_sub_split(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 8 * ph_tid();
    double c[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) c[j] = p[j];
    out[ph_tid()] = dot_bc12_sub_split(c, p[6], p[7], (threadIdx.x & 32) != 0);
  }
}

int finish() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return (int)e;
}

}  // namespace

#define PHS_LAUNCHER(NAME, KERNEL)                                                                  \
  extern "C" int NAME(const double* in, double* out, int nwaves, unsigned long long mask) {         \
    if (nwaves <= 0 || ((mask >> 32) ^ (mask & 0xFFFFFFFFull)) != 0) return -1;                     \
    hipLaunchKernelGGL(KERNEL, dim3(nwaves), dim3(64), 0, 0, in, out, mask);                        \
    return finish();                                                                                \
  }

extern "C" const char* prim_harness_split_id() { return "srbd-prim-id:" SRBD_PRIM_ID; }

PHS_LAUNCHER(phs_inverse, k_inverse_split)
PHS_LAUNCHER(phs_v_rows, k_v_rows_split)
PHS_LAUNCHER(phs_rows678, k_rows678_6<false>)
PHS_LAUNCHER(phs_rows678_neg, k_rows678_6<true>)
PHS_LAUNCHER(phs_dot, k_dot_split)
PHS_LAUNCHER(phs_dot_sub, k_dot_sub_split)
