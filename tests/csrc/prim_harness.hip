// prim_harness.hip -- test-only launchers for the building blocks of the DPP row kernels
// (tests/test_gpu_primitives.py). Built by biped_pympc_amd/build.py build_prim_harness() into
// tests/libprim_harness.so; never linked into the product libraries.
//
// The product headers are included unchanged. Every kernel only loads its operands, calls ONE
// primitive and stores the result: there is no solver logic here. One wavefront per block; thread
// t = 64 * blockIdx.x + lane reads `in + NIN * t` and writes `out + NOUT * t`. The lanes that call
// the primitive are the set bits of `mask` (the same mask in every wave): a runtime, lane-dependent
// branch around the call, which is how the product call sites run their primitives
// (`if (lane < 32) { ... if (act && !(mstep && g == 1)) ... }`). Inactive lanes store nothing.
#define SRBD_NO_GENERAL_KERNEL
#include "pdipm_srbd_reg.hpp"

#ifndef SRBD_PRIM_ID
#define SRBD_PRIM_ID "unset"
#endif

using namespace srbd;

namespace {

__device__ __forceinline__ bool ph_active(unsigned long long mask) { return (mask >> (threadIdx.x & 63)) & 1ull; }
__device__ __forceinline__ size_t ph_tid() { return (size_t)blockIdx.x * 64 + threadIdx.x; }

// ---------------------------------------------------------------- lane movers (16-lane rows) ----
// Active lanes as in the solve chains of pdipm_srbd.hpp:452-478 / pdipm.hpp:815-872 (bc16), in
// RegCtx::factor_chain, pdipm_srbd_reg.hpp:834, :841 (shl6) and in couple_cty2, :281 (shr6): inside
// `if (lane < 32)`, a group under `act` (both 16-lane groups, or one).
__global__ void k_bc16(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double v = in[ph_tid()];
#pragma unroll
    for (int k = 0; k < 12; ++k) out[12 * ph_tid() + k] = bc16(v, k);
  }
}
__global__ void k_shift6(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double v = in[ph_tid()];
    out[2 * ph_tid()] = shl6(v);
    out[2 * ph_tid() + 1] = shr6(v);
  }
}

// ------------------------------------------------------------------- broadcast dot products ----
// dot_bc12: RegCtx::factor_chain, pdipm_srbd_reg.hpp:871-872, and RegCtx::solve_chain, :1134-1139,
// `lane < 32 && act && !(mstep && g == 1)`.
// in: c[12], v
__global__ void k_dot_bc12(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 13 * ph_tid();
    double c[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) c[j] = p[j];
    out[ph_tid()] = dot_bc12(c, p[12]);
  }
}
// dot_bc12_sub: RegCtx::solve_chain's outward substitution, pdipm_srbd_reg.hpp:1155-1160,
// `lane < 32 && te < cnt` (cnt per group). in: c[12], v, init
__global__ void k_dot_bc12_sub(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 14 * ph_tid();
    double c[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) c[j] = p[j];
    out[ph_tid()] = dot_bc12_sub(c, p[12], p[13]);
  }
}
// fmac_rows678_4: RegCtx::factor_chain, pdipm_srbd_reg.hpp:837 (<true>) and :844 (<false>), `lane < 32 && act && prev`.
// in: x[4], v[4], c6, c7, c8
template <bool kNeg>
__global__ void k_rows678(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 11 * ph_tid();
    double x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
    fmac_rows678_4<kNeg>(x0, x1, x2, x3, p[4], p[5], p[6], p[7], p[8], p[9], p[10]);
    double* o = out + 4 * ph_tid();
    o[0] = x0;
    o[1] = x1;
    o[2] = x2;
    o[3] = x3;
  }
}
// v_rows: RegCtx::factor_chain, pdipm_srbd_reg.hpp:831, `lane < 32 && act && prev`. in: Dr[12], d, a0, a1, a2, b
__global__ void k_v_rows(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 17 * ph_tid();
    double Dr[12], V[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) Dr[j] = p[j];
    v_rows(V, Dr, p[12], p[13], p[14], p[15], p[16]);
#pragma unroll
    for (int j = 0; j < 12; ++j) out[12 * ph_tid() + j] = V[j];
  }
}
// couple_cw_sub: RegCtx::fwd_rhs, pdipm_srbd_reg.hpp:625, `lane < 32 && act && prev`. in: d, b, a0, a1, a2, w, base
__global__ void k_couple_cw_sub(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 7 * ph_tid();
    const CoupleRow c{p[0], p[1], p[2], p[3], p[4]};
    out[ph_tid()] = couple_cw_sub(c, p[5], p[6]);
  }
}
// couple_cty2: RegCtx::solve_chain, pdipm_srbd_reg.hpp:1160, `lane < 32 && te < cnt`. in: d, b, a0, a1, a2, y
__global__ void k_couple_cty2(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    const double* p = in + 6 * ph_tid();
    const CoupleRow c{p[0], p[1], p[2], p[3], p[4]};
    out[ph_tid()] = couple_cty2(c, p[5]);
  }
}

// ------------------------------------------------------------------------ wave reductions ----
// All 64 lanes active (srbd_common.hpp wave_reduce; the call sites -- RegCtx::block_reduce,
// pdipm_srbd_reg.hpp:481, the step lengths' wave_min2, :1292, and pdipm_srbd.hpp:142, :658-720 -- are
// wave-uniform). Every lane stores the value it got back.
__global__ void k_wave_sum(const double* in, double* out) { out[ph_tid()] = wave_sum(in[ph_tid()]); }
__global__ void k_wave_min(const double* in, double* out) { out[ph_tid()] = wave_min(in[ph_tid()]); }
__global__ void k_wave_min2(const double* in, double* out) {
  double a = in[2 * ph_tid()], b = in[2 * ph_tid() + 1];
  wave_min2(a, b);
  out[2 * ph_tid()] = a;
  out[2 * ph_tid() + 1] = b;
}

// ----------------------------------------------------------------------------------- rcp3 ----
__global__ void k_rcp3(const double* in, double* out, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = rcp3(in[t]);
}

// ---------------------------------------------------------------------------- 12x12 inverse ----
// inverse_rows12: RegCtx::factor_chain, pdipm_srbd_reg.hpp:860-861, `lane < 32 && act && !(mstep && g == 1)`: both 16-lane
// groups, or group 0 alone. Lanes >= 32 are never active (PivotLanes<K>::value sign-extends): the
// launcher refuses a mask with such a bit. in: Sr[12] (row min(lane & 15, 11) of the block)
template <bool kSwp>
__global__ void k_inverse_rows12(const double* in, double* out, unsigned long long mask) {
  if (ph_active(mask)) {
    double Sr[12], Dr[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) Sr[j] = in[12 * ph_tid() + j];
    inverse_rows12<kSwp>(Sr, Dr);
#pragma unroll
    for (int j = 0; j < 12; ++j) out[12 * ph_tid() + j] = Dr[j];
  }
}

// --------------------------------------------------------------------------- 4x4 foot blocks ----
// One block and right-hand side per thread (the product's per-stage foot task lanes), no lane
// condition beyond the bound. in: a[10] packed lower, v[4]; out: factors[10], x[4].
// Register path: RegCtx::foot_inverse, pdipm_srbd_reg.hpp:664 (ldlt_factor<4, true>), and RegCtx::phi_solve,
// :680 (ldlt_solve<4>).
__global__ void k_ldlt4_reg(const double* in, double* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    double a[10], v[4], x[4];
#pragma unroll
    for (int e = 0; e < 10; ++e) a[e] = in[14 * t + e];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = in[14 * t + 10 + e];
    ldlt_factor<4, true>(a);
    ldlt_solve<4>(a, v, x);
#pragma unroll
    for (int e = 0; e < 10; ++e) out[14 * t + e] = a[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) out[14 * t + 10 + e] = x[e];
  }
}
// Memory path: pdipm_srbd.hpp:174 / pdipm.hpp:514 (ldlt_factor<4>, factors stored to LDS) and
// pdipm_srbd.hpp:192 / pdipm.hpp:543 (ldlt_solve_p<4> reading them back from LDS).
__global__ void k_ldlt4_mem(const double* in, double* out, int n) {
  __shared__ double PH[64 * 10];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    double a[10], v[4], x[4];
#pragma unroll
    for (int e = 0; e < 10; ++e) a[e] = in[14 * t + e];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = in[14 * t + 10 + e];
    ldlt_factor<4>(a);
    double* f = PH + 10 * threadIdx.x;
#pragma unroll
    for (int e = 0; e < 10; ++e) f[e] = a[e];
    lds_wave_sync();
    ldlt_solve_p<4>(f, v, x);
#pragma unroll
    for (int e = 0; e < 10; ++e) out[14 * t + e] = f[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) out[14 * t + 10 + e] = x[e];
  }
}

// ------------------------------------------------------- products over the compact blocks ----
// Operands in memory at in + NIN * t, the row / column index from idx[t] (lane-dependent in the
// product); no lane condition (row-parallel passes over every thread of the QP).
// drow12: RegCtx::nrow, pdipm_srbd_reg.hpp:422. in: row[12], v[12]
__global__ void k_drow12(const double* in, const int* idx, double* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = drow12(in + 24 * t, in + 24 * t + 12);
}
// mrow_slot<t>: RegCtx::arow, pdipm_srbd_reg.hpp:529. in: mc[24], v[12]; idx: r
template <int S>
__global__ void k_mrow_slot(const double* in, const int* idx, double* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = mrow_slot<S>(in + 36 * t, idx[t], in + 36 * t + 24);
}
// mcol: pdipm_srbd_reg.hpp:563, :1191. in: mc[24], v[12]; idx: j
__global__ void k_mcol(const double* in, const int* idx, double* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = mcol(in + 36 * t, idx[t], in + 36 * t + 24);
}
// ncol<kForce>: pdipm_srbd_reg.hpp:586, :985, :1206-1217. in: nd[12 * kNdS], v[12]; idx: col (p = col % 3
// for the force columns, 0 otherwise: the call sites' arguments)
template <bool kForce>
__global__ void k_ncol(const double* in, const int* idx, double* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int S = 12 * kNdS + 12;
  if (t < n) out[t] = ncol<kForce>(in + S * t, idx[t], in + S * t + 12 * kNdS, kForce ? idx[t] % 3 : 0);
}
// grow4: pdipm_srbd_reg.hpp:609, :948, :1238. in: gf[kGfSize], xu[12]; idx: k
__global__ void k_grow4(const double* in, const int* idx, double* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int S = kGfSize + 12;
  if (t < n) out[t] = grow4(in + S * t, idx[t], in + S * t + kGfSize);
}
// cel: in: cc[24]; idx: 12 c + b
__global__ void k_cel(const double* in, const int* idx, double* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = cel(in + 24 * t, idx[t] / 12, idx[t] % 12);
}

// --------------------------------------------------------------------------- integer helpers ----
__global__ void k_div12(int* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = div12(t);
}
__global__ void k_div6(int* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = div6(t);
}
__global__ void k_m24(const int* a, const int* b, int* out, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = m24(a[t], b[t]);
}
// j = 0..11 -> foot_of, foot_pos; (f, a) = (t / 4, t % 4), t = 0..7 -> foot_colj
__global__ void k_foot(int* out) {
  const int t = threadIdx.x;
  if (t < 12) {
    out[t] = foot_of(t);
    out[12 + t] = foot_pos(t);
  }
  if (t < 8) out[24 + t] = foot_colj(t / 4, t % 4);
}

int finish() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return (int)e;
}
int blocks(size_t n, int tpb) { return (int)((n + tpb - 1) / tpb); }

}  // namespace

#define PH_WAVE_LAUNCHER(NAME, KERNEL)                                                              \
  extern "C" int NAME(const double* in, double* out, int nwaves, unsigned long long mask) {         \
    if (nwaves <= 0) return -1;                                                                     \
    hipLaunchKernelGGL(KERNEL, dim3(nwaves), dim3(64), 0, 0, in, out, mask);                        \
    return finish();                                                                                \
  }
#define PH_FULLWAVE_LAUNCHER(NAME, KERNEL)                                   \
  extern "C" int NAME(const double* in, double* out, int nwaves) {           \
    if (nwaves <= 0) return -1;                                              \
    hipLaunchKernelGGL(KERNEL, dim3(nwaves), dim3(64), 0, 0, in, out);       \
    return finish();                                                         \
  }
#define PH_ROW_LAUNCHER(NAME, KERNEL)                                                      \
  extern "C" int NAME(const double* in, const int* idx, double* out, int n) {              \
    if (n <= 0) return -1;                                                                 \
    hipLaunchKernelGGL(KERNEL, dim3(blocks(n, 64)), dim3(64), 0, 0, in, idx, out, n);      \
    return finish();                                                                       \
  }

extern "C" const char* prim_harness_id() { return "srbd-prim-id:" SRBD_PRIM_ID; }

PH_WAVE_LAUNCHER(ph_bc16, k_bc16)
PH_WAVE_LAUNCHER(ph_shift6, k_shift6)
PH_WAVE_LAUNCHER(ph_dot_bc12, k_dot_bc12)
PH_WAVE_LAUNCHER(ph_dot_bc12_sub, k_dot_bc12_sub)
PH_WAVE_LAUNCHER(ph_rows678, k_rows678<false>)
PH_WAVE_LAUNCHER(ph_rows678_neg, k_rows678<true>)
PH_WAVE_LAUNCHER(ph_v_rows, k_v_rows)
PH_WAVE_LAUNCHER(ph_couple_cw_sub, k_couple_cw_sub)
PH_WAVE_LAUNCHER(ph_couple_cty2, k_couple_cty2)
PH_FULLWAVE_LAUNCHER(ph_wave_sum, k_wave_sum)
PH_FULLWAVE_LAUNCHER(ph_wave_min, k_wave_min)
PH_FULLWAVE_LAUNCHER(ph_wave_min2, k_wave_min2)
PH_ROW_LAUNCHER(ph_drow12, k_drow12)
PH_ROW_LAUNCHER(ph_mrow_slot0, k_mrow_slot<0>)
PH_ROW_LAUNCHER(ph_mrow_slot1, k_mrow_slot<1>)
PH_ROW_LAUNCHER(ph_mcol, k_mcol)
PH_ROW_LAUNCHER(ph_ncol_force, k_ncol<true>)
PH_ROW_LAUNCHER(ph_ncol, k_ncol<false>)
PH_ROW_LAUNCHER(ph_grow4, k_grow4)
PH_ROW_LAUNCHER(ph_cel, k_cel)

extern "C" int ph_inverse_rows12(const double* in, double* out, int nwaves, unsigned long long mask, int swp) {
  if (nwaves <= 0 || (mask >> 32) != 0) return -1;  // lanes >= 32 must stay inactive
  if (swp) hipLaunchKernelGGL(k_inverse_rows12<true>, dim3(nwaves), dim3(64), 0, 0, in, out, mask);
  else hipLaunchKernelGGL(k_inverse_rows12<false>, dim3(nwaves), dim3(64), 0, 0, in, out, mask);
  return finish();
}
extern "C" int ph_rcp3(const double* in, double* out, size_t n) {
  if (n == 0) return -1;
  hipLaunchKernelGGL(k_rcp3, dim3(blocks(n, 256)), dim3(256), 0, 0, in, out, n);
  return finish();
}
extern "C" int ph_ldlt4(const double* in, double* out, int n, int mem) {
  if (n <= 0) return -1;
  if (mem) hipLaunchKernelGGL(k_ldlt4_mem, dim3(blocks(n, 64)), dim3(64), 0, 0, in, out, n);
  else hipLaunchKernelGGL(k_ldlt4_reg, dim3(blocks(n, 64)), dim3(64), 0, 0, in, out, n);
  return finish();
}
extern "C" int ph_div12(int* out, int n) {
  if (n <= 0) return -1;
  hipLaunchKernelGGL(k_div12, dim3(blocks(n, 256)), dim3(256), 0, 0, out, n);
  return finish();
}
extern "C" int ph_div6(int* out, int n) {
  if (n <= 0) return -1;
  hipLaunchKernelGGL(k_div6, dim3(blocks(n, 256)), dim3(256), 0, 0, out, n);
  return finish();
}
extern "C" int ph_m24(const int* a, const int* b, int* out, size_t n) {
  if (n == 0) return -1;
  hipLaunchKernelGGL(k_m24, dim3(blocks(n, 256)), dim3(256), 0, 0, a, b, out, n);
  return finish();
}
extern "C" int ph_foot(int* out) {  // out: 32 ints
  hipLaunchKernelGGL(k_foot, dim3(1), dim3(64), 0, 0, out);
  return finish();
}
