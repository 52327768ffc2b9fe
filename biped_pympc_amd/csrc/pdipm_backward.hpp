// pdipm_backward.hpp -- the backward pass of the MPC QP: the adjoint KKT solve of a stage-invariant
// SRBD QP at a given iterate and the gradients of a loss with respect to the QP data.
//
// The iterate (x, s, z, y) is read as a root of the solver's regularised KKT residual F (SURVEY.md
// Appendix A.2.2; the linear systems of sparse_pdipm_solver.py:412-439). Its Newton matrix
//   K = [[H + bI, 0, G^T, A^T], [0, W, I, 0], [G, I, -dI, 0], [A, 0, 0, -dI]],  W = z / s + d
// is symmetric, so the adjoint of a loss L with g = dL/dx is the solution of the SAME matrix,
//   K [lx; ls; lz; ly] = [g; 0; 0; 0],
// and the gradient with respect to a datum theta is -lambda^T dF/dtheta. In the reduced form the
// forward kernel eliminates to (pdipm.hpp), with Lam = W / (1 + dW):
//   (H + bI + G^T Lam G) lx + A^T ly = g,  A lx - d ly = 0,  lz = Lam G lx,  ls = -G lx + d lz.
// That is FastCtx's direction solve with RX = -g and RS = RE = R2 = 0 (pdipm_srbd.hpp): one factor(),
// one solve (mode 3: the right-hand sides are taken as given) and one step of refinement against the
// full K, exactly as the forward kernel refines its directions. At a non-converged iterate the result
// is the exact derivative of the linearised KKT conditions at that iterate (as in qpth).
//
// Seeds on the other outputs. A loss may also depend on s, z, y and on the QP objective
// J = 1/2 x^T H x + f^T x (H without the regularisation). With cotangents g_x, g_s, g_z, g_y, g_J the
// same matrix is solved for the full right-hand side,
//   K [lx; ls; lz; ly] = [g~; g_s; g_z; g_y],   g~ = g_x + g_J (H o x + f),
// in reduced form, with v = D^-1 (g_s - W g_z), D = 1 + dW:
//   (H + bI + G^T Lam G) lx + A^T ly = g~ - G^T v,  A lx - d ly = g_y,  lz = v + Lam G lx,
//   ls = g_z - G lx + d lz.
// By the residual definitions e1..e4 of FastCtx::refine_rhs that is RX = -g~, R2 = g_s, RS = -g_z,
// RE = -g_y and VV = DI (R2 + WD RS), formed after factor() (WD, DI are its results); solve(3),
// refine_rhs() and solve(2) are unchanged. The six formulas below are unchanged too (ls enters none);
// J's explicit dependence on H and f adds g_J (1/2 x[c] x[c]) to grad_H[c] and g_J x[c] to grad_f[c].
// A null cotangent is zero: with only g_x given the kernels run the statements, and give the bits, of the
// x-only form above. Each kernel has two instantiations: FULL = false takes g_x alone, with the other
// cotangents compiled out (carrying their pointers and g_J across the solve costs the x-only path 3-4 %
// in scalar-register spills); the host launches FULL = true when any other cotangent is given.
//
// Gradients, one value per CCS nonzero (every nonzero is its own parameter: nothing is summed over
// stages), in qp_former's output order and widths:
//   grad_H[c]     = -lx[c] x[c]                           (24N, H's pattern is its diagonal)
//   grad_f        = -lx                                   (24N)
//   grad_A[(r,c)] = -(lx[c] y[r] + ly[r] x[c])            (122N - 24)
//   grad_b        = ly                                    (14N)
//   grad_G[(r,c)] = -(lx[c] z[r] + lz[r] x[c])            (28N)
//   grad_d        = lz                                    (16N)
// Products and sums of the epilogue are never contracted and run in a fixed order per entry, so an
// env's gradients do not depend on the batch size or on the env's position in the batch.
//
// Mapping (gfx950): one 64-lane workgroup per QP, stage matrices, iterate and factors in LDS
// (FastLayout plus the refinement's saved lx / ly), any horizon 1..32. A QP that is not
// stage-invariant (the forward kernel's bitwise check) is not solved: its gradients are NaN and its
// status word is kStatusUnsupported.
#pragma once
#include <hip/hip_runtime.h>

#include "pdipm_srbd.hpp"

namespace srbd {

constexpr int kStatusUnsupported = 8;  // include/srbd_mpc.h SRBD_STATUS_UNSUPPORTED

// the cotangents of one solve's outputs, one row per seed; a null array is a zero cotangent
struct BackwardSeeds {
  const double *grad_x, *grad_s, *grad_z, *grad_y;  // rows of 24N, 16N, 16N, 14N
  const double* grad_objective;                     // one double per row
};

// the other cotangents, at the end of the kernels' argument structs: the x-only instantiations never load them
struct BackwardMoreSeeds {
  const double *grad_s, *grad_z, *grad_y, *grad_objective;
};

// the seeds a kernel instantiation takes: all five (FULL), or grad_x alone with the rest null at compile time
template <bool FULL>
__device__ __forceinline__ BackwardSeeds seeds_taken(const double* grad_x, const BackwardMoreSeeds& more) {
  if (FULL) return BackwardSeeds{grad_x, more.grad_s, more.grad_z, more.grad_y, more.grad_objective};
  return BackwardSeeds{grad_x, nullptr, nullptr, nullptr, nullptr};
}

struct BackwardArgs {
  const double* in[10];  // srbd_pdipm's inputs: Q_val, G_val, A_val, (f: with grad_objective; h, b: not read), x, s, z, y
  const double* grad_x;  // (B, 24N) dL/dx, or null (FULL)
  double* out[6];        // grad_H, grad_f, grad_A, grad_b, grad_G, grad_d; null: not written
  int* status;           // (B) or null
  int N;
  int batch;
  BackwardMoreSeeds more;  // rows of 16N, 16N, 14N and 1 per env
};

// FastLayout and, behind it, the saved lx / ly of the refinement step (the forward kernels park them
// in their x / y output rows; here they stay on chip)
struct BackwardLayout {
  FastLayout base;
  int XS, YS, total;
  __host__ __device__ explicit BackwardLayout(int N) : base(N) {
    XS = base.total;
    YS = XS + 24 * N;
    total = YS + 14 * N;
  }
};

__host__ __device__ inline size_t backward_lds_bytes(int N) { return sizeof(double) * (size_t)BackwardLayout(N).total; }

// (row, column) of value e of A_val / G_val (the inverse of the offset maps a_xblock / a_pidx /
// a_ublock and the per-stage G tables)
__device__ inline void a_entry_rc(int e, int N, int& r, int& c) {
  if (e < 36 * (N - 1)) {
    const int k = e / 36 + 1, o = e % 36, j = c_tab.xb_j[o], rr = c_tab.xb_r[o];
    c = 12 * (k - 1) + j;
    r = rr < 0 ? 12 * (k - 1) + j : 12 * k + rr;
  } else if (e < a_ubase(N)) {
    r = c = 12 * (N - 1) + (e - 36 * (N - 1));
  } else {
    const int i = (e - a_ubase(N)) / 86, q = (e - a_ubase(N)) % 86, j = c_tab.ub_j[q], rr = c_tab.ub_r[q];
    c = 12 * N + 12 * i + j;
    r = rr >= 12 ? 12 * N + 2 * i + (rr - 12) : 12 * i + rr;
  }
}

// -(lc * dr + lr * xc): a matrix nonzero's gradient from the two KKT rows it appears in
__device__ __forceinline__ double grad_entry(double lc, double dr, double lr, double xc) {
#pragma clang fp contract(off)
  const double a = lc * dr, b = lr * xc;
  return -(a + b);
}
__device__ __forceinline__ double grad_diag(double lc, double xc) {
#pragma clang fp contract(off)
  return -(lc * xc);
}

// the objective's direct terms: g_J d(1/2 x^T H x)/dH[c] and g_J d(f^T x)/df[c] added to the adjoint's
__device__ __forceinline__ double add_objective_H(double base, double gJ, double xc) {
#pragma clang fp contract(off)
  const double h = 0.5 * xc, q = h * xc, t = gJ * q;
  return base + t;
}
__device__ __forceinline__ double add_objective_f(double base, double gJ, double xc) {
#pragma clang fp contract(off)
  const double t = gJ * xc;
  return base + t;
}
// VV = DI (R2 + WD RS), solve(3)'s D^-1 (r2 + W r_s)
__device__ __forceinline__ double seed_vv(double di, double wd, double r2, double rs) {
#pragma clang fp contract(off)
  const double t = wd * rs, u = r2 + t;
  return di * u;
}

// Seed row `row`'s right-hand side in FastCtx's residual convention: RX = -(g_x + g_J (H o x + f)),
// R2 = g_s, RS = -g_z, RE = -g_y. VV = 0 here; seeded_vv() forms it once factor() has run. fg: this
// env's f, read only with grad_objective. X and Hu must be in place.
template <int NT>
__device__ __forceinline__ void seed_rhs(FastCtx<NT>& C, const BackwardSeeds& sd, size_t row, const double* fg,
                                         int N) {
#pragma clang fp contract(off)
  const int nz = 24 * N, m = 16 * N, p = 14 * N, lane = C.lane;
  const double* gx = sd.grad_x ? sd.grad_x + row * nz : nullptr;
  const double* gs = sd.grad_s ? sd.grad_s + row * m : nullptr;
  const double* gz = sd.grad_z ? sd.grad_z + row * m : nullptr;
  const double* gy = sd.grad_y ? sd.grad_y + row * p : nullptr;
  const bool hasJ = sd.grad_objective != nullptr;
  const double gJ = hasJ ? sd.grad_objective[row] : 0.0;
  for (int e = lane; e < nz; e += 64) {
    double g = gx ? gx[e] : 0.0;
    if (hasJ) {
      const double hx = C.Hu[(e < 12 * N ? 12 : 0) + e % 12] * C.X[e];  // Hu: [H_u | H_x]
      const double dj = hx + fg[e], t = gJ * dj;
      g = g + t;
    }
    C.RX[e] = -g;
  }
  for (int e = lane; e < m; e += 64) {
    C.RS[e] = gz ? 0.0 - gz[e] : 0.0;
    C.R2[e] = gs ? gs[e] : 0.0;
    C.VV[e] = 0.0;
  }
  for (int e = lane; e < p; e += 64) C.RE[e] = gy ? 0.0 - gy[e] : 0.0;
}

// after factor(): entry q's R2 and RS were written by this lane (seed_rhs strides alike), and solve()
// synchronises before it reads VV
template <int NT>
__device__ __forceinline__ void seeded_vv(FastCtx<NT>& C, const BackwardSeeds& sd, int N) {
  if (!sd.grad_s && !sd.grad_z) return;  // VV stays 0
  for (int q = C.lane; q < 16 * N; q += 64) C.VV[q] = seed_vv(C.DI[q], C.WD[q], C.R2[q], C.RS[q]);
}

template <int NT, bool FULL>  // NT as FastCtx: 0 = horizon at run time (the only one instantiated, srbd_backward.hip)
__global__ __launch_bounds__(64) void pdipm_backward_kernel(BackwardArgs args) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int env = xcd_item(blockIdx.x, gridDim.x);
  if (env >= args.batch) return;
  const int N = NT > 0 ? NT : args.N, lane = threadIdx.x;
  const BackwardLayout Lo(N);
  FastCtx<NT> C;
  C.N_ = N;
  C.lane = lane;
  C.bind(smem, Lo.base);
  C.fg = C.hg = C.bg = nullptr;  // residuals() is never called: f, h, b are not read
  C.xsg = smem + Lo.XS;
  C.ysg = smem + Lo.YS;
  const int nz = 24 * N, m = 16 * N, p = 14 * N, nA = nnz_A(N), nG = 28 * N;
  const double* Hg = args.in[0] + (size_t)env * nz;
  const double* Gg = args.in[1] + (size_t)env * nG;
  const double* Ag = args.in[2] + (size_t)env * nA;
  double* oH = args.out[0] ? args.out[0] + (size_t)env * nz : nullptr;
  double* of = args.out[1] ? args.out[1] + (size_t)env * nz : nullptr;
  double* oA = args.out[2] ? args.out[2] + (size_t)env * nA : nullptr;
  double* ob = args.out[3] ? args.out[3] + (size_t)env * p : nullptr;
  double* oG = args.out[4] ? args.out[4] + (size_t)env * nG : nullptr;
  double* od = args.out[5] ? args.out[5] + (size_t)env * m : nullptr;

  // ---- compact load and the stage-invariance check, as pdipm_srbd_kernel ----
  for (int e = lane; e < 144; e += 64) {
    const int r = e / 12, j = e % 12;
    const int om = c_tab.Mi[r][j], on = c_tab.Ni[r][j];
    C.Md[e] = (N >= 2 && om >= 0) ? Ag[a_xblock(1) + om] : 0.0;
    C.Nd[e] = on >= 0 ? Ag[a_ublock(N, 0) + on] : 0.0;
  }
  for (int e = lane; e < 192; e += 64) C.Gd[e] = 0.0;
  if (lane < 12) {
    C.Pd[lane] = Ag[a_pidx(c_tab, N, 0, lane)];
    C.Hu[lane] = Hg[12 * N + lane];
    C.Hu[12 + lane] = Hg[lane];
  }
  __syncthreads();
  if (lane < 28) C.Gd[c_tab.grow[lane] * 12 + c_tab.gcol[lane]] = Gg[lane];
  bool bad = false;
  for (int e = lane; e < nA; e += 64) {
    int ref;
    if (e < 36 * (N - 1)) ref = e % 36;
    else if (e < a_ubase(N)) ref = a_pidx(c_tab, N, 0, e - 36 * (N - 1));
    else ref = a_ubase(N) + (e - a_ubase(N)) % 86;
    bad |= !(Ag[e] == Ag[ref]);
  }
  for (int e = lane; e < nG; e += 64) bad |= !(Gg[e] == Gg[e % 28]);
  for (int e = lane; e < nz; e += 64) bad |= !(Hg[e] == Hg[(e < 12 * N ? 0 : 12 * N) + e % 12]);
  if (__any(bad)) {  // the general-algorithm backward does not exist: no solve, NaN gradients
    const double qnan = __builtin_nan("");
    if (oH) for (int e = lane; e < nz; e += 64) oH[e] = qnan;
    if (of) for (int e = lane; e < nz; e += 64) of[e] = qnan;
    if (oA) for (int e = lane; e < nA; e += 64) oA[e] = qnan;
    if (ob) for (int e = lane; e < p; e += 64) ob[e] = qnan;
    if (oG) for (int e = lane; e < nG; e += 64) oG[e] = qnan;
    if (od) for (int e = lane; e < m; e += 64) od[e] = qnan;
    if (args.status && lane == 0) args.status[env] = kStatusUnsupported;
    return;
  }
  C.constants(Ag[a_ubase(N) + c_tab.e6], Ag[a_ubase(N) + c_tab.e9]);

  // ---- the iterate and the adjoint right-hand side [g~; g_s; g_z; g_y] ----
  const BackwardSeeds sd = seeds_taken<FULL>(args.grad_x, args.more);
  const bool hasJ = sd.grad_objective != nullptr;
  const double gJ = hasJ ? sd.grad_objective[env] : 0.0;
  {
    const double* xg = args.in[6] + (size_t)env * nz;
    const double* sg = args.in[7] + (size_t)env * m;
    const double* zg = args.in[8] + (size_t)env * m;
    const double* yg = args.in[9] + (size_t)env * p;
    if (FULL) {
      for (int e = lane; e < nz; e += 64) C.X[e] = xg[e];
      for (int e = lane; e < m; e += 64) {
        C.S[e] = sg[e];
        C.Z[e] = zg[e];
      }
      for (int e = lane; e < p; e += 64) C.Y[e] = yg[e];
      // seed_rhs reads X[e] on the lane that wrote it, and Hu (synchronised by constants())
      seed_rhs(C, sd, (size_t)env, hasJ ? args.in[3] + (size_t)env * nz : nullptr, N);
    } else {  // [g; 0; 0; 0]: seed_rhs's values, loaded in the iterate's loops
      const double* gg = sd.grad_x + (size_t)env * nz;
      for (int e = lane; e < nz; e += 64) {
        C.X[e] = xg[e];
        C.RX[e] = -gg[e];
      }
      for (int e = lane; e < m; e += 64) {
        C.S[e] = sg[e];
        C.Z[e] = zg[e];
        C.RS[e] = 0.0;
        C.R2[e] = 0.0;
        C.VV[e] = 0.0;
      }
      for (int e = lane; e < p; e += 64) {
        C.Y[e] = yg[e];
        C.RE[e] = 0.0;
      }
    }
  }
  __syncthreads();

  // ---- one factorisation, one solve, one refinement step against the full K ----
  C.factor();
  seeded_vv(C, sd, N);
  C.solve(3, 0.0);
  C.refine_rhs();
  C.solve(2, 0.0);
  // lx = TV, ls = DS, lz = DZ, ly = saved + correction
  double* LY = C.ysg;
  for (int e = lane; e < p; e += 64) LY[e] = LY[e] + C.DY[e];
  __syncthreads();

  // ---- gradients ----
  const double *lx = C.TV, *lz = C.DZ;
  bool nf = false;
  for (int e = lane; e < nz; e += 64) {
    nf = nf || not_finite(lx[e]);
    if (oH) oH[e] = hasJ ? add_objective_H(grad_diag(lx[e], C.X[e]), gJ, C.X[e]) : grad_diag(lx[e], C.X[e]);
    if (of) of[e] = hasJ ? add_objective_f(-lx[e], gJ, C.X[e]) : -lx[e];
  }
  if (oA)
    for (int e = lane; e < nA; e += 64) {
      int r, c;
      a_entry_rc(e, N, r, c);
      oA[e] = grad_entry(lx[c], C.Y[r], LY[r], C.X[c]);
    }
  for (int e = lane; e < p; e += 64) {
    nf = nf || not_finite(LY[e]);
    if (ob) ob[e] = LY[e];
  }
  if (oG)
    for (int e = lane; e < nG; e += 64) {
      const int i = e / 28, q = e % 28;
      const int r = 16 * i + c_tab.grow[q], c = 12 * N + 12 * i + c_tab.gcol[q];
      oG[e] = grad_entry(lx[c], C.Z[r], lz[r], C.X[c]);
    }
  for (int e = lane; e < m; e += 64) {
    nf = nf || not_finite(lz[e]);
    if (od) od[e] = lz[e];
  }
  if (args.status) {
    const bool any_nf = __any(nf);
    if (lane == 0) args.status[env] = any_nf ? kStatusNonFinite : 0;
  }
}

// ---- several seeds at one iterate ----
// K depends on the QP and the iterate only, so M seeds g_0 .. g_{M-1} at the same iterate share the
// compact load, the stage-invariance check, constants() and factor(); only the solve, the refinement
// step and the gradient epilogue run per seed. factor()'s results (WD, DI, PH, DV) are read-only to
// solve() and refine_rhs() -- the forward kernel already runs two solves and two refinement solves per
// factorisation -- so seed k's outputs have the bits pdipm_backward_kernel<0> gives for g_k alone.
// Seed k of env e is seed row e * M + k of every given cotangent array, or row k with `shared`: one
// block of M rows for all envs (unit seeds: a Jacobian's rows) in place of (B, M, width) tensors.
// Output o's row of (env e, seed k) is e * M + k. A QP that is not stage-invariant gets NaN in its M
// rows; kStatusNonFinite reports a non-finite adjoint of any of the M seeds.
struct BackwardMultiArgs {
  const double* in[10];  // as BackwardArgs
  const double* grad_x;  // seed rows of 24N, addressed as above, or null (FULL)
  size_t shared;         // 1: M seed rows for all envs; 0: B * M
  double* out[6];        // (B, M, width) each; null: not written
  int* status;           // (B) or null
  int N;
  int batch;
  int n_seeds;           // M >= 1
  BackwardMoreSeeds more;  // seed rows of 16N, 16N, 14N and 1, addressed alike
};

template <int NT, bool FULL>  // NT = 0: horizon at run time (the only one instantiated, srbd_backward.hip)
__global__ __launch_bounds__(64) void pdipm_backward_multi_kernel(BackwardMultiArgs args) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int env = xcd_item(blockIdx.x, gridDim.x);
  if (env >= args.batch) return;
  const int N = NT > 0 ? NT : args.N, lane = threadIdx.x, M = args.n_seeds;
  const BackwardLayout Lo(N);
  FastCtx<NT> C;
  C.N_ = N;
  C.lane = lane;
  C.bind(smem, Lo.base);
  C.fg = C.hg = C.bg = nullptr;  // residuals() is never called: f, h, b are not read
  C.xsg = smem + Lo.XS;
  C.ysg = smem + Lo.YS;
  const int nz = 24 * N, m = 16 * N, p = 14 * N, nA = nnz_A(N), nG = 28 * N;
  const int width[6] = {nz, nz, nA, p, nG, m};
  const double* Hg = args.in[0] + (size_t)env * nz;
  const double* Gg = args.in[1] + (size_t)env * nG;
  const double* Ag = args.in[2] + (size_t)env * nA;
  const size_t row0 = (size_t)env * (size_t)M;  // this env's first output row

  // ---- compact load and the stage-invariance check, as pdipm_backward_kernel ----
  for (int e = lane; e < 144; e += 64) {
    const int r = e / 12, j = e % 12;
    const int om = c_tab.Mi[r][j], on = c_tab.Ni[r][j];
    C.Md[e] = (N >= 2 && om >= 0) ? Ag[a_xblock(1) + om] : 0.0;
    C.Nd[e] = on >= 0 ? Ag[a_ublock(N, 0) + on] : 0.0;
  }
  for (int e = lane; e < 192; e += 64) C.Gd[e] = 0.0;
  if (lane < 12) {
    C.Pd[lane] = Ag[a_pidx(c_tab, N, 0, lane)];
    C.Hu[lane] = Hg[12 * N + lane];
    C.Hu[12 + lane] = Hg[lane];
  }
  __syncthreads();
  if (lane < 28) C.Gd[c_tab.grow[lane] * 12 + c_tab.gcol[lane]] = Gg[lane];
  bool bad = false;
  for (int e = lane; e < nA; e += 64) {
    int ref;
    if (e < 36 * (N - 1)) ref = e % 36;
    else if (e < a_ubase(N)) ref = a_pidx(c_tab, N, 0, e - 36 * (N - 1));
    else ref = a_ubase(N) + (e - a_ubase(N)) % 86;
    bad |= !(Ag[e] == Ag[ref]);
  }
  for (int e = lane; e < nG; e += 64) bad |= !(Gg[e] == Gg[e % 28]);
  for (int e = lane; e < nz; e += 64) bad |= !(Hg[e] == Hg[(e < 12 * N ? 0 : 12 * N) + e % 12]);
  if (__any(bad)) {  // not differentiated: NaN in all M rows of every requested output
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int o = 0; o < 6; ++o) {
      if (!args.out[o]) continue;
      double* dst = args.out[o] + row0 * (size_t)width[o];
      const size_t n = (size_t)M * (size_t)width[o];
      for (size_t e = lane; e < n; e += 64) dst[e] = qnan;
    }
    if (args.status && lane == 0) args.status[env] = kStatusUnsupported;
    return;
  }
  C.constants(Ag[a_ubase(N) + c_tab.e6], Ag[a_ubase(N) + c_tab.e9]);

  // ---- the iterate and its factorisation, once ----
  {
    const double* xg = args.in[6] + (size_t)env * nz;
    const double* sg = args.in[7] + (size_t)env * m;
    const double* zg = args.in[8] + (size_t)env * m;
    const double* yg = args.in[9] + (size_t)env * p;
    for (int e = lane; e < nz; e += 64) C.X[e] = xg[e];
    for (int e = lane; e < m; e += 64) {
      C.S[e] = sg[e];
      C.Z[e] = zg[e];
    }
    for (int e = lane; e < p; e += 64) C.Y[e] = yg[e];
  }
  __syncthreads();
  C.factor();

  const BackwardSeeds sd = seeds_taken<FULL>(args.grad_x, args.more);
  const bool hasJ = sd.grad_objective != nullptr;
  const double* fg = hasJ ? args.in[3] + (size_t)env * nz : nullptr;
  bool nf = false;
#pragma unroll 1
  for (int k = 0; k < M; ++k) {
    // ---- seed k's right-hand side [g~_k; g_s; g_z; g_y]: every array the solve, the refinement and the
    // epilogue read is written here or by this seed's own solve (refine_rhs overwrites RX and RE,
    // solve(2) leaves its correction in VV, xsg / ysg are rewritten by refine_rhs) ----
    const size_t srow = args.shared ? (size_t)k : row0 + (size_t)k;
    const double gJ = hasJ ? sd.grad_objective[srow] : 0.0;
    seed_rhs(C, sd, srow, fg, N);
    seeded_vv(C, sd, N);
    __syncthreads();

    // ---- one solve and one refinement step against the full K ----
    C.solve(3, 0.0);
    C.refine_rhs();
    C.solve(2, 0.0);
    // lx = TV, ls = DS, lz = DZ, ly = saved + correction
    double* LY = C.ysg;
    for (int e = lane; e < p; e += 64) LY[e] = LY[e] + C.DY[e];
    __syncthreads();

    // ---- gradients, row env * M + k ----
    const size_t row = row0 + (size_t)k;
    double* oH = args.out[0] ? args.out[0] + row * nz : nullptr;
    double* of = args.out[1] ? args.out[1] + row * nz : nullptr;
    double* oA = args.out[2] ? args.out[2] + row * nA : nullptr;
    double* ob = args.out[3] ? args.out[3] + row * p : nullptr;
    double* oG = args.out[4] ? args.out[4] + row * nG : nullptr;
    double* od = args.out[5] ? args.out[5] + row * m : nullptr;
    const double *lx = C.TV, *lz = C.DZ;
    for (int e = lane; e < nz; e += 64) {
      nf = nf || not_finite(lx[e]);
      if (oH) oH[e] = hasJ ? add_objective_H(grad_diag(lx[e], C.X[e]), gJ, C.X[e]) : grad_diag(lx[e], C.X[e]);
      if (of) of[e] = hasJ ? add_objective_f(-lx[e], gJ, C.X[e]) : -lx[e];
    }
    if (oA)
      for (int e = lane; e < nA; e += 64) {
        int r, c;
        a_entry_rc(e, N, r, c);
        oA[e] = grad_entry(lx[c], C.Y[r], LY[r], C.X[c]);
      }
    for (int e = lane; e < p; e += 64) {
      nf = nf || not_finite(LY[e]);
      if (ob) ob[e] = LY[e];
    }
    if (oG)
      for (int e = lane; e < nG; e += 64) {
        const int i = e / 28, q = e % 28;
        const int r = 16 * i + c_tab.grow[q], c = 12 * N + 12 * i + c_tab.gcol[q];
        oG[e] = grad_entry(lx[c], C.Z[r], lz[r], C.X[c]);
      }
    for (int e = lane; e < m; e += 64) {
      nf = nf || not_finite(lz[e]);
      if (od) od[e] = lz[e];
    }
    __syncthreads();  // the epilogue's reads of TV, DZ, LY before the next seed's right-hand side and solve
  }
  if (args.status) {
    const bool any_nf = __any(nf);
    if (lane == 0) args.status[env] = any_nf ? kStatusNonFinite : 0;
  }
}

namespace bwd {
// host side of the backward translation unit (srbd_backward.hip): the kernels as the main unit launches
// them, 64 threads per env with backward_lds_bytes(N) of dynamic LDS
// full: the instantiation that takes every cotangent; otherwise grad_x alone
const void* adjoint_kernel(bool full);        // (BackwardArgs)
const void* adjoint_multi_kernel(bool full);  // (BackwardMultiArgs)
}  // namespace bwd

}  // namespace srbd
