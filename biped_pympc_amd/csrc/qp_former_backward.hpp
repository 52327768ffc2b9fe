// qp_former_backward.hpp -- the vector-Jacobian product of qp_former (qp_former.hpp; SURVEY.md
// Appendix A.1): the gradients of the six QP outputs (H, f, A, b, G, d nonzeros) folded back onto the
// 17 former inputs.
//
// qp_former is an affine map of most inputs composed with the closed-form discrete model
//   A_d = I + dt Ac,  B_d = (dt I + dt^2/2 Ac) Bc,  c_d = (dt I + dt^2/2 Ac) cc,
// so its transpose is a handful of sums over stages (every stage repeats the same block values, so the
// stage gradients of a block value add up) and the chain rule through the model:
//   Q, R          <- grad_H and (Q only) grad_f, f = -Q x_ref
//   x_ref         <- grad_f
//   contact_table <- grad_d (row k = 7 of each foot: d = Fmax * contact), ct[i, j] = v[i + N j]
//   mu            <- grad_G (the -mu entries of the friction rows)
//   x0            <- grad_b (stage 0: A_d x0 + c_d)
//   dt, m, R_body, I_world, body / foot positions, residual accelerations <- grad_A, grad_b through
//                    A_d, B_d, c_d (R_body and I_world decoded column-major, as the former reads them)
//   x, u          <- zero: the model is affine, the QP does not depend on the linearisation point
// Mapping: one wavefront per gradient row, four rows per workgroup, as the former; the row's model is
// recomputed by the former's own device code (former_model). Sums run in a fixed order per entry and
// products are not contracted: an env's gradients do not depend on its position in the batch.
// Seed rows (pdipm_backward.hpp, several seeds at one iterate): with n_seeds = M the gradients g[] and
// out[] have batch * M rows and row r belongs to env r / M, whose former inputs it reads; M = 1 is one
// row per env.
#pragma once
#include "qp_former.hpp"

namespace srbd {

struct FormerBackwardArgs {
  const double* in[17];  // the former inputs
  const double* g[6];    // grad_H, grad_f, grad_A, grad_b, grad_G, grad_d; null: taken as zero
  double* out[17];       // gradients of the former inputs; null: not written
  int N;
  int batch;
  int n_seeds;           // M >= 1: g[] and out[] hold batch * M rows, row r of env r / M
};

struct FormerBackwardLds {
  FormerLds F;
  double gXB[36];   // gradient of one x block of A (summed over k < N)
  double gUB[86];   // gradient of one u block of A (summed over stages)
  double gcd[12];   // gradient of c_d (every stage's b)
  double gax[12];   // gradient of A_d x0 (stage 0's b)
  double gBd[144];  // gradient of B_d, row-major
  double gMa[36];   // gradient of Ma = I^-1 [skew(rL) | skew(rR) | I | I]
  double gIi[9];    // gradient of I^-1
  double gS[18];    // gradients of skew(rL), skew(rR), row-major 3x3 each
  double gmu[28];   // per G value of a stage: its gradient summed over stages
};

__device__ __forceinline__ double bw_ld(const double* g, int e) { return g ? g[e] : 0.0; }

template <int kWaves>
__global__ __launch_bounds__(64 * kWaves) void qp_former_backward_kernel(FormerBackwardArgs args) {
#pragma clang fp contract(off)
  __shared__ FormerBackwardLds lds[kWaves];
  const Tables& tab = c_tab;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = xcd_item(blockIdx.x, gridDim.x) * kWaves + wave;
  if (row >= args.batch * args.n_seeds) return;
  const int env = row / args.n_seeds;
  const int N = args.N;
  FormerBackwardLds& W = lds[wave];
  FormerLds& L = W.F;
  const int in_nnz[17] = {12, 12 * N, 12 * N, 12 * N, 1, 1, 1, 9, 9, 3, 3, 3, 2 * N, 12, 12, 3, 3};
  const double* P[17];
  double* O[17];
#pragma unroll
  for (int i = 0; i < 17; ++i) {
    P[i] = args.in[i] + (size_t)env * in_nnz[i];
    O[i] = args.out[i] ? args.out[i] + (size_t)row * in_nnz[i] : nullptr;
  }
  former_model(L, P, lane);
  const double dt = P[4][0], mass = P[5][0], h2 = 0.5 * dt * dt;
  const double* gH = args.g[0] ? args.g[0] + (size_t)row * (24 * N) : nullptr;
  const double* gf = args.g[1] ? args.g[1] + (size_t)row * (24 * N) : nullptr;
  const double* gA = args.g[2] ? args.g[2] + (size_t)row * nnz_A(N) : nullptr;
  const double* gb = args.g[3] ? args.g[3] + (size_t)row * (14 * N) : nullptr;
  const double* gG = args.g[4] ? args.g[4] + (size_t)row * (28 * N) : nullptr;
  const double* gd = args.g[5] ? args.g[5] + (size_t)row * (16 * N) : nullptr;
  const double* Qw = P[13];
  const double* xr = P[3];

  // ---- sums over stages of the periodic values, and the inputs the QP is affine in ----
  for (int e = lane; e < 36 + 86; e += 64) {
    double a = 0.0;
    if (e < 36) {
      for (int k = 1; k < N; ++k) a += bw_ld(gA, a_xblock(k) + e);
      W.gXB[e] = a;
    } else {
      for (int i = 0; i < N; ++i) a += bw_ld(gA, a_ublock(N, i) + (e - 36));
      W.gUB[e - 36] = a;
    }
  }
  if (lane < 12) {
    double c = 0.0, q = 0.0, r = 0.0;
    for (int i = 0; i < N; ++i) {
      c += bw_ld(gb, 12 * i + lane);
      q += bw_ld(gH, 12 * i + lane) - bw_ld(gf, 12 * i + lane) * xr[12 * i + lane];
      r += bw_ld(gH, 12 * N + 12 * i + lane);
    }
    W.gcd[lane] = c;
    W.gax[lane] = bw_ld(gb, lane);
    if (O[13]) O[13][lane] = q;
    if (O[14]) O[14][lane] = r;
  }
  if (lane < 28) {
    double a = 0.0;
    const bool fz = tab.gcol[lane] % 3 == 2 && tab.gcol[lane] < 6;
    if (fz && tab.grow[lane] % 8 < 4)  // the -mu entries (former_g)
      for (int i = 0; i < N; ++i) a += bw_ld(gG, 28 * i + lane);
    W.gmu[lane] = a;
  }
  for (int e = lane; e < 12 * N; e += 64) {
    if (O[1]) O[1][e] = 0.0;
    if (O[2]) O[2][e] = 0.0;
    if (O[3]) O[3][e] = -(Qw[e % 12] * bw_ld(gf, e));
  }
  if (O[12])
    for (int t = lane; t < 2 * N; t += 64) {  // ct[i, f] = v[i + N f]
      const int f = t / N, i = t - f * N;
      O[12][t] = kFMax * bw_ld(gd, 16 * i + 8 * f + 7);
    }
  __syncthreads();

  // ---- gradient of B_d from the u block (A holds -B_d) ----
  for (int e = lane; e < 144; e += 64) {
    const int on = tab.Ni[e / 12][e % 12];
    W.gBd[e] = on >= 0 ? -W.gUB[on] : 0.0;
  }
  __syncthreads();
  // gradient of A_d's R entries (rows 0..2, columns 6..8) and dt entries (rows 3..5) from the x block
  auto gAdR = [&](int r, int c) { return -W.gXB[tab.Mi[r][6 + c]]; };
  auto gAdt = [&](int r) { return -W.gXB[tab.Mi[r][r + 6]]; };
  auto lin = [&](int r, int c) { return (c < 6 && (c % 3) == (r % 3)) ? 1.0 / mass : 0.0; };
  const double* aa = P[16];
  const double* al = P[15];
  const double* x0 = P[0];
  auto glin = [&](int r) { return (r % 3 == 2 ? kGravZ : 0.0) + al[r % 3]; };

  // ---- phase A: everything that reads gBd, gcd, gax ----
  if (lane < 36) {  // Ma[a][c]: B_d rows 0..2 = h2 R Ma, rows 6..8 = dt Ma
    const int a = lane / 12, c = lane % 12;
    double v = 0.0;
    for (int r = 0; r < 3; ++r) v += W.gBd[r * 12 + c] * L.R[3 * r + a];
    W.gMa[lane] = h2 * v + dt * W.gBd[(6 + a) * 12 + c];
  } else if (lane < 45) {  // R_body[r][a], stored column-major
    const int r = (lane - 36) / 3, a = (lane - 36) % 3;
    double v = 0.0;
    for (int c = 0; c < 12; ++c) v += W.gBd[r * 12 + c] * L.Ma[12 * a + c];
    v = h2 * v + h2 * (W.gcd[r] * aa[a]) + dt * (W.gax[r] * x0[6 + a]) + dt * gAdR(r, a);
    if (O[7]) O[7][r + 3 * a] = v;
  } else if (lane == 45) {  // dt (directly and through h2 = dt^2 / 2) and m
    double g2 = 0.0, g1 = 0.0, gim = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double* Rr = L.R + 3 * r;
      for (int c = 0; c < 12; ++c)
        g2 += W.gBd[r * 12 + c] * (Rr[0] * L.Ma[c] + Rr[1] * L.Ma[12 + c] + Rr[2] * L.Ma[24 + c]);
      g2 += W.gcd[r] * (Rr[0] * aa[0] + Rr[1] * aa[1] + Rr[2] * aa[2]);
      g1 += W.gax[r] * (Rr[0] * x0[6] + Rr[1] * x0[7] + Rr[2] * x0[8]);
      for (int c = 0; c < 3; ++c) g1 += gAdR(r, c) * Rr[c];
    }
    for (int r = 3; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) {
        g2 += W.gBd[r * 12 + c] * lin(r, c);
        g1 += W.gBd[(r + 6) * 12 + c] * lin(r, c);
        if (c % 3 == r % 3) gim += h2 * W.gBd[r * 12 + c] + dt * W.gBd[(r + 6) * 12 + c];
      }
      g2 += W.gcd[r] * glin(r);
      g1 += W.gcd[r + 6] * glin(r);
      g1 += W.gax[r] * x0[r + 6] + gAdt(r);
    }
    for (int a = 0; a < 3; ++a) {
      for (int c = 0; c < 12; ++c) g1 += W.gBd[(6 + a) * 12 + c] * L.Ma[12 * a + c];
      g1 += W.gcd[6 + a] * aa[a];
    }
    if (O[4]) O[4][0] = g1 + g2 * dt;
    if (O[5]) O[5][0] = -gim / (mass * mass);
  } else if (lane < 49) {  // residual angular acceleration
    const int a = lane - 46;
    double v = 0.0;
    for (int r = 0; r < 3; ++r) v += W.gcd[r] * L.R[3 * r + a];
    if (O[16]) O[16][a] = h2 * v + dt * W.gcd[6 + a];
  } else if (lane < 52) {  // residual linear acceleration
    const int k = lane - 49;
    if (O[15]) O[15][k] = h2 * W.gcd[3 + k] + dt * W.gcd[9 + k];
  } else {  // x0 through A_d x0
    const int j = lane - 52;
    double v = W.gax[j];
    if (j >= 9) {
      v += dt * W.gax[j - 6];
    } else if (j >= 6) {
      double t = 0.0;
      for (int r = 0; r < 3; ++r) t += W.gax[r] * L.R[3 * r + j - 6];
      v += dt * t;
    }
    if (O[0]) O[0][j] = v;
  }
  if (lane == 0 && O[6]) {  // mu
    double a = 0.0;
    for (int q = 0; q < 28; ++q) a += W.gmu[q];
    O[6][0] = -a;
  }
  __syncthreads();

  // ---- phase B: I^-1 and the two skew blocks from Ma ----
  auto skew = [&](const double* v, int r, int c) {  // [[0,-vz,vy],[vz,0,-vx],[-vy,vx,0]]
    if (r == c) return 0.0;
    const int k = 3 - r - c;
    const double s = ((c - r + 3) % 3 == 1) ? -1.0 : 1.0;
    return s * v[k];
  };
  if (lane < 9) {
    const int a = lane / 3, k = lane % 3;
    double v = W.gMa[12 * a + 6 + k] + W.gMa[12 * a + 9 + k];
    for (int fi = 0; fi < 2; ++fi)
      for (int c = 0; c < 3; ++c) v += W.gMa[12 * a + 3 * fi + c] * skew(L.rv + 3 * fi, k, c);
    W.gIi[lane] = v;
  } else if (lane < 27) {
    const int fi = (lane - 9) / 9, r = ((lane - 9) % 9) / 3, c = (lane - 9) % 3;
    double v = 0.0;
    for (int a = 0; a < 3; ++a) v += L.Ii[3 * a + r] * W.gMa[12 * a + 3 * fi + c];
    W.gS[lane - 9] = v;
  }
  __syncthreads();

  // ---- phase C: I_world (through the inverse), foot and body positions ----
  if (lane < 9) {  // -I^-T g I^-T, stored column-major
    const int r = lane / 3, c = lane % 3;
    double v = 0.0;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) v += L.Ii[3 * a + r] * W.gIi[3 * a + b] * L.Ii[3 * c + b];
    if (O[8]) O[8][r + 3 * c] = -v;
  } else if (lane < 12) {
    const int k = lane - 9, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    // d/dv_k of skew(v): +1 at (k2, k1), -1 at (k1, k2)
    const double gl = W.gS[3 * k2 + k1] - W.gS[3 * k1 + k2];
    const double gr = W.gS[9 + 3 * k2 + k1] - W.gS[9 + 3 * k1 + k2];
    if (O[10]) O[10][k] = gl;
    if (O[11]) O[11][k] = gr;
    if (O[9]) O[9][k] = -(gl + gr);
  }
}

namespace bwd {
void launch_former_backward(const FormerBackwardArgs& a, hipStream_t s);
}  // namespace bwd

}  // namespace srbd
