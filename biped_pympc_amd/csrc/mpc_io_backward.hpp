// mpc_io_backward.hpp -- the vector-Jacobian products of the controller step's FP32 ends (mpc_io.hpp):
// the u0 -> wrench / stance-torque epilogue (u0_wrench_kernel) and the input preparation (prepare_env).
// Between them sits the backward pass of the QP (pdipm_backward.hpp, qp_former_backward.hpp), so the chain
//   grad_wrench (, grad_tau) -> grad_x -> 17 former-input cotangents -> the controller's own FP32 tensors
// closes on the tensors a user of MPCControllerHIP holds.
//
// Arithmetic of both kernels: the forward's FP32 values are read and widened to FP64; every product and
// sum is FP64, not contracted, in a fixed order per entry; intermediate cotangents are FP64; a gradient on
// an FP32 controller input is rounded once, at its store. The forward intermediates the derivative needs
// (vw0, vw1, stationary) are recomputed with the forward's own FP32 ops. The selects (first_run,
// stationary) are constants of the derivative. No entry depends on the env's position in the batch.
//
// prepare_env is linear in the knot-point state it reads, so its VJP does not read world_position_desired
// or yaw_desired; first_run is the flag as it was BEFORE the forward step (the step clears it).
#pragma once
#include "../../include/srbd_mpc.h"  // SRBD_PREP_GRAD_*: the indices of the 15 gradients written here
#include "mpc_io.hpp"

namespace srbd {

struct PrepBackwardArgs {
  PrepArgs prep;        // the forward's arguments; read: rotation_body, des_vel_b, des_angvel_b, dt_mpc,
                        // first_run (pre-step snapshot), I_body, step_dt, literal, N, batch. Nothing is written.
  const double* g[17];  // cotangents of the 17 former inputs; null: zero
  const float* gwpd;    // (B,3) cotangent of the updated world_position_desired; null: zero
  const float* gyaw;    // (B)   cotangent of the updated yaw_desired; null: zero
  const double* gR;     // (B,9) direct term of rotation_body (the wrench's), added before the rounding; null: zero
  float* out[SRBD_PREP_GRAD_COUNT];  // null: not written
};

__device__ __forceinline__ double pb_ld(const double* g, size_t i) { return g ? g[i] : 0.0; }

// One wave per env, 4 envs per 256-thread block, as prepare_inputs_kernel. The sums over stages of the
// x_ref cotangent, S_j = sum_k gx[k, j] and T_j = sum_k k gx[k, j], are wave reductions: lane 12 r + j
// (r < 5) adds the stages k = r, r + 5, ... of column j in increasing k, then the five partial sums of
// a column are added in increasing r -- one order whatever the batch.
__global__ __launch_bounds__(256) void prepare_inputs_backward_kernel(PrepBackwardArgs a) {
#pragma clang fp contract(off)
  const PrepArgs& p = a.prep;
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= p.batch) return;  // wave-uniform
  const int N = p.N;
  const size_t se = (size_t)e;
  const bool first = p.first_run[e] != 0;
  const float* vb = p.des_vel_b + 3 * se;
  const float vb0 = vb[0], vb1 = vb[1], vb2 = vb[2];
  const float wz = p.des_angvel_b[3 * se + 2], dt = p.dt_mpc[e];
  const float* Rp = p.rotation_body + 9 * se;
  // the forward's own FP32 intermediates
  const bool stationary = fabsf(vb0) < 1e-2f;
  const float vw0 = dot3f(Rp[0], Rp[1], Rp[2], vb0, vb1, vb2);
  const float vw1 = dot3f(Rp[3], Rp[4], Rp[5], vb0, vb1, vb2);

  // ---- S_j, T_j over the stages ----
  const int j12 = lane % 12, r5 = lane / 12;
  const double* gx = a.g[3] ? a.g[3] + se * 12 * N : nullptr;
  double s = 0.0, t = 0.0;
  if (gx && r5 < 5)
    for (int k = r5; k < N; k += 5) {
      const double v = gx[12 * k + j12];
      s += v;
      t += (double)k * v;
    }
  double S = 0.0, T = 0.0;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    S += __shfl(s, j12 + 12 * q, 64);
    T += __shfl(t, j12 + 12 * q, 64);
  }
  const double S2 = __shfl(S, 2, 64), S3 = __shfl(S, 3, 64), S4 = __shfl(S, 4, 64), S5 = __shfl(S, 5, 64);
  const double S8 = __shfl(S, 8, 64), S9 = __shfl(S, 9, 64), S10 = __shfl(S, 10, 64);
  const double T2 = __shfl(T, 2, 64), T3 = __shfl(T, 3, 64), T4 = __shfl(T, 4, 64);

  const double c = (double)p.step_dt, dtd = (double)dt;
  const double gw0 = a.gwpd ? (double)a.gwpd[3 * se] : 0.0;
  const double gw1 = a.gwpd ? (double)a.gwpd[3 * se + 1] : 0.0;
  const double gw2 = a.gwpd ? (double)a.gwpd[3 * se + 2] : 0.0;
  const double gyaw = S2 + (a.gyaw ? (double)a.gyaw[e] : 0.0);  // cotangent of the advanced yaw
  const double gv0 = dtd * T3 + S9, gv1 = dtd * T4 + S10;       // cotangents of vw0, vw1

  if (lane < 12) {  // the four x0 groups: root_euler, root_position, angular velocity, velocity
    const int f = lane / 3, i = lane % 3;
    double v = pb_ld(a.g[0], 12 * se + lane);
    if (f == 0 && i == 2 && first) v += gyaw;
    if (f == 1) {
      v += pb_ld(a.g[9], 3 * se + i);
      if (i < 2) {
        if (!(stationary && !first)) v += i == 0 ? S3 : S4;
        if (first) v += i == 0 ? gw0 : gw1;
      }
    }
    float* o = a.out[f];  // SRBD_PREP_GRAD_ROOT_EULER .. ROOT_VELOCITY_W are 0..3
    if (o) o[3 * se + i] = (float)v;
  } else if (lane < 21) {  // rotation_body[i][jj]
    float* o = a.out[SRBD_PREP_GRAD_ROTATION_BODY];
    if (o) {
      const int l = lane - 12, i = l / 3, jj = l % 3;
      const double vbj = (double)(jj == 0 ? vb0 : jj == 1 ? vb1 : vb2);
      double v = i == 0 ? gv0 * vbj : i == 1 ? gv1 * vbj : 0.0;
      v += pb_ld(a.g[7], 9 * se + (p.literal ? 3 * i + jj : 3 * jj + i));
      if (a.g[8]) {  // I_world = R I_body R^T: Gamma R I_body^T + Gamma^T R I_body
        const double* G8 = a.g[8] + 9 * se;
        double A = 0.0, B = 0.0;
        for (int m = 0; m < 3; ++m) {
          double ra = 0.0, rb = 0.0;
          for (int n = 0; n < 3; ++n) {
            ra += (double)Rp[3 * m + n] * (double)p.I_body[3 * jj + n];
            rb += (double)Rp[3 * m + n] * (double)p.I_body[3 * n + jj];
          }
          A += G8[3 * i + m] * ra;
          B += G8[3 * m + i] * rb;
        }
        v += A + B;
      }
      v += pb_ld(a.gR, 9 * se + l);
      o[9 * se + l] = (float)v;
    }
  } else if (lane < 27) {  // foot_position: left, right
    const int l = lane - 21;
    float* o = a.out[SRBD_PREP_GRAD_FOOT_POSITION];
    if (o) o[6 * se + l] = (float)pb_ld(a.g[10 + l / 3], 3 * se + l % 3);
  } else if (lane < 30) {  // desired_velocity_b
    const int jj = lane - 27;
    float* o = a.out[SRBD_PREP_GRAD_DESIRED_VELOCITY_B];
    if (o) {
      double v = gv0 * (double)Rp[jj] + gv1 * (double)Rp[3 + jj];
      if (jj < 2) {
        if (stationary) v += c * (jj == 0 ? S3 : S4);
        v += c * (jj == 0 ? gw0 : gw1);
      }
      o[3 * se + jj] = (float)v;
    }
  } else if (lane < 33) {  // desired_angular_velocity_b: only the yaw rate is read
    const int jj = lane - 30;
    float* o = a.out[SRBD_PREP_GRAD_DESIRED_ANGULAR_VELOCITY_B];
    if (o) o[3 * se + jj] = jj == 2 ? (float)((c * gyaw + dtd * T2) + S8) : 0.0f;
  } else if (lane == 33) {
    float* o = a.out[SRBD_PREP_GRAD_DESIRED_HEIGHT];
    if (o) o[e] = (float)(S5 + gw2);
  } else if (lane < 37) {  // world_position_desired as read (its third entry is overwritten by the height)
    const int i = lane - 34;
    float* o = a.out[SRBD_PREP_GRAD_WORLD_POSITION_DESIRED];
    if (o) {
      double v = 0.0;
      if (i < 2) v = ((stationary && !first) ? (i == 0 ? S3 : S4) : 0.0) + (first ? 0.0 : (i == 0 ? gw0 : gw1));
      o[3 * se + i] = (float)v;
    }
  } else if (lane == 37) {
    float* o = a.out[SRBD_PREP_GRAD_YAW_DESIRED];
    if (o) o[e] = first ? 0.0f : (float)gyaw;
  } else if (lane == 38) {
    float* o = a.out[SRBD_PREP_GRAD_DT_MPC];
    if (o) o[e] = (float)(((pb_ld(a.g[4], se) + (double)wz * T2) + (double)vw0 * T3) + (double)vw1 * T4);
  } else if (lane < 42) {
    float* o = a.out[SRBD_PREP_GRAD_RESIDUAL_LIN_ACCEL];
    if (o) o[3 * se + lane - 39] = (float)pb_ld(a.g[15], 3 * se + lane - 39);
  } else if (lane < 45) {
    float* o = a.out[SRBD_PREP_GRAD_RESIDUAL_ANG_ACCEL];
    if (o) o[3 * se + lane - 42] = (float)pb_ld(a.g[16], 3 * se + lane - 42);
  }
  // contact_table[k][l]: the flattening prepare_env applied, undone (explicit-table mode only: the host
  // entry refuses this output when the schedule comes from the gait phase)
  if (float* o = a.out[SRBD_PREP_GRAD_CONTACT_TABLE])
    for (int q = lane; q < 2 * N; q += 64) {
      const int k = q / 2, l = q % 2;
      o[se * 2 * N + q] = (float)pb_ld(a.g[12], se * 2 * N + (p.literal ? q : l * N + k));
    }
}

// The VJP of u0_wrench_kernel, one thread per env: grad_wrench (B,2,6) and optionally grad_tau (B,2,ndof)
// -> grad_x (B,24N) FP64 (the whole row is written: zeros outside the u0 block, and at its entries 6 and
// 9, which the forward zeroes) and optionally the direct term grad_R (B,9) FP64 of rotation_body.
__global__ __launch_bounds__(256) void u0_wrench_backward_kernel(int N, int batch, const double* __restrict__ x,
                                                                 const float* __restrict__ rotation_body,
                                                                 const float* __restrict__ grad_wrench, int ndof,
                                                                 const float* __restrict__ J,
                                                                 const float* __restrict__ contact,
                                                                 const float* __restrict__ grad_tau,
                                                                 double* __restrict__ grad_x,
                                                                 double* __restrict__ grad_R) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= batch) return;
  const size_t se = (size_t)e;
  double gw[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) gw[j] = (double)grad_wrench[se * 12 + j];
  if (grad_tau) {  // tau_l = contact_l ? J_l^T w_l : 0
#pragma unroll
    for (int l = 0; l < 2; ++l) {
      if (contact[se * 2 + l] == 0.0f) continue;
      const float* Jl = J + (se * 2 + l) * 6 * ndof;
      const float* gt = grad_tau + (se * 2 + l) * ndof;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double sum = 0.0;
        for (int k = 0; k < ndof; ++k) sum += (double)Jl[j * ndof + k] * (double)gt[k];
        gw[6 * l + j] += sum;
      }
    }
  }
  double Rm[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rm[k] = (double)rotation_body[9 * se + k];
  double* row = grad_x + se * 24 * N;
  for (int q = 0; q < 12 * N; ++q) row[q] = 0.0;
  for (int q = 12 * N + 12; q < 24 * N; ++q) row[q] = 0.0;
  // w[3b + i] = -sum_k R[k][i] u[src_b + k], blocks [lf, lm | rf, rm] of u = [lf, rf, lm, rm]
  constexpr int src[4] = {0, 6, 3, 9};
  double* gu = row + 12 * N;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int q = src[b] + k;
      const double v = -((Rm[3 * k] * gw[3 * b] + Rm[3 * k + 1] * gw[3 * b + 1]) + Rm[3 * k + 2] * gw[3 * b + 2]);
      gu[q] = (q == 6 || q == 9) ? 0.0 : v;
    }
  if (!grad_R) return;
  double u[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) u[q] = (q == 6 || q == 9) ? 0.0 : (double)(float)x[se * 24 * N + 12 * N + q];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double sum = 0.0;
#pragma unroll
      for (int b = 0; b < 4; ++b) sum += u[src[b] + k] * gw[3 * b + i];
      grad_R[9 * se + 3 * k + i] = -sum;
    }
}

// The cotangent of the step's objective_f32 (B) widened to FP64 for the adjoint kernel: the one rounding of
// J to float32 in the forward is read as the identity.
__global__ __launch_bounds__(256) void widen_f32_kernel(int n, const float* __restrict__ src,
                                                        double* __restrict__ dst) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) dst[e] = (double)src[e];
}

namespace bwd {
void launch_widen(int n, const float* src, double* dst, hipStream_t s);
void launch_prepare_backward(const PrepArgs& prep, const double* const* g, const float* gwpd, const float* gyaw,
                             const double* gR, float* const* out, hipStream_t s);
void launch_wrench_backward(int N, int batch, const double* x, const float* rotation_body, const float* grad_wrench,
                            int ndof, const float* J, const float* contact, const float* grad_tau, double* grad_x,
                            double* grad_R, hipStream_t s);
}  // namespace bwd

}  // namespace srbd
