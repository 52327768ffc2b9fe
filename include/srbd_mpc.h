/*
 * srbd_mpc.h -- C-ABI of the MI355X-native SRBD-MPC QP engine (libsrbd_mpc.so + thin drop-ins).
 *
 * Drop-in boundary for the reference's CusADi hot path (rl-augmented-mpc/Biped-PyMPC):
 *   - `evaluate` below is the exact symbol each CusADi function library exports
 *     (reference biped_pympc/cusadi/src/generateCUDACode.py:157-183) and that
 *     CusadiFunction binds through ctypes (biped_pympc/cusadi/src/CusadiFunction.py:28-47).
 *     Two thin libraries export it: libqp_former.so (CasADi Function 'qp_former',
 *     srbd_constraints.py:75-79) and libsparse_pdipm_multiple_iterations.so ('sparse_pdipm_multiple_iterations',
 *     sparse_pdipm_solver.py:532-534), built for the deployed configuration N = 10, 5 iterations
 *     (mpc_controller_cusadi.py:28; generate_solver_function.py:106). Other horizons/iteration counts
 *     get libqp_former_N<N>.so / libsparse_pdipm_multiple_iterations_N<N>_K<K>.so.
 *   - the srbd_* entry points are the extended API (runtime horizon and iteration count, caller's
 *     HIP stream, fused former+solve), all plain pointers and sizes.
 *
 * Memory: every double* is DEVICE memory, batched row-major (batch, nnz) per tensor, exactly the
 * CusADi layout (input i of env e at inputs[i] + e*nnz_in[i]). The library allocates nothing on
 * the device; it never calls exit(): failures return an error code and set srbd_last_error().
 */
#ifndef SRBD_MPC_H_
#define SRBD_MPC_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRBD_ABI_VERSION 1
#define SRBD_MAX_HORIZON 32

/* ---- CusADi ABI (thin per-function libraries) ---------------------------------------------
 * inputs/outputs: DEVICE pointer to a DEVICE array of n_in / n_out DEVICE pointers
 * (CusadiFunction.py:84-92). work: ignored (CusADi's (batch, sz_w) scratch; may be NULL).
 * Blocking, legacy default stream. Returns kernel time in SECONDS (generateCUDACode.py:176-182),
 * or a negative value on error (the reference's gpuErrchk calls exit(); this never does). */
float evaluate(const double* inputs[], double* work, double* outputs[], const int batch_size);

/* ---- Extended API (libsrbd_mpc.so) ------------------------------------------------------------ */
int srbd_abi_version(void);
const char* srbd_last_error(void);
/* Build provenance: 16 hex digits of sha256 over the library's sources and compile flags
 * (biped_pympc_amd/build.py source_hash); smoke() and bench.py print it. */
const char* srbd_build_id(void);

/* CusADi-ABI implementations with explicit configuration (what the thin libraries call). */
float srbd_evaluate_qp_former(int horizon, const double* inputs[], double* work, double* outputs[],
                              int batch);
float srbd_evaluate_pdipm(int horizon, int n_iter, const double* inputs[], double* work,
                          double* outputs[], int batch);

/* qp_former: 17 inputs (x0, x, u, x_ref, dt, m, mu, R_body, I_world, body_pos, left_foot_pos,
 * right_foot_pos, contact_table, Q, R, residual_lin_accel, residual_ang_accel;
 * srbd_constraints.py:77) -> 6 outputs (nonzeros of H, f, A, b, G, d in CCS order).
 * `inputs`/`outputs` are HOST arrays of device pointers. Asynchronous on `stream` (hipStream_t,
 * NULL = default stream). Returns 0 or a hipError_t code. */
int srbd_qp_former(int horizon, int batch, const double* const* inputs, double* const* outputs,
                   void* stream);

/* sparse PDIPM: 10 inputs (Q_val, G_val, A_val, f, h, b, x, s, z, y; sparse_pdipm_solver.py:533)
 * -> 6 outputs (x, s, z, y, residuals[4] = [|rx|, |rs|, |re|, mu_new], mu_new), n_iter >= 1
 * Newton iterations at run time. Host array of device pointers; asynchronous on `stream`. */
int srbd_pdipm(int horizon, int n_iter, int batch, const double* const* inputs,
               double* const* outputs, void* stream);

/* Same, but the iterate is initialised on device as the GPU caller does
 * (mpc_controller_cusadi.py:138-141): x = 0, s = max(h, 1), z = 1, y = y0. Inputs 6..9 unused
 * (may be NULL). */
int srbd_pdipm_cold(int horizon, int n_iter, int batch, double y0, const double* const* inputs,
                    double* const* outputs, void* stream);

/* The reference's `_ccs` solver entry (sparse_pdipm_solver_ccs, sparse_pdipm_solver.py:4-35, and
 * initialize_pdipm_variables :537-558): the iterate starts from an arbitrary primal guess,
 * x = x_init (input 6), s = max(h - G x_init, 1), z = 1, y = 0; inputs 7..9 unused (may be NULL).
 * The reference Function returns x only; here all 6 outputs as srbd_pdipm. */
int srbd_pdipm_ccs(int horizon, int n_iter, int batch, const double* const* inputs, double* const* outputs,
                   void* stream);

/* Per-problem status word (failure detection; the reference has no such output, only its
 * clamps, sparse_pdipm_solver.py:466-467,501-515): int32 per env, OR of
 *   SRBD_STATUS_NONFINITE  a NaN / Inf in the returned x, s, z, y or mu
 *   SRBD_STATUS_STEP_FLOOR a combined-direction step length (primal or dual) at its 1e-12 floor in the
 *                          last iteration (the iterate is stalled at the boundary)
 *   SRBD_STATUS_FALLBACK   the QP was not stage-invariant and a stage-invariant kernel (solver path
 *                          "auto" or "lds") solved it by its in-launch general fallback; set only there:
 *                          under the "general" path (srbd_set_solver_path(1)) every QP takes the general
 *                          kernel and this bit stays clear
 * Written by the *_ex and *_info entry points when status != NULL (device memory, batch ints). */
#define SRBD_STATUS_NONFINITE 1
#define SRBD_STATUS_STEP_FLOOR 2
#define SRBD_STATUS_FALLBACK 4

/* srbd_pdipm (init_mode 0), srbd_pdipm_cold (1, y = y0) or srbd_pdipm_ccs (2) with the status word. */
int srbd_pdipm_ex(int horizon, int n_iter, int batch, int init_mode, double y0, const double* const* inputs,
                  double* const* outputs, int* status, void* stream);

/* Per-problem extras of a solve, each optional (NULL: not computed), all DEVICE memory of `batch`
 * entries; the *_info entry points take a pointer to this struct (NULL: no extras) where the *_ex ones
 * take `int* status`. The struct is read during the call only.
 *   objective: the QP objective of the iterate the call returns (after the last update and clamps),
 *     J = sum_e (H_e x_e / 2 + f_e) x_e over the 24N primal entries (H's CCS pattern is its diagonal;
 *     per-stage values are honoured for QPs that are not stage-invariant) = 0.5 x^T H x + f^T x, what
 *     the reference's qpth and OSQP back ends return as `cost` (mpc_controller_qpth.py:136,
 *     mpc_controller_osqp.py:95; its CusADi back end returns zeros, mpc_controller_cusadi.py:185) and
 *     MPCController.mpc_cost exposes (mpc_wrapper.py:151-153). The constant x_ref^T Q x_ref / 2 is not
 *     added (the reference does not add it). Formed in the solver kernel's epilogue from x, diag(H) and f
 *     on chip: each term with two roundings, one block sum in a fixed order (the fused step and
 *     qp_former -> solver give the same bits). A NaN / Inf in x propagates into J; SRBD_STATUS_NONFINITE
 *     reports it.
 *   objective_f32: the same J rounded once to FP32 (the dtype of the controller's `cost`). */
typedef struct srbd_solve_info {
  int*    status;         /* (B) int32, SRBD_STATUS_* word, or NULL */
  double* objective;      /* (B) FP64 J, or NULL */
  float*  objective_f32;  /* (B) the same J rounded once to FP32, or NULL */
} srbd_solve_info;

/* srbd_pdipm_ex with the extras struct in place of the status pointer (init_mode 0, 1 or 2). */
int srbd_pdipm_info(int horizon, int n_iter, int batch, int init_mode, double y0, const double* const* inputs,
                    double* const* outputs, const srbd_solve_info* info, void* stream);

/* Whole MPC QP step: qp_former -> cold-start PDIPM (n_iter iterations), one stream, no host sync.
 * `qp_workspace` is caller-owned device memory of srbd_mpc_workspace_doubles(horizon, batch)
 * doubles that receives H, f, A, b, G, d (CCS, batched). outputs as srbd_pdipm. */
size_t srbd_mpc_workspace_doubles(int horizon, int batch);
int srbd_mpc_solve(int horizon, int n_iter, int batch, double y0, const double* const* former_inputs,
                   double* qp_workspace, double* const* outputs, void* stream);

/* srbd_mpc_solve in ONE kernel at every horizon (the register kernels at N = 2..32, the
 * LDS-resident step kernel otherwise; a non-auto solver path runs srbd_mpc_solve and needs
 * qp_workspace): the QP is formed in the solver from the former inputs and never written, except
 * f, b, d into their qp_workspace slots when qp_workspace != NULL (NULL: no QP data leaves the
 * kernel). Same outputs as srbd_mpc_solve, bit for bit; any outputs[k] may be NULL (that output is
 * not written). */
int srbd_mpc_solve_fused(int horizon, int n_iter, int batch, double y0, const double* const* former_inputs,
                         double* qp_workspace, double* const* outputs, void* stream);
/* srbd_mpc_solve_fused with the status word (status may be NULL). */
int srbd_mpc_solve_fused_ex(int horizon, int n_iter, int batch, double y0, const double* const* former_inputs,
                            double* qp_workspace, double* const* outputs, int* status, void* stream);
/* srbd_mpc_solve_fused with the extras struct (info may be NULL); a non-auto solver path runs
 * former + solver with the same extras. */
int srbd_mpc_solve_fused_info(int horizon, int n_iter, int batch, double y0, const double* const* former_inputs,
                              double* qp_workspace, double* const* outputs, const srbd_solve_info* info,
                              void* stream);

/* LDS bytes one solver workgroup (one QP) uses at this horizon (0 if unsupported). */
size_t srbd_solver_lds_bytes(int horizon);

/* Solver kernel selection: 0 = auto (default): a stage-invariant kernel for stage-invariant QPs
 * (every QP qp_former emits; register-resident at N = 2..32, LDS-resident otherwise), the general
 * kernel for any other QP in the batch; 1 = general kernel only; 2 = LDS-resident stage-invariant
 * kernel at every horizon (plus the general fallback).
 * Results agree to round-off (tests/test_gpu_parity.py). Per device: applies to calls made while
 * the current HIP device is the one current here.
 *
 * Devices: every entry point works on the HIP device current at the call (one process per GPU is
 * the deployment model; a process that switches devices is supported too). What the
 * library keeps between calls -- configured kernel LDS limits, the blocking calls' events, the
 * solver path -- is kept per device (csrc/device_state.hpp). */
int srbd_set_solver_path(int path);
/* The solver path in effect for the current HIP device (0 if never set). srbd_mpc_solve_fused under a
 * non-auto path runs srbd_mpc_solve and so needs qp_workspace; srbd_mpc_step ignores the path and
 * always runs its one-launch step kernel (its QPs are stage-invariant by construction): the
 * register-resident kernel at N = 2..32, the LDS-resident step kernel at N = 1. */
int srbd_get_solver_path(void);

/* Affine-direction refinement of the register-resident kernels (the default solvers at N = 2..32), per
 * device like the solver path. Every Newton iteration refines the combined direction once against the
 * full KKT; the affine (predictor) direction, whose ds / dz set sigma and the corrector, is refined
 * 0 = (default) at the iterate a solve starts from (every dual z at its initial 1: the cold start's Newton
 *     step is the largest) and in iterations with an ill-conditioned iterate (some row with z / s >= 1e4
 *     or an s at its 1e-8 clamp) -- where an unrefined predictor lets the trajectory drift from the
 *     reference's; about the time at N = 10 of round 5's mode 0 (predictor at z / s >= 1e3 only);
 * 1 = in every iteration (as the LDS-resident and general kernels always do), ~15 % more time at N = 10.
 * scripts/parity_fuzz.py + scripts/parity_floor.py, every env above the tolerance floor-checked, 6657 cases
 * of each sequence: mode 0 fails a few register-kernel warm starts, mode 1 none (DESIGN.md 3.3 has the
 * counts), round 5's mode 0 23 and 26 -- a case fails when an env sits more than 4x its FP64 floor (the
 * larger distance of the AMD-ordered LDL^T and of dense LU from the checker) beyond the K tolerance; no env
 * of either mode is over 1e-4 relative in x or u0 beyond that (profiles/r06/). Returns 0, or
 * an error for another mode. */
int srbd_set_refinement(int mode);
/* The refinement mode in effect for the current HIP device (0 if never set; 2 after
 * srbd_set_refinement_policy). */
int srbd_get_refinement(void);

/* Diagnostics (A/B campaigns, scripts/parity_fuzz.py): an explicit refinement policy for the register
 * kernels on the current device, in place of the mode. flags: SRBD_REFINE_AFFINE_ALL (the affine
 * direction in every iteration), SRBD_REFINE_AFFINE_AT_INIT (at an iterate whose duals z are all 1: the
 * initial iterate of the GPU caller's and of the _ccs init), SRBD_REFINE_AFFINE_FIRST(k) /
 * SRBD_REFINE_AFFINE_LAST(k) (in the first / last k iterations of a call -- position-based: chained calls
 * then no longer equal one long call); w: the affine vote's W = z / s threshold (w <= 0: no W vote; an s
 * at its clamp always votes). Mode 0 is SRBD_REFINE_AFFINE_AT_INIT with w = 1e4, mode 1
 * SRBD_REFINE_AFFINE_ALL. The
 * combined direction is refined in every iteration whatever the policy. srbd_set_refinement(mode)
 * returns to a mode. Returns 0, or an error for unknown bits or a NaN threshold. */
#define SRBD_REFINE_AFFINE_ALL 1
#define SRBD_REFINE_AFFINE_AT_INIT 2
#define SRBD_REFINE_AFFINE_FIRST(k) (((k) & 255) << 8)
#define SRBD_REFINE_AFFINE_LAST(k) (((k) & 255) << 16)
int srbd_set_refinement_policy(int flags, double w);

/* Allocates what the solver entry points keep per device -- the general-fallback scratch pool of the
 * stage-invariant kernels (one slot per resident workgroup -- 2048 on an MI355X of
 * srbd_scratch_slot_bytes() = 162,000 B each: 332 MB of HBM per process and device, lock words
 * included) -- on the current HIP
 * device, synchronising it. Optional: the first srbd_pdipm* / srbd_mpc_solve* / evaluate call on a
 * device does the same, but that first call must then not be made inside a stream capture (it returns
 * an error there): call this, or make one ordinary call, before capturing a graph. Returns 0 or an
 * error code. (The pool's lock words are released by the workgroups that take them; a kernel that
 * faults leaves the HIP context unusable anyway.) */
int srbd_prepare_device(void);

/* Frees the current device's scratch pool after synchronising the device (the next solver call, or
 * srbd_prepare_device, allocates it again). Graphs captured before still hold the old pool's address:
 * do not replay them afterwards. Returns 0 or an error code. */
int srbd_release_device(void);

/* Caps the current device's pool at `slots` (>= 1; 0 = the default, one per resident workgroup) for
 * processes that share a GPU; the environment variable SRBD_SCRATCH_SLOTS does the same when no cap
 * is set. Any count >= 1 is correct: a QP that is not stage-invariant and finds every slot taken
 * waits for one. A pool of another size is released (device synchronised) and re-allocated on the
 * next call. */
int srbd_set_scratch_slots(int slots);

/* Bytes / slots of the current device's pool (0 before it is allocated), and the bytes of one slot
 * (host-only: no device needed). */
size_t srbd_scratch_pool_bytes(void);
int srbd_scratch_pool_slots(void);
size_t srbd_scratch_slot_bytes(void);

/* Host-only introspection: rebuild the CCS pattern of H (which = 0), A (1) or G (2) from the very
 * offset maps the kernels use to address A_val/G_val. colptr has 24*horizon+1 entries, rowind nnz.
 * Returns nnz, or a negative value if the kernel's offsets are not a bijection onto a sorted CCS. */
int srbd_pattern_ccs(int horizon, int which, int* colptr, int* rowind);

/* ---- MPC step around the QP ------------------------ */

/* Everything BaseMPCController / MPCControllerCusadi assemble on the host before qp_former, as
 * device arrays (float32 unless noted, batch-major). Field groups mirror the reference data
 * classes: StateEStimatorData and DesiredStateData (core/data/robot_data.py:9-60), the controller's
 * own knot-point state (base_controller.py:48,71-72), GaitGenerator (gait_generator.py:4-76) and
 * MPCConf / the robot model (configuration.py:23-57, core/robot/hector.py:33-38). */
typedef struct srbd_mpc_prep {
  const float* root_euler;                 /* (B,3) */
  const float* root_position;              /* (B,3) */
  const float* root_angular_velocity_w;    /* (B,3) */
  const float* root_velocity_w;            /* (B,3) */
  const float* rotation_body;              /* (B,3,3) row-major */
  const float* foot_position;              /* (B,2,3) world frame, [left, right] */
  const float* desired_velocity_b;         /* (B,3) */
  const float* desired_angular_velocity_b; /* (B,3) */
  const float* desired_height;             /* (B) */
  float* world_position_desired;           /* (B,3) read + updated */
  float* yaw_desired;                      /* (B)   read + updated */
  unsigned char* first_run;                /* (B)   bool, read + cleared */
  const float* gait_phase;                 /* (B) or NULL: then contact_table is used */
  const int* ssp_durations;                /* (B,2) int32 [left, right] */
  const int* dsp_durations;                /* (B,2) int32 */
  const float* contact_table;              /* (B,N,2), used when gait_phase == NULL */
  const float* dt_mpc;                     /* (B) */
  const float* residual_lin_accel;         /* (B,3) */
  const float* residual_ang_accel;         /* (B,3) */
  float I_body[9];                         /* host constants: body inertia (row-major) */
  double mass, mu;
  float Q[13];                             /* MPCConf.Q (13 entries in the reference config) */
  int q_len;                               /* 12 or 13 */
  float R[12];
  float step_dt;                           /* float32(decimation * dt) */
  int literal_layout;                      /* 1 = the reference GPU caller's flattening of R_body,
                                              contact_table and Q;
                                              0 = corrected layout */
} srbd_mpc_prep;

/* Replaces compute_knot_points + set_initial_state + compute_reference_trajectory
 * (base_controller.py:166-257), GaitGenerator.mpc_gait (gait_generator.py:216-252) and the input
 * assembly of MPCControllerCusadi.run (mpc_controller_cusadi.py:54-95): writes the 17 qp_former
 * inputs (FP64, (B, nnz_in[i]), Q well-formed 12 wide) and updates the knot-point state. */
int srbd_prepare_inputs(int horizon, int batch, const srbd_mpc_prep* prep, double* const* former_inputs,
                        void* stream);

/* The whole controller step in ONE kernel launch (any horizon 1..32): srbd_prepare_inputs' arithmetic
 * computes this env's 17 former inputs into on-chip memory (and advances the knot-point state in
 * prep), the fused former + cold PDIPM (n_iter iterations, y = y0) solves, and
 * srbd_u0_wrench_torque's arithmetic writes foot_wrench (B,2,6) float32 -- and tau (B,2,ndof) when
 * tau != NULL, from contact_jacobian (B,2,6,ndof) / contact_bool (B,2). former_inputs (host array
 * of 17 device pointers as srbd_prepare_inputs) may be NULL: the prepared inputs then never leave
 * the chip. outputs (host array of 6 device pointers as srbd_pdipm) may be NULL, and each entry
 * may be NULL: the step then writes only the wrench (48 B/env). Bit-identical to srbd_prepare_inputs -> srbd_mpc_solve_fused ->
 * srbd_u0_wrench_torque. Replaces MPCControllerCusadi.run (mpc_controller_cusadi.py:43-205) with
 * BaseMPCController's preparation (base_controller.py:166-257) and LegController.update_ff_torque
 * (leg_controller.py:87-95). */
int srbd_mpc_step(int horizon, int n_iter, int batch, double y0, const srbd_mpc_prep* prep,
                  double* const* former_inputs, double* const* outputs, float* foot_wrench, int ndof,
                  const float* contact_jacobian, const float* contact_bool, float* tau, void* stream);
/* srbd_mpc_step with the status word (status may be NULL). */
int srbd_mpc_step_ex(int horizon, int n_iter, int batch, double y0, const srbd_mpc_prep* prep,
                     double* const* former_inputs, double* const* outputs, float* foot_wrench, int ndof,
                     const float* contact_jacobian, const float* contact_bool, float* tau, int* status,
                     void* stream);
/* srbd_mpc_step with the extras struct (info may be NULL): with objective_f32 the step writes the MPC
 * cost next to the wrench, 4 more bytes per env. */
int srbd_mpc_step_info(int horizon, int n_iter, int batch, double y0, const srbd_mpc_prep* prep,
                       double* const* former_inputs, double* const* outputs, float* foot_wrench, int ndof,
                       const float* contact_jacobian, const float* contact_bool, float* tau,
                       const srbd_solve_info* info, void* stream);

/* u0 = x[:, 12N:12N+12] -> foot wrench (B,2,6) float32 in the body frame, x-moments zeroed and
 * negated as mpc_controller_cusadi.py:186-203. rotation_body (B,3,3) float32 row-major. */
int srbd_u0_wrench(int horizon, int batch, const double* x, const float* rotation_body, float* foot_wrench,
                   void* stream);

/* srbd_u0_wrench plus the stance feed-forward joint torque of LegController.update_ff_torque
 * (leg_controller.py:87-95; fed by BipedController._run_stance_leg_controller,
 * biped_controller.py:144-146): tau (B,2,ndof) float32 = contact_bool[b,l] != 0 ? J[b,l]^T wrench[b,l]
 * : 0, with contact_jacobian (B,2,6,ndof) and contact_bool (B,2) float32. tau == NULL skips it. */
int srbd_u0_wrench_torque(int horizon, int batch, const double* x, const float* rotation_body, float* foot_wrench,
                          int ndof, const float* contact_jacobian, const float* contact_bool, float* tau,
                          void* stream);

/* CusadiFunction.getDenseOutput (CusadiFunction.py:49-58) as one scatter: dense (B, rc) row-major
 * from nonzeros (B, nnz) through inverse_index[rc] (nonzero index of each dense entry, or -1). */
int srbd_dense_scatter(int batch, int nnz, int rc, const int* inverse_index, const double* values,
                       double* dense, void* stream);

/* ---- Backward pass: gradients of a loss on a solve's outputs through the QP solve and the former -----
 * The iterate (x, s, z, y) a solve returned is read as a root of the solver's regularised KKT
 * conditions; their Newton matrix K is symmetric, so one solve of
 *   K [lx; ls; lz; ly] = [grad_x; 0; 0; 0]
 * (one factorisation, one solve, one refinement step, the forward LDS-resident kernel's phases) gives
 * every gradient. At a non-converged iterate this is the exact derivative of the linearised KKT
 * conditions at that iterate (qpth's convention). The entries named *_seeds below take cotangents of
 * every output of a solve -- x, s, z, y and the objective -- as the right-hand side of the same K; the
 * others take grad_x alone and are those entries with one cotangent. All entry points: host arrays of device pointers, asynchronous on `stream`, no device
 * allocation (capture-safe after srbd_prepare_device), batch == 0 and bad arguments return without
 * touching the GPU, errors through srbd_last_error().
 *
 * Status bit of the backward entry points: the QP is not stage-invariant (any CCS input other than
 * qp_former's output). Such a QP is not differentiated: its gradients are NaN. SRBD_STATUS_NONFINITE
 * reports a NaN / Inf in the adjoint of a QP that was solved. */
#define SRBD_STATUS_UNSUPPORTED 8

/* inputs: srbd_pdipm's ten, in its order (Q_val, G_val, A_val, f, h, b, x, s, z, y); f, h, b are not
 * read here and may be NULL. grad_x (B, 24N) = dL/dx. qp_grads: six outputs in qp_former's output order and
 * CCS widths, each skipped when NULL (asking for a subset changes no bit of the others):
 *   grad_H (24N)       -lx[c] x[c]                      grad_f (24N)  -lx
 *   grad_A (122N-24)   -(lx[c] y[r] + ly[r] x[c])       grad_b (14N)   ly
 *   grad_G (28N)       -(lx[c] z[r] + lz[r] x[c])       grad_d (16N)   lz
 * Every CCS nonzero is its own parameter (nothing is summed over stages). status (B ints) may be NULL.
 * An env's gradients have the same bits at any batch size and position. Horizons 1..32. */
int srbd_pdipm_backward(int horizon, int batch, const double* const* inputs, const double* grad_x,
                        double* const* qp_grads, int* status, void* stream);

/* The vector-Jacobian product of srbd_qp_former: qp_grads (six, qp_former's output order; NULL = a zero
 * gradient) -> input_grads (17, the former inputs' order and widths; NULL = not written). The gradients
 * of x and u (inputs 1 and 2) are zero: the model is affine, so the QP does not depend on the
 * linearisation point. R_body and I_world are decoded column-major, as the former reads them. */
int srbd_qp_former_backward(int horizon, int batch, const double* const* former_inputs,
                            const double* const* qp_grads, double* const* input_grads, void* stream);

/* srbd_qp_former -> srbd_pdipm_backward -> srbd_qp_former_backward in one call (same bits): the QP and
 * its gradients go to `workspace`, caller-owned device memory of
 * srbd_mpc_backward_workspace_doubles(horizon, batch) doubles. That size (the QP and all six gradients)
 * is an upper bound: only the gradients that the non-NULL input_grads read are materialised, as in
 * srbd_mpc_backward_multi. All 17 input_grads may be NULL here: only `status` is written then.
 * iterate: x, s, z, y of the solve. */
size_t srbd_mpc_backward_workspace_doubles(int horizon, int batch);
int srbd_mpc_backward(int horizon, int batch, const double* const* former_inputs,
                      const double* const* iterate /* x, s, z, y */, const double* grad_x,
                      double* workspace, double* const* input_grads, int* status, void* stream);

/* ---- Several seeds at one iterate: solution Jacobians and the u0 feedback gain ----------------------
 * K depends on the QP and the iterate only, so n_seeds = M seeds g_0 .. g_{M-1} on x share the load, the
 * stage-invariance check and the factorisation: one factorisation and M solves (each with its refinement
 * step) in one launch. n_seeds = 1 is srbd_pdipm_backward, and seed k's results have the bits of a call
 * with g_k alone. The result is, as there, the derivative of the linearised KKT conditions at the iterate: exact at
 * convergence. Conventions as the entry points above (host arrays of device pointers, asynchronous, no
 * device allocation, batch == 0 returns 0 and bad arguments an error code without touching the GPU).
 * Bad arguments: horizon outside 1..32, n_seeds < 1, a stride that is neither 0 nor n_seeds * 24N, a
 * null required pointer, batch * n_seeds above INT_MAX. All row offsets are size_t.
 *
 * grad_x: seed k of env e at grad_x + e * grad_x_env_stride + k * 24N doubles. Stride 0: one (M, 24N)
 * block shared by every env (unit seeds never need a (B, M, 24N) tensor); stride M * 24N: a (B, M, 24N)
 * tensor. qp_grads: six outputs (B, M, width), row e * M + k, each skipped when NULL. A QP that is not
 * stage-invariant gets NaN in its M rows and SRBD_STATUS_UNSUPPORTED; SRBD_STATUS_NONFINITE reports a
 * non-finite adjoint of any of its seeds. status (B ints) may be NULL. */
int srbd_pdipm_backward_multi(int horizon, int batch, int n_seeds, const double* const* inputs,
                              const double* grad_x, size_t grad_x_env_stride /* 0 or n_seeds*24N */,
                              double* const* qp_grads /* each (B, M, width) or NULL */, int* status, void* stream);

/* srbd_qp_former_backward over seed rows: qp_grads and input_grads hold B * M rows, row r uses the
 * former inputs of env r / M (former_inputs: B rows). n_seeds = 1 is srbd_qp_former_backward. */
int srbd_qp_former_backward_multi(int horizon, int batch, int n_seeds, const double* const* former_inputs /* B rows */,
                                  const double* const* qp_grads /* B*M rows, NULL = zero */,
                                  double* const* input_grads /* B*M rows, NULL = skipped */, void* stream);

/* Host-only: which QP gradients the gradient of former input `input` (0..16) reads, as a mask with bit
 * 0..5 = grad_H, grad_f, grad_A, grad_b, grad_G, grad_d (0 for inputs 1 and 2, whose gradient is zero,
 * and for an index out of range):
 *   x0 <- b;  x_ref <- f;  Q <- H, f;  R <- H;  contact_table <- d;  mu <- G;
 *   dt, m, R_body, I_world, the three positions, the two residual accelerations <- A, b. */
unsigned srbd_former_grad_deps(int input);

/* srbd_qp_former (once per env) -> srbd_pdipm_backward_multi -> srbd_qp_former_backward_multi in one call
 * (same bits). Only the QP gradients that the requested inputs (non-NULL input_grads entries; at least
 * one) read are materialised: the others are NULL to both kernels. workspace: the QP, then those
 * gradients (B, M, width) -- srbd_mpc_backward_multi_workspace_doubles doubles, input_mask bit i = former
 * input i requested (0 = all 17; 0 doubles for bad arguments). For the gain (x0 only) at N = 10, M = 12:
 * the QP plus 12 * 140 doubles per env. */
size_t srbd_mpc_backward_multi_workspace_doubles(int horizon, int batch, int n_seeds, unsigned input_mask /* 0 = all 17 */);
int srbd_mpc_backward_multi(int horizon, int batch, int n_seeds, const double* const* former_inputs,
                            const double* const* iterate, const double* grad_x, size_t grad_x_env_stride,
                            double* workspace, double* const* input_grads, int* status, void* stream);

/* ---- Seeds on every output of a solve: x, s, z, y and the objective -----------------------------------
 * A solve returns x, the slacks s = d - G x (the friction-cone and force-limit margins), the multipliers z
 * and y, and on request the objective J = 1/2 x^T H x + f^T x (the MPC cost). With cotangents g_x, g_s,
 * g_z, g_y, g_J of a loss, the adjoint is the solution of the same symmetric K with the full right-hand side
 *   K [lx; ls; lz; ly] = [g_x + g_J (H o x + f); g_s; g_z; g_y],
 * the six gradient formulas of srbd_pdipm_backward hold unchanged (ls enters none of them), and J's explicit
 * dependence on the data adds g_J (1/2 x[c] x[c]) to grad_H[c] and g_J x[c] to grad_f[c] (when those are
 * written). One factorisation, and per seed one solve and one refinement step, as above. A NULL cotangent is
 * zero: with grad_x alone an entry gives the bits of its x-only counterpart, and a NULL array gives what an
 * all-zero one gives. All five NULL is a bad argument. f (solver input 3) is read only with grad_objective
 * and is required then.
 *
 * Each given array holds one row per seed, of its width: row e * n_seeds + k for seed k of env e (B * M
 * rows), or with `shared` row k for every env (M rows; unit seeds of a Jacobian). n_seeds = 1, shared = 0 is
 * one seed per env. Outputs, status words and conventions as srbd_pdipm_backward_multi. */
typedef struct srbd_backward_seeds {
  const double *grad_x, *grad_s, *grad_z, *grad_y; /* widths 24N, 16N, 16N, 14N; NULL = zero */
  const double* grad_objective;                    /* width 1; NULL = zero */
  int shared; /* 0: each array holds B*M rows, row e*M+k; 1: M rows shared by every env */
} srbd_backward_seeds;

int srbd_pdipm_backward_seeds(int horizon, int batch, int n_seeds, const double* const* inputs,
                              const srbd_backward_seeds* seeds, double* const* qp_grads, int* status,
                              void* stream);
/* srbd_qp_former -> srbd_pdipm_backward_seeds -> srbd_qp_former_backward_multi in one call (same bits); the
 * former's QP in the workspace supplies f. workspace: srbd_mpc_backward_multi_workspace_doubles doubles. All
 * 17 input_grads may be NULL: only `status` is written then. */
int srbd_mpc_backward_seeds(int horizon, int batch, int n_seeds, const double* const* former_inputs,
                            const double* const* iterate, const srbd_backward_seeds* seeds, double* workspace,
                            double* const* input_grads, int* status, void* stream);

/* ---- Backward pass of the controller step: wrench cotangent -> the controller's FP32 tensors ---------
 * srbd_mpc_step maps the FP32 tensors of srbd_mpc_prep to the FP32 foot wrench (and stance torque). The
 * entries above differentiate its middle, the QP, in FP64 coordinates; the two below differentiate its
 * FP32 ends, and srbd_mpc_step_backward chains all three. Conventions as above: host arrays of device
 * pointers, asynchronous on `stream`, no device allocation, batch == 0 returns 0, bad arguments return an
 * error code and a srbd_last_error() message without touching the GPU.
 *
 * Arithmetic: the forward's FP32 values are widened to FP64; products and sums are FP64, not contracted,
 * in a fixed order per entry; a gradient on an FP32 tensor is rounded once, at its store. The forward's
 * selects (first_run, the stationary test |v_x| < 1e-2) are constants of the derivative. An env's
 * gradients have the same bits at any batch size and position. */

/* The VJP of srbd_u0_wrench_torque. x (B,24N) the solution, rotation_body (B,3,3) float32, grad_wrench
 * (B,2,6) float32; grad_tau (B,2,ndof) float32 is optional and needs contact_jacobian, contact_bool and
 * ndof in 1..64. Writes grad_x (B,24N) FP64 -- the whole row: zeros outside the u0 block [12N, 12N+12)
 * and at its entries 6 and 9, which the forward zeroes -- and, when non-NULL, grad_rotation_body (B,9)
 * FP64, the wrench's direct dependence on rotation_body. */
int srbd_u0_wrench_backward(int horizon, int batch, const double* x, const float* rotation_body,
                            const float* grad_wrench, int ndof, const float* contact_jacobian,
                            const float* contact_bool, const float* grad_tau, double* grad_x,
                            double* grad_rotation_body, void* stream);

/* Indices of the 15 gradients of srbd_prepare_inputs_backward (prep_grads): the FP32 tensors of
 * srbd_mpc_prep, each with its tensor's shape. */
#define SRBD_PREP_GRAD_ROOT_EULER 0
#define SRBD_PREP_GRAD_ROOT_POSITION 1
#define SRBD_PREP_GRAD_ROOT_ANGULAR_VELOCITY_W 2
#define SRBD_PREP_GRAD_ROOT_VELOCITY_W 3
#define SRBD_PREP_GRAD_ROTATION_BODY 4
#define SRBD_PREP_GRAD_FOOT_POSITION 5
#define SRBD_PREP_GRAD_DESIRED_VELOCITY_B 6
#define SRBD_PREP_GRAD_DESIRED_ANGULAR_VELOCITY_B 7
#define SRBD_PREP_GRAD_DESIRED_HEIGHT 8
#define SRBD_PREP_GRAD_WORLD_POSITION_DESIRED 9 /* the value the step read */
#define SRBD_PREP_GRAD_YAW_DESIRED 10           /* the value the step read */
#define SRBD_PREP_GRAD_CONTACT_TABLE 11         /* explicit-table mode only */
#define SRBD_PREP_GRAD_DT_MPC 12
#define SRBD_PREP_GRAD_RESIDUAL_LIN_ACCEL 13
#define SRBD_PREP_GRAD_RESIDUAL_ANG_ACCEL 14
#define SRBD_PREP_GRAD_COUNT 15

/* The VJP of srbd_prepare_inputs: input_grads (17 FP64 cotangents of the former inputs, their order and
 * widths; NULL = zero) -> prep_grads (15 float32 arrays indexed by SRBD_PREP_GRAD_*; NULL = skipped, and
 * skipping changes no bit of the others). grad_wpd_out (B,3) / grad_yaw_out (B) float32, optional: the
 * cotangents of the UPDATED world_position_desired / yaw_desired, for callers that unroll several steps.
 * grad_rotation_body_direct (B,9) FP64, optional: srbd_u0_wrench_backward's, added before the one
 * rounding. `prep` is read only, and only rotation_body, desired_velocity_b, desired_angular_velocity_b,
 * dt_mpc, first_run, gait_phase (as a mode flag), I_body, step_dt and literal_layout of it (the other
 * arrays may be NULL: the map is linear in them); first_run is the flag as it was BEFORE the forward
 * step. With x_ref's cotangent gx[k,j] = input_grads[3][12k+j], S_j = sum_k gx[k,j], T_j = sum_k k gx[k,j]:
 * dt_mpc gets g_4 + wz T_2 + vw0 T_3 + vw1 T_4, the residual accelerations g_15 and g_16, rotation_body
 * the terms of vw = R v_b, R_body, I_world = R I_body R^T and the direct one (DESIGN.md 6c has the table).
 * The contact_table gradient is refused (bad arguments) when prep->gait_phase != NULL: the schedule then
 * comes from the gait phase, which is piecewise constant. */
int srbd_prepare_inputs_backward(int horizon, int batch, const srbd_mpc_prep* prep,
                                 const double* const* input_grads /* 17, NULL entry = zero */,
                                 const float* grad_wpd_out, const float* grad_yaw_out,
                                 const double* grad_rotation_body_direct,
                                 float* const* prep_grads /* 15, NULL entry = skipped */, void* stream);

/* Host-only: which former-input cotangents prep gradient `field` (SRBD_PREP_GRAD_*) reads, as a mask with
 * bit i = former input i (0 for an index out of range):
 *   root_euler <- 0, 3;  root_position <- 0, 3, 9;  the two root velocities <- 0;  rotation_body <- 3, 7, 8;
 *   foot_position <- 10, 11;  the three command tensors and the two knot-point tensors <- 3;
 *   contact_table <- 12;  dt_mpc <- 3, 4;  residual_lin_accel <- 15;  residual_ang_accel <- 16. */
unsigned srbd_prep_grad_deps(int field);

/* srbd_u0_wrench_backward -> srbd_mpc_backward -> srbd_prepare_inputs_backward in one call (same bits).
 * srbd_mpc_backward is asked for only the former inputs that the requested prep gradients (non-NULL
 * prep_grads entries; at least one) read. former_inputs and iterate (x, s, z, y) are what the step wrote
 * (srbd_mpc_step with former_inputs and outputs); rotation_body is prep's. status (B ints, may be NULL)
 * is the adjoint's. workspace: caller-owned device memory of srbd_mpc_step_backward_workspace_doubles
 * doubles, prep_mask bit f = prep gradient f requested (0 = all 15; 0 doubles for bad arguments): the seed
 * grad_x (B,24N), the direct rotation_body term (B,9), the former-input cotangents the requested prep
 * gradients read, then srbd_mpc_backward_multi_workspace_doubles(horizon, batch, 1, those inputs). */
size_t srbd_mpc_step_backward_workspace_doubles(int horizon, int batch, unsigned prep_mask /* 0 = all 15 */);
int srbd_mpc_step_backward(int horizon, int batch, const srbd_mpc_prep* prep, const double* const* former_inputs,
                           const double* const* iterate /* x, s, z, y */, const float* grad_wrench, int ndof,
                           const float* contact_jacobian, const float* contact_bool, const float* grad_tau,
                           const float* grad_wpd_out, const float* grad_yaw_out, double* workspace,
                           float* const* prep_grads, int* status, void* stream);

/* srbd_mpc_step_backward with the cotangent of the step's MPC cost: grad_cost (B) float32 is the cotangent
 * of objective_f32 (srbd_mpc_step_info). It is widened to FP64 and enters the adjoint as grad_objective; the
 * one rounding of J to float32 is read as the identity. grad_wrench may be NULL when grad_cost is not (and
 * grad_tau must then be NULL); with grad_cost NULL this is srbd_mpc_step_backward. The workspace is that
 * entry's, laid out alike, plus the widened cotangent (B doubles) behind it. */
size_t srbd_mpc_step_backward_cost_workspace_doubles(int horizon, int batch, unsigned prep_mask /* 0 = all 15 */);
int srbd_mpc_step_backward_cost(int horizon, int batch, const srbd_mpc_prep* prep,
                                const double* const* former_inputs, const double* const* iterate /* x, s, z, y */,
                                const float* grad_wrench, const float* grad_cost, int ndof,
                                const float* contact_jacobian, const float* contact_bool, const float* grad_tau,
                                const float* grad_wpd_out, const float* grad_yaw_out, double* workspace,
                                float* const* prep_grads, int* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SRBD_MPC_H_ */
