// srbd_mpc.hip -- libsrbd_mpc.so: HIP kernels (gfx950) + the C-ABI of include/srbd_mpc.h.
//
// The main translation unit; the register kernels at the horizons other than 10 are built apart in
// srbd_reg20.hip and srbd_regN.hip, the backward kernels in srbd_backward.hip. The constant-memory
// tables (srbd_common.hpp) are compile-time initialised, so each unit's copy is identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/srbd_mpc.h"
#include "pdipm.hpp"
#include "pdipm_srbd.hpp"
#include "pdipm_srbd_reg.hpp"
#include "mpc_step_lds.hpp"
#include "qp_former.hpp"
#include "mpc_io.hpp"
#include "reg20.hpp"
#include "regN.hpp"
#include "device_state.hpp"
#include "pdipm_backward.hpp"      // BackwardArgs; the kernels are instantiated in srbd_backward.hip
#include "qp_former_backward.hpp"  // FormerBackwardArgs

static_assert(srbd::kStatusUnsupported == SRBD_STATUS_UNSUPPORTED, "status bits of the header and the kernels");

#ifndef SRBD_BUILD_ID
#define SRBD_BUILD_ID "0000000000000000"  // diagnostic builds outside biped_pympc_amd/build.py
#endif

namespace {

// "srbd-build-id:" + the 16-hex source hash (build.py source_hash); build.py reads it from the file
__attribute__((used)) const char kBuildIdTag[] = "srbd-build-id:" SRBD_BUILD_ID;

thread_local std::string g_last_error;

int set_error(int code, const char* what) {
  char buf[512];
  std::snprintf(buf, sizeof(buf), "%s (code %d: %s)", what, code,
                code > 0 ? hipGetErrorString((hipError_t)code) : "invalid argument");
  g_last_error = buf;
  return code;
}

constexpr int kFormerWaves = 4;
constexpr int kErrInvalid = (int)hipErrorInvalidValue;
// general solves of non-stage-invariant QPs in flight per device: one slot per workgroup the device
// can hold resident of any stage-invariant kernel (at most 8 QPs per CU: the N <= 10 register kernels)
constexpr int kMaxQpsPerCu = 8;

// an argument the entry `what` rejects: "<what>: <msg>"
int fail(const char* what, const char* msg) { return set_error(kErrInvalid, (std::string(what) + ": " + msg).c_str()); }

// no HIP device is current, or its index is past the per-device state: as the setter `what` reports it,
// or (null) as a launch does on behalf of any entry
int no_device(const char* what = nullptr) {
  const std::string msg = what ? std::string(what) + ": no current HIP device" : "no current HIP device (or index >= 64)";
  return set_error((int)hipErrorInvalidDevice, msg.c_str());
}

// the result of the launch just enqueued; `what` names its kernel ("<kernel> launch")
int launched(const char* what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : set_error((int)e, what);
}

// the n device pointers of a caller's table into kernel arguments; a null one is the entry's "<what>: <msg>"
template <class Dst, class Src>
int copy_pointers(const char* what, const char* msg, Dst* dst, Src* const* src, int n) {
  for (int i = 0; i < n; ++i) {
    if (!src[i]) return fail(what, msg);
    dst[i] = src[i];
  }
  return 0;
}

bool horizon_ok(int N) { return N >= 1 && N <= srbd::kMaxN; }

// The six arrays of a QP as the former writes them -- H, f, A, b, G, d -- and how a workspace of a batch
// of them is laid out: array after array, each (rows, width).
struct QpLayout {
  size_t width[6];  // doubles per QP
  explicit QpLayout(int horizon) {
    const size_t N = (size_t)horizon;
    const size_t w[6] = {24 * N, 24 * N, 122 * N - 24, 14 * N, 28 * N, 16 * N};
    std::copy(w, w + 6, width);
  }
  // doubles of `rows` rows of every array in `mask` (bit i = array i)
  size_t doubles(size_t rows = 1, unsigned mask = 63u) const {
    size_t n = 0;
    for (int i = 0; i < 6; ++i)
      if (mask >> i & 1u) n += rows * width[i];
    return n;
  }
  // slot[i] = the next `rows` rows of array i at `p`, which moves past them; null for an array not in `mask`
  void carve(double*& p, size_t rows, double* (&slot)[6], unsigned mask = 63u) const {
    for (int i = 0; i < 6; ++i) {
      slot[i] = (mask >> i & 1u) ? p : nullptr;
      if (slot[i]) p += rows * width[i];
    }
  }
};

// the former's six arrays in the solver's input order H, G, A, f, d, b: its input slots 0..5
void solver_order(double* const (&qp)[6], const double* (&in)[10]) {
  constexpr int kFormerSlot[6] = {0, 4, 2, 1, 5, 3};
  for (int i = 0; i < 6; ++i) in[i] = qp[kFormerSlot[i]];
}

size_t solver_lds_bytes(int N) { return sizeof(double) * (size_t)srbd::SolverLayout(N).total; }
size_t fast_lds_bytes(int N) { return sizeof(double) * (size_t)srbd::FastLayout(N).total; }
constexpr size_t kRegLds10 = sizeof(double) * (size_t)srbd::RegLayout<10>::total;
constexpr size_t kRegLds20 = sizeof(double) * (size_t)srbd::RegLayout<20>::total;
// the register kernels' LDS is static (RegLayout<N>::total doubles per workgroup)
static_assert(kRegLds10 <= 20 * 1024, "N=10 register kernel must fit 8 QPs per CU");
static_assert(kRegLds20 <= 40 * 1024, "N=20 register kernel must fit 4 QPs per CU");

// The HIP device current at this call (-1 if none / out of range for the per-device state)
int current_device() {
  int d = -1;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= srbd::kMaxDevices) return -1;
  return d;
}

// Solver path per device: 0 = auto (stage-invariant kernels -- register-resident for N = 10 and 20,
// LDS-resident otherwise -- and the general kernel for flagged QPs); 1 = general kernel only;
// 2 = LDS-resident fast kernel. Selected by srbd_set_solver_path for the current device.
srbd::PerDevice<int> g_solver_path;
int solver_path() {
  const int* p = g_solver_path.at(current_device());
  return p ? *p : 0;
}

// Refinement policy per device (srbd_set_refinement / srbd_set_refinement_policy). Mode 0 (default):
// the affine direction at a solve's initial iterate and on ill-conditioned iterates (the policy word
// below), the combined one in every iteration; mode 1: both in every iteration; mode 2: a policy word set
// by srbd_set_refinement_policy. Read by the register kernels only (the LDS-resident and general kernels
// refine both directions in every iteration).
struct RefinePolicy {
  int mode = 0;
  int flags = 0;
  double w = 0.0;
};
// mode 0's policy: the predictor at a solve's initial iterate (all z = 1) and in every iteration with
// z / s >= 1e4 in some row (round 6, DESIGN.md 3.3: with correctly rounded reciprocals, about round 5's
// N = 10 time for 23 -> 4 failing _ccs-campaign cases of 6657)
constexpr int kDefaultRefineFlags = SRBD_REFINE_AFFINE_AT_INIT;
constexpr double kDefaultRefineW = 1e4;
srbd::PerDevice<RefinePolicy> g_refinement;
int refinement_mode() {
  const RefinePolicy* p = g_refinement.at(current_device());
  return p ? p->mode : 0;
}
// the kernel arguments of the policy in effect: the word and the W threshold
template <class Args>
void set_refinement_args(Args& a) {
  const RefinePolicy* p = g_refinement.at(current_device());
  const int mode = p ? p->mode : 0;
  a.refine_policy = mode == 2 ? p->flags : (mode == 1 ? SRBD_REFINE_AFFINE_ALL : kDefaultRefineFlags);
  const double w = mode == 2 ? p->w : kDefaultRefineW;
  a.refine_w = w > 0.0 ? w : INFINITY;
}

// the per-problem extras of a call (srbd_solve_info, any of them or the struct itself null) into the
// kernel arguments
template <class Args>
void set_info_args(Args& a, const srbd_solve_info* info) {
  a.status = info ? info->status : nullptr;
  a.objective = info ? info->objective : nullptr;
  a.objective_f32 = info ? info->objective_f32 : nullptr;
}
srbd_solve_info status_only(int* status) { return srbd_solve_info{status, nullptr, nullptr}; }

// A kernel taking Args that keeps its problem in dynamic LDS, and the largest size configured for it per
// device. A kernel of this unit gives Args itself; one of another unit comes as the handle its unit
// exports, with Args named where the LdsKernel is declared.
template <class Args>
struct LdsKernel {
  const void* fn;
  const char* what;       // "<kernel> launch"
  const char* too_large;  // the message for a horizon whose problem does not fit a workgroup's LDS
  srbd::LdsAttr cfg{};
  LdsKernel(void (*kernel)(Args), const char* what, const char* too_large)
      : fn((const void*)kernel), what(what), too_large(too_large) {}
  LdsKernel(const void* handle, const char* what, const char* too_large)
      : fn(handle), what(what), too_large(too_large) {}
};

// Launch of such a kernel, one workgroup of `threads` per problem of a.batch, with `lds` bytes: the
// 160 KiB a workgroup can have, the kernel's attribute on the current device (set when `lds` exceeds
// what was configured there), the launch and its result.
template <class Args>
int launch_dynamic_lds(LdsKernel<Args>& k, int threads, size_t lds, const Args& a, hipStream_t s) {
  if (lds > 160 * 1024) return set_error(kErrInvalid, k.too_large);
  const int dev = current_device();
  if (dev < 0) return no_device();
  if (k.cfg.claim(dev, lds)) {
    hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_error((int)e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    k.cfg.commit(dev, lds);
  }
  void* argv[] = {const_cast<Args*>(&a)};
  (void)hipLaunchKernel(k.fn, dim3(a.batch), dim3(threads), argv, lds, s);
  return launched(k.what);
}

int launch_former(const srbd::FormerArgs& a, hipStream_t s) {
  if (a.batch == 0) return 0;
  const int grid = (a.batch + kFormerWaves - 1) / kFormerWaves;
  hipLaunchKernelGGL(srbd::qp_former_kernel<kFormerWaves>, dim3(grid), dim3(64 * kFormerWaves), 0, s, a);
  return launched("qp_former_kernel launch");
}

// The per-device scratch pool of the stage-invariant solver kernels (pdipm.hpp
// pdipm_general_scratch): CUs x kMaxQpsPerCu slots of general_slot_doubles() (2048 slots of
// srbd_scratch_slot_bytes() = 162,000 B: 332 MB of the 288 GB on an MI355X) and their lock words, one
// per 128-byte line, allocated on the first stage-invariant solver call on a device (or
// srbd_prepare_device) and kept until srbd_release_device. With a slot for every resident workgroup
// no fallback solve waits for another: a batch of QPs that are all not stage-invariant runs at the
// general solve's rate instead of queueing on a few slots. srbd_set_scratch_slots (or the
// SRBD_SCRATCH_SLOTS environment variable, read when the pool is allocated) caps the slot count, for
// processes that share a GPU: a fallback QP that finds every slot taken waits for one (the holders are
// resident workgroups, so they finish), which is correct at any count >= 1, only slower.
struct ScratchPool {
  double* buf = nullptr;
  int* locks = nullptr;
  int slots = 0;
  int stride = 0;  // doubles per slot
};

// doubles one slot needs: the general solve's layout at its largest horizon (not necessarily N = kMaxN:
// the precomputed couplings are dropped where they would not fit 160 KiB of LDS)
int general_slot_doubles() {
  int s = 0;
  for (int n = 1; n <= srbd::kMaxN; ++n) {  // (KX, the last array, is the general kernel's only)
    const srbd::SolverLayout L(n);
    s = std::max(s, L.KX >= 0 ? L.KX : L.total);
  }
  return s;
}
srbd::PerDevice<ScratchPool> g_scratch;
srbd::PerDevice<int> g_scratch_cap;  // srbd_set_scratch_slots per device; 0 = default
std::mutex g_scratch_mu;
// A solver launch holds g_pool_rw shared from attaching the pool to its arguments until the kernel is
// enqueued; srbd_release_device / a resizing srbd_set_scratch_slots take it exclusively before their
// hipDeviceSynchronize, so a pool is never freed between another thread's attach and its launch (the
// kernel would run on freed HBM). Lock order: g_pool_rw, then g_scratch_mu.
std::shared_mutex g_pool_rw;

// slots of a new pool on device `dev` with `cus` compute units
int pool_slots(int dev, int cus) {
  const int* capp = g_scratch_cap.at(dev);
  int cap = capp ? *capp : 0;
  if (cap <= 0)
    if (const char* env = std::getenv("SRBD_SCRATCH_SLOTS")) cap = std::atoi(env);
  return cap > 0 ? std::min(cap, 1 << 16) : cus * kMaxQpsPerCu;
}

// frees the pool of `pool` after the device has drained (g_scratch_mu held)
int release_pool(ScratchPool* pool) {
  if (!pool || !pool->buf) return 0;
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return set_error((int)e, "srbd_release_device: device synchronisation");
  (void)hipFree(pool->buf);
  (void)hipFree(pool->locks);
  *pool = ScratchPool{};
  return 0;
}

// the current device's pool, allocated on first use (`s`: the stream of the calling launch, checked for
// capture; null from srbd_prepare_device)
ScratchPool* scratch_pool(hipStream_t s, bool check_capture, int& rc) {
  rc = 0;
  const int dev = current_device();
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  ScratchPool* pool = g_scratch.at(dev);
  if (!pool) {
    rc = no_device();
    return nullptr;
  }
  if (!pool->buf) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (check_capture && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) {
      rc = set_error(kErrInvalid, "srbd solver: first call on this device inside a stream capture (the "
                                  "scratch pool is allocated on first use: call srbd_prepare_device() first)");
      return nullptr;
    }
    const size_t per_slot = (size_t)general_slot_doubles();
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const int slots = pool_slots(dev, e == hipSuccess && cus > 0 ? cus : 256);
    const size_t lock_ints = (size_t)slots * srbd::kLockStride;
    double* buf = nullptr;
    int* locks = nullptr;
    if (e == hipSuccess) e = hipMalloc(&buf, sizeof(double) * per_slot * slots);
    if (e == hipSuccess) e = hipMalloc(&locks, sizeof(int) * lock_ints);
    if (e == hipSuccess) e = hipMemset(locks, 0, sizeof(int) * lock_ints);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      (void)hipFree(buf);
      (void)hipFree(locks);
      rc = set_error((int)e, "srbd solver: scratch pool allocation");
      return nullptr;
    }
    pool->buf = buf;
    pool->locks = locks;
    pool->slots = slots;
    pool->stride = (int)per_slot;
  }
  return pool;
}

int attach_scratch(srbd::SolverArgs& a, hipStream_t s) {
  int rc = 0;
  ScratchPool* pool = scratch_pool(s, true, rc);
  if (!pool) return rc;
  a.scratch = pool->buf;
  a.scratch_locks = pool->locks;
  a.scratch_slots = pool->slots;
  a.scratch_stride = pool->stride;
  return 0;
}

// Which stage-invariant kernels serve a horizon -- the one place that knows where each is built. The
// register kernels: N = 10 in this unit, N = 20 in srbd_reg20.hip, the other horizons they support in
// srbd_regN.hip; the LDS-resident ones (pdipm_srbd_kernel, mpc_step_lds_kernel) at every other horizon.
enum class Serves { Reg10, Reg20, RegN, Lds };
Serves serves(int N) {
  if (N == 10) return Serves::Reg10;
  if (N == 20) return Serves::Reg20;
  return srbd::regn::supported(N) ? Serves::RegN : Serves::Lds;  // RegN: regn::launch_* has this horizon's case
}

int launch_solver(const srbd::SolverArgs& a0, hipStream_t s) {
  if (a0.batch == 0) return 0;
  constexpr const char* kTooLarge = "horizon too large for the LDS-resident solver";
  static LdsKernel general{srbd::pdipm_kernel, "pdipm_kernel launch", kTooLarge};
  srbd::SolverArgs a = a0;
  set_refinement_args(a);
  const int path = solver_path();
  std::shared_lock<std::shared_mutex> keep_pool(g_pool_rw);  // until the launch is enqueued
  if (path == 1) return launch_dynamic_lds(general, srbd::kGeneralThreads, solver_lds_bytes(a.N), a, s);
  // the stage-invariant kernels solve any other QP of the batch in the same launch (scratch pool)
  if (int rc = attach_scratch(a, s)) return rc;
  switch (path == 2 ? Serves::Lds : serves(a.N)) {  // the register kernels' LDS is static (RegLayout)
    case Serves::Reg10:
      hipLaunchKernelGGL(srbd::pdipm_srbd_reg_kernel<10>, dim3(a.batch), dim3(64), 0, s, a);
      break;
    case Serves::Reg20: srbd::reg20::launch_solver(a, s); break;
    case Serves::RegN: srbd::regn::launch_solver(a.N, a, s); break;
    case Serves::Lds: {  // horizon-specialised instantiations for the common horizons, runtime-N otherwise
      static LdsKernel fast10{srbd::pdipm_srbd_kernel<10>, "pdipm_srbd_kernel launch", kTooLarge};
      static LdsKernel fast20{srbd::pdipm_srbd_kernel<20>, "pdipm_srbd_kernel launch", kTooLarge};
      static LdsKernel fast{srbd::pdipm_srbd_kernel<0>, "pdipm_srbd_kernel launch", kTooLarge};
      return launch_dynamic_lds(a.N == 10 ? fast10 : a.N == 20 ? fast20 : fast, 64, fast_lds_bytes(a.N), a, s);
    }
  }
  return launched("pdipm_srbd_reg_kernel launch");
}

// CusADi-style blocking call on the legacy default stream, timed with hipEvents (one event pair
// per device, created on first use there; the reference creates and leaks two per call).
template <class F>
float timed_blocking(F&& launch) {
  struct Events {
    hipEvent_t ev[2];
  };
  static std::mutex mu;
  static srbd::PerDevice<Events> events;
  std::lock_guard<std::mutex> lock(mu);
  Events* ev = events.at(current_device());
  if (!ev) {
    no_device();
    return -1.0f;
  }
  if (!ev->ev[0]) {
    if (hipEventCreate(&ev->ev[0]) != hipSuccess || hipEventCreate(&ev->ev[1]) != hipSuccess) {
      set_error((int)hipErrorInitializationError, "hipEventCreate");
      return -1.0f;
    }
  }
  (void)hipEventRecord(ev->ev[0], 0);
  if (launch() != 0) return -1.0f;
  (void)hipEventRecord(ev->ev[1], 0);
  hipError_t e = hipEventSynchronize(ev->ev[1]);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    set_error((int)e, "kernel execution");
    return -1.0f;
  }
  float ms = 0.0f;
  (void)hipEventElapsedTime(&ms, ev->ev[0], ev->ev[1]);
  return ms / 1000.0f;
}

}  // namespace

extern "C" {

int srbd_abi_version(void) { return SRBD_ABI_VERSION; }

const char* srbd_build_id(void) { return kBuildIdTag + sizeof("srbd-build-id:") - 1; }

const char* srbd_last_error(void) { return g_last_error.c_str(); }

size_t srbd_solver_lds_bytes(int horizon) { return horizon_ok(horizon) ? solver_lds_bytes(horizon) : 0; }

int srbd_set_solver_path(int path) {
  if (path < 0 || path > 2)
    return set_error(kErrInvalid, "srbd_set_solver_path: 0 (auto), 1 (general) or 2 (LDS-resident fast)");
  int* p = g_solver_path.at(current_device());
  if (!p) return no_device("srbd_set_solver_path");
  *p = path;
  return 0;
}

int srbd_get_solver_path(void) { return solver_path(); }

int srbd_set_refinement(int mode) {
  if (mode < 0 || mode > 1)
    return set_error(kErrInvalid, "srbd_set_refinement: 0 (ill-conditioned iterates) or 1 (every iteration)");
  RefinePolicy* p = g_refinement.at(current_device());
  if (!p) return no_device("srbd_set_refinement");
  *p = RefinePolicy{mode, 0, 0.0};
  return 0;
}

int srbd_set_refinement_policy(int flags, double w) {
  const int known = SRBD_REFINE_AFFINE_ALL | SRBD_REFINE_AFFINE_AT_INIT | SRBD_REFINE_AFFINE_FIRST(255) |
                    SRBD_REFINE_AFFINE_LAST(255);
  if ((flags & ~known) != 0 || w != w)
    return set_error(kErrInvalid, "srbd_set_refinement_policy: unknown policy bits or a NaN threshold");
  RefinePolicy* p = g_refinement.at(current_device());
  if (!p) return no_device("srbd_set_refinement_policy");
  *p = RefinePolicy{2, flags, w};
  return 0;
}

int srbd_get_refinement(void) { return refinement_mode(); }

int srbd_prepare_device(void) {
  int rc = 0;
  return scratch_pool(nullptr, false, rc) ? 0 : rc;
}

int srbd_release_device(void) {
  std::unique_lock<std::shared_mutex> no_launch(g_pool_rw);
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  ScratchPool* pool = g_scratch.at(current_device());
  if (!pool) return no_device("srbd_release_device");
  return release_pool(pool);
}

int srbd_set_scratch_slots(int slots) {
  if (slots < 0) return set_error(kErrInvalid, "srbd_set_scratch_slots: slots >= 0 (0 = one per resident workgroup)");
  std::unique_lock<std::shared_mutex> no_launch(g_pool_rw);
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  const int dev = current_device();
  int* cap = g_scratch_cap.at(dev);
  ScratchPool* pool = g_scratch.at(dev);
  if (!cap || !pool) return no_device("srbd_set_scratch_slots");
  *cap = slots;
  if (pool->buf) {  // re-sized on the next solver call (or srbd_prepare_device)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (pool_slots(dev, cus) != pool->slots) return release_pool(pool);
  }
  return 0;
}

size_t srbd_scratch_pool_bytes(void) {
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  const ScratchPool* pool = g_scratch.at(current_device());
  if (!pool || !pool->buf) return 0;
  return sizeof(double) * (size_t)pool->stride * pool->slots + sizeof(int) * (size_t)pool->slots * srbd::kLockStride;
}

int srbd_scratch_pool_slots(void) {
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  const ScratchPool* pool = g_scratch.at(current_device());
  return pool ? pool->slots : 0;
}

size_t srbd_scratch_slot_bytes(void) { return sizeof(double) * (size_t)general_slot_doubles(); }

size_t srbd_mpc_workspace_doubles(int horizon, int batch) {
  if (!horizon_ok(horizon) || batch < 0) return 0;
  return QpLayout(horizon).doubles((size_t)batch);
}

float srbd_evaluate_qp_former(int horizon, const double* inputs[], double* work, double* outputs[],
                              int batch) {
  (void)work;
  if (!horizon_ok(horizon) || batch < 0 || !inputs || !outputs) {
    set_error(kErrInvalid, "srbd_evaluate_qp_former: bad horizon/batch/pointer table");
    return -1.0f;
  }
  srbd::FormerArgs a{};
  a.dev_in = inputs;
  a.dev_out = outputs;
  a.N = horizon;
  a.batch = batch;
  return timed_blocking([&] { return launch_former(a, 0); });
}

float srbd_evaluate_pdipm(int horizon, int n_iter, const double* inputs[], double* work,
                          double* outputs[], int batch) {
  (void)work;
  if (!horizon_ok(horizon) || n_iter < 1 || batch < 0 || !inputs || !outputs) {
    set_error(kErrInvalid, "srbd_evaluate_pdipm: bad horizon/n_iter/batch/pointer table");
    return -1.0f;
  }
  srbd::SolverArgs a{};
  a.dev_in = inputs;
  a.dev_out = outputs;
  a.N = horizon;
  a.n_iter = n_iter;
  a.batch = batch;
  a.init_mode = 0;
  return timed_blocking([&] { return launch_solver(a, 0); });
}

int srbd_qp_former(int horizon, int batch, const double* const* inputs, double* const* outputs,
                   void* stream) {
  if (!horizon_ok(horizon) || batch < 0 || !inputs || !outputs)
    return set_error(kErrInvalid, "srbd_qp_former: bad arguments");
  if (batch == 0) return 0;  // empty batch: buffers may be null (zero-size allocations)
  srbd::FormerArgs a{};
  if (int rc = copy_pointers("srbd_qp_former", "null input", a.in, inputs, 17)) return rc;
  if (int rc = copy_pointers("srbd_qp_former", "null output", a.out, outputs, 6)) return rc;
  a.N = horizon;
  a.batch = batch;
  return launch_former(a, (hipStream_t)stream);
}

static int pdipm_common(int horizon, int n_iter, int batch, double y0, int init_mode, const double* const* inputs,
                        double* const* outputs, const srbd_solve_info* info, void* stream) {
  if (!horizon_ok(horizon) || n_iter < 1 || batch < 0 || !inputs || !outputs)
    return set_error(kErrInvalid, "srbd_pdipm: bad arguments");
  if (batch == 0) return 0;
  srbd::SolverArgs a{};
  const int nin = init_mode == 0 ? 10 : init_mode == 2 ? 7 : 6;  // QP + iterate / + x_init / QP only
  if (int rc = copy_pointers("srbd_pdipm", "null input", a.in, inputs, nin)) return rc;
  if (int rc = copy_pointers("srbd_pdipm", "null output", a.out, outputs, 6)) return rc;
  a.N = horizon;
  a.n_iter = n_iter;
  a.batch = batch;
  a.init_mode = init_mode;
  a.y0 = y0;
  set_info_args(a, info);
  return launch_solver(a, (hipStream_t)stream);
}

int srbd_pdipm(int horizon, int n_iter, int batch, const double* const* inputs,
               double* const* outputs, void* stream) {
  return pdipm_common(horizon, n_iter, batch, 0.0, 0, inputs, outputs, nullptr, stream);
}

int srbd_pdipm_cold(int horizon, int n_iter, int batch, double y0, const double* const* inputs,
                    double* const* outputs, void* stream) {
  return pdipm_common(horizon, n_iter, batch, y0, 1, inputs, outputs, nullptr, stream);
}

int srbd_pdipm_ccs(int horizon, int n_iter, int batch, const double* const* inputs, double* const* outputs,
                   void* stream) {
  if (!inputs || (batch > 0 && !inputs[6])) return set_error(kErrInvalid, "srbd_pdipm_ccs: null x_init");
  return pdipm_common(horizon, n_iter, batch, 0.0, 2, inputs, outputs, nullptr, stream);
}

int srbd_pdipm_info(int horizon, int n_iter, int batch, int init_mode, double y0, const double* const* inputs,
                    double* const* outputs, const srbd_solve_info* info, void* stream) {
  if (init_mode < 0 || init_mode > 2) return set_error(kErrInvalid, "srbd_pdipm_info: init_mode 0, 1 or 2");
  if (init_mode == 2 && (!inputs || (batch > 0 && !inputs[6])))
    return set_error(kErrInvalid, "srbd_pdipm_info: null x_init");
  return pdipm_common(horizon, n_iter, batch, init_mode == 1 ? y0 : 0.0, init_mode, inputs, outputs, info, stream);
}

int srbd_pdipm_ex(int horizon, int n_iter, int batch, int init_mode, double y0, const double* const* inputs,
                  double* const* outputs, int* status, void* stream) {
  const srbd_solve_info info = status_only(status);
  return srbd_pdipm_info(horizon, n_iter, batch, init_mode, y0, inputs, outputs, &info, stream);
}

static int mpc_solve_two_kernels(int horizon, int n_iter, int batch, double y0, const double* const* former_inputs,
                                 double* qp_workspace, double* const* outputs, const srbd_solve_info* info,
                                 void* stream) {
  if (!horizon_ok(horizon) || !qp_workspace) return set_error(kErrInvalid, "srbd_mpc_solve: bad arguments");
  double* qp[6];
  double* ws = qp_workspace;
  QpLayout(horizon).carve(ws, (size_t)(batch < 0 ? 0 : batch), qp);
  if (int rc = srbd_qp_former(horizon, batch, former_inputs, qp, stream)) return rc;
  const double* sin[10] = {};  // a cold start: the QP alone
  solver_order(qp, sin);
  return pdipm_common(horizon, n_iter, batch, y0, 1, sin, outputs, info, stream);
}

int srbd_mpc_solve(int horizon, int n_iter, int batch, double y0, const double* const* former_inputs,
                   double* qp_workspace, double* const* outputs, void* stream) {
  return mpc_solve_two_kernels(horizon, n_iter, batch, y0, former_inputs, qp_workspace, outputs, nullptr, stream);
}

// launch of the fused / controller-step kernel (a fully set up FusedArgs): the register kernels at
// the horizons they are instantiated for, the LDS-resident one-launch step (mpc_step_lds.hpp) at every
// other horizon
static int launch_step(const srbd::FusedArgs& a0, hipStream_t st) {
  srbd::FusedArgs a = a0;
  set_refinement_args(a);
  switch (serves(a.N)) {  // the register kernels' LDS is static (RegLayout)
    case Serves::Lds: {
      static LdsKernel step_lds{srbd::mpc_step_lds_kernel<0>, "mpc_step_lds_kernel launch",
                                "horizon too large for the one-launch step"};
      return launch_dynamic_lds(step_lds, 64, srbd::step_lds_bytes(a.N), a, st);
    }
    case Serves::Reg10:
      hipLaunchKernelGGL(srbd::mpc_step_reg_kernel<10>, dim3(a.batch), dim3(64), 0, st, a);
      break;
    case Serves::Reg20: srbd::reg20::launch_step(a, st); break;
    case Serves::RegN: srbd::regn::launch_step(a.N, a, st); break;
  }
  return launched("mpc_step_reg_kernel launch");
}

int srbd_mpc_solve_fused_info(int horizon, int n_iter, int batch, double y0, const double* const* former_inputs,
                              double* qp_workspace, double* const* outputs, const srbd_solve_info* info,
                              void* stream) {
  if (!horizon_ok(horizon)) return set_error(kErrInvalid, "srbd_mpc_solve_fused: bad horizon");
  if (solver_path() != 0) {  // a non-auto solver path: former + that solver kernel
    if (!qp_workspace) return set_error(kErrInvalid, "srbd_mpc_solve_fused: a non-auto solver path needs qp_workspace");
    return mpc_solve_two_kernels(horizon, n_iter, batch, y0, former_inputs, qp_workspace, outputs, info, stream);
  }
  if (n_iter < 1 || batch < 0 || !former_inputs || !outputs)
    return set_error(kErrInvalid, "srbd_mpc_solve_fused: bad arguments");
  if (batch == 0) return 0;
  srbd::FusedArgs a{};
  if (int rc = copy_pointers("srbd_mpc_solve_fused", "null input", a.in, former_inputs, 17)) return rc;
  for (int i = 0; i < 6; ++i) a.out[i] = outputs[i];  // null: not written
  if (qp_workspace) {  // the vectors f, b, d in the same slots as srbd_mpc_solve's H, f, A, b, G, d
    double* qp[6];
    double* ws = qp_workspace;
    QpLayout(horizon).carve(ws, (size_t)batch, qp);
    a.vec[0] = qp[1];
    a.vec[1] = qp[3];
    a.vec[2] = qp[5];
  }
  a.N = horizon;
  a.n_iter = n_iter;
  a.batch = batch;
  a.y0 = y0;
  set_info_args(a, info);
  return launch_step(a, (hipStream_t)stream);
}

int srbd_mpc_solve_fused_ex(int horizon, int n_iter, int batch, double y0, const double* const* former_inputs,
                            double* qp_workspace, double* const* outputs, int* status, void* stream) {
  const srbd_solve_info info = status_only(status);
  return srbd_mpc_solve_fused_info(horizon, n_iter, batch, y0, former_inputs, qp_workspace, outputs, &info, stream);
}

int srbd_mpc_solve_fused(int horizon, int n_iter, int batch, double y0, const double* const* former_inputs,
                         double* qp_workspace, double* const* outputs, void* stream) {
  return srbd_mpc_solve_fused_ex(horizon, n_iter, batch, y0, former_inputs, qp_workspace, outputs, nullptr, stream);
}

// srbd_mpc_prep (host struct of device pointers + constants) -> the kernels' PrepArgs
static int fill_prep(const srbd_mpc_prep* p, srbd::PrepArgs& a, const char* who) {
  if (!p->root_euler || !p->root_position || !p->root_angular_velocity_w || !p->root_velocity_w ||
      !p->rotation_body || !p->foot_position || !p->desired_velocity_b || !p->desired_angular_velocity_b ||
      !p->desired_height || !p->world_position_desired || !p->yaw_desired || !p->first_run || !p->dt_mpc ||
      !p->residual_lin_accel || !p->residual_ang_accel ||
      (p->gait_phase ? (!p->ssp_durations || !p->dsp_durations) : !p->contact_table) ||
      (p->q_len != 12 && p->q_len != 13))
    return fail(who, "missing array or bad q_len");
  a.root_euler = p->root_euler;
  a.root_position = p->root_position;
  a.ang_vel_w = p->root_angular_velocity_w;
  a.vel_w = p->root_velocity_w;
  a.rotation_body = p->rotation_body;
  a.foot_position = p->foot_position;
  a.des_vel_b = p->desired_velocity_b;
  a.des_angvel_b = p->desired_angular_velocity_b;
  a.des_height = p->desired_height;
  a.wpd = p->world_position_desired;
  a.yaw_des = p->yaw_desired;
  a.first_run = p->first_run;
  a.gait_phase = p->gait_phase;
  a.ssp = p->ssp_durations;
  a.dsp = p->dsp_durations;
  a.contact_table = p->contact_table;
  a.dt_mpc = p->dt_mpc;
  a.res_lin = p->residual_lin_accel;
  a.res_ang = p->residual_ang_accel;
  std::memcpy(a.I_body, p->I_body, sizeof(a.I_body));
  a.mass = p->mass;
  a.mu = p->mu;
  std::memcpy(a.Q, p->Q, sizeof(a.Q));
  a.q_len = p->q_len;
  std::memcpy(a.R, p->R, sizeof(a.R));
  a.step_dt = p->step_dt;
  a.literal = p->literal_layout ? 1 : 0;
  return 0;
}

int srbd_mpc_step_info(int horizon, int n_iter, int batch, double y0, const srbd_mpc_prep* prep,
                       double* const* former_inputs, double* const* outputs, float* foot_wrench, int ndof,
                       const float* contact_jacobian, const float* contact_bool, float* tau,
                       const srbd_solve_info* info, void* stream) {
  if (!horizon_ok(horizon)) return set_error(kErrInvalid, "srbd_mpc_step: bad horizon");
  if (n_iter < 1 || batch < 0 || !prep || (tau && (ndof < 1 || ndof > 64)))
    return set_error(kErrInvalid, "srbd_mpc_step: bad arguments");
  if (batch == 0) return 0;
  if (!foot_wrench || (tau && (!contact_jacobian || !contact_bool)))
    return set_error(kErrInvalid, "srbd_mpc_step: null foot_wrench / contact_jacobian / contact_bool");
  srbd::FusedArgs a{};
  if (int rc = fill_prep(prep, a.prep, "srbd_mpc_step")) return rc;
  a.prep.N = horizon;
  a.prep.batch = batch;
  if (former_inputs)
    if (int rc = copy_pointers("srbd_mpc_step", "null former_inputs entry", a.prep.out, former_inputs, 17)) return rc;
  a.ctrl = 1;
  if (outputs)
    for (int i = 0; i < 6; ++i) a.out[i] = outputs[i];
  a.wrench = foot_wrench;
  a.tau = tau;
  a.jac = contact_jacobian;
  a.contact = contact_bool;
  a.ndof = tau ? ndof : 0;
  a.N = horizon;
  a.n_iter = n_iter;
  a.batch = batch;
  a.y0 = y0;
  set_info_args(a, info);
  return launch_step(a, (hipStream_t)stream);
}

int srbd_mpc_step_ex(int horizon, int n_iter, int batch, double y0, const srbd_mpc_prep* prep,
                     double* const* former_inputs, double* const* outputs, float* foot_wrench, int ndof,
                     const float* contact_jacobian, const float* contact_bool, float* tau, int* status,
                     void* stream) {
  const srbd_solve_info info = status_only(status);
  return srbd_mpc_step_info(horizon, n_iter, batch, y0, prep, former_inputs, outputs, foot_wrench, ndof,
                            contact_jacobian, contact_bool, tau, &info, stream);
}

int srbd_mpc_step(int horizon, int n_iter, int batch, double y0, const srbd_mpc_prep* prep,
                  double* const* former_inputs, double* const* outputs, float* foot_wrench, int ndof,
                  const float* contact_jacobian, const float* contact_bool, float* tau, void* stream) {
  return srbd_mpc_step_ex(horizon, n_iter, batch, y0, prep, former_inputs, outputs, foot_wrench, ndof,
                          contact_jacobian, contact_bool, tau, nullptr, stream);
}

// ---- backward pass (pdipm_backward.hpp, qp_former_backward.hpp; kernels in srbd_backward.hip) ----
// One implementation per stage; the exported entries forward to them with their own name (`what`)
// for the messages. A single-seed entry is n_seeds = 1 with the seeds' env stride 24 * horizon; an
// x-only entry is a srbd_backward_seeds with grad_x alone (`x_only`: its messages name grad_x).

namespace {

// batch * n_seeds gradient rows must fit the launch grid's int
bool seed_rows_ok(int batch, int n_seeds) { return (long long)batch * (long long)n_seeds <= (long long)INT_MAX; }

// the checks every backward entry starts with
int check_seeds(const char* what, int horizon, int batch, int n_seeds, size_t env_stride, bool pointers_ok) {
  if (!horizon_ok(horizon) || batch < 0 || n_seeds < 1 || !pointers_ok) return fail(what, "bad arguments");
  if (env_stride != 0 && env_stride != (size_t)n_seeds * 24 * (size_t)horizon)
    return fail(what, "grad_x_env_stride must be 0 or n_seeds * 24 * horizon");
  if (!seed_rows_ok(batch, n_seeds)) return fail(what, "batch * n_seeds overflows");
  return 0;
}

// grad_x alone, addressed by the x-only entries' env stride (checked by check_seeds: 0 or n_seeds * 24N)
srbd_backward_seeds x_seed(const double* grad_x, size_t env_stride) {
  srbd_backward_seeds sd{};
  sd.grad_x = grad_x;
  sd.shared = env_stride == 0 ? 1 : 0;
  return sd;
}

bool any_seed(const srbd_backward_seeds& sd) {
  return sd.grad_x || sd.grad_s || sd.grad_z || sd.grad_y || sd.grad_objective;
}

// the adjoint KKT solve and the QP-data gradients of n_seeds seeds per env
int adjoint_impl(const char* what, bool x_only, int horizon, int batch, int n_seeds, const double* const* inputs,
                 const srbd_backward_seeds& sd, double* const* qp_grads, int* status, void* stream) {
  if (batch == 0) return 0;
  for (int i = 0; i < 10; ++i)
    if (!inputs[i] && !(i >= 3 && i <= 5)) return fail(what, "null input");  // f, h, b (3..5): see below
  if (!any_seed(sd)) return fail(what, x_only ? "null grad_x" : "no seed given: all five cotangents are null");
  if (sd.grad_objective && !inputs[3]) return fail(what, "grad_objective needs f (input 3)");
  const size_t lds = srbd::backward_lds_bytes(horizon);
  constexpr const char* kTooLarge = "horizon too large for the LDS-resident backward solve";
  auto fill = [&](auto& a) {  // the fields BackwardArgs and BackwardMultiArgs share
    for (int i = 0; i < 10; ++i) a.in[i] = inputs[i];
    a.grad_x = sd.grad_x;
    a.more = srbd::BackwardMoreSeeds{sd.grad_s, sd.grad_z, sd.grad_y, sd.grad_objective};
    for (int i = 0; i < 6; ++i) a.out[i] = qp_grads[i];  // null: not written
    a.status = status;
    a.N = horizon;
    a.batch = batch;
  };
  // grad_x alone: the instantiation with the other cotangents compiled out (the same bits)
  const bool full = sd.grad_s || sd.grad_z || sd.grad_y || sd.grad_objective;
  // one seed per env, B rows: the single-seed kernel (the other's bits, 1-2 % faster there)
  if (n_seeds == 1 && !sd.shared) {
    constexpr const char* kWhat = "pdipm_backward_kernel launch";
    static LdsKernel<srbd::BackwardArgs> of_x{srbd::bwd::adjoint_kernel(false), kWhat, kTooLarge};
    static LdsKernel<srbd::BackwardArgs> of_all{srbd::bwd::adjoint_kernel(true), kWhat, kTooLarge};
    srbd::BackwardArgs a{};
    fill(a);
    return launch_dynamic_lds(full ? of_all : of_x, 64, lds, a, (hipStream_t)stream);
  }
  constexpr const char* kWhat = "pdipm_backward_multi_kernel launch";
  static LdsKernel<srbd::BackwardMultiArgs> of_x{srbd::bwd::adjoint_multi_kernel(false), kWhat, kTooLarge};
  static LdsKernel<srbd::BackwardMultiArgs> of_all{srbd::bwd::adjoint_multi_kernel(true), kWhat, kTooLarge};
  srbd::BackwardMultiArgs a{};
  fill(a);
  a.shared = sd.shared ? 1 : 0;
  a.n_seeds = n_seeds;
  return launch_dynamic_lds(full ? of_all : of_x, 64, lds, a, (hipStream_t)stream);
}

// the former's vector-Jacobian product over batch * n_seeds gradient rows
int former_vjp_impl(const char* what, int horizon, int batch, int n_seeds, const double* const* former_inputs,
                    const double* const* qp_grads, double* const* input_grads, void* stream) {
  if (int rc = check_seeds(what, horizon, batch, n_seeds, 0, former_inputs && qp_grads && input_grads)) return rc;
  if (batch == 0) return 0;
  srbd::FormerBackwardArgs a{};
  if (int rc = copy_pointers(what, "null input", a.in, former_inputs, 17)) return rc;
  for (int i = 0; i < 17; ++i) a.out[i] = input_grads[i];  // null: not written
  for (int i = 0; i < 6; ++i) a.g[i] = qp_grads[i];  // null: a zero gradient
  a.N = horizon;
  a.batch = batch;
  a.n_seeds = n_seeds;
  srbd::bwd::launch_former_backward(a, (hipStream_t)stream);
  return launched("qp_former_backward_kernel launch");
}

// the QP gradients (bit o: H, f, A, b, G, d) the gradient of former input i reads: the table in the
// header comment of qp_former_backward.hpp
constexpr unsigned kGradH = 1u, kGradF = 2u, kGradA = 4u, kGradB = 8u, kGradG = 16u, kGradD = 32u;
constexpr unsigned kFormerGradDeps[17] = {
    kGradB,           // x0
    0u,               // x: zero gradient
    0u,               // u: zero gradient
    kGradF,           // x_ref
    kGradA | kGradB,  // dt
    kGradA | kGradB,  // m
    kGradG,           // mu
    kGradA | kGradB,  // R_body
    kGradA | kGradB,  // I_world
    kGradA | kGradB,  // body position
    kGradA | kGradB,  // left foot position
    kGradA | kGradB,  // right foot position
    kGradD,           // contact_table
    kGradH | kGradF,  // Q
    kGradH,           // R
    kGradA | kGradB,  // residual linear acceleration
    kGradA | kGradB,  // residual angular acceleration
};

// the union of the dependencies of the inputs in input_mask (bit i = former input i)
unsigned qp_grads_needed(unsigned input_mask) {
  unsigned need = 0;
  for (int i = 0; i < 17; ++i)
    if (input_mask >> i & 1u) need |= kFormerGradDeps[i];
  return need;
}

// former -> adjoint -> former VJP. The workspace holds the QP, then the QP gradients the non-null
// input_grads read, (B, M, width) each; the others are null to both kernels (the adjoint kernel skips a
// null output, the VJP reads a null gradient as zero). Whether asking for no gradient at all is an error
// (`need_request`) is the calling entry's business.
int mpc_backward_impl(const char* what, bool x_only, bool need_request, int horizon, int batch, int n_seeds,
                      const double* const* former_inputs, const double* const* iterate,
                      const srbd_backward_seeds& sd, double* workspace, double* const* input_grads, int* status,
                      void* stream) {
  if (batch == 0) return 0;
  if (!workspace || (x_only && !sd.grad_x) || !iterate[0] || !iterate[1] || !iterate[2] || !iterate[3])
    return fail(what, x_only ? "null workspace / grad_x / iterate" : "null workspace / iterate");
  if (!any_seed(sd)) return fail(what, "no seed given: all five cotangents are null");
  unsigned input_mask = 0;
  for (int i = 0; i < 17; ++i)
    if (input_grads[i]) input_mask |= 1u << i;
  if (need_request && input_mask == 0) return fail(what, "no input gradient requested");
  const unsigned need = qp_grads_needed(input_mask);
  const QpLayout layout(horizon);
  double* qp[6];
  double* gr[6];
  double* o = workspace;
  layout.carve(o, (size_t)batch, qp);
  layout.carve(o, (size_t)batch * (size_t)n_seeds, gr, need);
  if (int rc = srbd_qp_former(horizon, batch, former_inputs, qp, stream)) return rc;
  const double* sin[10];
  solver_order(qp, sin);
  std::copy(iterate, iterate + 4, sin + 6);
  if (int rc = adjoint_impl(what, x_only, horizon, batch, n_seeds, sin, sd, gr, status, stream)) return rc;
  return former_vjp_impl(what, horizon, batch, n_seeds, former_inputs, gr, input_grads, stream);
}

}  // namespace

int srbd_pdipm_backward(int horizon, int batch, const double* const* inputs, const double* grad_x,
                        double* const* qp_grads, int* status, void* stream) {
  const char* what = "srbd_pdipm_backward";
  if (int rc = check_seeds(what, horizon, batch, 1, 24 * (size_t)horizon, inputs && qp_grads)) return rc;
  return adjoint_impl(what, true, horizon, batch, 1, inputs, x_seed(grad_x, 24 * (size_t)horizon), qp_grads, status, stream);
}

int srbd_pdipm_backward_multi(int horizon, int batch, int n_seeds, const double* const* inputs,
                              const double* grad_x, size_t grad_x_env_stride, double* const* qp_grads,
                              int* status, void* stream) {
  const char* what = "srbd_pdipm_backward_multi";
  if (int rc = check_seeds(what, horizon, batch, n_seeds, grad_x_env_stride, inputs && qp_grads)) return rc;
  return adjoint_impl(what, true, horizon, batch, n_seeds, inputs, x_seed(grad_x, grad_x_env_stride), qp_grads,
                      status, stream);
}

int srbd_pdipm_backward_seeds(int horizon, int batch, int n_seeds, const double* const* inputs,
                              const srbd_backward_seeds* seeds, double* const* qp_grads, int* status, void* stream) {
  const char* what = "srbd_pdipm_backward_seeds";
  if (int rc = check_seeds(what, horizon, batch, n_seeds, 0, inputs && seeds && qp_grads)) return rc;
  return adjoint_impl(what, false, horizon, batch, n_seeds, inputs, *seeds, qp_grads, status, stream);
}

int srbd_qp_former_backward(int horizon, int batch, const double* const* former_inputs,
                            const double* const* qp_grads, double* const* input_grads, void* stream) {
  return former_vjp_impl("srbd_qp_former_backward", horizon, batch, 1, former_inputs, qp_grads, input_grads, stream);
}

int srbd_qp_former_backward_multi(int horizon, int batch, int n_seeds, const double* const* former_inputs,
                                  const double* const* qp_grads, double* const* input_grads, void* stream) {
  return former_vjp_impl("srbd_qp_former_backward_multi", horizon, batch, n_seeds, former_inputs, qp_grads,
                         input_grads, stream);
}

unsigned srbd_former_grad_deps(int input) { return input >= 0 && input < 17 ? kFormerGradDeps[input] : 0u; }

size_t srbd_mpc_backward_multi_workspace_doubles(int horizon, int batch, int n_seeds, unsigned input_mask) {
  if (!horizon_ok(horizon) || batch < 0 || n_seeds < 1 || !seed_rows_ok(batch, n_seeds)) return 0;
  const unsigned need = qp_grads_needed(input_mask ? input_mask : ~0u);  // 0 = all 17
  const QpLayout layout(horizon);  // what mpc_backward_impl carves
  return layout.doubles((size_t)batch) + layout.doubles((size_t)batch * (size_t)n_seeds, need);
}

size_t srbd_mpc_backward_workspace_doubles(int horizon, int batch) {
  return 2 * srbd_mpc_workspace_doubles(horizon, batch);  // the QP and all six gradients: an upper bound
}

int srbd_mpc_backward(int horizon, int batch, const double* const* former_inputs, const double* const* iterate,
                      const double* grad_x, double* workspace, double* const* input_grads, int* status,
                      void* stream) {  // all 17 input_grads may be null: only `status` is written then
  const char* what = "srbd_mpc_backward";
  if (int rc = check_seeds(what, horizon, batch, 1, 24 * (size_t)horizon, former_inputs && iterate && input_grads))
    return rc;
  return mpc_backward_impl(what, true, false, horizon, batch, 1, former_inputs, iterate, x_seed(grad_x, 24 * (size_t)horizon),
                           workspace, input_grads, status, stream);
}

int srbd_mpc_backward_multi(int horizon, int batch, int n_seeds, const double* const* former_inputs,
                            const double* const* iterate, const double* grad_x, size_t grad_x_env_stride,
                            double* workspace, double* const* input_grads, int* status, void* stream) {
  const char* what = "srbd_mpc_backward_multi";
  if (int rc = check_seeds(what, horizon, batch, n_seeds, grad_x_env_stride, former_inputs && iterate && input_grads))
    return rc;
  return mpc_backward_impl(what, true, true, horizon, batch, n_seeds, former_inputs, iterate,
                           x_seed(grad_x, grad_x_env_stride), workspace, input_grads, status, stream);
}

// All 17 input_grads may be null (only `status` is written then), as in srbd_mpc_backward.
int srbd_mpc_backward_seeds(int horizon, int batch, int n_seeds, const double* const* former_inputs,
                            const double* const* iterate, const srbd_backward_seeds* seeds, double* workspace,
                            double* const* input_grads, int* status, void* stream) {
  const char* what = "srbd_mpc_backward_seeds";
  if (int rc = check_seeds(what, horizon, batch, n_seeds, 0, former_inputs && iterate && seeds && input_grads))
    return rc;
  return mpc_backward_impl(what, false, false, horizon, batch, n_seeds, former_inputs, iterate, *seeds, workspace,
                           input_grads, status, stream);
}

}  // extern "C"

// ---- backward pass of the controller step's FP32 ends (mpc_io_backward.hpp; kernels in srbd_backward.hip,
// the only unit that includes that header: the forward units' code does not change with it) ----

namespace srbd {
namespace bwd {
void launch_prepare_backward(const PrepArgs& prep, const double* const* g, const float* gwpd, const float* gyaw,
                             const double* gR, float* const* out, hipStream_t s);
void launch_wrench_backward(int N, int batch, const double* x, const float* rotation_body, const float* grad_wrench,
                            int ndof, const float* J, const float* contact, const float* grad_tau, double* grad_x,
                            double* grad_R, hipStream_t s);
void launch_widen(int n, const float* src, double* dst, hipStream_t s);
}  // namespace bwd
}  // namespace srbd

namespace {

// the former-input cotangents (bit i = former input i) each prep gradient reads: the table of
// prepare_inputs_backward_kernel
constexpr unsigned fin(int i) { return 1u << i; }
constexpr unsigned kPrepGradDeps[SRBD_PREP_GRAD_COUNT] = {
    fin(0) | fin(3),           // root_euler: x0, and the yaw knot point on a first run
    fin(0) | fin(3) | fin(9),  // root_position: x0, x_ref's origin, body position
    fin(0),                    // root_angular_velocity_w
    fin(0),                    // root_velocity_w
    fin(3) | fin(7) | fin(8),  // rotation_body: vw = R v_b in x_ref, R_body, I_world
    fin(10) | fin(11),         // foot_position
    fin(3),                    // desired_velocity_b
    fin(3),                    // desired_angular_velocity_b
    fin(3),                    // desired_height
    fin(3),                    // world_position_desired
    fin(3),                    // yaw_desired
    fin(12),                   // contact_table
    fin(3) | fin(4),           // dt_mpc
    fin(15),                   // residual_lin_accel
    fin(16),                   // residual_ang_accel
};

unsigned former_inputs_needed(unsigned prep_mask) {
  unsigned need = 0;
  for (int f = 0; f < SRBD_PREP_GRAD_COUNT; ++f)
    if (prep_mask >> f & 1u) need |= kPrepGradDeps[f];
  return need;
}

unsigned prep_request_mask(float* const* prep_grads) {
  unsigned m = 0;
  for (int f = 0; f < SRBD_PREP_GRAD_COUNT; ++f)
    if (prep_grads[f]) m |= 1u << f;
  return m;
}

int wrench_vjp_impl(const char* what, int horizon, int batch, const double* x, const float* rotation_body,
                    const float* grad_wrench, int ndof, const float* contact_jacobian, const float* contact_bool,
                    const float* grad_tau, double* grad_x, double* grad_rotation_body, void* stream) {
  if (!horizon_ok(horizon) || batch < 0) return fail(what, "bad arguments");
  if (grad_tau && (ndof < 1 || ndof > 64 || !contact_jacobian || !contact_bool))
    return fail(what, "grad_tau needs contact_jacobian, contact_bool and ndof in 1..64");
  if (batch == 0) return 0;
  if (!x || !rotation_body || !grad_wrench || !grad_x) return fail(what, "null x / rotation_body / grad_wrench / grad_x");
  srbd::bwd::launch_wrench_backward(horizon, batch, x, rotation_body, grad_wrench, grad_tau ? ndof : 0,
                                    contact_jacobian, contact_bool, grad_tau, grad_x, grad_rotation_body,
                                    (hipStream_t)stream);
  return launched("u0_wrench_backward_kernel launch");
}

// the arrays of srbd_mpc_prep the prep VJP reads
int check_prep_backward(const char* what, const srbd_mpc_prep* p) {
  if (!p->rotation_body || !p->desired_velocity_b || !p->desired_angular_velocity_b || !p->dt_mpc || !p->first_run)
    return fail(what, "null rotation_body / desired_velocity_b / desired_angular_velocity_b / dt_mpc / first_run");
  return 0;
}

int prep_vjp_impl(const char* what, int horizon, int batch, const srbd_mpc_prep* p, const double* const* input_grads,
                  const float* grad_wpd_out, const float* grad_yaw_out, const double* grad_rotation_body_direct,
                  float* const* prep_grads, void* stream) {
  if (!horizon_ok(horizon) || batch < 0 || !p || !input_grads || !prep_grads) return fail(what, "bad arguments");
  if (p->gait_phase && prep_grads[SRBD_PREP_GRAD_CONTACT_TABLE])
    return fail(what, "no contact_table gradient when the schedule comes from gait_phase");
  if (batch == 0) return 0;
  if (int rc = check_prep_backward(what, p)) return rc;
  srbd::PrepArgs a{};  // only what the kernel reads
  a.rotation_body = p->rotation_body;
  a.des_vel_b = p->desired_velocity_b;
  a.des_angvel_b = p->desired_angular_velocity_b;
  a.dt_mpc = p->dt_mpc;
  a.first_run = p->first_run;  // the pre-step snapshot; read only
  std::memcpy(a.I_body, p->I_body, sizeof(a.I_body));
  a.step_dt = p->step_dt;
  a.literal = p->literal_layout ? 1 : 0;
  a.N = horizon;
  a.batch = batch;
  srbd::bwd::launch_prepare_backward(a, input_grads, grad_wpd_out, grad_yaw_out, grad_rotation_body_direct,
                                     prep_grads, (hipStream_t)stream);
  return launched("prepare_inputs_backward_kernel launch");
}

size_t former_in_width(int i, int N) { return (size_t)srbd::former_in_nnz(i, N); }

}  // namespace

extern "C" {

int srbd_u0_wrench_backward(int horizon, int batch, const double* x, const float* rotation_body,
                            const float* grad_wrench, int ndof, const float* contact_jacobian,
                            const float* contact_bool, const float* grad_tau, double* grad_x,
                            double* grad_rotation_body, void* stream) {
  return wrench_vjp_impl("srbd_u0_wrench_backward", horizon, batch, x, rotation_body, grad_wrench, ndof,
                         contact_jacobian, contact_bool, grad_tau, grad_x, grad_rotation_body, stream);
}

int srbd_prepare_inputs_backward(int horizon, int batch, const srbd_mpc_prep* prep, const double* const* input_grads,
                                 const float* grad_wpd_out, const float* grad_yaw_out,
                                 const double* grad_rotation_body_direct, float* const* prep_grads, void* stream) {
  return prep_vjp_impl("srbd_prepare_inputs_backward", horizon, batch, prep, input_grads, grad_wpd_out, grad_yaw_out,
                       grad_rotation_body_direct, prep_grads, stream);
}

unsigned srbd_prep_grad_deps(int field) {
  return field >= 0 && field < SRBD_PREP_GRAD_COUNT ? kPrepGradDeps[field] : 0u;
}

size_t srbd_mpc_step_backward_workspace_doubles(int horizon, int batch, unsigned prep_mask) {
  if (!horizon_ok(horizon) || batch < 0) return 0;
  const unsigned need = former_inputs_needed(prep_mask ? prep_mask : ~0u);  // 0 = all 15
  size_t per_env = 24 * (size_t)horizon + 9;  // the seed grad_x and the direct rotation_body term
  for (int i = 0; i < 17; ++i)
    if (need >> i & 1u) per_env += former_in_width(i, horizon);
  // need == 0 would read as "all 17" there; every prep gradient reads some former input, so it is never 0
  return (size_t)batch * per_env + srbd_mpc_backward_multi_workspace_doubles(horizon, batch, 1, need);
}

}  // extern "C"

namespace {

// wrench VJP (with grad_wrench) and the widened cost cotangent (with grad_cost) -> adjoint and former VJP
// -> input-preparation VJP. `with_cost`: the entry takes grad_cost, and grad_wrench may then be null.
int step_backward_impl(const char* what, bool with_cost, int horizon, int batch, const srbd_mpc_prep* prep,
                       const double* const* former_inputs, const double* const* iterate, const float* grad_wrench,
                       const float* grad_cost, int ndof, const float* contact_jacobian, const float* contact_bool,
                       const float* grad_tau, const float* grad_wpd_out, const float* grad_yaw_out,
                       double* workspace, float* const* prep_grads, int* status, void* stream) {
  if (!horizon_ok(horizon) || batch < 0 || !prep || !former_inputs || !iterate || !prep_grads)
    return fail(what, "bad arguments");
  if (grad_tau && (ndof < 1 || ndof > 64 || !contact_jacobian || !contact_bool))
    return fail(what, "grad_tau needs contact_jacobian, contact_bool and ndof in 1..64");
  if (prep->gait_phase && prep_grads[SRBD_PREP_GRAD_CONTACT_TABLE])
    return fail(what, "no contact_table gradient when the schedule comes from gait_phase");
  if (batch == 0) return 0;
  const unsigned prep_mask = prep_request_mask(prep_grads);
  if (prep_mask == 0) return fail(what, "no prep gradient requested");
  if (!workspace || (!with_cost && !grad_wrench) || !iterate[0] || !iterate[1] || !iterate[2] || !iterate[3])
    return fail(what, with_cost ? "null workspace / iterate" : "null workspace / grad_wrench / iterate");
  if (!grad_wrench && !grad_cost) return fail(what, "grad_wrench and grad_cost are both null");
  if (grad_tau && !grad_wrench) return fail(what, "grad_tau needs grad_wrench");
  if (int rc = check_prep_backward(what, prep)) return rc;
  const unsigned need = former_inputs_needed(prep_mask);
  const size_t B = (size_t)batch;
  double* seed = workspace;
  double* direct = seed + B * 24 * (size_t)horizon;
  double* o = direct + B * 9;
  double* fin_grads[17];
  for (int i = 0; i < 17; ++i) {
    fin_grads[i] = (need >> i & 1u) ? o : nullptr;
    if (fin_grads[i]) o += B * former_in_width(i, horizon);
  }
  // the wrench's direct rotation_body term exists only with a wrench cotangent
  const bool want_R = grad_wrench && prep_grads[SRBD_PREP_GRAD_ROTATION_BODY] != nullptr;
  srbd_backward_seeds sd{};
  if (grad_wrench) {
    if (int rc = wrench_vjp_impl(what, horizon, batch, iterate[0], prep->rotation_body, grad_wrench, ndof,
                                 contact_jacobian, contact_bool, grad_tau, seed, want_R ? direct : nullptr, stream))
      return rc;
    sd.grad_x = seed;
  }
  double* mpc_ws = o;
  if (grad_cost) {  // behind srbd_mpc_step_backward's layout: the cost cotangent, widened (B)
    double* gJ = o + srbd_mpc_backward_multi_workspace_doubles(horizon, batch, 1, need);
    srbd::bwd::launch_widen(batch, grad_cost, gJ, (hipStream_t)stream);
    if (int rc = launched("widen_f32_kernel launch")) return rc;
    sd.grad_objective = gJ;
  }
  if (int rc = mpc_backward_impl(what, !with_cost, false, horizon, batch, 1, former_inputs, iterate, sd, mpc_ws,
                                 fin_grads, status, stream))
    return rc;
  return prep_vjp_impl(what, horizon, batch, prep, fin_grads, grad_wpd_out, grad_yaw_out, want_R ? direct : nullptr,
                       prep_grads, stream);
}

}  // namespace

extern "C" {

int srbd_mpc_step_backward(int horizon, int batch, const srbd_mpc_prep* prep, const double* const* former_inputs,
                           const double* const* iterate, const float* grad_wrench, int ndof,
                           const float* contact_jacobian, const float* contact_bool, const float* grad_tau,
                           const float* grad_wpd_out, const float* grad_yaw_out, double* workspace,
                           float* const* prep_grads, int* status, void* stream) {
  return step_backward_impl("srbd_mpc_step_backward", false, horizon, batch, prep, former_inputs, iterate,
                            grad_wrench, nullptr, ndof, contact_jacobian, contact_bool, grad_tau, grad_wpd_out,
                            grad_yaw_out, workspace, prep_grads, status, stream);
}

size_t srbd_mpc_step_backward_cost_workspace_doubles(int horizon, int batch, unsigned prep_mask) {
  if (!horizon_ok(horizon) || batch < 0) return 0;
  return srbd_mpc_step_backward_workspace_doubles(horizon, batch, prep_mask) + (size_t)batch;
}

int srbd_mpc_step_backward_cost(int horizon, int batch, const srbd_mpc_prep* prep,
                                const double* const* former_inputs, const double* const* iterate,
                                const float* grad_wrench, const float* grad_cost, int ndof,
                                const float* contact_jacobian, const float* contact_bool, const float* grad_tau,
                                const float* grad_wpd_out, const float* grad_yaw_out, double* workspace,
                                float* const* prep_grads, int* status, void* stream) {
  return step_backward_impl("srbd_mpc_step_backward_cost", true, horizon, batch, prep, former_inputs, iterate,
                            grad_wrench, grad_cost, ndof, contact_jacobian, contact_bool, grad_tau, grad_wpd_out,
                            grad_yaw_out, workspace, prep_grads, status, stream);
}

int srbd_pattern_ccs(int horizon, int which, int* colptr, int* rowind) {
  if (!horizon_ok(horizon) || !colptr || !rowind) return -1;
  constexpr srbd::Tables T = srbd::make_tables();
  const int N = horizon, nz = 24 * N;
  int nnz = 0;
  std::vector<int> row, col;
  auto put = [&](int off, int r, int c) {
    if (off < 0 || off >= nnz) return false;
    if (row[off] != -1) return false;  // two entries mapped to one value slot
    row[off] = r;
    col[off] = c;
    return true;
  };
  if (which == 0) {
    nnz = nz;
    row.assign(nnz, -1);
    col.assign(nnz, -1);
    for (int c = 0; c < nz; ++c)
      if (!put(c, c, c)) return -2;
  } else if (which == 1) {
    nnz = srbd::nnz_A(N);
    row.assign(nnz, -1);
    col.assign(nnz, -1);
    for (int i = 0; i < N; ++i) {
      const int ub = srbd::a_ublock(N, i);
      for (int r = 0; r < 12; ++r) {
        if (!put(srbd::a_pidx(T, N, i, r), 12 * i + r, 12 * i + r)) return -2;  // x_{i+1}[r]
        for (int j = 0; j < 12; ++j) {
          if (i >= 1 && T.Mi[r][j] >= 0 && !put(srbd::a_xblock(i) + T.Mi[r][j], 12 * i + r, 12 * (i - 1) + j))
            return -2;
          if (T.Ni[r][j] >= 0 && !put(ub + T.Ni[r][j], 12 * i + r, 12 * N + 12 * i + j)) return -2;
        }
      }
      if (!put(ub + T.e6, 12 * N + 2 * i, 12 * N + 12 * i + 6)) return -2;
      if (!put(ub + T.e9, 12 * N + 2 * i + 1, 12 * N + 12 * i + 9)) return -2;
    }
  } else if (which == 2) {
    nnz = 28 * N;
    row.assign(nnz, -1);
    col.assign(nnz, -1);
    for (int i = 0; i < N; ++i)
      for (int q = 0; q < 28; ++q)
        if (!put(28 * i + q, 16 * i + T.grow[q], 12 * N + 12 * i + T.gcol[q])) return -2;
  } else {
    return -1;
  }
  // every slot filled, (col, row) strictly increasing in slot order  => valid sorted CCS
  for (int k = 0; k < nnz; ++k) {
    if (row[k] < 0) return -3;
    if (k > 0 && (col[k] < col[k - 1] || (col[k] == col[k - 1] && row[k] <= row[k - 1]))) return -4;
  }
  for (int c = 0; c <= nz; ++c) colptr[c] = 0;
  for (int k = 0; k < nnz; ++k) {
    colptr[col[k] + 1]++;
    rowind[k] = row[k];
  }
  for (int c = 0; c < nz; ++c) colptr[c + 1] += colptr[c];
  return nnz;
}

int srbd_prepare_inputs(int horizon, int batch, const srbd_mpc_prep* p, double* const* former_inputs,
                        void* stream) {
  if (!horizon_ok(horizon) || batch < 0 || !p || !former_inputs)
    return set_error(kErrInvalid, "srbd_prepare_inputs: bad arguments");
  if (batch == 0) return 0;
  srbd::PrepArgs a{};
  if (int rc = fill_prep(p, a, "srbd_prepare_inputs")) return rc;
  if (int rc = copy_pointers("srbd_prepare_inputs", "null output", a.out, former_inputs, 17)) return rc;
  a.N = horizon;
  a.batch = batch;
  hipLaunchKernelGGL(srbd::prepare_inputs_kernel, dim3((batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  return launched("prepare_inputs_kernel launch");
}

int srbd_u0_wrench(int horizon, int batch, const double* x, const float* rotation_body, float* foot_wrench,
                   void* stream) {
  return srbd_u0_wrench_torque(horizon, batch, x, rotation_body, foot_wrench, 0, nullptr, nullptr, nullptr, stream);
}

int srbd_u0_wrench_torque(int horizon, int batch, const double* x, const float* rotation_body, float* foot_wrench,
                          int ndof, const float* contact_jacobian, const float* contact_bool, float* tau,
                          void* stream) {
  const bool torque = tau != nullptr;
  if (!horizon_ok(horizon) || batch < 0 || (batch > 0 && (!x || !rotation_body || !foot_wrench)) ||
      (torque && (ndof < 1 || ndof > 64 || (batch > 0 && (!contact_jacobian || !contact_bool)))))
    return set_error(kErrInvalid, "srbd_u0_wrench_torque: bad arguments");
  if (batch == 0) return 0;
  hipLaunchKernelGGL(srbd::u0_wrench_kernel, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, horizon,
                     batch, x, rotation_body, foot_wrench, ndof, contact_jacobian, contact_bool, tau);
  return launched("u0_wrench_kernel launch");
}

int srbd_dense_scatter(int batch, int nnz, int rc, const int* inverse_index, const double* values, double* dense,
                       void* stream) {
  if (batch < 0 || nnz < 0 || rc < 0 || batch > 65535 ||
      (batch > 0 && rc > 0 && (!inverse_index || !dense || (nnz > 0 && !values))))
    return set_error(kErrInvalid, "srbd_dense_scatter: bad arguments (batch <= 65535 per call)");
  if (batch == 0 || rc == 0) return 0;
  hipLaunchKernelGGL(srbd::dense_scatter_kernel, dim3((rc + 511) / 512, batch), dim3(256), 0, (hipStream_t)stream, rc,
                     nnz, batch, (const int32_t*)inverse_index, values, dense);
  return launched("dense_scatter_kernel launch");
}

}  // extern "C"
