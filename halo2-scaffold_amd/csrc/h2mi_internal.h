// Internal host-side plumbing shared by the libh2mi.so translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/h2mi.h"

namespace h2 {

struct ProfRec {
  std::string name;
  hipEvent_t a, b;
};

// One entry per device the process drives (h2mi_init: one; h2mi_init_devices(n): n).  Entry 0 is the primary
// device: transforms, polynomial helpers and the final fold of a sharded MSM run there.  With fewer physical GPUs
// than requested (H2MI_VIRTUAL_DEVICES=1) several entries share one GPU — a rehearsal mode for one-GPU boxes.
struct DevCtx {
  int device = -1;
  hipStream_t stream = nullptr, head_stream = nullptr, accum_stream = nullptr, tail_stream = nullptr;
};

struct Ctx {
  bool inited = false;
  int device = -1;
  std::vector<DevCtx> devs;
  int cur = 0;  // index into devs of the entry whose streams are mirrored in the members below
  hipStream_t stream = nullptr;
  // MSM pipeline on the library's own stream: sort (memory-bound) | accumulation (VALU-bound) | bucket
  // reduction (latency-bound) of consecutive MSMs run on three internal streams and overlap.
  hipStream_t head_stream = nullptr, accum_stream = nullptr, tail_stream = nullptr;
  std::recursive_mutex mu;
  bool profiling = false;
  std::string prof_filter;
  std::vector<ProfRec> prof;
  char last_err[256] = {0};
};

Ctx& ctx();
// make entry `idx` current: this THREAD's HIP device + the stream members of Ctx mirror its streams (callers hold the mutex)
int use_device(int idx);
// make `device` the calling thread's HIP device (checked against hipGetDevice every time: HIP's current device is per host thread)
int set_thread_device(int device);
// every extern "C" entry point: the calling thread's HIP device = the primary device (entry 0), whatever another thread
// or an earlier call on this thread selected; entry points that drive other devices switch with use_device under the mutex
int bind_thread();
// the primary device's stream, for entry points that do not take the mutex (another thread may be switching the mirrors
// in Ctx between devices inside a sharded MSM)
inline hipStream_t primary_stream() { return ctx().devs.empty() ? nullptr : ctx().devs[0].stream; }

inline hipStream_t pick_stream(h2mi_stream_t s) { return s ? reinterpret_cast<hipStream_t>(s) : ctx().stream; }

void note_hip_error(hipError_t e, const char* file, int line);

#define H2_HIP(x)                                   \
  do {                                              \
    hipError_t e_ = (x);                            \
    if (e_ != hipSuccess) {                         \
      ::h2::note_hip_error(e_, __FILE__, __LINE__); \
      return H2MI_EHIP;                             \
    }                                               \
  } while (0)

// a HIP call on a release / teardown path whose failure cannot change what the caller does next: the status is still
// looked at — recorded for h2mi_strerror and printed under H2MI_VERBOSE — instead of being dropped on the floor
#define H2_IGNORE(x)                                                      \
  do {                                                                    \
    hipError_t ei_ = (x);                                                 \
    if (ei_ != hipSuccess) ::h2::note_hip_error(ei_, __FILE__, __LINE__); \
  } while (0)

#define H2_REQUIRE_INIT()                        \
  do {                                           \
    if (!::h2::ctx().inited) return H2MI_ENODEV; \
    int rcb_ = ::h2::bind_thread();              \
    if (rcb_) return rcb_;                       \
  } while (0)

// Event-bracketed launch: when profiling is on, record a HIP event before and after the kernel on the
// stream it is launched on (device time of exactly this launch); otherwise a plain launch.
void prof_begin(const char* name, hipStream_t s);
void prof_end(hipStream_t s);
inline bool prof_on(const char* name) {
  Ctx& c = ctx();
  return c.profiling && (c.prof_filter.empty() || strncmp(name, c.prof_filter.c_str(), c.prof_filter.size()) == 0);
}

#define H2_LAUNCH(name, kernel, grid, block, shmem, stream, ...)                       \
  do {                                                                                 \
    const bool prof_ = ::h2::prof_on(name);                                            \
    if (prof_) ::h2::prof_begin(name, stream);                                         \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), shmem, stream, __VA_ARGS__);   \
    if (prof_) ::h2::prof_end(stream);                                                 \
    H2_HIP(hipGetLastError());                                                         \
  } while (0)

// device allocation released on every exit path of the synchronous helper entry points
struct DevMem {
  void* p = nullptr;
  ~DevMem() { if (p) H2_IGNORE(hipFree(p)); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// A device table built by kernels on one stream and read by kernels on any stream: the builder records an
// event, a consumer on another stream waits for it (same stream: in order, no wait needed).
struct Built {
  hipEvent_t ev = nullptr;
  hipStream_t on = nullptr;
  hipError_t mark(hipStream_t s) {
    if (!ev) {
      hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
    on = s;
    return hipEventRecord(ev, s);
  }
  hipError_t use(hipStream_t s) const { return (ev && s != on) ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
  void destroy() {
    if (ev) H2_IGNORE(hipEventDestroy(ev));
    ev = nullptr;
  }
};

// h2mi_core.hip: out[j] = sum over r < world of pts[r*k + j] (Jacobian, Montgomery-2^256), one launch on `s`
int launch_fold_groups(const uint8_t* pts, size_t world, size_t k, uint8_t* out, hipStream_t s);

// h2mi_msm.hip: make `s` wait for all outstanding MSM tails
int msm_join_all(hipStream_t s);
int msm_flush_all();
// h2mi_msm.hip, test hook only (csrc/h2mi_hooks.hip: h2mi_dbg_msm_snapshot): what the general pipeline left in the workspace slot of the
// handle's last MSM (back = 0) or of the back-th MSM before it (the phase entry's batches take consecutive slots).  Flushes the
// deferred reductions and synchronises the device, as h2mi_msm_last_stats does; host code only.  Geometry, then device pointers with
// their lengths: 32-bit words unless stated, partial sums of PART = 144 bytes.
struct MsmSnapshot {
  uint32_t c, W, nb, lb, nbins, logNl, logNh, seg_log, rows, has_sum, slot, last_small;
  uint64_t n, stride;             // registered points; payload row stride (n + 1: slot n of a row is the sum point)
  const uint32_t* s0_dev;         // [1] chunk length of the accumulation
  const uint32_t* off;            // [nb + 1] first entry of each bucket, [nb] = entries
  const uint32_t* np[2];          // [nb + 1] partials the accumulation leaves per bucket, fold tasks
  const uint32_t* toff[2];        // [nb + 1] their exclusive scans, [nb] = totals
  const uint32_t* vals1;          // [vals_cap] payloads in bucket order; off[nb] of them are this MSM's
  uint64_t vals_cap;              // stride * rows
  const uint8_t* dense;           // [nb] bucket sums
  const uint8_t *dense2, *vsum;   // wide windows: [nseg] plain and local weighted segment sums; else null
  uint64_t nseg;                  // 2^16 for wide windows, else 0
  const uint32_t* shift;          // [8] the dominant value this slot's last shifted MSM subtracted (Montgomery)
};
// Hidden: libh2mi.so does not export it, and the hook's call binds to the copy inside libh2mi_hooks.so (whose handles it knows) even
// when the product library is loaded beside it with global symbols.
__attribute__((visibility("hidden"))) int msm_debug_snapshot(uint64_t handle, int back, MsmSnapshot* out);
// The same for the small path (h2mi_dbg_msm_small_snapshot, h2mi_dbg_msm_small_table): geometry of the base set and of the slot's
// MSM, then device pointers.  H2MI_EINVAL when the slot's last MSM did not take the small path.  Host code only.
struct MsmSmallSnapshot {
  uint32_t sc, sW, slanes, sr, sG, small_n, G, slot;  // G = workgroups (partial sums) of this MSM over small_n <= n_reg points
  uint64_t n_reg;
  const uint8_t* sdig;    // [sW][n_reg] digit bytes, sign << 7 | magnitude
  const uint32_t* scnt;   // [sG + 1] entries per workgroup, [sG] = the arrival counter
  const uint8_t* spart;   // [sG] partial sums, G of them this MSM's
  const uint8_t* stable;  // [2^(sc-1)][sW][n_reg] affine multiples, 64 bytes each
};
__attribute__((visibility("hidden"))) int msm_debug_small_snapshot(uint64_t handle, int back, MsmSmallSnapshot* out);
// per-module teardown hooks of h2mi_shutdown (device memory, events and cached tables of the devices being released)
void msm_teardown();
void ntt_teardown();
void lookup_teardown();
void witness_teardown();

// The environment variables the library reads, each a plain getenv: H2MI_VERBOSE, H2MI_VIRTUAL_DEVICES, H2MI_MSM_C /
// H2MI_MSM_S0 / H2MI_MSM_NO_PIPELINE (forced-path parity tests) and H2MI_POWTAB_MAX.  No tuning variable is read.

inline uint32_t ceil_div_u32(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace h2
