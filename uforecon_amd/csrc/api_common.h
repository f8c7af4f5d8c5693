// What the entry-point files of libufr.so (api_*.hip) share: error reporting, workspace carving, the status, precision
// and profiling interfaces of api_core.hip, and the argument checks that repeat.  Host only: no kernel file includes it.
#pragma once
#include <math.h>
#include <string.h>

#include "ufr_internal.h"

namespace ufr::api {

// writes the calling thread's ufr_last_error() text (one buffer per thread, api_core.hip) and returns `code`
int fail(int code, const char* fmt, ...);
#define UFR_HIP(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return ::ufr::api::fail(UFR_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define UFR_REQUIRE(cond, ...)                                       \
  do {                                                               \
    if (!(cond)) return ::ufr::api::fail(UFR_ERR_ARG, __VA_ARGS__);  \
  } while (0)
#define UFR_CHECK(call) do { if (int rc_ = (call)) return rc_; } while (0)   // pass a failed call's code on

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Bump allocator over a caller workspace.  Every workspace has ONE carve_* function that lays its regions out: the
// *_workspace_bytes query runs it over a null base (null regions, `off` = the size), the entry point over the caller's pointer.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* p) : base(static_cast<char*>(p)) {}
  template <class T>
  T* take(size_t n) {
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align_up(n * sizeof(T));
    return r;
  }
  float* f32(size_t n) { return take<float>(n); }
};
template <class F, class... A>
size_t carved_bytes(F carve, A... args) {   // what a *_workspace_bytes query returns
  Carver c(nullptr);
  carve(c, args...);
  return c.off;
}

// optional per-kernel timing with HIP events on the caller's stream (ufr_profile_enable / ufr_profile_read)
struct ProfScope {
  hipStream_t s;
  hipEvent_t a = nullptr, b = nullptr;
  const char* name;
  ProfScope(const char* n, hipStream_t st);
  ~ProfScope();
};
#define UFR_TIMED(name, s, call) do { ::ufr::api::ProfScope p_(name, s); UFR_HIP(call); } while (0)   // one timed launch

// precision argument of an entry point -> "reduced" flag of the launchers; false + error for an unknown value
bool resolve_precision(int precision, bool* lowp);
// (declares `lowp_var` and may return: a statement pair, for block scope only -- never under an unbraced if)
#define UFR_PRECISION(arg, lowp_var, who) \
  bool lowp_var = false;                  \
  if (!::ufr::api::resolve_precision(arg, &lowp_var)) return ::ufr::api::fail(UFR_ERR_ARG, "%s: unknown precision %d", who, (int)(arg))

// ---- sticky range status of the calling thread's device (include/ufr.h: ufr_status_poll; the protocol: api_core.hip)
struct StatusSlot;
int status_slot(StatusSlot** out);                                    // the slot, created on first use
int status_begin(StatusSlot** out, hipStream_t s, const char* who);   // ... and entry of a compute call: report (and clear) what an earlier call's copy delivered
int* status_word(StatusSlot* sl);                                     // device word the kernels OR their bits into
int status_leave(StatusSlot* sl, hipStream_t s);                      // exit of a compute call: deliver the words as of the end of this call's kernels
// the two forms every entry point uses; each DECLARES `sl` and may return: block scope only, never under an unbraced if
#define UFR_STATUS_SLOT(sl) ::ufr::api::StatusSlot* sl = nullptr; UFR_CHECK(::ufr::api::status_slot(&sl))
#define UFR_STATUS_ENTER(sl, s, who) ::ufr::api::StatusSlot* sl = nullptr; UFR_CHECK(::ufr::api::status_begin(&sl, s, who))

constexpr int kMaxDevices = 16;   // per-device state (status slots, side-stream pools) is kept in arrays of this length

inline PreSim presim_of(const ufr_raw_weights* r) {
  return PreSim{r->pre_sim.w0, r->pre_sim.b0, r->pre_sim.w2, r->pre_sim.b2, r->pre_sim.w4, r->pre_sim.b4};
}

inline const FrameDev* frame_of(const ufr_frame* f) {
  const FrameDev* d = reinterpret_cast<const FrameDev*>(f);
  return (f && d->magic == kFrameMagic) ? d : nullptr;
}

// ---- the checks that repeat; `who` is the entry point's name
inline bool views_ok(int NV) { return NV >= 2 && NV <= UFR_MAX_VIEWS; }
inline int check_views(const char* who, int NV) {
  UFR_REQUIRE(views_ok(NV), "%s: NV=%d unsupported (2..%d)", who, NV, UFR_MAX_VIEWS);
  return UFR_OK;
}
// what the ray transformer takes: whole 16-sample tiles, at most 16 of them
inline int check_ray_samples(const char* who, int RN, int SN) {
  UFR_REQUIRE(RN > 0 && SN >= 16 && SN % 16 == 0 && SN <= 256, "%s: SN=%d must be a multiple of 16 in [16,256]", who, SN);
  return UFR_OK;
}
inline int check_conv3d_mode(const char* who, int mode) {
  UFR_REQUIRE(mode == UFR_CONV3D_S1 || mode == UFR_CONV3D_S2 || mode == UFR_CONV3D_T2, "%s: unknown mode %d", who, mode);
  return UFR_OK;
}
inline int check_workspace(const char* who, size_t have, size_t need) {
  if (have < need) return fail(UFR_ERR_WORKSPACE, "%s: workspace too small: %zu < %zu bytes", who, have, need);
  return UFR_OK;
}

}  // namespace ufr::api
