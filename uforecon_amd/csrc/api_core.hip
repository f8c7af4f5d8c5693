// extern "C" surface of libufr.so (include/ufr.h): the process- and thread-wide state behind api_common.h --
// the error text, the matrix-precision default, the sticky range status and the profiling hooks.  The entry points
// themselves (api_*.hip) validate arguments, carve workspaces and sequence kernels on the caller's HIP stream: no torch
// types, no host<->device synchronisation.
#include <stdarg.h>
#include <stdio.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "api_common.h"

using namespace ufr;
using namespace ufr::api;

namespace {
thread_local char g_err[512] = "";

std::atomic<int> g_matrix_precision{UFR_PRECISION_FP32};   // what UFR_PRECISION_DEFAULT resolves to

// process-wide (the backward entry points are called from autograd's worker thread, not the caller's)
struct ProfEntry { const char* name; hipEvent_t a, b; };
std::atomic<bool> g_prof_on{false};
std::vector<ProfEntry> g_prof;
std::mutex g_prof_mu;
}  // namespace

namespace ufr::api {

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

bool resolve_precision(int precision, bool* lowp) {
  if (precision == UFR_PRECISION_DEFAULT) precision = g_matrix_precision.load(std::memory_order_relaxed);
  if (precision != UFR_PRECISION_FP32 && precision != UFR_PRECISION_16BIT) return false;
  *lowp = precision == UFR_PRECISION_16BIT;
  return true;
}

ProfScope::ProfScope(const char* n, hipStream_t st) : s(st), name(n) {
  if (g_prof_on.load(std::memory_order_relaxed)) {
    hipEventCreate(&a);
    hipEventCreate(&b);
    hipEventRecord(a, s);
  }
}
ProfScope::~ProfScope() {
  if (a) {
    hipEventRecord(b, s);
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof.push_back({name, a, b});
  }
}

// ---- sticky range status (include/ufr.h: ufr_status_poll): per device, created on first use (call_once: the entry points
// run on the caller's thread and on autograd's workers), never freed (process lifetime).
//   dev[0]  the bits the kernels OR into          dev[1]  generation tag, rewritten by every report-and-clear
//   host[0..1]  pinned copy of both words: written only by the D2H copies the entry points enqueue
// A report clears the reported bits on the device and starts a new generation; a copy that was already in flight then
// still delivers the OLD tag and is ignored -- without the tag it re-armed the host word with stale bits and a later,
// healthy call failed with UFR_ERR_RANGE (round-3 advisor finding).
struct StatusSlot {
  std::once_flag once;
  int rc = UFR_OK;
  int* dev = nullptr;
  volatile int* host = nullptr;
  std::atomic<int> gen{0};
  std::mutex report_mu;
  // recorded behind every report-and-clear kernel; the copies that deliver the words wait for it on THEIR stream, so a poll
  // on another stream than the one the last report was issued on cannot fetch the old tag and miss newly raised bits
  // (round-4 advisor finding: reports could be delayed or dropped across streams)
  hipEvent_t upd = nullptr;
  std::atomic<bool> upd_recorded{false};
};

}  // namespace ufr::api

namespace {
StatusSlot g_status[kMaxDevices];
constexpr int kStatusAll = 7;

__global__ void status_update_kernel(int* dev, int keep_mask, int gen) {
  atomicAnd(dev, keep_mask);
  dev[1] = gen;
}

int status_message(int bits, const char* who) {
  return fail(UFR_ERR_RANGE, "%s: range status 0x%x:%s%s%s (include/ufr.h: ufr_status_poll)", who, bits,
              (bits & 1) ? " a dense-layer input left the range of its fp16 planes (a token feature beyond the input_abs_max the weights were packed for -- ufr_weights_pack_for -- or infinite);" : "",
              (bits & 2) ? " NaN among the token / dir inputs handed to a transformer kernel;" : "",
              (bits & 4) ? " ufr_weights_pack met a parameter that is not finite (or an input bound that is not a positive finite number);" : "");
}

// what the last delivered copy says about the CURRENT generation, restricted to `mask`; reported bits are cleared on the
// device (enqueued on `s`) and a new generation starts
int status_consume(StatusSlot* sl, hipStream_t s, int mask, const char* who, int* flags_out) {
  std::lock_guard<std::mutex> lock(sl->report_mu);
  const int bits = sl->host[0], tag = sl->host[1];
  const int cur = sl->gen.load(std::memory_order_relaxed);
  const int hit = tag == cur ? bits & mask : 0;
  if (flags_out) *flags_out = tag == cur ? bits : 0;
  if (hit == 0) return UFR_OK;
  const int next = cur + 1;
  sl->gen.store(next, std::memory_order_relaxed);
  hipLaunchKernelGGL(status_update_kernel, dim3(1), dim3(1), 0, s, sl->dev, ~hit, next);
  UFR_HIP(hipGetLastError());
  if (sl->upd && hipEventRecord(sl->upd, s) == hipSuccess) sl->upd_recorded.store(true, std::memory_order_release);
  return status_message(hit, who);
}
}  // namespace

namespace ufr::api {

int status_slot(StatusSlot** out) {
  int dev = 0;
  UFR_HIP(hipGetDevice(&dev));
  UFR_REQUIRE(dev >= 0 && dev < kMaxDevices, "status: device %d out of range", dev);
  StatusSlot& sl = g_status[dev];
  std::call_once(sl.once, [&sl] {
    int* h = nullptr;
    int* d = nullptr;
    if (hipHostMalloc(reinterpret_cast<void**>(&h), 2 * sizeof(int), hipHostMallocDefault) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&d), 2 * sizeof(int)) != hipSuccess || hipMemset(d, 0, 2 * sizeof(int)) != hipSuccess) {
      sl.rc = UFR_ERR_HIP;
      return;
    }
    h[0] = h[1] = 0;
    sl.host = h;
    sl.dev = d;
    if (hipEventCreateWithFlags(&sl.upd, hipEventDisableTiming) != hipSuccess) sl.upd = nullptr;
  });
  if (sl.rc != UFR_OK) return fail(sl.rc, "status: could not allocate the device's status words");
  *out = &sl;
  return UFR_OK;
}

int status_begin(StatusSlot** out, hipStream_t s, const char* who) {
  UFR_CHECK(status_slot(out));
  return status_consume(*out, s, kStatusAll, who, nullptr);
}

int* status_word(StatusSlot* sl) { return sl->dev; }

int status_leave(StatusSlot* sl, hipStream_t s) {
  // behind the last report-and-clear, whatever stream issued it (a completed event costs nothing to wait for)
  if (sl->upd_recorded.load(std::memory_order_acquire)) UFR_HIP(hipStreamWaitEvent(s, sl->upd, 0));
  UFR_HIP(hipMemcpyAsync(const_cast<int*>(sl->host), sl->dev, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  return UFR_OK;
}

}  // namespace ufr::api

extern "C" {

int ufr_version(void) { return UFR_ABI_VERSION; }
const char* ufr_last_error(void) { return g_err; }

int ufr_set_matrix_precision(int mode) {
  UFR_REQUIRE(mode == UFR_PRECISION_FP32 || mode == UFR_PRECISION_16BIT, "ufr_set_matrix_precision: unknown mode %d", mode);
  g_matrix_precision.store(mode, std::memory_order_relaxed);
  return UFR_OK;
}
int ufr_get_matrix_precision(void) { return g_matrix_precision.load(std::memory_order_relaxed); }

int ufr_status_poll_bits(ufr_stream stream, int32_t synchronize, int32_t mask, int32_t* flags_out) {
  UFR_STATUS_SLOT(sl);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (synchronize) {
    UFR_CHECK(status_leave(sl, s));
    UFR_HIP(hipStreamSynchronize(s));
  }
  int flags = 0;
  const int rc = status_consume(sl, s, mask, "ufr_status_poll", &flags);
  if (flags_out) *flags_out = flags;
  if (rc == UFR_OK && !synchronize) return status_leave(sl, s);
  return rc;
}

int ufr_status_poll(ufr_stream stream, int32_t synchronize, int32_t* flags_out) {
  return ufr_status_poll_bits(stream, synchronize, kStatusAll, flags_out);
}

// ------------------------------------------------------------------ profiling hooks
void ufr_profile_enable(int on) {
  std::lock_guard<std::mutex> lock(g_prof_mu);
  for (auto& e : g_prof) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
  g_prof.clear();
  g_prof_on.store(on != 0, std::memory_order_relaxed);
}

int ufr_profile_read(const char** names, float* ms, int32_t* launches, int cap) {
  std::lock_guard<std::mutex> lock(g_prof_mu);
  int n = 0;
  for (auto& e : g_prof) {
    float t = 0.f;
    if (hipEventSynchronize(e.b) != hipSuccess || hipEventElapsedTime(&t, e.a, e.b) != hipSuccess) continue;
    int k = 0;
    for (; k < n; ++k)
      if (strcmp(names[k], e.name) == 0) break;
    if (k == n) {
      if (n >= cap) continue;
      names[n] = e.name; ms[n] = 0.f; launches[n] = 0; ++n;
    }
    ms[k] += t;
    launches[k] += 1;
  }
  for (auto& e : g_prof) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
  g_prof.clear();
  return n;
}

}  // extern "C"
