// extern "C" surface of libufr.so (include/ufr.h), the training step's own entry points: the optimizer update and the ray draw.
#include "api_common.h"

using namespace ufr;
using namespace ufr::api;

namespace {

SelectWorkspace carve_select(Carver& c, int n, int k) {
  SelectWorkspace w;
  const size_t blocks = (size_t)select_compact_blocks(n);
  w.hist = c.take<uint32_t>(3 * 2048 + 4);
  w.totals = c.take<int>(2 * blocks);
  w.off = c.take<long long>(2 * blocks);
  w.grand = c.take<long long>(2);
  w.cand = c.take<unsigned long long>((size_t)k);
  return w;
}

bool select_range_ok(int n, int k) { return n >= 1 && n <= (1 << 24) && k >= 1 && k <= kSelectMaxK && k <= n; }

}  // namespace

extern "C" {

int32_t ufr_adam_table_capacity(void) { return kAdamTableCap; }

int ufr_adam_step(const ufr_adam_tensor* tensors, int32_t n_tensors, double lr, double beta1, double beta2, double eps,
                  ufr_stream stream) {
  const char* who = "ufr_adam_step";
  UFR_REQUIRE(n_tensors >= 0 && (tensors || n_tensors == 0), "%s: null table with n_tensors=%d", who, n_tensors);
  UFR_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
              "%s: lr %g, betas (%g, %g), eps %g (lr, eps >= 0; 0 <= beta < 1)", who, lr, beta1, beta2, eps);
  for (int i = 0; i < n_tensors; ++i) {
    const ufr_adam_tensor& t = tensors[i];
    UFR_REQUIRE(t.numel >= 0 && t.numel < (1ll << 31), "%s: tensor %d has numel %lld (0 <= numel < 2^31)", who, i, (long long)t.numel);
    UFR_REQUIRE(t.numel == 0 || (t.param && t.grad && t.exp_avg && t.exp_avg_sq), "%s: tensor %d: null pointer", who, i);
    UFR_REQUIRE(((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) | reinterpret_cast<uintptr_t>(t.exp_avg) |
                  reinterpret_cast<uintptr_t>(t.exp_avg_sq)) & 3u) == 0, "%s: tensor %d: a pointer is not aligned to 4 bytes", who, i);
    UFR_REQUIRE(t.bias_correction1 > 0.0 && t.bias_correction1 <= 1.0 && t.bias_correction2 > 0.0 && t.bias_correction2 <= 1.0,
                "%s: tensor %d: bias corrections %g, %g (each 1 - beta^step, in (0, 1])", who, i, t.bias_correction1, t.bias_correction2);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n_tensors; i += kAdamTableCap)      // ceil(n_tensors / capacity) launches
    UFR_TIMED("adam_step", s, launch_adam(tensors + i, n_tensors - i < kAdamTableCap ? n_tensors - i : kAdamTableCap, lr, beta1, beta2, eps, s));
  return UFR_OK;
}

size_t ufr_select_rays_workspace_bytes(int32_t n, int32_t k) {
  if (!select_range_ok(n, k)) {
    fail(UFR_ERR_ARG, "ufr_select_rays_workspace_bytes: n=%d, k=%d (1 <= k <= min(n, %d), n <= 2^24)", n, k, kSelectMaxK);
    return 0;
  }
  return carved_bytes(carve_select, (int)n, (int)k);
}

int ufr_select_rays(const float* u, int32_t n, int32_t k, int64_t* idx_out, void* workspace, size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_select_rays";
  UFR_REQUIRE(select_range_ok(n, k), "%s: n=%d, k=%d (1 <= k <= min(n, %d), n <= 2^24)", who, n, k, kSelectMaxK);
  UFR_REQUIRE(u && idx_out && workspace, "%s: null argument", who);
  UFR_REQUIRE(reinterpret_cast<uintptr_t>(u) % 4 == 0 && reinterpret_cast<uintptr_t>(idx_out) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: u must be aligned to 4 bytes, idx_out and workspace to 8", who);
  Carver c(workspace);
  const SelectWorkspace w = carve_select(c, n, k);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("select_rays", s, launch_select_rays(u, n, k, reinterpret_cast<long long*>(idx_out), w, s));
  return UFR_OK;
}

}  // extern "C"
