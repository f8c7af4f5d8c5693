// extern "C" surface of libufr.so (include/ufr.h): validation -- a frame's scores and previews, the ground-truth depth of a
// training view.
#include "api_common.h"

using namespace ufr;
using namespace ufr::api;

extern "C" {

size_t ufr_frame_metrics_workspace_bytes(int32_t /*n*/) {
  return align_up((size_t)kFrameMetricsBlocks * 8 * sizeof(double));
}

int ufr_frame_metrics(const float* rgb_c, const float* rgb_f, const float* rgb_gt, const float* depth_c, const float* depth_f,
                      const float* depth_gt, float near, float far, int32_t n, double* out8, void* workspace, ufr_stream stream) {
  const char* who = "ufr_frame_metrics";
  UFR_REQUIRE(rgb_c && rgb_f && rgb_gt && depth_c && depth_f && depth_gt && out8 && workspace, "%s: null argument", who);
  UFR_REQUIRE(n >= 1 && (long long)n * 3 < (1ll << 31), "%s: n=%d (1 <= n < 2^31 / 3)", who, n);
  UFR_REQUIRE(reinterpret_cast<uintptr_t>(out8) % 8 == 0 && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
              "%s: out8 and workspace must be aligned to 8 bytes", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("frame_metrics", s, launch_frame_metrics(rgb_c, rgb_f, rgb_gt, depth_c, depth_f, depth_gt, near, far, n, out8,
      static_cast<double*>(workspace), s));
  return UFR_OK;
}

int ufr_frame_preview_u8(const float* rgb, const float* depth, const double* depth_max, float depth_scale, int32_t n, uint8_t* rgb8,
                         uint8_t* depth8, ufr_stream stream) {
  const char* who = "ufr_frame_preview_u8";
  UFR_REQUIRE((rgb != nullptr) == (rgb8 != nullptr), "%s: rgb and rgb8 go together", who);
  UFR_REQUIRE((depth != nullptr) == (depth8 != nullptr) && (depth != nullptr) == (depth_max != nullptr),
              "%s: depth, depth_max and depth8 go together", who);
  UFR_REQUIRE(rgb || depth, "%s: nothing to do (rgb and depth are both null)", who);
  UFR_REQUIRE(n >= 1 && (long long)n * 3 < (1ll << 31), "%s: n=%d (1 <= n < 2^31 / 3)", who, n);
  UFR_REQUIRE(!depth || depth_scale > 0.f, "%s: depth_scale %g (must be > 0: the max of the scaled depths is the scaled max)", who,
              (double)depth_scale);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("frame_preview_u8", s, launch_frame_preview_u8(rgb, depth, depth_max, depth_scale, n, rgb8, depth8, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ the ground-truth depth of a training view
int ufr_depth_gt_prepare(const float* pfm, int32_t Hs, int32_t Ws, int32_t bottom_up, int32_t y0, int32_t x0, int32_t H, int32_t W,
                         float scale_factor, const double* cam_ray_z, float* depth, ufr_stream stream) {
  const char* who = "ufr_depth_gt_prepare";
  UFR_REQUIRE(pfm && cam_ray_z && depth, "%s: null argument", who);
  UFR_REQUIRE(Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "%s: source %dx%d, output %dx%d (each must be >= 1)", who, Hs, Ws, H, W);
  UFR_REQUIRE((long long)Hs * Ws < (1ll << 31), "%s: a source of %dx%d has 2^31 pixels or more", who, Hs, Ws);
  UFR_REQUIRE(bottom_up == 0 || bottom_up == 1, "%s: bottom_up %d (0 or 1)", who, bottom_up);
  // the half-size picture has rint(size / 2) rows and columns (half to even, as OpenCV rounds fx * size); its pixel k is
  // source pixel 2k, which that size keeps inside the source
  const long long Hh = (Hs + (Hs % 4 == 3 ? 1 : 0)) / 2, Wh = (Ws + (Ws % 4 == 3 ? 1 : 0)) / 2;
  UFR_REQUIRE(y0 >= 0 && x0 >= 0 && (long long)y0 + H <= Hh && (long long)x0 + W <= Wh,
              "%s: the crop %dx%d at (%d, %d) leaves the half-size picture %lldx%lld of a %dx%d source", who, H, W, y0, x0, Hh, Wh, Hs, Ws);
  UFR_REQUIRE(reinterpret_cast<uintptr_t>(cam_ray_z) % 8 == 0, "%s: cam_ray_z must be aligned to 8 bytes", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("depth_gt_prepare", s, launch_depth_gt(pfm, Hs, Ws, bottom_up, y0, x0, H, W, scale_factor, cam_ray_z, depth, s));
  return UFR_OK;
}

}  // extern "C"
