// What api_geometry.hip and api_mesh.hip share: the count limit, the checks, the scan workspace and the small host helpers that
// entry points on both sides use.  Host only.
#pragma once
#include "api_common.h"

namespace ufr::api {

constexpr long long kChMax = (1ll << 31) - 1;   // most items (points, vertices, faces, pixels) an int32 index reaches

// the counts a scan left in a workspace, on the host: the one synchronisation of a count / emit pair
inline int read_counts(long long* host, const long long* dev, int n, hipStream_t s) {
  UFR_HIP(hipMemcpyAsync(host, dev, n * sizeof(long long), hipMemcpyDeviceToHost, s));
  UFR_HIP(hipStreamSynchronize(s));
  return UFR_OK;
}

inline int cell_grid_check(const char* who, double cell, const double* origin) {
  UFR_REQUIRE(cell > 0.0 && std::isfinite(cell) && std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]),
              "%s: cell %g, origin (%g, %g, %g) (cell must be positive, all finite)", who, cell, origin[0], origin[1], origin[2]);
  return UFR_OK;
}

inline int depth_image_check(const char* who, int32_t H, int32_t W) {
  UFR_REQUIRE(H >= 1 && W >= 1, "%s: image %dx%d (H and W must be >= 1)", who, H, W);
  UFR_REQUIRE((long long)H * W < (1ll << 31), "%s: image %dx%d has 2^31 pixels or more", who, H, W);
  return UFR_OK;
}

// every ordered compaction (voxel means, depth points, the simplifier's scans): [block sums int64 | block offsets int64 | total int64]
struct ScanWs { long long *block_tot, *block_off, *total; };
inline ScanWs carve_scan(Carver& c, size_t blocks) {
  ScanWs w;
  w.block_tot = c.take<long long>(blocks);
  w.block_off = c.take<long long>(blocks);
  w.total = c.take<long long>(1);
  return w;
}

inline bool invert3(const double* m, double* o) {
  const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
  if (!(det != 0.0) || !std::isfinite(det)) return false;
  o[0] = c0 / det, o[1] = (m[2] * m[7] - m[1] * m[8]) / det, o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  o[3] = c1 / det, o[4] = (m[0] * m[8] - m[2] * m[6]) / det, o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  o[6] = c2 / det, o[7] = (m[1] * m[6] - m[0] * m[7]) / det, o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(o[i])) return false;
  return true;
}

// rot, org of a host fp32 c2w, and the fp64 inverse of the fp32 ray generator: pixel ~ inv(k_inv) inv(R) (X - o)
inline int hit_camera(const char* who, const float* k_inv, const float* c2w, float* rot, float* org, double* proj) {
  double ki[9], r[9], kf[9], rw[9], m[9];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) rot[3 * i + j] = c2w[4 * i + j], r[3 * i + j] = (double)c2w[4 * i + j], ki[3 * i + j] = (double)k_inv[3 * i + j];
    org[i] = c2w[4 * i + 3];
  }
  UFR_REQUIRE(invert3(ki, kf) && invert3(r, rw), "%s: k_inv or the rotation of c2w is singular or not finite", who);
  UFR_REQUIRE(std::isfinite(org[0]) && std::isfinite(org[1]) && std::isfinite(org[2]), "%s: the camera centre is not finite", who);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m[3 * i + j] = kf[3 * i] * rw[j] + kf[3 * i + 1] * rw[3 + j] + kf[3 * i + 2] * rw[6 + j];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) proj[4 * i + j] = m[3 * i + j];
    proj[4 * i + 3] = -(m[3 * i] * (double)org[0] + m[3 * i + 1] * (double)org[1] + m[3 * i + 2] * (double)org[2]);
  }
  return UFR_OK;
}

// what both frame renderers take: a base colour (null: white; each channel 0 .. 1) and a background (null: white)
inline int frame_colors(const char* who, const float* base_color, const uint8_t* background, double* base, unsigned char* bg) {
  for (int k = 0; k < 3; ++k) {
    base[k] = base_color ? (double)base_color[k] : 1.0;
    bg[k] = background ? background[k] : 255;
    UFR_REQUIRE(base[k] >= 0.0 && base[k] <= 1.0, "%s: base colour %g (must be 0 .. 1)", who, base[k]);
  }
  return UFR_OK;
}

}  // namespace ufr::api
