// Depth-map fusion to a point cloud by geometric consistency (the reference's code1/encoder_utils/depth_fusion.py) on the
// device, with the arithmetic that tests/depth_fusion_ref.py restates (include/ufr.h, ufr_depth_*):
//
//   depth_consistency   one launch per reference view, one thread per reference pixel, a loop over the S source views.  Per
//          pair it is reproject_with_depth + check_geometric_consistency (depth_fusion.py:35-90) in fp64, narrowed to fp32
//          exactly where numpy narrows: x_src / y_src, the sampled source depth, depth_reprojected, x / y_reprojected, and
//          depth_diff / relative_depth_diff (fp32 - fp32, fp32 / fp32, compared in fp32 with the threshold rounded to fp32 as
//          numpy 2 does).  dist is fp64 of (fp32 coordinate - integer pixel index); + 1e-6 goes to the reprojection
//          denominator only (:68).  The masked depth_reprojected are summed in fp32 in source order (Python's sum()), the
//          reference depth is added in fp32, and the division by geo_mask_sum + 1 is fp64 (fp32 / int32 in numpy).
//          The six small matrices of a pair come from the host (fp32 LAPACK inverses cannot be reproduced here); the
//          table is wave-uniform, so it is read through the scalar cache.
//   remap_bilinear      cv2.remap(src, x, y, INTER_LINEAR) with the default constant-0 border, restated from OpenCV's source
//          (imgproc/src/imgwarp.cpp, remapBilinear and the fixed-point map conversion): coordinates to 1/32 pixel by
//          round-half-even of x * 32, integer part = arithmetic shift by 5 saturated to int16, fraction = the low 5 bits;
//          weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx*fy formed in fp32; the four products summed in fp32 in that order; a
//          tap outside the image reads 0, per tap.  A non-finite coordinate, or one whose x * 32 does not fit int32, is
//          tested explicitly and gives 0 (on x86 OpenCV's conversion yields INT_MIN there, which saturates to -32768: all
//          four taps outside).  NOT COMPARED WITH A REAL OpenCV: none exists where this was written.  It is one function so
//          that there is one place to check.  Every tap index is bounds-checked before the load.
//   depth_points_count / _scan / _emit   the ordered compaction of compact.h over the valid pixels of one reference view,
//          with block_rank as the block scan: pixel i's slot is block offset + lower waves + lower lanes: row-major pixel
//          order, the order x[valid_points] gives.  xyz = inv(E_ref) [inv(K_ref) (x, y, 1) depth ; 1] in
//          fp64 (:209-212), narrowed to fp32; rgb the 8-bit image value ((v / 255f) * 255f truncates back to v for every
//          v in 0..255).  No atomics; every output store is guarded by the caller's capacity.
//
// Block shape: 256 threads (4 waves), no LDS in the consistency kernel, 16 B of it in the compaction kernels.  The
// consistency kernel is a chain of fp64 3x3 products around four dependent 4-byte gathers per pair: latency bound, so what
// matters is waves in flight, and nothing here limits them but registers.
#include "compact.h"
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kDfThreads = 256;

// offsets of the six row-major matrices in a pair's record of UFR_DEPTH_PAIR_DOUBLES doubles
constexpr int kInvKRef = 0, kSrcFromRef = 9, kKSrc = 25, kInvKSrc = 34, kRefFromSrc = 43, kKRef = 59;
static_assert(kKRef + 9 == UFR_DEPTH_PAIR_DOUBLES, "record layout and ufr.h disagree");

struct Sources {   // by value in the kernel arguments: wave-uniform
  const float* depth[UFR_DEPTH_MAX_SOURCES];
  int h[UFR_DEPTH_MAX_SOURCES], w[UFR_DEPTH_MAX_SOURCES];
};

struct PointsCam {
  double inv_k[9], inv_e[16];
};

__device__ inline float tap(const float* __restrict__ src, int h, int w, int x, int y) {
  return (x >= 0 && x < w && y >= 0 && y < h) ? src[(long long)y * w + x] : 0.f;
}

// cv2.remap(src, x, y, INTER_LINEAR), borderMode = BORDER_CONSTANT, borderValue = 0, for one pixel (see the file header)
__device__ inline float remap_bilinear(const float* __restrict__ src, int h, int w, float x, float y) {
  const float x32 = x * 32.f, y32 = y * 32.f;
  // non-finite or beyond int32 (|x| >= 2^26): outside the image whatever the conversion would give
  if (!(fabsf(x32) < 2147483648.f) || !(fabsf(y32) < 2147483648.f)) return 0.f;
  const int sx = (int)rintf(x32), sy = (int)rintf(y32);              // rintf: round half to even
  int ix = sx >> 5, iy = sy >> 5;                                     // arithmetic shift: floor
  ix = ix < -32768 ? -32768 : (ix > 32767 ? 32767 : ix);
  iy = iy < -32768 ? -32768 : (iy > 32767 ? 32767 : iy);
  const float fx = (float)(sx & 31) * (1.f / 32.f), fy = (float)(sy & 31) * (1.f / 32.f);
  const float w00 = (1.f - fx) * (1.f - fy), w01 = fx * (1.f - fy), w10 = (1.f - fx) * fy, w11 = fx * fy;
  const float v00 = tap(src, h, w, ix, iy), v01 = tap(src, h, w, ix + 1, iy);
  const float v10 = tap(src, h, w, ix, iy + 1), v11 = tap(src, h, w, ix + 1, iy + 1);
  return ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11;
}

// row i of a row-major 3x3 times (a, b, c), left to right
__device__ inline double row3(const double* __restrict__ m, int i, double a, double b, double c) {
  return (m[3 * i] * a + m[3 * i + 1] * b) + m[3 * i + 2] * c;
}

// row i of a row-major 4x4 times (a, b, c, 1), left to right
__device__ inline double row4(const double* __restrict__ m, int i, double a, double b, double c) {
  return ((m[4 * i] * a + m[4 * i + 1] * b) + m[4 * i + 2] * c) + m[4 * i + 3] * 1.0;
}

__global__ void __launch_bounds__(kDfThreads) depth_consistency_kernel(const float* __restrict__ ref, int H, int W, Sources src,
                                                                        const double* __restrict__ mats, int S, double pix_thres,
                                                                        float depth_thres, int mask_thres,
                                                                        int* __restrict__ mask_sum, unsigned char* __restrict__ mask,
                                                                        double* __restrict__ depth_avg,
                                                                        unsigned char* __restrict__ pair_masks) {
  const long long n = (long long)H * W;
  const long long i = (long long)blockIdx.x * kDfThreads + threadIdx.x;
  if (i >= n) return;
  const int yi = (int)(i / W), xi = (int)(i - (long long)yi * W);
  const float d_ref = ref[i];
  const double xr = (double)xi, yr = (double)yi, dd = (double)d_ref;
  const double a0 = xr * dd, a1 = yr * dd, a2 = 1.0 * dd;                   // (x, y, 1) * depth
  int cnt = 0;
  float acc = 0.f;
  for (int s = 0; s < S; ++s) {
    const double* __restrict__ m = mats + (size_t)s * UFR_DEPTH_PAIR_DOUBLES;
    // reference pixel -> reference camera -> source camera -> source pixel (:42-49)
    const double p0 = row3(m + kInvKRef, 0, a0, a1, a2), p1 = row3(m + kInvKRef, 1, a0, a1, a2), p2 = row3(m + kInvKRef, 2, a0, a1, a2);
    const double q0 = row4(m + kSrcFromRef, 0, p0, p1, p2), q1 = row4(m + kSrcFromRef, 1, p0, p1, p2),
                 q2 = row4(m + kSrcFromRef, 2, p0, p1, p2);
    const double k0 = row3(m + kKSrc, 0, q0, q1, q2), k1 = row3(m + kKSrc, 1, q0, q1, q2), k2 = row3(m + kKSrc, 2, q0, q1, q2);
    const double xs = k0 / k2, ys = k1 / k2;
    const float sampled = remap_bilinear(src.depth[s], src.h[s], src.w[s], (float)xs, (float)ys);   // (:53-55)
    // source pixel with the sampled depth -> source camera -> reference camera -> reference pixel (:60-70)
    const double sd = (double)sampled;
    const double b0 = xs * sd, b1 = ys * sd, b2 = 1.0 * sd;
    const double u0 = row3(m + kInvKSrc, 0, b0, b1, b2), u1 = row3(m + kInvKSrc, 1, b0, b1, b2), u2 = row3(m + kInvKSrc, 2, b0, b1, b2);
    const double r0 = row4(m + kRefFromSrc, 0, u0, u1, u2), r1 = row4(m + kRefFromSrc, 1, u0, u1, u2),
                 r2 = row4(m + kRefFromSrc, 2, u0, u1, u2);
    const float d_rep = (float)r2;
    const double e0 = row3(m + kKRef, 0, r0, r1, r2), e1 = row3(m + kKRef, 1, r0, r1, r2), e2 = row3(m + kKRef, 2, r0, r1, r2);
    const double den = e2 + 1e-6;
    const float x_rep = (float)(e0 / den), y_rep = (float)(e1 / den);
    // (:82-87)
    const double dx = (double)x_rep - xr, dy = (double)y_rep - yr;
    const double dist = __dsqrt_rn(dx * dx + dy * dy);
    const float rel = __fdiv_rn(fabsf(d_rep - d_ref), d_ref);
    const bool ok = dist < pix_thres && rel < depth_thres;                   // NaN compares false: inconsistent
    if (ok) {
      ++cnt;
      acc = acc + d_rep;
    }
    if (pair_masks) pair_masks[(long long)s * n + i] = ok ? 1 : 0;
  }
  mask_sum[i] = cnt;
  mask[i] = cnt >= mask_thres ? 1 : 0;
  depth_avg[i] = (double)(acc + d_ref) / (double)(cnt + 1);
}

// ------------------------------------------------------------------ ordered compaction of the valid pixels
__global__ void __launch_bounds__(kDfThreads) depth_points_count_kernel(const unsigned char* __restrict__ mask, long long n,
                                                                         long long* __restrict__ block_tot) {
  __shared__ int lds[kDfThreads / 64];
  const long long i = (long long)blockIdx.x * kDfThreads + threadIdx.x;
  int total;
  block_rank<kDfThreads>(i < n && mask[i] != 0, lds, &total);
  if (threadIdx.x == 0) block_tot[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kDfThreads) depth_points_emit_kernel(const unsigned char* __restrict__ mask,
                                                                        const double* __restrict__ depth_avg,
                                                                        const unsigned char* __restrict__ color, int H, int W,
                                                                        PointsCam cam, const long long* __restrict__ block_off,
                                                                        float* __restrict__ xyz, unsigned char* __restrict__ rgb,
                                                                        long long capacity) {
  __shared__ int lds[kDfThreads / 64];
  const long long n = (long long)H * W;
  const long long i = (long long)blockIdx.x * kDfThreads + threadIdx.x;
  const bool valid = i < n && mask[i] != 0;
  int total;
  const int rank = block_rank<kDfThreads>(valid, lds, &total);
  if (!valid) return;
  const long long o = block_off[blockIdx.x] + rank;
  if (o < 0 || o >= capacity) return;
  const int yi = (int)(i / W), xi = (int)(i - (long long)yi * W);
  const double d = depth_avg[i];
  const double a0 = (double)xi * d, a1 = (double)yi * d, a2 = 1.0 * d;
  const double p0 = row3(cam.inv_k, 0, a0, a1, a2), p1 = row3(cam.inv_k, 1, a0, a1, a2), p2 = row3(cam.inv_k, 2, a0, a1, a2);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    xyz[3 * o + k] = (float)row4(cam.inv_e, k, p0, p1, p2);
    rgb[3 * o + k] = color[3 * i + k];
  }
}

}  // namespace

long long depth_points_blocks(long long n) { return (n + kDfThreads - 1) / kDfThreads; }

hipError_t launch_depth_consistency(const float* ref, int H, int W, const float* const* src_depth, const int* src_hw,
                                    const double* mats, int S, double pix_thres, float depth_thres, int mask_thres, int* mask_sum,
                                    unsigned char* mask, double* depth_avg, unsigned char* pair_masks, hipStream_t s) {
  Sources src;
  for (int k = 0; k < UFR_DEPTH_MAX_SOURCES; ++k) {
    src.depth[k] = k < S ? src_depth[k] : nullptr;
    src.h[k] = k < S ? src_hw[2 * k] : 0;
    src.w[k] = k < S ? src_hw[2 * k + 1] : 0;
  }
  const long long n = (long long)H * W;
  hipLaunchKernelGGL(depth_consistency_kernel, dim3((unsigned)depth_points_blocks(n)), dim3(kDfThreads), 0, s, ref, H, W, src, mats, S,
                     pix_thres, depth_thres, mask_thres, mask_sum, mask, depth_avg, pair_masks);
  return hipGetLastError();
}

hipError_t launch_depth_points_count(const unsigned char* mask, long long n, long long* block_tot, long long* block_off,
                                     long long* total, hipStream_t s) {
  const long long blocks = depth_points_blocks(n);
  hipLaunchKernelGGL(depth_points_count_kernel, dim3((unsigned)blocks), dim3(kDfThreads), 0, s, mask, n, block_tot);
  return launch_scan_totals<1>(block_tot, blocks, block_off, total, s);
}

hipError_t launch_depth_points_emit(const unsigned char* mask, const double* depth_avg, const unsigned char* color, int H, int W,
                                    const double* inv_k, const double* inv_e, const long long* block_off, float* xyz,
                                    unsigned char* rgb, long long capacity, hipStream_t s) {
  PointsCam cam;
  for (int k = 0; k < 9; ++k) cam.inv_k[k] = inv_k[k];
  for (int k = 0; k < 16; ++k) cam.inv_e[k] = inv_e[k];
  const long long n = (long long)H * W;
  hipLaunchKernelGGL(depth_points_emit_kernel, dim3((unsigned)depth_points_blocks(n)), dim3(kDfThreads), 0, s, mask, depth_avg, color,
                     H, W, cam, block_off, xyz, rgb, capacity);
  return hipGetLastError();
}

}  // namespace ufr
