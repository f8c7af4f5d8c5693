// The scores and the preview bytes of one validation frame (the reference's UFORecon.validation_step, code1/model.py:708-726
// and :731-742; include/ufr.h, ufr_frame_metrics / ufr_frame_preview_u8).  Streaming kernels: no matrix cores.
//
//   frame_metrics_partial   one pass over the frame.  min(256, ceil(n / 256)) blocks of 256 threads walk the n rays with a
//          grid stride; a thread reads a ray's two colours (3 consecutive floats each), the three planar ground-truth values
//          (coalesced along the ray index) and the three depths, forms every difference in double and keeps eight double
//          partials: sum (x - y)^2 coarse / fine, the same of the clamped values, sum |d - d_gt| coarse / fine over the valid
//          pixels, their count, and the running max of the coarse depth.  The partials are reduced across the 64 lanes with
//          __shfl_down (lane l takes lane l + off: a fixed tree), then the four waves' values are added in wave order through
//          LDS, and the block stores its row of eight doubles.
//   frame_metrics_finish    one block: thread v < 8 adds column v of the rows in row order; thread 0 then divides, takes the
//          logarithms and stores out8.
//          Nothing is accumulated with atomics, and the grid is a function of n alone, so the same inputs give the same bits.
//   frame_preview_u8        one thread per ray: three colour bytes and one depth byte, in the reference's fp32 arithmetic.
//
// NaN: a comparison with NaN is false, so clamp() written with comparisons keeps a NaN colour, a NaN depth_gt fails the mask,
// and a NaN depth enters the L1 sum and the max as torch and numpy have it.
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kFmThreads = 256;
constexpr int kFmWaves = kFmThreads / 64;
constexpr int kFmVals = 8;

__device__ inline float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }
// the larger of two values, NaN winning over everything (np.max)
__device__ inline double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

__global__ void __launch_bounds__(kFmThreads) frame_metrics_partial_kernel(
    const float* __restrict__ rgb_c, const float* __restrict__ rgb_f, const float* __restrict__ rgb_gt,
    const float* __restrict__ depth_c, const float* __restrict__ depth_f, const float* __restrict__ depth_gt, float near_z,
    float far_z, int n, double* __restrict__ rows) {
  double acc[kFmVals];
#pragma unroll
  for (int v = 0; v < 7; ++v) acc[v] = 0.0;
  acc[7] = -__builtin_inf();
  const long long stride = (long long)gridDim.x * kFmThreads;
  for (long long i = (long long)blockIdx.x * kFmThreads + threadIdx.x; i < n; i += stride) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float y = rgb_gt[(long long)c * n + i];
      const float xc = rgb_c[3 * i + c], xf = rgb_f[3 * i + c];
      const double dc = (double)xc - (double)y, df = (double)xf - (double)y;
      acc[0] += dc * dc;
      acc[1] += df * df;
      const float yk = clamp01(y);
      const double kc = (double)clamp01(xc) - (double)yk, kf = (double)clamp01(xf) - (double)yk;
      acc[2] += kc * kc;
      acc[3] += kf * kf;
    }
    const float g = depth_gt[i], zc = depth_c[i];
    if (g != 0.f && g >= near_z && g <= far_z) {   // model.py:719
      acc[4] += fabs((double)zc - (double)g);
      acc[5] += fabs((double)depth_f[i] - (double)g);
      acc[6] += 1.0;
    }
    acc[7] = max_nan(acc[7], (double)zc);
  }
  // across the wave: lane l += lane l + off, off = 32 .. 1
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int v = 0; v < 7; ++v) acc[v] += __shfl_down(acc[v], off, 64);
    acc[7] = max_nan(acc[7], __shfl_down(acc[7], off, 64));
  }
  __shared__ double part[kFmWaves][kFmVals];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int v = 0; v < kFmVals; ++v) part[wave][v] = acc[v];
  }
  __syncthreads();
  if (threadIdx.x < kFmVals) {
    const int v = threadIdx.x;
    double t = part[0][v];
    for (int w = 1; w < kFmWaves; ++w) t = v == 7 ? max_nan(t, part[w][v]) : t + part[w][v];
    rows[(long long)blockIdx.x * kFmVals + v] = t;
  }
}

__global__ void __launch_bounds__(64) frame_metrics_finish_kernel(const double* __restrict__ rows, int n_rows, int n,
                                                                   double* __restrict__ out8) {
  __shared__ double tot[kFmVals];
  if (threadIdx.x < kFmVals) {
    const int v = threadIdx.x;
    double t = rows[v];
    for (int r = 1; r < n_rows; ++r) t = v == 7 ? max_nan(t, rows[r * kFmVals + v]) : t + rows[r * kFmVals + v];
    tot[v] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double m = 3.0 * (double)n;
    out8[0] = tot[0] / m;
    out8[1] = tot[1] / m;
    out8[2] = -10.0 * log10(tot[2] / m + 1e-8);
    out8[3] = -10.0 * log10(tot[3] / m + 1e-8);
    out8[4] = tot[6] > 0.0 ? tot[4] / tot[6] : 0.0;
    out8[5] = tot[6] > 0.0 ? tot[5] / tot[6] : 0.0;
    out8[6] = tot[6];
    out8[7] = tot[7];
  }
}

// numpy's float32 -> uint8 cast: truncate towards zero, keep the low 8 bits
__device__ inline unsigned char to_u8(float v) { return (unsigned char)((int)v & 255); }

__global__ void __launch_bounds__(kFmThreads) frame_preview_kernel(const float* __restrict__ rgb, const float* __restrict__ depth,
                                                                    const double* __restrict__ depth_max, float depth_scale, int n,
                                                                    unsigned char* __restrict__ rgb8, unsigned char* __restrict__ depth8) {
  const long long i = (long long)blockIdx.x * kFmThreads + threadIdx.x;
  if (i >= n) return;
  if (rgb) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb8[3 * i + c] = to_u8(rgb[3 * i + c] * 255.f);          // model.py:731
  }
  if (depth) {
    const float top = (float)depth_max[0] * depth_scale;                                    // np.max(depths * scale), scale > 0
    depth8[i] = to_u8(__fdiv_rn(depth[i] * depth_scale, top) * 255.f);                      // model.py:734, :742
  }
}

}  // namespace

hipError_t launch_frame_metrics(const float* rgb_c, const float* rgb_f, const float* rgb_gt, const float* depth_c, const float* depth_f,
                                const float* depth_gt, float near_z, float far_z, int n, double* out8, double* rows, hipStream_t s) {
  int blocks = (n + kFmThreads - 1) / kFmThreads;
  if (blocks > kFrameMetricsBlocks) blocks = kFrameMetricsBlocks;
  hipLaunchKernelGGL(frame_metrics_partial_kernel, dim3(blocks), dim3(kFmThreads), 0, s, rgb_c, rgb_f, rgb_gt, depth_c, depth_f,
                     depth_gt, near_z, far_z, n, rows);
  hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3(1), dim3(64), 0, s, rows, blocks, n, out8);
  return hipGetLastError();
}

hipError_t launch_frame_preview_u8(const float* rgb, const float* depth, const double* depth_max, float depth_scale, int n,
                                   unsigned char* rgb8, unsigned char* depth8, hipStream_t s) {
  hipLaunchKernelGGL(frame_preview_kernel, dim3((n + kFmThreads - 1) / kFmThreads), dim3(kFmThreads), 0, s, rgb, depth, depth_max,
                     depth_scale, n, rgb8, depth8);
  return hipGetLastError();
}

}  // namespace ufr
