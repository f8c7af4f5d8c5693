// What a DTU scan loader computes per pixel (the reference's code1/dataset/dtu_test_sparse.py: load_scene's cv.resize(...) /
// 255., __getitem__'s ray tables), with the arithmetic that uforecon_amd/dtu_scan.py restates on the host (include/ufr.h,
// ufr_image_resize_u8 / ufr_pixel_rays).  Plain streaming kernels: no LDS, no matrix cores.
//
//   image_resize  one thread per output pixel of one image, all three channels.  8-bit bilinear resize as OpenCV's resize()
//          does it for CV_8U with INTER_LINEAR, restated from memory of resize.cpp (no OpenCV was at hand: the rule here is
//          the rule), then the crop, / 255 in double and the cast to float:
//            source coordinate   f = (float)((d + 0.5) * scale - 0.5), scale = (double)src_size / dst_size; s = floor(f), f -= s
//            horizontally        s < 0: s = 0, f = 0;  s >= Ws - 1: s = Ws - 1, f = 0 (the second tap then has weight 0 and is
//                                not read);  weights a0 = rint((1.f - f) * 2048.f), a1 = rint(f * 2048.f) (round half to even)
//            vertically          the weights b0, b1 keep f; the two rows s, s + 1 are clamped to 0 .. Hs - 1
//            row value           r = S[s] * a0 + S[s + 1] * a1                                          (int32)
//            pixel               (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
//          When Ws == 2 W and Hs == 2 H exactly, OpenCV takes its area path instead: (s00 + s01 + s10 + s11 + 2) >> 2.
//          Reads of a pixel's three bytes are as scattered as the source image makes them (stride 3 * scale bytes along a
//          row); the three plane writes are coalesced along W.
//   image_resize_mask  the same kernel with a second source, a single-channel 8-bit mask of the source size (the reference's
//          GeneralFit.load_scene, code1/dataset/general_fit.py:174-180): the mask goes through the same resize rule, and the
//          output is (float)(((double)v / 255.0) * ((double)m / 254.0)) -- 254 is the reference's divisor.
//   pixel_rays    one thread per pixel, in double: p = (x * 2 / (W - 1) - 1, y * 2 / (H - 1) - 1, 1, 1), v = (M p)[:3] - origin
//          with M the float32 matrix widened to double and the four products of a row summed left to right, then v / |v|,
//          |v| = sqrt((v0^2 + v1^2) + v2^2), stored as float.  numpy's matmul and torch.norm may sum in another order: the host
//          side differs by a few double ulps before the cast (tests/test_gpu_dtu_scan.py bounds what is left of that).
//
//   depth_gt      one thread per output pixel: the ground-truth depth of a training view as the reference's MVSDataset makes it
//          (code1/dataset/dtu_train.py:249-254, :429, :485) from the rows of a grey PFM file as stored: the row flip of read_pfm
//          (bottom_up), OpenCV's INTER_NEAREST at fx = fy = 0.5, restated (source pixel (2y, 2x); no OpenCV was compared), the
//          crop, x scale_factor in float32, then / cam_ray_d.z in DOUBLE (the reference divides by its float64 ray table)
//          and the cast to float.  A hole (0) stays 0.  The scale the PFM header carries is not applied (the reference drops it).
//
// Block shape: 256 threads, a 1-D grid over the pixels of all images; every index is 64-bit.
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kFiThreads = 256;

struct Tap {
  int s0, s1;   // source indices, in range
  int w0, w1;   // 11-bit weights
};

// the horizontal rule: the clamped side gets weight 0
__device__ inline Tap tap_x(int d, double scale, int n) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f = f - (float)s;
  if (s < 0) s = 0, f = 0.f;
  if (s >= n - 1) s = n - 1, f = 0.f;
  Tap t;
  t.s0 = s;
  t.s1 = s + 1 < n ? s + 1 : n - 1;
  t.w0 = (int)rintf((1.f - f) * 2048.f);
  t.w1 = (int)rintf(f * 2048.f);
  return t;
}

// the vertical rule: the weights stay, the rows are clamped
__device__ inline Tap tap_y(int d, double scale, int n) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f = f - (float)s;
  Tap t;
  t.s0 = s < 0 ? 0 : (s > n - 1 ? n - 1 : s);
  t.s1 = s + 1 < 0 ? 0 : (s + 1 > n - 1 ? n - 1 : s + 1);
  t.w0 = (int)rintf((1.f - f) * 2048.f);
  t.w1 = (int)rintf(f * 2048.f);
  return t;
}

struct ResizeArgs {
  int Hs, Ws, H, W;       // source size, resized size
  int x0, y0, Ho, Wo;     // crop: first column / row of the resized image that is kept, and the kept size
};

// kMask: a second, single-channel source (n,Hs,Ws) goes through the same resize, and the output is colour x mask (image_resize_mask)
template <bool kMask>
__global__ void __launch_bounds__(kFiThreads) image_resize_kernel(const unsigned char* __restrict__ src,
                                                                   const unsigned char* __restrict__ mask, long long total, ResizeArgs a,
                                                                   float* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x;
  if (i >= total) return;
  const long long plane = (long long)a.Ho * a.Wo;
  const long long n = i / plane;
  const long long p = i - n * plane;
  const int yo = (int)(p / a.Wo), xo = (int)(p - (long long)yo * a.Wo);
  const int dx = xo + a.x0, dy = yo + a.y0;
  const unsigned char* img = src + n * ((long long)a.Hs * a.Ws * 3);
  const unsigned char* msk = kMask ? mask + n * ((long long)a.Hs * a.Ws) : nullptr;
  int out[3], m = 0;
  if (a.Ws == 2 * a.W && a.Hs == 2 * a.H) {
    const unsigned char* r0 = img + ((long long)(2 * dy) * a.Ws + 2 * dx) * 3;
    const unsigned char* r1 = r0 + (long long)a.Ws * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = ((int)r0[c] + (int)r0[3 + c] + (int)r1[c] + (int)r1[3 + c] + 2) >> 2;
    if (kMask) {
      const unsigned char* m0 = msk + (long long)(2 * dy) * a.Ws + 2 * dx;
      const unsigned char* m1 = m0 + a.Ws;
      m = ((int)m0[0] + (int)m0[1] + (int)m1[0] + (int)m1[1] + 2) >> 2;
    }
  } else {
    const Tap tx = tap_x(dx, (double)a.Ws / (double)a.W, a.Ws);
    const Tap ty = tap_y(dy, (double)a.Hs / (double)a.H, a.Hs);
    const unsigned char* r0 = img + (long long)ty.s0 * a.Ws * 3;
    const unsigned char* r1 = img + (long long)ty.s1 * a.Ws * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int h0 = (int)r0[3 * (long long)tx.s0 + c] * tx.w0 + (int)r0[3 * (long long)tx.s1 + c] * tx.w1;
      const int h1 = (int)r1[3 * (long long)tx.s0 + c] * tx.w0 + (int)r1[3 * (long long)tx.s1 + c] * tx.w1;
      out[c] = (((ty.w0 * (h0 >> 4)) >> 16) + ((ty.w1 * (h1 >> 4)) >> 16) + 2) >> 2;
    }
    if (kMask) {
      const unsigned char* m0 = msk + (long long)ty.s0 * a.Ws;
      const unsigned char* m1 = msk + (long long)ty.s1 * a.Ws;
      const int h0 = (int)m0[tx.s0] * tx.w0 + (int)m0[tx.s1] * tx.w1;
      const int h1 = (int)m1[tx.s0] * tx.w0 + (int)m1[tx.s1] * tx.w1;
      m = (((ty.w0 * (h0 >> 4)) >> 16) + ((ty.w1 * (h1 >> 4)) >> 16) + 2) >> 2;
    }
  }
  if (kMask) {
    const double w = (double)m / 254.0;     // the reference's own divisor (general_fit.py:178), kept
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(n * 3 + c) * plane + p] = (float)(((double)out[c] / 255.0) * w);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(n * 3 + c) * plane + p] = (float)((double)out[c] / 255.0);
  }
}

struct RayArgs {
  double m[12];     // rows 0..2 of the matrix
  double o[3];
};

__global__ void __launch_bounds__(kFiThreads) pixel_rays_kernel(RayArgs a, int H, int W, float* __restrict__ dir) {
  const long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x;
  const long long HW = (long long)H * W;
  if (i >= HW) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const double px = ((double)x * 2.0) / (double)(W - 1) - 1.0;
  const double py = ((double)y * 2.0) / (double)(H - 1) - 1.0;
  double v[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) v[r] = (((a.m[4 * r] * px + a.m[4 * r + 1] * py) + a.m[4 * r + 2]) + a.m[4 * r + 3]) - a.o[r];
  const double len = __dsqrt_rn((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) dir[r * HW + i] = (float)(v[r] / len);
}

__global__ void __launch_bounds__(kFiThreads) depth_gt_kernel(const float* __restrict__ pfm, int Hs, int Ws, int bottom_up, int y0, int x0,
                                                               int H, int W, float scale_factor, const double* __restrict__ cam_ray_z,
                                                               float* __restrict__ depth) {
  const long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x;
  if (i >= (long long)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const int ys = 2 * (y + y0), xs = 2 * (x + x0);                 // inside the file: the entry point checked the crop
  const int row = bottom_up ? Hs - 1 - ys : ys;
  const float scaled = pfm[(long long)row * Ws + xs] * scale_factor;
  depth[i] = (float)((double)scaled / cam_ray_z[i]);
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kFiThreads - 1) / kFiThreads); }

}  // namespace

hipError_t launch_image_resize_u8(const unsigned char* src, const unsigned char* mask, long long n, int Hs, int Ws, int H, int W, int x0,
                                  int y0, int Ho, int Wo, float* dst, hipStream_t s) {
  const ResizeArgs a{Hs, Ws, H, W, x0, y0, Ho, Wo};
  const long long total = n * Ho * Wo;
  if (mask)
    hipLaunchKernelGGL(image_resize_kernel<true>, dim3(blocks_of(total)), dim3(kFiThreads), 0, s, src, mask, total, a, dst);
  else
    hipLaunchKernelGGL(image_resize_kernel<false>, dim3(blocks_of(total)), dim3(kFiThreads), 0, s, src, mask, total, a, dst);
  return hipGetLastError();
}

hipError_t launch_pixel_rays(const float* m_inv, const float* origin, int H, int W, float* dir, hipStream_t s) {
  RayArgs a;
  for (int k = 0; k < 12; ++k) a.m[k] = (double)m_inv[k];
  for (int k = 0; k < 3; ++k) a.o[k] = origin ? (double)origin[k] : 0.0;
  hipLaunchKernelGGL(pixel_rays_kernel, dim3(blocks_of((long long)H * W)), dim3(kFiThreads), 0, s, a, H, W, dir);
  return hipGetLastError();
}

hipError_t launch_depth_gt(const float* pfm, int Hs, int Ws, int bottom_up, int y0, int x0, int H, int W, float scale_factor,
                           const double* cam_ray_z, float* depth, hipStream_t s) {
  hipLaunchKernelGGL(depth_gt_kernel, dim3(blocks_of((long long)H * W)), dim3(kFiThreads), 0, s, pfm, Hs, Ws, bottom_up, y0, x0, H, W,
                     scale_factor, cam_ray_z, depth);
  return hipGetLastError();
}

}  // namespace ufr
