// Undistortion of a custom scene's pictures: n 8-bit images that share one COLMAP camera are resampled to the pinhole camera
// k_out (include/ufr.h, ufr_image_undistort_u8, states the rule; this file follows its operation order).  The rule restates
// COLMAP's public camera models; neither COLMAP nor OpenCV was compared.  A plain streaming kernel: no LDS, no matrix cores.
//
//   image_undistort  one thread per output pixel, x fastest.  The thread maps its pixel centre through the inverse of the output
//          intrinsics, the model's distortion and the source intrinsics ONCE -- the n images share the camera -- and then loops
//          over the images: four taps per channel straight from global memory, the bilinear value in fp64, rint (half to
//          even), one byte per channel.  A pixel whose source position lies outside [0, Ws-1] x [0, Hs-1] (or is NaN) reads
//          nothing and writes 0 to every channel of every image and 0 to `valid`.
//          Traffic: the stores of a wave's 64 neighbouring pixels are 64 C contiguous bytes per image; its taps fall into the
//          few source rows the distorted image of that run of pixels crosses, so neighbouring lanes share cache lines.  The
//          arithmetic (some tens of fp64 operations for the map, nine per image and channel) stays far below what the memory
//          traffic costs at the fp64 vector rate.
//
// The eleven COLMAP models reach the kernel as three families (launch_image_undistort sorts them, with every coefficient a model
// does not have set to 0; adding a zero term changes no finite result, so this IS each model's own formula):
//   polynomial  SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV           k1 k2 p1 p2
//   rational    FULL_OPENCV                                                      k1 k2 p1 p2 k3 k4 k5 k6
//   fisheye     OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE            k1 k2 k3 k4
//
// Block shape: 256 threads, a 1-D grid over the H W output pixels; every byte offset is 64-bit.  fp contraction is off: each
// product, sum and quotient is rounded on its own, as numpy rounds them.
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kUdThreads = 256;
constexpr double kFisheyeEps = 1e-8;      // below this radius the fisheye scale theta_d / r is taken as 1

enum UndistortFamily { kUdPolynomial = 0, kUdRational = 1, kUdFisheye = 2 };

struct UndistortArgs {
  double fx, fy, cx, cy;          // the source camera
  double fxo, fyo, cxo, cyo;      // the output pinhole (k_out)
  double k[8];                    // the family's coefficients, in the order of the table above
  int family;
  int n, Hs, Ws, H, W;
};

__device__ inline void distort(const UndistortArgs& a, double x, double y, double* xd, double* yd) {
  const double xx = x * x, yy = y * y;
  const double r2 = xx + yy;
  if (a.family == kUdFisheye) {
    const double r = __dsqrt_rn(r2);
    double s = 1.0;
    if (r >= kFisheyeEps) {          // (a NaN radius keeps s = 1 and leaves x, y NaN: invalid)
      const double t = atan(r);
      const double t2 = t * t, t4 = t2 * t2;
      const double t6 = t4 * t2, t8 = t4 * t4;
      const double poly = (((1.0 + a.k[0] * t2) + a.k[1] * t4) + a.k[2] * t6) + a.k[3] * t8;
      s = (t * poly) / r;
    }
    *xd = x * s;
    *yd = y * s;
    return;
  }
  const double r4 = r2 * r2;
  const double xy = x * y;
  const double tx = (2.0 * a.k[2]) * xy + a.k[3] * (r2 + 2.0 * xx);
  const double ty = (2.0 * a.k[3]) * xy + a.k[2] * (r2 + 2.0 * yy);
  if (a.family == kUdRational) {
    const double r6 = r4 * r2;
    const double num = ((1.0 + a.k[0] * r2) + a.k[1] * r4) + a.k[4] * r6;
    const double den = ((1.0 + a.k[5] * r2) + a.k[6] * r4) + a.k[7] * r6;
    const double rad = num / den;
    *xd = x * rad + tx;
    *yd = y * rad + ty;
  } else {
    const double rad = a.k[0] * r2 + a.k[1] * r4;
    *xd = (x + x * rad) + tx;
    *yd = (y + y * rad) + ty;
  }
}

template <int C>
__global__ void __launch_bounds__(kUdThreads) image_undistort_kernel(const unsigned char* __restrict__ src, UndistortArgs a,
                                                                      unsigned char* __restrict__ dst, unsigned char* __restrict__ valid) {
  const long long i = (long long)blockIdx.x * kUdThreads + threadIdx.x;
  const long long HW = (long long)a.H * a.W;
  if (i >= HW) return;
  const int y = (int)(i / a.W), x = (int)(i - (long long)y * a.W);
  const double xn = (((double)x + 0.5) - a.cxo) / a.fxo;
  const double yn = (((double)y + 0.5) - a.cyo) / a.fyo;
  double xd, yd;
  distort(a, xn, yn, &xd, &yd);
  const double u = (a.fx * xd + a.cx) - 0.5;
  const double v = (a.fy * yd + a.cy) - 0.5;
  const bool ok = u >= 0.0 && u <= (double)(a.Ws - 1) && v >= 0.0 && v <= (double)(a.Hs - 1);      // a NaN fails every comparison
  if (valid) valid[i] = ok ? 255 : 0;
  unsigned char* out = dst + i * C;
  const long long out_step = HW * C;
  if (!ok) {
    for (int im = 0; im < a.n; ++im, out += out_step) {
#pragma unroll
      for (int c = 0; c < C; ++c) out[c] = 0;
    }
    return;
  }
  const double fu = floor(u), fv = floor(v);
  int x0 = (int)fu, y0 = (int)fv;                      // 0 .. Ws - 1 and 0 .. Hs - 1: `ok` bounds u and v
  x0 = x0 < a.Ws - 1 ? x0 : a.Ws - 1;
  y0 = y0 < a.Hs - 1 ? y0 : a.Hs - 1;
  const int x1 = x0 + 1 < a.Ws - 1 ? x0 + 1 : a.Ws - 1;
  const int y1 = y0 + 1 < a.Hs - 1 ? y0 + 1 : a.Hs - 1;
  const double wa = u - (double)x0, wb = v - (double)y0;
  const double na = 1.0 - wa, nb = 1.0 - wb;
  const long long o00 = ((long long)y0 * a.Ws + x0) * C, o01 = ((long long)y0 * a.Ws + x1) * C;
  const long long o10 = ((long long)y1 * a.Ws + x0) * C, o11 = ((long long)y1 * a.Ws + x1) * C;
  const long long src_step = (long long)a.Hs * a.Ws * C;
  const unsigned char* img = src;
  for (int im = 0; im < a.n; ++im, img += src_step, out += out_step) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double top = na * (double)img[o00 + c] + wa * (double)img[o01 + c];
      const double bot = na * (double)img[o10 + c] + wa * (double)img[o11 + c];
      const double val = nb * top + wb * bot;
      out[c] = (unsigned char)(int)rint(val);          // 0 .. 255: a mean of bytes with weights that add up to 1
    }
  }
}

}  // namespace

// model: COLMAP's camera model id, one of the nine above (the entry point has checked it, and that every parameter is finite)
hipError_t launch_image_undistort(const unsigned char* src, int n, int Hs, int Ws, int C, int model, const double* params,
                                  const double* k_out, int H, int W, unsigned char* dst, unsigned char* valid, hipStream_t s) {
  UndistortArgs a = {};
  const bool single = model == 0 || model == 2 || model == 3 || model == 8 || model == 9;      // f, cx, cy come first
  a.fx = params[0];
  a.fy = single ? params[0] : params[1];
  a.cx = single ? params[1] : params[2];
  a.cy = single ? params[2] : params[3];
  const double* d = params + (single ? 3 : 4);           // the distortion coefficients
  switch (model) {
    case 0: case 1: a.family = kUdPolynomial; break;                                              // SIMPLE_PINHOLE, PINHOLE
    case 2: a.family = kUdPolynomial; a.k[0] = d[0]; break;                                       // SIMPLE_RADIAL
    case 3: a.family = kUdPolynomial; a.k[0] = d[0]; a.k[1] = d[1]; break;                        // RADIAL
    case 4: a.family = kUdPolynomial; for (int j = 0; j < 4; ++j) a.k[j] = d[j]; break;           // OPENCV
    case 6: a.family = kUdRational; for (int j = 0; j < 8; ++j) a.k[j] = d[j]; break;             // FULL_OPENCV
    case 5: a.family = kUdFisheye; for (int j = 0; j < 4; ++j) a.k[j] = d[j]; break;              // OPENCV_FISHEYE
    case 8: a.family = kUdFisheye; a.k[0] = d[0]; break;                                          // SIMPLE_RADIAL_FISHEYE
    case 9: a.family = kUdFisheye; a.k[0] = d[0]; a.k[1] = d[1]; break;                           // RADIAL_FISHEYE
    default: return hipErrorInvalidValue;
  }
  a.fxo = k_out[0], a.fyo = k_out[1], a.cxo = k_out[2], a.cyo = k_out[3];
  a.n = n, a.Hs = Hs, a.Ws = Ws, a.H = H, a.W = W;
  const dim3 grid((unsigned)(((long long)H * W + kUdThreads - 1) / kUdThreads)), block(kUdThreads);
  switch (C) {
    case 1: hipLaunchKernelGGL(image_undistort_kernel<1>, grid, block, 0, s, src, a, dst, valid); break;
    case 2: hipLaunchKernelGGL(image_undistort_kernel<2>, grid, block, 0, s, src, a, dst, valid); break;
    case 3: hipLaunchKernelGGL(image_undistort_kernel<3>, grid, block, 0, s, src, a, dst, valid); break;
    case 4: hipLaunchKernelGGL(image_undistort_kernel<4>, grid, block, 0, s, src, a, dst, valid); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace ufr
