// Point-cloud rendering on the device: a z-buffered splat of (N,3) fp64 points and a per-pixel resolve with eye-dome
// lighting, with the arithmetic that tests/points_ref.py restates (include/ufr.h, ufr_splat_frames).  The depth test is the
// first-hit design of mesh_clean.hip: a 64-bit key image, preset to all ones by the caller, merged with an atomic minimum.
//
//   splat    one thread per point.  In fp64, products summed left to right, no contraction:
//              c  = w2c[:3,:3] p + w2c[:3,3] (the three products, then the translation), q = k c
//              px = rint(q.x / q.z), py = rint(q.y / q.z) (round half to even; pixel centres are the integers)
//            Dropped: a point with a coordinate that is not finite, not c.z > z_min, px or py not finite, a footprint wholly
//            outside the image.  Footprint: the pixels (px + dx, py + dy) with dx^2 + dy^2 <= r^2 + r, clipped to the image.
//            Each gets key = (bits of (float)c.z) << 32 | point index: the nearest (float) depth wins, ties go to the lowest
//            index, whatever the order of arrival.  The pixel's key is read with a plain load first and the atomic is skipped
//            when the point cannot win: keys only ever fall, so a stale read is never smaller than the truth and never skips a winner.
//   resolve  one thread per pixel.  Key all ones (or an index >= N): background, depth 0, id -1.  Otherwise z = the stored
//            float, and in fp64 with z widened
//              o_k = max(0, log2(z) - log2(z_k)) over the neighbours (x - d, y), (x + d, y), (x, y - d), (x, y + d); an empty
//                    neighbour and one outside the image give 0
//              s   = ((o_1 + o_2) + o_3) + o_4,  I = exp(-(edl_strength * s) / 4); I = 1 with no exp when edl_strength or s is 0
//              pixel = rint(colour * I) clamped to 0..255, colour = colors[idx] or 255 * base_color
//
// Block shape: 256 threads, no LDS.  Every index read from the key image is range-checked before it is used.
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kSpThreads = 256;
constexpr unsigned long long kEmptyKey = ~0ull;

struct SplatCam {
  double k[9], r[9], t[3];
};

__global__ void __launch_bounds__(kSpThreads) splat_kernel(const double* __restrict__ points, long long N, SplatCam cam, int H, int W,
                                                            int radius, double z_min, unsigned long long* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * kSpThreads + threadIdx.x;
  if (i >= N) return;
  const double x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
  if (!(fabs(x) <= 1.7976931348623157e308 && fabs(y) <= 1.7976931348623157e308 && fabs(z) <= 1.7976931348623157e308)) return;
  const double c0 = ((cam.r[0] * x + cam.r[1] * y) + cam.r[2] * z) + cam.t[0];
  const double c1 = ((cam.r[3] * x + cam.r[4] * y) + cam.r[5] * z) + cam.t[1];
  const double c2 = ((cam.r[6] * x + cam.r[7] * y) + cam.r[8] * z) + cam.t[2];
  if (!(c2 > z_min)) return;                               // NaN too
  const double q0 = (cam.k[0] * c0 + cam.k[1] * c1) + cam.k[2] * c2;
  const double q1 = (cam.k[3] * c0 + cam.k[4] * c1) + cam.k[5] * c2;
  const double q2 = (cam.k[6] * c0 + cam.k[7] * c1) + cam.k[8] * c2;
  const double rx = rint(q0 / q2), ry = rint(q1 / q2);     // round half to even
  const double r = (double)radius;
  // the whole footprint outside, NaN and the infinities all fail here; what passes fits an int
  if (!(rx >= -r && rx <= (double)(W - 1) + r && ry >= -r && ry <= (double)(H - 1) + r)) return;
  const int px = (int)rx, py = (int)ry;
  const unsigned long long key = ((unsigned long long)__float_as_uint((float)c2) << 32) | (unsigned long long)i;
  const int lim = radius * radius + radius;
  for (int dy = -radius; dy <= radius; ++dy) {
    const int yy = py + dy;
    if (yy < 0 || yy >= H) continue;
    for (int dx = -radius; dx <= radius; ++dx) {
      const int xx = px + dx;
      if (xx < 0 || xx >= W || dx * dx + dy * dy > lim) continue;
      unsigned long long* slot = keys + ((long long)yy * W + xx);
      if (key < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, key);
    }
  }
}

struct ResolveArgs {
  double color[3], strength;   // 255 * base colour
  unsigned char bg[3];
  int d;
};

// log2 of the depth stored at pixel (x, y); false: empty or outside
__device__ inline bool neighbour_log2(const unsigned long long* __restrict__ keys, long long N, int H, int W, long long x, long long y, double* l) {
  if (x < 0 || x >= W || y < 0 || y >= H) return false;
  const unsigned long long k = keys[y * W + x];
  if (k == kEmptyKey || (long long)(k & 0xffffffffull) >= N) return false;
  *l = log2((double)__uint_as_float((unsigned)(k >> 32)));
  return true;
}

__global__ void __launch_bounds__(kSpThreads) resolve_kernel(const unsigned long long* __restrict__ keys, long long N,
                                                                    const unsigned char* __restrict__ colors, ResolveArgs a, int H, int W,
                                                                    unsigned char* __restrict__ image, float* __restrict__ depth,
                                                                    int* __restrict__ point_id) {
  const long long i = (long long)blockIdx.x * kSpThreads + threadIdx.x;
  if (i >= (long long)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const unsigned long long k = keys[i];
  const long long idx = (long long)(k & 0xffffffffull);
  unsigned char px[3] = {a.bg[0], a.bg[1], a.bg[2]};
  float dep = 0.f;
  int id = -1;
  if (k != kEmptyKey && idx < N) {
    dep = __uint_as_float((unsigned)(k >> 32));
    id = (int)idx;
    double I = 1.0;
    if (a.strength > 0.0) {
      const double lz = log2((double)dep);
      const long long d = a.d, nx[4] = {x - d, x + d, x, x}, ny[4] = {y, y, y - d, y + d};
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double l, o = 0.0;
        if (neighbour_log2(keys, N, H, W, nx[j], ny[j], &l)) o = fmax(0.0, lz - l);
        s = s + o;
      }
      if (s > 0.0) I = exp(-(a.strength * s) / 4.0);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double col = colors ? (double)colors[3 * idx + c] : a.color[c];
      double p = rint(col * I);   // round half to even
      if (!(p >= 0.0)) p = 0.0;   // NaN too
      if (p > 255.0) p = 255.0;
      px[c] = (unsigned char)(int)p;
    }
  }
  image[3 * i] = px[0];
  image[3 * i + 1] = px[1];
  image[3 * i + 2] = px[2];
  if (depth) depth[i] = dep;
  if (point_id) point_id[i] = id;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kSpThreads - 1) / kSpThreads); }

}  // namespace

hipError_t launch_splat(const double* points, long long N, const double* k, const double* w2c, int H, int W, int radius, double z_min,
                        unsigned long long* keys, hipStream_t s) {
  SplatCam cam;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) cam.k[3 * i + j] = k[3 * i + j], cam.r[3 * i + j] = w2c[4 * i + j];
    cam.t[i] = w2c[4 * i + 3];
  }
  hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)H * W * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(splat_kernel, dim3(blocks_of(N)), dim3(kSpThreads), 0, s, points, N, cam, H, W, radius, z_min, keys);
  return hipGetLastError();
}

hipError_t launch_splat_resolve(const unsigned long long* keys, long long N, const unsigned char* colors, const double* base,
                                const unsigned char* bg, double edl_strength, int edl_radius, int H, int W, unsigned char* image,
                                float* depth, int* point_id, hipStream_t s) {
  ResolveArgs a;
  for (int c = 0; c < 3; ++c) a.color[c] = 255.0 * base[c], a.bg[c] = bg[c];
  a.strength = edl_strength;
  a.d = edl_radius;
  hipLaunchKernelGGL(resolve_kernel, dim3(blocks_of((long long)H * W)), dim3(kSpThreads), 0, s, keys, N, colors, a, H, W, image,
                     depth, point_id);
  return hipGetLastError();
}

}  // namespace ufr
