// Mesh rendering on the device (the reference's render_trajectory_dtu.py / render_trajectory_open3d.py without Open3D, OpenGL or
// a display), with the arithmetic that tests/raster_ref.py restates (include/ufr.h, ufr_raster_*).  The first hit itself is
// mesh_clean.hip's, reached through launch_first_hit with a null mask; this file turns its face ids into pixels.
//
//   vertex_normals  one thread per vertex.  The caller passes the 3F corner slots 3f + e stably sorted by vertex and the V + 1
//          run starts; a vertex's run is walked in ascending slot order and the unnormalised face normals (b - a) x (c - a)
//          of its faces (formed from the face's own a, b, c, whichever corner the vertex is) are summed in fp64, each component
//          on its own, then divided by the length of the sum.  No atomics: the sum does not depend on scheduling.  An unused
//          vertex, a sum of length 0 (or not finite) give (0, 0, 0); a zero-area face adds zero; a face with an index outside
//          0..V-1, a slot outside 0..3F-1 and a slot that does not name the vertex contribute nothing.  This is the area
//          weighting of Open3D's compute_vertex_normals as remembered; no Open3D was at hand: the rule here is the rule.
//   shade           one thread per pixel of one frame.  Face -1 (or out of range): background, depth 0, normal 0.  Otherwise the
//          ray (pixel_ray) and a, b, c, e_bc, e_ca, e_ab, n, n . a (load_tri) are formed again by the first hit's own code
//          (mesh_ray.h), then in fp64:
//            w       = (e_bc, e_ca, e_ab) / ((e_bc + e_ca) + e_ab); t = (n . a) / (n . d); depth = (float)(t * v.z), v the
//                      camera-space unit ray: z-depth
//            N       smooth: (w_a N_a + w_b N_b) + w_c N_c per component, divided by its length; flat (no vertex normals, or
//                      that length is not > 0): n / |n|
//            I       = ambient + (1 - ambient) * |N . d|: a headlight, two-sided, so winding does not matter
//            colour  the base colour, or ((w_a C_a + w_b C_b) + w_c C_c) / 255 of the uint8 vertex colours, or (ufr_texture_frames,
//                      the kernel's textured instance) s / 255 of a texture: tx = (w_a xa + w_b xb) + w_c xc and ty likewise from
//                      the face's corner texels, x0 = floor(tx), fx = tx - x0, the indices x0 and x0 + 1 clamped to the texture
//                      after fx is formed, s the bilinear expression of mesh colouring; tx or ty not finite: white.  No mipmaps
//            pixel   = rint((255 * colour) * I) (round half to even) clamped to 0..255
//            normal  = R^T N (camera coordinates; products summed in row order), negated when N . d > 0: it faces the camera
//   downsample      one thread per output byte: the mean of an s x s block in integers, q = sum / s^2, r = sum % s^2, rounded up
//          iff 2r > s^2, or 2r == s^2 and q is odd (round half to even).
//
// Block shape: 256 threads throughout, no LDS.  Every index read from a caller's array is range-checked before it is used.
#include "mesh_ray.h"
#include "mesh_rows.h"

namespace ufr {
namespace {

constexpr int kRsThreads = 256;

__global__ void __launch_bounds__(kRsThreads) vertex_normals_kernel(const double* __restrict__ verts, const int* __restrict__ faces,
                                                                     long long V, long long F,
                                                                     const long long* __restrict__ slots,
                                                                     const long long* __restrict__ runs,
                                                                     double* __restrict__ normals) {
  const long long v = (long long)blockIdx.x * kRsThreads + threadIdx.x;
  if (v >= V) return;
  long long i0, i1;
  run_of(runs, v, 3 * F, &i0, &i1);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (long long i = i0; i < i1; ++i) {
    const long long slot = slots[i];
    if (!slot_names(slot, faces, F, v)) continue;
    const long long f = slot / 3;
    const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) continue;
    double p[3], q[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double a = verts[3 * (long long)ia + k];
      p[k] = verts[3 * (long long)ib + k] - a;
      q[k] = verts[3 * (long long)ic + k] - a;
    }
    cross3(p, q, n);
    sx = sx + n[0];
    sy = sy + n[1];
    sz = sz + n[2];
  }
  const double len = __dsqrt_rn((sx * sx + sy * sy) + sz * sz);
  const bool ok = len > 0.0 && len < 1.7976931348623157e308;   // zero, NaN and an overflowed sum give the zero normal
  normals[3 * v] = ok ? sx / len : 0.0;
  normals[3 * v + 1] = ok ? sy / len : 0.0;
  normals[3 * v + 2] = ok ? sz / len : 0.0;
}

struct ShadeArgs {
  double base[3], ambient;
  unsigned char bg[3];
};

// the two texel indices of one axis of a bilinear footprint at t0 = floor(t): t0 and t0 + 1, each clamped to 0..n-1 in double
// before the conversion (t is finite here, so both fit an int afterwards)
__device__ inline void clamped_pair(double t0, int n, int* i0, int* i1) {
  const double hi = (double)(n - 1), t1 = t0 + 1.0;
  *i0 = (int)(t0 < 0.0 ? 0.0 : (t0 > hi ? hi : t0));
  *i1 = (int)(t1 < 0.0 ? 0.0 : (t1 > hi ? hi : t1));
}

// kTextured false: ufr_raster_frames (tex is not looked at); true: ufr_texture_frames, the colour comes from tex
template <bool kTextured>
__global__ void __launch_bounds__(kRsThreads) shade_kernel(const double* __restrict__ verts, const int* __restrict__ faces, long long V,
                                                            long long F, const double* __restrict__ normals,
                                                            const unsigned char* __restrict__ colors, HitCam cam, ShadeArgs sh,
                                                            RasterTexture tex, const int* __restrict__ face_img, int H, int W,
                                                            unsigned char* __restrict__ image, float* __restrict__ depth,
                                                            int* __restrict__ face_out, float* __restrict__ normal_out) {
  const long long i = (long long)blockIdx.x * kRsThreads + threadIdx.x;
  if (i >= (long long)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const long long f = face_img[i];
  Tri t;
  double world[9];
  int idx[3];
  unsigned char px[3] = {sh.bg[0], sh.bg[1], sh.bg[2]};
  float dep = 0.f, nout[3] = {0.f, 0.f, 0.f};
  int fo = -1;
  if (f >= 0 && f < F && load_tri(verts, faces, V, f, cam, &t, world, idx)) {
    fo = (int)f;
    float v[3];
    double d[3];
    pixel_ray(cam, x, y, v, d);
    const double e0 = dot3(d, t.cbc), e1 = dot3(d, t.cca), e2 = dot3(d, t.cab);
    const double s = (e0 + e1) + e2;
    const double w0 = e0 / s, w1 = e1 / s, w2 = e2 / s;
    const double den = dot3(t.n, d);
    const double tt = t.na / den;
    dep = (float)(tt * (double)v[2]);
    double N[3];
    bool smooth = false;
    if (normals) {
      const double* Na = normals + 3 * (long long)idx[0];
      const double* Nb = normals + 3 * (long long)idx[1];
      const double* Nc = normals + 3 * (long long)idx[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) N[k] = (w0 * Na[k] + w1 * Nb[k]) + w2 * Nc[k];
      const double len = __dsqrt_rn(dot3(N, N));
      if (len > 0.0) {
        smooth = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) N[k] = N[k] / len;
      }
    }
    if (!smooth) {
      const double len = __dsqrt_rn(dot3(t.n, t.n));
#pragma unroll
      for (int k = 0; k < 3; ++k) N[k] = t.n[k] / len;
    }
    const double c = dot3(N, d);
    const double I = sh.ambient + (1.0 - sh.ambient) * fabs(c);
    double tcol[3] = {1.0, 1.0, 1.0};   // textured: white unless the texture coordinate is finite
    if (kTextured) {
      const double* xy = tex.corner_xy + 6 * f;   // (xa, ya, xb, yb, xc, yc) of face f
      const double tx = (w0 * xy[0] + w1 * xy[2]) + w2 * xy[4];
      const double ty = (w0 * xy[1] + w1 * xy[3]) + w2 * xy[5];
      if (fabs(tx) <= 1.7976931348623157e308 && fabs(ty) <= 1.7976931348623157e308) {   // NaN fails too
        const double xf = floor(tx), yf = floor(ty);
        const double fx = tx - xf, fy = ty - yf;
        int x0, x1, y0, y1;
        clamped_pair(xf, tex.Wt, &x0, &x1);
        clamped_pair(yf, tex.Ht, &y0, &y1);
        const unsigned char* r0 = tex.texture + 3 * (long long)y0 * tex.Wt;
        const unsigned char* r1 = tex.texture + 3 * (long long)y1 * tex.Wt;
        const double gx = 1.0 - fx, gy = 1.0 - fy;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double s = gy * (gx * (double)r0[3 * x0 + k] + fx * (double)r0[3 * x1 + k]) +
                           fy * (gx * (double)r1[3 * x0 + k] + fx * (double)r1[3 * x1 + k]);
          tcol[k] = s / 255.0;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double col = kTextured ? tcol[k] : sh.base[k];
      if (!kTextured && colors) {
        const double ca = (double)colors[3 * (long long)idx[0] + k], cb = (double)colors[3 * (long long)idx[1] + k],
                     cc = (double)colors[3 * (long long)idx[2] + k];
        col = ((w0 * ca + w1 * cb) + w2 * cc) / 255.0;
      }
      double p = rint((255.0 * col) * I);   // round half to even
      if (!(p >= 0.0)) p = 0.0;             // NaN too
      if (p > 255.0) p = 255.0;
      px[k] = (unsigned char)(int)p;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double nc = ((double)cam.rot[j] * N[0] + (double)cam.rot[3 + j] * N[1]) + (double)cam.rot[6 + j] * N[2];
      nout[j] = (float)(c > 0.0 ? -nc : nc);
    }
  }
  image[3 * i] = px[0];
  image[3 * i + 1] = px[1];
  image[3 * i + 2] = px[2];
  if (depth) depth[i] = dep;
  if (face_out) face_out[i] = fo;
  if (normal_out) {
    normal_out[3 * i] = nout[0];
    normal_out[3 * i + 1] = nout[1];
    normal_out[3 * i + 2] = nout[2];
  }
}

__global__ void __launch_bounds__(kRsThreads) downsample_kernel(const unsigned char* __restrict__ src, long long total, int H, int W,
                                                                 int s, unsigned char* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * kRsThreads + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % 3);
  const long long p = i / 3;
  const int x = (int)(p % W);
  const long long q = p / W;
  const int y = (int)(q % H);
  const long long n = q / H;
  const long long sW = (long long)s * W, sH = (long long)s * H;
  int sum = 0;
  for (int dy = 0; dy < s; ++dy)
    for (int dx = 0; dx < s; ++dx) sum += (int)src[((n * sH + ((long long)y * s + dy)) * sW + ((long long)x * s + dx)) * 3 + ch];
  const int n2 = s * s, quo = sum / n2, rem = sum % n2;
  const bool up = 2 * rem > n2 || (2 * rem == n2 && (quo & 1));
  dst[i] = (unsigned char)(quo + (up ? 1 : 0));
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kRsThreads - 1) / kRsThreads); }

}  // namespace

hipError_t launch_raster_vertex_normals(const double* verts, const int* faces, long long V, long long F, const long long* slots,
                                        const long long* runs, double* normals, hipStream_t s) {
  hipLaunchKernelGGL(vertex_normals_kernel, dim3(blocks_of(V)), dim3(kRsThreads), 0, s, verts, faces, V, F, slots, runs, normals);
  return hipGetLastError();
}

hipError_t launch_raster_shade(const double* verts, const int* faces, long long V, long long F, const double* normals,
                               const unsigned char* colors, const float* kinv, const float* rot, const float* org,
                               const double* proj, const double* base, double ambient, const unsigned char* bg, const int* face_img,
                               int H, int W, unsigned char* image, float* depth, int* face_out, float* normal_out, hipStream_t s,
                               const RasterTexture* tex) {
  const HitCam cam = make_hit_cam(kinv, rot, org, proj);
  ShadeArgs sh;
  for (int k = 0; k < 3; ++k) sh.base[k] = base[k], sh.bg[k] = bg[k];
  sh.ambient = ambient;
  const dim3 grid(blocks_of((long long)H * W)), block(kRsThreads);
  if (tex)
    hipLaunchKernelGGL(shade_kernel<true>, grid, block, 0, s, verts, faces, V, F, normals, colors, cam, sh, *tex, face_img, H, W, image,
                       depth, face_out, normal_out);
  else
    hipLaunchKernelGGL(shade_kernel<false>, grid, block, 0, s, verts, faces, V, F, normals, colors, cam, sh, RasterTexture{}, face_img,
                       H, W, image, depth, face_out, normal_out);
  return hipGetLastError();
}

hipError_t launch_raster_downsample(const unsigned char* src, long long n, int H, int W, int sf, unsigned char* dst, hipStream_t s) {
  const long long total = n * H * W * 3;
  hipLaunchKernelGGL(downsample_kernel, dim3(blocks_of(total)), dim3(kRsThreads), 0, s, src, total, H, W, sf, dst);
  return hipGetLastError();
}

}  // namespace ufr
