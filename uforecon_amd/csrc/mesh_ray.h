// The pixel ray and the triangle set-up of the first hit (mesh_clean.hip), shared with the shading kernel (raster.hip): one
// statement of the fp32 ray generator and of the fp64 edge products, so that a shaded pixel sees the numbers its first hit saw.
// Device only; every expression is evaluated as written (no contraction).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace ufr {

struct HitCam {
  float kinv[9], rot[9], org[3];
  double proj[12];   // pixel = proj (X, 1) / its third row: the fp64 inverse of the ray generator
};

struct Tri {
  double a[3], b[3], c[3];          // vertices - origin
  double cbc[3], cca[3], cab[3];    // b x c, c x a, a x b (each formed in ascending index order)
  double n[3], na;                  // (b - a) x (c - a), n . a
};

inline HitCam make_hit_cam(const float* kinv, const float* rot, const float* org, const double* proj) {
  HitCam cam;
  for (int i = 0; i < 9; ++i) cam.kinv[i] = kinv[i], cam.rot[i] = rot[i];
  for (int i = 0; i < 3; ++i) cam.org[i] = org[i];
  for (int i = 0; i < 12; ++i) cam.proj[i] = proj[i];
  return cam;
}

__device__ inline void cross3(const double* u, const double* v, double* o) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}
__device__ inline double dot3(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// u x v with u the vertex `iu`, v the vertex `iv`: computed for the lower index first, negated when iu > iv
__device__ inline void cross_ordered(const double* u, int iu, const double* v, int iv, double* o) {
  if (iu <= iv) {
    cross3(u, v, o);
  } else {
    cross3(v, u, o);
    o[0] = -o[0];
    o[1] = -o[1];
    o[2] = -o[2];
  }
}

// loads face f; false when an index is outside 0..V-1.  idx (nullable): the three vertex indices
__device__ inline bool load_tri(const double* __restrict__ verts, const int* __restrict__ faces, long long V, long long f,
                                const HitCam& cam, Tri* t, double world[9], int* idx = nullptr) {
  const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) return false;
  if (idx) idx[0] = ia, idx[1] = ib, idx[2] = ic;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double o = (double)cam.org[k];
    world[k] = verts[3 * (long long)ia + k];
    world[3 + k] = verts[3 * (long long)ib + k];
    world[6 + k] = verts[3 * (long long)ic + k];
    t->a[k] = world[k] - o;
    t->b[k] = world[3 + k] - o;
    t->c[k] = world[6 + k] - o;
  }
  cross_ordered(t->b, ib, t->c, ic, t->cbc);
  cross_ordered(t->c, ic, t->a, ia, t->cca);
  cross_ordered(t->a, ia, t->b, ib, t->cab);
  double u[3], v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    u[k] = t->b[k] - t->a[k];
    v[k] = t->c[k] - t->a[k];
  }
  cross3(u, v, t->n);
  t->na = dot3(t->n, t->a);
  return true;
}

// the ray of pixel (x, y) in fp32, as gen_rays_from_single_image: v the camera-space unit ray, d = R v widened to fp64
__device__ inline void pixel_ray(const HitCam& cam, int x, int y, float v[3], double d[3]) {
  const float fx = (float)x, fy = (float)y;
  const float p0 = (cam.kinv[0] * fx + cam.kinv[1] * fy) + cam.kinv[2] * 1.f;
  const float p1 = (cam.kinv[3] * fx + cam.kinv[4] * fy) + cam.kinv[5] * 1.f;
  const float p2 = (cam.kinv[6] * fx + cam.kinv[7] * fy) + cam.kinv[8] * 1.f;
  // correctly rounded fp32 sqrt and division, through fp64 (53 >= 2 * 24 + 2 bits: the second rounding is innocuous);
  // __fsqrt_rn is the native approximation unless the rounded OCML operations are compiled in
  const float len = (float)__dsqrt_rn((double)((p0 * p0 + p1 * p1) + p2 * p2));
  v[0] = (float)((double)p0 / (double)len);
  v[1] = (float)((double)p1 / (double)len);
  v[2] = (float)((double)p2 / (double)len);
  d[0] = (double)((cam.rot[0] * v[0] + cam.rot[1] * v[1]) + cam.rot[2] * v[2]);
  d[1] = (double)((cam.rot[3] * v[0] + cam.rot[4] * v[1]) + cam.rot[5] * v[2]);
  d[2] = (double)((cam.rot[6] * v[0] + cam.rot[7] * v[1]) + cam.rot[8] * v[2]);
}

}  // namespace ufr
