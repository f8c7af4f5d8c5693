// The per-(point, view) rule of mesh colouring and mesh texturing (include/ufr.h, ufr_color_vertices states it): projection,
// bounds, angle, the conservative four-texel depth test, the cos^power weight, the bilinear sample and the accumulation.
// mesh_color.hip runs it per vertex, mesh_texture.hip per texel of the atlas: one statement, so a texel on a vertex sees
// what the vertex saw.  Everything is fp64, every product and sum rounded on its own.  Only kernel files include this.
#pragma once
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {

constexpr double kColorDblMax = 1.7976931348623157e308;

__device__ inline bool color_finite3(double a, double b, double c) {
  return fabs(a) <= kColorDblMax && fabs(b) <= kColorDblMax && fabs(c) <= kColorDblMax;
}

__device__ inline unsigned char color_to_byte(double v) {
  double p = rint(v);          // round half to even
  if (!(p >= 0.0)) p = 0.0;    // NaN too
  if (p > 255.0) p = 255.0;
  return (unsigned char)(int)p;
}

struct ColorArgs {
  double z_min, one_tol, min_cos;   // one_tol = 1 + depth_tol, rounded once on the host
  int power, mode;
  unsigned char fill[3];
};

inline ColorArgs make_color_args(double z_min, double depth_tol, double min_cos, int power, int mode, const unsigned char* fill) {
  ColorArgs a;
  a.z_min = z_min, a.one_tol = 1.0 + depth_tol, a.min_cos = min_cos, a.power = power, a.mode = mode;
  for (int c = 0; c < 3; ++c) a.fill[c] = fill[c];
  return a;
}

// what a point gathers over its views: the weighted sums (mean), the best view's sample (best), the views not skipped
struct ColorAcc {
  double A0 = 0.0, A1 = 0.0, A2 = 0.0, Ws = 0.0, bw = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  int used = 0;
};

// View k of the point (px, py, pz): skipped, or added to acc.  has_normal false: no angle test, every view weighs 1.
// The tests that need no memory (projection, bounds, angle) come before the four depth loads, and those before the twelve
// byte loads: a skipped view costs as little as it can.  The order of the tests cannot change a result.
__device__ inline void color_view(const MeshColorCam& cam, int k, double px, double py, double pz, bool has_normal, double nx,
                                  double ny, double nz, const unsigned char* __restrict__ images, const float* __restrict__ depth,
                                  int H, int W, const ColorArgs& a, ColorAcc& acc) {
  const double c0 = ((cam.r[0] * px + cam.r[1] * py) + cam.r[2] * pz) + cam.t[0];
  const double c1 = ((cam.r[3] * px + cam.r[4] * py) + cam.r[5] * pz) + cam.t[1];
  const double c2 = ((cam.r[6] * px + cam.r[7] * py) + cam.r[8] * pz) + cam.t[2];
  if (!color_finite3(c0, c1, c2)) return;
  if (!(c2 > a.z_min)) return;
  const double q0 = (cam.k[0] * c0 + cam.k[1] * c1) + cam.k[2] * c2;
  const double q1 = (cam.k[3] * c0 + cam.k[4] * c1) + cam.k[5] * c2;
  const double q2 = (cam.k[6] * c0 + cam.k[7] * c1) + cam.k[8] * c2;
  const double x = q0 / q2, y = q1 / q2;
  const double xf = floor(x), yf = floor(y);
  // NaN and the infinities fail here; what passes fits an int
  if (!(xf >= 0.0 && xf + 1.0 <= (double)(W - 1) && yf >= 0.0 && yf + 1.0 <= (double)(H - 1))) return;
  const double fx = x - xf, fy = y - yf;
  double cosv = 1.0;
  if (has_normal) {
    const double e0 = px - cam.c[0], e1 = py - cam.c[1], e2 = pz - cam.c[2];
    const double len = __dsqrt_rn((e0 * e0 + e1 * e1) + e2 * e2);
    const double d0 = e0 / len, d1 = e1 / len, d2 = e2 / len;
    cosv = fabs((nx * d0 + ny * d1) + nz * d2);
    if (!(cosv >= a.min_cos && cosv > 0.0)) return;   // NaN too: a point at the camera centre
  }
  const long long t00 = ((long long)k * H + (int)yf) * W + (int)xf;   // texel (y0, x0) of view k: in range by the test above
  if (depth) {
    const float d00 = depth[t00], d01 = depth[t00 + 1], d10 = depth[t00 + W], d11 = depth[t00 + W + 1];
    if (!(d00 > 0.f && d01 > 0.f && d10 > 0.f && d11 > 0.f)) return;
    const float dm = fminf(fminf(d00, d01), fminf(d10, d11));
    if (!(c2 <= a.one_tol * (double)dm)) return;
  }
  double w = 1.0;
  for (int j = 0; j < a.power; ++j) w = w * cosv;
  const unsigned char* r0 = images + 3 * t00;
  const unsigned char* r1 = r0 + 3 * (long long)W;
  const double gx = 1.0 - fx, gy = 1.0 - fy;
  double s[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    s[ch] = gy * (gx * (double)r0[ch] + fx * (double)r0[3 + ch]) + fy * (gx * (double)r1[ch] + fx * (double)r1[3 + ch]);
  acc.A0 = acc.A0 + w * s[0];
  acc.A1 = acc.A1 + w * s[1];
  acc.A2 = acc.A2 + w * s[2];
  acc.Ws = acc.Ws + w;
  if (acc.used == 0 || w > acc.bw) acc.bw = w, acc.b0 = s[0], acc.b1 = s[1], acc.b2 = s[2];
  ++acc.used;
}

// the colour of a point some view saw (acc.used > 0)
__device__ inline void color_resolve(const ColorAcc& acc, int mode, unsigned char* o) {
  const bool best = mode == UFR_MESH_COLOR_BEST;
  o[0] = color_to_byte(best ? acc.b0 : acc.A0 / acc.Ws);
  o[1] = color_to_byte(best ? acc.b1 : acc.A1 / acc.Ws);
  o[2] = color_to_byte(best ? acc.b2 : acc.A2 / acc.Ws);
}

// the integer mean of the fill rounds: sum / count rounded half to even
__device__ inline unsigned char mean_half_even(long long sum, long long count) {
  const long long quo = sum / count, rem = sum % count;
  const bool up = 2 * rem > count || (2 * rem == count && (quo & 1));
  return (unsigned char)(quo + (up ? 1 : 0));
}

}  // namespace ufr
