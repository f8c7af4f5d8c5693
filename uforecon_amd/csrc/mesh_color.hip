// Mesh colouring on the device: per-vertex colour from the photographs, visibility-aware, and the Jacobi round that hands
// colour on to vertices no photograph saw, with the arithmetic that tests/color_mesh_ref.py restates (include/ufr.h,
// ufr_color_vertices and ufr_color_fill_round).  The reference has no such stage.
//
//   cams_upload    the camera records (k, w2c's rotation and translation, the centre: 24 doubles a view) arrive as kernel
//          arguments, kColorCamsPerLaunch views a launch, and are written to the caller's workspace: no copy from host
//          memory, nothing to wait for.
//   vertex_colors  one thread per vertex; it walks the views in ascending order, so a vertex's sums are taken in view order
//          whatever the launch shape, with no atomic.  The vertex and its normal are loaded once; a view's record is read
//          through a wave-uniform index.  Per view, in fp64, every product and sum rounded on its own:
//            c = R p + t (the three products, then the translation); skipped unless p and c are finite and c.z > z_min
//            q = k c, x = q.x / q.z, y = q.y / q.z, x0 = floor(x), y0 = floor(y), fx = x - x0, fy = y - y0
//            skipped unless 0 <= x0, x0 + 1 <= W - 1, 0 <= y0, y0 + 1 <= H - 1 (NaN and the infinities fail here too)
//            angle:     d = (p - centre) / |p - centre|, cosv = |N . d|; skipped unless cosv >= min_cos and cosv > 0
//            occlusion: the four depths under the footprint all > 0 and c.z <= (1 + depth_tol) * their minimum
//            w = cosv multiplied up `power` times; s = (1 - fy) * ((1 - fx) * I00 + fx * I01) + fy * ((1 - fx) * I10 + fx * I11)
//            mean: A += w * s, Wsum += w;  best: the largest w, ties to the earlier view
//          colour = rint(A / Wsum) or rint(s of the best view), clamped to 0..255; no view: the fill colour.
//          The tests that need no memory (projection, bounds, angle) come before the four depth loads, and those before the
//          twelve byte loads: a skipped view costs as little as it can.  The order of the tests cannot change a result.
//   fill_round     one thread per vertex.  A vertex with a state is copied.  An empty one walks its corner run (the layout of
//          raster.hip's vertex normals) in ascending position and, per slot 3f + e, visits corners (e + 1) % 3 and (e + 2) % 3
//          of face f: integer sums of the coloured ones, the mean rounded half to even.  Reads the in buffers only and writes
//          the out buffers only, so a round does not depend on scheduling.
//
// Block shape: kColorThreads (256) threads, no LDS.  Every index read from a caller's array is range-checked before it is used.
#include "mesh_rows.h"

namespace ufr {
namespace {

constexpr double kDblMax = 1.7976931348623157e308;

struct ColorCamChunk {
  MeshColorCam v[kColorCamsPerLaunch];
};
static_assert(sizeof(ColorCamChunk) + 64 <= 4096, "the chunk must fit a launch's argument segment");

__global__ void __launch_bounds__(kColorThreads) color_cams_upload_kernel(ColorCamChunk c, int count, MeshColorCam* __restrict__ table) {
  constexpr int per = (int)(sizeof(MeshColorCam) / sizeof(double));
  const int i = blockIdx.x * kColorThreads + threadIdx.x;
  if (i >= count * per) return;
  reinterpret_cast<double*>(table)[i] = reinterpret_cast<const double*>(c.v)[i];
}

__device__ inline bool finite3(double a, double b, double c) { return fabs(a) <= kDblMax && fabs(b) <= kDblMax && fabs(c) <= kDblMax; }

__device__ inline unsigned char to_byte(double v) {
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

__global__ void __launch_bounds__(kColorThreads) vertex_colors_kernel(const double* __restrict__ verts, const double* __restrict__ normals,
                                                                       long long V, const unsigned char* __restrict__ images,
                                                                       const float* __restrict__ depth,
                                                                       const MeshColorCam* __restrict__ cams, int n_views, int H, int W,
                                                                       ColorArgs a, unsigned char* __restrict__ colors,
                                                                       unsigned char* __restrict__ views_used) {
  const long long v = (long long)blockIdx.x * kColorThreads + threadIdx.x;
  if (v >= V) return;
  const double px = verts[3 * v], py = verts[3 * v + 1], pz = verts[3 * v + 2];
  double nx = 0.0, ny = 0.0, nz = 0.0;
  if (normals) nx = normals[3 * v], ny = normals[3 * v + 1], nz = normals[3 * v + 2];
  double A0 = 0.0, A1 = 0.0, A2 = 0.0, Ws = 0.0, bw = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  int used = 0;
  const int views = finite3(px, py, pz) ? n_views : 0;
  for (int k = 0; k < views; ++k) {
    const MeshColorCam& cam = cams[k];
    const double c0 = ((cam.r[0] * px + cam.r[1] * py) + cam.r[2] * pz) + cam.t[0];
    const double c1 = ((cam.r[3] * px + cam.r[4] * py) + cam.r[5] * pz) + cam.t[1];
    const double c2 = ((cam.r[6] * px + cam.r[7] * py) + cam.r[8] * pz) + cam.t[2];
    if (!finite3(c0, c1, c2)) continue;
    if (!(c2 > a.z_min)) continue;
    const double q0 = (cam.k[0] * c0 + cam.k[1] * c1) + cam.k[2] * c2;
    const double q1 = (cam.k[3] * c0 + cam.k[4] * c1) + cam.k[5] * c2;
    const double q2 = (cam.k[6] * c0 + cam.k[7] * c1) + cam.k[8] * c2;
    const double x = q0 / q2, y = q1 / q2;
    const double xf = floor(x), yf = floor(y);
    // NaN and the infinities fail here; what passes fits an int
    if (!(xf >= 0.0 && xf + 1.0 <= (double)(W - 1) && yf >= 0.0 && yf + 1.0 <= (double)(H - 1))) continue;
    const double fx = x - xf, fy = y - yf;
    double cosv = 1.0;
    if (normals) {
      const double e0 = px - cam.c[0], e1 = py - cam.c[1], e2 = pz - cam.c[2];
      const double len = __dsqrt_rn((e0 * e0 + e1 * e1) + e2 * e2);
      const double d0 = e0 / len, d1 = e1 / len, d2 = e2 / len;
      cosv = fabs((nx * d0 + ny * d1) + nz * d2);
      if (!(cosv >= a.min_cos && cosv > 0.0)) continue;   // NaN too: a vertex at the camera centre
    }
    const long long t00 = ((long long)k * H + (int)yf) * W + (int)xf;   // texel (y0, x0) of view k: in range by the test above
    if (depth) {
      const float d00 = depth[t00], d01 = depth[t00 + 1], d10 = depth[t00 + W], d11 = depth[t00 + W + 1];
      if (!(d00 > 0.f && d01 > 0.f && d10 > 0.f && d11 > 0.f)) continue;
      const float dm = fminf(fminf(d00, d01), fminf(d10, d11));
      if (!(c2 <= a.one_tol * (double)dm)) continue;
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
    A0 = A0 + w * s[0];
    A1 = A1 + w * s[1];
    A2 = A2 + w * s[2];
    Ws = Ws + w;
    if (used == 0 || w > bw) bw = w, b0 = s[0], b1 = s[1], b2 = s[2];
    ++used;
  }
  unsigned char o0 = a.fill[0], o1 = a.fill[1], o2 = a.fill[2];
  if (used > 0) {
    const bool best = a.mode == UFR_MESH_COLOR_BEST;
    o0 = to_byte(best ? b0 : A0 / Ws);
    o1 = to_byte(best ? b1 : A1 / Ws);
    o2 = to_byte(best ? b2 : A2 / Ws);
  }
  colors[3 * v] = o0;
  colors[3 * v + 1] = o1;
  colors[3 * v + 2] = o2;
  views_used[v] = (unsigned char)used;
}

__device__ inline unsigned char mean_half_even(long long sum, long long count) {
  const long long quo = sum / count, rem = sum % count;
  const bool up = 2 * rem > count || (2 * rem == count && (quo & 1));
  return (unsigned char)(quo + (up ? 1 : 0));
}

__global__ void __launch_bounds__(kColorThreads) color_fill_round_kernel(const int* __restrict__ faces, long long V, long long F,
                                                                          const long long* __restrict__ slots,
                                                                          const long long* __restrict__ runs,
                                                                          const unsigned char* __restrict__ colors_in,
                                                                          const unsigned char* __restrict__ state_in,
                                                                          unsigned char* __restrict__ colors_out,
                                                                          unsigned char* __restrict__ state_out, int* __restrict__ filled) {
  const long long v = (long long)blockIdx.x * kColorThreads + threadIdx.x;
  if (v >= V) return;
  unsigned char o0 = colors_in[3 * v], o1 = colors_in[3 * v + 1], o2 = colors_in[3 * v + 2], st = state_in[v];
  if (st == 0) {
    long long i0, i1;
    run_of(runs, v, 3 * F, &i0, &i1);
    long long s0 = 0, s1 = 0, s2 = 0, count = 0;
    for (long long i = i0; i < i1; ++i) {
      const long long slot = slots[i];
      if (!slot_names(slot, faces, F, v)) continue;
      const long long f = slot / 3;
      const int e = (int)(slot - 3 * f);
#pragma unroll
      for (int j = 1; j <= 2; ++j) {
        const long long u = faces[3 * f + (e + j) % 3];
        if (u < 0 || u >= V || state_in[u] == 0) continue;
        s0 += colors_in[3 * u];
        s1 += colors_in[3 * u + 1];
        s2 += colors_in[3 * u + 2];
        ++count;
      }
    }
    if (count > 0) {
      o0 = mean_half_even(s0, count);
      o1 = mean_half_even(s1, count);
      o2 = mean_half_even(s2, count);
      st = 1;
      atomicAdd(filled, 1);
    }
  }
  colors_out[3 * v] = o0;
  colors_out[3 * v + 1] = o1;
  colors_out[3 * v + 2] = o2;
  state_out[v] = st;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kColorThreads - 1) / kColorThreads); }

}  // namespace

hipError_t launch_mesh_color_cams(const MeshColorCam* cams_host, int n_views, MeshColorCam* table, hipStream_t s) {
  constexpr int per = (int)(sizeof(MeshColorCam) / sizeof(double));
  for (int first = 0; first < n_views; first += kColorCamsPerLaunch) {
    ColorCamChunk c;
    const int count = n_views - first < kColorCamsPerLaunch ? n_views - first : kColorCamsPerLaunch;
    for (int t = 0; t < kColorCamsPerLaunch; ++t) c.v[t] = cams_host[first + (t < count ? t : 0)];
    hipLaunchKernelGGL(color_cams_upload_kernel, dim3(blocks_of((long long)count * per)), dim3(kColorThreads), 0, s, c, count,
                       table + first);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_mesh_vertex_colors(const double* verts, const double* normals, long long V, const unsigned char* images,
                                     const float* depth, const MeshColorCam* table, int n_views, int H, int W, double z_min,
                                     double depth_tol, double min_cos, int power, int mode, const unsigned char* fill,
                                     unsigned char* colors, unsigned char* views_used, hipStream_t s) {
  ColorArgs a;
  a.z_min = z_min, a.one_tol = 1.0 + depth_tol, a.min_cos = min_cos, a.power = power, a.mode = mode;
  for (int c = 0; c < 3; ++c) a.fill[c] = fill[c];
  hipLaunchKernelGGL(vertex_colors_kernel, dim3(blocks_of(V)), dim3(kColorThreads), 0, s, verts, normals, V, images, depth, table,
                     n_views, H, W, a, colors, views_used);
  return hipGetLastError();
}

hipError_t launch_mesh_color_fill_round(const int* faces, long long V, long long F, const long long* slots, const long long* runs,
                                        const unsigned char* colors_in, const unsigned char* state_in, unsigned char* colors_out,
                                        unsigned char* state_out, int* filled, hipStream_t s) {
  hipLaunchKernelGGL(color_fill_round_kernel, dim3(blocks_of(V)), dim3(kColorThreads), 0, s, faces, V, F, slots, runs, colors_in,
                     state_in, colors_out, state_out, filled);
  return hipGetLastError();
}

}  // namespace ufr
