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
//          (mesh_color_rule.h holds this per-view body: mesh_texture.hip runs the same per texel)
//          colour = rint(A / Wsum) or rint(s of the best view), clamped to 0..255; no view: the fill colour.
//          The tests that need no memory (projection, bounds, angle) come before the four depth loads, and those before the
//          twelve byte loads: a skipped view costs as little as it can.  The order of the tests cannot change a result.
//   fill_round     one thread per vertex.  A vertex with a state is copied.  An empty one walks its corner run (the layout of
//          raster.hip's vertex normals) in ascending position and, per slot 3f + e, visits corners (e + 1) % 3 and (e + 2) % 3
//          of face f: integer sums of the coloured ones, the mean rounded half to even.  Reads the in buffers only and writes
//          the out buffers only, so a round does not depend on scheduling.
//
// Block shape: kColorThreads (256) threads, no LDS.  Every index read from a caller's array is range-checked before it is used.
#include "mesh_color_rule.h"
#include "mesh_rows.h"

namespace ufr {
namespace {

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
  ColorAcc acc;
  const int views = color_finite3(px, py, pz) ? n_views : 0;
  for (int k = 0; k < views; ++k) color_view(cams[k], k, px, py, pz, normals != nullptr, nx, ny, nz, images, depth, H, W, a, acc);
  unsigned char o[3] = {a.fill[0], a.fill[1], a.fill[2]};
  if (acc.used > 0) color_resolve(acc, a.mode, o);
  colors[3 * v] = o[0];
  colors[3 * v + 1] = o[1];
  colors[3 * v + 2] = o[2];
  views_used[v] = (unsigned char)acc.used;
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
  const ColorArgs a = make_color_args(z_min, depth_tol, min_cos, power, mode, fill);
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
