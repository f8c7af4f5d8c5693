// Mesh texturing on the device: a per-face atlas baked from the photographs, and the Jacobi round that hands colour on to
// texels no photograph saw, with the arithmetic that tests/texture_ref.py restates (include/ufr.h, "mesh texturing").  The
// reference has no such stage.  The textured shading of ufr_texture_frames is raster.hip's shade kernel, told to take its
// colour from the atlas.
//
//   the atlas      closed form, so host and device agree by construction.  Patch size S (texel steps along a triangle's legs),
//          cell side C = S + 3.  Faces 2q and 2q + 1 share cell q, at column q % cols and row q / cols of a grid of cols x rows
//          cells: Wt = cols * C, Ht = rows * C.  Local texel (i, j) of a cell belongs to the even face when i + j <= S + 2, else to
//          the odd face with (i, j) := (C - 1 - i, C - 1 - j): a half turn, nothing is mirrored.  A face's corners sit at local
//          (0, 0), (S, 0), (0, S); a texel's weights are wb = i / S, wc = j / S, wa = (1 - wb) - wc, negative in the gutter.
//          texel_owner below is the one statement of this on the device.
//   bake           one thread per texel.  It loads its face's three corners, forms p = (wa a + wb b) + wc c and the face normal
//          (b - a) x (c - a) / its length (zero when the length is not > 0 or not finite: no view sees it), then walks the
//          views in ascending order with the per-view rule of mesh colouring (mesh_color_rule.h).  No view: the barycentric mix
//          of the face's fallback colours when given, else the fill colour.  No face, or a face with an index outside
//          0..V-1: the fill colour.  Nothing synchronises and there is no atomic.
//   fill_round     one thread per texel, integers only.  A texel with a state, or of no face, is copied.  An empty one visits
//          (x-1, y), (x+1, y), (x, y-1), (x, y+1) in that order; a neighbour counts when it is inside the atlas, belongs to the
//          same face and has a state: the mean of those, rounded half to even.  Reads the in buffers only and writes the out
//          buffers only, so a round does not depend on scheduling.
//
// Block shape: kTextureThreads (256) threads.  Thread order of the bake: see profiles/mesh_texture_launch_shapes.md.  Every index
// read from a caller's array is range-checked before it is used; texel indices are formed from the closed form alone.
#include "mesh_color_rule.h"

namespace ufr {
namespace {

// the face that owns texel (x, y) and the texel's place (i, j) in that face's patch; false: no face
__device__ inline bool texel_owner(const TextureAtlas& at, int x, int y, long long* f, int* i, int* j) {
  const int C = at.S + 3;
  const int cx = x / C, cy = y / C;
  int li = x - cx * C, lj = y - cy * C;
  const long long q = (long long)cy * at.cols + cx;
  long long face = 2 * q;
  if (li + lj > at.S + 2) {
    face += 1;
    li = C - 1 - li;
    lj = C - 1 - lj;
  }
  *f = face, *i = li, *j = lj;
  return face < at.F;
}

// a face as the bake needs it: corners, unit normal (or zero), fallback colours of the corners; live: all indices in 0..V-1
struct BakeFace {
  double a[3], b[3], c[3], n[3], fa[3], fb[3], fc[3];
  int live;
};

__device__ inline void load_bake_face(const double* __restrict__ verts, const int* __restrict__ faces, long long V, long long f,
                                      const unsigned char* __restrict__ fallback, BakeFace* o) {
  const long long ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  o->live = ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V;
  if (!o->live) return;
  double u[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o->a[k] = verts[3 * ia + k];
    o->b[k] = verts[3 * ib + k];
    o->c[k] = verts[3 * ic + k];
    u[k] = o->b[k] - o->a[k];
    w[k] = o->c[k] - o->a[k];
    o->fa[k] = fallback ? (double)fallback[3 * ia + k] : 0.0;
    o->fb[k] = fallback ? (double)fallback[3 * ib + k] : 0.0;
    o->fc[k] = fallback ? (double)fallback[3 * ic + k] : 0.0;
  }
  const double n0 = u[1] * w[2] - u[2] * w[1];
  const double n1 = u[2] * w[0] - u[0] * w[2];
  const double n2 = u[0] * w[1] - u[1] * w[0];
  const double len = __dsqrt_rn((n0 * n0 + n1 * n1) + n2 * n2);
  const bool ok = len > 0.0 && len <= kColorDblMax;   // zero, NaN and an overflowed length give the zero normal
  o->n[0] = ok ? n0 / len : 0.0;
  o->n[1] = ok ? n1 / len : 0.0;
  o->n[2] = ok ? n2 / len : 0.0;
}

// the colour and the view count of the texel at (i, j) of a live face's patch
__device__ inline int bake_texel(const BakeFace& fc, int i, int j, int S, const unsigned char* __restrict__ images,
                                 const float* __restrict__ depth, const MeshColorCam* __restrict__ cams, int n_views, int H, int W,
                                 const ColorArgs& a, bool has_fallback, unsigned char* o) {
  const double wb = (double)i / (double)S, wc = (double)j / (double)S;
  const double wa = (1.0 - wb) - wc;
  const double px = (wa * fc.a[0] + wb * fc.b[0]) + wc * fc.c[0];
  const double py = (wa * fc.a[1] + wb * fc.b[1]) + wc * fc.c[1];
  const double pz = (wa * fc.a[2] + wb * fc.b[2]) + wc * fc.c[2];
  ColorAcc acc;
  const int views = color_finite3(px, py, pz) ? n_views : 0;
  for (int k = 0; k < views; ++k) color_view(cams[k], k, px, py, pz, true, fc.n[0], fc.n[1], fc.n[2], images, depth, H, W, a, acc);
  if (acc.used > 0) {
    color_resolve(acc, a.mode, o);
  } else if (has_fallback) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = color_to_byte((wa * fc.fa[k] + wb * fc.fb[k]) + wc * fc.fc[k]);
  }
  return acc.used;
}

// Thread order.  kCellMajor false: thread t owns texel (t % Wt, t / Wt), atlas row-major; every thread loads its own face.
// kCellMajor true: thread t owns local texel t % C^2 of cell t / C^2 (row-major inside the cell); the at most
// kTextureStagedFaces faces of the cells a block touches are loaded once, by the block's first threads, into LDS.
constexpr int kTextureStagedFaces = 2 * (kTextureThreads / 16 + 1);   // C >= 4: a block spans at most 256 / 16 + 1 cells

template <bool kCellMajor>
__global__ void __launch_bounds__(kTextureThreads) texture_bake_kernel(const double* __restrict__ verts, const int* __restrict__ faces,
                                                                        long long V, TextureAtlas at,
                                                                        const unsigned char* __restrict__ images,
                                                                        const float* __restrict__ depth,
                                                                        const MeshColorCam* __restrict__ cams, int n_views, int H, int W,
                                                                        ColorArgs a, const unsigned char* __restrict__ fallback,
                                                                        unsigned char* __restrict__ texture,
                                                                        unsigned char* __restrict__ views_used) {
  const long long total = (long long)at.Ht * at.Wt;
  const long long t = (long long)blockIdx.x * kTextureThreads + threadIdx.x;
  const int C = at.S + 3;
  int x = 0, y = 0;
  if constexpr (kCellMajor) {
    __shared__ BakeFace staged[kTextureStagedFaces];
    const long long cell_texels = (long long)C * C;
    const long long first = (long long)blockIdx.x * kTextureThreads;
    long long last = first + kTextureThreads - 1;
    if (last > total - 1) last = total - 1;
    const long long q0 = first / cell_texels, q1 = last / cell_texels;
    const int n_staged = (int)(2 * (q1 - q0 + 1));   // <= kTextureStagedFaces
    if ((int)threadIdx.x < n_staged) {
      const long long f = 2 * q0 + threadIdx.x;
      staged[threadIdx.x].live = 0;
      if (f < at.F) load_bake_face(verts, faces, V, f, fallback, &staged[threadIdx.x]);
    }
    __syncthreads();
    if (t >= total) return;
    const long long q = t / cell_texels;
    const int l = (int)(t - q * cell_texels);
    const int lj = l / C, li = l - lj * C;
    x = (int)(q % at.cols) * C + li;
    y = (int)(q / at.cols) * C + lj;
    long long f;
    int i, j;
    unsigned char o[3] = {a.fill[0], a.fill[1], a.fill[2]};
    int used = 0;
    if (texel_owner(at, x, y, &f, &i, &j)) {
      const BakeFace& fc = staged[(int)(f - 2 * q0)];
      if (fc.live) used = bake_texel(fc, i, j, at.S, images, depth, cams, n_views, H, W, a, fallback != nullptr, o);
    }
    const long long out = (long long)y * at.Wt + x;
    texture[3 * out] = o[0], texture[3 * out + 1] = o[1], texture[3 * out + 2] = o[2];
    views_used[out] = (unsigned char)used;
  } else {
    if (t >= total) return;
    y = (int)(t / at.Wt), x = (int)(t - (long long)y * at.Wt);
    long long f;
    int i, j;
    unsigned char o[3] = {a.fill[0], a.fill[1], a.fill[2]};
    int used = 0;
    if (texel_owner(at, x, y, &f, &i, &j)) {
      BakeFace fc;
      load_bake_face(verts, faces, V, f, fallback, &fc);
      if (fc.live) used = bake_texel(fc, i, j, at.S, images, depth, cams, n_views, H, W, a, fallback != nullptr, o);
    }
    texture[3 * t] = o[0], texture[3 * t + 1] = o[1], texture[3 * t + 2] = o[2];
    views_used[t] = (unsigned char)used;
  }
}

__global__ void __launch_bounds__(kTextureThreads) texture_fill_round_kernel(TextureAtlas at, const unsigned char* __restrict__ colors_in,
                                                                              const unsigned char* __restrict__ state_in,
                                                                              unsigned char* __restrict__ colors_out,
                                                                              unsigned char* __restrict__ state_out,
                                                                              int* __restrict__ filled) {
  const long long t = (long long)blockIdx.x * kTextureThreads + threadIdx.x;
  if (t >= (long long)at.Ht * at.Wt) return;
  const int y = (int)(t / at.Wt), x = (int)(t - (long long)y * at.Wt);
  unsigned char o0 = colors_in[3 * t], o1 = colors_in[3 * t + 1], o2 = colors_in[3 * t + 2], st = state_in[t];
  long long f;
  int i, j;
  if (st == 0 && texel_owner(at, x, y, &f, &i, &j)) {
    const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
    long long s0 = 0, s1 = 0, s2 = 0, count = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ux = x + dx[k], uy = y + dy[k];
      if (ux < 0 || ux >= at.Wt || uy < 0 || uy >= at.Ht) continue;
      long long g;
      int gi, gj;
      if (!texel_owner(at, ux, uy, &g, &gi, &gj) || g != f) continue;
      const long long u = (long long)uy * at.Wt + ux;
      if (state_in[u] == 0) continue;
      s0 += colors_in[3 * u];
      s1 += colors_in[3 * u + 1];
      s2 += colors_in[3 * u + 2];
      ++count;
    }
    if (count > 0) {
      o0 = mean_half_even(s0, count);
      o1 = mean_half_even(s1, count);
      o2 = mean_half_even(s2, count);
      st = 1;
      atomicAdd(filled, 1);
    }
  }
  colors_out[3 * t] = o0;
  colors_out[3 * t + 1] = o1;
  colors_out[3 * t + 2] = o2;
  state_out[t] = st;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kTextureThreads - 1) / kTextureThreads); }

}  // namespace

hipError_t launch_texture_bake(const double* verts, const int* faces, long long V, const TextureAtlas& at, const unsigned char* images,
                               const float* depth, const MeshColorCam* table, int n_views, int H, int W, double z_min,
                               double depth_tol, double min_cos, int power, int mode, const unsigned char* fill,
                               const unsigned char* fallback, unsigned char* texture, unsigned char* views_used, hipStream_t s) {
  const ColorArgs a = make_color_args(z_min, depth_tol, min_cos, power, mode, fill);
  hipLaunchKernelGGL(texture_bake_kernel<kTextureBakeCellMajor>, dim3(blocks_of((long long)at.Ht * at.Wt)), dim3(kTextureThreads), 0, s,
                     verts, faces, V, at, images, depth, table, n_views, H, W, a, fallback, texture, views_used);
  return hipGetLastError();
}

hipError_t launch_texture_fill_round(const TextureAtlas& at, const unsigned char* colors_in, const unsigned char* state_in,
                                     unsigned char* colors_out, unsigned char* state_out, int* filled, hipStream_t s) {
  hipLaunchKernelGGL(texture_fill_round_kernel, dim3(blocks_of((long long)at.Ht * at.Wt)), dim3(kTextureThreads), 0, s, at, colors_in,
                     state_in, colors_out, state_out, filled);
  return hipGetLastError();
}

}  // namespace ufr
