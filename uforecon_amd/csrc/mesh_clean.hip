// DTU mesh cleaning (the reference's evaluation/clean_mesh.py) on the device, with the arithmetic that tests/clean_mesh_ref.py
// restates (include/ufr.h, ufr_mask_dilate / ufr_mesh_*):
//
//   mask_dilate     one thread per pixel: the maximum of the uint8 image under cv.getStructuringElement(MORPH_ELLIPSE, (k, k)),
//          given as row half-widths (the host makes the table); pixels outside the image are ignored.
//   vertex_votes    one thread per (view, vertex): q = P[:3,:3] x + P[:3,3] in fp64 (P fp32, widened; products summed left to
//          right), q / q.z, round-half-even, then the reference's ones-border test.  Integer atomic adds: order-independent.
//   first_hit       rasterisation-shaped ray casting of one view.  All rays leave one centre, so a ray can only hit a triangle
//          inside the bounding box of its projection.  first_hit_small: one thread per triangle projects the three vertices with
//          the fp64 inverse of the ray generator (padded by kBoxPad pixels: the generator is fp32, its inverse is not exact),
//          and runs the exact test for the masked pixels of a box of at most kSmallBox pixels; a larger box goes to a list.
//          first_hit_big: one workgroup per listed triangle strides over its box.  A triangle with a vertex at camera depth
//          <= 0 (or a non-finite projection) gets the whole image; one wholly behind the camera is skipped (a ray with t > 0
//          only reaches points of positive depth).  The exact test, per pixel:
//            ray     fp32, as gen_rays_from_single_image: p = Kinv (x, y, 1), v = p / |p|, d = R v, every product summed left
//                    to right without fused multiply-add, sqrt and division correctly rounded (formed in fp64, narrowed)
//            edges   with a, b, c = the vertices - o in fp64: e_ab = d . (a x b), formed for the vertex pair in ascending
//                    index order and negated for the other direction, so the two faces of an edge see the same number with
//                    opposite signs and no ray passes between them.  Hit iff e_bc, e_ca, e_ab are all >= 0 or all <= 0 (both
//                    sides, edges and vertices inclusive) and not all zero
//            t       n = (b - a) x (c - a), t = (n . a) / (n . d); n . d = 0 (zero area, or edge-on) never hits; t > 0 only
//          and merges (float bits of t) << 32 | face into a 64-bit key image with an atomic minimum: the nearest (float) t wins,
//          ties go to the lowest face, whatever the order of arrival.  first_hit_resolve turns keys into face ids and sets the
//          per-face flags (every writer stores the same 1).  A null mask means every pixel (the renderer, raster.hip); the ray
//          and the triangle set-up live in mesh_ray.h, which the shading kernel shares.
//   face_components edge keys (lo << 32 | hi of the merged vertex ids, a unique negative key per slot of a degenerate face),
//          sorted by the caller; mark_pairs keeps the runs of exactly two as adjacent face pairs; then rounds of union-find:
//          hook (per pair, the larger root gets parent = min(parent, smaller root), atomically) and jump (every face to its
//          root), until a round hooks nothing.  parent[f] <= f always, so a chase ends and a root is its tree's lowest face.
//
// Block shape: 256 threads throughout, no LDS.  Every index read from a caller's array is range-checked before it is used.
#include "ufr_internal.h"
#include "mesh_ray.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kMcThreads = 256;
constexpr int kSmallBox = 64;        // pixels one thread tests itself; above: a workgroup
constexpr double kBoxPad = 0.0625;   // pixels added round a projected box (the fp32 ray generator's inverse is good to ~1e-3)
constexpr int kBigBlocks = 2048;

struct DilateElem { short hw[UFR_MASK_MAX_KERNEL]; };

__global__ void __launch_bounds__(kMcThreads) mask_dilate_kernel(const unsigned char* __restrict__ src, int H, int W, int r,
                                                                  DilateElem el, int thresh, unsigned char* __restrict__ dilated,
                                                                  unsigned char* __restrict__ mask) {
  const long long i = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (i >= (long long)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  int m = 0;
  for (int dy = -r; dy <= r; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;
    const int hw = el.hw[dy + r];
    const int x0 = max(0, x - hw), x1 = min(W - 1, x + hw);
    for (int xx = x0; xx <= x1; ++xx) m = max(m, (int)src[(long long)yy * W + xx]);
  }
  if (dilated) dilated[i] = (unsigned char)m;
  if (mask) mask[i] = m > thresh ? 1 : 0;
}

__global__ void __launch_bounds__(kMcThreads) vertex_votes_kernel(const double* __restrict__ verts, long long V,
                                                                   const float* __restrict__ P, int NV,
                                                                   const unsigned char* __restrict__ masks, int H, int W,
                                                                   int* __restrict__ votes) {
  const long long i = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (i >= V * NV) return;
  const int view = (int)(i / V);
  const long long v = i - (long long)view * V;
  const float* __restrict__ p = P + 12 * view;
  const double x = verts[3 * v], y = verts[3 * v + 1], z = verts[3 * v + 2];
  const double q0 = (((double)p[0] * x + (double)p[1] * y) + (double)p[2] * z) + (double)p[3];
  const double q1 = (((double)p[4] * x + (double)p[5] * y) + (double)p[6] * z) + (double)p[7];
  const double q2 = (((double)p[8] * x + (double)p[9] * y) + (double)p[10] * z) + (double)p[11];
  const double rx = rint(q0 / q2), ry = rint(q1 / q2);   // round half to even; q2 / q2 is 1 or NaN
  if (!(q2 / q2 == 1.0)) return;                         // q.z zero or non-finite
  if (!(rx >= -1.0 && rx <= (double)(W - 1) && ry >= -1.0 && ry <= (double)(H - 1))) return;   // NaN and infinities fail
  const int px = (int)rx, py = (int)ry;
  if (px == -1 || py == -1 || masks[((long long)view * H + py) * W + px] != 0) atomicAdd(&votes[v], 1);
}

// ------------------------------------------------------------------ first hit
// the pixel box of the triangle's projection, clamped to the image; false: nothing to test
__device__ inline bool tri_box(const HitCam& cam, const double world[9], int H, int W, int* x0, int* y0, int* x1, int* y1) {
  double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300;
  bool whole = false, front = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double* X = world + 3 * k;
    const double px = ((cam.proj[0] * X[0] + cam.proj[1] * X[1]) + cam.proj[2] * X[2]) + cam.proj[3];
    const double py = ((cam.proj[4] * X[0] + cam.proj[5] * X[1]) + cam.proj[6] * X[2]) + cam.proj[7];
    const double pz = ((cam.proj[8] * X[0] + cam.proj[9] * X[1]) + cam.proj[10] * X[2]) + cam.proj[11];
    if (!(pz < 0.0)) front = true;                       // zero and NaN count as "not behind"
    const double u = px / pz, v = py / pz;
    if (!(pz > 0.0) || !(fabs(u) < 1e15) || !(fabs(v) < 1e15)) {
      whole = true;
    } else {
      xmin = fmin(xmin, u);
      xmax = fmax(xmax, u);
      ymin = fmin(ymin, v);
      ymax = fmax(ymax, v);
    }
  }
  if (!front) return false;
  if (whole) {
    *x0 = 0, *y0 = 0, *x1 = W - 1, *y1 = H - 1;
    return true;
  }
  const double fx0 = floor(xmin - kBoxPad), fy0 = floor(ymin - kBoxPad), fx1 = ceil(xmax + kBoxPad), fy1 = ceil(ymax + kBoxPad);
  if (fx1 < 0.0 || fy1 < 0.0 || fx0 > (double)(W - 1) || fy0 > (double)(H - 1)) return false;
  *x0 = (int)fmax(fx0, 0.0);
  *y0 = (int)fmax(fy0, 0.0);
  *x1 = (int)fmin(fx1, (double)(W - 1));
  *y1 = (int)fmin(fy1, (double)(H - 1));
  return true;
}

// the exact test of pixel (x, y)'s ray against the triangle; merges into the key image on a hit
__device__ inline void test_pixel(const HitCam& cam, const Tri& t, unsigned int face, int x, int y, int W,
                                  unsigned long long* __restrict__ keys) {
  float v[3];
  double d[3];
  pixel_ray(cam, x, y, v, d);
  const double e0 = dot3(d, t.cbc), e1 = dot3(d, t.cca), e2 = dot3(d, t.cab);
  const bool pos = e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0, neg = e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0;
  if (!(pos || neg) || (pos && neg)) return;             // NaN fails both; all zero passes both
  const double den = dot3(t.n, d);
  if (!(den > 0.0 || den < 0.0)) return;
  const double tt = t.na / den;
  if (!(tt > 0.0)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint((float)tt) << 32) | face;
  atomicMin(&keys[(long long)y * W + x], key);
}

__global__ void __launch_bounds__(kMcThreads) first_hit_small_kernel(const double* __restrict__ verts, const int* __restrict__ faces,
                                                                      long long V, long long F, HitCam cam,
                                                                      const unsigned char* __restrict__ mask, int H, int W,
                                                                      unsigned long long* __restrict__ keys, int* __restrict__ big_count,
                                                                      int* __restrict__ big_list) {
  const long long f = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (f >= F) return;
  Tri t;
  double world[9];
  if (!load_tri(verts, faces, V, f, cam, &t, world)) return;
  int x0, y0, x1, y1;
  if (!tri_box(cam, world, H, W, &x0, &y0, &x1, &y1)) return;
  if ((long long)(x1 - x0 + 1) * (y1 - y0 + 1) > kSmallBox) {
    const int slot = atomicAdd(big_count, 1);
    if (slot >= 0 && slot < F) big_list[slot] = (int)f;   // at most one slot per face: never beyond F
    return;
  }
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x)
      if (!mask || mask[(long long)y * W + x] != 0) test_pixel(cam, t, (unsigned int)f, x, y, W, keys);
}

__global__ void __launch_bounds__(kMcThreads) first_hit_big_kernel(const double* __restrict__ verts, const int* __restrict__ faces,
                                                                    long long V, long long F, HitCam cam,
                                                                    const unsigned char* __restrict__ mask, int H, int W,
                                                                    unsigned long long* __restrict__ keys,
                                                                    const int* __restrict__ big_count,
                                                                    const int* __restrict__ big_list) {
  const long long n = min((long long)*big_count, F);
  for (long long i = blockIdx.x; i < n; i += gridDim.x) {
    const long long f = big_list[i];
    if (f < 0 || f >= F) continue;
    Tri t;
    double world[9];
    if (!load_tri(verts, faces, V, f, cam, &t, world)) continue;
    int x0, y0, x1, y1;
    if (!tri_box(cam, world, H, W, &x0, &y0, &x1, &y1)) continue;
    const int bw = x1 - x0 + 1;
    const long long area = (long long)bw * (y1 - y0 + 1);
    for (long long j = threadIdx.x; j < area; j += kMcThreads) {
      const int y = y0 + (int)(j / bw), x = x0 + (int)(j % bw);
      if (!mask || mask[(long long)y * W + x] != 0) test_pixel(cam, t, (unsigned int)f, x, y, W, keys);
    }
  }
}

__global__ void __launch_bounds__(kMcThreads) first_hit_resolve_kernel(const unsigned long long* __restrict__ keys, long long n,
                                                                        long long F, int* __restrict__ face_id,
                                                                        unsigned char* __restrict__ face_hit) {
  const long long i = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  const long long f = (long long)(k & 0xffffffffull);
  const bool hit = k != ~0ull && f < F;
  face_id[i] = hit ? (int)f : -1;
  if (hit && face_hit) face_hit[f] = 1;
}

// ------------------------------------------------------------------ components
__global__ void __launch_bounds__(kMcThreads) edge_keys_kernel(const int* __restrict__ faces, const int* __restrict__ vid, long long V,
                                                                long long F, long long* __restrict__ keys) {
  const long long f = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (f >= F) return;
  int v[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = faces[3 * f + k];
    ok = ok && i >= 0 && i < V;
    v[k] = ok ? (vid ? vid[i] : i) : -1;
    ok = ok && v[k] >= 0;
  }
  ok = ok && v[0] != v[1] && v[1] != v[2] && v[2] != v[0];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = v[k], b = v[(k + 1) % 3];
    const long long lo = a < b ? a : b, hi = a < b ? b : a;
    keys[3 * f + k] = ok ? ((lo << 32) | hi) : -(3 * f + k + 1);   // a degenerate face's slots pair with nothing
  }
}

// position i of the sorted keys starts a run of exactly two: the faces of its two slots are adjacent
__global__ void __launch_bounds__(kMcThreads) mark_pairs_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                                 long long n, long long F, int* __restrict__ pair_a,
                                                                 int* __restrict__ pair_b, unsigned char* __restrict__ has_adj) {
  const long long i = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (i >= n) return;
  int a = -1, b = -1;
  if (i + 1 < n) {
    const long long k = keys[i];
    const bool two = k >= 0 && keys[i + 1] == k && (i == 0 || keys[i - 1] != k) && (i + 2 >= n || keys[i + 2] != k);
    const long long sa = order[i], sb = order[i + 1];
    if (two && sa >= 0 && sa < 3 * F && sb >= 0 && sb < 3 * F && sa / 3 != sb / 3) {
      a = (int)(sa / 3);
      b = (int)(sb / 3);
      has_adj[a] = 1;
      has_adj[b] = 1;
    }
  }
  pair_a[i] = a;
  pair_b[i] = b;
}

__global__ void __launch_bounds__(kMcThreads) iota_kernel(int* __restrict__ parent, long long F) {
  const long long i = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (i < F) parent[i] = (int)i;
}

// parent[x] <= x, and only ever decreases: the chase ends at a face that was a root when it was read
__device__ inline int find_root(const int* parent, int x) {
  int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) {
    x = p;
    p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return x;
}

__global__ void __launch_bounds__(kMcThreads) hook_kernel(const int* __restrict__ pair_a, const int* __restrict__ pair_b, long long n,
                                                           int* parent, int* __restrict__ changed) {
  const long long i = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (i >= n) return;
  const int a = pair_a[i];
  if (a < 0) return;
  const int ra = find_root(parent, a), rb = find_root(parent, pair_b[i]);
  if (ra == rb) return;
  atomicMin(&parent[ra > rb ? ra : rb], ra > rb ? rb : ra);
  *changed = 1;
}

__global__ void __launch_bounds__(kMcThreads) jump_kernel(int* parent, long long F) {
  const long long i = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (i >= F) return;
  const int r = find_root(parent, (int)i);
  if (r != (int)i) __hip_atomic_store(&parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kMcThreads) labels_kernel(const int* __restrict__ parent, const unsigned char* __restrict__ has_adj,
                                                             long long F, int* __restrict__ labels) {
  const long long i = (long long)blockIdx.x * kMcThreads + threadIdx.x;
  if (i < F) labels[i] = has_adj[i] ? parent[i] : -1;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kMcThreads - 1) / kMcThreads); }

}  // namespace

hipError_t launch_mask_dilate(const unsigned char* src, int H, int W, int k, const short* half_widths, int thresh,
                              unsigned char* dilated, unsigned char* mask, hipStream_t s) {
  DilateElem el;
  for (int i = 0; i < UFR_MASK_MAX_KERNEL; ++i) el.hw[i] = i < k ? half_widths[i] : 0;
  hipLaunchKernelGGL(mask_dilate_kernel, dim3(blocks_of((long long)H * W)), dim3(kMcThreads), 0, s, src, H, W, k / 2, el, thresh,
                     dilated, mask);
  return hipGetLastError();
}

hipError_t launch_vertex_votes(const double* verts, long long V, const float* P, int NV, const unsigned char* masks, int H, int W,
                               int* votes, hipStream_t s) {
  hipLaunchKernelGGL(vertex_votes_kernel, dim3(blocks_of(V * NV)), dim3(kMcThreads), 0, s, verts, V, P, NV, masks, H, W, votes);
  return hipGetLastError();
}

hipError_t launch_first_hit(const double* verts, const int* faces, long long V, long long F, const float* kinv, const float* rot,
                            const float* org, const double* proj, const unsigned char* mask, int H, int W,
                            unsigned long long* keys, int* big_count, int* big_list, int* face_id, unsigned char* face_hit,
                            hipStream_t s) {
  const HitCam cam = make_hit_cam(kinv, rot, org, proj);
  const long long n = (long long)H * W;
  hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)n * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(big_count, 0, sizeof(int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(first_hit_small_kernel, dim3(blocks_of(F)), dim3(kMcThreads), 0, s, verts, faces, V, F, cam, mask, H, W, keys,
                     big_count, big_list);
  const unsigned big_blocks = (unsigned)(F < kBigBlocks ? F : kBigBlocks);
  hipLaunchKernelGGL(first_hit_big_kernel, dim3(big_blocks), dim3(kMcThreads), 0, s, verts, faces, V, F, cam, mask, H, W, keys,
                     big_count, big_list);
  hipLaunchKernelGGL(first_hit_resolve_kernel, dim3(blocks_of(n)), dim3(kMcThreads), 0, s, keys, n, F, face_id, face_hit);
  return hipGetLastError();
}

hipError_t launch_edge_keys(const int* faces, const int* vid, long long V, long long F, long long* keys, hipStream_t s) {
  hipLaunchKernelGGL(edge_keys_kernel, dim3(blocks_of(F)), dim3(kMcThreads), 0, s, faces, vid, V, F, keys);
  return hipGetLastError();
}

hipError_t launch_mark_pairs(const long long* keys, const long long* order, long long F, int* pair_a, int* pair_b,
                             unsigned char* has_adj, int* parent, hipStream_t s) {
  hipError_t e = hipMemsetAsync(has_adj, 0, (size_t)F, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mark_pairs_kernel, dim3(blocks_of(3 * F)), dim3(kMcThreads), 0, s, keys, order, 3 * F, F, pair_a, pair_b, has_adj);
  hipLaunchKernelGGL(iota_kernel, dim3(blocks_of(F)), dim3(kMcThreads), 0, s, parent, F);
  return hipGetLastError();
}

hipError_t launch_component_round(const int* pair_a, const int* pair_b, long long F, int* parent, int* changed, hipStream_t s) {
  hipLaunchKernelGGL(hook_kernel, dim3(blocks_of(3 * F)), dim3(kMcThreads), 0, s, pair_a, pair_b, 3 * F, parent, changed);
  hipLaunchKernelGGL(jump_kernel, dim3(blocks_of(F)), dim3(kMcThreads), 0, s, parent, F);
  return hipGetLastError();
}

hipError_t launch_component_labels(const int* parent, const unsigned char* has_adj, long long F, int* labels, hipStream_t s) {
  hipLaunchKernelGGL(labels_kernel, dim3(blocks_of(F)), dim3(kMcThreads), 0, s, parent, has_adj, F, labels);
  return hipGetLastError();
}

}  // namespace ufr
