// Mesh simplification by vertex clustering with quadric placement (include/ufr.h, "mesh simplification"), every value fp64,
// every product and sum rounded on its own, with the arithmetic that tests/simplify_ref.py restates:
//
//   clusters          runs of equal cell keys -> the cluster number of every input vertex and the key of every cluster: run
//          heads ranked by compact.h's block_rank and scan_totals, as points_filter.hip's voxel_mean ranks them.
//   face_keys         up to three (cluster << 32 | face) rows per face, kSimplifyNone in the unused slots.  The caller sorts
//          them, so that a cluster's faces stand in ascending face index.
//   quadrics          one thread per sorted row; the head of a run of equal cluster sums the ten terms of its faces left to
//          right and stores them: poisson.hip's splat_sum, no float atomic.  The terms are recomputed from the face, nothing
//          but keys is sorted.  A run may be longer than a block (a coarse cell): its head's loop is then long, not wrong.
//          One wave per cluster with a shuffle tree is faster and sums in another order than the rule states: not taken
//          (profiles/mesh_simplify_launch_shapes.md).
//   place             the regularised quadric's minimiser by cofactors, tested and taken or not, one thread per cluster.
//   face_triples      corners -> cluster numbers, collapsed faces marked, the rest rotated to smallest-first; sort keys.
//   face_heads        after the caller's two stable sorts: the first row of every run of equal triples survives.
//   compact_faces     the survivors in ascending input index (count / scan / emit), and the clusters they name.
//   compact_vertices  the named clusters renumbered in key order (count / scan / emit), the faces rewritten, the vertex map.
// Integer flags and scans only; every store is a plain store guarded by the array's size.  Grids are functions of the sizes.
#include "compact.h"
#include "points_octree.h"
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kSt = kSimplifyThreads;
constexpr long long kSimplifyNone = 0x7fffffffffffffffll;   // a row no cluster takes; sorts last

unsigned blocks_of(long long n) { return (unsigned)((n + kSt - 1) / kSt); }

// ------------------------------------------------------------------ clusters
__device__ inline bool run_head(const long long* __restrict__ keys, long long n, long long i) {
  return i < n && (i == 0 || keys[i] != keys[i - 1]);
}

__global__ void __launch_bounds__(kSt) head_count_kernel(const long long* __restrict__ keys, long long n,
                                                          long long* __restrict__ block_tot) {
  __shared__ int lds[kSt / 64];
  const long long i = (long long)blockIdx.x * kSt + threadIdx.x;
  int count;
  block_rank<kSt>(run_head(keys, n, i), lds, &count);
  if (threadIdx.x == 0) block_tot[blockIdx.x] = count;
}

__global__ void __launch_bounds__(kSt) clusters_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                        long long n, const long long* __restrict__ block_off,
                                                        int* __restrict__ cluster, long long* __restrict__ cluster_key,
                                                        long long capacity) {
  __shared__ int lds[kSt / 64];
  const long long i = (long long)blockIdx.x * kSt + threadIdx.x;
  const bool head = run_head(keys, n, i);
  int count;
  const int rank = block_rank<kSt>(head, lds, &count);
  if (i >= n) return;
  const long long c = block_off[blockIdx.x] + rank + (head ? 0 : -1);   // heads before this row, this row's own included, - 1
  const long long v = order[i];
  if (v >= 0 && v < n) cluster[v] = (int)c;
  if (head && c >= 0 && c < capacity) cluster_key[c] = keys[i];
}

// ------------------------------------------------------------------ face rows
// the clusters of a face's corners; false: a corner outside 0 .. V-1
__device__ inline bool face_clusters(const int* __restrict__ faces, const int* __restrict__ cluster, long long V, long long f,
                                     int* c) {
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int v = faces[3 * f + e];
    if (v < 0 || v >= V) return false;
    c[e] = cluster[v];
  }
  return c[0] >= 0 && c[1] >= 0 && c[2] >= 0;
}

__global__ void __launch_bounds__(kSt) face_keys_kernel(const int* __restrict__ faces, const int* __restrict__ cluster, long long V,
                                                         long long F, long long* __restrict__ keys) {
  const long long f = (long long)blockIdx.x * kSt + threadIdx.x;
  if (f >= F) return;
  int c[3];
  const bool ok = face_clusters(faces, cluster, V, f, c);
  keys[3 * f] = ok ? ((long long)c[0] << 32 | f) : kSimplifyNone;
  keys[3 * f + 1] = ok && c[1] != c[0] ? ((long long)c[1] << 32 | f) : kSimplifyNone;
  keys[3 * f + 2] = ok && c[2] != c[0] && c[2] != c[1] ? ((long long)c[2] << 32 | f) : kSimplifyNone;
}

struct SimplifyGrid { double o[3]; double h; };

// the centre of the cell a cluster's key names
__device__ inline void cell_centre(long long key, const SimplifyGrid& g, double* m) {
  const unsigned long long k = (unsigned long long)key;
  m[0] = g.o[0] + ((double)compact3(k >> 2) + 0.5) * g.h;
  m[1] = g.o[1] + ((double)compact3(k >> 1) + 0.5) * g.h;
  m[2] = g.o[2] + ((double)compact3(k) + 0.5) * g.h;
}

__global__ void __launch_bounds__(kSt) quadrics_kernel(const double* __restrict__ verts, const int* __restrict__ faces,
                                                        const long long* __restrict__ cluster_key, long long V, long long F,
                                                        long long C, SimplifyGrid g, const long long* __restrict__ keys,
                                                        double* __restrict__ quadrics, int* __restrict__ n_faces) {
  const long long rows = 3 * F;
  const long long i = (long long)blockIdx.x * kSt + threadIdx.x;
  if (i >= rows) return;
  const long long cl = keys[i] >> 32;
  if (i > 0 && (keys[i - 1] >> 32) == cl) return;     // not the head of its run
  if (cl < 0 || cl >= C) return;                      // kSimplifyNone
  double m[3];
  cell_centre(cluster_key[cl], g, m);
  double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, q4 = 0.0, q5 = 0.0, q6 = 0.0, q7 = 0.0, q8 = 0.0, q9 = 0.0;
  int cnt = 0;
  for (long long j = i; j < rows && (keys[j] >> 32) == cl; ++j) {      // the run, left to right: ascending face index
    const long long f = keys[j] & 0xffffffffll;
    if (f >= F) continue;
    const long long a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) continue;
    const double ax = verts[3 * a], ay = verts[3 * a + 1], az = verts[3 * a + 2];
    const double u0 = verts[3 * b] - ax, u1 = verts[3 * b + 1] - ay, u2 = verts[3 * b + 2] - az;
    const double v0 = verts[3 * c] - ax, v1 = verts[3 * c + 1] - ay, v2 = verts[3 * c + 2] - az;
    const double n0 = u1 * v2 - u2 * v1, n1 = u2 * v0 - u0 * v2, n2 = u0 * v1 - u1 * v0;
    const double r0 = ax - m[0], r1 = ay - m[1], r2 = az - m[2];
    const double d = -((n0 * r0 + n1 * r1) + n2 * r2);
    q0 += n0 * n0;
    q1 += n0 * n1;
    q2 += n0 * n2;
    q3 += n1 * n1;
    q4 += n1 * n2;
    q5 += n2 * n2;
    q6 += n0 * d;
    q7 += n1 * d;
    q8 += n2 * d;
    q9 += d * d;
    ++cnt;
  }
  double* q = quadrics + 10 * cl;
  q[0] = q0, q[1] = q1, q[2] = q2, q[3] = q3, q[4] = q4, q[5] = q5, q[6] = q6, q[7] = q7, q[8] = q8, q[9] = q9;
  n_faces[cl] = cnt;
}

// ------------------------------------------------------------------ placement
// E'(y) of include/ufr.h; A: A'00 A01 A02 A'11 A12 A'22
__device__ inline double quadric_error(const double* A, const double* b, double c, double y0, double y1, double y2) {
  const double g0 = (A[0] * y0 + A[1] * y1) + A[2] * y2;
  const double g1 = (A[1] * y0 + A[3] * y1) + A[4] * y2;
  const double g2 = (A[2] * y0 + A[4] * y1) + A[5] * y2;
  const double quad = (y0 * g0 + y1 * g1) + y2 * g2;
  const double lin = (b[0] * y0 + b[1] * y1) + b[2] * y2;
  return (quad + 2.0 * lin) + c;
}

__global__ void __launch_bounds__(kSt) place_kernel(const double* __restrict__ quadrics, const int* __restrict__ n_faces,
                                                     const double* __restrict__ mean, const long long* __restrict__ cluster_key,
                                                     long long C, SimplifyGrid g, int placement, double* __restrict__ position,
                                                     unsigned char* __restrict__ placed) {
  const long long i = (long long)blockIdx.x * kSt + threadIdx.x;
  if (i >= C) return;
  const double xm0 = mean[3 * i], xm1 = mean[3 * i + 1], xm2 = mean[3 * i + 2];
  double p0 = xm0, p1 = xm1, p2 = xm2;
  bool take = false;
  if (placement == UFR_SIMPLIFY_QUADRIC && n_faces[i] > 0) {
    double m[3];
    cell_centre(cluster_key[i], g, m);
    const double* q = quadrics + 10 * i;
    const double xb0 = xm0 - m[0], xb1 = xm1 - m[1], xb2 = xm2 - m[2];
    const double w = 0.0009765625 * ((q[0] + q[3]) + q[5]);
    const double A[6] = {q[0] + w, q[1], q[2], q[3] + w, q[4], q[5] + w};
    const double b[3] = {q[6] - w * xb0, q[7] - w * xb1, q[8] - w * xb2};
    const double c = q[9] + w * ((xb0 * xb0 + xb1 * xb1) + xb2 * xb2);
    const double C00 = A[3] * A[5] - A[4] * A[4];
    const double C01 = A[2] * A[4] - A[1] * A[5];
    const double C02 = A[1] * A[4] - A[2] * A[3];
    const double C11 = A[0] * A[5] - A[2] * A[2];
    const double C12 = A[1] * A[2] - A[0] * A[4];
    const double C22 = A[0] * A[3] - A[1] * A[1];
    const double det = (A[0] * C00 + A[1] * C01) + A[2] * C02;
    const double r0 = -b[0], r1 = -b[1], r2 = -b[2];
    const double x0 = ((C00 * r0 + C01 * r1) + C02 * r2) / det;
    const double x1 = ((C01 * r0 + C11 * r1) + C12 * r2) / det;
    const double x2 = ((C02 * r0 + C12 * r1) + C22 * r2) / det;
    const double half = 0.5 * g.h;
    if (isfinite(x0) && isfinite(x1) && isfinite(x2) && fabs(x0) <= half && fabs(x1) <= half && fabs(x2) <= half &&
        quadric_error(A, b, c, x0, x1, x2) <= quadric_error(A, b, c, xb0, xb1, xb2)) {
      take = true;
      p0 = m[0] + x0;
      p1 = m[1] + x1;
      p2 = m[2] + x2;
    }
  }
  position[3 * i] = p0;
  position[3 * i + 1] = p1;
  position[3 * i + 2] = p2;
  placed[i] = take ? 1 : 0;
}

// ------------------------------------------------------------------ faces
__global__ void __launch_bounds__(kSt) face_triples_kernel(const int* __restrict__ faces, const int* __restrict__ cluster,
                                                            long long V, long long F, int* __restrict__ triples,
                                                            long long* __restrict__ key_a, long long* __restrict__ key_bc) {
  const long long f = (long long)blockIdx.x * kSt + threadIdx.x;
  if (f >= F) return;
  int c[3];
  const bool ok = face_clusters(faces, cluster, V, f, c) && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
  int a = -1, b = -1, d = -1;
  if (ok) {
    if (c[0] < c[1] && c[0] < c[2]) { a = c[0]; b = c[1]; d = c[2]; }
    else if (c[1] < c[0] && c[1] < c[2]) { a = c[1]; b = c[2]; d = c[0]; }
    else { a = c[2]; b = c[0]; d = c[1]; }
  }
  triples[3 * f] = a;
  triples[3 * f + 1] = b;
  triples[3 * f + 2] = d;
  key_a[f] = ok ? (long long)a : kSimplifyNone;
  key_bc[f] = ok ? ((long long)b << 32 | (long long)d) : kSimplifyNone;
}

__global__ void __launch_bounds__(kSt) face_heads_kernel(const long long* __restrict__ key_a, const long long* __restrict__ key_bc,
                                                          const long long* __restrict__ order, long long F,
                                                          unsigned char* __restrict__ keep) {
  const long long i = (long long)blockIdx.x * kSt + threadIdx.x;
  if (i >= F) return;
  const long long f = order[i];
  if (f < 0 || f >= F) return;
  const long long a = key_a[f], bc = key_bc[f];
  bool head = a != kSimplifyNone;
  if (head && i > 0) {
    const long long p = order[i - 1];
    if (p >= 0 && p < F && key_a[p] == a && key_bc[p] == bc) head = false;
  }
  keep[f] = head ? 1 : 0;
}

__global__ void __launch_bounds__(kSt) flag_count_kernel(const unsigned char* __restrict__ flag, long long n,
                                                          long long* __restrict__ block_tot) {
  __shared__ int lds[kSt / 64];
  const long long i = (long long)blockIdx.x * kSt + threadIdx.x;
  int count;
  block_rank<kSt>(i < n && flag[i] != 0, lds, &count);
  if (threadIdx.x == 0) block_tot[blockIdx.x] = count;
}

__global__ void __launch_bounds__(kSt) face_emit_kernel(const int* __restrict__ triples, const unsigned char* __restrict__ keep,
                                                         long long F, long long C, const long long* __restrict__ block_off,
                                                         int* __restrict__ out_faces, int* __restrict__ face_map,
                                                         long long capacity, unsigned char* __restrict__ referenced) {
  __shared__ int lds[kSt / 64];
  const long long f = (long long)blockIdx.x * kSt + threadIdx.x;
  const bool kept = f < F && keep[f] != 0;
  int count;
  const int rank = block_rank<kSt>(kept, lds, &count);
  if (!kept) return;
  const long long o = block_off[blockIdx.x] + rank;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int c = triples[3 * f + e];
    if (o >= 0 && o < capacity) out_faces[3 * o + e] = c;
    if (c >= 0 && c < C) referenced[c] = 1;           // every writer stores the same byte
  }
  if (o >= 0 && o < capacity) face_map[o] = (int)f;
}

// ------------------------------------------------------------------ vertices
__global__ void __launch_bounds__(kSt) vertex_emit_kernel(const unsigned char* __restrict__ referenced, long long C,
                                                           const long long* __restrict__ block_off,
                                                           const double* __restrict__ position,
                                                           const unsigned char* __restrict__ colors,
                                                           const unsigned char* __restrict__ placed, const int* __restrict__ count,
                                                           double* __restrict__ out_verts, unsigned char* __restrict__ out_colors,
                                                           unsigned char* __restrict__ out_placed, int* __restrict__ out_count,
                                                           long long capacity, int* __restrict__ cluster_vertex) {
  __shared__ int lds[kSt / 64];
  const long long i = (long long)blockIdx.x * kSt + threadIdx.x;
  const bool ref = i < C && referenced[i] != 0;
  int total;
  const int rank = block_rank<kSt>(ref, lds, &total);
  if (i >= C) return;
  const long long o = block_off[blockIdx.x] + rank;
  const bool fits = ref && o >= 0 && o < capacity;
  cluster_vertex[i] = fits ? (int)o : -1;
  if (!fits) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out_verts[3 * o + a] = position[3 * i + a];
    if (colors) out_colors[3 * o + a] = colors[3 * i + a];
  }
  out_placed[o] = placed[i];
  out_count[o] = count[i];
}

// faces from cluster numbers to output vertices (rows 0 .. 3 n_faces - 1), then the vertex map (rows 3 n_faces ..)
__global__ void __launch_bounds__(kSt) renumber_kernel(const int* __restrict__ cluster_vertex, long long C,
                                                        int* __restrict__ faces, long long n_faces,
                                                        const int* __restrict__ cluster, long long V,
                                                        int* __restrict__ vertex_map) {
  const long long i = (long long)blockIdx.x * kSt + threadIdx.x;
  const long long rows = 3 * n_faces;
  if (i < rows) {
    const int c = faces[i];
    faces[i] = c >= 0 && c < C ? cluster_vertex[c] : -1;
  } else if (i - rows < V) {
    const int c = cluster[i - rows];
    vertex_map[i - rows] = c >= 0 && c < C ? cluster_vertex[c] : -1;
  }
}

SimplifyGrid make_grid(const double* origin, double cell) {
  SimplifyGrid g;
  for (int a = 0; a < 3; ++a) g.o[a] = origin[a];
  g.h = cell;
  return g;
}

}  // namespace

long long simplify_blocks(long long n) { return (n + kSt - 1) / kSt; }

hipError_t launch_simplify_clusters(const long long* keys, const long long* order, long long V, int* cluster,
                                    long long* cluster_key, long long capacity, long long* block_tot, long long* block_off,
                                    long long* total, hipStream_t s) {
  hipLaunchKernelGGL(head_count_kernel, dim3(blocks_of(V)), dim3(kSt), 0, s, keys, V, block_tot);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_scan_totals<1>(block_tot, simplify_blocks(V), block_off, total, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(clusters_kernel, dim3(blocks_of(V)), dim3(kSt), 0, s, keys, order, V, block_off, cluster, cluster_key, capacity);
  return hipGetLastError();
}

hipError_t launch_simplify_face_keys(const int* faces, const int* cluster, long long V, long long F, long long* keys, hipStream_t s) {
  hipLaunchKernelGGL(face_keys_kernel, dim3(blocks_of(F)), dim3(kSt), 0, s, faces, cluster, V, F, keys);
  return hipGetLastError();
}

hipError_t launch_simplify_quadrics(const double* verts, const int* faces, const long long* cluster_key, long long V, long long F,
                                    long long C, const double* origin, double cell, const long long* sorted_keys,
                                    double* quadrics, int* n_faces, hipStream_t s) {
  hipError_t e = hipMemsetAsync(quadrics, 0, (size_t)C * 10 * sizeof(double), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(n_faces, 0, (size_t)C * sizeof(int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(quadrics_kernel, dim3(blocks_of(3 * F)), dim3(kSt), 0, s, verts, faces, cluster_key, V, F, C,
                     make_grid(origin, cell), sorted_keys, quadrics, n_faces);
  return hipGetLastError();
}

hipError_t launch_simplify_place(const double* quadrics, const int* n_faces, const double* mean, const long long* cluster_key,
                                 long long C, const double* origin, double cell, int placement, double* position,
                                 unsigned char* placed, hipStream_t s) {
  hipLaunchKernelGGL(place_kernel, dim3(blocks_of(C)), dim3(kSt), 0, s, quadrics, n_faces, mean, cluster_key, C,
                     make_grid(origin, cell), placement, position, placed);
  return hipGetLastError();
}

hipError_t launch_simplify_face_triples(const int* faces, const int* cluster, long long V, long long F, int* triples,
                                        long long* key_a, long long* key_bc, hipStream_t s) {
  hipLaunchKernelGGL(face_triples_kernel, dim3(blocks_of(F)), dim3(kSt), 0, s, faces, cluster, V, F, triples, key_a, key_bc);
  return hipGetLastError();
}

hipError_t launch_simplify_face_heads(const long long* key_a, const long long* key_bc, const long long* order, long long F,
                                      unsigned char* keep, hipStream_t s) {
  hipError_t e = hipMemsetAsync(keep, 0, (size_t)F, s);           // an order that is no permutation leaves zeros, not garbage
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(face_heads_kernel, dim3(blocks_of(F)), dim3(kSt), 0, s, key_a, key_bc, order, F, keep);
  return hipGetLastError();
}

hipError_t launch_simplify_compact_faces(const int* triples, const unsigned char* keep, long long F, long long C, int* out_faces,
                                         int* face_map, long long capacity, unsigned char* referenced, long long* block_tot,
                                         long long* block_off, long long* total, hipStream_t s) {
  hipError_t e = hipMemsetAsync(referenced, 0, (size_t)C, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flag_count_kernel, dim3(blocks_of(F)), dim3(kSt), 0, s, keep, F, block_tot);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_scan_totals<1>(block_tot, simplify_blocks(F), block_off, total, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(face_emit_kernel, dim3(blocks_of(F)), dim3(kSt), 0, s, triples, keep, F, C, block_off, out_faces, face_map,
                     capacity, referenced);
  return hipGetLastError();
}

hipError_t launch_simplify_compact_vertices(const unsigned char* referenced, long long C, const double* position,
                                            const unsigned char* colors, const unsigned char* placed, const int* count,
                                            const int* cluster, long long V, int* faces, long long n_faces, double* out_verts,
                                            unsigned char* out_colors, unsigned char* out_placed, int* out_count,
                                            long long capacity, int* cluster_vertex, int* vertex_map, long long* block_tot,
                                            long long* block_off, long long* total, hipStream_t s) {
  hipLaunchKernelGGL(flag_count_kernel, dim3(blocks_of(C)), dim3(kSt), 0, s, referenced, C, block_tot);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_scan_totals<1>(block_tot, simplify_blocks(C), block_off, total, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vertex_emit_kernel, dim3(blocks_of(C)), dim3(kSt), 0, s, referenced, C, block_off, position, colors, placed,
                     count, out_verts, out_colors, out_placed, out_count, capacity, cluster_vertex);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(renumber_kernel, dim3(blocks_of(3 * n_faces + V)), dim3(kSt), 0, s, cluster_vertex, C, faces, n_faces, cluster,
                     V, vertex_map);
  return hipGetLastError();
}

}  // namespace ufr
