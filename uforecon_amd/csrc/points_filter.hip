// Point-cloud filtering between depth fusion and scoring (include/ufr.h, "point-cloud filtering"), all positions and distances
// in fp64 with the arithmetic that tests/pcd_ref.py restates:
//
//   knn          the k nearest reference points of every query.  The Morton-sorted reference set is the implicit octree of
//          points_octree.h, walked depth-first with the nearest octant first as chamfer.hip's nn_dist does.  A candidate's key is
//          (d2, caller's index); the k smallest keys are kept as an ascending list by insertion.  A node is dropped only when its
//          box is STRICTLY farther than the k-th d2 so far (max_dist^2 until the list is full): a point at exactly that distance
//          with a lower index may sit in another node.  Every node is visited at most once and the stack holds kNnStack entries
//          (a node that could not push its children is tested point by point), so the walk is finite whatever the data.
//          One wave per block; the lists live in LDS, slot j of lane t at [j][t] (no bank conflicts, no scratch): k x 64 x 12
//          bytes of dynamic LDS.  The walk's stack is per-thread scratch, as in nn_dist.
//   normals      centroid, covariance and the eigenvector of the smallest eigenvalue (eight sweeps of cyclic Jacobi on the
//          symmetric 3x3, everything in named registers), oriented towards the best-seen viewpoint.
//   voxel_mean   runs of equal cell keys -> one mean point each, in key order: run heads ranked by compact.h's block_rank and
//          scan_totals, then the head's thread sums its run left to right.
// No float atomics anywhere: a rerun gives the same bits.  Every output store is guarded by the caller's capacity.
#include "compact.h"
#include "points_octree.h"
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kPfThreads = 256;
constexpr int kKnnThreads = 64;                     // one wave: its lists are k x 64 slots of LDS
constexpr int kKnnLeaf = 16;                        // a node with at most this many points is tested point by point

// ------------------------------------------------------------------ k nearest neighbours
// One query's walk.  ld2 / lidx: this query's list, slot j at [j * stride].  Returns the number of filled slots.
__host__ __device__ inline int knn_query(const double* q, const double* __restrict__ ref, const long long* __restrict__ keys,
                                         const int* __restrict__ ref_index, long long nr, const NnGrid& g, int k, double md2,
                                         int self, double* ld2, int* lidx, int stride) {
  int cnt = 0;
  int slo[kNnStack], shi[kNnStack];
  unsigned char sdep[kNnStack];
  int sp = 0;
  if (nr > 0) { slo[0] = 0; shi[0] = (int)nr; sdep[0] = 0; sp = 1; }
  const int last = (k - 1) * stride;
  while (sp > 0) {
    --sp;
    const long long lo = slo[sp], hi = shi[sp];
    const int dep = sdep[sp];
    const int shift = 3 * (kKeyBits - dep);
    const unsigned long long P = shift >= 63 ? 0ull : (unsigned long long)keys[lo] >> shift;
    const double size = (double)(1ll << (kKeyBits - dep));
    const unsigned long long b[3] = {compact3(P >> 2), compact3(P >> 1), compact3(P)};
    // the node's box, one cell wider on every side than its cells (rounding in the cell index can never put a point outside)
    double box2 = 0.0, mid[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double blo = g.o[a] + ((double)b[a] * size - 1.0) * g.cell;
      const double bhi = g.o[a] + ((double)(b[a] + 1) * size + 1.0) * g.cell;
      mid[a] = g.o[a] + ((double)b[a] + 0.5) * size * g.cell;
      const double d = q[a] < blo ? blo - q[a] : (q[a] > bhi ? q[a] - bhi : 0.0);
      box2 += d * d;
    }
    if (box2 > (cnt == k ? ld2[last] : md2)) continue;            // strictly greater: see the file header
    if (hi - lo <= kKnnLeaf || dep >= kKeyBits || sp + 8 > kNnStack) {
      for (long long j = lo; j < hi; ++j) {
        const double dx = q[0] - ref[3 * j], dy = q[1] - ref[3 * j + 1], dz = q[2] - ref[3 * j + 2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (!(d2 <= md2)) continue;
        const int id = ref_index[j];
        if (id == self) continue;
        if (cnt == k) {
          const double wd = ld2[last];
          if (d2 > wd || (d2 == wd && id >= lidx[last])) continue;
        }
        int s = cnt < k ? cnt : k - 1;                            // the slot that opens; larger keys move one slot down
        while (s > 0) {
          const double pd = ld2[(s - 1) * stride];
          const int pi = lidx[(s - 1) * stride];
          if (pd < d2 || (pd == d2 && pi < id)) break;
          ld2[s * stride] = pd;
          lidx[s * stride] = pi;
          --s;
        }
        ld2[s * stride] = d2;
        lidx[s * stride] = id;
        if (cnt < k) ++cnt;
      }
      continue;
    }
    const int cshift = shift - 3;
    long long cb[9];
    cb[0] = lo;
    cb[8] = hi;
#pragma unroll
    for (int c = 1; c < 8; ++c) cb[c] = lower_bound(keys, cb[c - 1], hi, (long long)((P * 8 + c) << cshift));
    const int qoct = (q[0] >= mid[0] ? 4 : 0) | (q[1] >= mid[1] ? 2 : 0) | (q[2] >= mid[2] ? 1 : 0);
    for (int i = 7; i >= 0; --i) {                 // pushed far to near: the query's own octant is popped first
      const int c = qoct ^ i;
      if (cb[c + 1] > cb[c]) {
        slo[sp] = (int)cb[c];
        shi[sp] = (int)cb[c + 1];
        sdep[sp] = (unsigned char)(dep + 1);
        ++sp;
      }
    }
  }
  return cnt;
}

__global__ void __launch_bounds__(kKnnThreads) knn_kernel(const double* __restrict__ query, long long nq,
                                                           const double* __restrict__ ref, const long long* __restrict__ keys,
                                                           const int* __restrict__ ref_index, long long nr,
                                                           const int* __restrict__ self_index, NnGrid g, int k, double max_dist,
                                                           int* __restrict__ idx, double* __restrict__ dist) {
  extern __shared__ double knn_lds[];                // [k][64] d2, then [k][64] index
  double* ld2 = knn_lds + threadIdx.x;
  int* lidx = reinterpret_cast<int*>(knn_lds + (size_t)k * kKnnThreads) + threadIdx.x;
  const long long qi = (long long)blockIdx.x * kKnnThreads + threadIdx.x;
  if (qi >= nq) return;
  const double q[3] = {query[3 * qi], query[3 * qi + 1], query[3 * qi + 2]};
  int cnt = 0;
  if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))
    cnt = knn_query(q, ref, keys, ref_index, nr, g, k, max_dist * max_dist, self_index ? self_index[qi] : -1, ld2, lidx,
                    kKnnThreads);
  for (int j = 0; j < k; ++j) {
    idx[qi * k + j] = j < cnt ? lidx[j * kKnnThreads] : -1;
    dist[qi * k + j] = j < cnt ? sqrt(ld2[j * kKnnThreads]) : INFINITY;
  }
}

// ------------------------------------------------------------------ normals
// one Jacobi rotation in the (p, q) plane of a symmetric 3x3 (r: the third index); vp / vq: columns p and q of V
__host__ __device__ inline void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double* vp,
                                              double* vq) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double x = vp[i], y = vq[i];
    vp[i] = c * x - s * y;
    vq[i] = s * x + c * y;
  }
}

constexpr int kJacobiSweeps = 8;                    // cyclic Jacobi converges quadratically: a 3x3 is at rounding level after five

// normal, curvature and validity of one point from its neighbour row; false: fewer than three neighbours (or not finite)
__host__ __device__ inline bool point_normal(const double* __restrict__ pts, long long n, const int* __restrict__ row, int k,
                                             const double* __restrict__ views, int V, const double* p, double* nrm,
                                             double* curv) {
  int m = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = 0; j < k; ++j) {
    const long long i = row[j];
    if (i < 0 || i >= n) continue;
    sx += pts[3 * i];
    sy += pts[3 * i + 1];
    sz += pts[3 * i + 2];
    ++m;
  }
  if (m < 3) return false;
  const double dm = (double)m, cx = sx / dm, cy = sy / dm, cz = sz / dm;
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
  for (int j = 0; j < k; ++j) {
    const long long i = row[j];
    if (i < 0 || i >= n) continue;
    const double dx = pts[3 * i] - cx, dy = pts[3 * i + 1] - cy, dz = pts[3 * i + 2] - cz;
    a00 += dx * dx;
    a01 += dx * dy;
    a02 += dx * dz;
    a11 += dy * dy;
    a12 += dy * dz;
    a22 += dz * dz;
  }
  a00 /= dm, a01 /= dm, a02 /= dm, a11 /= dm, a12 /= dm, a22 /= dm;
  double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);
    jacobi_rotate(a00, a22, a02, a01, a12, v0, v2);
    jacobi_rotate(a11, a22, a12, a01, a02, v1, v2);
  }
  double l0 = a00, e[3] = {v0[0], v0[1], v0[2]};
  if (a11 < l0) { l0 = a11; e[0] = v1[0]; e[1] = v1[1]; e[2] = v1[2]; }
  if (a22 < l0) { l0 = a22; e[0] = v2[0]; e[1] = v2[1]; e[2] = v2[2]; }
  const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
  if (!(len > 0.0 && len < INFINITY && fabs(l0) < INFINITY)) return false;      // a NaN fails every comparison
  e[0] /= len, e[1] /= len, e[2] /= len;
  const double tr = (a00 + a11) + a22;
  *curv = tr != 0.0 ? l0 / tr : 0.0;
  bool flip;
  if (V > 0) {          // the viewpoint that sees the surface most squarely decides; ties to the lowest j
    double best = -1.0, bdot = 0.0;
    for (int j = 0; j < V; ++j) {
      const double dx = views[3 * j] - p[0], dy = views[3 * j + 1] - p[1], dz = views[3 * j + 2] - p[2];
      const double dot = (e[0] * dx + e[1] * dy) + e[2] * dz;
      const double c = fabs(dot) / sqrt((dx * dx + dy * dy) + dz * dz);
      if (c > best) { best = c; bdot = dot; }
    }
    flip = bdot < 0.0;
  } else {              // no viewpoint: the component of largest magnitude is made positive; ties to the lowest axis
    int ax = 0;
    if (fabs(e[1]) > fabs(e[ax])) ax = 1;
    const double big = ax == 0 ? e[0] : e[1];
    flip = fabs(e[2]) > fabs(big) ? e[2] < 0.0 : big < 0.0;
  }
  nrm[0] = flip ? -e[0] : e[0];
  nrm[1] = flip ? -e[1] : e[1];
  nrm[2] = flip ? -e[2] : e[2];
  return true;
}

__global__ void __launch_bounds__(kPfThreads) normals_kernel(const double* __restrict__ pts, long long n,
                                                              const int* __restrict__ idx, int k,
                                                              const double* __restrict__ views, int V,
                                                              double* __restrict__ normal, double* __restrict__ curvature,
                                                              unsigned char* __restrict__ valid) {
  const long long i = (long long)blockIdx.x * kPfThreads + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  double nrm[3] = {0.0, 0.0, 0.0}, curv = 0.0;
  const bool ok = point_normal(pts, n, idx + i * k, k, views, V, p, nrm, &curv);
  normal[3 * i] = ok ? nrm[0] : 0.0;
  normal[3 * i + 1] = ok ? nrm[1] : 0.0;
  normal[3 * i + 2] = ok ? nrm[2] : 0.0;
  curvature[i] = ok ? curv : 0.0;
  valid[i] = ok ? 1 : 0;
}

// ------------------------------------------------------------------ voxel mean
__device__ inline bool run_head(const long long* __restrict__ keys, long long n, long long i) {
  return i < n && (i == 0 || keys[i] != keys[i - 1]);
}

__global__ void __launch_bounds__(kPfThreads) voxel_count_kernel(const long long* __restrict__ keys, long long n,
                                                                  long long* __restrict__ block_tot) {
  __shared__ int lds[kPfThreads / 64];
  const long long i = (long long)blockIdx.x * kPfThreads + threadIdx.x;
  int count;
  block_rank<kPfThreads>(run_head(keys, n, i), lds, &count);
  if (threadIdx.x == 0) block_tot[blockIdx.x] = count;
}

__global__ void __launch_bounds__(kPfThreads) voxel_mean_kernel(const double* __restrict__ pts, const long long* __restrict__ keys,
                                                                 long long n, const unsigned char* __restrict__ colors,
                                                                 const double* __restrict__ normals,
                                                                 const long long* __restrict__ block_off,
                                                                 double* __restrict__ out_pts, unsigned char* __restrict__ out_colors,
                                                                 double* __restrict__ out_normals, int* __restrict__ out_count,
                                                                 long long capacity) {
  __shared__ int lds[kPfThreads / 64];
  const long long i = (long long)blockIdx.x * kPfThreads + threadIdx.x;
  const bool head = run_head(keys, n, i);
  int count;
  const int rank = block_rank<kPfThreads>(head, lds, &count);
  if (!head) return;
  const long long o = block_off[blockIdx.x] + rank;
  if (o < 0 || o >= capacity) return;
  const long long key = keys[i];
  long long c = 0, cr = 0, cg = 0, cb = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
  for (long long j = i; j < n && keys[j] == key; ++j, ++c) {      // the run, left to right
    sx += pts[3 * j];
    sy += pts[3 * j + 1];
    sz += pts[3 * j + 2];
    if (colors) { cr += colors[3 * j]; cg += colors[3 * j + 1]; cb += colors[3 * j + 2]; }
    if (normals) { nx += normals[3 * j]; ny += normals[3 * j + 1]; nz += normals[3 * j + 2]; }
  }
  const double dc = (double)c;
  out_pts[3 * o] = sx / dc;
  out_pts[3 * o + 1] = sy / dc;
  out_pts[3 * o + 2] = sz / dc;
  if (colors) {                                                   // the mean rounded half up, in integers
    out_colors[3 * o] = (unsigned char)((2 * cr + c) / (2 * c));
    out_colors[3 * o + 1] = (unsigned char)((2 * cg + c) / (2 * c));
    out_colors[3 * o + 2] = (unsigned char)((2 * cb + c) / (2 * c));
  }
  if (normals) {
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    const bool ok = len > 0.0 && isfinite(len);
    out_normals[3 * o] = ok ? nx / len : 0.0;
    out_normals[3 * o + 1] = ok ? ny / len : 0.0;
    out_normals[3 * o + 2] = ok ? nz / len : 0.0;
  }
  out_count[o] = (int)(c < 2147483647ll ? c : 2147483647ll);
}

}  // namespace

long long points_filter_blocks(long long n) { return (n + kPfThreads - 1) / kPfThreads; }

hipError_t launch_points_knn(const double* query, long long nq, const double* ref, const long long* keys, const int* ref_index,
                             long long nr, const double* origin, double cell, const int* self_index, int k, double max_dist,
                             int* idx, double* dist, hipStream_t s) {
  NnGrid g;
  for (int a = 0; a < 3; ++a) g.o[a] = origin[a];
  g.cell = cell;
  const size_t lds = (size_t)k * kKnnThreads * (sizeof(double) + sizeof(int));
  hipLaunchKernelGGL(knn_kernel, dim3((unsigned)((nq + kKnnThreads - 1) / kKnnThreads)), dim3(kKnnThreads), lds, s, query, nq, ref,
                     keys, ref_index, nr, self_index, g, k, max_dist, idx, dist);
  return hipGetLastError();
}

hipError_t launch_points_normals(const double* pts, long long n, const int* idx, int k, const double* views, int V, double* normal,
                                 double* curvature, unsigned char* valid, hipStream_t s) {
  hipLaunchKernelGGL(normals_kernel, dim3((unsigned)points_filter_blocks(n)), dim3(kPfThreads), 0, s, pts, n, idx, k, views, V, normal,
                     curvature, valid);
  return hipGetLastError();
}

hipError_t launch_voxel_count(const long long* keys, long long n, long long* block_tot, long long* block_off, long long* total,
                              hipStream_t s) {
  hipLaunchKernelGGL(voxel_count_kernel, dim3((unsigned)points_filter_blocks(n)), dim3(kPfThreads), 0, s, keys, n, block_tot);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_scan_totals<1>(block_tot, points_filter_blocks(n), block_off, total, s);
}

hipError_t launch_voxel_mean(const double* pts, const long long* keys, long long n, const unsigned char* colors,
                             const double* normals, const long long* block_off, double* out_pts, unsigned char* out_colors,
                             double* out_normals, int* out_count, long long capacity, hipStream_t s) {
  hipLaunchKernelGGL(voxel_mean_kernel, dim3((unsigned)points_filter_blocks(n)), dim3(kPfThreads), 0, s, pts, keys, n, colors, normals,
                     block_off, out_pts, out_colors, out_normals, out_count, capacity);
  return hipGetLastError();
}

}  // namespace ufr
