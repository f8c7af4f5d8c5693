// DTU chamfer evaluation (the reference's evaluation/dtu_eval.py) on the device, all positions and distances in fp64, with
// the arithmetic that tests/chamfer_ref.py restates (include/ufr.h, ufr_mesh_sample_*, ufr_points_*):
//
//   mesh_sample_count / _scan / _emit   points on every triangle at the given density (dtu_eval.py:68-91): one thread per
//          triangle counts its samples (the count of a row i is found in O(1) from the monotone test a + b < 1, then
//          corrected with that very test), the scans of compact.h give every triangle its offset, and the same thread
//          emits its points in (i, j) order.
//   points_cell_keys   Morton key (21 bits per axis) of the grid cell of every point; the caller sorts by it.
//   thin_round   one round of the thinning fixpoint (dtu_eval.py:105-115): an undecided point looks at the earlier points
//          within r in its 27 cells; removed if one of them is kept, kept if all of them are removed.  A decision reads only
//          decided earlier neighbours and is final, so a state written earlier in the same launch, or a stale "undecided",
//          changes when a point is decided, never how.  One byte per state, plain loads and stores, no flags, no spinning;
//          the host reads the undecided count between rounds.
//   nn_dist      nearest reference point of every query (dtu_eval.py:139-155): the Morton-sorted reference set is an implicit
//          octree (a node = a key prefix = a contiguous range, children found by binary search inside the range); depth-first,
//          nearest octant first, a node is dropped when its box is farther than the best distance so far, which starts at
//          max_dist: a query far from everything leaves after a handful of nodes.  Every node is visited at most once and
//          the stack is bounded by 7 x 21 + 1 entries, so the walk is finite whatever the data.  Block sums of the
//          distances below max_dist, then one summing block: no float atomics, the mean is the same run after run.
// Every output store is guarded by the caller's capacity; point and triangle indices are 64-bit.
#include "compact.h"
#include "points_octree.h"
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kChThreads = 256;

// cell index along one axis, clamped to the key range (clamping never separates neighbours); NaN -> 0
__device__ inline long long cell_of(double p, double o, double cell) {
  const double t = floor((p - o) / cell);
  return t >= 0.0 ? (t < (double)kMaxCell ? (long long)t : kMaxCell) : 0;
}

__global__ void __launch_bounds__(kChThreads) points_cell_keys_kernel(const double* __restrict__ pts, long long n, double ox,
                                                                       double oy, double oz, double cell,
                                                                       long long* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * kChThreads + threadIdx.x;
  if (i >= n) return;
  keys[i] = morton(cell_of(pts[3 * i], ox, cell), cell_of(pts[3 * i + 1], oy, cell), cell_of(pts[3 * i + 2], oz, cell));
}

// ------------------------------------------------------------------ mesh sampling
struct Tri {
  double p0[3], v1[3], v2[3];
  double n1, n2;            // floor(l / thr); samples exist iff both >= 1
};

// dtu_eval.py:70-85 for one triangle, in numpy's order of operations (sums of three left to right).  false: no samples.
__device__ inline bool tri_setup(const double* __restrict__ verts, const int* __restrict__ faces, long long V, long long t,
                                 double density, Tri& s) {
  const long long i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;      // the caller validates; never read outside
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    s.p0[d] = verts[3 * i0 + d];
    s.v1[d] = verts[3 * i1 + d] - s.p0[d];
    s.v2[d] = verts[3 * i2 + d] - s.p0[d];
  }
  const double l1 = sqrt((s.v1[0] * s.v1[0] + s.v1[1] * s.v1[1]) + s.v1[2] * s.v1[2]);
  const double l2 = sqrt((s.v2[0] * s.v2[0] + s.v2[1] * s.v2[1]) + s.v2[2] * s.v2[2]);
  const double cx = s.v1[1] * s.v2[2] - s.v1[2] * s.v2[1];
  const double cy = s.v1[2] * s.v2[0] - s.v1[0] * s.v2[2];
  const double cz = s.v1[0] * s.v2[1] - s.v1[1] * s.v2[0];
  const double area2 = sqrt((cx * cx + cy * cy) + cz * cz);
  if (!(area2 > 0.0)) return false;
  const double thr = density * sqrt(l1 * l2 / area2);
  s.n1 = floor(l1 / thr);
  s.n2 = floor(l2 / thr);
  // n == 0: the reference divides by 1e-7 instead and every a + b is >= 1.  Beyond 2^31 rows (or NaN) nothing is sampled.
  return s.n1 >= 1.0 && s.n2 >= 1.0 && s.n1 < 2147483648.0 && s.n2 < 2147483648.0;
}

// number of j in 0..n2 with a + (j + 0.5) / n2 < 1: the test is monotone in j, so an estimate corrected by the test itself
__device__ inline long long row_count(double a, double n2) {
  const long long m = (long long)n2 + 1;
  double e = floor((1.0 - a) * n2 - 0.5) + 1.0;
  long long c = e > 0.0 ? (e < (double)m ? (long long)e : m) : 0;
  while (c > 0 && !(a + ((double)(c - 1) + 0.5) / n2 < 1.0)) --c;
  while (c < m && a + ((double)c + 0.5) / n2 < 1.0) ++c;
  return c;
}

__global__ void __launch_bounds__(kChThreads) mesh_sample_count_kernel(const double* __restrict__ verts,
                                                                        const int* __restrict__ faces, long long V, long long F,
                                                                        double density, long long* __restrict__ tri_off,
                                                                        long long* __restrict__ block_tot) {
  __shared__ long long lds[kChThreads / 64];
  const long long t = (long long)blockIdx.x * kChThreads + threadIdx.x;
  long long cnt = 0;
  Tri s;
  if (t < F && tri_setup(verts, faces, V, t, density, s)) {
    const long long rows = (long long)s.n1;          // i = 0..n1; row n1 has a > 1: empty
    for (long long i = 0; i <= rows; ++i) cnt += row_count(((double)i + 0.5) / s.n1, s.n2);
  }
  long long tot;
  const long long pre = block_scan_excl<long long, kChThreads>(cnt, lds, &tot);
  if (t < F) tri_off[t] = pre;
  if (threadIdx.x == 0) block_tot[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kChThreads) mesh_sample_emit_kernel(const double* __restrict__ verts,
                                                                       const int* __restrict__ faces, long long V, long long F,
                                                                       double density, const long long* __restrict__ tri_off,
                                                                       const long long* __restrict__ block_off,
                                                                       double* __restrict__ out, long long capacity) {
  const long long t = (long long)blockIdx.x * kChThreads + threadIdx.x;
  Tri s;
  if (t >= F || !tri_setup(verts, faces, V, t, density, s)) return;
  long long o = block_off[blockIdx.x] + tri_off[t];
  const long long rows = (long long)s.n1;
  for (long long i = 0; i <= rows; ++i) {
    const double a = ((double)i + 0.5) / s.n1;
    const long long c = row_count(a, s.n2);
    for (long long j = 0; j < c; ++j, ++o) {
      if (o < 0 || o >= capacity) return;
      const double b = ((double)j + 0.5) / s.n2;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double x = s.v1[d] * a, y = s.v2[d] * b;
        out[3 * o + d] = (x + y) + s.p0[d];
      }
    }
  }
}

// ------------------------------------------------------------------ thinning
constexpr unsigned char kUndecided = 0, kKept = 1, kRemoved = 2;

__global__ void __launch_bounds__(kChThreads) thin_round_kernel(const double* __restrict__ pts, const long long* __restrict__ keys,
                                                                 const int* __restrict__ rank, long long n, double r2,
                                                                 volatile unsigned char* state, int* __restrict__ undecided) {
  __shared__ int lds[kChThreads / 64];
  const long long i = (long long)blockIdx.x * kChThreads + threadIdx.x;
  int und = 0;
  if (i < n && state[i] == kUndecided) {
    const unsigned long long k = (unsigned long long)keys[i];
    const long long cx = (long long)compact3(k >> 2), cy = (long long)compact3(k >> 1), cz = (long long)compact3(k);
    const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    const int me = rank[i];
    bool removed = false, wait = false;
    for (int c = 0; c < 27 && !removed; ++c) {
      const long long nx = cx + c / 9 - 1, ny = cy + (c / 3) % 3 - 1, nz = cz + c % 3 - 1;
      if (nx < 0 || ny < 0 || nz < 0 || nx > kMaxCell || ny > kMaxCell || nz > kMaxCell) continue;
      const long long nk = morton(nx, ny, nz);
      for (long long j = lower_bound(keys, 0, n, nk); j < n && keys[j] == nk; ++j) {
        if (rank[j] >= me) continue;                                // later points and the point itself
        const double dx = pts[3 * j] - px, dy = pts[3 * j + 1] - py, dz = pts[3 * j + 2] - pz;
        if (!((dx * dx + dy * dy) + dz * dz <= r2)) continue;
        const unsigned char st = state[j];
        if (st == kKept) { removed = true; break; }
        if (st == kUndecided) wait = true;
      }
    }
    if (removed) state[i] = kRemoved;
    else if (!wait) state[i] = kKept;
    else und = 1;
  }
  // undecided points of the block -> one integer atomic (integer sums do not depend on the order)
  const unsigned long long ballot = __ballot(und);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = __popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < kChThreads / 64; ++w) tot += lds[w];
    if (tot) atomicAdd(undecided, tot);
  }
}

// ------------------------------------------------------------------ nearest neighbour
constexpr int kNnLeaf = 8;                          // a node with at most this many points is tested point by point

__global__ void __launch_bounds__(kChThreads) nn_dist_kernel(const double* __restrict__ query, long long nq,
                                                              const double* __restrict__ ref, const long long* __restrict__ keys,
                                                              long long nr, NnGrid g, double max_dist, double* __restrict__ dist,
                                                              double* __restrict__ block_sum, long long* __restrict__ block_cnt) {
  __shared__ double lsum[kChThreads];
  __shared__ int lcnt[kChThreads];
  const long long qi = (long long)blockIdx.x * kChThreads + threadIdx.x;
  double res = 0.0;
  int below = 0;
  if (qi < nq) {
    const double q[3] = {query[3 * qi], query[3 * qi + 1], query[3 * qi + 2]};
    const double md2 = max_dist * max_dist;
    double best2 = md2 + md2 * 1e-15;               // every d2 whose square root can round below max_dist
    bool found = false;
    int slo[kNnStack], shi[kNnStack];
    unsigned char sdep[kNnStack];
    int sp = 0;
    const bool finite = isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
    if (finite && nr > 0) { slo[0] = 0; shi[0] = (int)nr; sdep[0] = 0; sp = 1; }
    while (sp > 0) {
      --sp;
      const long long lo = slo[sp], hi = shi[sp];
      const int dep = sdep[sp];
      const int shift = 3 * (kKeyBits - dep);
      const unsigned long long P = shift >= 63 ? 0ull : (unsigned long long)keys[lo] >> shift;
      const double size = (double)(1ll << (kKeyBits - dep));
      const unsigned long long b[3] = {compact3(P >> 2), compact3(P >> 1), compact3(P)};
      // the node's box, one cell wider on every side than its cells (rounding in cell_of can never put a point outside)
      double box2 = 0.0, mid[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double blo = g.o[a] + ((double)b[a] * size - 1.0) * g.cell;
        const double bhi = g.o[a] + ((double)(b[a] + 1) * size + 1.0) * g.cell;
        mid[a] = g.o[a] + ((double)b[a] + 0.5) * size * g.cell;
        const double d = q[a] < blo ? blo - q[a] : (q[a] > bhi ? q[a] - bhi : 0.0);
        box2 += d * d;
      }
      if (box2 > best2) continue;
      if (hi - lo <= kNnLeaf || dep >= kKeyBits || sp + 8 > kNnStack) {
        for (long long j = lo; j < hi; ++j) {
          const double dx = q[0] - ref[3 * j], dy = q[1] - ref[3 * j + 1], dz = q[2] - ref[3 * j + 2];
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          if (d2 < best2) { best2 = d2; found = true; }
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
    res = found ? sqrt(best2) : INFINITY;
    dist[qi] = res;
    below = res < max_dist;
  }
  lsum[threadIdx.x] = below ? res : 0.0;
  lcnt[threadIdx.x] = below;
  __syncthreads();
  for (int d = kChThreads / 2; d > 0; d >>= 1) {
    if (threadIdx.x < (unsigned)d) {
      lsum[threadIdx.x] += lsum[threadIdx.x + d];
      lcnt[threadIdx.x] += lcnt[threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    block_sum[blockIdx.x] = lsum[0];
    block_cnt[blockIdx.x] = lcnt[0];
  }
}

// one block: mean_out[0] = sum of the block sums, mean_out[1] = the count, in a fixed order
__global__ void __launch_bounds__(kScanThreads) nn_sum_kernel(const double* __restrict__ block_sum,
                                                               const long long* __restrict__ block_cnt, long long n_blocks,
                                                               double* __restrict__ mean_out) {
  __shared__ double ss[kScanThreads];
  __shared__ long long sc[kScanThreads];
  const long long per = (n_blocks + kScanThreads - 1) / kScanThreads;
  const long long t0 = min((long long)threadIdx.x * per, n_blocks), t1 = min(t0 + per, n_blocks);
  double s = 0.0;
  long long c = 0;
  for (long long t = t0; t < t1; ++t) { s += block_sum[t]; c += block_cnt[t]; }
  ss[threadIdx.x] = s;
  sc[threadIdx.x] = c;
  __syncthreads();
  for (int d = kScanThreads / 2; d > 0; d >>= 1) {
    if (threadIdx.x < (unsigned)d) {
      ss[threadIdx.x] += ss[threadIdx.x + d];
      sc[threadIdx.x] += sc[threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mean_out[0] = ss[0];
    mean_out[1] = (double)sc[0];
  }
}

}  // namespace

long long chamfer_blocks(long long n) { return (n + kChThreads - 1) / kChThreads; }

hipError_t launch_points_cell_keys(const double* pts, long long n, const double* origin, double cell, long long* keys,
                                   hipStream_t s) {
  hipLaunchKernelGGL(points_cell_keys_kernel, dim3((unsigned)chamfer_blocks(n)), dim3(kChThreads), 0, s, pts, n, origin[0], origin[1], origin[2],
                     cell, keys);
  return hipGetLastError();
}

hipError_t launch_mesh_sample_count(const double* verts, const int* faces, long long V, long long F, double density,
                                    long long* tri_off, long long* block_tot, hipStream_t s) {
  hipLaunchKernelGGL(mesh_sample_count_kernel, dim3((unsigned)chamfer_blocks(F)), dim3(kChThreads), 0, s, verts, faces, V, F, density, tri_off,
                     block_tot);
  return hipGetLastError();
}

hipError_t launch_mesh_sample_scan(const long long* block_tot, long long n_blocks, long long* block_off, long long* total,
                                   hipStream_t s) {
  return launch_scan_totals<1>(block_tot, n_blocks, block_off, total, s);
}

hipError_t launch_mesh_sample_emit(const double* verts, const int* faces, long long V, long long F, double density,
                                   const long long* tri_off, const long long* block_off, double* out, long long capacity,
                                   hipStream_t s) {
  hipLaunchKernelGGL(mesh_sample_emit_kernel, dim3((unsigned)chamfer_blocks(F)), dim3(kChThreads), 0, s, verts, faces, V, F, density, tri_off,
                     block_off, out, capacity);
  return hipGetLastError();
}

hipError_t launch_thin_round(const double* pts, const long long* keys, const int* rank, long long n, double radius,
                             unsigned char* state, int* undecided, hipStream_t s) {
  hipLaunchKernelGGL(thin_round_kernel, dim3((unsigned)chamfer_blocks(n)), dim3(kChThreads), 0, s, pts, keys, rank, n, radius * radius, state,
                     undecided);
  return hipGetLastError();
}

hipError_t launch_nn_dist(const double* query, long long nq, const double* ref, const long long* keys, long long nr,
                          const double* origin, double cell, double max_dist, double* dist, double* block_sum,
                          long long* block_cnt, double* mean_out, hipStream_t s) {
  NnGrid g;
  for (int a = 0; a < 3; ++a) g.o[a] = origin[a];
  g.cell = cell;
  hipLaunchKernelGGL(nn_dist_kernel, dim3((unsigned)chamfer_blocks(nq)), dim3(kChThreads), 0, s, query, nq, ref, keys, nr, g, max_dist, dist,
                     block_sum, block_cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !mean_out) return e;
  hipLaunchKernelGGL(nn_sum_kernel, dim3(1), dim3(kScanThreads), 0, s, block_sum, block_cnt, chamfer_blocks(nq), mean_out);
  return hipGetLastError();
}

}  // namespace ufr
