// Uniform-grid Poisson surface reconstruction (include/ufr.h, "Poisson surface reconstruction"), every value fp64, every
// product and sum rounded on its own, with the arithmetic that tests/poisson_ref.py restates:
//
//   splat_keys   8 rows per sample: the linear index of every node of the sample's cell (row 8 p + c, c = 4 a + 2 b + g for
//          the corner (a, b, g)).  The caller sorts the rows by key with a STABLE sort, so that the rows of a node stand in
//          ascending sample index.
//   splat_sum    one thread per sorted row; the head of a run of equal keys sums the run left to right (w n into V, w into W)
//          and stores the node.  The weights are recomputed from the sample, nothing but keys and row numbers is sorted.
//          The store-and-sum form of ufr_points_voxel_mean: no float atomic, a rerun gives the same bits.
//   divergence   b = div V by central differences, one thread per node, V = 0 outside.
//   laplace      q = A p, A = the negated 7-point Laplacian over h^2 with 0 outside the grid.  A block owns tiles of
//          kPsTileX x kPsTileY x kPsTileZ nodes: a wave is one z-row of 64 doubles (512 contiguous bytes), the block's four
//          waves are four neighbouring rows, and the block marches kPsTileX planes along x with p[i-1], p[i], p[i+1] in
//          registers; the y and z neighbours are the block's own rows (L1 hits) except at the tile's rim.  With kDot the
//          thread keeps p q and the block stores one partial sum.
//   cg_*         conjugate gradients on A x = -b.  The scalars never leave the device: a dot product is at most
//          kPsMaxBlocks per-block partials (shuffle tree over the wave, the four waves added in wave order), and EVERY block
//          of the next kernel adds the partials up again in the same fixed order, so that all blocks hold the same bits
//          (8 KiB of L2 reads per block instead of a finishing launch).  r.r of the current iteration lives in state[slot],
//          written by block 0 of cg_direction into the slot nobody reads during that kernel.
//          alpha = r.r / p.q and beta = r'.r' / r.r are 0 when their denominator is 0: a residual that reaches exactly 0
//          between two looks of the host stays 0 instead of becoming 0 / 0.
//   sample       the trilinear value of a volume at points, and their mean through the same partial sums.
// Grids are functions of the sizes alone.  Every store is guarded by the volume's or the array's size.
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kPsThreads = 256;
constexpr int kPsWaves = kPsThreads / 64;

struct PsGrid { double o[3]; double h; int d[3]; };

// all threads of the block get the sum of v over the block: lane l += lane l + off (off = 32 .. 1), then the waves in order
__device__ inline double block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = lds[0];
#pragma unroll
  for (int w = 1; w < kPsWaves; ++w) t += lds[w];
  __syncthreads();                                   // lds may be written again
  return t;
}

// the sum of n_part partials, the same bits in every block: thread t adds part[t], part[t + 256], ..., then block_sum
__device__ inline double partials_sum(const double* __restrict__ part, int n_part, double* lds) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n_part; i += kPsThreads) s += part[i];
  return block_sum(s, lds);
}

// a point's cell and offsets: u = (p - o) / h clamped to [0, d - 1]; cell = min(floor(u), d - 2); t = u - cell in [0, 1]
__device__ inline bool cell_of(const double* __restrict__ pts, long long p, const PsGrid& g, int* c, double* t) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double x = pts[3 * p + a];
    if (!isfinite(x)) return false;
    double u = (x - g.o[a]) / g.h;
    const double top = (double)(g.d[a] - 1);
    u = u < 0.0 ? 0.0 : (u > top ? top : u);
    int ci = (int)floor(u);
    if (ci > g.d[a] - 2) ci = g.d[a] - 2;
    c[a] = ci;
    t[a] = u - (double)ci;
  }
  return true;
}

__device__ inline double corner_weight(const double* t, int corner) {
  const double wx = (corner & 4) ? t[0] : 1.0 - t[0];
  const double wy = (corner & 2) ? t[1] : 1.0 - t[1];
  const double wz = (corner & 1) ? t[2] : 1.0 - t[2];
  return (wx * wy) * wz;
}

__device__ inline long long node_of(const int* c, int corner, const PsGrid& g) {
  const long long i = c[0] + ((corner >> 2) & 1), j = c[1] + ((corner >> 1) & 1), k = c[2] + (corner & 1);
  return (i * g.d[1] + j) * g.d[2] + k;
}

// ------------------------------------------------------------------ splat
__global__ void __launch_bounds__(kPsThreads) splat_keys_kernel(const double* __restrict__ pts, long long n, PsGrid g,
                                                                 long long* __restrict__ keys) {
  const long long p = (long long)blockIdx.x * kPsThreads + threadIdx.x;
  if (p >= n) return;
  int c[3];
  double t[3];
  const bool ok = cell_of(pts, p, g, c, t);
#pragma unroll
  for (int corner = 0; corner < 8; ++corner) keys[8 * p + corner] = ok ? node_of(c, corner, g) : -1;   // -1: a row no node takes
}

__global__ void __launch_bounds__(kPsThreads) splat_sum_kernel(const double* __restrict__ pts, const double* __restrict__ nrm,
                                                                long long n, PsGrid g, const long long* __restrict__ keys,
                                                                const long long* __restrict__ rows, double* __restrict__ V,
                                                                double* __restrict__ W) {
  const long long m = 8 * n;
  const long long i = (long long)blockIdx.x * kPsThreads + threadIdx.x;
  if (i >= m) return;
  const long long key = keys[i];
  if (i > 0 && keys[i - 1] == key) return;           // not the head of its run
  const long long nn = (long long)g.d[0] * g.d[1] * g.d[2];
  if (key < 0 || key >= nn) return;
  double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
  for (long long j = i; j < m && keys[j] == key; ++j) {          // the run, left to right: ascending sample index
    const long long row = rows[j];
    if (row < 0 || row >= m) continue;
    const long long p = row >> 3;
    int c[3];
    double t[3];
    if (!cell_of(pts, p, g, c, t)) continue;
    const double w = corner_weight(t, (int)(row & 7));
    sx += w * nrm[3 * p];
    sy += w * nrm[3 * p + 1];
    sz += w * nrm[3 * p + 2];
    sw += w;
  }
  V[key] = sx;
  V[nn + key] = sy;
  V[2 * nn + key] = sz;
  W[key] = sw;
}

// ------------------------------------------------------------------ divergence
__global__ void __launch_bounds__(kPsThreads) divergence_kernel(const double* __restrict__ V, int X, int Y, int Z, double two_h,
                                                                 double* __restrict__ b) {
  const long long nn = (long long)X * Y * Z;
  const long long idx = (long long)blockIdx.x * kPsThreads + threadIdx.x;
  if (idx >= nn) return;
  const int k = (int)(idx % Z), j = (int)((idx / Z) % Y), i = (int)(idx / ((long long)Y * Z));
  const long long sx = (long long)Y * Z;
  const double* Vx = V;
  const double* Vy = V + nn;
  const double* Vz = V + 2 * nn;
  const double dx = (i + 1 < X ? Vx[idx + sx] : 0.0) - (i > 0 ? Vx[idx - sx] : 0.0);
  const double dy = (j + 1 < Y ? Vy[idx + Z] : 0.0) - (j > 0 ? Vy[idx - Z] : 0.0);
  const double dz = (k + 1 < Z ? Vz[idx + 1] : 0.0) - (k > 0 ? Vz[idx - 1] : 0.0);
  b[idx] = ((dx + dy) + dz) / two_h;
}

// ------------------------------------------------------------------ q = A p
template <bool kDot>
__global__ void __launch_bounds__(kPsThreads) laplace_kernel(const double* __restrict__ p, double* __restrict__ q, int X, int Y,
                                                              int Z, double h2, int ty_n, int tz_n, long long tiles,
                                                              double* __restrict__ part) {
  __shared__ double lds[kPsWaves];
  const int lz = threadIdx.x & (kPsTileZ - 1), ly = threadIdx.x / kPsTileZ;
  const long long sx = (long long)Y * Z;
  double acc = 0.0;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int tz = (int)(t % tz_n), ty = (int)((t / tz_n) % ty_n), tx = (int)(t / ((long long)tz_n * ty_n));
    const int k = tz * kPsTileZ + lz, j = ty * kPsTileY + ly;
    if (k >= Z || j >= Y) continue;
    const int i0 = tx * kPsTileX, i1 = i0 + kPsTileX < X ? i0 + kPsTileX : X;
    long long idx = ((long long)i0 * Y + j) * Z + k;
    double lo = i0 > 0 ? p[idx - sx] : 0.0, c = p[idx];
    for (int i = i0; i < i1; ++i, idx += sx) {
      const double hi = i + 1 < X ? p[idx + sx] : 0.0;
      const double ym = j > 0 ? p[idx - Z] : 0.0, yp = j + 1 < Y ? p[idx + Z] : 0.0;
      const double zm = k > 0 ? p[idx - 1] : 0.0, zp = k + 1 < Z ? p[idx + 1] : 0.0;
      const double v = (6.0 * c - (((lo + hi) + (ym + yp)) + (zm + zp))) / h2;
      q[idx] = v;
      if (kDot) acc += c * v;
      lo = c;
      c = hi;
    }
  }
  if (kDot) {
    const double tot = block_sum(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
  }
}

// ------------------------------------------------------------------ conjugate gradients
// r = p = -b, x = 0, partials of r.r
__global__ void __launch_bounds__(kPsThreads) cg_init_kernel(const double* __restrict__ b, long long n, double* __restrict__ x,
                                                              double* __restrict__ r, double* __restrict__ p,
                                                              double* __restrict__ part) {
  __shared__ double lds[kPsWaves];
  const long long stride = (long long)gridDim.x * kPsThreads;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * kPsThreads + threadIdx.x; i < n; i += stride) {
    const double v = -b[i];
    x[i] = 0.0;
    r[i] = v;
    p[i] = v;
    acc += v * v;
  }
  const double tot = block_sum(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// state[0] = state[2] = r.r = b.b
__global__ void __launch_bounds__(kPsThreads) cg_init_finish_kernel(const double* __restrict__ part, int n_part,
                                                                     double* __restrict__ state) {
  __shared__ double lds[kPsWaves];
  const double tot = partials_sum(part, n_part, lds);
  if (threadIdx.x == 0) {
    state[0] = tot;
    state[1] = 0.0;
    state[2] = tot;
  }
}

// alpha = r.r / p.q; x += alpha p; r -= alpha q; partials of the new r.r
__global__ void __launch_bounds__(kPsThreads) cg_update_kernel(double* __restrict__ x, double* __restrict__ r,
                                                                const double* __restrict__ p, const double* __restrict__ q,
                                                                long long n, const double* __restrict__ pq_part, int n_pq,
                                                                const double* __restrict__ state, int slot,
                                                                double* __restrict__ rr_part) {
  __shared__ double lds[kPsWaves];
  const double pq = partials_sum(pq_part, n_pq, lds);
  const double rr = state[slot];
  const double alpha = pq > 0.0 ? rr / pq : 0.0;
  const long long stride = (long long)gridDim.x * kPsThreads;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * kPsThreads + threadIdx.x; i < n; i += stride) {
    x[i] = x[i] + alpha * p[i];
    const double v = r[i] - alpha * q[i];
    r[i] = v;
    acc += v * v;
  }
  const double tot = block_sum(acc, lds);
  if (threadIdx.x == 0) rr_part[blockIdx.x] = tot;
}

// beta = r'.r' / r.r; p = r + beta p; block 0 leaves r'.r' in the other slot
__global__ void __launch_bounds__(kPsThreads) cg_direction_kernel(const double* __restrict__ r, double* __restrict__ p, long long n,
                                                                   const double* __restrict__ rr_part, int n_rr,
                                                                   double* __restrict__ state, int slot) {
  __shared__ double lds[kPsWaves];
  const double rr_new = partials_sum(rr_part, n_rr, lds);
  const double rr = state[slot];
  const double beta = rr > 0.0 ? rr_new / rr : 0.0;
  const long long stride = (long long)gridDim.x * kPsThreads;
  for (long long i = (long long)blockIdx.x * kPsThreads + threadIdx.x; i < n; i += stride) p[i] = r[i] + beta * p[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) state[slot ^ 1] = rr_new;
}

// ------------------------------------------------------------------ trilinear samples of a volume
__global__ void __launch_bounds__(kPsThreads) sample_kernel(const double* __restrict__ vol, PsGrid g, const double* __restrict__ pts,
                                                             long long n, double* __restrict__ values, double* __restrict__ part) {
  __shared__ double lds[kPsWaves];
  const long long stride = (long long)gridDim.x * kPsThreads;
  double acc = 0.0;
  for (long long p = (long long)blockIdx.x * kPsThreads + threadIdx.x; p < n; p += stride) {
    int c[3];
    double t[3];
    double v = NAN;
    if (cell_of(pts, p, g, c, t)) {
      v = 0.0;
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) v += corner_weight(t, corner) * vol[node_of(c, corner, g)];
    }
    values[p] = v;
    acc += v;
  }
  const double tot = block_sum(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kPsThreads) sample_finish_kernel(const double* __restrict__ part, int n_part, long long n,
                                                                    double* __restrict__ mean_out) {
  __shared__ double lds[kPsWaves];
  const double tot = partials_sum(part, n_part, lds);
  if (threadIdx.x == 0) mean_out[0] = tot / (double)n;
}

PsGrid make_grid(const double* origin, double h, const int* dims) {
  PsGrid g;
  for (int a = 0; a < 3; ++a) { g.o[a] = origin[a]; g.d[a] = dims[a]; }
  g.h = h;
  return g;
}

unsigned linear_blocks(long long n) { return (unsigned)((n + kPsThreads - 1) / kPsThreads); }

}  // namespace

long long poisson_tiles(const int* dims) {
  return (long long)((dims[0] + kPsTileX - 1) / kPsTileX) * ((dims[1] + kPsTileY - 1) / kPsTileY) * ((dims[2] + kPsTileZ - 1) / kPsTileZ);
}

int poisson_blocks(long long work_items) {   // blocks of a kernel that leaves one partial each
  return (int)(work_items < kPsMaxBlocks ? (work_items < 1 ? 1 : work_items) : kPsMaxBlocks);
}

hipError_t launch_poisson_splat_keys(const double* pts, long long n, const double* origin, double h, const int* dims, long long* keys,
                                     hipStream_t s) {
  hipLaunchKernelGGL(splat_keys_kernel, dim3(linear_blocks(n)), dim3(kPsThreads), 0, s, pts, n, make_grid(origin, h, dims), keys);
  return hipGetLastError();
}

hipError_t launch_poisson_splat_sum(const double* pts, const double* nrm, long long n, const double* origin, double h, const int* dims,
                                    const long long* keys, const long long* rows, double* V, double* W, hipStream_t s) {
  const size_t nn = (size_t)dims[0] * dims[1] * dims[2];
  hipError_t e = hipMemsetAsync(V, 0, 3 * nn * sizeof(double), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(W, 0, nn * sizeof(double), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(splat_sum_kernel, dim3(linear_blocks(8 * n)), dim3(kPsThreads), 0, s, pts, nrm, n, make_grid(origin, h, dims),
                     keys, rows, V, W);
  return hipGetLastError();
}

hipError_t launch_poisson_divergence(const double* V, const int* dims, double h, double* b, hipStream_t s) {
  const long long nn = (long long)dims[0] * dims[1] * dims[2];
  hipLaunchKernelGGL(divergence_kernel, dim3(linear_blocks(nn)), dim3(kPsThreads), 0, s, V, dims[0], dims[1], dims[2], 2.0 * h, b);
  return hipGetLastError();
}

hipError_t launch_poisson_laplace(const double* p, const int* dims, double h, double* q, double* part, hipStream_t s) {
  const long long tiles = poisson_tiles(dims);
  const int ty_n = (dims[1] + kPsTileY - 1) / kPsTileY, tz_n = (dims[2] + kPsTileZ - 1) / kPsTileZ;
  const dim3 grid((unsigned)poisson_blocks(tiles));
  if (part)
    hipLaunchKernelGGL(laplace_kernel<true>, grid, dim3(kPsThreads), 0, s, p, q, dims[0], dims[1], dims[2], h * h, ty_n, tz_n, tiles, part);
  else
    hipLaunchKernelGGL(laplace_kernel<false>, grid, dim3(kPsThreads), 0, s, p, q, dims[0], dims[1], dims[2], h * h, ty_n, tz_n, tiles,
                       part);
  return hipGetLastError();
}

hipError_t launch_poisson_cg_init(const double* b, long long n, double* x, double* r, double* p, double* part, double* state,
                                  hipStream_t s) {
  const int blocks = poisson_blocks((n + kPsThreads - 1) / kPsThreads);
  hipLaunchKernelGGL(cg_init_kernel, dim3(blocks), dim3(kPsThreads), 0, s, b, n, x, r, p, part);
  hipLaunchKernelGGL(cg_init_finish_kernel, dim3(1), dim3(kPsThreads), 0, s, part, blocks, state);
  return hipGetLastError();
}

hipError_t launch_poisson_cg_iteration(const int* dims, double h, double* x, double* r, double* p, double* q, double* pq_part,
                                       double* rr_part, double* state, int slot, hipStream_t s) {
  const long long n = (long long)dims[0] * dims[1] * dims[2];
  hipError_t e = launch_poisson_laplace(p, dims, h, q, pq_part, s);
  if (e != hipSuccess) return e;
  const int n_pq = poisson_blocks(poisson_tiles(dims));
  const int blocks = poisson_blocks((n + kPsThreads - 1) / kPsThreads);
  hipLaunchKernelGGL(cg_update_kernel, dim3(blocks), dim3(kPsThreads), 0, s, x, r, p, q, n, pq_part, n_pq, state, slot, rr_part);
  hipLaunchKernelGGL(cg_direction_kernel, dim3(blocks), dim3(kPsThreads), 0, s, r, p, n, rr_part, blocks, state, slot);
  return hipGetLastError();
}

hipError_t launch_poisson_sample(const double* vol, const int* dims, const double* origin, double h, const double* pts, long long n,
                                 double* values, double* mean_out, double* part, hipStream_t s) {
  const int blocks = poisson_blocks((n + kPsThreads - 1) / kPsThreads);
  hipLaunchKernelGGL(sample_kernel, dim3(blocks), dim3(kPsThreads), 0, s, vol, make_grid(origin, h, dims), pts, n, values, part);
  if (mean_out) hipLaunchKernelGGL(sample_finish_kernel, dim3(1), dim3(kPsThreads), 0, s, part, blocks, n, mean_out);
  return hipGetLastError();
}

}  // namespace ufr
