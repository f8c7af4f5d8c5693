// Mesh smoothing: Laplacian and Taubin steps with uniform or cotangent weights (include/ufr.h, "mesh smoothing"), every value
// fp64, every product and sum rounded on its own, with the arithmetic that tests/smooth_ref.py restates:
//
//   rows     one thread per sorted corner slot (the slots of ufr_raster_vertex_normals): the two other corners of the slot's
//          face and, for cotangent weights, their two clamped weights from the INPUT positions, stored in row order; a dead
//          row stores (-1, -1) and (0, 0).  Run once per call.
//   border   one thread per vertex: a neighbour that does not stand exactly twice in the vertex's live rows marks it.  The
//          count is a double loop over the run: quadratic in the degree, which is 6 on a mesh and whatever a soup makes it.
//   step     one thread per vertex walks its rows in order -- ascending slot -- and reads the previous positions only (Jacobi);
//          the caller ping-pongs two buffers.  The rows of a block's 256 vertices are one span of the row arrays: the block
//          stages it in LDS, kSmoothChunk rows at a time with coalesced loads, and every thread then takes its own rows of
//          the chunk from there, keeping its sums across chunks.  The sums are sequential per vertex, so there is no float
//          atomic and a rerun gives the same bits.  A run may be longer than a chunk or a block: its thread's loop is then
//          long, not wrong.  Three shapes that sum in this order were timed (profiles/mesh_smooth_launch_shapes.md): every
//          thread reading its rows from memory itself (2.2 times this one's time with cotangent weights), walking
//          slots -> faces and recomputing the weights in every step (3 times), and this one.  A shuffle tree per vertex sums
//          in another order than the rule states and is not taken.
// 256 threads a block: block sizes from 64 to 1024 time within 6 % of each other on the unstaged cotangent step, 44 VGPRs allow eight
// waves a SIMD, and a chunk of 1024 rows (24 KiB with weights, 8 KiB without) leaves room for six blocks a CU; chunks of 512
// and 2048 rows are 4 % and 17 % slower.  Every store is a plain store guarded by the array's size.
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kSm = kSmoothThreads;
constexpr double kSmoothMaxWeight = 64.0;   // the cotangent of a sliver angle under 0.9 degrees

unsigned blocks_of(long long n) { return (unsigned)((n + kSm - 1) / kSm); }

__device__ inline double dot3(double x0, double x1, double x2, double y0, double y1, double y2) {
  return (x0 * y0 + x1 * y1) + x2 * y2;
}

// not above 0 (a negative cotangent, a NaN): 0; above 64: 64
__device__ inline double clamp_weight(double w) {
  if (!(w > 0.0)) w = 0.0;
  return w > kSmoothMaxWeight ? kSmoothMaxWeight : w;
}

__global__ void __launch_bounds__(kSm) smooth_rows_kernel(const double* __restrict__ verts, const int* __restrict__ faces, long long V,
                                                           long long F, const long long* __restrict__ slots, int cotangent,
                                                           int* __restrict__ nbr, double* __restrict__ wgt) {
  const long long rows = 3 * F;
  const long long i = (long long)blockIdx.x * kSm + threadIdx.x;
  if (i >= rows) return;
  int oa = -1, ob = -1;
  double wa = 0.0, wb = 0.0;
  const long long slot = slots[i];
  if (slot >= 0 && slot < rows) {
    const long long f = slot / 3;
    const int e = (int)(slot - 3 * f);
    const long long c0 = faces[3 * f], c1 = faces[3 * f + 1], c2 = faces[3 * f + 2];
    bool live = c0 >= 0 && c0 < V && c1 >= 0 && c1 < V && c2 >= 0 && c2 < V && c0 != c1 && c1 != c2 && c0 != c2;
    if (live) {
      const long long v = e == 0 ? c0 : e == 1 ? c1 : c2;
      const long long a = e == 0 ? c1 : e == 1 ? c2 : c0;
      const long long b = e == 0 ? c2 : e == 1 ? c0 : c1;
      if (cotangent) {
        const double p0 = verts[3 * c0], p1 = verts[3 * c0 + 1], p2 = verts[3 * c0 + 2];
        const double u0 = verts[3 * c1] - p0, u1 = verts[3 * c1 + 1] - p1, u2 = verts[3 * c1 + 2] - p2;
        const double t0 = verts[3 * c2] - p0, t1 = verts[3 * c2 + 1] - p1, t2 = verts[3 * c2 + 2] - p2;
        const double n0 = u1 * t2 - u2 * t1, n1 = u2 * t0 - u0 * t2, n2 = u0 * t1 - u1 * t0;
        const double nf = sqrt(dot3(n0, n1, n2, n0, n1, n2));
        live = nf > 0.0 && isfinite(nf);
        if (live) {
          const double v0 = verts[3 * v], v1 = verts[3 * v + 1], v2 = verts[3 * v + 2];
          const double a0 = verts[3 * a], a1 = verts[3 * a + 1], a2 = verts[3 * a + 2];
          const double b0 = verts[3 * b], b1 = verts[3 * b + 1], b2 = verts[3 * b + 2];
          wa = clamp_weight(dot3(v0 - b0, v1 - b1, v2 - b2, a0 - b0, a1 - b1, a2 - b2) / nf);   // the angle at b
          wb = clamp_weight(dot3(v0 - a0, v1 - a1, v2 - a2, b0 - a0, b1 - a1, b2 - a2) / nf);   // the angle at a
        }
      }
      if (live) oa = (int)a, ob = (int)b;
    }
  }
  nbr[2 * i] = oa;
  nbr[2 * i + 1] = ob;
  if (cotangent) {
    wgt[2 * i] = wa;
    wgt[2 * i + 1] = wb;
  }
}

// the run of vertex v, clipped to the rows there are
__device__ inline void run_of(const long long* __restrict__ runs, long long v, long long rows, long long* i0, long long* i1) {
  long long a = runs[v], b = runs[v + 1];
  if (a < 0) a = 0;
  if (b > rows) b = rows;
  *i0 = a, *i1 = b;
}

__global__ void __launch_bounds__(kSm) smooth_border_kernel(long long V, long long F, const long long* __restrict__ runs,
                                                             const int* __restrict__ nbr, unsigned char* __restrict__ border) {
  const long long v = (long long)blockIdx.x * kSm + threadIdx.x;
  if (v >= V) return;
  long long i0, i1;
  run_of(runs, v, 3 * F, &i0, &i1);
  const int2* __restrict__ pairs = reinterpret_cast<const int2*>(nbr);
  bool open = false;
  for (long long i = i0; i < i1 && !open; ++i) {
    const int2 ab = pairs[i];
    if (ab.x < 0) continue;                                 // a dead row: (-1, -1), equal to no neighbour
    int ca = 0, cb = 0;                                     // both neighbours of the row are counted in one pass over the run
    for (long long k = i0; k < i1; ++k) {
      const int2 q = pairs[k];
      ca += (q.x == ab.x ? 1 : 0) + (q.y == ab.x ? 1 : 0);
      cb += (q.x == ab.y ? 1 : 0) + (q.y == ab.y ? 1 : 0);
    }
    open = ca != 2 || cb != 2;
  }
  border[v] = open ? 1 : 0;
}

// kCot: the rows carry weight pairs (else every weight is 1 and no weight is staged)
template <bool kCot>
__global__ void __launch_bounds__(kSm) smooth_step_kernel(long long V, long long F, const long long* __restrict__ runs,
                                                           const int* __restrict__ nbr, const double* __restrict__ wgt,
                                                           const unsigned char* __restrict__ border,
                                                           const unsigned char* __restrict__ pinned, double t,
                                                           const double* __restrict__ in, double* __restrict__ out) {
  __shared__ int2 s_nbr[kSmoothChunk];
  __shared__ double2 s_wgt[kCot ? kSmoothChunk : 1];
  const long long rows = 3 * F;
  const long long first = (long long)blockIdx.x * kSm;     // < V: the grid is ceil(V / kSm)
  const long long last = first + kSm < V ? first + kSm : V;
  const long long v = first + threadIdx.x;
  const bool valid = v < V;
  long long b0, b1;                                         // the block's rows: the runs of its vertices are one span
  run_of(runs, first, rows, &b0, &b1);
  b1 = runs[last] > rows ? rows : runs[last];
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  long long i = 0, i1 = 0;
  bool walk = false;
  if (valid) {
    p0 = in[3 * v], p1 = in[3 * v + 1], p2 = in[3 * v + 2];
    run_of(runs, v, rows, &i, &i1);
    walk = !((border && border[v]) || (pinned && pinned[v]));
  }
  double n0 = 0.0, n1 = 0.0, n2 = 0.0, den = 0.0;
  for (long long base = b0; base < b1; base += kSmoothChunk) {
    const int cnt = (int)(b1 - base < kSmoothChunk ? b1 - base : kSmoothChunk);
    for (int j = threadIdx.x; j < cnt; j += kSm) {         // the chunk's rows, coalesced
      s_nbr[j] = reinterpret_cast<const int2*>(nbr)[base + j];
      if (kCot) s_wgt[j] = reinterpret_cast<const double2*>(wgt)[base + j];
    }
    __syncthreads();
    if (walk) {
      if (i < base) i = base;                               // runs that are not ascending: rows outside the span are skipped
      for (; i < i1 && i < base + cnt; ++i) {               // this thread's rows of the chunk, in order
        const int2 ab = s_nbr[i - base];
        const long long a = ab.x, b = ab.y;
        if (a < 0 || a >= V || b < 0 || b >= V) continue;
        double wa = 1.0, wb = 1.0;
        if (kCot) {
          const double2 w = s_wgt[i - base];
          wa = w.x, wb = w.y;
        }
        n0 += wa * (in[3 * a] - p0) + wb * (in[3 * b] - p0);
        n1 += wa * (in[3 * a + 1] - p1) + wb * (in[3 * b + 1] - p1);
        n2 += wa * (in[3 * a + 2] - p2) + wb * (in[3 * b + 2] - p2);
        den += wa + wb;
      }
    }
    __syncthreads();
  }
  if (!valid) return;
  double o0 = p0, o1 = p1, o2 = p2;
  if (walk && den > 0.0) {
    o0 = p0 + (t * n0) / den;
    o1 = p1 + (t * n1) / den;
    o2 = p2 + (t * n2) / den;
  }
  out[3 * v] = o0;
  out[3 * v + 1] = o1;
  out[3 * v + 2] = o2;
}

}  // namespace

hipError_t launch_mesh_smooth_rows(const double* verts, const int* faces, long long V, long long F, const long long* slots,
                                   int cotangent, int* nbr, double* wgt, hipStream_t s) {
  hipLaunchKernelGGL(smooth_rows_kernel, dim3(blocks_of(3 * F)), dim3(kSm), 0, s, verts, faces, V, F, slots, cotangent, nbr, wgt);
  return hipGetLastError();
}

hipError_t launch_mesh_smooth_border(long long V, long long F, const long long* runs, const int* nbr, unsigned char* border,
                                     hipStream_t s) {
  hipLaunchKernelGGL(smooth_border_kernel, dim3(blocks_of(V)), dim3(kSm), 0, s, V, F, runs, nbr, border);
  return hipGetLastError();
}

hipError_t launch_mesh_smooth_step(long long V, long long F, const long long* runs, const int* nbr, const double* wgt,
                                   const unsigned char* border, const unsigned char* pinned, double t, const double* in,
                                   double* out, hipStream_t s) {
  if (wgt)
    hipLaunchKernelGGL(smooth_step_kernel<true>, dim3(blocks_of(V)), dim3(kSm), 0, s, V, F, runs, nbr, wgt, border, pinned, t, in, out);
  else
    hipLaunchKernelGGL(smooth_step_kernel<false>, dim3(blocks_of(V)), dim3(kSm), 0, s, V, F, runs, nbr, wgt, border, pinned, t, in, out);
  return hipGetLastError();
}

}  // namespace ufr
