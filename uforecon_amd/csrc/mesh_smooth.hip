// Mesh smoothing: Laplacian and Taubin steps with uniform or cotangent weights (include/ufr.h, "mesh smoothing"), every value
// fp64, every product and sum rounded on its own, with the arithmetic that tests/smooth_ref.py restates:
//
//   rows     one thread per sorted corner slot (the slots of ufr_raster_vertex_normals): the two other corners of the slot's
//          face and, for cotangent weights, their two clamped weights from the INPUT positions, stored in row order; a dead
//          row stores (-1, -1) and (0, 0).  Run once per call.
//   border   mesh_rows.h's border rule over the (a, b) rows.
//   step     one thread per vertex walks its rows in order -- ascending slot -- and reads the previous positions only (Jacobi);
//          the caller ping-pongs two buffers.  The walk is mesh_rows.h's staged one: the rows of a block's 256 vertices are
//          staged in LDS, kMeshRowChunk rows at a time, and every thread takes its own rows of the chunk from there, keeping
//          its sums across chunks.  The sums are sequential per vertex, so there is no float atomic and a rerun gives the
//          same bits.  Three shapes that sum in this order were timed (profiles/mesh_smooth_launch_shapes.md): every
//          thread reading its rows from memory itself (2.2 times this one's time with cotangent weights), walking
//          slots -> faces and recomputing the weights in every step (3 times), and this one.  A shuffle tree per vertex sums
//          in another order than the rule states and is not taken.
// 256 threads a block: block sizes from 64 to 1024 time within 6 % of each other on the unstaged cotangent step.  The staged step
// takes 56 VGPRs and 24 KiB of LDS with weights (six waves a SIMD, six blocks a CU), 48 VGPRs and 8 KiB without (eight waves);
// chunks of 512 and 2048 rows are 4 % and 17 % slower.  Every store is a plain store guarded by the array's size.
#include "mesh_rows.h"

namespace ufr {
namespace {

constexpr double kSmoothMaxWeight = 64.0;   // the cotangent of a sliver angle under 0.9 degrees

// not above 0 (a negative cotangent, a NaN): 0; above 64: 64
__device__ inline double clamp_weight(double w) {
  if (!(w > 0.0)) w = 0.0;
  return w > kSmoothMaxWeight ? kSmoothMaxWeight : w;
}

__global__ void __launch_bounds__(kMeshRowThreads) smooth_rows_kernel(const double* __restrict__ verts, const int* __restrict__ faces,
                                                                       long long V, long long F, const long long* __restrict__ slots,
                                                                       int cotangent, int* __restrict__ nbr, double* __restrict__ wgt) {
  const long long i = (long long)blockIdx.x * kMeshRowThreads + threadIdx.x;
  if (i >= 3 * F) return;
  int oa = -1, ob = -1;
  double wa = 0.0, wb = 0.0;
  const SlotCorners c = decode_slot(slots[i], faces, V, F);
  if (c.ok) {
    const long long v = c.v, a = c.a, b = c.b;
    bool live = true;
    if (cotangent) {
      const double p0 = verts[3 * c.c0], p1 = verts[3 * c.c0 + 1], p2 = verts[3 * c.c0 + 2];
      const double u0 = verts[3 * c.c1] - p0, u1 = verts[3 * c.c1 + 1] - p1, u2 = verts[3 * c.c1 + 2] - p2;
      const double t0 = verts[3 * c.c2] - p0, t1 = verts[3 * c.c2 + 1] - p1, t2 = verts[3 * c.c2 + 2] - p2;
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
  nbr[2 * i] = oa;
  nbr[2 * i + 1] = ob;
  if (cotangent) {
    wgt[2 * i] = wa;
    wgt[2 * i + 1] = wb;
  }
}

// kCot: the rows carry weight pairs (else every weight is 1 and no weight is staged)
template <bool kCot>
__global__ void __launch_bounds__(kMeshRowThreads) smooth_step_kernel(long long V, long long F, const long long* __restrict__ runs,
                                                                       const int* __restrict__ nbr, const double* __restrict__ wgt,
                                                                       const unsigned char* __restrict__ border,
                                                                       const unsigned char* __restrict__ pinned, double t,
                                                                       const double* __restrict__ in, double* __restrict__ out) {
  __shared__ int2 s_nbr[kMeshRowChunk];
  __shared__ double2 s_wgt[kCot ? kMeshRowChunk : 1];
  const long long v = (long long)blockIdx.x * kMeshRowThreads + threadIdx.x;
  const bool valid = v < V;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  bool walk = false;
  if (valid) {
    p0 = in[3 * v], p1 = in[3 * v + 1], p2 = in[3 * v + 2];
    walk = !((border && border[v]) || (pinned && pinned[v]));
  }
  double n0 = 0.0, n1 = 0.0, n2 = 0.0, den = 0.0;
  for_each_staged_row(
      runs, V, 3 * F, walk,
      [&](int j, long long i) {
        s_nbr[j] = reinterpret_cast<const int2*>(nbr)[i];
        if (kCot) s_wgt[j] = reinterpret_cast<const double2*>(wgt)[i];
      },
      [&](int j) {
        const int2 ab = s_nbr[j];
        const long long a = ab.x, b = ab.y;
        if (a < 0 || a >= V || b < 0 || b >= V) return;
        double wa = 1.0, wb = 1.0;
        if (kCot) {
          const double2 w = s_wgt[j];
          wa = w.x, wb = w.y;
        }
        n0 += wa * (in[3 * a] - p0) + wb * (in[3 * b] - p0);
        n1 += wa * (in[3 * a + 1] - p1) + wb * (in[3 * b + 1] - p1);
        n2 += wa * (in[3 * a + 2] - p2) + wb * (in[3 * b + 2] - p2);
        den += wa + wb;
      });
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
  hipLaunchKernelGGL(smooth_rows_kernel, dim3(mesh_row_blocks(3 * F)), dim3(kMeshRowThreads), 0, s, verts, faces, V, F, slots, cotangent,
                     nbr, wgt);
  return hipGetLastError();
}

hipError_t launch_mesh_smooth_border(long long V, long long F, const long long* runs, const int* nbr, unsigned char* border,
                                     hipStream_t s) {
  hipLaunchKernelGGL(mesh_border_kernel<int2>, dim3(mesh_row_blocks(V)), dim3(kMeshRowThreads), 0, s, V, F, runs,
                     reinterpret_cast<const int2*>(nbr), border);
  return hipGetLastError();
}

hipError_t launch_mesh_smooth_step(long long V, long long F, const long long* runs, const int* nbr, const double* wgt,
                                   const unsigned char* border, const unsigned char* pinned, double t, const double* in,
                                   double* out, hipStream_t s) {
  const auto kernel = wgt ? smooth_step_kernel<true> : smooth_step_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(mesh_row_blocks(V)), dim3(kMeshRowThreads), 0, s, V, F, runs, nbr, wgt, border, pinned, t, in, out);
  return hipGetLastError();
}

}  // namespace ufr
