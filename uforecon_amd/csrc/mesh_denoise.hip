// Mesh denoising: the bilateral normal filter of Zheng et al. 2011 (local, iterative) with the vertex update of Sun et al. 2007
// (include/ufr.h, "mesh denoising"), every value fp64, every product, quotient and sum rounded on its own, with the arithmetic
// that tests/denoise_ref.py restates:
//
//   faces    one thread per face: the 64-byte record (n0, n1, n2, A | c0, c1, c2, live) from the INPUT positions, zeros for a
//          dead face, and the face's own normal into the caller's (F,3) array.  Run once per call.
//   rows     one thread per sorted corner slot (the slots of ufr_raster_vertex_normals): (g, a, b, e) -- the slot's face, its
//          two other corners and the corner the row stands at -- or (-1, -1, -1, 0) for a row of a dead face; and g once more in
//          an array of its own, 4 bytes a row, for the normal step.  Run once per call.
//   border   mesh_rows.h's border rule over these rows, as smoothing runs it over its own.
//   normals  one thread per face, the hot path: itself first, then the rows of its three corner vertices in ascending slot,
//          each row's g read by the thread that uses it (4 bytes; the runs of one face's corners are not one span, so there is
//          nothing for a block to stage).  At the second and third corner the neighbour's three indices say whether it names an
//          earlier corner of this face; then g fetches the neighbour's record: ONE 64-byte gather, half a cache line, normal,
//          area and centroid together.  Reads the previous records only (Jacobi) and writes the whole next record, so the
//          caller ping-pongs two record buffers; the last step also writes the (F,3) normals.
//   vertices one thread per vertex walks its rows in order and reads the previous positions only; the rows of a block's 256
//          vertices are one span, staged in LDS kMeshRowChunk rows at a time by mesh_rows.h's staged walk.  A row's e
//          gives the face's own corner order back, so the centroid is summed as the rule states without a read of the faces.
// Every sum is sequential per face or vertex in the header's order: no float atomic, no shuffle tree, a rerun gives the same
// bits.  A run may be longer than a chunk or a block: its thread's loop is then long, not wrong.  Every index read from
// memory (slot, g, a, b, e, the corner indices) is range-checked before use; every store is a plain store guarded by the
// array's size.  k(u) = (1 - u / 256)^256 by eight squarings stands in for exp(-u) without a transcendental call.
// The shapes of the normal step that were timed are in profiles/mesh_denoise_launch_shapes.md.
// 256 threads a block everywhere (64, 128 and 512 are 13 %, 6 % and 2 % slower on the normal step).  normals: 58 VGPRs, no LDS.
// vertices: 59 VGPRs, 16 KiB of LDS (1024 rows of 16 bytes; ten blocks a CU by LDS, eight by waves).  faces 55, rows 20, border
// 37 VGPRs, no LDS.  All five fit eight waves a SIMD.
#include "mesh_rows.h"

namespace ufr {
namespace {

// (1 - u / 256)^256; 0 from u = 256 on and for a NaN
__device__ inline double weight_kernel(double u) {
  double x = 1.0 - u / 256.0;
  if (!(x > 0.0)) return 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) x = x * x;
  return x;
}

__global__ void __launch_bounds__(kMeshRowThreads) denoise_faces_kernel(const double* __restrict__ verts, const int* __restrict__ faces, long long V,
                                                                         long long F, double2* __restrict__ rec, double* __restrict__ normals) {
  const long long f = (long long)blockIdx.x * kMeshRowThreads + threadIdx.x;
  if (f >= F) return;
  const long long c0 = faces[3 * f], c1 = faces[3 * f + 1], c2 = faces[3 * f + 2];
  double n0 = 0.0, n1 = 0.0, n2 = 0.0, A = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, flag = 0.0;
  if (corners_live(c0, c1, c2, V)) {
    const double p0 = verts[3 * c0], p1 = verts[3 * c0 + 1], p2 = verts[3 * c0 + 2];
    const double q0 = verts[3 * c1], q1 = verts[3 * c1 + 1], q2 = verts[3 * c1 + 2];
    const double r0 = verts[3 * c2], r1 = verts[3 * c2 + 1], r2 = verts[3 * c2 + 2];
    const double u0 = q0 - p0, u1 = q1 - p1, u2 = q2 - p2;
    const double t0 = r0 - p0, t1 = r1 - p1, t2 = r2 - p2;
    const double m0 = u1 * t2 - u2 * t1, m1 = u2 * t0 - u0 * t2, m2 = u0 * t1 - u1 * t0;
    const double nf = sqrt(dot3(m0, m1, m2, m0, m1, m2));
    if (nf > 0.0 && isfinite(nf)) {
      n0 = m0 / nf, n1 = m1 / nf, n2 = m2 / nf;
      A = 0.5 * nf;
      g0 = ((p0 + q0) + r0) / 3.0, g1 = ((p1 + q1) + r1) / 3.0, g2 = ((p2 + q2) + r2) / 3.0;
      flag = 1.0;
    }
  }
  rec[4 * f] = make_double2(n0, n1);
  rec[4 * f + 1] = make_double2(n2, A);
  rec[4 * f + 2] = make_double2(g0, g1);
  rec[4 * f + 3] = make_double2(g2, flag);
  normals[3 * f] = n0;
  normals[3 * f + 1] = n1;
  normals[3 * f + 2] = n2;
}

__global__ void __launch_bounds__(kMeshRowThreads) denoise_rows_kernel(const int* __restrict__ faces, long long V, long long F,
                                                                        const long long* __restrict__ slots, const double2* __restrict__ rec,
                                                                        int4* __restrict__ rows, int* __restrict__ row_face) {
  const long long i = (long long)blockIdx.x * kMeshRowThreads + threadIdx.x;
  if (i >= 3 * F) return;
  int4 row = make_int4(-1, -1, -1, 0);
  const SlotCorners c = decode_slot(slots[i], faces, V, F);
  if (c.ok && rec[4 * c.f + 3].y != 0.0)                     // live: its normal is finite too
    row = make_int4((int)c.f, (int)c.a, (int)c.b, c.e);
  rows[i] = row;
  row_face[i] = row.x;
}

__global__ void __launch_bounds__(kMeshRowThreads) denoise_normal_kernel(const int* __restrict__ faces, long long V, long long F,
                                                                          const long long* __restrict__ runs, const int* __restrict__ row_face,
                                                                          double two_ss, double two_rr, const double2* __restrict__ in,
                                                                          double2* __restrict__ out, double* __restrict__ normals) {
  const long long f = (long long)blockIdx.x * kMeshRowThreads + threadIdx.x;
  if (f >= F) return;
  const double2 r0 = in[4 * f], r1 = in[4 * f + 1], r2 = in[4 * f + 2], r3 = in[4 * f + 3];
  const double n0 = r0.x, n1 = r0.y, n2 = r1.x, c0 = r2.x, c1 = r2.y, c2 = r3.x;
  double o0 = n0, o1 = n1, o2 = n2;
  if (r3.y != 0.0) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const auto add = [&](const double2 g0, const double2 g1, const double2 g2, const double2 g3) {
      const double d0 = g2.x - c0, d1 = g2.y - c1, d2 = g3.x - c2;
      const double e0 = g0.x - n0, e1 = g0.y - n1, e2 = g1.x - n2;
      const double w = (g1.y * weight_kernel(dot3(d0, d1, d2, d0, d1, d2) / two_ss)) * weight_kernel(dot3(e0, e1, e2, e0, e1, e2) / two_rr);
      a0 += w * g0.x;
      a1 += w * g0.y;
      a2 += w * g1.x;
    };
    add(r0, r1, r2, r3);                                    // itself first
    const int cv[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const long long v = cv[e];
      if (v < 0 || v >= V) continue;
      long long i, i1;
      run_of(runs, v, 3 * F, &i, &i1);
      for (; i < i1; ++i) {
        const long long g = row_face[i];
        if (g < 0 || g >= F || g == f) continue;            // a dead row; itself
        if (e >= 1) {                                       // names an earlier corner: counted there.  g is live: its indices are distinct
          const int h0 = faces[3 * g], h1 = faces[3 * g + 1], h2 = faces[3 * g + 2];
          if (h0 == cv[0] || h1 == cv[0] || h2 == cv[0]) continue;
          if (e == 2 && (h0 == cv[1] || h1 == cv[1] || h2 == cv[1])) continue;
        }
        add(in[4 * g], in[4 * g + 1], in[4 * g + 2], in[4 * g + 3]);
      }
    }
    const double L = sqrt(dot3(a0, a1, a2, a0, a1, a2));
    if (L > 0.0 && isfinite(L)) o0 = a0 / L, o1 = a1 / L, o2 = a2 / L;
  }
  out[4 * f] = make_double2(o0, o1);
  out[4 * f + 1] = make_double2(o2, r1.y);
  out[4 * f + 2] = r2;
  out[4 * f + 3] = r3;
  if (normals) {
    normals[3 * f] = o0;
    normals[3 * f + 1] = o1;
    normals[3 * f + 2] = o2;
  }
}

__global__ void __launch_bounds__(kMeshRowThreads) denoise_vertex_kernel(long long V, long long F, const long long* __restrict__ runs,
                                                                          const int4* __restrict__ rows, const double* __restrict__ normals,
                                                                          const unsigned char* __restrict__ border,
                                                                          const unsigned char* __restrict__ pinned, const double* __restrict__ in,
                                                                          double* __restrict__ out) {
  __shared__ int4 s_rows[kMeshRowChunk];
  const long long v = (long long)blockIdx.x * kMeshRowThreads + threadIdx.x;
  const bool valid = v < V;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  bool walk = false;
  if (valid) {
    p0 = in[3 * v], p1 = in[3 * v + 1], p2 = in[3 * v + 2];
    walk = !((border && border[v]) || (pinned && pinned[v]));
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, cnt = 0.0;
  for_each_staged_row(
      runs, V, 3 * F, walk, [&](int j, long long i) { s_rows[j] = rows[i]; },
      [&](int j) {
        const int4 row = s_rows[j];
        const long long g = row.x, a = row.y, b = row.z;
        if (g < 0 || g >= F || a < 0 || a >= V || b < 0 || b >= V || row.w < 0 || row.w > 2) return;
        const double a0 = in[3 * a], a1 = in[3 * a + 1], a2 = in[3 * a + 2];
        const double q0 = in[3 * b], q1 = in[3 * b + 1], q2 = in[3 * b + 2];
        const double m0 = normals[3 * g], m1 = normals[3 * g + 1], m2 = normals[3 * g + 2];
        double g0, g1, g2;                                  // the centroid in the face's own corner order
        if (row.w == 0) g0 = (p0 + a0) + q0, g1 = (p1 + a1) + q1, g2 = (p2 + a2) + q2;            // (v, a, b)
        else if (row.w == 1) g0 = (q0 + p0) + a0, g1 = (q1 + p1) + a1, g2 = (q2 + p2) + a2;       // (b, v, a)
        else g0 = (a0 + q0) + p0, g1 = (a1 + q1) + p1, g2 = (a2 + q2) + p2;                       // (a, b, v)
        const double d = dot3(g0 / 3.0 - p0, g1 / 3.0 - p1, g2 / 3.0 - p2, m0, m1, m2);
        s0 += m0 * d;
        s1 += m1 * d;
        s2 += m2 * d;
        cnt += 1.0;
      });
  if (!valid) return;
  double o0 = p0, o1 = p1, o2 = p2;
  if (walk && cnt > 0.0) {
    o0 = p0 + s0 / cnt;
    o1 = p1 + s1 / cnt;
    o2 = p2 + s2 / cnt;
  }
  out[3 * v] = o0;
  out[3 * v + 1] = o1;
  out[3 * v + 2] = o2;
}

}  // namespace

hipError_t launch_mesh_denoise_faces(const double* verts, const int* faces, long long V, long long F, double* rec, double* normals,
                                     hipStream_t s) {
  hipLaunchKernelGGL(denoise_faces_kernel, dim3(mesh_row_blocks(F)), dim3(kMeshRowThreads), 0, s, verts, faces, V, F, reinterpret_cast<double2*>(rec), normals);
  return hipGetLastError();
}

hipError_t launch_mesh_denoise_rows(const int* faces, long long V, long long F, const long long* slots, const double* rec, int* rows,
                                    int* row_face, hipStream_t s) {
  hipLaunchKernelGGL(denoise_rows_kernel, dim3(mesh_row_blocks(3 * F)), dim3(kMeshRowThreads), 0, s, faces, V, F, slots,
                     reinterpret_cast<const double2*>(rec), reinterpret_cast<int4*>(rows), row_face);
  return hipGetLastError();
}

hipError_t launch_mesh_denoise_border(long long V, long long F, const long long* runs, const int* rows, unsigned char* border,
                                      hipStream_t s) {
  hipLaunchKernelGGL(mesh_border_kernel<int4>, dim3(mesh_row_blocks(V)), dim3(kMeshRowThreads), 0, s, V, F, runs,
                     reinterpret_cast<const int4*>(rows), border);
  return hipGetLastError();
}

hipError_t launch_mesh_denoise_normals(const int* faces, long long V, long long F, const long long* runs, const int* row_face, double two_ss,
                                       double two_rr, const double* in, double* out, double* normals, hipStream_t s) {
  hipLaunchKernelGGL(denoise_normal_kernel, dim3(mesh_row_blocks(F)), dim3(kMeshRowThreads), 0, s, faces, V, F, runs, row_face,
                     two_ss, two_rr, reinterpret_cast<const double2*>(in), reinterpret_cast<double2*>(out), normals);
  return hipGetLastError();
}

hipError_t launch_mesh_denoise_vertices(long long V, long long F, const long long* runs, const int* rows, const double* normals,
                                        const unsigned char* border, const unsigned char* pinned, const double* in, double* out,
                                        hipStream_t s) {
  hipLaunchKernelGGL(denoise_vertex_kernel, dim3(mesh_row_blocks(V)), dim3(kMeshRowThreads), 0, s, V, F, runs, reinterpret_cast<const int4*>(rows), normals,
                     border, pinned, in, out);
  return hipGetLastError();
}

}  // namespace ufr
