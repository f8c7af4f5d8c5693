// What the per-vertex mesh stages share on the device (raster.hip's vertex normals, mesh_color.hip's fill round, mesh_smooth.hip,
// mesh_denoise.hip).  The caller sorts the 3F corner slots 3f + e stably by the vertex they name and passes the V + 1 run
// starts; a vertex's run is walked in ascending slot, so every sum has one order: no float atomic, a rerun gives the same bits.
// A ring stage supplies a row format, a rows kernel (slot -> row, through decode_slot) and a per-row body; it gets the run
// clipping, the border rule (mesh_border_kernel over its rows) and the staged block walk (for_each_staged_row) from here.
// Every index read from memory is range-checked before use: a wrong caller array gives wrong numbers, never a fault.
// Only kernel files include this.
#pragma once
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {

constexpr int kMeshRowThreads = 256;      // rows, faces or vertices a block owns (ops.MESH_ROW_BLOCK says the same to the tests)
constexpr int kMeshRowChunk = 1024;       // rows a block of a staged walk holds in LDS at a time (ops.MESH_ROW_CHUNK)

inline unsigned mesh_row_blocks(long long n) { return (unsigned)((n + kMeshRowThreads - 1) / kMeshRowThreads); }

__device__ inline double dot3(double x0, double x1, double x2, double y0, double y1, double y2) {
  return (x0 * y0 + x1 * y1) + x2 * y2;
}

// three corners in 0 .. V-1 and distinct
__device__ inline bool corners_live(long long c0, long long c1, long long c2, long long V) {
  return c0 >= 0 && c0 < V && c1 >= 0 && c1 < V && c2 >= 0 && c2 < V && c0 != c1 && c1 != c2 && c0 != c2;
}

// the run of vertex v, clipped to the rows there are
__device__ inline void run_of(const long long* __restrict__ runs, long long v, long long rows, long long* i0, long long* i1) {
  long long a = runs[v], b = runs[v + 1];
  if (a < 0) a = 0;
  if (b > rows) b = rows;
  *i0 = a, *i1 = b;
}

// Two readings of a slot, kept apart because they are behaviour:
//   slot_names   (vertex normals, colour fill): the slot is in 0 .. 3F-1 and names vertex v; the corners need not be distinct.
//   decode_slot  (smooth and denoise rows): the slot is in 0 .. 3F-1 and its face's corners are in range and distinct; v is not asked.
__device__ inline bool slot_names(long long slot, const int* __restrict__ faces, long long F, long long v) {
  return slot >= 0 && slot < 3 * F && (long long)faces[slot] == v;
}

// slot 3f + e: whether it is usable, the face, e, the face's corners, and the corner the slot names (v) with the other two
// in the face's order after it (a, b).  v, a and b are picked from locals here, not by the caller from the fields: a pick among
// neighbouring fields becomes an indexed read of the struct, and the compiler then keeps the struct in LDS.
struct SlotCorners {
  bool ok;
  int e;
  long long f, c0, c1, c2, v, a, b;
};
__device__ __forceinline__ SlotCorners decode_slot(long long slot, const int* __restrict__ faces, long long V, long long F) {
  SlotCorners s = {false, 0, 0, 0, 0, 0, 0, 0, 0};
  if (slot < 0 || slot >= 3 * F) return s;
  const long long f = slot / 3;
  const int e = (int)(slot - 3 * f);
  const long long c0 = faces[3 * f], c1 = faces[3 * f + 1], c2 = faces[3 * f + 2];
  s.f = f, s.e = e, s.c0 = c0, s.c1 = c1, s.c2 = c2;
  s.v = e == 0 ? c0 : e == 1 ? c1 : c2;
  s.a = e == 0 ? c1 : e == 1 ? c2 : c0;
  s.b = e == 0 ? c2 : e == 1 ? c0 : c1;
  s.ok = corners_live(c0, c1, c2, V);
  return s;
}

// a row's neighbour pair, and whether the row is dead (its first field is -1), for the two row formats
__device__ inline int2 row_pair(int2 r) { return r; }                       // smoothing: (a, b)
__device__ inline int2 row_pair(int4 r) { return make_int2(r.y, r.z); }    // denoising: (g, a, b, e)
__device__ inline bool row_dead(int2 r) { return r.x < 0; }
__device__ inline bool row_dead(int4 r) { return r.x < 0; }

// One thread per vertex: a neighbour that does not stand exactly twice in the vertex's live rows marks it.  The count is a
// double loop over the run: quadratic in the degree, which is 6 on a mesh and whatever a soup makes it.  A dead row's pair is
// (-1, -1), equal to no neighbour.
template <class Row>
__global__ void __launch_bounds__(kMeshRowThreads) mesh_border_kernel(long long V, long long F, const long long* __restrict__ runs,
                                                                       const Row* __restrict__ rows, unsigned char* __restrict__ border) {
  const long long v = (long long)blockIdx.x * kMeshRowThreads + threadIdx.x;
  if (v >= V) return;
  long long i0, i1;
  run_of(runs, v, 3 * F, &i0, &i1);
  bool open = false;
  for (long long i = i0; i < i1 && !open; ++i) {
    const Row row = rows[i];
    if (row_dead(row)) continue;
    const int2 ab = row_pair(row);
    int ca = 0, cb = 0;                                     // both neighbours of the row are counted in one pass over the run
    for (long long k = i0; k < i1; ++k) {
      const int2 q = row_pair(rows[k]);
      ca += (q.x == ab.x ? 1 : 0) + (q.y == ab.x ? 1 : 0);
      cb += (q.x == ab.y ? 1 : 0) + (q.y == ab.y ? 1 : 0);
    }
    open = ca != 2 || cb != 2;
  }
  border[v] = open ? 1 : 0;
}

// The staged walk of a block of kMeshRowThreads vertices (the grid is ceil(V / kMeshRowThreads)).  The runs of the block's
// vertices are one span of the row arrays: the block stages it kMeshRowChunk rows at a time -- stage(j, i) copies global row i
// to LDS place j, coalesced -- and between two barriers a thread with `walk` set calls use(j) for its own rows of the chunk, in
// ascending order, keeping whatever it sums across chunks.  Every thread of the block must call this, walking or not.  A run
// may be longer than a chunk or a block: its thread's loop is then long, not wrong.
template <class Stage, class Use>
__device__ __forceinline__ void for_each_staged_row(const long long* __restrict__ runs, long long V, long long rows, bool walk,
                                                    Stage stage, Use use) {
  const long long first = (long long)blockIdx.x * kMeshRowThreads;     // < V
  const long long last = first + kMeshRowThreads < V ? first + kMeshRowThreads : V;
  const long long v = first + threadIdx.x;
  long long b0, b1;                                         // the block's rows
  run_of(runs, first, rows, &b0, &b1);
  b1 = runs[last] > rows ? rows : runs[last];
  long long i = 0, i1 = 0;
  if (v < V) run_of(runs, v, rows, &i, &i1);
  for (long long base = b0; base < b1; base += kMeshRowChunk) {
    const int cnt = (int)(b1 - base < kMeshRowChunk ? b1 - base : kMeshRowChunk);
    for (int j = threadIdx.x; j < cnt; j += kMeshRowThreads) stage(j, base + j);
    __syncthreads();
    if (walk) {
      if (i < base) i = base;                               // runs that are not ascending: rows outside the span are skipped
      for (; i < i1 && i < base + cnt; ++i) use((int)(i - base));
    }
    __syncthreads();
  }
}

}  // namespace ufr
