// Marching cubes over a TSDF volume (the step after csrc/tsdf.hip): an indexed triangle mesh with shared vertices, in the
// order and with the arithmetic that tests/mcubes_ref.py restates bit for bit (include/ufr.h, ufr_marching_cubes_*).
// Replaces skimage.measure.marching_cubes_lewiner as the reference's TSDFVolume.get_mesh calls it (tsdf_fusion.py:340-357),
// without copying the volumes to the host.
//
// Four launches, the ordered compaction of compact.h with two columns (vertices, faces) and two emit kernels:
//   count  one thread per voxel (lanes along z, coalesced), TILE voxels per block: the voxel's crossing edges (<= 3,
//          owned by it: p -> p + e_axis) and, for a cube origin, its case's triangle count; one block sum per tile;
//   scan   the tile sums -> tile offsets and the two totals (the host reads those);
//   verts  recount, block scan + tile offset -> vertex ids in (voxel, axis) order; position, normal; the voxel's first
//          vertex id into the index volume (workspace, written only where the voxel owns a vertex);
//   faces  recount cases, block scan + tile offset -> face ids in (cube, table order) order; vertex id of a triangle
//          edge = index[owner] + popcount(owner's crossing bits below the edge's axis).
// Every output store is guarded by the caller's capacity.  Volumes hold fewer than 2^31 voxels (api_geometry.hip checks it).
#include "compact.h"
#include "mcubes_table.h"
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kMcThreads = 256;
constexpr int kMcIters = 16;

struct McVol {
  const float* f;
  int X, Y, Z;
  float level;
  __device__ float at(int x, int y, int z) const { return f[((size_t)x * Y + y) * Z + z]; }
  __device__ bool below(int x, int y, int z) const { return at(x, y, z) < level; }
  __device__ int dim(int a) const { return a == 0 ? X : a == 1 ? Y : Z; }
};

__device__ inline void coords(const McVol& v, unsigned idx, int& x, int& y, int& z) {
  const unsigned yz = (unsigned)v.Y * (unsigned)v.Z;
  x = (int)(idx / yz);
  const unsigned r = idx - (unsigned)x * yz;
  y = (int)(r / (unsigned)v.Z);
  z = (int)(r - (unsigned)y * (unsigned)v.Z);
}

// crossing bits of voxel (x,y,z): bit a iff the edge to p + e_a exists and exactly one end is below
__device__ inline int crossing_bits(const McVol& v, int x, int y, int z, bool b0) {
  int m = 0;
  if (x + 1 < v.X && v.below(x + 1, y, z) != b0) m |= 1;
  if (y + 1 < v.Y && v.below(x, y + 1, z) != b0) m |= 2;
  if (z + 1 < v.Z && v.below(x, y, z + 1) != b0) m |= 4;
  return m;
}

// case index of the cube with lowest corner (x,y,z); -1 if (x,y,z) is not a cube origin
__device__ inline int cube_case(const McVol& v, int x, int y, int z) {
  if (x + 1 >= v.X || y + 1 >= v.Y || z + 1 >= v.Z) return -1;
  int c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) c |= (int)v.below(x + (k & 1), y + ((k >> 1) & 1), z + ((k >> 2) & 1)) << k;
  return c;
}

// d f / d axis at (x,y,z): central difference inside, one-sided at the border
__device__ inline float grad(const McVol& v, int x, int y, int z, int a) {
  const int n = v.dim(a), i = a == 0 ? x : a == 1 ? y : z;
  const int dx = a == 0, dy = a == 1, dz = a == 2;
  if (i == 0) return v.at(x + dx, y + dy, z + dz) - v.at(x, y, z);
  if (i == n - 1) return v.at(x, y, z) - v.at(x - dx, y - dy, z - dz);
  return (v.at(x + dx, y + dy, z + dz) - v.at(x - dx, y - dy, z - dz)) * 0.5f;
}

__global__ void __launch_bounds__(kMcThreads) mcubes_count_kernel(McVol v, unsigned n, int* __restrict__ tile_counts) {
  __shared__ long long lds[kMcThreads / 64];
  const unsigned base = blockIdx.x * (unsigned)(kMcThreads * kMcIters);
  int nv = 0, nt = 0;
  for (int it = 0; it < kMcIters; ++it) {
    const unsigned idx = base + it * kMcThreads + threadIdx.x;
    if (idx >= n) break;
    int x, y, z;
    coords(v, idx, x, y, z);
    nv += __popc(crossing_bits(v, x, y, z, v.below(x, y, z)));
    const int c = cube_case(v, x, y, z);
    if (c >= 0) nt += kMcTriCount[c];
  }
  // both block sums from one scan: vertices in the high word, triangles in the low one (a tile has at most 3 * 4096 and
  // 5 * 4096 of them, so the low word never carries): the shuffles and LDS traffic of one scan of an int pair
  long long tot;
  block_scan_excl<long long, kMcThreads>((long long)nv << 32 | nt, lds, &tot);
  if (threadIdx.x == 0) {
    tile_counts[2 * blockIdx.x] = (int)(tot >> 32);
    tile_counts[2 * blockIdx.x + 1] = (int)tot;
  }
}

__global__ void __launch_bounds__(kMcThreads) mcubes_verts_kernel(McVol v, unsigned n, const long long* __restrict__ tile_off,
                                                                   int* __restrict__ index, float* __restrict__ verts,
                                                                   float* __restrict__ normals, long long n_verts) {
  __shared__ int lds[kMcThreads / 64];
  const unsigned base = blockIdx.x * (unsigned)(kMcThreads * kMcIters);
  long long run = tile_off[2 * blockIdx.x];
  for (int it = 0; it < kMcIters; ++it) {
    const unsigned idx = base + it * kMcThreads + threadIdx.x;
    if (base + it * kMcThreads >= n) break;              // block-uniform: the scan below needs every thread
    int x = 0, y = 0, z = 0, m = 0;
    float f0 = 0.f;
    if (idx < n) {
      coords(v, idx, x, y, z);
      f0 = v.at(x, y, z);
      m = crossing_bits(v, x, y, z, f0 < v.level);
    }
    int tot;
    long long id = run + block_scan_excl<int, kMcThreads>(__popc(m), lds, &tot);
    run += tot;
    if (!m) continue;
    index[idx] = (int)id;
    for (int a = 0; a < 3; ++a) {
      if (!(m >> a & 1)) continue;
      const long long vid = id++;
      if (vid < 0 || vid >= n_verts) continue;
      const int qx = x + (a == 0), qy = y + (a == 1), qz = z + (a == 2);
      const float f1 = v.at(qx, qy, qz);
      const float t = (v.level - f0) / (f1 - f0);     // f1 != f0: exactly one of them is below the level
      float pos[3] = {(float)x, (float)y, (float)z};
      pos[a] = pos[a] + t;
      float g[3];
      for (int d = 0; d < 3; ++d) {
        const float g0 = grad(v, x, y, z, d), g1 = grad(v, qx, qy, qz, d);
        const float dg = g1 - g0;
        const float tg = t * dg;
        g[d] = g0 + tg;
      }
      const float xx = g[0] * g[0], yy = g[1] * g[1], zz = g[2] * g[2];
      const float len = sqrtf((xx + yy) + zz);
      for (int d = 0; d < 3; ++d) {
        verts[3 * vid + d] = pos[d];
        normals[3 * vid + d] = len > 0.f ? g[d] / len : 0.f;
      }
    }
  }
}

// the vertex id of edge (owner (x,y,z), axis a)
__device__ inline long long edge_vertex(const McVol& v, const int* __restrict__ index, int x, int y, int z, int a) {
  long long id = index[((size_t)x * v.Y + y) * v.Z + z];
  if (a > 0) {
    const bool b0 = v.below(x, y, z);
    if (x + 1 < v.X && v.below(x + 1, y, z) != b0) ++id;
    if (a > 1 && y + 1 < v.Y && v.below(x, y + 1, z) != b0) ++id;
  }
  return id;
}

__global__ void __launch_bounds__(kMcThreads) mcubes_faces_kernel(McVol v, unsigned n, const long long* __restrict__ tile_off,
                                                                   const int* __restrict__ index, int* __restrict__ faces,
                                                                   long long n_faces) {
  __shared__ int lds[kMcThreads / 64];
  const unsigned base = blockIdx.x * (unsigned)(kMcThreads * kMcIters);
  long long run = tile_off[2 * blockIdx.x + 1];
  for (int it = 0; it < kMcIters; ++it) {
    const unsigned idx = base + it * kMcThreads + threadIdx.x;
    if (base + it * kMcThreads >= n) break;
    int x = 0, y = 0, z = 0, c = -1;
    if (idx < n) {
      coords(v, idx, x, y, z);
      c = cube_case(v, x, y, z);
    }
    const int nt = c >= 0 ? (int)kMcTriCount[c] : 0;
    int tot;
    const long long first = run + block_scan_excl<int, kMcThreads>(nt, lds, &tot);
    run += tot;
    for (int k = 0; k < nt; ++k) {
      const long long fid = first + k;
      if (fid < 0 || fid >= n_faces) continue;
      for (int j = 0; j < 3; ++j) {
        const int e = kMcTable[c][3 * k + j];
        const int a = e >> 2, r = e & 3;
        const int o1 = a == 0 ? 1 : 0, o2 = a == 2 ? 1 : 2;      // the other two axes, lower first
        int off[3] = {0, 0, 0};
        off[o1] = r & 1;
        off[o2] = r >> 1;
        faces[3 * fid + j] = (int)edge_vertex(v, index, x + off[0], y + off[1], z + off[2], a);
      }
    }
  }
}

McVol make_vol(const float* vol, const int* dim, float level) {
  McVol v;
  v.f = vol;
  v.X = dim[0];
  v.Y = dim[1];
  v.Z = dim[2];
  v.level = level;
  return v;
}

}  // namespace

int mcubes_tiles(const int* dim) {
  const long long n = (long long)dim[0] * dim[1] * dim[2];
  return (int)((n + kMcThreads * kMcIters - 1) / (kMcThreads * kMcIters));
}

hipError_t launch_mcubes_count(const float* vol, const int* dim, float level, int* tile_counts, hipStream_t s) {
  const unsigned n = (unsigned)((long long)dim[0] * dim[1] * dim[2]);
  hipLaunchKernelGGL(mcubes_count_kernel, dim3(mcubes_tiles(dim)), dim3(kMcThreads), 0, s, make_vol(vol, dim, level), n,
                     tile_counts);
  return hipGetLastError();
}

// tile_counts and tile_off hold two interleaved columns: vertices, faces
hipError_t launch_mcubes_scan(const int* tile_counts, int n_tiles, long long* tile_off, long long* totals, hipStream_t s) {
  return launch_scan_totals<2>(tile_counts, n_tiles, tile_off, totals, s);
}

hipError_t launch_mcubes_verts(const float* vol, const int* dim, float level, const long long* tile_off, int* index,
                               float* verts, float* normals, long long n_verts, hipStream_t s) {
  const unsigned n = (unsigned)((long long)dim[0] * dim[1] * dim[2]);
  hipLaunchKernelGGL(mcubes_verts_kernel, dim3(mcubes_tiles(dim)), dim3(kMcThreads), 0, s, make_vol(vol, dim, level), n,
                     tile_off, index, verts, normals, n_verts);
  return hipGetLastError();
}

hipError_t launch_mcubes_faces(const float* vol, const int* dim, float level, const long long* tile_off, const int* index,
                               int* faces, long long n_faces, hipStream_t s) {
  const unsigned n = (unsigned)((long long)dim[0] * dim[1] * dim[2]);
  hipLaunchKernelGGL(mcubes_faces_kernel, dim3(mcubes_tiles(dim)), dim3(kMcThreads), 0, s, make_vol(vol, dim, level), n,
                     tile_off, index, faces, n_faces);
  return hipGetLastError();
}

}  // namespace ufr
