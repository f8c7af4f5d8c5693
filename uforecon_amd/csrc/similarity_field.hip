// The similarity field: the mean grouped cosine similarity of the cross-view matching features on a voxel grid.
//   UFORecon.extract_fields / extract_similarity   code1/model.py:844-911
//   UFORecon.query_cond_info                       code1/model.py:218-305  (pairwise cosine similarity, AC=True/border)
// = gather.hip's pair similarity (sim8) on grid points, averaged over the 8 groups, and nothing else of the gather: it reads
// the match maps only and writes 4 bytes per voxel (include/ufr.h: ufr_similarity_field).
//
// A wave owns a run of 64 z-consecutive voxels of one (x, y) column.  Phase A, lane L = voxel L of the run: the projection
// into every view (the gather's arithmetic), the visibility count, the border-clamped bilinear footprint per view into LDS.
// Phase B, eight passes of 8 voxels: 8 adjacent lanes share a voxel and each takes one 4-channel group, so a side's
// 32-channel chunk of a texel is one 128-byte line per load instruction; the pair mean stays in the lane, the group mean is
// three cross-lane steps.  The 64 results go through LDS back to lane L = voxel L: one 256-byte store per wave.
// The match maps (5 MB per view at 128x160x64) stay cache resident; the kernel is bound by the issue of its gathers.
//
// The grid's coordinate tables travel as kernel arguments, one tile of at most kSfTileX x kSfTileY x kSfTileZ voxels per
// launch: no device allocation, no copy, nothing the caller has to keep alive.
#include <algorithm>
#include "ufr_device.h"
#include "ufr_internal.h"

namespace ufr {

namespace {

constexpr int kSfWaves = 4;                                   // waves (= runs) per block
constexpr int kSfRun = 64;                                    // voxels per run
constexpr int kSfTileX = 64, kSfTileY = 128, kSfTileZ = 512;  // a launch's tile: 2 816 bytes of tables in the kernel arguments

struct SfTile {
  int x0, y0, z0, nx, ny, nz;   // origin and extent of the tile in the grid
  float gx[kSfTileX], gy[kSfTileY], gz[kSfTileZ];
};

typedef int sf_i32x4 __attribute__((ext_vector_type(4)));

// The three helpers below restate gather.hip's (lerp_tap4_buf, put_tap, get_tap), which are private to that file and stay
// untouched: the same loads, the same fma chain.
// out = fma(v_se,se, fma(v_sw,sw, fma(v_ne,ne, v_nw*nw))) per channel; border clamping leaves no masked corner
__device__ __forceinline__ f32x4 sf_lerp_tap4(__amdgpu_buffer_rsrc_t r, unsigned base, unsigned stride_bytes, const Tap2& t, unsigned c4) {
  f32x4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = buf_ld4(r, t.o[k] >= 0 ? base + (unsigned)t.o[k] * stride_bytes + c4 : kBufOut);
  f32x4 acc;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a = mul_rn(v[0][e], t.w[0]);
    a = fmaf(v[1][e], t.w[1], a);
    a = fmaf(v[2][e], t.w[2], a);
    acc[e] = fmaf(v[3][e], t.w[3], a);
  }
  return acc;
}
__device__ __forceinline__ void sf_put_tap(float* dst, const Tap2& t) {
  *reinterpret_cast<sf_i32x4*>(dst) = sf_i32x4{t.o[0], t.o[1], t.o[2], t.o[3]};
  *reinterpret_cast<f32x4*>(dst + 4) = f32x4{t.w[0], t.w[1], t.w[2], t.w[3]};
}
__device__ __forceinline__ Tap2 sf_get_tap(const float* src) {
  const sf_i32x4 o = *reinterpret_cast<const sf_i32x4*>(src);
  const f32x4 w = *reinterpret_cast<const f32x4*>(src + 4);
  Tap2 t;
#pragma unroll
  for (int k = 0; k < 4; ++k) { t.o[k] = o[k]; t.w[k] = w[k]; }
  return t;
}

// LDS (floats), per wave: taps[NV][64][8] | u[64]
__global__ __launch_bounds__(kSfWaves * 64) void similarity_field_kernel(const FrameDev f, const SfTile tile, int Y, int Z,
                                                                         float* __restrict__ u, unsigned char* __restrict__ n_vis,
                                                                         int min_views) {
  extern __shared__ __attribute__((aligned(16))) float sf_lds[];
  const int NV = f.NV, npair = NV * (NV - 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* sh_tap = sf_lds + (size_t)wave * (NV * 64 * 8 + 64);
  float* sh_u = sh_tap + NV * 64 * 8;

  // the wave's run; a wave past the last run repeats it without storing (every thread reaches the barriers)
  const int zruns = (tile.nz + kSfRun - 1) / kSfRun;
  const long long n_runs = (long long)tile.nx * tile.ny * zruns;
  const long long run_raw = (long long)blockIdx.x * kSfWaves + wave;
  const bool run_ok = run_raw < n_runs;
  const long long run = run_ok ? run_raw : n_runs - 1;
  const int col = (int)(run / zruns), zr = (int)(run - (long long)col * zruns);
  const int i = col / tile.ny, j = col - i * tile.ny;
  const int k = zr * kSfRun + lane;
  const bool store = run_ok && k < tile.nz;
  const int kc = k < tile.nz ? k : tile.nz - 1;

  // ---- phase A: lane = voxel
  const float px = tile.gx[i], py = tile.gy[j], pz = tile.gz[kc];
  int vis = 0;
  bool finite = true;
  for (int v = 0; v < NV; ++v) {
    // projection into view v: gather.hip's k-ordered fma chain (camera.py:384-393), no depth mask on the similarity
    const float* M = f.pose[v];
    const float qx = fmaf(M[2], pz, fmaf(M[1], py, mul_rn(M[0], px))) + M[3];
    const float qy = fmaf(M[6], pz, fmaf(M[5], py, mul_rn(M[4], px))) + M[7];
    const float qz = fmaf(M[10], pz, fmaf(M[9], py, mul_rn(M[8], px))) + M[11];
    const float x = qx / qz, y = qy / qz;
    finite = finite && fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff();   // false for NaN too
    vis += (qz > 0.f && x > -1.f && x < 1.f && y > -1.f && y < 1.f) ? 1 : 0;         // mask_valid_depth & in_mask
    sf_put_tap(sh_tap + (v * 64 + lane) * 8, taps_border(unnorm2d_ac(x, f.w), unnorm2d_ac(y, f.h), f.w, f.h));
  }
  __syncthreads();

  // ---- phase B: 8 lanes = one voxel, lane c8 = channel group gi of model.py:278-280
  const int c8 = lane & 7, sub = lane >> 3;
  const unsigned map_px = (unsigned)(f.h * f.w), mrow = (unsigned)f.match_ch * 4u;
  const __amdgpu_buffer_rsrc_t rmatch = buf_rsrc(f.match, (unsigned)NV * map_px * mrow);
  for (int pass = 0; pass < 8; ++pass) {
    const int lp = pass * 8 + sub;
    float s = 0.f;
    // pair (a, b): sides (view a, chunk b) / (view b + 1, chunk a) (model.py:271-283), in the reference's order
    for (int a = 0; a < NV - 1; ++a) {
      const Tap2 ta = sf_get_tap(sh_tap + (a * 64 + lp) * 8);
      for (int b = a; b < NV - 1; ++b) {
        const Tap2 tb = sf_get_tap(sh_tap + ((b + 1) * 64 + lp) * 8);
        const f32x4 fa = sf_lerp_tap4(rmatch, (unsigned)a * map_px * mrow + 128u * (unsigned)b, mrow, ta, 16u * c8);
        const f32x4 fb = sf_lerp_tap4(rmatch, (unsigned)(b + 1) * map_px * mrow + 128u * (unsigned)a, mrow, tb, 16u * c8);
        // gather.hip's sim8 expression: F.normalize(x) = x * (1 / max(|x|, eps)), then the dot product
        const float na = fmaxf(sqrtf(fa[0] * fa[0] + fa[1] * fa[1] + fa[2] * fa[2] + fa[3] * fa[3]), 1e-8f);
        const float nb = fmaxf(sqrtf(fb[0] * fb[0] + fb[1] * fb[1] + fb[2] * fb[2] + fb[3] * fb[3]), 1e-8f);
        const float ra = __builtin_amdgcn_rcpf(na), rb = __builtin_amdgcn_rcpf(nb);
        s += (fa[0] * ra) * (fb[0] * rb) + (fa[1] * ra) * (fb[1] * rb) + (fa[2] * ra) * (fb[2] * rb) + (fa[3] * ra) * (fb[3] * rb);
      }
    }
    float m = s / (float)npair;          // torch.mean over pairs
    m += __shfl_xor(m, 1);               // ... then over the 8 groups: every lane of the voxel ends with the same sum
    m += __shfl_xor(m, 2);
    m += __shfl_xor(m, 4);
    if (c8 == 0) sh_u[lp] = m * 0.125f;
  }
  __syncthreads();

  // ---- lane = voxel again: 64 consecutive floats per wave
  if (store) {
    const bool keep = finite && vis >= min_views;
    const long long idx = ((long long)(tile.x0 + i) * Y + (tile.y0 + j)) * Z + (tile.z0 + k);
    u[idx] = keep ? sh_u[lane] : -1.f;
    if (n_vis) n_vis[idx] = (unsigned char)vis;
  }
}

}  // namespace

hipError_t launch_similarity_field(const FrameDev& f, const float* gx, const float* gy, const float* gz, const int* dim, float* u,
                                   unsigned char* n_vis, int min_views, hipStream_t s) {
  const int X = dim[0], Y = dim[1], Z = dim[2];
  const size_t lds = sizeof(float) * (size_t)kSfWaves * ((size_t)f.NV * 64 * 8 + 64);
  SfTile t = {};
  for (t.z0 = 0; t.z0 < Z; t.z0 += kSfTileZ) {
    t.nz = std::min(kSfTileZ, Z - t.z0);
    std::copy(gz + t.z0, gz + t.z0 + t.nz, t.gz);
    for (t.y0 = 0; t.y0 < Y; t.y0 += kSfTileY) {
      t.ny = std::min(kSfTileY, Y - t.y0);
      std::copy(gy + t.y0, gy + t.y0 + t.ny, t.gy);
      for (t.x0 = 0; t.x0 < X; t.x0 += kSfTileX) {
        t.nx = std::min(kSfTileX, X - t.x0);
        std::copy(gx + t.x0, gx + t.x0 + t.nx, t.gx);
        const long long runs = (long long)t.nx * t.ny * ((t.nz + kSfRun - 1) / kSfRun);   // <= 64 * 128 * 8
        const unsigned blocks = (unsigned)((runs + kSfWaves - 1) / kSfWaves);
        hipLaunchKernelGGL(similarity_field_kernel, dim3(blocks), dim3(kSfWaves * 64), lds, s, f, t, Y, Z, u, n_vis, min_views);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
      }
    }
  }
  return hipSuccess;
}

}  // namespace ufr
