// Tile helpers shared by the transformer kernels (view_transformer.hip, ray_transformer.hip and their data-gradient chains
// view_dgrad.hip, ray_dgrad.hip): activations are fp32 accumulator tiles in registers, tokens the 16 MFMA columns, lane (g, j)
// = (lane >> 4, lane & 15) holding features 4g + r (or the kernel's feature map of (tile, g, r)) of token column j.  The GEMM
// core and the weight stream are weight_stream_f16.h; the lane-exchange primitives underneath are ufr_device.h.
// A helper belongs here only if every kernel using it compiles to the device code it had with the helper written out.
#pragma once
#include "weight_stream_f16.h"

namespace ufr {

// base + 32-bit element offset, the byte offset computed in 32 bits: the access becomes "scalar base + 32-bit lane
// offset" (global_load ... v_off, s[base]) with no 64-bit per-lane address to keep alive (the launcher bounds the sizes)
template <class T>
__device__ __forceinline__ T* at32(T* base, unsigned elem) {
  typedef typename std::conditional<std::is_const<T>::value, const char, char>::type B;
  return reinterpret_cast<T*>(reinterpret_cast<B*>(base) + (elem * (unsigned)sizeof(T)));
}

template <int C, int N>
__device__ __forceinline__ void zero_tiles(f32x4 (&t)[C][N]) {
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) t[c][i] = splat4(0.f);
}

// LayerNorm over the D features of each token: NT tiles x 4 registers in each of the 4 lane groups.  D = 80: five whole
// tiles; D = 88 (nat88): five whole tiles and tile 5 with registers 0, 1 real, 2, 3 padding (VW / VB are zero there).
// t holds raw accumulators (asc = 2^(s_M + a_M) times the values; asc = 1: plain values): the normalised value is scale-free
// once the epsilon carries the square of the scale (eps = 1e-5 asc^2, formed once per launch), and with a power-of-two scale
// every intermediate is the exact multiple -- bit-identical to descaling first.
// XH / RS (TAPE builds): the normalised input (0 in padding registers) and 1 / sigma of the TRUE values (asc times the raw
// one), which the backward needs.
// The operation order is part of the contract (the tape and the forward-only builds are compared bit for bit): whole tiles
// summed as (t0 + t1) + (t2 + t3), then the tail t0 + t1; the variance skips padding registers.
template <int NT, int D, int VW, int VB, int C, class WS>
__device__ __forceinline__ void layer_norm_tiles(f32x4 (&t)[C][NT], const WS& ws, int g, float eps, float asc, f32x4 (*XH)[NT] = nullptr, float* RS = nullptr) {
  constexpr int FULL = D / 16, TAIL = (D - 16 * FULL) / 4;   // whole tiles; real registers of the tile behind them
  static_assert((TAIL == 0 || TAIL == 2) && NT == FULL + (TAIL ? 1 : 0) && D == 16 * FULL + 4 * TAIL, "natural or nat88 layout");
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < FULL; ++i) s += (t[c][i][0] + t[c][i][1]) + (t[c][i][2] + t[c][i][3]);
    if constexpr (TAIL == 2) s += t[c][FULL][0] + t[c][FULL][1];
    const float mean = sum_groups(s) * (1.f / (float)D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (i < FULL || r < TAIL) {
          float d = t[c][i][r] - mean;
          q = fmaf(d, d, q);
        }
      }
    const float rstd = fast_rsqrt(sum_groups(q) * (1.f / (float)D) + eps);
    if (RS) RS[c] = rstd * asc;
    // element by element on purpose: f32x4 expressions become v_pk_mul / v_pk_fma_f32, which cost more beside the
    // partner wave's MFMAs than the two scalar instructions they replace (MI355X_MICROARCH.md, price of a filler)
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const f32x4 gw = vec_frag<VW>(ws, i, g), gb = vec_frag<VB>(ws, i, g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xh = (t[c][i][r] - mean) * rstd;
        if (XH) XH[c][i][r] = (i >= FULL && r >= TAIL) ? 0.f : xh;
        t[c][i][r] = xh * gw[r] + gb[r];
      }
    }
  }
}

// ---- token reductions of the data-gradient chains (LayerNorm gamma / beta, the view token)
// v[i] <- sum of v[i] over the 16 lanes of the DPP row (= the 16 token columns of a lane group), for ten values.  One block
// of assembly: a DPP read needs two wait states after a VALU write of the same register and the hazard recogniser does not
// look inside inline assembly -- within the block a register's next read is ten instructions after its write.
__device__ __forceinline__ void row_allreduce10(float (&v)[10]) {
#define UFR_RR_STEP(CTRL)                                                    \
  "v_add_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_dpp %1, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_dpp %2, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_dpp %3, %3, %3 " CTRL " row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_dpp %4, %4, %4 " CTRL " row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_dpp %5, %5, %5 " CTRL " row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_dpp %6, %6, %6 " CTRL " row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_dpp %7, %7, %7 " CTRL " row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_dpp %8, %8, %8 " CTRL " row_mask:0xf bank_mask:0xf\n\t"        \
  "v_add_f32_dpp %9, %9, %9 " CTRL " row_mask:0xf bank_mask:0xf\n\t"
  asm volatile("s_nop 1\n\t" UFR_RR_STEP("quad_perm:[1,0,3,2]") UFR_RR_STEP("quad_perm:[2,3,0,1]") UFR_RR_STEP("row_half_mirror")
               UFR_RR_STEP("row_mirror")
               : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), "+v"(v[9]));
#undef UFR_RR_STEP
}
// acc[64 b] += sum over the 16 token lanes of value 10 b + j of the NT-tile vector t (4 NT values per lane group, in blocks
// of ten, the padding ones zero): after the all-reduce every lane of a row holds all ten sums and lane j < 10 keeps the
// j-th.  Accumulated over the wave's whole persistent loop -- in a private LDS slot per (vector, block, lane): ten more live
// registers cost view_dgrad 50..70 spills -- and flushed once (flush80 / rd_flush88 of the kernels): per iteration the atomics of all waves
// would queue up on the same few hundred addresses (measured: +0.1 ms, more than the tiles had cost).
__host__ __device__ constexpr int acc_blocks(int nt) { return (4 * nt + 9) / 10; }
template <int NT>
__device__ __forceinline__ void reduce_acc_tiles(const f32x4 (&t)[NT], float* acc /* LDS: [acc_blocks(NT)][64], this lane's column */, int j) {
#pragma unroll
  for (int b = 0; b < acc_blocks(NT); ++b) {
    float v[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) v[i] = 10 * b + i < 4 * NT ? t[(10 * b + i) >> 2][(10 * b + i) & 3] : 0.f;
    row_allreduce10(v);
    float mine = v[0];
#pragma unroll
    for (int i = 1; i < 10; ++i) mine = j == i ? v[i] : mine;
    acc[64 * b] += mine;
  }
}

}  // namespace ufr
