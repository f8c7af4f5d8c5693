// Ordered compaction, shared by marching cubes (mcubes.hip), mesh sampling (chamfer.hip) and the depth fusion's point cloud
// (depth_fusion.hip): every item (voxel, triangle, pixel) emits a variable number of outputs, and the outputs are stored
// densely in item order.  Three steps, no atomics, no inter-block flags, the same result run after run:
//   count  one thread per item counts its outputs; a block-wide exclusive scan (block_scan_excl, or block_rank where the
//          count is 0 or 1) gives the block's sum, one per block ("block total");
//   scan   one block of kScanThreads threads per column of totals (scan_totals_kernel): exclusive prefix of the block totals
//          -> block offsets, and the grand total, which the host reads to size the output (one synchronisation);
//   emit   the count again, the same block scan, + the block's offset -> every item's first output slot.
// All sums are integer sums, so how a scan groups them cannot change a result.
#pragma once
#include <hip/hip_runtime.h>

namespace ufr {

constexpr int kScanThreads = 1024;

// block-wide exclusive scan of v over kThreads threads (wave shuffles, then the wave totals through lds[kThreads / 64]);
// *total gets the block sum.  Every thread of the block must call it.  Ends with a barrier, so it may be called again
// with the same lds.
template <typename T, int kThreads>
__device__ inline T block_scan_excl(T v, T* lds, T* total) {
  static_assert(kThreads % 64 == 0, "whole waves");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T u = __shfl_up(incl, d);
    if (lane >= d) incl += u;
  }
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const T s = lds[w];
    before += w < wave ? s : 0;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// block_scan_excl for counts of 0 or 1, by ballot: this thread's slot among the valid threads of its block, and their
// number.  Every thread of the block must call it; one barrier, so a second call needs another lds[kThreads / 64].
template <int kThreads>
__device__ inline int block_rank(bool valid, int* lds, int* count) {
  const unsigned long long b = __ballot(valid);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = __popcll(b);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const int c = lds[w];
    before += w < wave ? c : 0;
    total += c;
  }
  *count = total;
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

// block c of the grid scans column c of in[n][kColumns]: off[t][c] = in[0][c] + ... + in[t - 1][c], totals[c] = the sum.
// Thread i sums rows i * per .. (i + 1) * per - 1; past kScanThreads rows, per > 1 and the last threads may have none.
// The block's scan is a Hillis-Steele loop in LDS, not block_scan_excl: the kernel runs once per compaction, with a cold
// instruction cache, and there the short loop measured faster than the unrolled shuffles (profiles/compaction_refactor.md).
template <int kColumns, typename T>
__global__ void __launch_bounds__(kScanThreads) scan_totals_kernel(const T* __restrict__ in, long long n,
                                                                    long long* __restrict__ off, long long* __restrict__ totals) {
  __shared__ long long sa[kScanThreads];
  const int c = blockIdx.x;
  const long long per = (n + kScanThreads - 1) / kScanThreads;
  const long long t0 = min((long long)threadIdx.x * per, n), t1 = min(t0 + per, n);
  long long a = 0;
  for (long long t = t0; t < t1; ++t) a += in[t * kColumns + c];
  sa[threadIdx.x] = a;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const long long u = threadIdx.x >= (unsigned)d ? sa[threadIdx.x - d] : 0;
    __syncthreads();
    sa[threadIdx.x] += u;
    __syncthreads();
  }
  long long o = sa[threadIdx.x] - a;
  for (long long t = t0; t < t1; ++t) {
    off[t * kColumns + c] = o;
    o += in[t * kColumns + c];
  }
  if (threadIdx.x == kScanThreads - 1) totals[c] = sa[threadIdx.x];
}

template <int kColumns, typename T>
inline hipError_t launch_scan_totals(const T* in, long long n, long long* off, long long* totals, hipStream_t s) {
  hipLaunchKernelGGL((scan_totals_kernel<kColumns, T>), dim3(kColumns), dim3(kScanThreads), 0, s, in, n, off, totals);
  return hipGetLastError();
}

}  // namespace ufr
