// Morton keys of grid cells and the implicit octree over a key-sorted point set, shared by the chamfer evaluation (chamfer.hip:
// cell keys, thinning, nearest neighbour) and the point-cloud filters (points_filter.hip: k nearest neighbours).  A node of the
// octree is a key prefix, that is a contiguous range of the sorted set; its children are found by binary search inside the range.
#pragma once
#include <hip/hip_runtime.h>

namespace ufr {

constexpr int kKeyBits = 21;                       // per axis
constexpr long long kMaxCell = (1ll << kKeyBits) - 1;
constexpr int kNnStack = 7 * kKeyBits + 8;         // a depth-first walk pushes at most 8 children per level and pops one

struct NnGrid { double o[3], cell; };              // the origin and cell the keys were made with

__host__ __device__ inline unsigned long long spread3(unsigned long long x) {
  x &= 0x1fffffull;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

__host__ __device__ inline unsigned long long compact3(unsigned long long x) {
  x &= 0x1249249249249249ull;
  x = (x | x >> 2) & 0x10c30c30c30c30c3ull;
  x = (x | x >> 4) & 0x100f00f00f00f00full;
  x = (x | x >> 8) & 0x1f0000ff0000ffull;
  x = (x | x >> 16) & 0x1f00000000ffffull;
  x = (x | x >> 32) & 0x1fffffull;
  return x;
}

__host__ __device__ inline long long morton(long long cx, long long cy, long long cz) {
  return (long long)(spread3((unsigned long long)cx) << 2 | spread3((unsigned long long)cy) << 1 | spread3((unsigned long long)cz));
}

// first index in [lo, hi) whose key is >= k
__host__ __device__ inline long long lower_bound(const long long* __restrict__ keys, long long lo, long long hi, long long k) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace ufr
