// View selection of a COLMAP model: the score of every image pair that the reference's colmap2mvsnet.py computes in Python
// (calc_score, :385-399) -- for i < j the sum, over the observations of image i whose 3-D point image j also sees, of a
// piecewise Gaussian of the triangulation angle at that point (include/ufr.h, ufr_view_pair_scores, states the formula).
//
//   offsets_upload  the CSR offsets are HOST memory; they reach the workspace in launch arguments, kOffsetsPerLaunch at a time
//          (no staging buffer, no copy that could wait for the stream).
//   sort_lists      one workgroup per image: a copy of its observation list, sorted ascending in place in the workspace by a
//          bitonic network whose compare-exchanges all point the same way (the first step of every merge pairs t with
//          t ^ (2k - 1)), so that a list of any length sorts as if padded with +inf: a pair whose upper index is past the end
//          is skipped.  Integers only: the result does not depend on scheduling.  The network runs in global memory (the L1 /
//          L2 hold a list of some thousand indices); one barrier per step.
//   pair_scores     one workgroup of 256 threads per pair i < j.  Thread t takes the observations t, t + 256, ... of image i IN
//          FILE ORDER (so multiplicity follows image i's list), looks each index up in image j's sorted copy by binary search
//          and adds the term to its own fp64 partial sum; the 256 partial sums are then added in a fixed tree: inside a wave
//          lane l += lane l + 32, 16, 8, 4, 2, 1 (shuffles), then (w0 + w1) + (w2 + w3) through LDS.  Which observation goes
//          to which thread, and the tree, depend on the list's length alone: a rerun gives the same bits, and there is no
//          floating-point atomic.  score[i][j] and its copy score[j][i] are written by thread 0; the diagonal is the memset
//          of the launcher.  The index lists are the memory traffic (image i's list streams once, coalesced; the ~log2(len_j)
//          probes of a search hit lines of image j's list that the whole workgroup shares through the L1), the fp64 acos / exp /
//          sqrt of a shared point the arithmetic.  LDS: four doubles.  An index outside 0 .. M-1 counts as "no point".
//
// Every index is 64-bit where it can exceed 2^31 (positions in the concatenated lists); fp contraction is off: the formula's
// products and sums are rounded one by one, as numpy rounds them.
#include "ufr_internal.h"

#pragma clang fp contract(off)

namespace ufr {
namespace {

constexpr int kVsThreads = 256;
constexpr int kOffsetsPerLaunch = 448;   // 3584 bytes of a launch's 4 KiB of arguments

struct OffsetChunk {
  long long v[kOffsetsPerLaunch];
};

__global__ void __launch_bounds__(kVsThreads) offsets_upload_kernel(OffsetChunk c, int first, int count, long long* __restrict__ dst) {
  const int t = blockIdx.x * kVsThreads + threadIdx.x;
  if (t < count) dst[first + t] = c.v[t];
}

__global__ void __launch_bounds__(kVsThreads) sort_lists_kernel(const int* __restrict__ obs, const long long* __restrict__ offsets,
                                                                 int* __restrict__ sorted) {
  const long long begin = offsets[blockIdx.x];
  const long long n = offsets[blockIdx.x + 1] - begin;
  const int* src = obs + begin;
  int* a = sorted + begin;
  for (long long t = threadIdx.x; t < n; t += kVsThreads) a[t] = src[t];
  __syncthreads();
  for (long long k = 2; (k >> 1) < n; k <<= 1) {
    for (long long j = k >> 1; j > 0; j >>= 1) {
      const long long flip = (j == (k >> 1)) ? k - 1 : j;
      for (long long t = threadIdx.x; t < n; t += kVsThreads) {
        const long long u = t ^ flip;
        if (u > t && u < n) {
          const int x = a[t], y = a[u];
          if (x > y) a[t] = y, a[u] = x;
        }
      }
      __syncthreads();
    }
  }
}

struct PairArgs {
  double theta0, inv1, inv2;   // inv = 2 sigma^2, the divisor of the exponent
  long long M;
  int N;
};

// pair number k = 0 .. N(N-1)/2 - 1, rows i = 0, 1, ... in turn: row i holds the pairs (i, i+1) .. (i, N-1)
__device__ inline void pair_of(long long k, int N, int* pi, int* pj) {
  const double b = 2.0 * N - 1.0;
  long long i = (long long)((b - sqrt(b * b - 8.0 * (double)k)) * 0.5);
  if (i < 0) i = 0;
  if (i > N - 2) i = N - 2;
  // first pair of row i: i N - i (i + 1) / 2
  while (i > 0 && i * N - i * (i + 1) / 2 > k) --i;
  while (i < N - 2 && (i + 1) * N - (i + 1) * (i + 2) / 2 <= k) ++i;
  *pi = (int)i;
  *pj = (int)(k - (i * N - i * (i + 1) / 2) + i + 1);
}

__global__ void __launch_bounds__(kVsThreads) pair_scores_kernel(const int* __restrict__ obs, const int* __restrict__ sorted,
                                                                  const long long* __restrict__ offsets,
                                                                  const double* __restrict__ points,
                                                                  const double* __restrict__ centres, PairArgs a,
                                                                  double* __restrict__ score) {
  __shared__ double wave_sum[kVsThreads / 64];
  int i, j;
  pair_of(blockIdx.x, a.N, &i, &j);
  const long long bi = offsets[i], ni = offsets[i + 1] - bi;
  const long long bj = offsets[j], nj = offsets[j + 1] - bj;
  const int* li = obs + bi;
  const int* lj = sorted + bj;
  const double ci[3] = {centres[3 * i], centres[3 * i + 1], centres[3 * i + 2]};
  const double cj[3] = {centres[3 * j], centres[3 * j + 1], centres[3 * j + 2]};
  double sum = 0.0;
  for (long long o = threadIdx.x; o < ni; o += kVsThreads) {
    const int p = li[o];
    if (p < 0 || (long long)p >= a.M) continue;
    long long lo = 0, hi = nj;             // the first position of lj that holds a value >= p
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (lj[mid] < p) lo = mid + 1; else hi = mid;
    }
    if (lo >= nj || lj[lo] != p) continue;
    const double* x = points + 3 * (long long)p;
    const double u0 = ci[0] - x[0], u1 = ci[1] - x[1], u2 = ci[2] - x[2];
    const double v0 = cj[0] - x[0], v1 = cj[1] - x[1], v2 = cj[2] - x[2];
    const double dot = (u0 * v0 + u1 * v1) + u2 * v2;
    const double nu = __dsqrt_rn((u0 * u0 + u1 * u1) + u2 * u2);
    const double nv = __dsqrt_rn((v0 * v0 + v1 * v1) + v2 * v2);
    double c = dot / nu / nv;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);       // (a NaN stays a NaN: both comparisons are false)
    const double theta = (180.0 / 3.141592653589793) * acos(c);
    const double d = theta - a.theta0;
    sum += exp(-d * d / (theta <= a.theta0 ? a.inv1 : a.inv2));
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) sum += __shfl_down(sum, s, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double total = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    score[(long long)i * a.N + j] = total;
    score[(long long)j * a.N + i] = total;
  }
}

}  // namespace

hipError_t launch_view_pair_scores(const long long* offsets_host, const int* obs, const double* points, long long M,
                                   const double* centres, int N, double theta0, double sigma1, double sigma2, double* score,
                                   long long* offsets_dev, int* sorted, hipStream_t s) {
  for (int first = 0; first <= N; first += kOffsetsPerLaunch) {
    OffsetChunk c;
    const int count = N + 1 - first < kOffsetsPerLaunch ? N + 1 - first : kOffsetsPerLaunch;
    for (int t = 0; t < kOffsetsPerLaunch; ++t) c.v[t] = t < count ? offsets_host[first + t] : 0;
    hipLaunchKernelGGL(offsets_upload_kernel, dim3((count + kVsThreads - 1) / kVsThreads), dim3(kVsThreads), 0, s, c, first, count,
                       offsets_dev);
  }
  hipError_t e = hipMemsetAsync(score, 0, (size_t)N * N * sizeof(double), s);
  if (e != hipSuccess) return e;
  const long long pairs = (long long)N * (N - 1) / 2;
  if (pairs > 0) {
    hipLaunchKernelGGL(sort_lists_kernel, dim3(N), dim3(kVsThreads), 0, s, obs, offsets_dev, sorted);
    const PairArgs a{theta0, 2.0 * (sigma1 * sigma1), 2.0 * (sigma2 * sigma2), M, N};
    hipLaunchKernelGGL(pair_scores_kernel, dim3((unsigned)pairs), dim3(kVsThreads), 0, s, obs, sorted, offsets_dev, points, centres, a,
                       score);
  }
  return hipGetLastError();
}

}  // namespace ufr
