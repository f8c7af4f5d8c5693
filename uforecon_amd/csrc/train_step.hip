// What a training step runs around the ray path, as launches of its own instead of many small library ones:
//
//   adam_kernel        torch.optim.Adam's update (defaults: no weight decay, no amsgrad, no maximize) for up to kAdamTableCap
//                      tensors in ONE launch.  The table of tensors travels BY VALUE in the kernel arguments (48 B per tensor,
//                      3 KiB of the 4 KiB a launch may carry): no staging buffer, no copy to wait for, nothing that a later
//                      call could overwrite while this one is still queued.  The grid is balanced over ELEMENTS: every block
//                      owns one chunk of kAdamChunk elements of one tensor, the table holds each tensor's first chunk, a
//                      block finds its tensor by bisection over that column (wave-uniform reads of the argument segment).
//                      Nothing is assumed about the pointers' alignment beyond 4 bytes: a tensor whose four pointers are all
//                      16-byte aligned runs 4 elements per lane and access (a chunk starts a multiple of 16 bytes into it),
//                      every other one 1 -- the gradients of cost_reg_2 are slices of one flat buffer at arbitrary offsets.
//
//   select_rays        the first k entries of the stable ascending argsort of n keys -- argsort(rand(H W))[:k] with ties
//                      broken by the smaller index.  The keys are the floats' BIT PATTERNS compared as unsigned integers, which
//                      for non-negative, non-NaN floats is the floats' order; any other pattern is still a key like the rest,
//                      so the output is k distinct in-range indices whatever the input holds.
//                        select   three digit passes (11 / 11 / 10 bits from the top): a histogram of the digit over the
//                                 keys that share the digits found so far (LDS counters per block, added to the global
//                                 counters with integer atomics -- integer sums, the same whichever block comes first), then
//                                 one block that scans the 2048 counters and picks the digit holding the k-th smallest.  After
//                                 the third pass: the k-th smallest key t, the number of keys below t, and how many keys equal
//                                 to t the result still needs.
//                        compact  compact.h, one key per thread: every key < t, and the first `needed` keys == t in index
//                                 order, each as (key << 32 | index).
//                        sort     one block sorts the k pairs in LDS (bitonic over the next power of two, padded with all-ones)
//                                 and stores the indices: the pair's order IS (value, then index).
//                      No float atomics, no dependence on which block runs when: a rerun gives the same bits.
#include "compact.h"
#include "ufr_internal.h"

namespace ufr {

// ------------------------------------------------------------------------------------------------------------ Adam
struct AdamEntry {
  float* p;
  const float* g;
  float* m;
  float* v;
  uint32_t n;        // elements
  uint32_t chunk0;   // the tensor's first chunk = first block
  float step;        // lr / bias_correction1
  float bc2_sqrt;    // sqrt(bias_correction2)
};
struct AdamTable {
  AdamEntry e[kAdamTableCap];
};
static_assert(sizeof(AdamTable) + 64 <= 4096, "the table must fit a launch's argument segment");

constexpr int kAdamThreads = 256;
constexpr uint32_t kAdamChunk = 4096;   // elements per block: 4 float4 per lane, or 16 scalars

__device__ inline void adam_update(float& p, float g, float& m, float& v, float w1, float beta2, float w2, float eps, float step,
                                   float bc2_sqrt) {
  m = m + w1 * (g - m);                 // exp_avg.lerp_(grad, 1 - beta1)
  v = v * beta2 + w2 * g * g;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = p - step * (m / denom);           // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ void __launch_bounds__(kAdamThreads) adam_kernel(const AdamTable T, int nt, float w1, float beta2, float w2, float eps) {
  const uint32_t b = blockIdx.x;
  int lo = 0, hi = nt - 1;              // the last tensor whose first chunk is <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T.e[mid].chunk0 <= b) lo = mid; else hi = mid - 1;
  }
  const AdamEntry e = T.e[lo];
  const uint32_t i0 = (b - e.chunk0) * kAdamChunk;
  if (i0 >= e.n) return;                // (cannot happen for a table the launcher built)
  const uint32_t cnt = min(kAdamChunk, e.n - i0);
  float* p = e.p + i0;
  const float* g = e.g + i0;
  float* m = e.m + i0;
  float* v = e.v + i0;
  const bool wide = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                      reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
  uint32_t done = 0;
  if (wide) {
    const uint32_t n4 = cnt >> 2;
    for (uint32_t q = threadIdx.x; q < n4; q += kAdamThreads) {
      float4 P = reinterpret_cast<float4*>(p)[q], M = reinterpret_cast<float4*>(m)[q], V = reinterpret_cast<float4*>(v)[q];
      const float4 G = reinterpret_cast<const float4*>(g)[q];
      adam_update(P.x, G.x, M.x, V.x, w1, beta2, w2, eps, e.step, e.bc2_sqrt);
      adam_update(P.y, G.y, M.y, V.y, w1, beta2, w2, eps, e.step, e.bc2_sqrt);
      adam_update(P.z, G.z, M.z, V.z, w1, beta2, w2, eps, e.step, e.bc2_sqrt);
      adam_update(P.w, G.w, M.w, V.w, w1, beta2, w2, eps, e.step, e.bc2_sqrt);
      reinterpret_cast<float4*>(p)[q] = P;
      reinterpret_cast<float4*>(m)[q] = M;
      reinterpret_cast<float4*>(v)[q] = V;
    }
    done = n4 << 2;                     // the tail (a tensor's last chunk only) one element per lane
  }
  for (uint32_t i = done + threadIdx.x; i < cnt; i += kAdamThreads) {
    float P = p[i], M = m[i], V = v[i];
    adam_update(P, g[i], M, V, w1, beta2, w2, eps, e.step, e.bc2_sqrt);
    p[i] = P;
    m[i] = M;
    v[i] = V;
  }
}

hipError_t launch_adam(const ufr_adam_tensor* t, int nt, double lr, double beta1, double beta2, double eps, hipStream_t s) {
  AdamTable T{};
  uint32_t chunks = 0;
  int k = 0;
  for (int i = 0; i < nt; ++i) {
    if (t[i].numel <= 0) continue;      // (an empty tensor owns no block)
    AdamEntry& e = T.e[k++];
    e.p = t[i].param;
    e.g = t[i].grad;
    e.m = t[i].exp_avg;
    e.v = t[i].exp_avg_sq;
    e.n = (uint32_t)t[i].numel;
    e.chunk0 = chunks;
    e.step = (float)(lr / t[i].bias_correction1);
    e.bc2_sqrt = (float)sqrt(t[i].bias_correction2);
    chunks += (e.n + kAdamChunk - 1) / kAdamChunk;
  }
  if (k == 0) return hipSuccess;
  hipLaunchKernelGGL(adam_kernel, dim3(chunks), dim3(kAdamThreads), 0, s, T, k, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------ select_rays
constexpr int kSelBins = 2048;
constexpr int kSelHistThreads = 256;
constexpr int kSelHistItems = 8;          // keys per thread and block before the grid-stride loop takes over
constexpr int kSelHistMaxBlocks = 2048;
constexpr int kSelCompactThreads = 1024;  // one key per thread
constexpr int kSelSortThreads = 1024;

// pass 0 / 1 / 2: the digit's shift and its width
__host__ __device__ constexpr int sel_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr int sel_bits(int pass) { return pass == 2 ? 10 : 11; }
// does key u share the digits found before this pass (`found`: state[0])?
template <int kPass>
__device__ inline bool sel_match(uint32_t u, uint32_t found) {
  if constexpr (kPass == 0) return true;
  else return (u >> (kPass == 1 ? 21 : 10)) == (found >> (kPass == 1 ? 21 : 10));
}

// state[0]: the digits found so far (a key's top bits), [1]: how many keys the result still needs among those that share
// them, [2]: the number of keys below every such key
template <int kPass>
__global__ void __launch_bounds__(kSelHistThreads) select_hist_kernel(const uint32_t* __restrict__ key, int n,
                                                                       const uint32_t* __restrict__ state, uint32_t* __restrict__ hist) {
  __shared__ uint32_t sh[kSelBins];
  for (int i = threadIdx.x; i < kSelBins; i += kSelHistThreads) sh[i] = 0;
  __syncthreads();
  const uint32_t found = kPass == 0 ? 0u : state[0];
  for (long long i = (long long)blockIdx.x * kSelHistThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kSelHistThreads) {
    const uint32_t u = key[i];
    if (sel_match<kPass>(u, found)) atomicAdd(&sh[(u >> sel_shift(kPass)) & ((1u << sel_bits(kPass)) - 1u)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSelBins; i += kSelHistThreads)
    if (sh[i]) atomicAdd(&hist[kPass * kSelBins + i], sh[i]);
}

// one block: the digit whose counter holds the k-th smallest of the keys counted
template <int kPass>
__global__ void __launch_bounds__(kScanThreads) select_pick_kernel(const uint32_t* __restrict__ hist, uint32_t k, uint32_t* __restrict__ state) {
  static_assert(kSelBins == 2 * kScanThreads, "two counters per thread");
  __shared__ uint32_t lds[kScanThreads / 64];
  const uint32_t need = kPass == 0 ? k : state[1], below = kPass == 0 ? 0u : state[2], prefix = kPass == 0 ? 0u : state[0];
  const uint32_t c0 = hist[kPass * kSelBins + 2 * threadIdx.x], c1 = hist[kPass * kSelBins + 2 * threadIdx.x + 1];
  uint32_t total;
  const uint32_t ex = block_scan_excl<uint32_t, kScanThreads>(c0 + c1, lds, &total);   // (ends with a barrier: every thread has read the state)
  // exactly one counter has  keys before it < need <= keys before it + its own  (1 <= need <= total)
  if (ex < need && need <= ex + c0) {
    state[0] = prefix | ((uint32_t)(2 * threadIdx.x) << sel_shift(kPass));
    state[1] = need - ex;
    state[2] = below + ex;
  } else if (ex + c0 < need && need <= ex + c0 + c1) {
    state[0] = prefix | ((uint32_t)(2 * threadIdx.x + 1) << sel_shift(kPass));
    state[1] = need - (ex + c0);
    state[2] = below + ex + c0;
  }
}

// compact.h's count and emit steps: column 0 the keys < t, column 1 the keys == t
template <bool kEmit>
__global__ void __launch_bounds__(kSelCompactThreads) select_compact_kernel(const uint32_t* __restrict__ key, int n,
                                                                             const uint32_t* __restrict__ state, int* __restrict__ totals,
                                                                             const long long* __restrict__ off, int k,
                                                                             unsigned long long* __restrict__ cand) {
  __shared__ int la[kSelCompactThreads / 64], lb[kSelCompactThreads / 64];
  const long long i = (long long)blockIdx.x * kSelCompactThreads + threadIdx.x;
  const uint32_t t = state[0];
  const uint32_t u = i < n ? key[i] : 0u;
  const bool lt = i < n && u < t, eq = i < n && u == t;
  int n_lt, n_eq;
  const int r_lt = block_rank<kSelCompactThreads>(lt, la, &n_lt);
  const int r_eq = block_rank<kSelCompactThreads>(eq, lb, &n_eq);
  if (!kEmit) {
    if (threadIdx.x == 0) {
      totals[2 * blockIdx.x] = n_lt;
      totals[2 * blockIdx.x + 1] = n_eq;
    }
    return;
  }
  const long long below = state[2], needed = state[1];
  long long slot = -1;
  if (lt) slot = off[2 * blockIdx.x] + r_lt;
  if (eq && off[2 * blockIdx.x + 1] + r_eq < needed) slot = below + off[2 * blockIdx.x + 1] + r_eq;
  if (slot >= 0 && slot < k) cand[slot] = ((unsigned long long)u << 32) | (unsigned long long)i;   // (slot < k by construction)
}

// one block: the k pairs in order, their indices out
__global__ void __launch_bounds__(kSelSortThreads) select_sort_kernel(const unsigned long long* __restrict__ cand, int k, int P,
                                                                      long long* __restrict__ idx_out) {
  __shared__ unsigned long long a[kSelectMaxK];
  for (int i = threadIdx.x; i < P; i += kSelSortThreads) a[i] = i < k ? cand[i] : ~0ull;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int q = threadIdx.x; q < (P >> 1); q += kSelSortThreads) {
        const int lo = ((q & ~(stride - 1)) << 1) | (q & (stride - 1)), hi = lo + stride;   // lo has bit `stride` clear
        const bool up = (lo & size) == 0;
        const unsigned long long x = a[lo], y = a[hi];
        if ((x > y) == up) {
          a[lo] = y;
          a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < k; i += kSelSortThreads) idx_out[i] = (long long)(a[i] & 0xffffffffull);
}

int select_compact_blocks(int n) { return (n + kSelCompactThreads - 1) / kSelCompactThreads; }

hipError_t launch_select_rays(const float* u, int n, int k, long long* idx_out, const SelectWorkspace& w, hipStream_t s) {
  const uint32_t* key = reinterpret_cast<const uint32_t*>(u);
  hipError_t e = hipMemsetAsync(w.hist, 0, (3 * kSelBins + 4) * sizeof(uint32_t), s);   // the counters and the state behind them
  if (e != hipSuccess) return e;
  uint32_t* state = w.hist + 3 * kSelBins;
  const int hb = min(kSelHistMaxBlocks, (n + kSelHistThreads * kSelHistItems - 1) / (kSelHistThreads * kSelHistItems));
  hipLaunchKernelGGL(select_hist_kernel<0>, dim3(hb), dim3(kSelHistThreads), 0, s, key, n, state, w.hist);
  hipLaunchKernelGGL(select_pick_kernel<0>, dim3(1), dim3(kScanThreads), 0, s, w.hist, (uint32_t)k, state);
  hipLaunchKernelGGL(select_hist_kernel<1>, dim3(hb), dim3(kSelHistThreads), 0, s, key, n, state, w.hist);
  hipLaunchKernelGGL(select_pick_kernel<1>, dim3(1), dim3(kScanThreads), 0, s, w.hist, (uint32_t)k, state);
  hipLaunchKernelGGL(select_hist_kernel<2>, dim3(hb), dim3(kSelHistThreads), 0, s, key, n, state, w.hist);
  hipLaunchKernelGGL(select_pick_kernel<2>, dim3(1), dim3(kScanThreads), 0, s, w.hist, (uint32_t)k, state);
  const int cb = select_compact_blocks(n);
  hipLaunchKernelGGL(select_compact_kernel<false>, dim3(cb), dim3(kSelCompactThreads), 0, s, key, n, state, w.totals, w.off, k, w.cand);
  e = launch_scan_totals<2, int>(w.totals, cb, w.off, w.grand, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(select_compact_kernel<true>, dim3(cb), dim3(kSelCompactThreads), 0, s, key, n, state, w.totals, w.off, k, w.cand);
  int P = 1;
  while (P < k) P <<= 1;
  hipLaunchKernelGGL(select_sort_kernel, dim3(1), dim3(kSelSortThreads), 0, s, w.cand, k, P, idx_out);
  return hipGetLastError();
}

}  // namespace ufr
