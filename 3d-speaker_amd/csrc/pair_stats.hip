// Pair-cosine statistics of a ragged batch of embedding groups, gfx950: the device side of the
// single-speaker check (speakerlab/bin/check_single_speaker.py), where a group is the segment
// embeddings of one file and the statistics are the minimum and the mean of all its pair cosines.
//
// pair_cosine_kernel: one wave per pair, a launch covering a range of at most kPairLaunchMax of
// the batch's pairs (the grid is a 32-bit count of work-items).  A wave's global pair index is located in the batch's
// prefix sums (kernel arguments, at most kPairChunk groups: a binary search on wave-uniform
// values), mapped to (i, j) inside its group and scored by wave_pair_cosine (cosine_pair.h), the
// device function behind spk_cosine_trials: the same bits for the same two rows.  The condensed
// array is written in np.triu_indices(n, 1) order.
//
// pair_stats_kernel: one kPairThreads workgroup per group.  <true> reads the group's condensed
// cosines; <false> (no cosine array was asked for) scores the pairs itself, wave w taking pairs
// [64 w, 64 w + 64) of every kPairThreads-pair block one after the other and lane l keeping the
// l-th: thread t then holds pairs t, t + kPairThreads, ... exactly as in <true>, so both forms add
// the same fp32 values in the same order.  Per thread: an fp64 sum in ascending pair order, the
// first minimum, the count below the threshold.  Per wave a fixed xor butterfly (an fp64 add
// commutes, so every lane ends with the same bits), then thread 0 adds the waves in order.  The
// minimum keeps the smallest condensed index among equal values; a NaN cosine (a non-finite row)
// orders below every number, so min is NaN, argmin the first NaN and the mean NaN, as numpy's min,
// argmin and mean of the cosines.  Nothing depends on where the
// group sits in the batch, so a group's outputs have the same bits alone and in any batch.
#include <climits>

#include "cosine_pair.h"
#include "pair_stats.h"

namespace spk {

namespace {

constexpr int NT = kPairThreads, NW = NT / 64;

// first pair of row i of an n-row group in condensed order
__device__ __forceinline__ long long row_start(long long n, long long i) { return i * (2 * n - i - 1) / 2; }

// condensed index p in [0, n (n - 1) / 2) -> (i, j), i < j.  The fp64 root only proposes a row
// (its argument is at least 9 and below 2^33); the integer loops make it exact.
__device__ __forceinline__ void condensed_to_ij(int n, long long p, int& i, int& j) {
  const double b = 2.0 * (double)n - 1.0;
  long long r = (long long)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
  r = r < 0 ? 0 : (r > n - 2 ? n - 2 : r);
  while (r > 0 && row_start(n, r) > p) --r;
  while (r < n - 2 && row_start(n, r + 1) <= p) ++r;
  i = (int)r;
  j = (int)(p - row_start(n, r)) + i + 1;
}

__global__ void __launch_bounds__(256)
pair_cosine_kernel(const PairBatchArgs a, long long q0, long long q1, const float* __restrict__ X, long long ldx, int E,
                   float* __restrict__ cos) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const long long q = q0 + (long long)blockIdx.x * 4 + wave;
  if (q >= q1) return;
  // the group holding q: the first k with pair0[k + 1] > q (groups without pairs are stepped over)
  int lo = 0, hi = a.ng - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.pair0[mid + 1] > q) hi = mid; else lo = mid + 1;
  }
  int i, j;
  condensed_to_ij(a.n[lo], q - a.pair0[lo], i, j);
  const float* __restrict__ Xg = X + a.row0[lo] * ldx;
  const float s = wave_pair_cosine(Xg + i * ldx, Xg + j * ldx, E, lane);
  if (lane == 0) cos[q] = s;
}

template <bool FROM_COS>
__global__ void __launch_bounds__(NT)
pair_stats_kernel(const PairBatchArgs a, const float* __restrict__ X, long long ldx, int E, float thr,
                  const float* __restrict__ cos, float* __restrict__ mn, float* __restrict__ mean,
                  long long* __restrict__ argmin, long long* __restrict__ n_below) {
  __shared__ double part_sum[NW];
  __shared__ float part_min[NW];
  __shared__ long long part_idx[NW], part_cnt[NW];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.n[g];
  const long long P = n > 1 ? (long long)n * (n - 1) / 2 : 0;
  if (P == 0) {
    // the reference's rule for fewer than two segments
    if (tid == 0) { mn[g] = 1.f; mean[g] = 1.f; argmin[g] = -1; n_below[g] = 0; }
    return;
  }
  double sum = 0.0;
  float best = INFINITY;
  long long idx = LLONG_MAX, cnt = 0;
  // a NaN orders below every number (numpy's min / argmin: the first NaN wins)
  auto take = [&](float v, long long p) {
    sum += (double)v;
    if (v < best || (v != v && best == best)) { best = v; idx = p; }
    cnt += v < thr ? 1 : 0;
  };
  // whether (ob, oi) comes before (b, bi): NaN first, then the smaller value, then the smaller index
  auto before = [](float ob, long long oi, float b, long long bi) {
    const bool on = ob != ob, bn = b != b;
    return on != bn ? on : ((on || ob == b) ? oi < bi : ob < b);
  };
  if (FROM_COS) {
    const float* __restrict__ c = cos + a.pair0[g];
    for (long long p = tid; p < P; p += NT) take(c[p], p);
  } else {
    const float* __restrict__ Xg = X + a.row0[g] * ldx;
    for (long long base = (long long)wave * 64; base < P; base += NT) {
      const int m = P - base < 64 ? (int)(P - base) : 64;
      int i, j;
      condensed_to_ij(n, base, i, j);
      float v = 0.f;
      for (int l = 0; l < m; ++l) {
        const float s = wave_pair_cosine(Xg + i * ldx, Xg + j * ldx, E, lane);
        if (lane == l) v = s;
        if (++j == n) { ++i; j = i + 1; }
      }
      if (lane < m) take(v, base + lane);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
    const float ob = __shfl_xor(best, o, 64);
    const long long oi = __shfl_xor(idx, o, 64);
    if (before(ob, oi, best, idx)) { best = ob; idx = oi; }
  }
  if (lane == 0) { part_sum[wave] = sum; part_min[wave] = best; part_idx[wave] = idx; part_cnt[wave] = cnt; }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    float b = INFINITY;
    long long bi = LLONG_MAX, c = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      t += part_sum[w];
      c += part_cnt[w];
      if (before(part_min[w], part_idx[w], b, bi)) { b = part_min[w]; bi = part_idx[w]; }
    }
    mn[g] = b;
    mean[g] = (float)(t / (double)P);
    argmin[g] = bi;
    n_below[g] = c;
  }
}

}  // namespace

hipError_t launch_pair_cosine(const PairBatchArgs& a, long long q0, long long q1, const float* X, long long ldx, int E,
                              float* cos, hipStream_t s) {
  if (a.ng < 1 || a.ng > kPairChunk || E <= 0 || E % 4 || ldx < E) return hipErrorInvalidValue;
  // [q0, q1) inside the batch's pairs, and a grid of at most 2^31 work-items
  if (q0 < a.pair0[0] || q1 > a.pair0[a.ng] || q1 < q0 || q1 - q0 > kPairLaunchMax) return hipErrorInvalidValue;
  if (q1 == q0) return hipSuccess;
  hipLaunchKernelGGL(pair_cosine_kernel, dim3((unsigned)((q1 - q0 + 3) / 4)), dim3(256), 0, s, a, q0, q1, X, ldx, E,
                     cos);
  return hipGetLastError();
}

hipError_t launch_pair_stats(const PairBatchArgs& a, const float* X, long long ldx, int E, float threshold,
                             const float* cos, float* mn, float* mean, long long* argmin, long long* n_below,
                             hipStream_t s) {
  if (a.ng < 1 || a.ng > kPairChunk || E <= 0 || E % 4 || ldx < E) return hipErrorInvalidValue;
  if (cos)
    hipLaunchKernelGGL(pair_stats_kernel<true>, dim3((unsigned)a.ng), dim3(NT), 0, s, a, X, ldx, E, threshold, cos, mn,
                       mean, argmin, n_below);
  else
    hipLaunchKernelGGL(pair_stats_kernel<false>, dim3((unsigned)a.ng), dim3(NT), 0, s, a, X, ldx, E, threshold, cos, mn,
                       mean, argmin, n_below);
  return hipGetLastError();
}

}  // namespace spk
