// Cohort score normalisation on the device, gfx950 (S-norm and its adaptive top-N form, AS-norm).
//
// topk_stats_kernel: mean and population standard deviation of the K largest entries of every
// row of a score matrix, one 256-thread workgroup per row.  The K-th largest value v is found
// exactly by an MSB-first radix select over an order-preserving 32-bit key of the fp32 bits:
// four passes over the row, each a 256-bin histogram (LDS integer atomics, one histogram per wave)
// of the digit of the entries that match the prefix found so far, followed by a suffix scan that
// picks the bin the K-th largest falls into.  The last pass leaves v and the number of copies of v
// that belong to the K best, K - g with g the count of entries strictly above v; one more pass sums
// s and s^2 over the entries above v, and the copies of v are added as (K - g) v and (K - g) v^2.
// Which of several equal entries is "chosen" never enters, so ties across the cut cannot change
// the result.  Sums are fp64: per-thread partials in a fixed strided order, a fixed shuffle tree
// per wave, the four waves added in order.  No float atomics: the same input gives the same bits.
//
// cosine_trials_norm_kernel: the trial gather of affinity.hip with
//   score = 0.5 ((s - mu_a) / max(sd_a, 1e-6) + (s - mu_b) / max(sd_b, 1e-6))
// applied to the raw cosine s of the shared wave_pair_cosine (cosine_pair.h).
#include "cosine_pair.h"
#include "score_norm.h"

namespace spk {

namespace {

constexpr int NT = 256, NW = NT / 64;

// fp32 bits -> unsigned key with the order of the floats; -0.0 shares the key of +0.0
__device__ __forceinline__ unsigned order_key(float x) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__global__ void __launch_bounds__(NT)
topk_stats_kernel(const float* __restrict__ S, long long rows, long long cols, long long lds, int K,
                  float* __restrict__ mean, float* __restrict__ sd) {
  __shared__ unsigned hist[NW][256];
  __shared__ unsigned sel[2];          // the digit picked by a pass, and what is left of K below it
  __shared__ double part[NW][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* __restrict__ p = S + row * lds;
    unsigned prefix = 0;               // the digits found so far, in place
    unsigned krem = (unsigned)K;       // rank of the K-th largest among the entries matching prefix
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const unsigned himask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
      for (int b = tid; b < NW * 256; b += NT) (&hist[0][0])[b] = 0u;
      __syncthreads();
      for (long long c = tid; c < cols; c += NT) {
        const unsigned k = order_key(p[c]);
        if ((k & himask) == prefix) atomicAdd(&hist[wave][(k >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (wave == 0) {
        // lane l owns bins 4l .. 4l+3; inclusive suffix sum of the lanes' totals by shuffles
        unsigned h[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          h[b] = 0u;
#pragma unroll
          for (int w = 0; w < NW; ++w) h[b] += hist[w][4 * lane + b];
        }
        const unsigned tot = h[0] + h[1] + h[2] + h[3];
        unsigned incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned y = __shfl_down(incl, o, 64);
          if (lane + o < 64) incl += y;
        }
        unsigned above = incl - tot;   // entries in bins above this lane's
#pragma unroll
        for (int b = 3; b >= 0; --b) {
          if (above < krem && krem <= above + h[b]) {   // true for exactly one bin of one lane
            sel[0] = (unsigned)(4 * lane + b);
            sel[1] = krem - above;
          }
          above += h[b];
        }
      }
      __syncthreads();
      prefix |= sel[0] << shift;
      krem = sel[1];
      // the next pass's zeroing of hist and sel's next write are both behind a barrier that
      // every thread reaches only after reading sel here
    }
    // prefix is the key of v; krem = K - g copies of v are among the K best
    const float v = key_value(prefix);
    double s1 = 0.0, s2 = 0.0;
    for (long long c = tid; c < cols; c += NT) {
      const float x = p[c];
      if (order_key(x) > prefix) {
        const double d = (double)x;
        s1 += d;
        s2 += d * d;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    if (lane == 0) { part[wave][0] = s1; part[wave][1] = s2; }
    __syncthreads();
    if (tid == 0) {
      double t1 = 0.0, t2 = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) { t1 += part[w][0]; t2 += part[w][1]; }
      const double dv = (double)v, n = (double)krem;
      t1 += n * dv;
      t2 += n * (dv * dv);
      const double m = t1 / (double)K;
      const double var = t2 / (double)K - m * m;
      mean[row] = (float)m;
      sd[row] = (float)sqrt(var > 0.0 ? var : 0.0);
    }
    __syncthreads();   // part and sel are reused by the block's next row
  }
}

__global__ void __launch_bounds__(256)
cosine_trials_norm_kernel(const float* __restrict__ A, const float* __restrict__ Bm, int E,
                          const long long* __restrict__ ia, const long long* __restrict__ ib, long long T,
                          const float* __restrict__ mean_a, const float* __restrict__ std_a,
                          const float* __restrict__ mean_b, const float* __restrict__ std_b, float* __restrict__ out) {
  const long long tr = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (tr >= T) return;
  const long long a = ia[tr], b = ib[tr];
  const float s = wave_pair_cosine(A + a * E, Bm + b * E, E, lane);
  if (lane == 0) {
    const float za = (s - mean_a[a]) / fmaxf(std_a[a], 1e-6f);
    const float zb = (s - mean_b[b]) / fmaxf(std_b[b], 1e-6f);
    out[tr] = 0.5f * (za + zb);
  }
}

}  // namespace

hipError_t launch_topk_stats(const float* S, int64_t rows, int64_t cols, int64_t lds, int K, float* mean, float* std,
                             hipStream_t s) {
  if (rows < 1 || cols < 1 || lds < cols || K < 1 || K > cols) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)(rows < (1 << 20) ? rows : (1 << 20));   // further rows by grid stride
  hipLaunchKernelGGL(topk_stats_kernel, dim3(grid), dim3(NT), 0, s, S, (long long)rows, (long long)cols,
                     (long long)lds, K, mean, std);
  return hipGetLastError();
}

hipError_t launch_cosine_trials_norm(const float* A, const float* B, int E, const long long* ia, const long long* ib,
                                     long long T, const float* mean_a, const float* std_a, const float* mean_b,
                                     const float* std_b, float* out, hipStream_t s) {
  if (E <= 0 || E % 4 || T < 0) return hipErrorInvalidValue;
  if (T == 0) return hipSuccess;
  if ((T + 3) / 4 > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cosine_trials_norm_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, A, B, E, ia, ib, T,
                     mean_a, std_a, mean_b, std_b, out);
  return hipGetLastError();
}

}  // namespace spk
