// Class-aware consumers of a row block of the N x N cosine matrix of one labelled embedding set,
// gfx950: what exact verification metrics over all pairs i < j need.  Pair (i, j) is a target pair
// (class 1) when labels[i] == labels[j], a non-target pair (class 0) otherwise.  As in sim_stats.hip
// the block is the caller's workspace, filled by the affinity kernel just before
// (verif_stats_abi.cpp), and every kernel takes one workgroup of 256 threads per row of the block
// over the columns j > i, so the reads hit the block while it is still in the Infinity Cache.
//
// Everything the metrics rest on is an integer: scores are compared through the order-preserving
// 32-bit key of sim_stats.h (-0.0 shares the key of +0.0), counts are u32 atomics in LDS, flushed
// once per row as u64 atomics (exact in any order).  No float atomics.
//
// fp64 sums.  A row's sum of a class: thread t of 256 adds its columns i + 1 + t, i + 1 + t + 256, ...
// of that class in ascending order, a wave adds its lanes by a fixed xor butterfly, thread 0 adds
// the four waves in order.  A class's total: thread t of 1024 adds the rows' sums t, t + 1024, ... in
// ascending order, the same butterfly per wave, thread 0 adds the sixteen waves in order.  Neither
// depends on how the rows were cut into blocks, so every workspace size gives the same bits.
//
// LDS per workgroup: verif_moments_kernel 2 KiB of edges + 2 KiB of bins + 200 B;
// verif_digits_kernel, dynamic: level 0 16 KiB (8 copies of 2 x 256 bins, so that the few exponent
// bins scores share do not serialise a wave), level L >= 1 2 KiB per prefix (2 x 256 bins) + 4 KiB
// of prefix tables per level, at most 32 + 12 KiB with 16 prefixes at level 3.  One prefix (the EER
// search) leaves the kernel bound by its waves per CU, sixteen at level 3 hold three workgroups per CU.
#include "verif_stats.h"

namespace spk {

namespace {

constexpr int NT = kSimThreads, NW = NT / 64;
constexpr int UNR = 4;             // columns a thread loads before it consumes them
constexpr int REP0 = 8;            // copies of the level-0 histogram

__device__ __forceinline__ unsigned order_key(float x) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned y = __shfl_xor(v, o, 64); v = y < v ? y : v; }
  return v;
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned y = __shfl_xor(v, o, 64); v = y > v ? y : v; }
  return v;
}

// state sections (verif_stats.h)
struct VerifPtrs {
  double* row_sum;
  double* row_sumsq;
  double* total;
  unsigned long long* count;
  unsigned* minmax;
  const double* edges;
  unsigned long long* hist;
  unsigned long long* digits;
  const signed char* lut;
  int* flag;
  long long npad;
};

__global__ void __launch_bounds__(1024) verif_label_min_kernel(const int* __restrict__ labels, long long N, VerifPtrs st) {
  int m = 0x7FFFFFFF;
  for (long long r = (long long)blockIdx.x * 1024 + threadIdx.x; r < N; r += (long long)gridDim.x * 1024) {
    const int l = labels[r];
    m = l < m ? l : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_xor(m, o, 64); m = y < m ? y : m; }
  if ((threadIdx.x & 63) == 0) atomicMin(&st.flag[0], m);
}

// ------------------------------------------------------------------------------ moments + histogram
__global__ void __launch_bounds__(NT)
verif_moments_kernel(const float* __restrict__ S, const int* __restrict__ labels, long long r0, long long N, int nbins,
                     VerifPtrs st) {
  __shared__ double edges[kSimMaxBins + 1];
  __shared__ unsigned fh[2][kSimMaxBins];
  __shared__ double part[NW][4];
  __shared__ unsigned pmm[NW][4];
  __shared__ unsigned pcnt[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = r0 + blockIdx.x;
  const float* __restrict__ p = S + (long long)blockIdx.x * N;
  const int li = labels[i];
  for (int b = tid; b <= nbins && nbins > 0; b += NT) edges[b] = st.edges[b];
  for (int b = tid; b < 2 * kSimMaxBins; b += NT) (&fh[0][0])[b] = 0u;
  __syncthreads();
  const double e0 = nbins > 0 ? edges[0] : 0.0, e1 = nbins > 0 ? edges[nbins] : 0.0;
  const double inv = e1 > e0 ? (double)nbins / (e1 - e0) : 0.0;
  double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
  unsigned kmin[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, kmax[2] = {0u, 0u};
  unsigned ntgt = 0u;                            // the row's target pairs seen by this thread
  for (long long c0 = i + 1 + tid; c0 < N; c0 += (long long)UNR * NT) {
    float x[UNR];
    int l[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long long c = c0 + (long long)u * NT;
      x[u] = c < N ? p[c] : 0.f;
      l[u] = c < N ? labels[c] : -1;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (c0 + (long long)u * NT >= N) break;
      const int cls = l[u] == li ? 1 : 0;
      const double d = (double)x[u];
      const unsigned key = order_key(x[u]);
      ntgt += (unsigned)cls;
      // both classes' accumulators are touched with a select, never indexed at run time
      s1[0] += cls ? 0.0 : d;
      s1[1] += cls ? d : 0.0;
      s2[0] += cls ? 0.0 : d * d;
      s2[1] += cls ? d * d : 0.0;
      if (cls) {
        kmin[1] = key < kmin[1] ? key : kmin[1];
        kmax[1] = key > kmax[1] ? key : kmax[1];
      } else {
        kmin[0] = key < kmin[0] ? key : kmin[0];
        kmax[0] = key > kmax[0] ? key : kmax[0];
      }
      if (nbins > 0 && d >= e0 && d <= e1) {
        // an arithmetic estimate, then corrected against the edges (spk_cosine_triu_hist's bins)
        int b = (int)((d - e0) * inv);
        b = b < 0 ? 0 : (b > nbins - 1 ? nbins - 1 : b);
        while (b > 0 && d < edges[b]) --b;
        while (b < nbins - 1 && d >= edges[b + 1]) ++b;
        atomicAdd(&fh[cls][b], 1u);
      }
    }
  }
  // adding 0.0 leaves a sum's bits alone (x + 0.0 == x, and -0.0 never arises from +0.0 starts), so
  // each class's sum is the sum of its own columns in ascending order
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    s1[c] = wave_sum(s1[c]);
    s2[c] = wave_sum(s2[c]);
    kmin[c] = wave_min(kmin[c]);
    kmax[c] = wave_max(kmax[c]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ntgt += __shfl_xor(ntgt, o, 64);
  if (lane == 0) {
    part[wave][0] = s1[0]; part[wave][1] = s1[1]; part[wave][2] = s2[0]; part[wave][3] = s2[1];
    pmm[wave][0] = kmin[0]; pmm[wave][1] = kmin[1]; pmm[wave][2] = kmax[0]; pmm[wave][3] = kmax[1];
    pcnt[wave] = ntgt;
  }
  __syncthreads();
  for (int b = tid; b < 2 * nbins; b += NT) {
    const int c = b / nbins, q = b - c * nbins;
    if (fh[c][q]) atomicAdd(&st.hist[c * kSimMaxBins + q], (unsigned long long)fh[c][q]);
  }
  if (tid == 0) {
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned a[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, b[2] = {0u, 0u};
    unsigned long long n1 = 0ull;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] += part[w][q];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        a[c] = pmm[w][c] < a[c] ? pmm[w][c] : a[c];
        b[c] = pmm[w][2 + c] > b[c] ? pmm[w][2 + c] : b[c];
      }
      n1 += pcnt[w];
    }
    st.row_sum[i] = t[0];
    st.row_sum[st.npad + i] = t[1];
    st.row_sumsq[i] = t[2];
    st.row_sumsq[st.npad + i] = t[3];
    const unsigned long long n0 = (unsigned long long)(N - 1 - i) - n1;
    if (n0) {
      atomicAdd(&st.count[0], n0);
      atomicMin(&st.minmax[0], a[0]);
      atomicMax(&st.minmax[2], b[0]);
    }
    if (n1) {
      atomicAdd(&st.count[1], n1);
      atomicMin(&st.minmax[1], a[1]);
      atomicMax(&st.minmax[3], b[1]);
    }
  }
}

__global__ void __launch_bounds__(1024) verif_total_kernel(long long N, VerifPtrs st) {
  __shared__ double part[16][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long r = tid; r < N; r += 1024) {
    s[0] += st.row_sum[r];
    s[1] += st.row_sum[st.npad + r];
    s[2] += st.row_sumsq[r];
    s[3] += st.row_sumsq[st.npad + r];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = wave_sum(s[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) part[wave][q] = s[q];
  }
  __syncthreads();
  if (tid < 4) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += part[w][tid];
    st.total[tid] = t;
  }
}

// ------------------------------------------------------------------------------ digit histograms
// Dynamic LDS: the histograms (LEVEL 0: [2][256][REP0]; else [n_slots][2][256]) u32, then LEVEL tables
// of kVerifMaxPrefixes x 256 signed bytes.
template <int LEVEL>
__global__ void __launch_bounds__(NT)
verif_digits_kernel(const float* __restrict__ S, const int* __restrict__ labels, long long r0, long long N, int n_slots,
                    VerifPtrs st) {
  extern __shared__ unsigned dyn[];
  const int nh = LEVEL == 0 ? 2 * 256 * REP0 : n_slots * 512;
  unsigned* hist = dyn;
  const signed char* lut = reinterpret_cast<const signed char*>(dyn + nh);
  const int tid = threadIdx.x, lane = tid & 63;
  const long long i = r0 + blockIdx.x;
  const float* __restrict__ p = S + (long long)blockIdx.x * N;
  const int li = labels[i];
  for (int b = tid; b < nh; b += NT) hist[b] = 0u;
  if constexpr (LEVEL > 0) {
    // whole words: the tables are LEVEL * 4 KiB, the section is 16-byte aligned
    const unsigned* src = reinterpret_cast<const unsigned*>(st.lut);
    unsigned* dst = dyn + nh;
    for (int b = tid; b < LEVEL * kVerifMaxPrefixes * 64; b += NT) dst[b] = src[b];
  }
  __syncthreads();
  for (long long c0 = i + 1 + tid; c0 < N; c0 += (long long)UNR * NT) {
    float x[UNR];
    int l[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long long c = c0 + (long long)u * NT;
      x[u] = c < N ? p[c] : 0.f;
      l[u] = c < N ? labels[c] : -1;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (c0 + (long long)u * NT >= N) break;
      const int cls = l[u] == li ? 1 : 0;
      const unsigned key = order_key(x[u]);
      if constexpr (LEVEL == 0) {
        atomicAdd(&hist[(cls * 256 + (int)(key >> 24)) * REP0 + (lane & (REP0 - 1))], 1u);
      } else {
        int sl = lut[key >> 24];
        if constexpr (LEVEL >= 2) if (sl >= 0) sl = lut[(kVerifMaxPrefixes + sl) * 256 + ((key >> 16) & 255u)];
        if constexpr (LEVEL >= 3) if (sl >= 0) sl = lut[(2 * kVerifMaxPrefixes + sl) * 256 + ((key >> 8) & 255u)];
        if (sl >= 0) atomicAdd(&hist[(sl * 2 + cls) * 256 + (int)((key >> (24 - 8 * LEVEL)) & 255u)], 1u);
      }
    }
  }
  __syncthreads();
  if constexpr (LEVEL == 0) {
    for (int b = tid; b < 512; b += NT) {
      unsigned h = 0u;
#pragma unroll
      for (int r = 0; r < REP0; ++r) h += hist[b * REP0 + r];
      if (h) atomicAdd(&st.digits[b], (unsigned long long)h);
    }
  } else {
    for (int b = tid; b < nh; b += NT)
      if (hist[b]) atomicAdd(&st.digits[b], (unsigned long long)hist[b]);
  }
}

VerifPtrs verif_ptrs(void* state, long long N) {
  const VerifState l = verif_state_layout(N);
  char* b = static_cast<char*>(state);
  VerifPtrs p;
  p.row_sum = reinterpret_cast<double*>(b + l.row_sum);
  p.row_sumsq = reinterpret_cast<double*>(b + l.row_sumsq);
  p.total = reinterpret_cast<double*>(b + l.total);
  p.count = reinterpret_cast<unsigned long long*>(b + l.count);
  p.minmax = reinterpret_cast<unsigned*>(b + l.minmax);
  p.edges = reinterpret_cast<const double*>(b + l.edges);
  p.hist = reinterpret_cast<unsigned long long*>(b + l.hist);
  p.digits = reinterpret_cast<unsigned long long*>(b + l.digits);
  p.lut = reinterpret_cast<const signed char*>(b + l.lut);
  p.flag = reinterpret_cast<int*>(b + l.flag);
  p.npad = l.npad;
  return p;
}

// a workgroup per row: rows * NT work-items, below 2^31 (sim_block_rows keeps a block there)
bool rows_fit(long long rows) { return rows >= 1 && rows * NT < kSimGridItems; }

}  // namespace

hipError_t launch_verif_label_min(const int* labels, long long N, void* state, hipStream_t s) {
  if (N < 1 || !labels) return hipErrorInvalidValue;
  long long blocks = (N + 1023) / 1024;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(verif_label_min_kernel, dim3((unsigned)blocks), dim3(1024), 0, s, labels, N, verif_ptrs(state, N));
  return hipGetLastError();
}

hipError_t launch_verif_moments(const float* S, const int* labels, long long r0, long long rows, long long N, int nbins,
                                void* state, hipStream_t s) {
  if (!rows_fit(rows) || r0 < 0 || r0 + rows > N || nbins < 0 || nbins > kSimMaxBins) return hipErrorInvalidValue;
  hipLaunchKernelGGL(verif_moments_kernel, dim3((unsigned)rows), dim3(NT), 0, s, S, labels, r0, N, nbins,
                     verif_ptrs(state, N));
  return hipGetLastError();
}

hipError_t launch_verif_total(long long N, void* state, hipStream_t s) {
  if (N < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(verif_total_kernel, dim3(1), dim3(1024), 0, s, N, verif_ptrs(state, N));
  return hipGetLastError();
}

hipError_t launch_verif_digits(const float* S, const int* labels, long long r0, long long rows, long long N, int level,
                               int n_slots, void* state, hipStream_t s) {
  if (!rows_fit(rows) || r0 < 0 || r0 + rows > N || level < 0 || level > 3 || n_slots < 1 ||
      n_slots > kVerifMaxPrefixes || (level == 0 && n_slots != 1))
    return hipErrorInvalidValue;
  const VerifPtrs st = verif_ptrs(state, N);
  const dim3 grid((unsigned)rows), block(NT);
  const size_t lds = level == 0 ? (size_t)2 * 256 * REP0 * 4
                                : (size_t)n_slots * 512 * 4 + (size_t)level * kVerifMaxPrefixes * 256;
  switch (level) {
    case 0: hipLaunchKernelGGL(verif_digits_kernel<0>, grid, block, lds, s, S, labels, r0, N, n_slots, st); break;
    case 1: hipLaunchKernelGGL(verif_digits_kernel<1>, grid, block, lds, s, S, labels, r0, N, n_slots, st); break;
    case 2: hipLaunchKernelGGL(verif_digits_kernel<2>, grid, block, lds, s, S, labels, r0, N, n_slots, st); break;
    default: hipLaunchKernelGGL(verif_digits_kernel<3>, grid, block, lds, s, S, labels, r0, N, n_slots, st); break;
  }
  return hipGetLastError();
}

}  // namespace spk
