// Consumers of a row block of the N x N cosine matrix of one embedding set, gfx950: per-row top-k
// with indices for k up to 1024, and the statistics of the upper triangle (moments, threshold
// counts, exact order statistics, a histogram over given edges, the extreme pairs).  The block is
// the caller's workspace, filled by the affinity kernel just before (sim_stats_abi.cpp); every
// kernel takes one workgroup of 256 threads per row of the block, so the reads hit the block while
// it is still in the Infinity Cache.
//
// Selection is exact and has no float atomics.  Scores are compared through the order-preserving
// 32-bit key of score_norm.hip (-0.0 shares the key of +0.0), counts are integer atomics (exact in
// any order), and wherever the choice among equal scores matters it is made by a workgroup prefix
// count in column order, never by the order threads arrive in.
//
// fp64 sums.  A row's sum: thread t of 256 adds its columns t, t + 256, ... (rows_topk: of all
// columns but the row's own; triangle: of the columns j > i, counted from i + 1) in ascending order,
// a wave adds its lanes by a fixed xor butterfly, thread 0 adds the four waves in order.  The
// triangle's total: thread t of 1024 adds the rows' sums t, t + 1024, ... in ascending order, the
// same butterfly per wave, thread 0 adds the sixteen waves in order.  Neither depends on how the
// rows were cut into blocks, so every workspace size gives the same bits.
//
// LDS per workgroup: rows_topk_kernel 4 KiB of digit histograms (one per wave) + 8 KiB of
// (key, column) pairs to sort + 100 B; triu_select_kernel 18 KiB of histograms (pass 0: 16 copies
// of the 256 bins, so that the few exponent bins scores share do not serialise a wave; later
// passes: 18 prefixes x 256 bins) + 13.5 KiB of prefix tables + 4.1 KiB of threshold buckets (32
// copies of 33) + 200 B; triu_final_kernel 2 KiB of edges + 1 KiB of bins + 100 B; triu_tie_kernel
// under 100 B.  All far below the 160 KiB of a CU, several workgroups per CU stay resident.
#include "sim_stats.h"

namespace spk {

namespace {

constexpr int NT = kSimThreads, NW = NT / 64;

__device__ __forceinline__ unsigned order_key(float x) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
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

// lanes below this one with the flag set, and the wave's total
__device__ __forceinline__ int wave_prefix(bool flag, int lane, int* total) {
  const unsigned long long b = __ballot(flag);
  *total = __popcll(b);
  return __popcll(b & ((1ull << lane) - 1ull));
}

// ------------------------------------------------------------------------------ rows: top-k + moments
__global__ void __launch_bounds__(NT)
rows_topk_kernel(const float* __restrict__ S, long long r0, long long N, int k, float* __restrict__ top_s,
                 long long* __restrict__ top_i, double* __restrict__ sum, double* __restrict__ sumsq,
                 float* __restrict__ mn, float* __restrict__ mx, float* __restrict__ self) {
  __shared__ unsigned hist[NW][256];
  __shared__ unsigned long long srt[kSimMaxK];   // (key << 32) | ~column: descending = score desc, column asc
  __shared__ unsigned sel[2];
  __shared__ double part[NW][2];
  __shared__ unsigned pmm[NW][2];
  __shared__ int wcnt[NW][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = r0 + blockIdx.x;
  const float* __restrict__ p = S + (long long)blockIdx.x * N;
  const long long M = N - 1;                     // the other columns

  // moments over the other columns
  double s1 = 0.0, s2 = 0.0;
  unsigned kmin = 0xFFFFFFFFu, kmax = 0u;
  for (long long c = tid; c < N; c += NT) {
    if (c == i) continue;
    const float x = p[c];
    const double d = (double)x;
    s1 += d;
    s2 += d * d;
    const unsigned key = order_key(x);
    kmin = key < kmin ? key : kmin;
    kmax = key > kmax ? key : kmax;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  kmin = wave_min(kmin);
  kmax = wave_max(kmax);
  if (lane == 0) { part[wave][0] = s1; part[wave][1] = s2; pmm[wave][0] = kmin; pmm[wave][1] = kmax; }
  __syncthreads();
  if (tid == 0) {
    double t1 = 0.0, t2 = 0.0;
    unsigned a = 0xFFFFFFFFu, b = 0u;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      t1 += part[w][0];
      t2 += part[w][1];
      a = pmm[w][0] < a ? pmm[w][0] : a;
      b = pmm[w][1] > b ? pmm[w][1] : b;
    }
    sum[i] = t1;
    sumsq[i] = t2;
    mn[i] = M > 0 ? key_value(a) : __uint_as_float(0x7FC00000u);
    mx[i] = M > 0 ? key_value(b) : __uint_as_float(0x7FC00000u);
    self[i] = p[i];
  }

  int L = 1;                                     // entries to sort: a power of two, at most kSimMaxK
  if (M <= (long long)k) {
    // everything is taken: the row is just sorted
    while (L < (int)M) L <<= 1;
    for (long long c = tid; c < N; c += NT) {
      if (c == i) continue;
      srt[c < i ? c : c - 1] = ((unsigned long long)order_key(p[c]) << 32) | (unsigned)~(unsigned)c;
    }
    for (int t = (int)M + tid; t < L; t += NT) srt[t] = 0ull;
  } else {
    while (L < k) L <<= 1;
    // the k-th largest key by an MSB-first radix select (score_norm.hip)
    unsigned prefix = 0, krem = (unsigned)k;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const unsigned himask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
      for (int b = tid; b < NW * 256; b += NT) (&hist[0][0])[b] = 0u;
      __syncthreads();
      for (long long c = tid; c < N; c += NT) {
        if (c == i) continue;
        const unsigned key = order_key(p[c]);
        if ((key & himask) == prefix) atomicAdd(&hist[wave][(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (wave == 0) {
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
        unsigned above = incl - tot;
#pragma unroll
        for (int b = 3; b >= 0; --b) {
          if (above < krem && krem <= above + h[b]) {
            sel[0] = (unsigned)(4 * lane + b);
            sel[1] = krem - above;
          }
          above += h[b];
        }
      }
      __syncthreads();
      prefix |= sel[0] << shift;
      krem = sel[1];
    }
    // prefix: the key of the cut; g = k - krem entries lie above it and krem copies of it are taken,
    // the first ones in column order.  Slots by a prefix count over the columns in order.
    const int g = k - (int)krem;
    int baseA = 0, baseT = 0;
    for (long long c0 = 0; c0 < N; c0 += NT) {
      const long long c = c0 + tid;
      const bool valid = c < N && c != i;
      const unsigned key = valid ? order_key(p[c]) : 0u;
      const bool isA = valid && key > prefix, isT = valid && key == prefix;
      int totA, totT;
      const int offA = wave_prefix(isA, lane, &totA), offT = wave_prefix(isT, lane, &totT);
      if (lane == 0) { wcnt[wave][0] = totA; wcnt[wave][1] = totT; }
      __syncthreads();
      int preA = 0, preT = 0, allA = 0, allT = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (w < wave) { preA += wcnt[w][0]; preT += wcnt[w][1]; }
        allA += wcnt[w][0];
        allT += wcnt[w][1];
      }
      const unsigned long long e = ((unsigned long long)key << 32) | (unsigned)~(unsigned)c;
      if (isA && baseA + preA + offA < g) srt[baseA + preA + offA] = e;   // always below g, by the select
      if (isT && baseT + preT + offT < (int)krem) srt[g + baseT + preT + offT] = e;
      baseA += allA;
      baseT = baseT + allT < (int)krem ? baseT + allT : (int)krem; // only "enough" matters: no overflow
      __syncthreads();
    }
    for (int t = k + tid; t < L; t += NT) srt[t] = 0ull;
  }
  // bitonic sort of L entries, descending
  for (int size = 2; size <= L; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < L / 2; t += NT) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const unsigned long long a = srt[lo], b = srt[hi];
        const bool desc = (lo & size) == 0;
        if ((a < b) == desc && a != b) { srt[lo] = b; srt[hi] = a; }
      }
    }
  __syncthreads();
  const long long have = M < (long long)k ? M : (long long)k;
  for (int t = tid; t < k; t += NT) {
    const unsigned long long e = t < have ? srt[t] : 0ull;
    top_s[i * k + t] = t < have ? key_value((unsigned)(e >> 32)) : __uint_as_float(0xFF800000u);
    top_i[i * k + t] = t < have ? (long long)(~(unsigned)e) : -1ll;
  }
}

// ------------------------------------------------------------------------------ triangle: select passes
// state sections (sim_stats.h)
struct TriuPtrs {
  double* row_sum;
  double* row_sumsq;
  double* total;
  unsigned long long* digit_hist;
  unsigned long long* count_le;
  unsigned* minmax;
  const signed char* lut;
  const float* thr;
  const double* edges;
  unsigned long long* hist;
  unsigned long long* counters;
  int* row_tie;
  unsigned* ext;
  long long npad;
};

template <int PASS>
__global__ void __launch_bounds__(NT)
triu_select_kernel(const float* __restrict__ S, long long r0, long long N, int n_thr, TriuPtrs st) {
  constexpr int REP = PASS == 0 ? 16 : 1;
  __shared__ unsigned hist[kSimMaxTargets * 256];
  __shared__ signed char lut[PASS == 0 ? 1 : PASS * kSimMaxTargets * 256];
  __shared__ unsigned cle[PASS == 0 ? (kSimMaxThr + 1) * 32 : 1];
  __shared__ float thr[kSimMaxThr];
  __shared__ double part[NW][2];
  __shared__ unsigned pmm[NW][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = r0 + blockIdx.x;
  const float* __restrict__ p = S + (long long)blockIdx.x * N;
  for (int b = tid; b < kSimMaxTargets * 256; b += NT) hist[b] = 0u;
  if constexpr (PASS == 0) {
    for (int b = tid; b < (kSimMaxThr + 1) * 32; b += NT) cle[b] = 0u;
    if (tid < kSimMaxThr) thr[tid] = tid < n_thr ? st.thr[tid] : 0.f;
  } else {
    for (int b = tid; b < PASS * kSimMaxTargets * 256; b += NT) lut[b] = st.lut[b];
  }
  __syncthreads();
  double s1 = 0.0, s2 = 0.0;
  unsigned kmin = 0xFFFFFFFFu, kmax = 0u;
  for (long long c = i + 1 + tid; c < N; c += NT) {
    const float x = p[c];
    const unsigned key = order_key(x);
    if constexpr (PASS == 0) {
      const double d = (double)x;
      s1 += d;
      s2 += d * d;
      kmin = key < kmin ? key : kmin;
      kmax = key > kmax ? key : kmax;
      int lo = 0, hi = n_thr;                    // thresholds at or below x (float32 compares)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thr[mid] <= x) lo = mid + 1; else hi = mid;
      }
      if (n_thr > 0) atomicAdd(&cle[lo * 32 + (lane & 31)], 1u);
      atomicAdd(&hist[(key >> 24) * REP + (lane & (REP - 1))], 1u);
    } else {
      int sl = lut[key >> 24];
      if constexpr (PASS >= 2) if (sl >= 0) sl = lut[(kSimMaxTargets + sl) * 256 + ((key >> 16) & 255u)];
      if constexpr (PASS >= 3) if (sl >= 0) sl = lut[(2 * kSimMaxTargets + sl) * 256 + ((key >> 8) & 255u)];
      if (sl >= 0) atomicAdd(&hist[sl * 256 + ((key >> (24 - 8 * PASS)) & 255u)], 1u);
    }
  }
  __syncthreads();
  if constexpr (PASS == 0) {
    unsigned h = 0u;
#pragma unroll
    for (int r = 0; r < REP; ++r) h += hist[tid * REP + r];
    if (h) atomicAdd(&st.digit_hist[tid], (unsigned long long)h);
    if (tid <= n_thr && n_thr > 0) {
      unsigned c = 0u;
      for (int r = 0; r < 32; ++r) c += cle[tid * 32 + r];
      if (c) atomicAdd(&st.count_le[tid], (unsigned long long)c);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    kmin = wave_min(kmin);
    kmax = wave_max(kmax);
    if (lane == 0) { part[wave][0] = s1; part[wave][1] = s2; pmm[wave][0] = kmin; pmm[wave][1] = kmax; }
    __syncthreads();
    if (tid == 0) {
      double t1 = 0.0, t2 = 0.0;
      unsigned a = 0xFFFFFFFFu, b = 0u;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        t1 += part[w][0];
        t2 += part[w][1];
        a = pmm[w][0] < a ? pmm[w][0] : a;
        b = pmm[w][1] > b ? pmm[w][1] : b;
      }
      st.row_sum[i] = t1;
      st.row_sumsq[i] = t2;
      if (i + 1 < N) {
        atomicMin(&st.minmax[0], a);
        atomicMax(&st.minmax[1], b);
      }
    }
  } else {
    for (int b = tid; b < kSimMaxTargets * 256; b += NT)
      if (hist[b]) atomicAdd(&st.digit_hist[b], (unsigned long long)hist[b]);
  }
}

__global__ void __launch_bounds__(1024) triu_total_kernel(long long N, TriuPtrs st) {
  __shared__ double part[16][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s1 = 0.0, s2 = 0.0;
  for (long long r = tid; r < N; r += 1024) {
    s1 += st.row_sum[r];
    s2 += st.row_sumsq[r];
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) { part[wave][0] = s1; part[wave][1] = s2; }
  __syncthreads();
  if (tid == 0) {
    double t1 = 0.0, t2 = 0.0;
    for (int w = 0; w < 16; ++w) { t1 += part[w][0]; t2 += part[w][1]; }
    st.total[0] = t1;
    st.total[1] = t2;
  }
}

// ------------------------------------------------------------------------------ triangle: histogram + extremes
__global__ void __launch_bounds__(NT)
triu_final_kernel(const float* __restrict__ S, long long r0, long long N, int nbins, unsigned key_hi, unsigned key_lo,
                  int want_ext, TriuPtrs st) {
  __shared__ double edges[kSimMaxBins + 1];
  __shared__ unsigned fh[kSimMaxBins];
  __shared__ int ties[2];
  const int tid = threadIdx.x;
  const long long i = r0 + blockIdx.x;
  const float* __restrict__ p = S + (long long)blockIdx.x * N;
  for (int b = tid; b <= nbins; b += NT) edges[b] = st.edges[b];
  for (int b = tid; b < kSimMaxBins; b += NT) fh[b] = 0u;
  if (tid < 2) ties[tid] = 0;
  __syncthreads();
  const double e0 = nbins > 0 ? edges[0] : 0.0, e1 = nbins > 0 ? edges[nbins] : 0.0;
  const double inv = e1 > e0 ? (double)nbins / (e1 - e0) : 0.0;
  int th = 0, tl = 0;
  for (long long c = i + 1 + tid; c < N; c += NT) {
    const float x = p[c];
    const double d = (double)x;
    if (nbins > 0 && d >= e0 && d <= e1) {
      // an arithmetic estimate, then corrected against the edges: bin b holds edges[b] <= d <
      // edges[b + 1], the last bin also d == edges[nbins]
      int b = (int)((d - e0) * inv);
      b = b < 0 ? 0 : (b > nbins - 1 ? nbins - 1 : b);
      while (b > 0 && d < edges[b]) --b;
      while (b < nbins - 1 && d >= edges[b + 1]) ++b;
      atomicAdd(&fh[b], 1u);
    }
    if (want_ext) {
      const unsigned key = order_key(x);
      if (key > key_hi) {
        const unsigned long long slot = atomicAdd(&st.counters[0], 1ull);
        if (slot < (unsigned long long)kSimMaxExt) {
          unsigned* e = st.ext + (0 * (size_t)kSimMaxExt + slot) * 3;
          e[0] = key; e[1] = (unsigned)i; e[2] = (unsigned)c;
        }
      }
      if (key < key_lo) {
        const unsigned long long slot = atomicAdd(&st.counters[1], 1ull);
        if (slot < (unsigned long long)kSimMaxExt) {
          unsigned* e = st.ext + (1 * (size_t)kSimMaxExt + slot) * 3;
          e[0] = key; e[1] = (unsigned)i; e[2] = (unsigned)c;
        }
      }
      th += key == key_hi;
      tl += key == key_lo;
    }
  }
  if (want_ext) {
    if (th) atomicAdd(&ties[0], th);
    if (tl) atomicAdd(&ties[1], tl);
  }
  __syncthreads();
  for (int b = tid; b < nbins; b += NT)
    if (fh[b]) atomicAdd(&st.hist[b], (unsigned long long)fh[b]);
  if (want_ext && tid < 2) st.row_tie[(long long)tid * st.npad + blockIdx.x] = ties[tid];
}

// The copies of a cut value that belong to the extremes are the first `take` in (i, j) order.  Row r
// of the block starts at base (the copies in earlier blocks) + the copies in the block's rows before
// it; inside the row the order is the columns', by a prefix count.  The block's last row leaves the
// next block's base in the other slot of the pair, so no block reads what a later one writes.
__global__ void __launch_bounds__(NT)
triu_tie_kernel(const float* __restrict__ S, long long r0, long long rows, long long N, unsigned key_hi, int take_hi,
                unsigned key_lo, int take_lo, int slot, TriuPtrs st) {
  __shared__ long long red[NW];
  __shared__ int wcnt[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long r = blockIdx.x, i = r0 + r;
  const float* __restrict__ p = S + r * N;
  for (int which = 0; which < 2; ++which) {
    const unsigned cut = which ? key_lo : key_hi;
    const long long take = which ? take_lo : take_hi;
    const int* __restrict__ cnt = st.row_tie + (long long)which * st.npad;
    long long pre = 0;
    for (long long q = tid; q < r; q += NT) pre += cnt[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o, 64);
    __syncthreads();                             // red and wcnt of the previous round are done with
    if (lane == 0) red[wave] = pre;
    __syncthreads();
    pre = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) pre += red[w];
    const long long base = (long long)st.counters[2 + which * 2 + slot];
    const long long mine = cnt[r];
    if (r == rows - 1 && tid == 0) st.counters[2 + which * 2 + (slot ^ 1)] = (unsigned long long)(base + pre + mine);
    long long at = base + pre;                   // uniform over the workgroup from here on
    if (mine == 0 || at >= take) continue;
    for (long long c0 = i + 1; c0 < N && at < take; c0 += NT) {
      const long long c = c0 + tid;
      const bool is = c < N && order_key(p[c]) == cut;
      int tot;
      const int off = wave_prefix(is, lane, &tot);
      if (lane == 0) wcnt[wave] = tot;
      __syncthreads();
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (w < wave) before += wcnt[w];
        all += wcnt[w];
      }
      const long long ord = at + before + off;
      if (is && ord < take) {
        unsigned* e = st.ext + ((size_t)(2 + which) * kSimMaxExt + (size_t)ord) * 3;
        e[0] = cut; e[1] = (unsigned)i; e[2] = (unsigned)c;
      }
      at += all;
      __syncthreads();
    }
  }
}

TriuPtrs triu_ptrs(void* state, long long N) {
  const TriuState l = triu_state_layout(N);
  char* b = static_cast<char*>(state);
  TriuPtrs p;
  p.row_sum = reinterpret_cast<double*>(b + l.row_sum);
  p.row_sumsq = reinterpret_cast<double*>(b + l.row_sumsq);
  p.total = reinterpret_cast<double*>(b + l.total);
  p.digit_hist = reinterpret_cast<unsigned long long*>(b + l.digit_hist);
  p.count_le = reinterpret_cast<unsigned long long*>(b + l.count_le);
  p.minmax = reinterpret_cast<unsigned*>(b + l.minmax);
  p.lut = reinterpret_cast<const signed char*>(b + l.lut);
  p.thr = reinterpret_cast<const float*>(b + l.thr);
  p.edges = reinterpret_cast<const double*>(b + l.edges);
  p.hist = reinterpret_cast<unsigned long long*>(b + l.hist);
  p.counters = reinterpret_cast<unsigned long long*>(b + l.counters);
  p.row_tie = reinterpret_cast<int*>(b + l.row_tie);
  p.ext = reinterpret_cast<unsigned*>(b + l.ext);
  p.npad = l.npad;
  return p;
}

// a workgroup per row: rows * NT work-items, below 2^31 (sim_block_rows keeps a block there)
bool rows_fit(long long rows) { return rows >= 1 && rows * NT < kSimGridItems; }

}  // namespace

hipError_t launch_rows_topk(const float* S, long long r0, long long rows, long long N, int k, float* top_scores,
                            long long* top_index, double* sum, double* sumsq, float* mn, float* mx, float* self,
                            hipStream_t s) {
  if (!rows_fit(rows) || r0 < 0 || r0 + rows > N || k < 1 || k > kSimMaxK) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rows_topk_kernel, dim3((unsigned)rows), dim3(NT), 0, s, S, r0, N, k, top_scores, top_index, sum,
                     sumsq, mn, mx, self);
  return hipGetLastError();
}

hipError_t launch_triu_select_pass(const float* S, long long r0, long long rows, long long N, int pass, int n_thr,
                                   void* state, hipStream_t s) {
  if (!rows_fit(rows) || r0 < 0 || r0 + rows > N || pass < 0 || pass > 3 || n_thr < 0 || n_thr > kSimMaxThr)
    return hipErrorInvalidValue;
  const TriuPtrs st = triu_ptrs(state, N);
  const dim3 grid((unsigned)rows), block(NT);
  switch (pass) {
    case 0: hipLaunchKernelGGL(triu_select_kernel<0>, grid, block, 0, s, S, r0, N, n_thr, st); break;
    case 1: hipLaunchKernelGGL(triu_select_kernel<1>, grid, block, 0, s, S, r0, N, n_thr, st); break;
    case 2: hipLaunchKernelGGL(triu_select_kernel<2>, grid, block, 0, s, S, r0, N, n_thr, st); break;
    default: hipLaunchKernelGGL(triu_select_kernel<3>, grid, block, 0, s, S, r0, N, n_thr, st); break;
  }
  return hipGetLastError();
}

hipError_t launch_triu_total(long long N, void* state, hipStream_t s) {
  if (N < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(triu_total_kernel, dim3(1), dim3(1024), 0, s, N, triu_ptrs(state, N));
  return hipGetLastError();
}

hipError_t launch_triu_final(const float* S, long long r0, long long rows, long long N, int nbins, unsigned key_hi,
                             int take_hi, unsigned key_lo, int take_lo, int want_ext, long long block_index,
                             void* state, hipStream_t s) {
  if (!rows_fit(rows) || r0 < 0 || r0 + rows > N || nbins < 0 || nbins > kSimMaxBins || take_hi < 0 ||
      take_hi > kSimMaxExt || take_lo < 0 || take_lo > kSimMaxExt)
    return hipErrorInvalidValue;
  const TriuPtrs st = triu_ptrs(state, N);
  hipLaunchKernelGGL(triu_final_kernel, dim3((unsigned)rows), dim3(NT), 0, s, S, r0, N, nbins, key_hi, key_lo, want_ext,
                     st);
  if (want_ext)
    hipLaunchKernelGGL(triu_tie_kernel, dim3((unsigned)rows), dim3(NT), 0, s, S, r0, rows, N, key_hi, take_hi, key_lo,
                       take_lo, (int)(block_index & 1), st);
  return hipGetLastError();
}

}  // namespace spk
