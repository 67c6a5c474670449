// VAD front end of the diarization pipeline on the device (gfx950): the O(L) arithmetic of
// EnergyVad / vad_post.frame_energy / vad_post.apply_mask, 16 kHz.
//
// vad_energy_kernel: one pass over the signal, two mean-square tracks of the clipped samples
// c = min(max(x, -1), 1) of every utterance of a ragged batch:
//   e16[f] = mean(c^2) over the 16 ms frame [256 f, 256 f + 256)                  fp64, L / 256 frames
//   e20[j] = mean(c^2) over the 20 ms window [160 j, 160 j + 320), 10 ms hop      fp32, (L - 320) / 160 + 1
// The arithmetic is fixed so that an utterance has the same bits alone, in any batch, at any
// offset and on any grid:
//   - squares and sums are fp64 (a square of an fp32 value is exact in fp64);
//   - a QUAD is 4 samples, counted from the utterance's first sample: ((c0^2 + c1^2) + c2^2) + c3^2;
//   - a BLOCK is 32 = gcd(160, 256) samples, i.e. 8 quads added in ascending order;
//   - a hop is its 5 blocks added in ascending order, a frame its 8 blocks likewise;
//   - e16 = frame / 256.0;  e20[j] = float(hop[j] + hop[j + 1]) / 320.0f  (one rounding to fp32,
//     one fp32 division);
//   - no FMA contraction (the pragma below), so the chain is the same on every compiler setting.
// Non-finite samples are outside the contract (fminf / fmaxf drop a NaN where np.clip keeps it).
//
// The kernel is bandwidth-bound (4 B read per sample, 12 B written per 1280).  A workgroup walks
// tiles of 64 hops = 40 frames = 10240 samples of ONE utterance (1280 = lcm(160, 256), so a tile
// starts on a hop, a frame and a quad) plus one hop of look-ahead for the last window: 2600 quads,
// one dwordx4 load per lane each (consecutive lanes, consecutive 16 B; scalar loads when the
// utterance does not start on a 16 B boundary).  Quad sums go to LDS, then one lane per block adds
// its 8 quads, then one lane per output adds its blocks.  The quad array is padded by one double
// per 8, so the 8-double stride of the second step falls on distinct banks.  No atomics.  Grid: G
// slices per utterance, slice g taking tiles g, g + G, ... (lengths are read from the device
// offsets: the call only enqueues).
//
// vad_apply_kernel: out[i] = wav[i] inside one of n_iv sorted, disjoint intervals, else 0.  A
// workgroup owns 4096 consecutive samples; the intervals that meet them are found by two uniform
// binary searches, each lane then searches that (usually one-element) range for each of its 4
// samples, starting from the previous sample's answer.
#include "vad.h"

#pragma clang fp contract(off)

namespace spk {
namespace {

constexpr int VE_THREADS = 256;
constexpr int VE_U = 4;                                        // dwordx4 loads in flight per lane
constexpr int VE_TILE_HOPS = 64;
constexpr int VE_TILE = VE_TILE_HOPS * kVadHop;                // 10240 samples
constexpr int VE_TILE_FRAMES = VE_TILE / kVadFrame;            // 40
constexpr int VE_BLOCKS = (VE_TILE + kVadHop) / kVadBlock;     // 325, the look-ahead hop included
constexpr int VE_QUADS = VE_BLOCKS * (kVadBlock / 4);          // 2600
constexpr int VE_BLOCKS_PER_HOP = kVadHop / kVadBlock;         // 5
constexpr int VE_BLOCKS_PER_FRAME = kVadFrame / kVadBlock;     // 8
static_assert(VE_TILE % kVadFrame == 0 && VE_TILE % kVadHop == 0, "a tile starts on a frame and on a hop");
static_assert(VE_TILE_HOPS + VE_TILE_FRAMES <= VE_THREADS, "one lane per output of a tile");

__device__ __forceinline__ int quad_slot(int q) { return q + (q >> 3); }

__device__ __forceinline__ double clipped_square(float x) {
  const double c = (double)fminf(fmaxf(x, -1.0f), 1.0f);
  return c * c;
}

__device__ __forceinline__ double quad_sum(const float4& v) {
  return ((clipped_square(v.x) + clipped_square(v.y)) + clipped_square(v.z)) + clipped_square(v.w);
}

template <int N>
__device__ __forceinline__ double chain_sum(const double* p) {
  double s = p[0];
#pragma unroll
  for (int i = 1; i < N; ++i) s = s + p[i];
  return s;
}

__global__ void __launch_bounds__(VE_THREADS)
vad_energy_kernel(const float* __restrict__ wav, const int64_t* __restrict__ wav_off, double* __restrict__ e16,
                  const int64_t* __restrict__ e16_off, float* __restrict__ e20, const int64_t* __restrict__ e20_off,
                  int G) {
  __shared__ double s_quad[VE_QUADS + VE_QUADS / 8];
  __shared__ double s_blk[VE_BLOCKS];

  const int utt = blockIdx.x / G, g = blockIdx.x % G, tid = threadIdx.x;
  const int64_t x0 = wav_off[utt], L = wav_off[utt + 1] - x0;
  const int64_t o16 = e16_off[utt], o20 = e20_off[utt];
  // never past the declared ranges, whatever the offsets say
  const int64_t n16 = min(L >= 0 ? L / kVadFrame : 0, e16_off[utt + 1] - o16);
  const int64_t n20 = min(L >= kVadWin ? (L - kVadWin) / kVadHop + 1 : 0, e20_off[utt + 1] - o20);
  const int64_t ntiles =
      max((n16 + VE_TILE_FRAMES - 1) / VE_TILE_FRAMES, (n20 + VE_TILE_HOPS - 1) / VE_TILE_HOPS);
  if (g >= ntiles) return;
  const float* x = wav + x0;
  const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const int64_t nq_all = L / kVadBlock * (kVadBlock / 4);     // quads of the complete blocks: all an output reads

  for (int64_t tile = g; tile < ntiles; tile += G) {
    const int64_t q0 = tile * (VE_TILE / 4);
    const int nq = (int)min((int64_t)VE_QUADS, nq_all - q0);  // >= 1: the tile has an output
    __syncthreads();                                          // the previous tile's reads are done
    for (int base = 0; base < VE_QUADS; base += VE_THREADS * VE_U) {
      float4 v[VE_U];
#pragma unroll
      for (int u = 0; u < VE_U; ++u) {
        const int q = base + u * VE_THREADS + tid;
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < nq) {
          const float* p = x + 4 * (q0 + q);
          if (aligned) v[u] = *reinterpret_cast<const float4*>(p);
          else v[u] = make_float4(p[0], p[1], p[2], p[3]);
        }
      }
#pragma unroll
      for (int u = 0; u < VE_U; ++u) {
        const int q = base + u * VE_THREADS + tid;
        if (q < VE_QUADS) s_quad[quad_slot(q)] = quad_sum(v[u]);
      }
    }
    __syncthreads();
    for (int b = tid; b < VE_BLOCKS; b += VE_THREADS) s_blk[b] = chain_sum<8>(s_quad + quad_slot(8 * b));
    __syncthreads();
    if (tid < VE_TILE_HOPS) {
      const int64_t j = tile * VE_TILE_HOPS + tid;
      if (j < n20) {
        const double h0 = chain_sum<VE_BLOCKS_PER_HOP>(s_blk + VE_BLOCKS_PER_HOP * tid);
        const double h1 = chain_sum<VE_BLOCKS_PER_HOP>(s_blk + VE_BLOCKS_PER_HOP * (tid + 1));
        e20[o20 + j] = __fdiv_rn((float)(h0 + h1), (float)kVadWin);
      }
    } else if (tid < VE_TILE_HOPS + VE_TILE_FRAMES) {
      const int fl = tid - VE_TILE_HOPS;
      const int64_t f = tile * VE_TILE_FRAMES + fl;
      if (f < n16) e16[o16 + f] = chain_sum<VE_BLOCKS_PER_FRAME>(s_blk + VE_BLOCKS_PER_FRAME * fl) / (double)kVadFrame;
    }
  }
}

constexpr int VA_THREADS = 256;
constexpr int VA_U = 4;
constexpr int VA_TILE = VA_THREADS * VA_U * 4;   // samples per workgroup

// first k in [lo, hi) with a[k] > v (a ascending), hi when there is none
__device__ __forceinline__ int64_t first_above(const int64_t* __restrict__ a, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a[mid] > v) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ void __launch_bounds__(VA_THREADS)
vad_apply_kernel(const float* __restrict__ wav, int64_t L, const int64_t* __restrict__ starts,
                 const int64_t* __restrict__ ends, int64_t n_iv, float* __restrict__ out) {
  const int64_t t0 = (int64_t)blockIdx.x * VA_TILE, t1 = min(L, t0 + VA_TILE);
  // intervals [k0, k1) meet [t0, t1): the first that ends past t0, up to the first that starts at or past t1
  const int64_t k0 = first_above(ends, 0, n_iv, t0);
  const int64_t k1 = first_above(starts, k0, n_iv, t1 - 1);
  const bool aligned = ((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
#pragma unroll
  for (int u = 0; u < VA_U; ++u) {
    const int64_t i = t0 + (int64_t)(u * VA_THREADS + threadIdx.x) * 4;
    if (i >= t1) continue;
    const int cnt = (int)min((int64_t)4, t1 - i);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (k0 < k1) {
      if (aligned && cnt == 4) {
        const float4 w = *reinterpret_cast<const float4*>(wav + i);
        v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
      } else {
        for (int c = 0; c < cnt; ++c) v[c] = wav[i + c];
      }
      int64_t k = k0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        // the only interval that can hold idx: the first that ends past it (k1 - 1 >= k0: a valid index)
        const int64_t idx = i + c;
        k = first_above(ends, k, k1, idx);
        const bool keep = (k < k1) & (starts[min(k, k1 - 1)] <= idx);
        v[c] = keep ? v[c] : 0.f;
      }
    }
    if (aligned && cnt == 4) {
      *reinterpret_cast<float4*>(out + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int c = 0; c < cnt; ++c) out[i + c] = v[c];
    }
  }
}

}  // namespace

hipError_t launch_vad_energy(const float* wav, const int64_t* wav_off, int n_utt, double* e16, const int64_t* e16_off,
                             float* e20, const int64_t* e20_off, hipStream_t s) {
  if (n_utt < 0) return hipErrorInvalidValue;
  if (n_utt == 0) return hipSuccess;
  if (!wav || !wav_off || !e16 || !e16_off || !e20 || !e20_off) return hipErrorInvalidValue;
  // about 2048 workgroups in the grid (256 CUs, up to six resident on each), at least one per utterance
  const int G = n_utt >= 2048 ? 1 : (2048 + n_utt - 1) / n_utt;
  if ((int64_t)n_utt * G > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vad_energy_kernel, dim3((unsigned)(n_utt * G)), dim3(VE_THREADS), 0, s, wav, wav_off, e16, e16_off,
                     e20, e20_off, G);
  return hipGetLastError();
}

hipError_t launch_vad_apply_intervals(const float* wav, int64_t L, const int64_t* starts, const int64_t* ends,
                                      int64_t n_iv, float* out, hipStream_t s) {
  if (L < 0 || n_iv < 0) return hipErrorInvalidValue;
  if (L == 0) return hipSuccess;
  if (!wav || !out || (n_iv > 0 && (!starts || !ends))) return hipErrorInvalidValue;
  const int64_t blocks = (L + VA_TILE - 1) / VA_TILE;
  if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vad_apply_kernel, dim3((unsigned)blocks), dim3(VA_THREADS), 0, s, wav, L, starts, ends, n_iv, out);
  return hipGetLastError();
}

}  // namespace spk
