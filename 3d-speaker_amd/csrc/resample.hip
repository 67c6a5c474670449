// Windowed-sinc polyphase resampler (torchaudio.functional.resample's default path; tables and
// arithmetic: resample_abi.cpp), gfx950.
//
//   y[b n + p] = sum_s x[b o - w + k0[p] + s] * taps[p][s],  s < S    (ResampleTable, resample.h)
//
// one fp32 fmaf chain per output in ascending tap order, so an output's bits depend on its
// utterance's samples only: not on the batch around it, the tile it falls into or the grid.
// x reads as zero outside its utterance's [0, L).
//
// Work per output is S ~ 12 max(o, n) / n FMAs (14 for 8 -> 16 kHz, 38 for 48 -> 16 kHz, 34 for
// 44.1 -> 16 kHz) on 4 B written, and every operand is shared between neighbouring outputs, so
// both operands come from LDS:
//  - the compact table (n x S floats: 22 KB for 44.1 -> 16 kHz, where the full n x K table is
//    304 KB) is staged once per workgroup, rows an odd number of floats apart: the lanes of a
//    wave hold consecutive outputs, i.e. consecutive phases, which then read distinct banks
//    (one phase, n = 1: a broadcast);
//  - a workgroup walks tiles of NB consecutive b of ONE utterance (NB n consecutive outputs):
//    the tile's input span, NB o + 2 w samples, is staged with coalesced loads, zero-filled
//    outside the utterance, and each wave stores contiguous runs of 64 outputs.
// Every thread carries U independent chains (outputs 256 apart) so that LDS latency overlaps.
// Grid: G slices per utterance, slice g taking tiles g, g + G, ... of its utterance (lengths
// are read from the device offsets: the call only enqueues).
//
// Rate pairs whose table or span does not fit the LDS budget (max(o, n) in the thousands: no
// audio rate pair in use) run resample_direct_kernel: the same chain, operands from global memory.
#include "resample.h"

#include <algorithm>

namespace spk {
namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_U = 4;
constexpr int RS_LDS_BYTES = 48 * 1024;        // per workgroup: three workgroups per CU
constexpr int RS_TABLE_LDS_BYTES = 36 * 1024;  // of which the table may take this much
constexpr int RS_TILE_OUT = 4096;              // outputs per tile aimed at

__global__ void __launch_bounds__(RS_THREADS)
resample_tile_kernel(const float* __restrict__ wav, const int64_t* __restrict__ wav_off, float* __restrict__ out,
                     const int64_t* __restrict__ out_off, const float* __restrict__ taps, const int* __restrict__ k0,
                     int o, int n, int w, int S, int ld, int NB, int G) {
  extern __shared__ float smem[];
  float* s_taps = smem;                                     // [n][ld]
  int* s_k0 = reinterpret_cast<int*>(smem + n * ld);        // [n]
  float* s_x = smem + n * ld + n;                           // [NB o + 2 w]

  const int utt = blockIdx.x / G, g = blockIdx.x % G, tid = threadIdx.x;
  const int64_t x0 = wav_off[utt], L = wav_off[utt + 1] - x0;
  const int64_t y0 = out_off[utt], M = out_off[utt + 1] - y0;
  const int tile_out = NB * n;
  const int64_t ntiles = (M + tile_out - 1) / tile_out;
  if (g >= ntiles) return;
  const float* x = wav + x0;
  float* y = out + y0;

  for (int i = tid; i < n * ld; i += RS_THREADS) s_taps[i] = taps[i];
  for (int i = tid; i < n; i += RS_THREADS) s_k0[i] = k0[i];

  // a tile starts at a multiple of n, so output tid + 256 i of a tile has the same (phase, b
  // within the tile) in every tile; from one to the next: + (256 % n, 256 / n) with carry
  const int span = NB * o + 2 * w;
  const int dp = RS_THREADS % n, db = RS_THREADS / n;
  const int p0 = tid % n, b0 = tid / n;

  for (int64_t tile = g; tile < ntiles; tile += G) {
    const int64_t xs = tile * NB * o - w;       // sample of the utterance held by s_x[0]
    __syncthreads();                            // the previous tile's reads are done
    for (int i = tid; i < span; i += RS_THREADS) {
      const int64_t gi = xs + i;
      s_x[i] = gi >= 0 && gi < L ? x[gi] : 0.f;
    }
    __syncthreads();
    const int64_t j0 = tile * tile_out;
    const int cnt = (int)min((int64_t)tile_out, M - j0);
    int p = p0, b = b0;
    for (int q = tid; q < cnt; q += RS_THREADS * RS_U) {
      const float* hp[RS_U];
      const float* xp[RS_U];
      float acc[RS_U];
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        const bool live = q + u * RS_THREADS < cnt;   // a chain past the tile's end re-does output 0
        const int pp = live ? p : 0, bb = live ? b : 0;
        hp[u] = s_taps + pp * ld;
        xp[u] = s_x + bb * o + s_k0[pp];
        acc[u] = 0.f;
        p += dp;
        b += db;
        if (p >= n) {
          p -= n;
          ++b;
        }
      }
      for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int u = 0; u < RS_U; ++u) acc[u] = fmaf(xp[u][s], hp[u][s], acc[u]);
      }
#pragma unroll
      for (int u = 0; u < RS_U; ++u)
        if (q + u * RS_THREADS < cnt) y[j0 + q + u * RS_THREADS] = acc[u];
    }
  }
}

__global__ void __launch_bounds__(RS_THREADS)
resample_direct_kernel(const float* __restrict__ wav, const int64_t* __restrict__ wav_off, float* __restrict__ out,
                       const int64_t* __restrict__ out_off, const float* __restrict__ taps, const int* __restrict__ k0,
                       int o, int n, int w, int S, int ld, int G) {
  const int utt = blockIdx.x / G, g = blockIdx.x % G;
  const int64_t x0 = wav_off[utt], L = wav_off[utt + 1] - x0;
  const int64_t y0 = out_off[utt], M = out_off[utt + 1] - y0;
  const float* x = wav + x0;
  for (int64_t j = (int64_t)g * RS_THREADS + threadIdx.x; j < M; j += (int64_t)G * RS_THREADS) {
    const int p = (int)(j % n);
    const int64_t xs = j / n * o - w + k0[p];
    const float* hp = taps + (size_t)p * ld;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) {
      const int64_t gi = xs + s;
      acc = fmaf(gi >= 0 && gi < L ? x[gi] : 0.f, hp[s], acc);
    }
    out[y0 + j] = acc;
  }
}

}  // namespace

hipError_t launch_resample(const float* wav, const int64_t* wav_off, int n_utt, const ResampleTable& t, float* out,
                           const int64_t* out_off, hipStream_t s) {
  if (n_utt < 0 || !wav_off || !out_off || !t.taps || !t.k0 || t.o <= 0 || t.n <= 0 || t.S <= 0 || t.ld < t.S)
    return hipErrorInvalidValue;
  if (n_utt == 0) return hipSuccess;
  // about 2048 workgroups in the grid (256 CUs, three resident on each), at least one per utterance
  const int G = std::max(1, std::min(2048, (2048 + n_utt - 1) / n_utt));
  if ((int64_t)n_utt * G > 0x7FFFFFFF) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(n_utt * G)), block(RS_THREADS);
  // tile: NB consecutive b with table + span inside the LDS budget
  const int64_t table_floats = (int64_t)t.n * t.ld + t.n;
  int NB = 0;
  if (table_floats * 4 <= RS_TABLE_LDS_BYTES) {
    const int64_t room = RS_LDS_BYTES / 4 - table_floats - 2 * (int64_t)t.width;
    NB = (int)std::min<int64_t>((RS_TILE_OUT + t.n - 1) / t.n, room > 0 ? room / t.o : 0);
  }
  if (NB >= 1 && (int64_t)NB * t.n >= RS_THREADS) {
    const size_t lds = (size_t)(table_floats + (int64_t)NB * t.o + 2 * t.width) * sizeof(float);
    hipLaunchKernelGGL(resample_tile_kernel, grid, block, lds, s, wav, wav_off, out, out_off, t.taps, t.k0, t.o, t.n,
                       t.width, t.S, t.ld, NB, G);
  } else {
    hipLaunchKernelGGL(resample_direct_kernel, grid, block, 0, s, wav, wav_off, out, out_off, t.taps, t.k0, t.o, t.n,
                       t.width, t.S, t.ld, G);
  }
  return hipGetLastError();
}

}  // namespace spk
