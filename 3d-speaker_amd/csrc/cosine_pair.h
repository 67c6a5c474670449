// The cosine of one (row of A, row of Bm) pair, computed by one wave: the device function behind
// spk_cosine_trials (affinity.hip) and spk_cosine_trials_norm (score_norm.hip), so that both give
// a trial's raw score the same bits.  float4 per lane, the three sums reduced across the wave
// (every lane ends with the full sums and returns the same value); sklearn semantics, a zero-norm
// row divides by 1.  E % 4 == 0.
#pragma once
#include "common.h"

#ifdef __HIPCC__
namespace spk {

__device__ __forceinline__ float wave_pair_cosine(const float* __restrict__ a, const float* __restrict__ b, int E,
                                                  int lane) {
  typedef float pair_f32x4 __attribute__((ext_vector_type(4)));
  float d = 0.f, na = 0.f, nb = 0.f;
  for (int k = lane * 4; k < E; k += 256) {
    const pair_f32x4 x = *reinterpret_cast<const pair_f32x4*>(a + k);
    const pair_f32x4 y = *reinterpret_cast<const pair_f32x4*>(b + k);
    d += x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
    na += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
    nb += y[0] * y[0] + y[1] * y[1] + y[2] * y[2] + y[3] * y[3];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    d += __shfl_xor(d, o, 64);
    na += __shfl_xor(na, o, 64);
    nb += __shfl_xor(nb, o, 64);
  }
  const float sa = na == 0.f ? 1.f : sqrtf(na), sb = nb == 0.f ? 1.f : sqrtf(nb);
  return d / (sa * sb);
}

}  // namespace spk
#endif
