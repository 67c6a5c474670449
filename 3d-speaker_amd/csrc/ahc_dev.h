// Device helpers shared by the two AHC kernel files (ahc.hip: three launches per merge;
// ahc_batched.hip: one workgroup per problem): the candidate order of the tie rule, the workgroup
// reduction over it and the Lance-Williams update.  Included by .hip files only.
#pragma once
#include "common.h"

namespace spk {

struct Cand {
  double v;
  int r, c;   // c < 0: no candidate
};

// b beats a: larger value, then smaller row, then smaller column
__device__ __forceinline__ bool beats(const Cand& a, const Cand& b) {
  if (b.c < 0) return false;
  if (a.c < 0) return true;
  if (b.v != a.v) return b.v > a.v;
  if (b.r != a.r) return b.r < a.r;
  return b.c < a.c;
}

// best candidate of the wave in lane 0
__device__ __forceinline__ Cand wave_best(Cand x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Cand o;
    o.v = __shfl_down(x.v, off);
    o.r = __shfl_down(x.r, off);
    o.c = __shfl_down(x.c, off);
    if (beats(x, o)) x = o;
  }
  return x;
}

// best candidate of the workgroup in thread 0: shuffles inside a wave, one LDS slot per wave
template <int NT>
__device__ __forceinline__ Cand block_best(Cand x, Cand* slots) {
  constexpr int NW = NT / 64;
  x = wave_best(x);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) slots[w] = x;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 1; q < NW; ++q)
      if (beats(x, slots[q])) x = slots[q];
  return x;
}

// average linkage of the merged cluster (sizes si, sj) to a third one, written without FMA
// contraction: the rounding of the numpy restatement in tests/test_gpu_ahc.py
__device__ __forceinline__ double lance_williams(double a, double b, int si, int sj) {
#pragma clang fp contract(off)
  const double pa = (double)si * a;
  const double pb = (double)sj * b;
  const double num = pa + pb;
  return num / (double)(si + sj);
}

}  // namespace spk
