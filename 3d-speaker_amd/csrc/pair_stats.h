// Pair-cosine statistics of a ragged batch of embedding groups (the single-speaker check): the
// batch descriptor, the launch plan and the launchers (pair_stats.hip); checks and the launch
// loop in pair_stats_abi.cpp.
#pragma once
#include "common.h"

namespace spk {

// largest group: 32768 rows are 536,854,528 pairs (a 2 GiB condensed cosine array)
constexpr int64_t kPairMaxRows = 32768;
// largest group the form without a cosine array takes: one workgroup scores all of a group's
// pairs there (4096 rows: 8,386,560 pairs, about half a million per wave)
constexpr int64_t kPairFusedMaxRows = 4096;
// groups per launch: their descriptors travel as kernel arguments (20 bytes each)
constexpr int kPairChunk = 64;
// pairs per launch of the pair kernel.  A launch's grid is counted in work-items, a 32-bit number:
// a pair takes a wave, so 2^25 pairs are 2^31 work-items (2^23 blocks of 256).  A chunk's pair
// range is cut into launches of at most this many, wherever the cuts fall inside its groups.
constexpr int64_t kPairLaunchMax = (int64_t)1 << 25;
// threads of the workgroup that reduces a group; also the stride of the summation order below
constexpr int kPairThreads = 1024;

inline int64_t pair_count(int64_t n) { return n > 1 ? n * (n - 1) / 2 : 0; }

// Groups [g0, g0 + ng) of a call.  Pair p of group k is cos[pair0[k] + p]: pair0 holds the call's
// own prefix sums, so one condensed array serves every launch.
struct PairBatchArgs {
  long long row0[kPairChunk];        // first row of X
  long long pair0[kPairChunk + 1];
  int n[kPairChunk];                 // rows
  int ng;
};

// The launch plan of a call, shared by the launch loop and spk_pair_cosine_plan: the groups in
// chunks of kPairChunk; per chunk pairs(a, q0, q1) for every range [q0, q1) of at most
// kPairLaunchMax of its pairs (none for a chunk without pairs; skipped altogether unless
// with_pairs), then stats(a, g0).  A callback returns 0 to go on; anything else ends the walk and
// is returned.
template <class FP, class FS>
inline int plan_pair_launches(const int64_t* offsets, int32_t G, bool with_pairs, FP pairs, FS stats) {
  int64_t pair0 = 0;   // pairs of the groups before g0
  for (int32_t g0 = 0; g0 < G;) {
    PairBatchArgs a;
    a.ng = 0;
    a.pair0[0] = pair0;
    for (; g0 + a.ng < G && a.ng < kPairChunk; ++a.ng) {
      const int64_t n = offsets[g0 + a.ng + 1] - offsets[g0 + a.ng];
      a.row0[a.ng] = offsets[g0 + a.ng];
      a.n[a.ng] = (int)n;
      a.pair0[a.ng + 1] = a.pair0[a.ng] + pair_count(n);
    }
    if (with_pairs)
      for (int64_t q0 = pair0; q0 < a.pair0[a.ng]; q0 += kPairLaunchMax) {
        const int64_t q1 = a.pair0[a.ng] - q0 < kPairLaunchMax ? a.pair0[a.ng] : q0 + kPairLaunchMax;
        if (int rc = pairs(a, q0, q1)) return rc;
      }
    if (int rc = stats(a, g0)) return rc;
    pair0 = a.pair0[a.ng];
    g0 += a.ng;
  }
  return 0;
}

// Not linked into the host-only build of the executor (tests/emu): weak, checked by the ABI.
// cos[q] for the pairs q in [q0, q1) of the batch's condensed range, one wave per pair
hipError_t launch_pair_cosine(const PairBatchArgs& a, long long q0, long long q1, const float* X, long long ldx, int E,
                              float* cos, hipStream_t s) __attribute__((weak));
// min / mean / argmin / n_below of every group of the batch (outputs: this batch's slices), one
// workgroup per group; from cos when it is given, else from X directly.  The order of the fp64 sum
// is the same in both forms: thread t of kPairThreads adds pairs t, t + kPairThreads, ... in
// ascending order, a wave adds its lanes by a fixed butterfly, thread 0 adds the waves in order.
hipError_t launch_pair_stats(const PairBatchArgs& a, const float* X, long long ldx, int E, float threshold,
                             const float* cos, float* mn, float* mean, long long* argmin, long long* n_below,
                             hipStream_t s) __attribute__((weak));

}  // namespace spk
