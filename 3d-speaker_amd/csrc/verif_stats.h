// All-pairs verification statistics (the N x N cosine matrix of one labelled embedding set, never
// stored): the device state and the launchers of verif_stats.hip; checks, the prefix tables and the
// launch loops in verif_stats_abi.cpp.  The row blocking, the key map and the workspace sizes are
// those of the corpus similarity statistics (sim_stats.h).
#pragma once
#include "sim_stats.h"

namespace spk {

constexpr int kVerifMaxPrefixes = 16;   // prefixes of one digits pass
constexpr int kVerifClasses = 2;        // 0: labels differ (non-target), 1: labels agree (target)

// Device state (spk_cosine_verif_workspace_bytes): everything but the block of scores.  Offsets in
// bytes, every section 16-byte aligned.
struct VerifState {
  size_t row_sum, row_sumsq;     // double [2][Npad]: each row's fp64 sums over its columns j > i, per class
  size_t total;                  // double [4]: sum[2], sumsq[2] in the fixed order of verif_total_kernel
  size_t count;                  // u64 [2]: pairs per class
  size_t minmax;                 // u32 [4]: smallest key [2], largest key [2]
  size_t edges;                  // double [kSimMaxBins + 1]
  size_t hist;                   // u64 [2][kSimMaxBins]
  size_t digits;                 // u64 [kVerifMaxPrefixes][2][256]
  size_t lut;                    // i8 [3][kVerifMaxPrefixes][256]: slot of a prefix's next digit, -1 none
  size_t flag;                   // i32 [4]: [0] the smallest label
  size_t bytes;
  int64_t npad;
};

inline VerifState verif_state_layout(int64_t N) {
  VerifState s;
  s.npad = (N + kSimRowTile - 1) / kSimRowTile * kSimRowTile;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 15) / 16 * 16; return at; };
  s.row_sum = take((size_t)2 * s.npad * 8);
  s.row_sumsq = take((size_t)2 * s.npad * 8);
  s.total = take(4 * 8);
  s.count = take(2 * 8);
  s.minmax = take(4 * 4);
  s.edges = take((kSimMaxBins + 1) * 8);
  s.hist = take((size_t)2 * kSimMaxBins * 8);
  s.digits = take((size_t)kVerifMaxPrefixes * 2 * 256 * 8);
  s.lut = take((size_t)3 * kVerifMaxPrefixes * 256);
  s.flag = take(4 * 4);
  s.bytes = o;
  return s;
}

// Not linked into the host-only builds: weak, checked by the ABI.
// the smallest of the N labels into the state's flag
hipError_t launch_verif_label_min(const int* labels, long long N, void* state, hipStream_t s) __attribute__((weak));
// rows [r0, r0 + rows) of the N x N scores in S (row stride N), the columns j > i of each, per class:
// counts, smallest and largest key, the histogram over the state's edges, and the row's fp64 sums.
// fp64 sums: thread t of kSimThreads adds its columns i + 1 + t, i + 1 + t + kSimThreads, ... of a class
// in ascending order, a wave adds its lanes by a fixed butterfly, thread 0 adds the four waves in order.
hipError_t launch_verif_moments(const float* S, const int* labels, long long r0, long long rows, long long N, int nbins,
                                void* state, hipStream_t s) __attribute__((weak));
// the rows' fp64 sums added up per class: thread t of 1024 adds rows t, t + 1024, ... in ascending
// order, a wave adds its lanes by a fixed butterfly, thread 0 adds the sixteen waves in order
hipError_t launch_verif_total(long long N, void* state, hipStream_t s) __attribute__((weak));
// the per-class histograms of the next digit of the keys that match one of the n_slots prefixes of
// `level` bytes (through the state's tables; level 0: every key, one slot)
hipError_t launch_verif_digits(const float* S, const int* labels, long long r0, long long rows, long long N, int level,
                               int n_slots, void* state, hipStream_t s) __attribute__((weak));

}  // namespace spk
