// Corpus similarity statistics (the N x N cosine matrix of one embedding set, never stored): the
// row blocking, the device state of the triangle statistics and the launchers (sim_stats.hip);
// checks, the host side of the multi-target select and the launch loops in sim_stats_abi.cpp.
#pragma once
#include "common.h"

namespace spk {

constexpr int64_t kSimRowTile = 128;              // rows of the affinity tile (affinity.hip)
constexpr int64_t kSimMaxRows = 0x7FFFFFFF;
constexpr size_t kSimBlockBytes = (size_t)128 << 20;   // half of the Infinity Cache, as the cohort statistics
constexpr int kSimMaxK = 1024, kSimMaxThr = 32, kSimMaxRanks = 16, kSimMaxBins = 256, kSimMaxExt = 4096;
// targets of the select: the caller's ranks and the two cuts of the extreme pairs
constexpr int kSimMaxTargets = kSimMaxRanks + 2;
constexpr int kSimThreads = 256;
// A launch's grid is counted in work-items, a 32-bit number.  The consumers take a workgroup of
// kSimThreads per row, the affinity a workgroup of 256 per 128 x 128 tile: a block of R rows is
// R * 256 work-items here and ceil(N / 128) * (R / 128) * 256 there, both kept below 2^31.
constexpr int64_t kSimGridItems = (int64_t)1 << 31;

inline int64_t sim_pairs(int64_t N) { return N * (N - 1) / 2; }   // N <= 2^31 - 1: below 2^62
inline size_t sim_min_bytes(int64_t N) { return (size_t)kSimRowTile * (size_t)N * sizeof(float); }

// rows per block for a workspace: the largest multiple of the row tile that fits, no more than N
// rounded up, no more than the grid limits allow (0: below the minimum, or N too large for one tile
// of rows to be one launch)
inline int64_t sim_block_rows(int64_t N, size_t workspace_bytes) {
  const size_t row = (size_t)N * sizeof(float);
  int64_t r = (int64_t)(workspace_bytes / row / kSimRowTile) * kSimRowTile;
  const int64_t all = (N + kSimRowTile - 1) / kSimRowTile * kSimRowTile;
  if (r > all) r = all;
  const int64_t col_tiles = (N + kSimRowTile - 1) / kSimRowTile;
  const int64_t by_affinity = ((kSimGridItems - 1) / 256 / col_tiles) * kSimRowTile;   // row tiles * 128
  const int64_t by_rows = ((kSimGridItems - 1) / kSimThreads / kSimRowTile) * kSimRowTile;
  const int64_t by_grid_y = (int64_t)65535 * kSimRowTile;                              // the affinity's grid.y
  if (r > by_affinity) r = by_affinity;
  if (r > by_rows) r = by_rows;
  if (r > by_grid_y) r = by_grid_y;
  return r;
}

inline size_t sim_workspace_bytes(int64_t N) {
  const size_t want = kSimBlockBytes > sim_min_bytes(N) ? kSimBlockBytes : sim_min_bytes(N);
  return (size_t)sim_block_rows(N, want) * (size_t)N * sizeof(float);
}

// Device state of the triangle statistics (spk_cosine_triu_state_bytes): everything but the block
// of scores.  Offsets in bytes, every section 16-byte aligned.
struct TriuState {
  size_t row_sum, row_sumsq;     // double [Npad]: each row's fp64 sums over its columns j > i
  size_t total;                  // double [2]: their sums in the fixed order of triu_total_kernel
  size_t digit_hist;             // u64 [kSimMaxTargets][256]: the select pass's digit histograms
  size_t count_le;               // u64 [kSimMaxThr + 1]: scores by the number of thresholds at or below them
  size_t minmax;                 // u32 [2]: smallest and largest key
  size_t lut;                    // i8 [3][kSimMaxTargets][256]: slot of a prefix's next digit, -1 none
  size_t thr;                    // float [kSimMaxThr], ascending
  size_t edges;                  // double [kSimMaxBins + 1]
  size_t hist;                   // u64 [kSimMaxBins]
  size_t counters;               // u64 [8]: n_hi, n_lo, tie base hi[2], tie base lo[2]
  size_t row_tie;                // i32 [2][Npad]: a block's per-row copies of the two cut values
  size_t ext;                    // u32 [4][kSimMaxExt][3]: beyond hi, beyond lo, ties hi, ties lo as (key, i, j)
  size_t bytes;
  int64_t npad;
};

inline TriuState triu_state_layout(int64_t N) {
  TriuState s;
  s.npad = (N + kSimRowTile - 1) / kSimRowTile * kSimRowTile;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 15) / 16 * 16; return at; };
  s.row_sum = take((size_t)s.npad * 8);
  s.row_sumsq = take((size_t)s.npad * 8);
  s.total = take(16);
  s.digit_hist = take((size_t)kSimMaxTargets * 256 * 8);
  s.count_le = take((kSimMaxThr + 1) * 8);
  s.minmax = take(8);
  s.lut = take((size_t)3 * kSimMaxTargets * 256);
  s.thr = take(kSimMaxThr * 4);
  s.edges = take((kSimMaxBins + 1) * 8);
  s.hist = take(kSimMaxBins * 8);
  s.counters = take(8 * 8);
  s.row_tie = take((size_t)2 * s.npad * 4);
  s.ext = take((size_t)4 * kSimMaxExt * 3 * 4);
  s.bytes = o;
  return s;
}

// Not linked into the host-only build of the executor (tests/emu) or the sanitizer program: weak,
// checked by the ABI.
hipError_t launch_cosine_affinity(const float* A, long long Na, const float* B, long long Nb, int E, float* out,
                                  long long ldo, hipStream_t s) __attribute__((weak));
// rows [r0, r0 + rows) of the N x N scores in S (row stride N): per row the k best other columns and
// the moments over them.  fp64 sums: thread t of kSimThreads adds columns t, t + kSimThreads, ... in
// ascending order, a wave adds its lanes by a fixed butterfly, thread 0 adds the four waves in order.
hipError_t launch_rows_topk(const float* S, long long r0, long long rows, long long N, int k, float* top_scores,
                            long long* top_index, double* sum, double* sumsq, float* mn, float* mx, float* self,
                            hipStream_t s) __attribute__((weak));
// one pass (0..3) of the triangle select over a block; pass 0 also takes the moments
hipError_t launch_triu_select_pass(const float* S, long long r0, long long rows, long long N, int pass, int n_thr,
                                   void* state, hipStream_t s) __attribute__((weak));
// the rows' fp64 sums added up: thread t of 1024 adds rows t, t + 1024, ... in ascending order, a
// wave adds its lanes by a fixed butterfly, thread 0 adds the sixteen waves in order
hipError_t launch_triu_total(long long N, void* state, hipStream_t s) __attribute__((weak));
// the histogram and the extreme pairs of a block; block_index alternates the tie counters' slots
hipError_t launch_triu_final(const float* S, long long r0, long long rows, long long N, int nbins, unsigned key_hi,
                             int take_hi, unsigned key_lo, int take_lo, int want_ext, long long block_index,
                             void* state, hipStream_t s) __attribute__((weak));

// fp32 bits -> unsigned key with the order of the floats; -0.0 shares the key of +0.0 (score_norm.hip)
inline unsigned sim_key_of_bits(unsigned u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline unsigned sim_bits_of_key(unsigned k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

}  // namespace spk
