// Cohort score normalisation (S-norm / AS-norm): the row blocking of the cohort statistics
// (host, score_norm_abi.cpp) + launchers (score_norm.hip).
#pragma once
#include "common.h"

namespace spk {

// rows of the affinity tile (affinity.hip): a block of cohort scores is a whole number of them
constexpr int64_t kCohortRowTile = 128;
// largest N / Nc the cohort statistics take (the affinity's grid and 32-bit tile arithmetic)
constexpr int64_t kCohortMaxRows = 0x7FFFFFFF;
// recommended block of scores: half of the 256 MiB Infinity Cache, so that the passes of the
// select re-read the block the affinity kernel just wrote from cache instead of from HBM
constexpr size_t kCohortBlockBytes = (size_t)128 << 20;

// smallest workspace: one tile of rows against the whole cohort
inline size_t cohort_min_bytes(int64_t Nc) { return (size_t)kCohortRowTile * (size_t)Nc * sizeof(float); }

// rows per block for a workspace: the largest multiple of the row tile that fits, no more than N
// rounded up (0: below the minimum)
inline int64_t cohort_block_rows(int64_t N, int64_t Nc, size_t workspace_bytes) {
  const size_t row = (size_t)Nc * sizeof(float);
  const int64_t fit = (int64_t)(workspace_bytes / row / kCohortRowTile) * kCohortRowTile;
  const int64_t all = (N + kCohortRowTile - 1) / kCohortRowTile * kCohortRowTile;
  return fit < all ? fit : all;
}

// recommended workspace: blocks of about kCohortBlockBytes, never below the minimum or above N rows
inline size_t cohort_workspace_bytes(int64_t N, int64_t Nc) {
  const size_t want = kCohortBlockBytes > cohort_min_bytes(Nc) ? kCohortBlockBytes : cohort_min_bytes(Nc);
  return (size_t)cohort_block_rows(N, Nc, want) * (size_t)Nc * sizeof(float);
}

// The scores of a row block (affinity.hip; emulated on the host in tests/emu).  Weak here only so
// that a program with the ABI's argument checks alone links (tests/sanitize).
hipError_t launch_cosine_affinity(const float* A, long long Na, const float* B, long long Nb, int E, float* out,
                                  long long ldo, hipStream_t s) __attribute__((weak));
// Not linked into the host-only build of the executor (tests/emu): weak, checked by the ABI.
// mean / std (ddof 0) of the K largest of [0, cols) of every row of S (row stride lds)
hipError_t launch_topk_stats(const float* S, int64_t rows, int64_t cols, int64_t lds, int K, float* mean, float* std,
                             hipStream_t s) __attribute__((weak));
// the trial gather with the normalisation applied to each raw cosine
hipError_t launch_cosine_trials_norm(const float* A, const float* B, int E, const long long* ia, const long long* ib,
                                     long long T, const float* mean_a, const float* std_a, const float* mean_b,
                                     const float* std_b, float* out, hipStream_t s) __attribute__((weak));

}  // namespace spk
