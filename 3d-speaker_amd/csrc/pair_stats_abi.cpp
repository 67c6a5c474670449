// C ABI entries of the pair-cosine statistics (pair_stats.hip): argument checks, the host-side
// prefix sums and the launch loop.  The group offsets are host memory: they are checked here and
// travel to the kernels as arguments, kPairChunk groups per launch, so the call only enqueues.
// Every check runs before the first launch.
#include "pair_stats.h"
#include "runtime.h"

using namespace spk;

namespace {

int bad(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

int hip_fail(const char* fn, const char* what, hipError_t e) {
  set_error(std::string(fn) + ": " + what + ": " + hipGetErrorString(e));
  return e == hipErrorInvalidValue ? SPK_E_INVALID : SPK_E_HIP;
}

// offsets[0] == 0, non-decreasing, no group above the cap
int check_offsets(const char* fn, const int64_t* offsets, int32_t G) {
  if (offsets[0] != 0) return bad(SPK_E_INVALID, std::string(fn) + ": offsets[0] must be 0");
  for (int32_t g = 0; g < G; ++g)
    if (offsets[g + 1] < offsets[g]) return bad(SPK_E_INVALID, std::string(fn) + ": offsets decrease at group " + std::to_string(g));
  for (int32_t g = 0; g < G; ++g)
    if (offsets[g + 1] - offsets[g] > kPairMaxRows)
      return bad(SPK_E_UNSUPPORTED, std::string(fn) + ": group " + std::to_string(g) + " has " +
                                        std::to_string((long long)(offsets[g + 1] - offsets[g])) +
                                        " rows, above the cap of " + std::to_string((long long)kPairMaxRows));
  return SPK_OK;
}

}  // namespace

extern "C" int spk_pair_cosine_sizes(const int64_t* offsets, int32_t G, int64_t* pair_offsets) {
  if (!offsets || !pair_offsets || G < 0)
    return bad(SPK_E_INVALID, "spk_pair_cosine_sizes: invalid argument (null pointer or G < 0)");
  if (int rc = check_offsets("spk_pair_cosine_sizes", offsets, G)) return rc;
  pair_offsets[0] = 0;
  for (int32_t g = 0; g < G; ++g) pair_offsets[g + 1] = pair_offsets[g] + pair_count(offsets[g + 1] - offsets[g]);
  return SPK_OK;
}

extern "C" int spk_pair_cosine_plan(const int64_t* offsets, int32_t G, int32_t with_cos, int64_t* n_pair_launches,
                                    int64_t* n_stats_launches, int64_t* max_launch_pairs, int64_t* planned_pairs) {
  if (!offsets || !n_pair_launches || !n_stats_launches || !max_launch_pairs || !planned_pairs || G < 0)
    return bad(SPK_E_INVALID, "spk_pair_cosine_plan: invalid argument (null pointer or G < 0)");
  if (int rc = check_offsets("spk_pair_cosine_plan", offsets, G)) return rc;
  int64_t np = 0, ns = 0, mx = 0, total = 0, next = 0;
  int rc = plan_pair_launches(
      offsets, G, with_cos != 0,
      [&](const PairBatchArgs& a, int64_t q0, int64_t q1) {
        // the ranges tile the condensed array in order and stay inside their chunk
        if (q0 != next || q1 <= q0 || q0 < a.pair0[0] || q1 > a.pair0[a.ng]) return 1;
        next = q1;
        ++np;
        total += q1 - q0;
        if (q1 - q0 > mx) mx = q1 - q0;
        return 0;
      },
      [&](const PairBatchArgs&, int32_t) {
        ++ns;
        return 0;
      });
  if (rc) return bad(SPK_E_HIP, "spk_pair_cosine_plan: the plan's pair ranges do not tile the condensed array");
  *n_pair_launches = np;
  *n_stats_launches = ns;
  *max_launch_pairs = mx;
  *planned_pairs = total;
  return SPK_OK;
}

extern "C" int spk_pair_cosine_stats(const float* X, int64_t ldx, int32_t E, const int64_t* offsets, int32_t G,
                                     float threshold, float* cos, float* min, float* mean, int64_t* argmin,
                                     int64_t* n_below, void* stream) {
  if (!offsets || G < 0) return bad(SPK_E_INVALID, "spk_pair_cosine_stats: invalid argument (null offsets or G < 0)");
  if (E <= 0 || E % 4) return bad(SPK_E_INVALID, "spk_pair_cosine_stats: E must be a positive multiple of 4");
  if (ldx < E || ldx % 4)
    return bad(SPK_E_INVALID, "spk_pair_cosine_stats: ldx must be at least E and a multiple of 4 (16-byte rows)");
  if (int rc = check_offsets("spk_pair_cosine_stats", offsets, G)) return rc;
  if (!cos)
    for (int32_t g = 0; g < G; ++g)
      if (offsets[g + 1] - offsets[g] > kPairFusedMaxRows)
        return bad(SPK_E_UNSUPPORTED, "spk_pair_cosine_stats: group " + std::to_string(g) + " has " +
                                          std::to_string((long long)(offsets[g + 1] - offsets[g])) +
                                          " rows; without cos a group is one workgroup's work and is capped at " +
                                          std::to_string((long long)kPairFusedMaxRows) + " rows: pass cos");
  if (G == 0) return SPK_OK;
  if (!min || !mean || !argmin || !n_below || (!X && offsets[G] > 0))
    return bad(SPK_E_INVALID, "spk_pair_cosine_stats: null pointer");
  if (reinterpret_cast<uintptr_t>(X) % 16 != 0)
    return bad(SPK_E_INVALID, "spk_pair_cosine_stats: X must be 16-byte aligned");
  if (!launch_pair_cosine || !launch_pair_stats)
    return bad(SPK_E_UNSUPPORTED, "spk_pair_cosine_stats: this build of the library has no kernels");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return plan_pair_launches(
      offsets, G, cos != nullptr,
      [&](const PairBatchArgs& a, int64_t q0, int64_t q1) {
        if (hipError_t e = launch_pair_cosine(a, q0, q1, X, ldx, E, cos, s))
          return hip_fail("spk_pair_cosine_stats", "pairs", e);
        return SPK_OK;
      },
      [&](const PairBatchArgs& a, int32_t g0) {
        if (hipError_t e = launch_pair_stats(a, X, ldx, E, threshold, cos, min + g0, mean + g0,
                                             reinterpret_cast<long long*>(argmin) + g0,
                                             reinterpret_cast<long long*>(n_below) + g0, s))
          return hip_fail("spk_pair_cosine_stats", "statistics", e);
        return SPK_OK;
      });
}
