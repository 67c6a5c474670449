// C ABI entries of the cohort score normalisation (score_norm.hip): argument checks, the row
// blocking of the cohort statistics (score_norm.h) and its launch loop.  A block of R rows of X is
// scored against the whole cohort into the caller's workspace by the affinity kernel, reduced to
// its rows' statistics by topk_stats_kernel, and the next block overwrites it behind it on the
// same stream: the N x Nc matrix never exists at once.  Every check runs before the first launch.
#include "score_norm.h"
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

}  // namespace

extern "C" int spk_topk_stats(const float* S, int64_t rows, int64_t cols, int64_t lds, int32_t K, float* mean,
                              float* std, void* stream) {
  if (!S || !mean || !std || rows < 1 || cols < 1 || lds < cols || K < 1 || K > cols)
    return bad(SPK_E_INVALID, "spk_topk_stats: invalid argument (null pointer, rows < 1, cols < 1, lds < cols or K "
                              "outside 1..cols)");
  if (cols > kCohortMaxRows)
    return bad(SPK_E_UNSUPPORTED, "spk_topk_stats: cols = " + std::to_string((long long)cols) + " is above the cap of " +
                                      std::to_string((long long)kCohortMaxRows));
  if (!launch_topk_stats) return bad(SPK_E_UNSUPPORTED, "spk_topk_stats: this build of the library has no kernels");
  if (hipError_t e = launch_topk_stats(S, rows, cols, lds, K, mean, std, reinterpret_cast<hipStream_t>(stream)))
    return hip_fail("spk_topk_stats", "launch", e);
  return SPK_OK;
}

extern "C" int spk_cosine_cohort_stats_workspace_bytes(int64_t N, int64_t Nc, size_t* min_bytes, size_t* bytes) {
  if (!min_bytes || !bytes || N < 1 || Nc < 1)
    return bad(SPK_E_INVALID, "spk_cosine_cohort_stats_workspace_bytes: invalid argument");
  if (N > kCohortMaxRows || Nc > kCohortMaxRows)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_cohort_stats_workspace_bytes: N or Nc is above the cap of " +
                                      std::to_string((long long)kCohortMaxRows));
  *min_bytes = cohort_min_bytes(Nc);
  *bytes = cohort_workspace_bytes(N, Nc);
  return SPK_OK;
}

extern "C" int spk_cosine_cohort_stats(const float* X, int64_t N, const float* C, int64_t Nc, int32_t E, int32_t K,
                                       float* mean, float* std, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  if (!X || !C || !mean || !std || !workspace || N < 1 || Nc < 1 || K < 1 || K > Nc)
    return bad(SPK_E_INVALID, "spk_cosine_cohort_stats: invalid argument (null pointer, N < 1, Nc < 1 or K outside "
                              "1..Nc)");
  if (E <= 0 || E % 4)
    return bad(SPK_E_INVALID, "spk_cosine_cohort_stats: E must be a positive multiple of 4 (spk_cosine_affinity)");
  if (N > kCohortMaxRows || Nc > kCohortMaxRows)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_cohort_stats: N or Nc is above the cap of " +
                                      std::to_string((long long)kCohortMaxRows));
  if (workspace_bytes < cohort_min_bytes(Nc))
    return bad(SPK_E_WORKSPACE, "spk_cosine_cohort_stats: workspace of " + std::to_string(workspace_bytes) +
                                    " bytes, " + std::to_string(cohort_min_bytes(Nc)) + " needed");
  if (reinterpret_cast<uintptr_t>(workspace) % alignof(float) != 0)
    return bad(SPK_E_INVALID, "spk_cosine_cohort_stats: the workspace must be 4-byte aligned");
  if (!launch_cosine_affinity || !launch_topk_stats)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_cohort_stats: this build of the library has no kernels");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* scores = static_cast<float*>(workspace);
  const int64_t R = cohort_block_rows(N, Nc, workspace_bytes);
  for (int64_t r0 = 0; r0 < N; r0 += R) {
    const int64_t rows = N - r0 < R ? N - r0 : R;
    if (hipError_t e = launch_cosine_affinity(X + r0 * E, rows, C, Nc, E, scores, Nc, s))
      return hip_fail("spk_cosine_cohort_stats", "affinity", e);
    if (hipError_t e = launch_topk_stats(scores, rows, Nc, Nc, K, mean + r0, std + r0, s))
      return hip_fail("spk_cosine_cohort_stats", "topk_stats", e);
  }
  return SPK_OK;
}

extern "C" int spk_cosine_trials_norm(const float* Ea, const float* Eb, int32_t E, const int64_t* ia,
                                      const int64_t* ib, int64_t n_trials, const float* mean_a, const float* std_a,
                                      const float* mean_b, const float* std_b, float* scores, void* stream) {
  if (!Ea || !Eb || !ia || !ib || !mean_a || !std_a || !mean_b || !std_b || !scores || n_trials < 1)
    return bad(SPK_E_INVALID, "spk_cosine_trials_norm: invalid argument (null pointer or n_trials < 1)");
  if (E <= 0 || E % 4)
    return bad(SPK_E_INVALID, "spk_cosine_trials_norm: E must be a positive multiple of 4 (spk_cosine_affinity)");
  if (n_trials > 4 * (int64_t)0x7FFFFFFF)
    return bad(SPK_E_INVALID, "spk_cosine_trials_norm: n_trials is above the grid limit");
  if (!launch_cosine_trials_norm)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_trials_norm: this build of the library has no kernels");
  if (hipError_t e = launch_cosine_trials_norm(Ea, Eb, E, reinterpret_cast<const long long*>(ia),
                                               reinterpret_cast<const long long*>(ib), n_trials, mean_a, std_a, mean_b,
                                               std_b, scores, reinterpret_cast<hipStream_t>(stream)))
    return hip_fail("spk_cosine_trials_norm", "launch", e);
  return SPK_OK;
}
