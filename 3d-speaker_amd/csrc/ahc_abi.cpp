// C ABI entries of the average-linkage AHC (ahc.hip): argument checks, the workspace layout
// (ahc.h) and the chunked launch loop.  The host enqueues kAhcChunkSteps merge steps at a time
// (never more than the N - 1 merges that can still happen) and reads the run word between
// chunks; once select has cleared it, the rest of a chunk's launches return at their gate.
// The batched entry (ahc_batched.hip) carves one working matrix per problem from the workspace and
// hands kAhcBatchChunk problems to a launch; it never reads anything back.
#include "ahc.h"
#include "runtime.h"

#include <algorithm>

using namespace spk;

namespace {

int bad(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

int hip_fail(const char* what, hipError_t e) {
  set_error(std::string("spk_ahc_average: ") + what + ": " + hipGetErrorString(e));
  return e == hipErrorInvalidValue ? SPK_E_INVALID : SPK_E_HIP;
}

// SPK_OK, or the code of the first N[p] outside [1, SPK_AHC_BATCH_MAX_N] (spk_last_error set)
int check_batched_sizes(const char* fn, const int64_t* N, int32_t n_prob) {
  for (int32_t p = 0; p < n_prob; ++p) {
    if (N[p] < 1)
      return bad(SPK_E_INVALID, std::string(fn) + ": N[" + std::to_string(p) + "] = " + std::to_string((long long)N[p]) +
                                    " is below 1");
    if (N[p] > SPK_AHC_BATCH_MAX_N)
      return bad(SPK_E_UNSUPPORTED, std::string(fn) + ": N[" + std::to_string(p) + "] = " +
                                        std::to_string((long long)N[p]) + " is above the batched cap of " +
                                        std::to_string(SPK_AHC_BATCH_MAX_N));
  }
  return SPK_OK;
}

}  // namespace

extern "C" int spk_ahc_workspace_bytes(int64_t N, size_t* bytes) {
  if (!bytes || N < 1) return bad(SPK_E_INVALID, "spk_ahc_workspace_bytes: invalid argument");
  if (N > kAhcMaxN)
    return bad(SPK_E_UNSUPPORTED, "spk_ahc_workspace_bytes: N = " + std::to_string((long long)N) + " is above the cap of " +
                                      std::to_string((long long)kAhcMaxN));
  *bytes = ahc_workspace_bytes(N);
  return SPK_OK;
}

extern "C" int spk_ahc_average(const float* S, int64_t N, int64_t lds, float threshold, int32_t* labels,
                               int32_t* n_clusters, void* workspace, size_t workspace_bytes, void* stream) {
  if (!S || !labels || !n_clusters || !workspace || N < 1 || lds < N)
    return bad(SPK_E_INVALID, "spk_ahc_average: invalid argument (null pointer, N < 1 or lds < N)");
  if (N > kAhcMaxN)
    return bad(SPK_E_UNSUPPORTED, "spk_ahc_average: N = " + std::to_string((long long)N) + " is above the cap of " +
                                      std::to_string((long long)kAhcMaxN));
  if (workspace_bytes < ahc_workspace_bytes(N))
    return bad(SPK_E_WORKSPACE, "spk_ahc_average: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                    std::to_string(ahc_workspace_bytes(N)) + " needed");
  if (reinterpret_cast<uintptr_t>(workspace) % alignof(double) != 0)
    return bad(SPK_E_INVALID, "spk_ahc_average: the workspace must be 8-byte aligned");
  if (!launch_ahc_init || !launch_ahc_steps || !launch_ahc_labels)
    return bad(SPK_E_UNSUPPORTED, "spk_ahc_average: this build of the library has no kernels");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const AhcState st = ahc_carve(workspace, N);
  if (hipError_t e = launch_ahc_init(S, N, lds, st, s)) return hip_fail("init", e);
  int64_t left = N - 1;   // merges that can still happen
  while (left > 0) {
    const int steps = (int)std::min<int64_t>(left, kAhcChunkSteps);
    if (hipError_t e = launch_ahc_steps(N, threshold, st, steps, s)) return hip_fail("steps", e);
    left -= steps;
    if (left == 0) break;
    int run = 0;
    if (hipError_t e = hipMemcpyAsync(&run, st.ctrl + AHC_RUN, sizeof(int), hipMemcpyDeviceToHost, s))
      return hip_fail("hipMemcpyAsync", e);
    if (hipError_t e = hipStreamSynchronize(s)) return hip_fail("hipStreamSynchronize", e);
    if (!run) break;
  }
  if (hipError_t e = launch_ahc_labels(N, st, labels, n_clusters, s)) return hip_fail("labels", e);
  return SPK_OK;
}

extern "C" int spk_ahc_batched_max_n(void) { return SPK_AHC_BATCH_MAX_N; }

extern "C" int spk_ahc_average_batched_workspace_bytes(const int64_t* N, int32_t n_prob, size_t* bytes) {
  const char* fn = "spk_ahc_average_batched_workspace_bytes";
  if (!bytes || n_prob < 0 || (n_prob > 0 && !N)) return bad(SPK_E_INVALID, std::string(fn) + ": invalid argument");
  if (int rc = check_batched_sizes(fn, N, n_prob)) return rc;
  size_t total = 0;
  for (int32_t p = 0; p < n_prob; ++p) total += ahc_batched_matrix_bytes(N[p]);
  *bytes = total;
  return SPK_OK;
}

extern "C" int spk_ahc_average_batched(const float* const* S, const int64_t* N, const int64_t* lds,
                                       const float* threshold, int32_t n_prob, int32_t* const* labels,
                                       int32_t* n_clusters, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "spk_ahc_average_batched";
  if (n_prob < 0) return bad(SPK_E_INVALID, std::string(fn) + ": n_prob < 0");
  if (n_prob == 0) return SPK_OK;
  if (!S || !N || !lds || !threshold || !labels || !n_clusters || !workspace)
    return bad(SPK_E_INVALID, std::string(fn) + ": invalid argument (null pointer)");
  if (int rc = check_batched_sizes(fn, N, n_prob)) return rc;
  size_t need = 0;
  for (int32_t p = 0; p < n_prob; ++p) {
    if (!S[p] || !labels[p] || lds[p] < N[p])
      return bad(SPK_E_INVALID, std::string(fn) + ": problem " + std::to_string(p) + ": null pointer or lds < N");
    need += ahc_batched_matrix_bytes(N[p]);
  }
  if (workspace_bytes < need)
    return bad(SPK_E_WORKSPACE, std::string(fn) + ": workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                    std::to_string(need) + " needed");
  if (reinterpret_cast<uintptr_t>(workspace) % alignof(double) != 0)
    return bad(SPK_E_INVALID, std::string(fn) + ": the workspace must be 8-byte aligned");
  if (!launch_ahc_batched) return bad(SPK_E_UNSUPPORTED, std::string(fn) + ": this build of the library has no kernels");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* at = reinterpret_cast<char*>(workspace);
  for (int32_t lo = 0; lo < n_prob; lo += kAhcBatchChunk) {
    AhcBatchArgs a;
    a.n = (int)std::min<int32_t>(n_prob - lo, kAhcBatchChunk);
    a.n_clusters = n_clusters + lo;
    for (int q = 0; q < a.n; ++q) {
      const int32_t p = lo + q;
      a.p[q] = AhcBatchProb{S[p], labels[p], reinterpret_cast<double*>(at), (long long)lds[p], (int)N[p], threshold[p]};
      at += ahc_batched_matrix_bytes(N[p]);
    }
    for (int q = a.n; q < kAhcBatchChunk; ++q) a.p[q] = AhcBatchProb{nullptr, nullptr, nullptr, 0, 0, 0.f};
    if (hipError_t e = launch_ahc_batched(a, s)) {
      set_error(std::string(fn) + ": launch: " + hipGetErrorString(e));
      return e == hipErrorInvalidValue ? SPK_E_INVALID : SPK_E_HIP;
    }
  }
  return SPK_OK;
}
