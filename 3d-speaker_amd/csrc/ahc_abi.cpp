// C ABI entries of the average-linkage AHC (ahc.hip): argument checks, the workspace layout
// (ahc.h) and the chunked launch loop.  The host enqueues kAhcChunkSteps merge steps at a time
// (never more than the N - 1 merges that can still happen) and reads the run word between
// chunks; once select has cleared it, the rest of a chunk's launches return at their gate.
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
