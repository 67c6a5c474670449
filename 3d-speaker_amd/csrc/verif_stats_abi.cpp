// C ABI entries of the all-pairs verification statistics (verif_stats.hip): argument checks, the row
// blocking of sim_stats.h, the prefix tables of the digits pass and the launch loops.  A block of R
// rows of X is scored against all of X into the caller's workspace by the affinity kernel, consumed
// by one class-aware kernel, and overwritten by the next block behind it on the same stream: the
// N x N matrix never exists at once.  Every check of the host arguments runs before the first
// launch; the labels live on the device, so their smallest value is fetched by one small kernel
// before any pass.  Outputs (host memory) are written only once everything has succeeded.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "verif_stats.h"
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

// what the two passes share: X, labels, N, E, the workspace and the state.  0 or the error code.
int check_common(const char* fn, const float* X, const int32_t* labels, int64_t N, int32_t E, const void* workspace,
                 size_t workspace_bytes, const void* state, size_t state_bytes) {
  const std::string f(fn);
  if (!X || !labels || !workspace || N < 1)
    return bad(SPK_E_INVALID, f + ": invalid argument (null pointer or N < 1)");
  if (E <= 0 || E % 4) return bad(SPK_E_INVALID, f + ": E must be a positive multiple of 4 (spk_cosine_affinity)");
  if (reinterpret_cast<uintptr_t>(X) % 16 != 0) return bad(SPK_E_INVALID, f + ": X must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(labels) % alignof(int32_t) != 0 ||
      reinterpret_cast<uintptr_t>(workspace) % alignof(float) != 0)
    return bad(SPK_E_INVALID, f + ": labels and the workspace must be 4-byte aligned");
  if (N > kSimMaxRows)
    return bad(SPK_E_UNSUPPORTED, f + ": N = " + std::to_string((long long)N) + " is above the cap of " +
                                      std::to_string((long long)kSimMaxRows));
  if (workspace_bytes < sim_min_bytes(N))
    return bad(SPK_E_WORKSPACE, f + ": workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                    std::to_string(sim_min_bytes(N)) + " needed");
  // every launch's grid in work-items against 2^31 (sim_stats.h): a block of at least one row tile
  if (sim_block_rows(N, workspace_bytes) < kSimRowTile)
    return bad(SPK_E_UNSUPPORTED, f + ": N = " + std::to_string((long long)N) +
                                      " needs more than 2^31 work-items for one tile of rows");
  if (!state || reinterpret_cast<uintptr_t>(state) % 16 != 0)
    return bad(SPK_E_INVALID, f + ": the state must be a 16-byte aligned device buffer");
  if (state_bytes < verif_state_layout(N).bytes)
    return bad(SPK_E_WORKSPACE, f + ": state of " + std::to_string(state_bytes) + " bytes, " +
                                    std::to_string(verif_state_layout(N).bytes) + " needed");
  return SPK_OK;
}

// On an error the stream is drained before the return: copies into the frame's buffers may be in flight.
#define SPK_VERIF_HIP(call, what)          \
  if (hipError_t e_ = (call)) {            \
    (void)hipStreamSynchronize(s);         \
    return hip_fail(fn, what, e_);         \
  }

// the smallest label, fetched before any pass; SPK_E_INVALID when it is negative
int check_labels(const char* fn, const int32_t* labels, int64_t N, void* state, hipStream_t s) {
  char* st = static_cast<char*>(state);
  const VerifState lay = verif_state_layout(N);
  const int32_t init[4] = {std::numeric_limits<int32_t>::max(), 0, 0, 0};
  int32_t got[4] = {0, 0, 0, 0};
  SPK_VERIF_HIP(hipMemcpyAsync(st + lay.flag, init, sizeof(init), hipMemcpyHostToDevice, s), "upload");
  SPK_VERIF_HIP(launch_verif_label_min(labels, N, state, s), "label check");
  SPK_VERIF_HIP(hipMemcpyAsync(got, st + lay.flag, sizeof(got), hipMemcpyDeviceToHost, s), "download");
  SPK_VERIF_HIP(hipStreamSynchronize(s), "synchronize");
  if (got[0] < 0) return bad(SPK_E_INVALID, std::string(fn) + ": a label is negative");
  return SPK_OK;
}

}  // namespace

extern "C" int spk_cosine_verif_workspace_bytes(int64_t N, size_t* min_bytes, size_t* bytes, size_t* state_bytes) {
  if (!min_bytes || !bytes || !state_bytes || N < 1)
    return bad(SPK_E_INVALID, "spk_cosine_verif_workspace_bytes: invalid argument (null pointer or N < 1)");
  if (N > kSimMaxRows)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_verif_workspace_bytes: N is above the cap of " +
                                      std::to_string((long long)kSimMaxRows));
  if (sim_block_rows(N, sim_min_bytes(N)) < kSimRowTile)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_verif_workspace_bytes: N needs more than 2^31 work-items for one tile of "
                                  "rows");
  *min_bytes = sim_min_bytes(N);
  *bytes = sim_workspace_bytes(N);
  *state_bytes = verif_state_layout(N).bytes;
  return SPK_OK;
}

extern "C" int spk_cosine_verif_moments(const float* X, const int32_t* labels, int64_t N, int32_t E, const double* edges,
                                        int32_t nbins, int64_t* count, double* sum, double* sumsq, float* min, float* max,
                                        int64_t* hist, void* workspace, size_t workspace_bytes, void* state,
                                        size_t state_bytes, void* stream) {
  const char* fn = "spk_cosine_verif_moments";
  if (!count || !sum || !sumsq || !min || !max) return bad(SPK_E_INVALID, "spk_cosine_verif_moments: null output pointer");
  if (nbins < 0 || nbins > kSimMaxBins || (nbins > 0 && (!edges || !hist)))
    return bad(SPK_E_INVALID, "spk_cosine_verif_moments: nbins must be in 0..256, with edges and hist");
  for (int b = 0; b <= nbins && nbins > 0; ++b)
    if (!std::isfinite(edges[b]) || (b > 0 && edges[b] < edges[b - 1]))
      return bad(SPK_E_INVALID, "spk_cosine_verif_moments: edges must be finite and ascending");
  if (int rc = check_common(fn, X, labels, N, E, workspace, workspace_bytes, state, state_bytes)) return rc;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const double dnan = std::numeric_limits<double>::quiet_NaN();
  if (sim_pairs(N) == 0) {   // N == 1: no pair
    for (int c = 0; c < 2; ++c) {
      count[c] = 0;
      sum[c] = sumsq[c] = dnan;
      min[c] = max[c] = nan;
    }
    for (int b = 0; b < 2 * nbins; ++b) hist[b] = 0;
    return SPK_OK;
  }
  if (!launch_cosine_affinity || !launch_verif_label_min || !launch_verif_moments || !launch_verif_total)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_verif_moments: this build of the library has no kernels");

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = check_labels(fn, labels, N, state, s)) return rc;
  float* scores = static_cast<float*>(workspace);
  char* st = static_cast<char*>(state);
  const VerifState lay = verif_state_layout(N);
  const int64_t R = sim_block_rows(N, workspace_bytes);
  const unsigned minmax0[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
  unsigned minmax[4];
  double total[4];
  unsigned long long cnt[2];
  std::vector<unsigned long long> h((size_t)2 * kSimMaxBins);

  SPK_VERIF_HIP(hipMemsetAsync(st + lay.count, 0, sizeof(cnt), s), "memset");
  SPK_VERIF_HIP(hipMemsetAsync(st + lay.hist, 0, h.size() * 8, s), "memset");
  SPK_VERIF_HIP(hipMemcpyAsync(st + lay.minmax, minmax0, sizeof(minmax0), hipMemcpyHostToDevice, s), "upload");
  if (nbins > 0)
    SPK_VERIF_HIP(hipMemcpyAsync(st + lay.edges, edges, (size_t)(nbins + 1) * 8, hipMemcpyHostToDevice, s), "upload");
  for (int64_t r0 = 0; r0 < N; r0 += R) {
    const int64_t rows = N - r0 < R ? N - r0 : R;
    SPK_VERIF_HIP(launch_cosine_affinity(X + r0 * E, rows, X, N, E, scores, N, s), "affinity");
    SPK_VERIF_HIP(launch_verif_moments(scores, labels, r0, rows, N, nbins, state, s), "moments");
  }
  SPK_VERIF_HIP(launch_verif_total(N, state, s), "total");
  SPK_VERIF_HIP(hipMemcpyAsync(total, st + lay.total, sizeof(total), hipMemcpyDeviceToHost, s), "download");
  SPK_VERIF_HIP(hipMemcpyAsync(minmax, st + lay.minmax, sizeof(minmax), hipMemcpyDeviceToHost, s), "download");
  SPK_VERIF_HIP(hipMemcpyAsync(cnt, st + lay.count, sizeof(cnt), hipMemcpyDeviceToHost, s), "download");
  SPK_VERIF_HIP(hipMemcpyAsync(h.data(), st + lay.hist, h.size() * 8, hipMemcpyDeviceToHost, s), "download");
  SPK_VERIF_HIP(hipStreamSynchronize(s), "synchronize");

  for (int c = 0; c < 2; ++c) {
    count[c] = (int64_t)cnt[c];
    if (cnt[c] == 0) {
      sum[c] = total[c];       // 0.0: nothing was added
      sumsq[c] = total[2 + c];
      min[c] = max[c] = nan;
      continue;
    }
    sum[c] = total[c];
    sumsq[c] = total[2 + c];
    unsigned bits = sim_bits_of_key(minmax[c]);
    std::memcpy(min + c, &bits, 4);
    bits = sim_bits_of_key(minmax[2 + c]);
    std::memcpy(max + c, &bits, 4);
  }
  for (int c = 0; c < 2; ++c)
    for (int b = 0; b < nbins; ++b) hist[(size_t)c * nbins + b] = (int64_t)h[(size_t)c * kSimMaxBins + b];
  return SPK_OK;
}

extern "C" int spk_cosine_verif_digits(const float* X, const int32_t* labels, int64_t N, int32_t E, int32_t level,
                                       const uint32_t* prefixes, int32_t n_prefix, int64_t* digits, void* workspace,
                                       size_t workspace_bytes, void* state, size_t state_bytes, void* stream) {
  const char* fn = "spk_cosine_verif_digits";
  if (!digits) return bad(SPK_E_INVALID, "spk_cosine_verif_digits: null output pointer");
  if (level < 0 || level > 3) return bad(SPK_E_INVALID, "spk_cosine_verif_digits: level must be in 0..3");
  if (level == 0 ? n_prefix != 1 : (n_prefix < 1 || n_prefix > kVerifMaxPrefixes || !prefixes))
    return bad(SPK_E_INVALID, "spk_cosine_verif_digits: n_prefix must be 1 at level 0 and in 1..16 above it, with prefixes");
  if (int rc = check_common(fn, X, labels, N, E, workspace, workspace_bytes, state, state_bytes)) return rc;
  const size_t n_out = (size_t)n_prefix * 2 * 256;
  if (sim_pairs(N) == 0) {
    for (size_t q = 0; q < n_out; ++q) digits[q] = 0;
    return SPK_OK;
  }
  if (!launch_cosine_affinity || !launch_verif_label_min || !launch_verif_digits)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_verif_digits: this build of the library has no kernels");

  // The tables (sim_stats_abi.cpp's scheme): table t maps (slot after t digits, digit t) to the slot
  // after t + 1 digits, -1 where no prefix goes on.  Equal prefixes share their last slot.
  std::vector<signed char> lut((size_t)3 * kVerifMaxPrefixes * 256, (signed char)-1);
  int slot_of[kVerifMaxPrefixes] = {};
  int n_slots = 1;
  if (level > 0) {
    int cur[kVerifMaxPrefixes] = {};
    for (int t = 0; t < level; ++t) {
      signed char* table = lut.data() + (size_t)t * kVerifMaxPrefixes * 256;
      int slots = 0;
      for (int p = 0; p < n_prefix; ++p) {
        signed char& e = table[(size_t)cur[p] * 256 + ((prefixes[p] >> (24 - 8 * t)) & 255u)];
        if (e < 0) e = (signed char)slots++;
        cur[p] = e;
      }
      n_slots = slots;
    }
    for (int p = 0; p < n_prefix; ++p) slot_of[p] = cur[p];
  }

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = check_labels(fn, labels, N, state, s)) return rc;
  float* scores = static_cast<float*>(workspace);
  char* st = static_cast<char*>(state);
  const VerifState lay = verif_state_layout(N);
  const int64_t R = sim_block_rows(N, workspace_bytes);
  std::vector<unsigned long long> h((size_t)n_slots * 2 * 256);

  SPK_VERIF_HIP(hipMemsetAsync(st + lay.digits, 0, h.size() * 8, s), "memset");
  if (level > 0)
    SPK_VERIF_HIP(hipMemcpyAsync(st + lay.lut, lut.data(), (size_t)level * kVerifMaxPrefixes * 256, hipMemcpyHostToDevice, s),
                  "upload");
  for (int64_t r0 = 0; r0 < N; r0 += R) {
    const int64_t rows = N - r0 < R ? N - r0 : R;
    SPK_VERIF_HIP(launch_cosine_affinity(X + r0 * E, rows, X, N, E, scores, N, s), "affinity");
    SPK_VERIF_HIP(launch_verif_digits(scores, labels, r0, rows, N, level, n_slots, state, s), "digits");
  }
  SPK_VERIF_HIP(hipMemcpyAsync(h.data(), st + lay.digits, h.size() * 8, hipMemcpyDeviceToHost, s), "download");
  SPK_VERIF_HIP(hipStreamSynchronize(s), "synchronize");

  for (int p = 0; p < n_prefix; ++p)
    for (int q = 0; q < 512; ++q) digits[(size_t)p * 512 + q] = (int64_t)h[(size_t)slot_of[p] * 512 + q];
  return SPK_OK;
}
#undef SPK_VERIF_HIP
