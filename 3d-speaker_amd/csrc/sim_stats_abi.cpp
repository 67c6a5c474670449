// C ABI entries of the corpus similarity statistics (sim_stats.hip): argument checks, the row
// blocking (sim_stats.h), the launch loops and the host side of the multi-target radix select.  A
// block of R rows of X is scored against all of X into the caller's workspace by the affinity
// kernel, consumed by the statistics' kernels, and overwritten by the next block behind it on the
// same stream: the N x N matrix never exists at once.  Every check runs before the first launch,
// and the triangle entries write their (host) outputs only once everything has succeeded.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "sim_stats.h"
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

// what the three entries share: X, N, E, the workspace.  0 or the error code.
int check_common(const char* fn, const float* X, int64_t N, int32_t E, const void* workspace, size_t workspace_bytes) {
  const std::string f(fn);
  if (!X || !workspace || N < 1) return bad(SPK_E_INVALID, f + ": invalid argument (null pointer or N < 1)");
  if (E <= 0 || E % 4) return bad(SPK_E_INVALID, f + ": E must be a positive multiple of 4 (spk_cosine_affinity)");
  if (reinterpret_cast<uintptr_t>(X) % 16 != 0) return bad(SPK_E_INVALID, f + ": X must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(workspace) % alignof(float) != 0)
    return bad(SPK_E_INVALID, f + ": the workspace must be 4-byte aligned");
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
  return SPK_OK;
}

int check_state(const char* fn, int64_t N, const void* state, size_t state_bytes) {
  const std::string f(fn);
  if (!state || reinterpret_cast<uintptr_t>(state) % 16 != 0)
    return bad(SPK_E_INVALID, f + ": the state must be a 16-byte aligned device buffer");
  if (state_bytes < triu_state_layout(N).bytes)
    return bad(SPK_E_WORKSPACE, f + ": state of " + std::to_string(state_bytes) + " bytes, " +
                                    std::to_string(triu_state_layout(N).bytes) + " needed");
  return SPK_OK;
}

struct Target {
  int64_t rank;        // 0-based ascending rank among the entries that share the prefix
  int64_t below = 0;   // entries strictly below the prefix's range
  int64_t equal = 0;   // entries in the bin picked last
  unsigned prefix = 0;
  int slot = 0;
};

}  // namespace

extern "C" int spk_cosine_sim_workspace_bytes(int64_t N, size_t* min_bytes, size_t* bytes, size_t* state_bytes) {
  if (!min_bytes || !bytes || !state_bytes || N < 1)
    return bad(SPK_E_INVALID, "spk_cosine_sim_workspace_bytes: invalid argument (null pointer or N < 1)");
  if (N > kSimMaxRows)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_sim_workspace_bytes: N is above the cap of " +
                                      std::to_string((long long)kSimMaxRows));
  if (sim_block_rows(N, sim_min_bytes(N)) < kSimRowTile)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_sim_workspace_bytes: N needs more than 2^31 work-items for one tile of "
                                  "rows");
  *min_bytes = sim_min_bytes(N);
  *bytes = sim_workspace_bytes(N);
  *state_bytes = triu_state_layout(N).bytes;
  return SPK_OK;
}

extern "C" int spk_cosine_rows_topk(const float* X, int64_t N, int32_t E, int32_t k, float* top_scores,
                                    int64_t* top_index, double* sum, double* sumsq, float* min, float* max, float* self,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "spk_cosine_rows_topk";
  if (!top_scores || !top_index || !sum || !sumsq || !min || !max || !self)
    return bad(SPK_E_INVALID, "spk_cosine_rows_topk: null output pointer");
  if (k < 1 || k > kSimMaxK) return bad(SPK_E_INVALID, "spk_cosine_rows_topk: k must be in 1..1024");
  if (int rc = check_common(fn, X, N, E, workspace, workspace_bytes)) return rc;
  if (!launch_cosine_affinity || !launch_rows_topk)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_rows_topk: this build of the library has no kernels");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* scores = static_cast<float*>(workspace);
  const int64_t R = sim_block_rows(N, workspace_bytes);
  for (int64_t r0 = 0; r0 < N; r0 += R) {
    const int64_t rows = N - r0 < R ? N - r0 : R;
    if (hipError_t e = launch_cosine_affinity(X + r0 * E, rows, X, N, E, scores, N, s)) return hip_fail(fn, "affinity", e);
    if (hipError_t e = launch_rows_topk(scores, r0, rows, N, k, top_scores, reinterpret_cast<long long*>(top_index), sum,
                                        sumsq, min, max, self, s))
      return hip_fail(fn, "top-k", e);
  }
  return SPK_OK;
}

extern "C" int spk_cosine_triu_stats(const float* X, int64_t N, int32_t E, const float* thresholds, int32_t n_thr,
                                     const int64_t* ranks, int32_t n_ranks, int32_t n_ext, int64_t* count, double* sum,
                                     double* sumsq, float* min, float* max, int64_t* count_ge, float* order_stats,
                                     float* ext_cut, int32_t* ext_take, void* workspace, size_t workspace_bytes,
                                     void* state, size_t state_bytes, void* stream) {
  const char* fn = "spk_cosine_triu_stats";
  if (!count || !sum || !sumsq || !min || !max || !ext_cut || !ext_take)
    return bad(SPK_E_INVALID, "spk_cosine_triu_stats: null output pointer");
  if (n_thr < 0 || n_thr > kSimMaxThr || (n_thr > 0 && (!thresholds || !count_ge)))
    return bad(SPK_E_INVALID, "spk_cosine_triu_stats: n_thr must be in 0..32, with thresholds and count_ge");
  if (n_ranks < 0 || n_ranks > kSimMaxRanks || (n_ranks > 0 && (!ranks || !order_stats)))
    return bad(SPK_E_INVALID, "spk_cosine_triu_stats: n_ranks must be in 0..16, with ranks and order_stats");
  if (n_ext < 0 || n_ext > kSimMaxExt) return bad(SPK_E_INVALID, "spk_cosine_triu_stats: n_ext must be in 0..4096");
  for (int t = 0; t < n_thr; ++t)
    if (std::isnan(thresholds[t])) return bad(SPK_E_INVALID, "spk_cosine_triu_stats: a threshold is NaN");
  if (int rc = check_common(fn, X, N, E, workspace, workspace_bytes)) return rc;
  const int64_t P = sim_pairs(N);
  for (int t = 0; t < n_ranks; ++t)
    if (ranks[t] < 0 || ranks[t] >= P || (t > 0 && ranks[t] < ranks[t - 1]))
      return bad(SPK_E_INVALID, "spk_cosine_triu_stats: ranks must be ascending and below the number of pairs");
  if (int rc = check_state(fn, N, state, state_bytes)) return rc;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  if (P == 0) {   // N == 1: no pair
    *count = 0;
    *sum = *sumsq = std::numeric_limits<double>::quiet_NaN();
    *min = *max = nan;
    for (int t = 0; t < n_thr; ++t) count_ge[t] = 0;
    ext_cut[0] = ext_cut[1] = nan;
    ext_take[0] = ext_take[1] = 0;
    return SPK_OK;
  }
  if (!launch_cosine_affinity || !launch_triu_select_pass || !launch_triu_total)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_triu_stats: this build of the library has no kernels");

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* scores = static_cast<float*>(workspace);
  char* st = static_cast<char*>(state);
  const TriuState lay = triu_state_layout(N);
  const int64_t R = sim_block_rows(N, workspace_bytes);

  // thresholds ascending for the kernel's binary search; order[] maps back
  std::vector<int> order(n_thr);
  for (int t = 0; t < n_thr; ++t) order[t] = t;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return thresholds[a] < thresholds[b]; });
  float thr_sorted[kSimMaxThr] = {};
  for (int t = 0; t < n_thr; ++t) thr_sorted[t] = thresholds[order[t]];

  // the targets: the caller's ranks, then the cuts of the largest and the smallest n_eff pairs
  const int64_t n_eff = (int64_t)n_ext < P ? (int64_t)n_ext : P;
  std::vector<Target> tg;
  for (int t = 0; t < n_ranks; ++t) tg.push_back(Target{ranks[t]});
  if (n_eff > 0) {
    tg.push_back(Target{P - n_eff});
    tg.push_back(Target{n_eff - 1});
  }
  const int passes = tg.empty() ? 1 : 4;

  std::vector<signed char> lut((size_t)3 * kSimMaxTargets * 256, (signed char)-1);
  std::vector<unsigned long long> hist((size_t)kSimMaxTargets * 256);
  const unsigned minmax0[2] = {0xFFFFFFFFu, 0u};
  unsigned minmax[2];
  double total[2];
  unsigned long long count_le[kSimMaxThr + 1] = {};

// On an error the stream is drained before the return: copies into this frame's buffers may be in flight.
#define SPK_SIM_HIP(call, what)            \
  if (hipError_t e_ = (call)) {            \
    (void)hipStreamSynchronize(s);         \
    return hip_fail(fn, what, e_);         \
  }
  SPK_SIM_HIP(hipMemsetAsync(st + lay.count_le, 0, sizeof(count_le), s), "memset");
  SPK_SIM_HIP(hipMemcpyAsync(st + lay.minmax, minmax0, sizeof(minmax0), hipMemcpyHostToDevice, s), "upload");
  SPK_SIM_HIP(hipMemcpyAsync(st + lay.thr, thr_sorted, sizeof(thr_sorted), hipMemcpyHostToDevice, s), "upload");
  for (int pass = 0; pass < passes; ++pass) {
    SPK_SIM_HIP(hipMemsetAsync(st + lay.digit_hist, 0, hist.size() * 8, s), "memset");
    if (pass > 0) SPK_SIM_HIP(hipMemcpyAsync(st + lay.lut, lut.data(), lut.size(), hipMemcpyHostToDevice, s), "upload");
    for (int64_t r0 = 0; r0 < N; r0 += R) {
      const int64_t rows = N - r0 < R ? N - r0 : R;
      SPK_SIM_HIP(launch_cosine_affinity(X + r0 * E, rows, X, N, E, scores, N, s), "affinity");
      SPK_SIM_HIP(launch_triu_select_pass(scores, r0, rows, N, pass, n_thr, state, s), "select pass");
    }
    if (pass == 0) {
      SPK_SIM_HIP(launch_triu_total(N, state, s), "total");
      SPK_SIM_HIP(hipMemcpyAsync(total, st + lay.total, sizeof(total), hipMemcpyDeviceToHost, s), "download");
      SPK_SIM_HIP(hipMemcpyAsync(minmax, st + lay.minmax, sizeof(minmax), hipMemcpyDeviceToHost, s), "download");
      SPK_SIM_HIP(hipMemcpyAsync(count_le, st + lay.count_le, sizeof(count_le), hipMemcpyDeviceToHost, s), "download");
    }
    SPK_SIM_HIP(hipMemcpyAsync(hist.data(), st + lay.digit_hist, hist.size() * 8, hipMemcpyDeviceToHost, s), "download");
    SPK_SIM_HIP(hipStreamSynchronize(s), "synchronize");
    if (tg.empty()) break;
    // every target's bin of this digit among the entries that share its prefix
    const int shift = 24 - 8 * pass;
    for (Target& t : tg) {
      const unsigned long long* h = hist.data() + (size_t)t.slot * 256;
      int64_t cum = 0;
      int b = 0;
      for (; b < 255 && cum + (int64_t)h[b] <= t.rank; ++b) cum += (int64_t)h[b];
      if (cum + (int64_t)h[b] <= t.rank)   // after the pass's synchronisation: nothing is in flight
        return bad(SPK_E_HIP, "spk_cosine_triu_stats: the select's histogram does not cover its rank");
      t.below += cum;
      t.rank -= cum;
      t.equal = (int64_t)h[b];
      t.prefix |= (unsigned)b << shift;
    }
    if (pass < 3) {
      // a slot per distinct prefix; the table of this level maps (old slot, digit) to it
      signed char* level = lut.data() + (size_t)pass * kSimMaxTargets * 256;
      int slots = 0;
      for (Target& t : tg) {
        signed char& e = level[(size_t)t.slot * 256 + ((t.prefix >> shift) & 255u)];
        if (e < 0) e = (signed char)slots++;
        t.slot = e;
      }
    }
  }
#undef SPK_SIM_HIP

  *count = P;
  *sum = total[0];
  *sumsq = total[1];
  unsigned bits = sim_bits_of_key(minmax[0]);
  std::memcpy(min, &bits, 4);
  bits = sim_bits_of_key(minmax[1]);
  std::memcpy(max, &bits, 4);
  // count_le[b]: scores with exactly b thresholds at or below them; >= the t-th smallest: b > t
  for (int t = 0; t < n_thr; ++t) {
    unsigned long long c = 0;
    for (int b = t + 1; b <= n_thr; ++b) c += count_le[b];
    count_ge[order[t]] = (int64_t)c;
  }
  for (int t = 0; t < n_ranks; ++t) {
    bits = sim_bits_of_key(tg[t].prefix);
    std::memcpy(order_stats + t, &bits, 4);
  }
  if (n_eff > 0) {
    const Target &hi = tg[n_ranks], &lo = tg[n_ranks + 1];
    bits = sim_bits_of_key(hi.prefix);
    std::memcpy(ext_cut, &bits, 4);
    bits = sim_bits_of_key(lo.prefix);
    std::memcpy(ext_cut + 1, &bits, 4);
    ext_take[0] = (int32_t)(n_eff - (P - hi.below - hi.equal));   // n_eff less the pairs above the cut
    ext_take[1] = (int32_t)(n_eff - lo.below);
  } else {
    ext_cut[0] = ext_cut[1] = nan;
    ext_take[0] = ext_take[1] = 0;
  }
  return SPK_OK;
}

extern "C" int spk_cosine_triu_hist(const float* X, int64_t N, int32_t E, const double* edges, int32_t nbins,
                                    int32_t n_ext, const float* ext_cut, const int32_t* ext_take, int64_t* hist,
                                    float* ext_scores, int64_t* ext_i, int64_t* ext_j, int32_t* n_found,
                                    void* workspace, size_t workspace_bytes, void* state, size_t state_bytes,
                                    void* stream) {
  const char* fn = "spk_cosine_triu_hist";
  if (nbins < 0 || nbins > kSimMaxBins || (nbins > 0 && (!edges || !hist)))
    return bad(SPK_E_INVALID, "spk_cosine_triu_hist: nbins must be in 0..256, with edges and hist");
  if (n_ext < 0 || n_ext > kSimMaxExt || !n_found || (n_ext > 0 && (!ext_cut || !ext_take || !ext_scores || !ext_i || !ext_j)))
    return bad(SPK_E_INVALID, "spk_cosine_triu_hist: n_ext must be in 0..4096, with the cuts and the outputs");
  for (int b = 0; b <= nbins && nbins > 0; ++b)
    if (!std::isfinite(edges[b]) || (b > 0 && edges[b] < edges[b - 1]))
      return bad(SPK_E_INVALID, "spk_cosine_triu_hist: edges must be finite and ascending");
  if (int rc = check_common(fn, X, N, E, workspace, workspace_bytes)) return rc;
  if (int rc = check_state(fn, N, state, state_bytes)) return rc;
  const int64_t P = sim_pairs(N);
  const int64_t n_eff = (int64_t)n_ext < P ? (int64_t)n_ext : P;
  if (n_eff > 0 && (std::isnan(ext_cut[0]) || std::isnan(ext_cut[1]) || ext_take[0] < 1 || ext_take[0] > n_eff ||
                    ext_take[1] < 1 || ext_take[1] > n_eff))
    return bad(SPK_E_INVALID, "spk_cosine_triu_hist: the cuts are not those spk_cosine_triu_stats gives for n_ext");
  if (P == 0) {
    for (int b = 0; b < nbins; ++b) hist[b] = 0;
    n_found[0] = n_found[1] = 0;
    return SPK_OK;
  }
  if (!launch_cosine_affinity || !launch_triu_final)
    return bad(SPK_E_UNSUPPORTED, "spk_cosine_triu_hist: this build of the library has no kernels");

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* scores = static_cast<float*>(workspace);
  char* st = static_cast<char*>(state);
  const TriuState lay = triu_state_layout(N);
  const int64_t R = sim_block_rows(N, workspace_bytes);
  unsigned key[2] = {0u, 0u};
  int take[2] = {0, 0};
  if (n_eff > 0)
    for (int w = 0; w < 2; ++w) {
      unsigned bits;
      std::memcpy(&bits, ext_cut + w, 4);
      key[w] = sim_key_of_bits(bits);
      take[w] = ext_take[w];
    }
  std::vector<unsigned long long> h(kSimMaxBins);
  unsigned long long counters[8];
  std::vector<unsigned> ext((size_t)4 * kSimMaxExt * 3);

// On an error the stream is drained before the return: copies into this frame's buffers may be in flight.
#define SPK_SIM_HIP(call, what)            \
  if (hipError_t e_ = (call)) {            \
    (void)hipStreamSynchronize(s);         \
    return hip_fail(fn, what, e_);         \
  }
  SPK_SIM_HIP(hipMemsetAsync(st + lay.hist, 0, kSimMaxBins * 8, s), "memset");
  SPK_SIM_HIP(hipMemsetAsync(st + lay.counters, 0, sizeof(counters), s), "memset");
  if (nbins > 0)
    SPK_SIM_HIP(hipMemcpyAsync(st + lay.edges, edges, (size_t)(nbins + 1) * 8, hipMemcpyHostToDevice, s), "upload");
  int64_t block = 0;
  for (int64_t r0 = 0; r0 < N; r0 += R, ++block) {
    const int64_t rows = N - r0 < R ? N - r0 : R;
    SPK_SIM_HIP(launch_cosine_affinity(X + r0 * E, rows, X, N, E, scores, N, s), "affinity");
    SPK_SIM_HIP(launch_triu_final(scores, r0, rows, N, nbins, key[0], take[0], key[1], take[1], n_eff > 0, block, state, s),
                "histogram and extremes");
  }
  SPK_SIM_HIP(hipMemcpyAsync(h.data(), st + lay.hist, kSimMaxBins * 8, hipMemcpyDeviceToHost, s), "download");
  SPK_SIM_HIP(hipMemcpyAsync(counters, st + lay.counters, sizeof(counters), hipMemcpyDeviceToHost, s), "download");
  if (n_eff > 0) SPK_SIM_HIP(hipMemcpyAsync(ext.data(), st + lay.ext, ext.size() * 4, hipMemcpyDeviceToHost, s), "download");
  SPK_SIM_HIP(hipStreamSynchronize(s), "synchronize");
#undef SPK_SIM_HIP

  // the pairs beyond each cut and the first copies of the cut value, sorted on the host: at most 2 x 4096
  struct Pair { unsigned key, i, j; };
  std::vector<Pair> sel[2];
  for (int w = 0; w < 2 && n_eff > 0; ++w) {
    const int64_t beyond = (int64_t)counters[w];
    const int64_t ties_seen = (int64_t)counters[2 + 2 * w + (block & 1)];   // the slot the last block left
    if (beyond + take[w] != n_eff || ties_seen < take[w])
      return bad(SPK_E_INVALID, "spk_cosine_triu_hist: the cuts are not those spk_cosine_triu_stats gives for this input");
    for (int64_t q = 0; q < beyond; ++q) {
      const unsigned* e = ext.data() + ((size_t)w * kSimMaxExt + q) * 3;
      sel[w].push_back(Pair{e[0], e[1], e[2]});
    }
    for (int64_t q = 0; q < take[w]; ++q) {
      const unsigned* e = ext.data() + ((size_t)(2 + w) * kSimMaxExt + q) * 3;
      sel[w].push_back(Pair{e[0], e[1], e[2]});
    }
    std::sort(sel[w].begin(), sel[w].end(), [w](const Pair& a, const Pair& b) {
      if (a.key != b.key) return w == 0 ? a.key > b.key : a.key < b.key;
      return a.i != b.i ? a.i < b.i : a.j < b.j;
    });
  }
  for (int b = 0; b < nbins; ++b) hist[b] = (int64_t)h[b];
  for (int w = 0; w < 2; ++w) {
    n_found[w] = (int32_t)sel[w].size();
    for (size_t q = 0; q < sel[w].size(); ++q) {
      const unsigned bits = sim_bits_of_key(sel[w][q].key);
      std::memcpy(ext_scores + (size_t)w * n_ext + q, &bits, 4);
      ext_i[(size_t)w * n_ext + q] = sel[w][q].i;
      ext_j[(size_t)w * n_ext + q] = sel[w][q].j;
    }
  }
  return SPK_OK;
}
