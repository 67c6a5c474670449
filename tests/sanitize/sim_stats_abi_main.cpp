// Stand-alone host check of csrc/sim_stats_abi.cpp for a -fsanitize=address,undefined build
// (tests/test_sim_stats_host.py compiles and runs it; no GPU, no Python).  The kernels' launchers
// are absent, so what runs is the argument checking, the row-block arithmetic and the state layout:
// the workspace sizes over a range of N up to the cap, the rows per block for workspaces between
// the minimum and the recommended size against the grid limits, and the error codes of the four
// entry points, with every output pre-filled and checked unchanged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../3d-speaker_amd/csrc/sim_stats.h"
#include "../../include/spk_hip.h"

// what sim_stats_abi.cpp needs from the rest of the library and from the HIP runtime; none of the
// runtime calls is reached without kernels
namespace spk {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace spk
static int g_runtime_calls = 0;
extern "C" {
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { ++g_runtime_calls; return hipErrorUnknown; }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { ++g_runtime_calls; return hipErrorUnknown; }
hipError_t hipStreamSynchronize(hipStream_t) { ++g_runtime_calls; return hipErrorUnknown; }
}

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

int main() {
  using namespace spk;
  size_t lo = 77, rec = 78, sb = 79;
  CHECK(spk_cosine_sim_workspace_bytes(0, &lo, &rec, &sb) == SPK_E_INVALID);
  CHECK(spk_cosine_sim_workspace_bytes(-1, &lo, &rec, &sb) == SPK_E_INVALID);
  CHECK(spk_cosine_sim_workspace_bytes(5, nullptr, &rec, &sb) == SPK_E_INVALID);
  CHECK(spk_cosine_sim_workspace_bytes(5, &lo, nullptr, &sb) == SPK_E_INVALID);
  CHECK(spk_cosine_sim_workspace_bytes(5, &lo, &rec, nullptr) == SPK_E_INVALID);
  CHECK(spk_cosine_sim_workspace_bytes(kSimMaxRows + 1, &lo, &rec, &sb) == SPK_E_UNSUPPORTED);
  CHECK(spk_cosine_sim_workspace_bytes(INT64_MAX, &lo, &rec, &sb) == SPK_E_UNSUPPORTED);
  CHECK(spk_cosine_sim_workspace_bytes(kSimMaxRows, &lo, &rec, &sb) == SPK_E_UNSUPPORTED);   // the affinity's grid
  CHECK(lo == 77 && rec == 78 && sb == 79);
  for (int64_t n = 1; n <= kSimMaxRows; n = n < 300 ? n + 1 : n * 2 - 7) {
    const int rc = spk_cosine_sim_workspace_bytes(n, &lo, &rec, &sb);
    const size_t row = (size_t)n * 4;
    const int64_t all = (n + 127) / 128 * 128, col_tiles = (n + 127) / 128;
    if (rc == SPK_E_UNSUPPORTED) {                                        // not even one tile of rows is a launch
      CHECK(col_tiles * 256 >= kSimGridItems);
      continue;
    }
    CHECK(rc == SPK_OK);
    CHECK(lo == 128 * row && rec >= lo && rec % (128 * row) == 0 && rec <= (size_t)all * row);
    CHECK(rec == lo || rec <= kSimBlockBytes);
    const TriuState l = triu_state_layout(n);
    CHECK(sb == l.bytes && l.npad == all && l.row_tie + (size_t)2 * all * 4 <= l.ext && l.ext + 4 * 4096 * 12 == l.bytes);
    CHECK(l.row_sum % 16 == 0 && l.digit_hist % 16 == 0 && l.edges % 16 == 0 && l.counters % 16 == 0 && l.ext % 16 == 0);
    CHECK(sim_block_rows(n, lo - 1) == 0 && sim_block_rows(n, 0) == 0);
    for (size_t b : {lo, lo + 1, lo + 128 * row - 1, lo + 128 * row, rec, rec + 12345, (size_t)-1}) {
      const int64_t r = sim_block_rows(n, b);
      CHECK(r >= 128 && r % 128 == 0 && r <= all && (size_t)r * row <= b);
      // every launch of a block stays below 2^31 work-items, and inside the affinity's grid.y
      CHECK(r * kSimThreads < kSimGridItems && col_tiles * (r / 128) * 256 < kSimGridItems && r / 128 <= 65535);
    }
  }
  CHECK(sim_pairs(1) == 0 && sim_pairs(2) == 1 && sim_pairs(kSimMaxRows) == (int64_t)2305843005992468481LL);
  for (unsigned bits : {0u, 0x80000000u, 0x3F800000u, 0xBF800000u, 0x00000001u, 0x80000001u, 0x7F800000u, 0xFF800000u}) {
    const unsigned k = sim_key_of_bits(bits);
    CHECK(sim_bits_of_key(k) == (bits == 0x80000000u ? 0u : bits));
  }
  CHECK(sim_key_of_bits(0xBF800000u) < sim_key_of_bits(0x80000001u) && sim_key_of_bits(0x80000001u) < sim_key_of_bits(0u) &&
        sim_key_of_bits(0u) < sim_key_of_bits(1u) && sim_key_of_bits(1u) < sim_key_of_bits(0x3F800000u));

  const int64_t n = 9;
  const int32_t e = 8, k = 3, ne = 4;
  CHECK(spk_cosine_sim_workspace_bytes(n, &lo, &rec, &sb) == SPK_OK);
  std::vector<float> X(n * e + 4, 1.f), top_s(n * k, -7.f), f1(n, -7.f), f2(n, -7.f), f3(n, -7.f);
  std::vector<int64_t> top_i(n * k, -7);
  std::vector<double> d1(n, -7.0), d2(n, -7.0);
  std::vector<double> wsd(rec / 8 + 1, 0.0), std_(sb / 8 + 2, 0.0);   // doubles: 16-byte alignment is found below
  char* ws = reinterpret_cast<char*>(wsd.data());
  char* st = reinterpret_cast<char*>(std_.data());
  if (reinterpret_cast<uintptr_t>(st) % 16) st += 8;
  const float* x = X.data();
  if (reinterpret_cast<uintptr_t>(x) % 16) x += (16 - reinterpret_cast<uintptr_t>(x) % 16) / 4;

  auto rows = [&](const float* x_, int64_t N, int32_t E, int32_t k_, float* a, int64_t* b, double* c, void* w, size_t wb) {
    return spk_cosine_rows_topk(x_, N, E, k_, a, b, c, d2.data(), f1.data(), f2.data(), f3.data(), w, wb, nullptr);
  };
  CHECK(rows(nullptr, n, e, k, top_s.data(), top_i.data(), d1.data(), ws, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, e, k, nullptr, top_i.data(), d1.data(), ws, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, e, k, top_s.data(), nullptr, d1.data(), ws, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, e, k, top_s.data(), top_i.data(), nullptr, ws, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, e, k, top_s.data(), top_i.data(), d1.data(), nullptr, rec) == SPK_E_INVALID);
  CHECK(rows(x, 0, e, k, top_s.data(), top_i.data(), d1.data(), ws, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, 0, k, top_s.data(), top_i.data(), d1.data(), ws, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, 6, k, top_s.data(), top_i.data(), d1.data(), ws, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, e, 0, top_s.data(), top_i.data(), d1.data(), ws, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, e, 1025, top_s.data(), top_i.data(), d1.data(), ws, rec) == SPK_E_INVALID);
  CHECK(rows(x + 1, n, e, k, top_s.data(), top_i.data(), d1.data(), ws, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, e, k, top_s.data(), top_i.data(), d1.data(), ws + 2, rec) == SPK_E_INVALID);
  CHECK(rows(x, n, e, k, top_s.data(), top_i.data(), d1.data(), ws, lo - 1) == SPK_E_WORKSPACE);
  CHECK(rows(x, INT64_MAX, e, k, top_s.data(), top_i.data(), d1.data(), ws, (size_t)-1) == SPK_E_UNSUPPORTED);
  CHECK(rows(x, n, e, k, top_s.data(), top_i.data(), d1.data(), ws, lo) == SPK_E_UNSUPPORTED);
  CHECK(g_err.find("no kernels") != std::string::npos);

  float thr[2] = {0.5f, 0.1f}, mm[2] = {-7.f, -7.f}, order[2] = {-7.f, -7.f}, cut[2] = {-7.f, -7.f};
  int64_t ranks[2] = {0, 35}, count = -7, cge[2] = {-7, -7};
  double sums[2] = {-7.0, -7.0};
  int32_t take[2] = {-7, -7};
  auto stats = [&](int64_t N, int32_t E, const float* t, int32_t nt, const int64_t* r, int32_t nr, int32_t ne_, size_t wb,
                   void* s, size_t sbytes) {
    return spk_cosine_triu_stats(x, N, E, t, nt, r, nr, ne_, &count, sums, sums + 1, mm, mm + 1, cge, order, cut, take, ws,
                                 wb, s, sbytes, nullptr);
  };
  const int64_t down[2] = {5, 4}, high[2] = {0, 36}, neg[2] = {-1, 3};
  const float nanthr[2] = {0.5f, NAN};
  CHECK(stats(0, e, thr, 2, ranks, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, 10, thr, 2, ranks, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, nullptr, 2, ranks, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 33, ranks, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, -1, ranks, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, nanthr, 2, ranks, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 2, nullptr, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 2, ranks, 17, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 2, down, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 2, high, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 2, neg, 2, ne, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 2, ranks, 2, -1, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 2, ranks, 2, 4097, rec, st, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 2, ranks, 2, ne, rec, nullptr, sb) == SPK_E_INVALID);
  CHECK(stats(n, e, thr, 2, ranks, 2, ne, rec, st + 4, sb) == SPK_E_INVALID);
  CHECK(stats(1, e, thr, 2, ranks, 1, ne, rec, st, sb) == SPK_E_INVALID);             // N == 1: any rank is at or above P
  CHECK(stats(n, e, thr, 2, ranks, 2, ne, lo - 1, st, sb) == SPK_E_WORKSPACE);
  CHECK(stats(n, e, thr, 2, ranks, 2, ne, rec, st, sb - 1) == SPK_E_WORKSPACE);
  CHECK(stats(INT64_MAX, e, thr, 2, ranks, 0, ne, (size_t)-1, st, sb) == SPK_E_UNSUPPORTED);
  CHECK(stats(n, e, thr, 2, ranks, 2, ne, rec, st, sb) == SPK_E_UNSUPPORTED);
  CHECK(g_err.find("no kernels") != std::string::npos);
  CHECK(count == -7 && sums[0] == -7.0 && sums[1] == -7.0 && mm[0] == -7.f && cge[0] == -7 && order[0] == -7.f &&
        cut[0] == -7.f && take[0] == -7);

  double edges[6] = {-1.0, -0.5, 0.0, 0.5, 0.7, 1.0}, bad_edges[6] = {-1.0, 0.0, -0.5, 0.5, 0.7, 1.0};
  int64_t hist[5] = {-7, -7, -7, -7, -7}, ei[8], ej[8];
  float es[8], gcut[2] = {0.5f, -0.5f};
  int32_t gtake[2] = {1, 1}, bad_take[2] = {0, 1}, found[2] = {-7, -7};
  for (int q = 0; q < 8; ++q) { ei[q] = ej[q] = -7; es[q] = -7.f; }
  auto hist_ = [&](int64_t N, const double* ed, int32_t nb, int32_t ne_, const float* ec, const int32_t* et, size_t wb,
                   size_t sbytes) {
    return spk_cosine_triu_hist(x, N, e, ed, nb, ne_, ec, et, hist, es, ei, ej, found, ws, wb, st, sbytes, nullptr);
  };
  CHECK(hist_(0, edges, 5, ne, gcut, gtake, rec, sb) == SPK_E_INVALID);
  CHECK(hist_(n, nullptr, 5, ne, gcut, gtake, rec, sb) == SPK_E_INVALID);
  CHECK(hist_(n, bad_edges, 5, ne, gcut, gtake, rec, sb) == SPK_E_INVALID);
  CHECK(hist_(n, edges, 257, ne, gcut, gtake, rec, sb) == SPK_E_INVALID);
  CHECK(hist_(n, edges, -1, ne, gcut, gtake, rec, sb) == SPK_E_INVALID);
  CHECK(hist_(n, edges, 5, 4097, gcut, gtake, rec, sb) == SPK_E_INVALID);
  CHECK(hist_(n, edges, 5, ne, nullptr, gtake, rec, sb) == SPK_E_INVALID);
  CHECK(hist_(n, edges, 5, ne, gcut, bad_take, rec, sb) == SPK_E_INVALID);
  CHECK(hist_(n, edges, 5, ne, gcut, gtake, lo - 1, sb) == SPK_E_WORKSPACE);
  CHECK(hist_(n, edges, 5, ne, gcut, gtake, rec, sb - 1) == SPK_E_WORKSPACE);
  CHECK(hist_(n, edges, 5, ne, gcut, gtake, rec, sb) == SPK_E_UNSUPPORTED);
  CHECK(hist[0] == -7 && found[0] == -7 && es[0] == -7.f && ei[0] == -7 && ej[0] == -7);
  // N == 1 has no pair: answered on the host, nothing launched
  CHECK(stats(1, e, thr, 2, ranks, 0, ne, rec, st, sb) == SPK_OK);
  CHECK(count == 0 && std::isnan(sums[0]) && std::isnan(sums[1]) && std::isnan(mm[0]) && std::isnan(mm[1]) &&
        cge[0] == 0 && cge[1] == 0 && std::isnan(cut[0]) && take[0] == 0 && take[1] == 0);
  CHECK(hist_(1, edges, 5, ne, gcut, gtake, rec, sb) == SPK_OK);
  CHECK(hist[0] == 0 && hist[4] == 0 && found[0] == 0 && found[1] == 0 && es[0] == -7.f);

  CHECK(g_runtime_calls == 0);
  for (float v : top_s) CHECK(v == -7.f);
  for (int64_t v : top_i) CHECK(v == -7);
  for (double v : d1) CHECK(v == -7.0);
  for (double v : wsd) CHECK(v == 0.0);
  for (double v : std_) CHECK(v == 0.0);
  std::puts("sim_stats_abi host checks ok");
  return 0;
}
