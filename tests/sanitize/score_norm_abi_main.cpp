// Stand-alone host check of csrc/score_norm_abi.cpp for a -fsanitize=address,undefined build
// (tests/test_score_norm_host.py compiles and runs it; no GPU, no Python).  The kernels' launchers
// are absent, so what runs is the argument checking and the row-block arithmetic: the workspace
// sizes over a range of shapes up to the caps, the rows per block for workspaces between the
// minimum and the recommended size, and the error codes of the four entry points, with every
// output pre-filled and checked unchanged.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../3d-speaker_amd/csrc/score_norm.h"
#include "../../include/spk_hip.h"

// what score_norm_abi.cpp needs from the rest of the library and from the HIP runtime
namespace spk {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace spk
extern "C" {
const char* hipGetErrorString(hipError_t) { return "stub"; }
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
  size_t lo = 77, rec = 78;
  CHECK(spk_cosine_cohort_stats_workspace_bytes(0, 5, &lo, &rec) == SPK_E_INVALID && lo == 77 && rec == 78);
  CHECK(spk_cosine_cohort_stats_workspace_bytes(5, 0, &lo, &rec) == SPK_E_INVALID);
  CHECK(spk_cosine_cohort_stats_workspace_bytes(-1, 5, &lo, &rec) == SPK_E_INVALID);
  CHECK(spk_cosine_cohort_stats_workspace_bytes(5, 5, nullptr, &rec) == SPK_E_INVALID);
  CHECK(spk_cosine_cohort_stats_workspace_bytes(5, 5, &lo, nullptr) == SPK_E_INVALID);
  CHECK(spk_cosine_cohort_stats_workspace_bytes(kCohortMaxRows + 1, 5, &lo, &rec) == SPK_E_UNSUPPORTED);
  CHECK(spk_cosine_cohort_stats_workspace_bytes(5, INT64_MAX, &lo, &rec) == SPK_E_UNSUPPORTED);
  CHECK(lo == 77 && rec == 78);
  for (int64_t n = 1; n <= kCohortMaxRows; n = n < 300 ? n + 1 : n * 2 - 7)
    for (int64_t nc = 1; nc <= kCohortMaxRows; nc = nc < 5 ? nc + 1 : nc * 3 + 1) {
      CHECK(spk_cosine_cohort_stats_workspace_bytes(n, nc, &lo, &rec) == SPK_OK);
      const size_t row = (size_t)nc * 4;
      CHECK(lo == 128 * row && rec >= lo && rec % (128 * row) == 0);
      const int64_t all = (n + 127) / 128 * 128;
      CHECK(rec <= (size_t)all * row);                                   // never more than N rows
      CHECK(rec == (size_t)all * row || rec == lo || rec + 128 * row > kCohortBlockBytes);
      CHECK(rec == lo || rec <= kCohortBlockBytes);
      // rows per block: a multiple of 128 the workspace holds; 0 only below the minimum
      CHECK(cohort_block_rows(n, nc, lo - 1) == 0 && cohort_block_rows(n, nc, 0) == 0);
      for (size_t b : {lo, lo + 1, lo + 128 * row - 1, lo + 128 * row, rec, rec + 12345, (size_t)-1}) {
        const int64_t r = cohort_block_rows(n, nc, b);
        CHECK(r >= 128 && r % 128 == 0 && r <= all && (size_t)r * row <= b);
        CHECK(r == all || (size_t)(r + 128) * row > b);
      }
    }

  const int64_t n = 9, nc = 11;
  const int32_t e = 8;
  CHECK(spk_cosine_cohort_stats_workspace_bytes(n, nc, &lo, &rec) == SPK_OK);
  std::vector<float> ws(rec / sizeof(float), 0.f), X(n * e, 1.f), C(nc * e, 1.f), S(n * nc, 0.5f);
  std::vector<float> mean(n, -7.f), sd(n, -7.f), out(n, -7.f);
  std::vector<int64_t> ia(n, 0), ib(n, 0);

  auto stats = [&](const float* s, int64_t rows, int64_t cols, int64_t lds, int32_t k, float* m, float* d) {
    return spk_topk_stats(s, rows, cols, lds, k, m, d, nullptr);
  };
  CHECK(stats(nullptr, n, nc, nc, 3, mean.data(), sd.data()) == SPK_E_INVALID);
  CHECK(stats(S.data(), n, nc, nc, 3, nullptr, sd.data()) == SPK_E_INVALID);
  CHECK(stats(S.data(), n, nc, nc, 3, mean.data(), nullptr) == SPK_E_INVALID);
  CHECK(stats(S.data(), 0, nc, nc, 3, mean.data(), sd.data()) == SPK_E_INVALID);
  CHECK(stats(S.data(), -1, nc, nc, 3, mean.data(), sd.data()) == SPK_E_INVALID);
  CHECK(stats(S.data(), n, 0, nc, 1, mean.data(), sd.data()) == SPK_E_INVALID);
  CHECK(stats(S.data(), n, nc, nc - 1, 3, mean.data(), sd.data()) == SPK_E_INVALID);
  CHECK(stats(S.data(), n, nc, nc, 0, mean.data(), sd.data()) == SPK_E_INVALID);
  CHECK(stats(S.data(), n, nc, nc, -2, mean.data(), sd.data()) == SPK_E_INVALID);
  CHECK(stats(S.data(), n, nc, nc, (int32_t)nc + 1, mean.data(), sd.data()) == SPK_E_INVALID);
  CHECK(stats(S.data(), n, INT64_MAX, INT64_MAX, 3, mean.data(), sd.data()) == SPK_E_UNSUPPORTED);
  CHECK(stats(S.data(), INT64_MAX, nc, INT64_MAX, 3, mean.data(), sd.data()) == SPK_E_UNSUPPORTED);   // no kernels
  CHECK(stats(S.data(), n, nc, nc, (int32_t)nc, mean.data(), sd.data()) == SPK_E_UNSUPPORTED);
  CHECK(g_err.find("no kernels") != std::string::npos);

  auto cohort = [&](const float* x, int64_t N, const float* c, int64_t Nc, int32_t E, int32_t k, float* m, float* d,
                    void* w, size_t wb) { return spk_cosine_cohort_stats(x, N, c, Nc, E, k, m, d, w, wb, nullptr); };
  CHECK(cohort(nullptr, n, C.data(), nc, e, 3, mean.data(), sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, nullptr, nc, e, 3, mean.data(), sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, e, 3, nullptr, sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, e, 3, mean.data(), nullptr, ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, e, 3, mean.data(), sd.data(), nullptr, rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), 0, C.data(), nc, e, 3, mean.data(), sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), 0, e, 1, mean.data(), sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, e, 0, mean.data(), sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, e, (int32_t)nc + 1, mean.data(), sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, 0, 3, mean.data(), sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, -4, 3, mean.data(), sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, 6, 3, mean.data(), sd.data(), ws.data(), rec) == SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, e, 3, mean.data(), sd.data(), ws.data(), lo - 1) == SPK_E_WORKSPACE);
  CHECK(cohort(X.data(), n, C.data(), nc, e, 3, mean.data(), sd.data(), ws.data(), 0) == SPK_E_WORKSPACE);
  CHECK(cohort(X.data(), INT64_MAX, C.data(), nc, e, 3, mean.data(), sd.data(), ws.data(), rec) == SPK_E_UNSUPPORTED);
  CHECK(cohort(X.data(), n, C.data(), INT64_MAX, e, 3, mean.data(), sd.data(), ws.data(), (size_t)-1) ==
        SPK_E_UNSUPPORTED);
  CHECK(cohort(X.data(), n, C.data(), nc, e, 3, mean.data(), sd.data(), reinterpret_cast<char*>(ws.data()) + 2, rec) ==
        SPK_E_INVALID);
  CHECK(cohort(X.data(), n, C.data(), nc, e, 3, mean.data(), sd.data(), ws.data(), lo) == SPK_E_UNSUPPORTED);
  CHECK(g_err.find("no kernels") != std::string::npos);

  auto trials = [&](const float* a, const float* b, int32_t E, const int64_t* i, const int64_t* j, int64_t T,
                    const float* ma, const float* sa, const float* mb, const float* sb, float* o) {
    return spk_cosine_trials_norm(a, b, E, i, j, T, ma, sa, mb, sb, o, nullptr);
  };
  const float *x = X.data(), *m = S.data();
  CHECK(trials(nullptr, x, e, ia.data(), ib.data(), n, m, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, nullptr, e, ia.data(), ib.data(), n, m, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, nullptr, ib.data(), n, m, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), nullptr, n, m, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), ib.data(), n, nullptr, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), ib.data(), n, m, nullptr, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), ib.data(), n, m, m, nullptr, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), ib.data(), n, m, m, m, nullptr, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), ib.data(), n, m, m, m, m, nullptr) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), ib.data(), 0, m, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), ib.data(), -5, m, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), ib.data(), INT64_MAX, m, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, 0, ia.data(), ib.data(), n, m, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, 7, ia.data(), ib.data(), n, m, m, m, m, out.data()) == SPK_E_INVALID);
  CHECK(trials(x, x, e, ia.data(), ib.data(), n, m, m, m, m, out.data()) == SPK_E_UNSUPPORTED);
  CHECK(g_err.find("no kernels") != std::string::npos);

  for (float v : mean) CHECK(v == -7.f);
  for (float v : sd) CHECK(v == -7.f);
  for (float v : out) CHECK(v == -7.f);
  for (float v : ws) CHECK(v == 0.f);
  std::puts("score_norm_abi host checks ok");
  return 0;
}
