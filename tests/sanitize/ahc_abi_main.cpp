// Stand-alone host check of csrc/ahc_abi.cpp for a -fsanitize=address,undefined build
// (tests/test_ahc_host.py compiles and runs it; no GPU, no Python).  The kernels' launchers are
// absent, so what runs is the argument checking and the workspace arithmetic: every size up to
// the cap, the carve-up of a real buffer (each array inside it, aligned, not overlapping), and
// the error codes of the entry points.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../3d-speaker_amd/csrc/ahc.h"
#include "../../include/spk_hip.h"

// what ahc_abi.cpp needs from the rest of the library and from the HIP runtime
namespace spk {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace spk
extern "C" {
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { std::abort(); }
hipError_t hipStreamSynchronize(hipStream_t) { std::abort(); }
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
  size_t bytes = 77;
  CHECK(spk_ahc_workspace_bytes(0, &bytes) == SPK_E_INVALID && bytes == 77);
  CHECK(spk_ahc_workspace_bytes(-3, &bytes) == SPK_E_INVALID);
  CHECK(spk_ahc_workspace_bytes(5, nullptr) == SPK_E_INVALID);
  CHECK(spk_ahc_workspace_bytes(kAhcMaxN + 1, &bytes) == SPK_E_UNSUPPORTED && bytes == 77);
  CHECK(spk_ahc_workspace_bytes(INT64_MAX, &bytes) == SPK_E_UNSUPPORTED && bytes == 77);
  size_t prev = 0;
  for (int64_t n = 1; n <= kAhcMaxN; n = n < 300 ? n + 1 : n * 2 - 7) {
    CHECK(spk_ahc_workspace_bytes(n, &bytes) == SPK_OK);
    const size_t need = (size_t)n * n * 8 + (size_t)n * 8 + (size_t)n * 24 + AHC_CTRL_WORDS * 4;
    CHECK(bytes >= need && bytes < need + 256 && bytes % 256 == 0 && bytes >= prev);
    prev = bytes;
  }
  CHECK(spk_ahc_workspace_bytes(kAhcMaxN, &bytes) == SPK_OK && bytes > (size_t)8 << 30);

  // the carve-up of a buffer of exactly the advertised size: touch every byte of every array
  for (int64_t n : {1, 2, 63, 257}) {
    CHECK(spk_ahc_workspace_bytes(n, &bytes) == SPK_OK);
    std::vector<double> buf(bytes / sizeof(double));
    const AhcState st = ahc_carve(buf.data(), n);
    std::memset(st.A, 1, (size_t)n * n * sizeof(double));
    std::memset(st.val, 2, (size_t)n * sizeof(double));
    int* ints[] = {st.col, st.size, st.active, st.member, st.stale, st.rank};
    for (int* p : ints) std::memset(p, 3, (size_t)n * sizeof(int));
    std::memset(st.ctrl, 4, AHC_CTRL_WORDS * sizeof(int));
    CHECK(reinterpret_cast<char*>(st.ctrl + AHC_CTRL_WORDS) <= reinterpret_cast<char*>(buf.data()) + bytes);
    CHECK(reinterpret_cast<uintptr_t>(st.val) % 8 == 0 && reinterpret_cast<uintptr_t>(st.ctrl) % 4 == 0);
    CHECK(st.ctrl[0] == 0x04040404 && st.rank[n - 1] == 0x03030303 && st.col[0] == 0x03030303);
  }

  const int64_t n = 9;
  CHECK(spk_ahc_workspace_bytes(n, &bytes) == SPK_OK);
  std::vector<double> ws(bytes / sizeof(double));
  std::vector<float> S((size_t)n * n, 0.f);
  std::vector<int32_t> labels(n, -7);
  int32_t count = -7;
  auto call = [&](const float* s, int64_t N, int64_t lds, int32_t* lab, int32_t* cnt, void* w, size_t wb) {
    return spk_ahc_average(s, N, lds, 0.3f, lab, cnt, w, wb, nullptr);
  };
  CHECK(call(nullptr, n, n, labels.data(), &count, ws.data(), bytes) == SPK_E_INVALID);
  CHECK(call(S.data(), n, n, nullptr, &count, ws.data(), bytes) == SPK_E_INVALID);
  CHECK(call(S.data(), n, n, labels.data(), nullptr, ws.data(), bytes) == SPK_E_INVALID);
  CHECK(call(S.data(), n, n, labels.data(), &count, nullptr, bytes) == SPK_E_INVALID);
  CHECK(call(S.data(), 0, n, labels.data(), &count, ws.data(), bytes) == SPK_E_INVALID);
  CHECK(call(S.data(), n, n - 1, labels.data(), &count, ws.data(), bytes) == SPK_E_INVALID);
  CHECK(call(S.data(), n, n, labels.data(), &count, ws.data(), bytes - 1) == SPK_E_WORKSPACE);
  CHECK(call(S.data(), n, n, labels.data(), &count, ws.data(), 0) == SPK_E_WORKSPACE);
  CHECK(call(S.data(), kAhcMaxN + 1, kAhcMaxN + 1, labels.data(), &count, ws.data(), bytes) == SPK_E_UNSUPPORTED);
  CHECK(call(S.data(), INT64_MAX, INT64_MAX, labels.data(), &count, ws.data(), (size_t)-1) == SPK_E_UNSUPPORTED);
  CHECK(call(S.data(), n, n, labels.data(), &count, reinterpret_cast<char*>(ws.data()) + 4, bytes) == SPK_E_INVALID);
  CHECK(call(S.data(), n, n, labels.data(), &count, ws.data(), bytes) == SPK_E_UNSUPPORTED);   // no kernels linked
  CHECK(g_err.find("no kernels") != std::string::npos);
  for (int32_t v : labels) CHECK(v == -7);
  CHECK(count == -7);
  for (double v : ws) CHECK(v == 0.0);
  std::puts("ahc_abi host checks ok");
  return 0;
}
