// Windowed-sinc resampler: polyphase tap tables (double precision, host) and the C ABI
// entries of resample.hip.  The arithmetic is torchaudio.functional.resample's default path
// (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), which the reference calls at
// speakerlab/utils/fileio.py:110,126:
//   o, n = orig / gcd, new / gcd;  base = min(o, n) * rolloff;  w = ceil(6 * o / base)
//   t = clamp((k - w) / o - p / n, +-6 / base) * base
//   h[p][k] = sinc(t) * cos^2(pi t / 12) * base / o,  k < K = 2 w + o
//   y[b n + p] = sum_k x[b o - w + k] h[p][k]
// torchaudio builds h in the waveform's dtype (fp32: ~1e-5 relative error on the taps at
// 44.1 kHz, tests/test_resample.py); here every tap is computed in double and rounded once.
#include "resample.h"
#include "runtime.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

namespace spk {

ResampleShape resample_shape(int orig_freq, int new_freq) {
  if (orig_freq <= 0 || new_freq <= 0) throw SpkError(SPK_E_INVALID, "resample: rates must be positive");
  if (orig_freq == new_freq) throw SpkError(SPK_E_INVALID, "resample: equal rates, nothing to resample");
  const int g = std::gcd(orig_freq, new_freq);
  ResampleShape s;
  s.o = orig_freq / g;
  s.n = new_freq / g;
  const double base = (double)std::min(s.o, s.n) * kResampleRolloff;
  const double width = std::ceil((double)((int64_t)kResampleLowpassWidth * s.o) / base);
  const double K = 2.0 * width + s.o;
  if (K * s.n * sizeof(float) > (double)kResampleMaxTableBytes)
    throw SpkError(SPK_E_UNSUPPORTED, "resample: the polyphase table of " + std::to_string(orig_freq) + " -> " +
                                          std::to_string(new_freq) + " Hz (" + std::to_string(s.n) + " phases x " +
                                          std::to_string((long long)K) + " taps) is above the 8 MiB cap");
  s.width = (int)width;
  s.K = (int)K;
  return s;
}

std::vector<float> build_resample_taps(const ResampleShape& s) {
  const double pi = 3.14159265358979323846;
  const double base = (double)std::min(s.o, s.n) * kResampleRolloff;
  const double lim = (double)kResampleLowpassWidth / base, scale = base / s.o;
  std::vector<float> h((size_t)s.n * s.K);
  for (int p = 0; p < s.n; ++p)
    for (int k = 0; k < s.K; ++k) {
      double t = (double)(k - s.width) / s.o - (double)p / s.n;
      t = std::min(std::max(t, -lim), lim) * base;
      const double c = std::cos(t * pi / (2.0 * kResampleLowpassWidth));
      const double sinc = t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t);
      h[(size_t)p * s.K + k] = (float)(sinc * c * c * scale);
    }
  return h;
}

namespace {

struct DeviceTable {
  ResampleTable t;
};
std::mutex g_mu;
std::map<std::tuple<int, int, int>, DeviceTable> g_tables;   // (device, o, n); entries live as long as the library

int hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return SPK_OK;
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return SPK_E_HIP;
}

// the compact table of ResampleTable (resample.h), uploaded once per (device, o, n)
int device_table(const ResampleShape& s, ResampleTable* out) {
  int dev = 0;
  if (int rc = hip_check(hipGetDevice(&dev), "hipGetDevice")) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  const auto key = std::make_tuple(dev, s.o, s.n);
  auto it = g_tables.find(key);
  if (it != g_tables.end()) {
    *out = it->second.t;
    return SPK_OK;
  }
  const std::vector<float> h = build_resample_taps(s);
  std::vector<int> lo(s.n), k0(s.n);
  int S = 1;
  for (int p = 0; p < s.n; ++p) {
    const float* row = h.data() + (size_t)p * s.K;
    int a = 0, b = s.K - 1;
    while (a < s.K - 1 && row[a] == 0.f) ++a;
    while (b > a && row[b] == 0.f) --b;
    lo[p] = a;
    S = std::max(S, b - a + 1);
  }
  const int ld = S | 1;   // odd row stride: consecutive phases fall on distinct LDS banks
  std::vector<float> c((size_t)s.n * ld, 0.f);
  for (int p = 0; p < s.n; ++p) {
    k0[p] = std::min(lo[p], s.K - S);
    std::memcpy(c.data() + (size_t)p * ld, h.data() + (size_t)p * s.K + k0[p], (size_t)S * sizeof(float));
  }
  float* d_taps = nullptr;
  int* d_k0 = nullptr;
  if (int rc = hip_check(hipMalloc(reinterpret_cast<void**>(&d_taps), c.size() * sizeof(float)), "hipMalloc(resample taps)"))
    return rc;
  if (int rc = hip_check(hipMalloc(reinterpret_cast<void**>(&d_k0), k0.size() * sizeof(int)), "hipMalloc(resample taps)")) {
    (void)hipFree(d_taps);
    return rc;
  }
  int rc = hip_check(hipMemcpy(d_taps, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(resample taps)");
  if (!rc) rc = hip_check(hipMemcpy(d_k0, k0.data(), k0.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy(resample taps)");
  if (rc) {
    (void)hipFree(d_taps);
    (void)hipFree(d_k0);
    return rc;
  }
  DeviceTable e;
  e.t.taps = d_taps;
  e.t.k0 = d_k0;
  e.t.o = s.o;
  e.t.n = s.n;
  e.t.width = s.width;
  e.t.S = S;
  e.t.ld = ld;
  g_tables.emplace(key, e);
  *out = e.t;
  return SPK_OK;
}

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const SpkError& e) {
    set_error(e.what());
    return e.code;
  } catch (const std::exception& e) {
    set_error(std::string("internal error: ") + e.what());
    return SPK_E_INVALID;
  }
}

}  // namespace
}  // namespace spk

using namespace spk;

extern "C" int spk_resample_out_len(int64_t L, int32_t orig_freq, int32_t new_freq, int64_t* out_len) {
  if (!out_len || L < 0 || orig_freq <= 0 || new_freq <= 0) {
    set_error("spk_resample_out_len: invalid argument");
    return SPK_E_INVALID;
  }
  const int g = std::gcd(orig_freq, new_freq);
  const __int128 o = orig_freq / g, n = new_freq / g;
  *out_len = (int64_t)((n * L + o - 1) / o);
  return SPK_OK;
}

extern "C" int spk_resample_taps(int32_t orig_freq, int32_t new_freq, int32_t* n_phases, int32_t* n_taps, int32_t* width,
                                 float* taps, size_t taps_len) {
  return guarded([&]() -> int {
    const ResampleShape s = resample_shape(orig_freq, new_freq);
    if (n_phases) *n_phases = s.n;
    if (n_taps) *n_taps = s.K;
    if (width) *width = s.width;
    if (!taps) return SPK_OK;
    if (taps_len < (size_t)s.n * s.K) {
      set_error("spk_resample_taps: taps_len is smaller than n_phases * n_taps");
      return SPK_E_INVALID;
    }
    const std::vector<float> h = build_resample_taps(s);
    std::memcpy(taps, h.data(), h.size() * sizeof(float));
    return SPK_OK;
  });
}

extern "C" int spk_resample_f32(const float* wav, const int64_t* wav_offsets, int32_t n_utt, int32_t orig_freq,
                                int32_t new_freq, float* out, const int64_t* out_offsets, void* stream) {
  return guarded([&]() -> int {
    const ResampleShape s = resample_shape(orig_freq, new_freq);
    if (n_utt < 0 || (n_utt > 0 && (!wav_offsets || !out_offsets))) {
      set_error("spk_resample_f32: invalid argument");
      return SPK_E_INVALID;
    }
    if (n_utt == 0) return SPK_OK;
    if (!launch_resample) {
      set_error("spk_resample_f32: this build of the library has no kernels");
      return SPK_E_UNSUPPORTED;
    }
    ResampleTable t;
    if (int rc = device_table(s, &t)) return rc;
    const hipError_t e = launch_resample(wav, wav_offsets, n_utt, t, out, out_offsets, reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
      set_error(std::string("spk_resample_f32: ") + hipGetErrorString(e));
      return e == hipErrorInvalidValue ? SPK_E_INVALID : SPK_E_HIP;
    }
    return SPK_OK;
  });
}
