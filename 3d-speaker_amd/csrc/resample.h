// Windowed-sinc resampler: tap tables (host, resample_abi.cpp) + launcher (resample.hip).
#pragma once
#include "common.h"

#include <vector>

namespace spk {

// torchaudio.functional.resample's defaults
constexpr int kResampleLowpassWidth = 6;
constexpr double kResampleRolloff = 0.99;
// largest full polyphase table (n_phases * n_taps * 4 bytes) the library builds
constexpr size_t kResampleMaxTableBytes = 8u << 20;

// gcd-reduced rates and the table's shape: K = 2 * width + o taps for each of n phases
struct ResampleShape {
  int o = 0, n = 0, width = 0, K = 0;
};
ResampleShape resample_shape(int orig_freq, int new_freq);

// The polyphase table h[n][K], every tap computed in double from the closed formula and
// rounded once to fp32.
std::vector<float> build_resample_taps(const ResampleShape& s);

// What the kernels read.  The Hann window clamps |t| at lowpass_width, where it is zero, so
// only ~12 * o / min(o, n) taps of a row's K are non-zero.  taps[p][0..S) is the slice
// [k0[p], k0[p] + S) of row p of the full table; S is the widest non-zero support over the
// phases, and every tap outside the slice is an exact fp32 zero, so the chain over the slice in
// ascending k has the bits of the chain over all K taps (x finite).  Rows are ld floats apart.
struct ResampleTable {
  const float* taps = nullptr;   // device [n][ld]
  const int* k0 = nullptr;       // device [n]
  int o = 0, n = 0, width = 0, S = 0, ld = 0;
};

// One workgroup slice g of G per utterance, striding over that utterance's output tiles.
// Not linked into the host-only build of the executor (tests/emu): weak, checked by the ABI.
hipError_t launch_resample(const float* wav, const int64_t* wav_off, int n_utt, const ResampleTable& t, float* out,
                           const int64_t* out_off, hipStream_t s) __attribute__((weak));

}  // namespace spk
