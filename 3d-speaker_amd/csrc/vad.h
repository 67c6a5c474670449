// VAD front end on the device: the two mean-square tracks the energy VAD and the boundary
// refinement read, and the masked copy of the signal (vad.hip); C ABI in vad_abi.cpp.
#pragma once
#include "common.h"

namespace spk {

// 16 kHz only: 16 ms VAD frames, 20 ms refinement windows at a 10 ms hop, and the block of
// 32 = gcd(160, 256) samples both are built from
constexpr int kVadFrame = 256;
constexpr int kVadHop = 160;
constexpr int kVadWin = 2 * kVadHop;
constexpr int kVadBlock = 32;

inline int64_t vad_n16(int64_t L) { return L / kVadFrame; }
inline int64_t vad_n20(int64_t L) { return L >= kVadWin ? (L - kVadWin) / kVadHop + 1 : 0; }

// Not linked into the host-only build of the executor (tests/emu): weak, checked by the ABI.
hipError_t launch_vad_energy(const float* wav, const int64_t* wav_off, int n_utt, double* e16, const int64_t* e16_off,
                             float* e20, const int64_t* e20_off, hipStream_t s) __attribute__((weak));
hipError_t launch_vad_apply_intervals(const float* wav, int64_t L, const int64_t* starts, const int64_t* ends,
                                      int64_t n_iv, float* out, hipStream_t s) __attribute__((weak));

}  // namespace spk
