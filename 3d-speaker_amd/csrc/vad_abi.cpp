// C ABI entries of the device VAD front end (vad.hip): argument checks and the host-side size
// helper.  Every check runs before the launch; lengths live in device offsets, so the entries
// only enqueue.
#include "vad.h"
#include "runtime.h"

using namespace spk;

namespace {

int bad(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

int hip_fail(const char* fn, hipError_t e) {
  set_error(std::string(fn) + ": " + hipGetErrorString(e));
  return e == hipErrorInvalidValue ? SPK_E_INVALID : SPK_E_HIP;
}

}  // namespace

extern "C" int spk_vad_energy_sizes(int64_t L, int64_t* n16, int64_t* n20) {
  if (L < 0 || !n16 || !n20) return bad(SPK_E_INVALID, "spk_vad_energy_sizes: invalid argument (L < 0 or a null pointer)");
  *n16 = vad_n16(L);
  *n20 = vad_n20(L);
  return SPK_OK;
}

extern "C" int spk_vad_energy_f32(const float* wav, const int64_t* wav_offsets, int32_t n_utt, double* e16,
                                  const int64_t* e16_offsets, float* e20, const int64_t* e20_offsets, void* stream) {
  if (n_utt < 0) return bad(SPK_E_INVALID, "spk_vad_energy_f32: n_utt < 0");
  if (n_utt == 0) return SPK_OK;
  if (!wav || !wav_offsets || !e16 || !e16_offsets || !e20 || !e20_offsets)
    return bad(SPK_E_INVALID, "spk_vad_energy_f32: null pointer");
  if (reinterpret_cast<uintptr_t>(e16) % alignof(double) != 0)
    return bad(SPK_E_INVALID, "spk_vad_energy_f32: e16 must be 8-byte aligned");
  if (!launch_vad_energy) return bad(SPK_E_UNSUPPORTED, "spk_vad_energy_f32: this build of the library has no kernels");
  if (hipError_t e = launch_vad_energy(wav, wav_offsets, n_utt, e16, e16_offsets, e20, e20_offsets,
                                       reinterpret_cast<hipStream_t>(stream)))
    return hip_fail("spk_vad_energy_f32", e);
  return SPK_OK;
}

extern "C" int spk_vad_apply_intervals_f32(const float* wav, int64_t L, const int64_t* starts, const int64_t* ends,
                                           int64_t n_iv, float* out, void* stream) {
  if (L < 0 || n_iv < 0) return bad(SPK_E_INVALID, "spk_vad_apply_intervals_f32: L < 0 or n_iv < 0");
  if (L == 0) return SPK_OK;
  if (!wav || !out || (n_iv > 0 && (!starts || !ends)))
    return bad(SPK_E_INVALID, "spk_vad_apply_intervals_f32: null pointer");
  if (!launch_vad_apply_intervals)
    return bad(SPK_E_UNSUPPORTED, "spk_vad_apply_intervals_f32: this build of the library has no kernels");
  if (hipError_t e = launch_vad_apply_intervals(wav, L, starts, ends, n_iv, out, reinterpret_cast<hipStream_t>(stream)))
    return hip_fail("spk_vad_apply_intervals_f32", e);
  return SPK_OK;
}
