// Route selection of the CAM++ gate (tdnn_ops.h): which of the three kernel forms of
// tdnn_ops.hip serves a shape.  Host arithmetic only, so the device library and the host
// emulation link the same definition.
#include <cstdint>
#include <cstdlib>

#include "tdnn_ops.h"

namespace spk {

CamPick cam_gate_pick(int B, int C, int ld, int nseg, const float* w1, int k1p, int red, const float* w2, int k2p,
                      int growth) {
  if (C % 4 || C / 4 > 256 || ld % 4 || red <= 0 || red > 1024 || growth <= 0 || growth > 1024 || B <= 0 || nseg <= 0)
    return {CAM_REFUSED, 0};
  static const bool lean_off = std::getenv("SPK_CAM_GATE_LDS") != nullptr;   // A/B: the transposing kernel
  static const bool fuse_off = std::getenv("SPK_CAM_GATE_PAIR") != nullptr;  // A/B: segment sums as their own launch
  // the lean kernel's butterfly sums Q = 256 / red (or 256 / growth) adjacent lanes with
  // __shfl_xor, i.e. within one wave only when Q <= 64
  const bool lean = !lean_off && red >= 4 && growth >= 4 && 256 % red == 0 && 256 % growth == 0 && C % (4 * (256 / red)) == 0 &&
                    red % (4 * (256 / growth)) == 0 && C / (256 / red) <= 4 * CAM_WQ &&
                    red / (256 / growth) <= 4 * CAM_WQ && k1p % 4 == 0 && k2p % 4 == 0 &&
                    (reinterpret_cast<uintptr_t>(w1) & 15) == 0 && (reinterpret_cast<uintptr_t>(w2) & 15) == 0;
  const size_t lds_f = sizeof(float) * (4 * 256 + (size_t)nseg * C + C + CAM_SEGS * ((size_t)C + red));
  if (lean && !fuse_off && lds_f <= 64 * 1024) return {CAM_FUSED, lds_f};
  if (lean) return {CAM_PAIR_LEAN, sizeof(float) * ((size_t)C + CAM_SEGS * ((size_t)C + red))};
  const size_t lds = sizeof(float) * ((size_t)C * (red + 1) + (size_t)red * (growth + 1) + C +
                                      CAM_SEGS * (C + red + 1024));
  if (lds > 64 * 1024) return {CAM_REFUSED, 0};
  return {CAM_PAIR_LDS, lds};
}

__attribute__((weak)) std::string cam_gate_kernel_name(int B, int C, int ld, int nseg, const float* w1, int k1p,
                                                       int red, const float* w2, int k2p, int growth) {
  switch (cam_gate_pick(B, C, ld, nseg, w1, k1p, red, w2, k2p, growth).route) {
    case CAM_FUSED: return "cam_gate_fused_kernel";
    case CAM_PAIR_LEAN: return "cam_segsum_kernel+cam_gate_lean_kernel";
    case CAM_PAIR_LDS: return "cam_segsum_kernel+cam_gate_kernel";
    default: return "";
  }
}

}  // namespace spk
