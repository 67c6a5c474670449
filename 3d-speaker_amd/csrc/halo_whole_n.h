// LDS layouts of the fp16x3 halo kernel's two forms at 52 channels (conv3x3_halo.hip), as index
// functions that host code can evaluate too (tests/test_halo_whole_n_layout.py compares them).
//
// Padded form (two 32-channel slices, two k-groups): rows of 80 halves, K padded 52 -> 64.
//
// Whole-N form (one block computes all 52 output channels): rows of 56 halves = seven 16-byte
// k-blocks (channels 52..55 zero, the eighth k-block not stored), weights for 52 channels only.
// A row stride of seven 16-byte units alone is not conflict-free for ds_read_b128: the read is
// served in lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (and the same + 32), i.e.
// eight MFMA rows of one k-block with the other eight rows of the next, and 7 (r - r') = +-1
// (mod 16) has solutions between those row sets.  Two permutations remove them:
//   - the lane quarters g = lane >> 4 take the k-blocks in the order 0, 2, 1, 3, so the two
//     k-blocks of a lane group are two units apart;
//   - MFMA row i = lane & 15 stands for row perm16(i) of its 16-row block, which sends the rows
//     {0-3, 12-15} to the even and {4-11} to the odd ones.
// Then 7 (r - r') = +-2 (mod 16) needs an even r - r', and r - r' is odd.  (Pixel rows: true
// where the 16 pixels of a block are consecutive halo pixels, tile widths 16 and 32; at width 8
// a block spans two tile rows and one pair of lanes per group shares a bank.)
// The k-block that does not exist (quarter 3 of the second 32-deep step) is read as zeros from
// the weights: each tap's rows are followed by two zero blocks, one per row parity so that
// they too stay off the banks of the quarter-2 lanes of their group.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPK_WN_HD __host__ __device__
#else
#define SPK_WN_HD
#endif

namespace spk {
namespace halo_wn {

constexpr int CIN = 52;
constexpr int ROW = 56;                       // halves per pixel / weight row
constexpr int WROWS = 55;                     // weight row positions per tap: wrow(51) = 54
constexpr int WTAP = WROWS * ROW + 16;        // halves per tap and plane: rows + two zero blocks
constexpr int WPLANE = 9 * WTAP;
constexpr int HALO_PIX = 204;                 // max (TH + 2)(TW + 2) of a 128-pixel tile
constexpr int HPLANE = HALO_PIX * ROW;
constexpr int LDS_BYTES = 2 * 2 * (HPLANE + WPLANE);   // hi + lo planes, 2 bytes a half
static_assert(LDS_BYTES <= 160 * 1024, "whole-N halo form: LDS");
static_assert(WTAP % 8 == 0 && HPLANE % 8 == 0 && WPLANE % 8 == 0, "16-byte aligned planes");

SPK_WN_HD constexpr int perm16(int i) { return i < 4 ? 2 * i : i >= 12 ? 2 * (i - 8) : 2 * (i - 4) + 1; }
SPK_WN_HD constexpr int perm16_inv(int r) { return (r & 1) ? (r >> 1) + 4 : (r >> 1) < 4 ? (r >> 1) : (r >> 1) + 8; }
// k-block (8 channels) of lane quarter g in 32-deep step s; 7: past the row (zeros)
SPK_WN_HD constexpr int kblock(int g, int s) { return 4 * s + (((g & 1) << 1) | (g >> 1)); }
// row position of output channel n within a tap
SPK_WN_HD constexpr int wrow(int n) { return (n & ~15) | perm16(n & 15); }
// channel held at row position r (>= CIN: none, the row is zero)
SPK_WN_HD constexpr int wrow_channel(int r) { return (r & ~15) | perm16_inv(r & 15); }
// pixel of its 16-pixel block that a lane's MFMA column stands for
SPK_WN_HD constexpr int lane_pixel(int lane) { return perm16(lane & 15); }

// pixel operand of a lane in step s: halves from the start of a halo plane, q = the halo
// pixel of lane_pixel(lane) at the tap.  The absent k-block reads block 5 (it meets zeros).
SPK_WN_HD constexpr int pix_off(int q, int lane, int s) {
  const int kb = kblock(lane >> 4, s);
  return q * ROW + 8 * (kb == 7 ? 5 : kb);
}
// weight operand of a lane: channel 16 cb + (lane & 15) of 16-channel block cb (0..3), step s,
// halves from the start of a weight plane.  Lanes of channels past 51 read the row 16 above
// (same banks, never stored); the absent k-block reads the tap's zero block of the row's parity.
SPK_WN_HD constexpr int w_off(int cb, int lane, int s, int tap) {
  const int i = lane & 15, kb = kblock(lane >> 4, s);
  if (kb == 7) return tap * WTAP + WROWS * ROW + 8 * (perm16(i) & 1);
  const int r = 16 * cb + perm16(i) - (16 * cb + i >= CIN ? 16 : 0);
  return tap * WTAP + r * ROW + 8 * kb;
}

}  // namespace halo_wn

// the padded form's operands at 52 / 64 channels (HaloX3Cfg M16: rows of 80 halves, k-group kg
// takes channels 32 kg .. 32 kg + 31 of every tap, lane quarter g the k-block 4 kg + g)
namespace halo_pad {
constexpr int ROW = 80, NP = 32;
SPK_WN_HD constexpr int pix_off(int q, int lane, int kg) { return q * ROW + 8 * (lane >> 4) + 32 * kg; }
// channel 16 cb + (lane & 15) of the block's 32-channel slice, cb = 0 / 1
SPK_WN_HD constexpr int w_off(int cb, int lane, int kg, int tap) {
  return (tap * NP + 16 * cb + (lane & 15)) * ROW + 8 * (lane >> 4) + 32 * kg;
}
}  // namespace halo_pad

}  // namespace spk
