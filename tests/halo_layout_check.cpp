// Host check of csrc/halo_whole_n.h (built and run by test_halo_whole_n_layout.py): the whole-N
// form's compact fragment addressing fetches the operands the padded layout's does, over all
// lanes, steps, taps and blocks, for 52 and 50 real input channels; each lane group of a
// ds_read_b128 stays on distinct banks.  Prints "ok" and the counts; any mismatch exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "halo_whole_n.h"

using namespace spk;
namespace L = spk::halo_wn;
namespace P = spk::halo_pad;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// logical operands: distinct non-zero values, so a wrong address cannot match by accident
static float xval(int q, int c, int creal) { return c < 52 ? (c < creal ? 1.0f : 1000.0f) + q * 64 + c : 0.0f; }
static float wval(int tap, int n, int c, int creal) { return (n < 52 && c < creal) ? 0.5f + (tap * 64 + n) * 64 + c : 0.0f; }

// the four lane groups of a ds_read_b128 (one LDS cycle each when their banks are distinct)
static int lane_group(int lane) {
  const int l = lane & 31, hi = lane >> 5;
  const bool first = l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28);
  return 2 * hi + (first ? 0 : 1);
}
// extra LDS cycles of one wave-wide 16-byte read at byte offsets off[lane]: per group, addresses
// that differ but share a bank (identical addresses broadcast)
static int conflicts(const int (&off_halves)[64]) {
  int extra = 0;
  for (int grp = 0; grp < 4; ++grp) {
    std::set<int> units[16];
    for (int lane = 0; lane < 64; ++lane)
      if (lane_group(lane) == grp) units[(off_halves[lane] / 8) % 16].insert(off_halves[lane] / 8);
    int worst = 1;
    for (auto& u : units) worst = std::max<int>(worst, (int)u.size());
    extra += worst - 1;
  }
  return extra;
}

int main() {
  // the permutations
  {
    bool seen[16] = {};
    for (int i = 0; i < 16; ++i) {
      CHECK(L::perm16(i) >= 0 && L::perm16(i) < 16 && !seen[L::perm16(i)], "perm16(%d)", i);
      seen[L::perm16(i)] = true;
      CHECK(L::perm16_inv(L::perm16(i)) == i, "perm16_inv");
    }
    bool kb[8] = {};
    for (int s = 0; s < 2; ++s)
      for (int g = 0; g < 4; ++g) {
        CHECK(!kb[L::kblock(g, s)], "kblock(%d, %d) twice", g, s);
        kb[L::kblock(g, s)] = true;
      }
    for (int n = 0; n < 52; ++n) {
      CHECK(L::wrow(n) < L::WROWS, "wrow(%d) = %d", n, L::wrow(n));
      CHECK(L::wrow_channel(L::wrow(n)) == n, "wrow_channel");
    }
  }
  long ops = 0;
  for (int creal : {52, 50}) {
    for (int TW : {8, 16, 32}) {
      const int TH = 128 / TW, HW = TW + 2, HH = TH + 2;
      // LDS images: one plane each (hi and lo planes share the addressing)
      std::vector<float> hp(204 * P::ROW, 0.f), hc(L::HPLANE, -7.f);
      for (int q = 0; q < HH * HW; ++q)
        for (int c = 0; c < 64; ++c) {
          hp[q * P::ROW + c] = xval(q, c, creal);
          if (c < L::ROW) hc[q * L::ROW + c] = xval(q, c, creal);
        }
      std::vector<float> wp[2], wc(L::WPLANE, -7.f);
      for (int sl = 0; sl < 2; ++sl) {
        wp[sl].assign(9 * P::NP * P::ROW, 0.f);
        for (int tap = 0; tap < 9; ++tap)
          for (int n = 0; n < 32; ++n)
            for (int c = 0; c < 64; ++c) wp[sl][(tap * P::NP + n) * P::ROW + c] = wval(tap, 32 * sl + n, c, creal);
      }
      for (int tap = 0; tap < 9; ++tap) {
        for (int r = 0; r < L::WROWS; ++r)   // the kernel's staging: row position r holds wrow_channel(r)
          for (int c = 0; c < L::ROW; ++c) wc[tap * L::WTAP + r * L::ROW + c] = wval(tap, L::wrow_channel(r), c, creal);
        for (int z = 0; z < 16; ++z) wc[tap * L::WTAP + L::WROWS * L::ROW + z] = 0.f;
      }
      for (int tap = 0; tap < 9; ++tap) {
        const int tq = (tap / 3) * HW + tap % 3;
        for (int s = 0; s < 2; ++s) {
          // pixel operands: every 16-pixel block of the tile
          for (int blk = 0; blk < 8; ++blk) {
            int off[64];
            for (int lane = 0; lane < 64; ++lane) {
              const int p = 16 * blk + L::lane_pixel(lane), q = (p / TW) * HW + p % TW + tq;
              const int kb = L::kblock(lane >> 4, s);
              off[lane] = L::pix_off(q, lane, s);
              CHECK(off[lane] >= 0 && off[lane] + 8 <= L::HPLANE && off[lane] % 8 == 0, "pixel offset");
              if (kb == 7) continue;   // meets the weights' zero block
              // the padded form's lane for the same pixel and k-block: quarter kb % 4, group kb / 4
              const int pl = (p & 15) + 16 * (kb % 4);
              const int po = P::pix_off(q, pl, kb / 4);
              CHECK(std::memcmp(&hc[off[lane]], &hp[po], 8 * sizeof(float)) == 0, "pixel operand tap %d s %d lane %d", tap, s, lane);
              ++ops;
            }
            if (TW != 8) CHECK(conflicts(off) == 0, "pixel banks TW %d tap %d s %d blk %d", TW, tap, s, blk);
            else CHECK(conflicts(off) <= 4, "pixel banks TW 8");
          }
          // weight operands: the four 16-channel blocks
          for (int cb = 0; cb < 4; ++cb) {
            int off[64];
            for (int lane = 0; lane < 64; ++lane) {
              const int n = 16 * cb + (lane & 15), kb = L::kblock(lane >> 4, s);
              off[lane] = L::w_off(cb, lane, s, tap);
              CHECK(off[lane] >= 0 && off[lane] + 8 <= L::WPLANE && off[lane] % 8 == 0, "weight offset");
              if (n >= 52) continue;   // no such channel: never stored
              float want[8] = {};
              if (kb < 7) {
                const int po = P::w_off((cb & 1), (lane & 15) + 16 * (kb % 4), kb / 4, tap);
                std::memcpy(want, &wp[cb >> 1][po], sizeof want);
              } else {                 // the padded layout's k-block 7 is zero padding
                const int po = P::w_off((cb & 1), (lane & 15) + 16 * 3, 1, tap);
                for (int e = 0; e < 8; ++e) CHECK(wp[cb >> 1][po + e] == 0.f, "padded k-block 7");
              }
              CHECK(std::memcmp(&wc[off[lane]], want, sizeof want) == 0, "weight operand tap %d s %d cb %d lane %d", tap, s, cb, lane);
              ++ops;
            }
            CHECK(conflicts(off) == 0, "weight banks tap %d s %d cb %d", tap, s, cb);
          }
        }
      }
    }
  }
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("ok %ld operands, LDS %d bytes\n", ops, L::LDS_BYTES);
  return 0;
}
