// Diagnostics (tests/conv_diag.py; not in include/spk_hip.h): launch one conv through
// spk::launch_conv from a plain-C mirror of ConvDesc, so that every kernel route can be
// checked one launch at a time.  Uses only symbols that the host emulation defines too
// (launch_conv, conv_kernel_name, launch_split_f16, frag_halves, launch_pack_frag), so the
// same entry drives libspk_hip.so and tests/emu/libspk_emu.so.  Allocates nothing and does
// not synchronise: every buffer is the caller's.
#include <cstring>
#include <exception>
#include <string>

#include "common.h"
#include "misc.h"
#include "runtime.h"

extern "C" {

// ConvSrc (common.h), field for field
struct spk_diag_src_t {
  const float* p;
  const float* p2;
  int32_t ld, ld2;
  int32_t H, W;
  int32_t cin;
  int32_t kh, kw, sh, sw, ph, pw, dh, dw;
  int32_t reflect;
  const float* pre_scale;
  const float* pre_shift;
  const int32_t* vlen;
};

// ConvDesc (common.h) without run_if (launch_conv sets it), plus the caller's buffers for
// the split planes and the fragment pack
struct spk_diag_conv_t {
  spk_diag_src_t s0, s1;
  int32_t nimg, Ho, Wo;
  int32_t N, K, Kp;
  const float* w;          // [N][Kp]: N * Kp floats, like wh / wl below (N * Kp halves each)
  // 0: no planes (exact-fp32 GEMM, persistent / plain halo), 1: hi / lo planes,
  // 2: hi / lo planes and the fragment pack (LDS-DMA GEMM)
  int32_t planes;
  uint16_t* wh;            // planes >= 1: [N][Kp] halves each, written here
  uint16_t* wl;
  uint16_t* wf;            // planes == 2: spk_diag_frag_halves(N, Kp) halves, written here
  const float* bias;
  const float* rowbias; int32_t rowbias_ld;
  float* out; int32_t ldo;
  int32_t osplit; int64_t oplane;
  int32_t act, act2;
  const float* res; int32_t ldr;
  const float* post_scale;
  const float* post_shift;
  const float* affx; int32_t ldx;
  const float* affy; int32_t ldy;
  const float* gate; int32_t gate_ld, gate_seg, gate_nseg;
  int32_t ksplit; float* partial;
  const int32_t* rowlen;
  int32_t* range_flag;
  int32_t x1, wbig, kcb;
  const int32_t* range_in;
};

}  // extern "C"

namespace {

using namespace spk;

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

int hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return SPK_OK;
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return SPK_E_HIP;
}

ConvSrc to_src(const spk_diag_src_t& s) {
  ConvSrc r;
  r.p = s.p; r.p2 = s.p2; r.ld = s.ld; r.ld2 = s.ld2; r.H = s.H; r.W = s.W; r.cin = s.cin;
  r.kh = s.kh; r.kw = s.kw; r.sh = s.sh; r.sw = s.sw; r.ph = s.ph; r.pw = s.pw; r.dh = s.dh; r.dw = s.dw;
  r.reflect = s.reflect; r.pre_scale = s.pre_scale; r.pre_shift = s.pre_shift; r.vlen = s.vlen;
  return r;
}

}  // namespace

extern "C" {

int spk_diag_frag_halves(int32_t N, int32_t Kp, size_t* halves) {
  return guarded([&]() -> int {
    if (!halves || N <= 0 || Kp <= 0) {
      set_error("spk_diag_frag_halves: invalid argument");
      return SPK_E_INVALID;
    }
    *halves = frag_halves(N, Kp);
    return SPK_OK;
  });
}

// Splits (planes >= 1) and fragment-packs (planes == 2) the weights on `stream`, writes the
// name of the kernel launch_conv will pick into `kernel`, then launches the conv.
int spk_diag_conv(const spk_diag_conv_t* c, char* kernel, int32_t kernel_len, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->w || !c->out || c->planes < 0 || c->planes > 2 || (c->planes >= 1 && (!c->wh || !c->wl)) ||
        (c->planes == 2 && !c->wf) || (kernel && kernel_len <= 0)) {
      set_error("spk_diag_conv: invalid argument");
      return SPK_E_INVALID;
    }
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ConvDesc d;
    d.s0 = to_src(c->s0);
    d.s1 = to_src(c->s1);
    d.nimg = c->nimg; d.Ho = c->Ho; d.Wo = c->Wo;
    d.N = c->N; d.K = c->K; d.Kp = c->Kp;
    d.w = c->w;
    d.bias = c->bias;
    d.rowbias = c->rowbias; d.rowbias_ld = c->rowbias_ld;
    d.out = c->out; d.ldo = c->ldo;
    d.osplit = c->osplit; d.oplane = c->oplane;
    d.act = c->act; d.act2 = c->act2;
    d.res = c->res; d.ldr = c->ldr;
    d.post_scale = c->post_scale; d.post_shift = c->post_shift;
    d.affx = c->affx; d.ldx = c->ldx;
    d.affy = c->affy; d.ldy = c->ldy;
    d.gate = c->gate; d.gate_ld = c->gate_ld; d.gate_seg = c->gate_seg; d.gate_nseg = c->gate_nseg;
    d.ksplit = c->ksplit; d.partial = c->partial;
    d.rowlen = c->rowlen;
    d.range_flag = c->range_flag;
    d.x1 = c->x1; d.wbig = c->wbig; d.kcb = c->kcb;
    d.range_in = c->range_in;
    if (c->planes >= 1) { d.wh = c->wh; d.wl = c->wl; }
    if (c->planes == 2) d.wf = c->wf;
    // the name first: it depends on the descriptor alone, and a caller reads it even when a
    // launch below fails.  A descriptor without outputs has no kernel (the tile selection
    // divides by the output size; launch_conv refuses such a descriptor before it gets there)
    if (kernel) {
      const bool sized = d.N > 0 && d.nimg > 0 && d.Ho > 0 && d.Wo > 0;
      const std::string name = sized ? conv_kernel_name(d) : std::string();
      std::strncpy(kernel, name.c_str(), (size_t)kernel_len - 1);
      kernel[kernel_len - 1] = '\0';
    }
    // The split and the pack run over N * Kp elements of the caller's w / wh / wl (and
    // spk_diag_frag_halves(N, Kp) halves of wf), which the caller sized for a descriptor that
    // launch_conv accepts.  A descriptor whose weight matrix launch_conv's host check refuses
    // (N, Kp alignment, K <= Kp, alignment of w) is therefore neither split nor packed: it
    // goes to launch_conv as it is, which refuses it before any kernel reads the planes.
    const bool weights_ok = c->N > 0 && c->Kp > 0 && c->Kp % 32 == 0 && c->K <= c->Kp &&
                            (reinterpret_cast<uintptr_t>(c->w) & 15) == 0;
    if (c->planes >= 1 && weights_ok)
      if (int rc = hip_check(launch_split_f16(c->w, c->wh, c->wl, (size_t)c->N * c->Kp, s), "spk_diag_conv: split"))
        return rc;
    if (c->planes == 2 && weights_ok)
      if (int rc = hip_check(launch_pack_frag(c->wh, c->wl, c->N, c->Kp, c->wf, s), "spk_diag_conv: fragment pack"))
        return rc;
    return hip_check(launch_conv(d, s), "spk_diag_conv");
  });
}

}  // extern "C"
