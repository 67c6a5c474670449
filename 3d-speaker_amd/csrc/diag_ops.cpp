// Diagnostics (tests/op_diag.py; not in include/spk_hip.h): one launch of each kernel entry
// that is not a conv -- the fused AFF (aff.h), the fused Res2Net block (res2block.h), the TDNN
// reductions (tdnn_ops.h) and the small kernels of misc.h -- from plain-C mirrors of their
// descriptors and argument lists, so that every kernel can be checked one launch at a time.
// Uses only symbols that the host emulation defines too, so the same entries drive
// libspk_hip.so and tests/emu/libspk_emu.so.  Allocates nothing and does not synchronise:
// every buffer is the caller's.
#include <cstring>
#include <exception>
#include <string>

#include "aff.h"
#include "common.h"
#include "misc.h"
#include "res2block.h"
#include "runtime.h"
#include "tdnn_ops.h"

extern "C" {

// AffDesc (aff.h); w1 / w2 are fp32 in the kernel's packed layout ([nmid][kp1], [cp][kp2]),
// the hi / lo planes are buffers of the same element counts that the entry fills
struct spk_diag_aff_t {
  const float* x; int32_t ldx;
  const float* y; int32_t ldy;
  float* out; int32_t ldo;
  int32_t M, cp, nmid;
  const float* w1; uint16_t* w1h; uint16_t* w1l; const float* b1; int32_t kp1;
  const float* w2; uint16_t* w2h; uint16_t* w2l; const float* b2; int32_t kp2;
  int32_t* range_flag;
};

// Res2Desc (res2block.h); w1 [64][C], wa / wb [32][9*32], w3 [Cout][64 (+C)] in fp32, planes as above
struct spk_diag_res2_t {
  const float* x; float* out;
  int32_t nimg, H, W, C, Cout, stride, Hin, Win, proj, width;
  const float* w1; uint16_t* w1h; uint16_t* w1l; const float* b1;
  const float* wa; uint16_t* wah; uint16_t* wal; const float* ba;
  const float* wb; uint16_t* wbh; uint16_t* wbl; const float* bb;
  const float* w3; uint16_t* w3h; uint16_t* w3l; const float* b3;
};

// tdnn_ops.h, argument for argument
struct spk_diag_time_mean_t { const float* x; int32_t B, T, C, ld; float* out; int32_t ldo; const int32_t* vlen; };
struct spk_diag_asp_stats_t { const float* x; int32_t B, T, C, ld; float eps; float* out; const int32_t* vlen; };
struct spk_diag_attn_pool_t {
  const float* logit; int32_t ldl; const float* x; int32_t ldx; int32_t B, T, C; float eps; float* out;
  const int32_t* vlen;
};
struct spk_diag_se_apply_t {
  const float* x; int32_t ldx; const float* gate; int32_t ldg; const float* res; int32_t ldr; float* out; int32_t ldo;
  int32_t B, T, C; int32_t* range_flag;
};
struct spk_diag_cam_context_t {
  const float* x; int32_t B, T, C, ld, seg, nseg; float* out; int32_t ldo; const int32_t* vlen;
};
struct spk_diag_cam_gate_t {
  const float* x; int32_t B, T, C, ld, seg, nseg;
  const float* w1; int32_t k1p; const float* b1; int32_t red;
  const float* w2; int32_t k2p; const float* b2; int32_t growth;
  float* gate; int32_t ldg; float* segsum; const int32_t* vlen;
};
struct spk_diag_stats_pool_t { const float* x; int32_t B, T, C, ld; float* out; const int32_t* vlen; };
struct spk_diag_derive_len_t { const int32_t* in; int32_t* out; int32_t B, pad, k, stride; };

// misc.h, argument for argument
struct spk_diag_stem_t {
  const float* feats; int32_t B, T, F; const float* w; const float* bias; int32_t cout, act, wstride; float* out;
  int32_t ldo; const int32_t* vlen; int32_t* range_flag;
};
struct spk_diag_word_reset_t { int32_t* w; };
struct spk_diag_range_check_t { const float* x; size_t n; int32_t* flag; };
struct spk_diag_split_f16_t { const float* w; uint16_t* hi; uint16_t* lo; size_t n; };
struct spk_diag_tstp_t {
  const float* x; int32_t B, H, W, C, ld; float eps; int32_t unbiased; float* out; int32_t parts;
};
struct spk_diag_astp_pool_t {
  const float* logit; int32_t ldl; const float* x; int32_t ldx; int32_t B, F, T, C; float* out;
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

// a launch function's own refusal (its host check) is SPK_E_INVALID, anything else a HIP error
int hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return SPK_OK;
  if (e == hipErrorInvalidValue) {
    set_error(std::string(what) + ": refused by the host check");
    return SPK_E_INVALID;
  }
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return SPK_E_HIP;
}

int invalid(const char* what) {
  set_error(std::string(what) + ": invalid argument");
  return SPK_E_INVALID;
}

void put_name(char* kernel, int32_t kernel_len, const std::string& name) {
  if (!kernel) return;
  std::strncpy(kernel, name.c_str(), (size_t)kernel_len - 1);
  kernel[kernel_len - 1] = '\0';
}

hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace

extern "C" {

// Splits w1 / w2 into the caller's planes on `stream`, writes the name of the kernel
// launch_aff_x3 will pick into `kernel`, then launches.
int spk_diag_aff(const spk_diag_aff_t* c, char* kernel, int32_t kernel_len, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->w1 || !c->w2 || !c->w1h || !c->w1l || !c->w2h || !c->w2l || (kernel && kernel_len <= 0))
      return invalid("spk_diag_aff");
    const hipStream_t s = as_stream(stream);
    AffDesc a;
    a.x = c->x; a.ldx = c->ldx; a.y = c->y; a.ldy = c->ldy; a.out = c->out; a.ldo = c->ldo;
    a.M = c->M; a.cp = c->cp; a.nmid = c->nmid;
    a.w1 = c->w1; a.w1h = c->w1h; a.w1l = c->w1l; a.b1 = c->b1; a.kp1 = c->kp1;
    a.w2 = c->w2; a.w2h = c->w2h; a.w2l = c->w2l; a.b2 = c->b2; a.kp2 = c->kp2;
    a.range_flag = c->range_flag;
    // the planes were sized for a descriptor that launch_aff_x3 accepts: one whose weight shapes
    // its host check refuses is not split, it goes to the launch as it is
    const bool shaped = aff_x3_supported(c->cp, c->nmid) && c->kp1 >= 2 * c->cp && c->kp2 >= c->nmid;
    put_name(kernel, kernel_len, shaped ? aff_x3_kernel_name(c->cp, c->nmid) : "");
    if (shaped) {
      if (int rc = hip_check(launch_split_f16(c->w1, c->w1h, c->w1l, (size_t)c->nmid * c->kp1, s), "spk_diag_aff: split w1"))
        return rc;
      if (int rc = hip_check(launch_split_f16(c->w2, c->w2h, c->w2l, (size_t)c->cp * c->kp2, s), "spk_diag_aff: split w2"))
        return rc;
    }
    return hip_check(launch_aff_x3(a, s), "spk_diag_aff");
  });
}

// The same for the fused Res2Net block: the four weight matrices are split on `stream`, the
// descriptor carries the planes and the fp32 matrices both.  A null plane buffer goes to
// launch_res2_block as it is (which refuses it); the other matrices are still split.
int spk_diag_res2(const spk_diag_res2_t* c, char* kernel, int32_t kernel_len, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->w1 || !c->wa || !c->wb || !c->w3 || (kernel && kernel_len <= 0)) return invalid("spk_diag_res2");
    const hipStream_t s = as_stream(stream);
    Res2Desc d;
    d.x = c->x; d.out = c->out;
    d.nimg = c->nimg; d.H = c->H; d.W = c->W; d.C = c->C; d.Cout = c->Cout;
    d.stride = c->stride; d.Hin = c->Hin; d.Win = c->Win; d.proj = c->proj != 0; d.width = c->width;
    d.w1h = c->w1h; d.w1l = c->w1l; d.b1 = c->b1;
    d.wah = c->wah; d.wal = c->wal; d.ba = c->ba;
    d.wbh = c->wbh; d.wbl = c->wbl; d.bb = c->bb;
    d.w3h = c->w3h; d.w3l = c->w3l; d.b3 = c->b3;
    d.w1 = c->w1; d.wa = c->wa; d.wb = c->wb; d.w3 = c->w3;
    put_name(kernel, kernel_len, res2_block_supported(d) ? res2_block_kernel_name(d) : "");
    // the packed sizes of the two shapes the kernel has (C 64 with the projection, C 128 without);
    // any other C is refused below before a plane is read
    const bool shaped = c->proj ? c->C == 64 : c->C == 128;
    const int co = c->Cout ? c->Cout : c->C;
    if (shaped && co == 128) {
      struct { const float* w; uint16_t* h; uint16_t* l; size_t n; } m[4] = {
          {c->w1, c->w1h, c->w1l, (size_t)64 * c->C},
          {c->wa, c->wah, c->wal, (size_t)32 * 288},
          {c->wb, c->wbh, c->wbl, (size_t)32 * 288},
          {c->w3, c->w3h, c->w3l, (size_t)co * (c->proj ? 64 + c->C : 64)}};
      for (const auto& e : m)
        if (e.h && e.l)
          if (int rc = hip_check(launch_split_f16(e.w, e.h, e.l, e.n, s), "spk_diag_res2: split")) return rc;
    }
    return hip_check(launch_res2_block(d, s), "spk_diag_res2");
  });
}

int spk_diag_time_mean(const spk_diag_time_mean_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->x || !c->out) return invalid("spk_diag_time_mean");
    return hip_check(launch_time_mean(c->x, c->B, c->T, c->C, c->ld, c->out, c->ldo, as_stream(stream), c->vlen),
                     "spk_diag_time_mean");
  });
}

int spk_diag_asp_stats(const spk_diag_asp_stats_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->x || !c->out) return invalid("spk_diag_asp_stats");
    return hip_check(launch_asp_stats(c->x, c->B, c->T, c->C, c->ld, c->eps, c->out, as_stream(stream), c->vlen),
                     "spk_diag_asp_stats");
  });
}

int spk_diag_attn_pool(const spk_diag_attn_pool_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->logit || !c->x || !c->out) return invalid("spk_diag_attn_pool");
    return hip_check(launch_attn_pool(c->logit, c->ldl, c->x, c->ldx, c->B, c->T, c->C, c->eps, c->out,
                                      as_stream(stream), c->vlen), "spk_diag_attn_pool");
  });
}

int spk_diag_se_apply(const spk_diag_se_apply_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->x || !c->gate || !c->res || !c->out) return invalid("spk_diag_se_apply");
    return hip_check(launch_se_apply(c->x, c->ldx, c->gate, c->ldg, c->res, c->ldr, c->out, c->ldo, c->B, c->T, c->C,
                                     as_stream(stream), c->range_flag), "spk_diag_se_apply");
  });
}

int spk_diag_cam_context(const spk_diag_cam_context_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->x || !c->out) return invalid("spk_diag_cam_context");
    return hip_check(launch_cam_context(c->x, c->B, c->T, c->C, c->ld, c->seg, c->nseg, c->out, c->ldo,
                                        as_stream(stream), c->vlen), "spk_diag_cam_context");
  });
}

// writes the name of the kernel(s) launch_cam_gate will run into `kernel`, then launches
int spk_diag_cam_gate(const spk_diag_cam_gate_t* c, char* kernel, int32_t kernel_len, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->x || !c->w1 || !c->w2 || !c->gate || !c->segsum || (kernel && kernel_len <= 0))
      return invalid("spk_diag_cam_gate");
    put_name(kernel, kernel_len,
             cam_gate_kernel_name(c->B, c->C, c->ld, c->nseg, c->w1, c->k1p, c->red, c->w2, c->k2p, c->growth));
    return hip_check(launch_cam_gate(c->x, c->B, c->T, c->C, c->ld, c->seg, c->nseg, c->w1, c->k1p, c->b1, c->red,
                                     c->w2, c->k2p, c->b2, c->growth, c->gate, c->ldg, c->segsum, as_stream(stream),
                                     c->vlen), "spk_diag_cam_gate");
  });
}

int spk_diag_stats_pool(const spk_diag_stats_pool_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->x || !c->out) return invalid("spk_diag_stats_pool");
    return hip_check(launch_stats_pool(c->x, c->B, c->T, c->C, c->ld, c->out, as_stream(stream), c->vlen),
                     "spk_diag_stats_pool");
  });
}

int spk_diag_derive_len(const spk_diag_derive_len_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->in || !c->out || c->stride <= 0) return invalid("spk_diag_derive_len");
    return hip_check(launch_derive_len(c->in, c->out, c->B, c->pad, c->k, c->stride, as_stream(stream)),
                     "spk_diag_derive_len");
  });
}

int spk_diag_stem(const spk_diag_stem_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->feats || !c->w || !c->bias || !c->out) return invalid("spk_diag_stem");
    return hip_check(launch_stem_conv3x3(c->feats, c->B, c->T, c->F, c->w, c->bias, c->cout, c->act, c->wstride,
                                         c->out, c->ldo, as_stream(stream), c->vlen, c->range_flag), "spk_diag_stem");
  });
}

int spk_diag_word_reset(const spk_diag_word_reset_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->w) return invalid("spk_diag_word_reset");
    return hip_check(launch_word_reset(c->w, as_stream(stream)), "spk_diag_word_reset");
  });
}

int spk_diag_range_check(const spk_diag_range_check_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->x) return invalid("spk_diag_range_check");
    return hip_check(launch_range_check(c->x, c->n, c->flag, as_stream(stream)), "spk_diag_range_check");
  });
}

int spk_diag_split_f16(const spk_diag_split_f16_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->w || !c->hi || !c->lo) return invalid("spk_diag_split_f16");
    return hip_check(launch_split_f16(c->w, c->hi, c->lo, c->n, as_stream(stream)), "spk_diag_split_f16");
  });
}

int spk_diag_tstp(const spk_diag_tstp_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->x || !c->out) return invalid("spk_diag_tstp");
    return hip_check(launch_tstp(c->x, c->B, c->H, c->W, c->C, c->ld, c->eps, c->unbiased, c->out, as_stream(stream),
                                 c->parts), "spk_diag_tstp");
  });
}

int spk_diag_astp_pool(const spk_diag_astp_pool_t* c, void* stream) {
  return guarded([&]() -> int {
    if (!c || !c->logit || !c->x || !c->out) return invalid("spk_diag_astp_pool");
    return hip_check(launch_astp_pool(c->logit, c->ldl, c->x, c->ldx, c->B, c->F, c->T, c->C, c->out,
                                      as_stream(stream)), "spk_diag_astp_pool");
  });
}

}  // extern "C"
