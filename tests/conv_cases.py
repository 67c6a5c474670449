"""TEST INFRASTRUCTURE: the table of direct conv cases (one spk::launch_conv each, through
csrc/diag_conv.cpp) and the code that builds a case's tensors, launches it and checks it
against tests/conv_ref.py.  Consumed twice: test_conv_contract_emu.py (host emulation, no
GPU) and test_gpu_conv_kernels.py (the real kernels).

Inputs: activations uniform in [0, 2), weights uniform in [-1, 1] / sqrt(K) (the
distributions of tools/gemm_bench.cpp; no value is zero, so a dropped or misplaced product
shows).  Padded input channels (zero weights) hold 1e3, frames at or past vlen hold
1e4 * randn, and every leading dimension is larger than its channel count.

Range word: `big_out` cases pass 2^14 through the bias (every third bias x 3e5: the epilogue's
note is exercised with in-range operands, and since |bias| is part of mag the bound on those
columns is loose); `range_in` cases (fp16x3 / fp16 kernels, scaled split) and `big_in` cases
(kernels without a split) scale the activations to 1e5, so the accumulator itself passes 2^14.
All three assert a non-zero word; `huge_masked` cases assert a zero one.

Bound, elementwise: |out - ref| <= c * mag * L + 4 * 2^-24 * |ref| (+ TRANS_T * |ref| for the
transcendental epilogues on the GPU), with mag and L from conv_ref.reference()."""
import math
import re

import torch

import conv_diag
import conv_ref
from conv_ref import ACT_NONE, ACT_RELU, ACT_HTANH, ACT_SILU, ACT_SIGMOID, ACT_TANH

C_EMU = 1e-6     # double accumulation, one rounding to fp32 (6e-8), 4x margin and the fp32 epilogue
C_X3 = 3e-6      # fp16x3 and exact-fp32 kernels: the project's bar (tools/gemm_bench.cpp)
C_X1 = 1e-3      # single fp16 product: each operand rounded once, 2^-10 + 2^-22 per product
EPS_EPI = 4 * 2.0 ** -24
# Extra relative allowance for SiLU / sigmoid / tanh / AFF epilogues on the GPU (fast
# intrinsics).  What was measured on an MI355X, over every transcendental case of this table,
# is the excess of |out - ref| over the plain bound above, relative to |ref|: it is 0 for
# every element (the intrinsics' own error was not separated from the accumulation error; the
# worst err / (mag L) of those cases is 2.2e-7 against c = 3e-6).  4 x 0 = 0: nothing is
# added, which is the stricter choice.
TRANS_T = 0.0

SENTINEL = 0x7FC5A5A5   # a NaN bit pattern no kernel produces
GUARD_ROWS = 8


def round_up(x, m):
    return (x + m - 1) // m * m


CASES = []


def case(name, fam, expect, **kw):
    d = dict(name=name, fam=fam, expect=expect, planes=1, k=(1, 1), s=(1, 1), d=(1, 1), p=None, reflect=0, add=0,
             pre=0, vlen=None, s1=None, kcb=0, ksplit=1, x1=0, wbig=0, bias=1, rowbias=0, res=0, aff=0,
             act=ACT_HTANH, act2=ACT_NONE, post=0, gate=0, rowlen=None, osplit=0, flag=0, big_out=0, range_in=0,
             huge_masked=0, big_in=0, cin_real=None)
    unknown = set(kw) - set(d) - {'nimg', 'H', 'W', 'cin', 'N'}
    assert not unknown, unknown
    d.update(kw)
    CASES.append(d)
    return d


def _b(v):
    return 'true' if v else 'false'


# ---------------------------------------------------------------------------- halo 3x3
# below any tile; tall and narrow; 33 wide: one column past a multiple of every tile width
HALO_GEO = [(3, 5, 7), (2, 80, 13), (2, 9, 33)]
# pick_tw() gives the fp16x3 kernel's 128-pixel tile width 8 on all three of those; these give 16
# and 32 (and the persistent kernel's 256-pixel tile width 32 on the first): two model shapes
HALO_GEO_TW = [(1, 40, 99), (2, 20, 50)]
HALO_TW = {(5, 7): 8, (80, 13): 8, (9, 33): 8, (40, 99): 16, (20, 50): 32}   # fp16x3 kernel, stride 1
HALO_CH = [(28, 28), (32, 32), (52, 52), (64, 64), (32, 64)]


def _halo_x3(cin, add, lean, sh=1, tw=r'\d+'):
    return rf'conv3x3_halo_x3_kernel<{cin}, {tw}, {_b(add)}, 128, \d+, {_b(lean)}, {sh}>'


for ci, (cin, n) in enumerate(HALO_CH):
    for gi, (nimg, h, w) in enumerate(HALO_GEO):
        case(f'halo_x3_{cin}to{n}_g{gi}_plain', 'halo_x3', _halo_x3(cin, 0, 1), nimg=nimg, H=h, W=w, cin=cin, N=n,
             k=(3, 3), cin_real=cin - 2 if cin in (28, 52) else None, flag=(gi == 0))
    # the epilogue variants, each on a geometry that rotates with the channel count
    for vi, (vname, vkw, lean) in enumerate([('add', dict(add=1), 1), ('res', dict(res=1), 0),
                                            ('post', dict(post=1, act=ACT_RELU), 0), ('rowlen', dict(rowlen='auto'), 0),
                                            ('osplit', dict(osplit='half'), 0)]):
        nimg, h, w = HALO_GEO[(ci + vi) % 3]
        case(f'halo_x3_{cin}to{n}_{vname}', 'halo_x3', _halo_x3(cin, vkw.get('add', 0), lean), nimg=nimg, H=h, W=w,
             cin=cin, N=n, k=(3, 3), **vkw)
    # every tile width x addend x lean / full epilogue: each is its own instantiation
    for nimg, h, w in HALO_GEO_TW + [HALO_GEO[(ci + 1) % 3]]:
        for vname, vkw, lean in [('plain', {}, 1), ('add', dict(add=1), 1), ('res', dict(res=1), 0),
                                 ('add_res', dict(add=1, res=1), 0)]:
            if (h, w) in HALO_GEO[0:3] and vname != 'add_res':
                continue   # the narrow geometries have these above
            case(f'halo_x3_{cin}to{n}_{h}x{w}_{vname}', 'halo_x3',
                 _halo_x3(cin, vkw.get('add', 0), lean, tw=HALO_TW[(h, w)]), nimg=nimg, H=h, W=w, cin=cin, N=n,
                 k=(3, 3), **vkw)
case('halo_x3_s2_h9', 'halo_x3', _halo_x3(32, 0, 1, 2), nimg=3, H=9, W=7, cin=32, N=32, k=(3, 3), s=(2, 1))
case('halo_x3_s2_h8', 'halo_x3', _halo_x3(32, 0, 0, 2), nimg=2, H=8, W=33, cin=32, N=64, k=(3, 3), s=(2, 1), res=1)
# stride 2 at every tile width (output 40 x 99 -> 16, 20 x 50 -> 32), lean and full epilogue
case('halo_x3_s2_80x99', 'halo_x3', _halo_x3(32, 0, 1, 2, tw=16), nimg=1, H=80, W=99, cin=32, N=32, k=(3, 3), s=(2, 1))
case('halo_x3_s2_80x99_res', 'halo_x3', _halo_x3(32, 0, 0, 2, tw=16), nimg=1, H=80, W=99, cin=32, N=64, k=(3, 3),
     s=(2, 1), res=1)
case('halo_x3_s2_40x50', 'halo_x3', _halo_x3(32, 0, 1, 2, tw=32), nimg=2, H=40, W=50, cin=32, N=64, k=(3, 3), s=(2, 1))
case('halo_x3_s2_h9_post', 'halo_x3', _halo_x3(32, 0, 0, 2, tw=8), nimg=3, H=9, W=7, cin=32, N=32, k=(3, 3), s=(2, 1),
     post=1, act=ACT_RELU)
case('halo_x3_range_up', 'halo_x3', _halo_x3(32, 0, 1), nimg=2, H=9, W=33, cin=32, N=32, k=(3, 3), flag=1, big_out=1,
     act=ACT_RELU)
case('halo_x3_range_masked', 'halo_x3', _halo_x3(64, 0, 0), nimg=2, H=9, W=33, cin=64, N=64, k=(3, 3), flag=1,
     rowlen='auto', huge_masked=1, act=ACT_RELU)
case('halo_x3_scaled', 'halo_x3', _halo_x3(52, 1, 1), nimg=2, H=9, W=33, cin=52, N=52, k=(3, 3), add=1, range_in=1,
     act=ACT_RELU, flag=1)
# without planes: the persistent kernel (N <= 32, cin 28 / 32) and the plain halo kernel
for cin, (nimg, h, w), add in [(28, HALO_GEO[0], 0), (32, HALO_GEO[1], 1), (32, HALO_GEO[2], 0)]:
    case(f'halo_persistent_{cin}_{h}x{w}', 'halo_f32', rf'conv3x3_halo_persistent_kernel<{cin}, \d+, {_b(add)}>',
         nimg=nimg, H=h, W=w, cin=cin, N=cin, k=(3, 3), planes=0, add=add, res=(h == 9), flag=(h == 5))
for cin in (28, 32):
    for (nimg, h, w), tw in [(HALO_GEO[0], 8), (HALO_GEO[1], 16), (HALO_GEO_TW[0], 32)]:
        for add in (0, 1):
            case(f'halo_persistent_{cin}_{h}x{w}_tw{tw}_add{add}', 'halo_f32',
                 rf'conv3x3_halo_persistent_kernel<{cin}, {tw}, {_b(add)}>', nimg=nimg, H=h, W=w, cin=cin, N=cin,
                 k=(3, 3), planes=0, add=add)
case('halo_persistent_range_masked', 'halo_f32', r'conv3x3_halo_persistent_kernel<32, \d+, false>', nimg=2, H=9, W=33,
     cin=32, N=32, k=(3, 3), planes=0, flag=1, rowlen='auto', huge_masked=1, act=ACT_RELU)
case('halo_persistent_big_in', 'halo_f32', r'conv3x3_halo_persistent_kernel<28, \d+, false>', nimg=2, H=9, W=33,
     cin=28, N=28, k=(3, 3), planes=0, flag=1, big_in=1, act=ACT_RELU)
case('halo_plain_range_masked', 'halo_f32', r'conv3x3_halo_kernel<64, 64, 128, false>', nimg=2, H=9, W=33, cin=64,
     N=64, k=(3, 3), planes=0, flag=1, rowlen='auto', huge_masked=1, act=ACT_RELU)
case('halo_plain_big_in', 'halo_f32', r'conv3x3_halo_kernel<52, 64, 128, false>', nimg=2, H=9, W=33, cin=52, N=52,
     k=(3, 3), planes=0, flag=1, big_in=1, act=ACT_RELU)
for cin, n, (nimg, h, w), pix, add in [(52, 52, HALO_GEO[1], 256, 0), (52, 52, HALO_GEO[0], 128, 1),
                                       (64, 64, HALO_GEO[0], 128, 0), (64, 64, HALO_GEO[1], 256, 1),
                                       (32, 64, HALO_GEO[2], 128, 0)]:
    case(f'halo_plain_{cin}to{n}_{h}x{w}', 'halo_f32', rf'conv3x3_halo_kernel<{cin}, 64, {pix}, {_b(add)}>', nimg=nimg,
         H=h, W=w, cin=cin, N=n, k=(3, 3), planes=0, add=add, rowlen='auto' if h == 80 else None, flag=(h == 5),
         big_out=(h == 5 and cin == 64), act=ACT_RELU)

# ---------------------------------------------------------------------------- persistent short-K 1x1 (pw)
PW_GEO = dict(nimg=3, H=80, W=275)   # M = 66000: a multiple of neither 128 nor 256


def _pw(kp, bn, s1, res):
    return rf'pw_gemm_x3_kernel<{kp}, {bn}, {_b(s1)}, {_b(res)}>'


case('pw_k32_n28', 'pw', _pw(32, 32, 0, 0), cin=28, N=28, cin_real=26, **PW_GEO)
case('pw_k32_n28_res', 'pw', _pw(32, 32, 0, 1), cin=28, N=28, res=1, flag=1, **PW_GEO)
case('pw_k64_n52', 'pw', _pw(64, 64, 0, 0), cin=52, N=52, act=ACT_RELU, post=1, **PW_GEO)
case('pw_k64_n52_res', 'pw', _pw(64, 64, 0, 1), cin=64, N=52, res=1, **PW_GEO)
case('pw_k64_n104', 'pw', _pw(64, 128, 0, 0), cin=64, N=104, osplit='half', **PW_GEO)
case('pw_k64_n104_res', 'pw', _pw(64, 128, 0, 1), cin=52, N=104, res=1, **PW_GEO)
case('pw_k128_n64', 'pw', _pw(128, 64, 0, 0), cin=128, N=64, act=ACT_SILU, **PW_GEO)
case('pw_k128_n64_res', 'pw', _pw(128, 64, 0, 1), cin=104, N=64, res=1, **PW_GEO)
case('pw_k128_n208', 'pw', _pw(128, 128, 0, 0), cin=128, N=208, flag=1, big_out=1, act=ACT_NONE, **PW_GEO)
case('pw_k128_n208_res', 'pw', _pw(128, 128, 0, 1), cin=128, N=208, res=1, **PW_GEO)
case('pw_s1', 'pw', _pw(128, 128, 1, 0), cin=64, N=104, s1=dict(cin=64, stride=1), **PW_GEO)
case('pw_s1_res', 'pw', _pw(128, 64, 1, 1), cin=64, N=64, s1=dict(cin=64, stride=1), res=1, **PW_GEO)
case('pw_stride2', 'pw', _pw(64, 128, 0, 0), nimg=3, H=159, W=549, cin=64, N=104, s=(2, 2), p=(0, 0))
case('pw_scaled', 'pw', _pw(64, 64, 0, 0), cin=64, N=64, range_in=1, flag=1, act=ACT_RELU, **PW_GEO)

# ---------------------------------------------------------------------------- LDS-DMA fragment GEMM
F128 = r'conv_gemm_x3f_kernel<128, 128, 2, 4, %d>'
F_GEO = dict(nimg=1, H=17, W=241)   # M = 4097: the first M the route takes
case('f_1x1_k208', 'gemm_f', F128 % 0, cin=208, N=104, planes=2, res=1, **F_GEO)
case('f_3x3_c104', 'gemm_f', F128 % 0, cin=104, N=104, k=(3, 3), planes=2, flag=1, **F_GEO)
case('f_3x3_add', 'gemm_f', F128 % 1, cin=104, N=104, k=(3, 3), planes=2, add=1, act=ACT_RELU, **F_GEO)
case('f_s1_stride2', 'gemm_f', F128 % 2, cin=208, N=104, planes=2, s1=dict(cin=128, stride=2), **F_GEO)
case('f_ksplit2', 'gemm_f', F128 % 0, cin=512, N=104, planes=2, ksplit=2, **F_GEO)
case('f_aff', 'gemm_f', F128 % 0, cin=256, N=104, planes=2, aff=1, **F_GEO)
case('f_range_up', 'gemm_f', F128 % 0, cin=208, N=104, planes=2, flag=1, big_out=1, act=ACT_NONE, **F_GEO)
case('f_range_masked', 'gemm_f', F128 % 0, nimg=3, H=20, W=70, cin=208, N=104, planes=2, flag=1, rowlen='auto',
     huge_masked=1, act=ACT_RELU)   # M = 4200
case('f_scaled', 'gemm_f', F128 % 0, cin=208, N=104, planes=2, range_in=1, flag=1, act=ACT_RELU, **F_GEO)
# the 256x256 tile: geometry by f_tile()'s rule for the device's CU count (f256_geometry)
case('f_256x256', 'gemm_f', r'conv_gemm_x3f_kernel<256, 256, 2, 4, 0>', nimg=2, H=100, W='f256', cin=512, N=208,
     planes=2, res=1)

# ---------------------------------------------------------------------------- tiled fp16x3 / fp16 / exact fp32
def _x3(bm, bn, wm, wn, s1=0, add=0, pre=0, buf=1):
    return f'conv_gemm_x3_kernel<{bm}, {bn}, {wm}, {wn}, {_b(s1)}, {_b(add)}, {_b(pre)}, {_b(buf)}>'


def _x1(bm, bn, wm, wn, s1=0, add=0, pre=0):
    return f'conv_gemm_x1_kernel<{bm}, {bn}, {wm}, {wn}, {_b(s1)}, {_b(add)}, {_b(pre)}>'


def _f32(bm, bn, bk, wm, wn, s1=0, add=0, pre=0):
    return f'conv_gemm_kernel<{bm}, {bn}, {bk}, {wm}, {wn}, {_b(s1)}, {_b(add)}, {_b(pre)}>'


T64x32 = dict(nimg=3, H=1, W=50, N=32, k=(1, 3))                 # M = 150
T256x32 = dict(nimg=1000, H=1, W=131, N=32, k=(1, 3))            # M = 131000: 512 row tiles
T256x64 = dict(nimg=3, H=10, W=10, N=64)                         # M = 300
T64x128 = dict(nimg=1, H=64, W=64, N=104)                        # M = 4096 exactly
T128x128 = dict(nimg=1, H=17, W=241, N=104)                      # M = 4097
T256x128 = dict(nimg=1, H=34, W=482, cin=512, N=512, k=(3, 3), s=(2, 2))   # M = 17 * 241 = 4097, K = 4608

case('x3_64x32_relu', 'x3', _x3(64, 32, 2, 1), cin=64, act=ACT_RELU, flag=1, **T64x32)
case('x3_64x32_add_silu', 'x3', _x3(64, 32, 2, 1, add=1), cin=64, add=1, act=ACT_SILU, **T64x32)
case('x3_256x32_pre_gate', 'x3', _x3(256, 32, 8, 1, pre=1), cin=128, pre=1, gate=100, act=ACT_RELU, **T256x32)
case('x3_256x64_s1_res', 'x3', _x3(256, 64, 4, 2, s1=1), cin=128, s1=dict(cin=128, stride=2), res=1, **T256x64)
case('x3_64x128_sigmoid_osplit', 'x3', _x3(64, 128, 1, 4), cin=64, act=ACT_SIGMOID, osplit='half', **T64x128)
case('x3_128x128_pre_tanh', 'x3', _x3(128, 128, 2, 4, pre=1), cin=64, pre=1, act=ACT_TANH, **T128x128)
case('x3_256x128_deep_kcb', 'x3', _x3(256, 128, 4, 2), kcb=1, act=ACT_NONE, flag=1, **T256x128)
case('x3_generic_cin8', 'x3', _x3(64, 32, 2, 1, buf=0), nimg=2, H=9, W=33, cin=8, N=32, k=(3, 3), cin_real=6)
case('x3_generic_cin8_add', 'x3', _x3(64, 32, 2, 1, add=1, buf=0), nimg=2, H=9, W=33, cin=8, N=32, k=(3, 3), add=1)
case('x3_generic_31tap', 'x3', _x3(256, 64, 4, 2, buf=0), nimg=2, H=1, W=100, cin=32, N=64, k=(1, 31), act=ACT_RELU)
case('x3_reflect_dil2', 'x3', _x3(64, 128, 1, 4), nimg=3, H=1, W=50, cin=64, N=128, k=(1, 3), d=(1, 2), reflect=1,
     act=ACT_RELU, post=1)
case('x3_reflect_dil3_fullpad', 'x3', _x3(64, 128, 1, 4), nimg=40, H=1, W=4, cin=64, N=128, k=(1, 3), d=(1, 3),
     reflect=1, act=ACT_RELU)   # pw = 3 = W - 1
case('x3_vlen_rowlen', 'x3', _x3(256, 64, 4, 2), nimg=3, H=1, W=60, cin=64, N=64, k=(1, 5), vlen=[60, 1, 37],
     rowlen=[60, 1, 37], act=ACT_RELU)
case('x3_vlen_rowlen_pre', 'x3', _x3(256, 64, 4, 2, pre=1), nimg=3, H=1, W=60, cin=64, N=64, k=(1, 5), pre=1,
     vlen=[1, 60, 23], rowlen=[1, 60, 23], act=ACT_NONE)
case('x3_range_masked', 'x3', _x3(256, 64, 4, 2), nimg=3, H=1, W=60, cin=64, N=64, rowlen=[60, 1, 37], flag=1,
     huge_masked=1, act=ACT_RELU)
case('x3_kcb_small', 'x3', _x3(64, 128, 1, 4), nimg=2, H=9, W=33, cin=96, N=128, k=(3, 3), kcb=1)
case('x3_ksplit2', 'x3', _x3(64, 128, 1, 4), nimg=6, H=1, W=1, cin=1024, N=192, ksplit=2, act=ACT_NONE, flag=1)
case('x3_ksplit3', 'x3', _x3(64, 128, 1, 4), nimg=7, H=1, W=3, cin=1024, N=192, ksplit=3, act=ACT_RELU, res=1)
case('x3_rowbias_post_tanh', 'x3', _x3(64, 128, 1, 4), nimg=3, H=1, W=50, cin=128, N=128, rowbias=1, act=ACT_RELU,
     post=1, act2=ACT_TANH)
case('x3_aff', 'x3', _x3(64, 128, 1, 4), nimg=2, H=9, W=33, cin=64, N=104, aff=1)
case('x3_range_up', 'x3', _x3(128, 128, 2, 4), cin=64, flag=1, big_out=1, act=ACT_NONE, **T128x128)
case('x3_scaled', 'x3', _x3(128, 128, 2, 4), cin=64, range_in=1, flag=1, act=ACT_RELU, **T128x128)
case('x3_wbig_exact', 'f32', _f32(256, 64, 16, 4, 2), cin=64, wbig=1, **T256x64)

case('x1_128x128', 'x1', _x1(128, 128, 2, 4), cin=64, x1=1, **T128x128)
case('x1_64x32_add', 'x1', _x1(64, 32, 2, 1, add=1), cin=64, x1=1, add=1, act=ACT_RELU, **T64x32)
case('x1_256x64_s1', 'x1', _x1(256, 64, 4, 2, s1=1), cin=128, x1=1, s1=dict(cin=128, stride=1), **T256x64)
case('x1_64x128_pre', 'x1', _x1(64, 128, 1, 4, pre=1), cin=64, x1=1, pre=1, act=ACT_RELU, **T64x128)
case('x1_scaled', 'x1', _x1(128, 128, 2, 4), cin=64, x1=1, range_in=1, flag=1, act=ACT_RELU, **T128x128)

# exact fp32 (no planes): each tile select_cfg() gives without planes, at BK 16 (Kp < 256) and
# BK 32, the S1 / ADD / PRE forms spread over them
case('f32_64x32_bk16_add', 'f32', _f32(64, 32, 16, 2, 1, add=1), cin=64, planes=0, add=1, **T64x32)
case('f32_64x32_bk32_pre', 'f32', _f32(64, 32, 32, 2, 1, pre=1), cin=128, planes=0, pre=1, act=ACT_RELU, **T64x32)
case('f32_256x32_bk16', 'f32', _f32(256, 32, 16, 8, 1), cin=64, planes=0, act=ACT_RELU, **T256x32)
case('f32_256x32_bk32_pre', 'f32', _f32(256, 32, 32, 8, 1, pre=1), cin=128, planes=0, pre=1, gate=100, **T256x32)
case('f32_256x64_bk16_s1', 'f32', _f32(256, 64, 16, 4, 2, s1=1), cin=64, planes=0, s1=dict(cin=64, stride=2),
     **T256x64)
case('f32_256x64_bk32_add', 'f32', _f32(256, 64, 32, 4, 2, add=1), cin=256, planes=0, add=1, flag=1, **T256x64)
case('f32_64x128_bk16_pre', 'f32', _f32(64, 128, 16, 1, 4, pre=1), cin=64, planes=0, pre=1, act=ACT_SILU, **T64x128)
case('f32_64x128_bk32_s1', 'f32', _f32(64, 128, 32, 1, 4, s1=1), cin=208, planes=0, s1=dict(cin=128, stride=1),
     res=1, **T64x128)
case('f32_128x128_shortk_add', 'f32', _f32(128, 128, 32, 2, 4, add=1), cin=104, planes=0, add=1, flag=1, big_out=1,
     act=ACT_NONE, **T128x128)
case('f32_128x128_bk32_s1', 'f32', _f32(128, 128, 32, 2, 4, s1=1), cin=208, planes=0, s1=dict(cin=128, stride=2),
     osplit='half', **T128x128)
case('f32_128x128_bk32_3x3_kcb', 'f32', _f32(128, 128, 32, 2, 4), cin=96, k=(3, 3), planes=0, kcb=1, rowlen='auto',
     **T128x128)

case('f32_range_masked', 'f32', _f32(256, 64, 16, 4, 2), nimg=3, H=1, W=60, cin=64, N=64, planes=0,
     rowlen=[60, 1, 37], flag=1, huge_masked=1, act=ACT_RELU)
case('f32_big_in', 'f32', _f32(128, 128, 32, 2, 4), cin=64, planes=0, flag=1, big_in=1, act=ACT_RELU, **T128x128)
# every (tile, BK, loader form) cell: 1x1 shapes, K = 128 (BK 16) or 256 (BK 32); the 128x128
# tile has BK 32 only (select_cfg)
for (bm, bn, wm, wn), geo in [((64, 32, 2, 1), T64x32), ((256, 32, 8, 1), T256x32), ((256, 64, 4, 2), T256x64),
                              ((64, 128, 1, 4), T64x128), ((128, 128, 2, 4), T128x128)]:
    for bk in ((32,) if bm == bn else (16, 32)):
        kk = 128 if bk == 16 and bm != bn else 256
        geo1 = dict(geo, k=(1, 1))
        case(f'f32_{bm}x{bn}_bk{bk}_grid_s1', 'f32', _f32(bm, bn, bk, wm, wn, s1=1), cin=kk // 2, planes=0,
             s1=dict(cin=kk // 2, stride=1), **geo1)
        case(f'f32_{bm}x{bn}_bk{bk}_grid_add', 'f32', _f32(bm, bn, bk, wm, wn, add=1), cin=kk, planes=0, add=1, **geo1)
        case(f'f32_{bm}x{bn}_bk{bk}_grid_pre', 'f32', _f32(bm, bn, bk, wm, wn, pre=1), cin=kk, planes=0, pre=1,
             act=ACT_RELU, **geo1)

# the remaining tile x loader-form instantiations that the models' launch plans name
# (test_gpu_conv_kernels.py: the coverage test lists what the table lacks)
T_DEEP_S1 = dict(nimg=1, H=17, W=241, cin=2048, N=512, s1=dict(cin=2048, stride=1))   # K = 4096: the 256x128 tile
case('x3_128x128_add', 'x3', _x3(128, 128, 2, 4, add=1), cin=64, add=1, **T128x128)
case('x3_128x128_generic_31tap', 'x3', _x3(128, 128, 2, 4, buf=0), nimg=17, H=1, W=241, cin=32, N=104, k=(1, 31))
case('x3_256x32_generic_cin16', 'x3', _x3(256, 32, 8, 1, buf=0), nimg=10, H=100, W=131, cin=16, N=32, k=(3, 3))
case('x3_256x32_generic_cin16_add', 'x3', _x3(256, 32, 8, 1, add=1, buf=0), nimg=10, H=100, W=131, cin=16, N=32,
     k=(3, 3), add=1, cin_real=14)
case('x3_256x64_add', 'x3', _x3(256, 64, 4, 2, add=1), cin=64, add=1, **T256x64)
case('x3_64x128_generic_31tap', 'x3', _x3(64, 128, 1, 4, buf=0), nimg=2, H=1, W=100, cin=32, N=104, k=(1, 31))
case('x3_64x128_pre', 'x3', _x3(64, 128, 1, 4, pre=1), cin=64, pre=1, act=ACT_RELU, **T64x128)
case('x3_64x128_add', 'x3', _x3(64, 128, 1, 4, add=1), cin=64, add=1, **T64x128)
case('x3_64x128_s1', 'x3', _x3(64, 128, 1, 4, s1=1), cin=64, s1=dict(cin=32, stride=2), **T64x128)
case('pw_k64_s1', 'pw', _pw(64, 64, 1, 0), cin=32, N=52, s1=dict(cin=32, stride=1), **PW_GEO)
case('x1_128x128_pre', 'x1', _x1(128, 128, 2, 4, pre=1), cin=64, x1=1, pre=1, act=ACT_RELU, **T128x128)
case('x1_128x128_add', 'x1', _x1(128, 128, 2, 4, add=1), cin=64, x1=1, add=1, **T128x128)
case('x1_128x128_s1', 'x1', _x1(128, 128, 2, 4, s1=1), cin=64, x1=1, s1=dict(cin=64, stride=2), **T128x128)
case('x1_256x128_deep', 'x1', _x1(256, 128, 4, 2), x1=1, act=ACT_NONE, **T256x128)
case('x1_256x128_deep_s1', 'x1', _x1(256, 128, 4, 2, s1=1), x1=1, act=ACT_SILU, **T_DEEP_S1)
case('x1_256x64', 'x1', _x1(256, 64, 4, 2), cin=64, x1=1, **T256x64)
case('x1_256x64_add', 'x1', _x1(256, 64, 4, 2, add=1), cin=64, x1=1, add=1, **T256x64)
case('x1_64x128', 'x1', _x1(64, 128, 1, 4), cin=64, x1=1, **T64x128)
case('x1_64x128_add', 'x1', _x1(64, 128, 1, 4, add=1), cin=64, x1=1, add=1, **T64x128)
case('x1_64x128_s1', 'x1', _x1(64, 128, 1, 4, s1=1), cin=64, x1=1, s1=dict(cin=64, stride=1), **T64x128)
case('x1_64x32', 'x1', _x1(64, 32, 2, 1), cin=64, x1=1, **T64x32)

BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def f256_geometry(cus):
    """W of the f_256x256 case (nimg 2, H 100, N 208, K 512): the smallest W >= 200 whose M the
    rule of f_tile() (conv_gemm_f.hip) sends to the 256x256 tile on a device of `cus` CUs, with
    a ragged last row tile.  256 CUs: W = 200, M = 40000, 157 blocks, a 0.61 last round."""
    for w in range(200, 4000):
        m = 2 * 100 * w
        rounds = ((m + 255) // 256) * 1 / cus
        tail = rounds - int(rounds)
        if m >= 16384 and m % 256 and (rounds >= 4.0 or tail == 0.0 or tail >= 0.6):
            return w
    raise AssertionError(cus)


# ---------------------------------------------------------------------------- building a case
def _geometry(c, cus):
    kh, kw = c['k']
    dh, dw = c['d']
    ph, pw = c['p'] if c['p'] is not None else (dh * (kh // 2), dw * (kw // 2))
    W = f256_geometry(cus) if c['W'] == 'f256' else c['W']
    s0 = dict(H=c['H'], W=W, cin=c['cin'], kh=kh, kw=kw, sh=c['s'][0], sw=c['s'][1], ph=ph, pw=pw, dh=dh, dw=dw,
              reflect=c['reflect'])
    Ho, Wo = conv_ref.out_geometry(s0, c['H'], W)
    g = dict(nimg=c['nimg'], Ho=Ho, Wo=Wo, N=c['N'], act=c['act'], act2=c['act2'], s0=s0)
    if c['s1']:
        st = c['s1']['stride']
        g['s1'] = dict(H=Ho * st, W=Wo * st, cin=c['s1']['cin'], sh=st, sw=st)
    if c['gate']:
        g['gate_seg'] = c['gate']
    return g


def build(c, cus=256):
    """(geometry, host tensors) of a case; deterministic per case name."""
    g = _geometry(c, cus)
    gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c['name'])))
    s0 = g['s0']
    nimg, H, W, cin, N = g['nimg'], s0['H'], s0['W'], s0['cin'], g['N']
    Ho, Wo = g['Ho'], g['Wo']
    M = nimg * Ho * Wo
    taps = s0['kh'] * s0['kw']
    creal = c['cin_real'] or cin

    def ua(*shape):
        return torch.rand(*shape, generator=gen) * 2.0 + 1e-6

    def uw(*shape):
        v = torch.rand(*shape, generator=gen) * 2.0 - 1.0
        return torch.where(v == 0, torch.full_like(v, 0.5), v)

    t = {}
    in_scale = 5e4 if c['range_in'] or c['big_in'] else 1.0   # inputs near 1e5 (scaled split, or no split)

    def operand(ld):
        x = ua(nimg, H, W, ld) * in_scale
        x[..., creal:cin] = 1e3          # padded channels meet zero weights
        return x

    t['x'] = operand(cin + 4)
    if c['add']:
        t['x2'] = operand(cin + 8)
    if c['vlen'] is not None:
        t['vlen'] = torch.tensor(c['vlen'], dtype=torch.int32)
        past = torch.arange(W)[None, :] >= t['vlen'][:, None].long()            # [nimg, W]
        junk = 1e4 * torch.randn(nimg, H, W, t['x'].shape[-1], generator=gen)
        t['x'] = torch.where(past[:, None, :, None], junk, t['x'])
    if c['s1']:
        s1 = g['s1']
        t['xs1'] = ua(nimg, s1['H'], s1['W'], s1['cin'] + 12) * in_scale
    K = taps * cin + (g['s1']['cin'] if c['s1'] else 0)
    wscale = 1.0 / math.sqrt(K)
    t['w0'] = uw(N, taps, cin) * wscale
    t['w0'][:, :, creal:] = 0.0
    if c['s1']:
        t['w1'] = uw(N, g['s1']['cin']) * wscale
    if c['pre']:
        t['pre_scale'] = 0.5 + 0.5 * ua(cin)
        t['pre_shift'] = uw(cin)
    if c['bias']:
        t['bias'] = uw(N) * 0.1
        if c['big_out']:
            t['bias'][::3] *= 3e5      # outputs pass 2^14 with operands that stay in range
    if c['rowbias']:
        t['rowbias'] = uw(nimg, N + 4)
    if c['res']:
        t['res'] = ua(M, N + 8)
    if c['aff']:
        t['affx'] = ua(M, N + 4)
        t['affy'] = ua(M, N + 12)
    if c['post']:
        t['post_scale'] = (0.5 + 0.5 * ua(N)) * torch.where(torch.arange(N) % 5 == 0, -1.0, 1.0)
        t['post_shift'] = uw(N) * 0.5
    if c['gate']:
        nseg = (Wo + c['gate'] - 1) // c['gate']
        t['gate'] = 0.05 + 0.45 * ua(nimg, nseg, N + 4)
    if c['rowlen'] is not None:
        rl = [max(1, Wo - 3 * (i + 1)) for i in range(nimg)] if c['rowlen'] == 'auto' else c['rowlen']
        t['rowlen'] = torch.tensor(rl, dtype=torch.int32)
        if c['huge_masked']:
            # columns two past the valid length (a 3x3 window of a valid output does not reach
            # them) hold values near fp16's largest: only masked outputs see them, and their
            # pre-mask values are far past 2^14
            far = torch.arange(W)[None, :] >= t['rowlen'][:, None].long() + 2
            t['x'] = torch.where(far[:, None, :, None], t['x'] * 3e4, t['x'])
    return g, t


def pack_weights(c, g, t):
    """[N][Kp] fp32 in the packed K order (the test's own statement of ConvDesc::kcb)."""
    N = g['N']
    cin = g['s0']['cin']
    taps = g['s0']['kh'] * g['s0']['kw']
    w0 = t['w0']
    if c['kcb']:   # k = ((c / 32) * taps + tap) * 32 + c % 32
        w0 = w0.reshape(N, taps, cin // 32, 32).permute(0, 2, 1, 3)
    cols = [w0.reshape(N, -1)]
    if t.get('w1') is not None:
        cols.append(t['w1'])
    w = torch.cat(cols, dim=1)
    K = w.shape[1]
    Kp = round_up(K, 32)
    out = torch.zeros(N, Kp)
    out[:, :K] = w
    return out, K, Kp


_small_refs = {}


def reference(c, g, t):
    """conv_ref.reference, computed once per case and shared by both legs (small cases are
    kept: the large ones would hold gigabytes)."""
    key = (c['name'], g['s0']['W'])
    if key in _small_refs:
        return _small_refs[key]
    r = conv_ref.reference(g, t)
    if r['out'].numel() <= 1 << 20:
        _small_refs[key] = r
    return r


class LaunchError(RuntimeError):
    """spk_diag_conv returned an error for a case the table means to run."""


class Backend:
    """Where a case runs: the library handle, the torch device its buffers live on, the
    accumulation tolerance per case and whether the kernel name is asserted."""

    def __init__(self, handle, device, emu, cus=256):
        self.handle, self.device, self.emu, self.cus = handle, device, emu, cus

    def sync(self):
        if not self.emu:
            torch.cuda.synchronize()

    def c_for(self, c):
        if self.emu:
            return C_EMU
        return C_X1 if c['x1'] else C_X3


def descriptor(c, g, t, be, keep):
    """The spk_diag_conv_t fields of a case as a dict, its buffers on the backend's device.
    `keep` collects what must stay alive; returns (desc, out buffer, out index, words)."""
    dev = be.device
    s0, N = g['s0'], g['N']
    M = g['nimg'] * g['Ho'] * g['Wo']

    def up(v, dtype=None):
        if v is None:
            return None
        v = v.contiguous().to(dev)
        keep.append(v)
        return v

    w, K, Kp = pack_weights(c, g, t)
    # 'half': two planes, the second one narrower where N / 2 is no multiple of 4
    osplit = round_up(N // 2, 4) if c['osplit'] == 'half' else 0
    ldo = (osplit or N) + 4
    nplanes = 2 if osplit else 1
    oplane = (M + GUARD_ROWS) * ldo
    out = torch.full((nplanes * oplane,), SENTINEL, dtype=torch.int32, device=dev)
    d = dict(nimg=g['nimg'], Ho=g['Ho'], Wo=g['Wo'], N=N, K=K, Kp=Kp, planes=c['planes'], act=c['act'],
             act2=c['act2'], ldo=ldo, osplit=osplit, oplane=oplane if osplit else 0, ksplit=c['ksplit'], x1=c['x1'],
             wbig=c['wbig'], kcb=c['kcb'])
    d['out'] = out
    d['w'] = up(w)
    if c['planes'] >= 1:
        d['wh'] = torch.zeros(N * Kp, dtype=torch.int16, device=dev)
        d['wl'] = torch.zeros(N * Kp, dtype=torch.int16, device=dev)
    if c['planes'] == 2:
        d['wf'] = torch.zeros(conv_diag.frag_halves(be.handle, N, Kp), dtype=torch.int16, device=dev)
    src0 = dict(s0)
    src0['p'] = up(t['x'])
    src0['ld'] = t['x'].shape[-1]
    if t.get('x2') is not None:
        src0['p2'] = up(t['x2'])
        src0['ld2'] = t['x2'].shape[-1]
    if t.get('pre_scale') is not None:
        src0['pre_scale'] = up(t['pre_scale'])
        src0['pre_shift'] = up(t['pre_shift'])
    if t.get('vlen') is not None:
        src0['vlen'] = up(t['vlen'])
    d['s0'] = src0
    if t.get('xs1') is not None:
        d['s1'] = dict(g['s1'], p=up(t['xs1']), ld=t['xs1'].shape[-1])
    if t.get('bias') is not None:
        d['bias'] = up(t['bias'])
    if t.get('rowbias') is not None:
        d['rowbias'], d['rowbias_ld'] = up(t['rowbias']), t['rowbias'].shape[-1]
    if t.get('res') is not None:
        d['res'], d['ldr'] = up(t['res']), t['res'].shape[-1]
    if t.get('affx') is not None:
        d['affx'], d['ldx'] = up(t['affx']), t['affx'].shape[-1]
        d['affy'], d['ldy'] = up(t['affy']), t['affy'].shape[-1]
    if t.get('post_scale') is not None:
        d['post_scale'], d['post_shift'] = up(t['post_scale']), up(t['post_shift'])
    if t.get('gate') is not None:
        d['gate'], d['gate_ld'] = up(t['gate']), t['gate'].shape[-1]
        d['gate_seg'], d['gate_nseg'] = g['gate_seg'], t['gate'].shape[1]
    if t.get('rowlen') is not None:
        d['rowlen'] = up(t['rowlen'])
    if c['ksplit'] > 1:
        d['partial'] = torch.zeros(c['ksplit'] * M * N, dtype=torch.float32, device=dev)
    words = {}
    if c['flag']:
        words['flag'] = d['range_flag'] = torch.zeros(4, dtype=torch.int32, device=dev)
    if c['range_in']:
        amax = max(float(v.abs().max()) for k, v in t.items() if k in ('x', 'x2', 'xs1'))
        words['in'] = d['range_in'] = torch.tensor([amax, 0, 0, 0], dtype=torch.float32).view(torch.int32).to(dev)
    keep.extend(v for v in d.values() if isinstance(v, torch.Tensor))
    return d, out, conv_ref.out_index(M, N, ldo, osplit, oplane), words


def run_case(c, be):
    """Launch one case on a backend and check everything the table promises.  Returns a
    report dict (kernel name, worst normalised error, ...) for the caller to print."""
    g, t = build(c, be.cus)
    ref = reference(c, g, t)
    keep = []
    d, out, oidx, words = descriptor(c, g, t, be, keep)
    rc, kernel, err = conv_diag.launch(be.handle, d)
    be.sync()
    if rc != 0:   # a launch error, not a mismatch: callers stop launching (LaunchError is no AssertionError)
        raise LaunchError(f"{c['name']}: spk_diag_conv failed ({rc}): {err} [{kernel}]")
    if not be.emu:
        assert re.fullmatch(c['expect'], kernel), f"{c['name']}: reached {kernel!r}, meant {c['expect']!r}"
    raw = out.cpu()
    got32 = raw.view(torch.float32)[oidx]
    # writes stay in bounds: everything outside the (m, n) elements still holds the sentinel
    touched = torch.zeros(raw.numel(), dtype=torch.bool)
    touched[oidx.reshape(-1)] = True
    stray = (~touched) & (raw != SENTINEL)
    assert not bool(stray.any()), f"{c['name']} [{kernel}]: {int(stray.sum())} writes outside the output, " \
                                  f"first at float offset {int(stray.nonzero()[0])}"
    unwritten = raw[oidx] == SENTINEL
    assert not bool(unwritten.any()), f"{c['name']} [{kernel}]: {int(unwritten.sum())} outputs not written"
    got = got32.to(torch.float64)
    # masked rows are exactly zero
    if bool(ref['masked'].any()):
        assert bool((got32[ref['masked']] == 0).all()), f"{c['name']} [{kernel}]: a masked row is not 0"
    cc = be.c_for(c)
    e = (got - ref['out']).abs()
    scale = ref['mag'] * ref['L']
    bound = cc * scale + EPS_EPI * ref['out'].abs()
    trans = c['aff'] or c['act'] in conv_ref.TRANSCENDENTAL or c['act2'] in conv_ref.TRANSCENDENTAL
    excess = ((e - bound).clamp(min=0) / ref['out'].abs().clamp(min=1e-30)).max().item() if trans else 0.0
    if trans and not be.emu:
        bound = bound + TRANS_T * ref['out'].abs()
    live = ~ref['masked']
    worst = (e[live] / scale[live].clamp(min=1e-30)).max().item() if bool(live.any()) else 0.0
    report = dict(case=c['name'], fam=c['fam'], kernel=kernel, worst=worst, c=cc, trans_excess=excess,
                  M=got.shape[0], N=got.shape[1])
    print(f"{c['name']}: {kernel}  M={got.shape[0]} N={got.shape[1]}  worst err/(mag*L) {worst:.3e} (c = {cc:g})"
          + (f"  transcendental excess/|ref| {excess:.3e}" if trans else ''))
    bad = ~(e <= bound)   # NaN counts as bad
    if bool(bad.any()):
        m, n = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(
            f"{c['name']} [{kernel}]: {int(bad.sum())} of {bad.numel()} outputs outside the bound; first (m={m}, n={n}) "
            f"got {got[m, n].item():.9g} ref {ref['out'][m, n].item():.9g} err {e[m, n].item():.3e} "
            f"bound {bound[m, n].item():.3e}; worst err/(mag*L) {worst:.3e}")
    # range word: 0 below 2^14, else the bits of the largest |output| the kernel wrote
    if 'flag' in words:
        word = int(words['flag'].cpu()[0])
        amax = got32.abs().max()
        want = int(amax.view(torch.int32)) if float(amax) >= 16384.0 else 0
        report['word'] = word
        assert word == want, f"{c['name']} [{kernel}]: range word {word:#x}, want {want:#x} (max |out| {float(amax)})"
        if c['big_out'] or c['big_in'] or c['range_in']:
            assert word != 0, c['name']
        if c['huge_masked']:
            assert word == 0, c['name']
    return report


# ---------------------------------------------------------------------------- rejected descriptors
def _set(path, value):
    def f(d):
        tgt = d
        for k in path[:-1]:
            tgt = tgt[k]
        tgt[path[-1]] = value
    return f


def _misalign(path):
    def f(d):
        tgt = d
        for k in path[:-1]:
            tgt = tgt[k]
        tgt[path[-1]] = tgt[path[-1]].data_ptr() + 4
    return f


def _also_pre(d):
    d['s0']['pre_scale'] = d['bias']
    d['s0']['pre_shift'] = d['bias']


def _drop_partial(d):
    d['ksplit'] = 2
    d.pop('partial', None)


# every clause of launch_conv's host check (conv_gemm.hip), and two of s1 / addend / pre at
# once: (name, case the descriptor starts from, what breaks it)
REJECTS = [
    ('s0_cin_mod4', 'x3_256x64_s1_res', _set(('s0', 'cin'), 126)),
    ('s0_ld_mod4', 'x3_256x64_s1_res', _set(('s0', 'ld'), 130)),
    ('s0_ld2_mod4', 'x3_64x32_add_silu', _set(('s0', 'ld2'), 70)),
    ('kp_align', 'x3_256x64_s1_res', _set(('Kp',), 272)),
    ('osplit_mod4', 'x3_64x128_sigmoid_osplit', _set(('osplit',), 54)),
    ('ldo_below_osplit', 'x3_64x128_sigmoid_osplit', _set(('ldo',), 48)),
    ('ldo_below_n', 'x3_256x64_s1_res', _set(('ldo',), 60)),
    ('s1_cin_mod4', 'x3_256x64_s1_res', _set(('s1', 'cin'), 126)),
    ('s1_ld_mod4', 'x3_256x64_s1_res', _set(('s1', 'ld'), 138)),
    ('n_zero', 'x3_256x64_s1_res', _set(('N',), 0)),
    ('nimg_zero', 'x3_256x64_s1_res', _set(('nimg',), 0)),
    ('ho_zero', 'x3_256x64_s1_res', _set(('Ho',), 0)),
    ('wo_negative', 'x3_256x64_s1_res', _set(('Wo',), -1)),
    ('s0_p_misaligned', 'x3_256x64_s1_res', _misalign(('s0', 'p'))),
    ('w_misaligned', 'x3_256x64_s1_res', _misalign(('w',))),
    ('k_above_kp', 'x3_256x64_s1_res', _set(('K',), 257)),
    ('ksplit_without_partial', 'x3_256x64_s1_res', _drop_partial),
    ('s1_and_pre', 'x3_256x64_s1_res', _also_pre),
    ('add_and_pre', 'x3_64x32_add_silu', _also_pre),
    ('s1_and_add', 'x3_256x64_s1_res', lambda d: d['s0'].update(p2=d['s0']['p'], ld2=d['s0']['ld'])),
    # the same from descriptors that the halo, pointwise and LDS-DMA routes would otherwise take:
    # each route's predicate excludes one of the pair, so launch_tile sees and refuses them
    ('halo_add_and_pre', 'halo_x3_32to32_add', _also_pre),
    ('pw_s1_and_add', 'pw_s1', lambda d: d['s0'].update(p2=d['s0']['p'], ld2=d['s0']['ld'])),
    ('f_s1_and_add', 'f_s1_stride2', lambda d: d['s0'].update(p2=d['s0']['p'], ld2=d['s0']['ld'])),
]


def run_reject(name, be):
    """A descriptor the host check must refuse: an error comes back, nothing is written."""
    _, base, breakit = next(r for r in REJECTS if r[0] == name)
    c = BY_NAME[base]
    g, t = build(c, be.cus)
    keep = []
    d, out, _, _ = descriptor(c, g, t, be, keep)
    breakit(d)
    rc, kernel, err = conv_diag.launch(be.handle, d)
    be.sync()
    assert rc != 0, f'{name}: accepted [{kernel}]'
    assert err, name
    assert bool((out.cpu() == SENTINEL).all()), f'{name}: the refused launch wrote to the output'
    print(f'{name}: refused ({rc}): {err}')
