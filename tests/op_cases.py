"""TEST INFRASTRUCTURE: the table of direct cases of the kernel entries that are not convs (one
launch each through csrc/diag_ops.cpp) and the code that builds a case's tensors, launches it
and checks it against tests/op_ref.py.  Consumed twice: test_op_contract_emu.py (host
emulation, no GPU) and test_gpu_op_kernels.py (the real kernels).

Every case asserts the kernel name (where the entry reports one), every output element,
that nothing outside the output was written (row padding ld > C, GUARD elements after the
last row, scratch), exact zeros in masked rows and the range word (where the op has one; it
starts at 5 so that "untouched" is visible).  Every operand has a leading dimension larger
than its width; the padding holds 1e3.

Bounds (u = 2^-24), elementwise:
  * exact ops, masks, canaries, refused descriptors: equality;
  * fp32 sums and FMAs (time_mean, stem, se_apply, cam_context, the gate's dot products):
    (n + 4) u mag, n the number of terms reduced, mag = sum |terms| from the reference;
  * the running mean of a one-pass Welford reduction (asp_stats, stats_pool, tstp) is no plain
    sum: step k rounds a subtraction, a division and an addition of values of at most 2 amax,
    amax = max_t |x|: (3 n + 4) u amax;
  * fp16x3 stages (AFF, Res2 block): conv_cases.C_X3 per stage, carried through the later
    stages (op_ref.aff / res2_block);
  * one-pass standard deviations and both outputs of the online-softmax pools (attn_pool,
    astp_pool): 4 x the case-wide worst error / mag of the model source's own fp32 PyTorch
    formula (op_ref with dt = float32, on the CPU) against float64, plus one fp32 ulp of the
    output.  MEASURED holds the ratios seen (formula and kernel);
  * transcendental intrinsics (__expf, the hardware reciprocal, tanh): no allowance
    (TRANS_T = 0), as in conv_cases.

Not reached: the grid-stride paths of the lane-per-channel reductions and of se_apply need
more than 65536 * 256 = 16.7 M elements per launch."""
import math

import numpy as np
import torch

import op_diag
import op_ref
from conv_cases import C_EMU, C_X3, SENTINEL, Backend, LaunchError, round_up   # noqa: F401  (Backend re-exported)
from op_ref import F32, F64

U = 2.0 ** -24
TRANS_T = 0.0
GUARD = 64            # sentinel elements after every buffer's last row
FLAG0 = 5             # the range word's start value: below the bits of any float >= 2^14
PAD = 1e3             # what operand padding (columns >= C) holds
STD_FACTOR = 4.0
# Measured on an MI355X, per family: (worst err / mag of the fp32 PyTorch formula against
# float64 over the family's cases, worst kernel err / bound over all its cases).
MEASURED = {'asp_stats': (1.45e-7, 0.40), 'stats_pool': (6.3e-8, 0.82), 'tstp': (1.1e-7, 0.64),
            'attn_pool': (6.4e-7, 0.33), 'astp_pool': (7.9e-4, 0.27)}

CASES = []


def case(name, fam, **kw):
    assert all(c['name'] != name for c in CASES), name
    CASES.append(dict(name=name, fam=fam, **kw))


def _gen(name):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))


# ---------------------------------------------------------------------------- buffers and checks
class Ctx:
    """one case on one backend: uploads, sentinel-filled outputs, the comparator"""

    def __init__(self, c, be):
        self.c, self.be, self.keep, self.kernel = c, be, [], ''
        self.gen = _gen(c['name'])
        self.worst = 0.0

    def up(self, t):
        if t is None:
            return None
        t = t.contiguous().to(self.be.device)
        self.keep.append(t)
        return t

    def rows(self, t, ld):
        """[..., C] -> uploaded [..., ld] with PAD in the padding columns"""
        full = torch.full(t.shape[:-1] + (ld,), PAD, dtype=t.dtype)
        full[..., :t.shape[-1]] = t
        return self.up(full)

    def out(self, n):
        o = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=self.be.device)
        self.keep.append(o)
        return o

    def flag(self):
        return self.up(torch.tensor([FLAG0, 0, 0, 0], dtype=torch.int32))

    def launch(self, op, fields, want_kernel=None):
        rc, kernel, err = op_diag.launch(self.be.handle, op, fields)
        self.be.sync()
        self.kernel = kernel
        if rc != 0:
            raise LaunchError(f"{self.c['name']}: spk_diag_{op} failed ({rc}): {err} [{kernel}]")
        if want_kernel is not None:
            if self.be.emu:
                assert kernel.startswith('emu_'), kernel
            else:
                assert kernel == want_kernel, f"{self.c['name']}: reached {kernel!r}, meant {want_kernel!r}"
        return kernel

    def untouched(self, raw, what):
        raw = raw.cpu()
        assert bool((raw == SENTINEL).all()), f"{self.c['name']}: {what} was written"

    def check(self, raw, idx, ref, bound, what='out', exact=False, zero=None, part=False):
        """raw: the sentinel-filled int32 buffer; idx: flat positions of the outputs, shaped as
        ref; bound: elementwise; exact: equality (NaN where ref is NaN in either mode); zero: a
        bool mask of outputs that must be exactly 0; part: idx is a part of an output checked
        already (no canary check)"""
        name, kernel = self.c['name'], self.kernel
        raw = raw.cpu()
        touched = torch.zeros(raw.numel(), dtype=torch.bool)
        touched[idx.reshape(-1)] = True
        stray = (~touched) & (raw != SENTINEL)
        assert part or not bool(stray.any()), f"{name} [{kernel}]: {int(stray.sum())} writes outside {what}, first at " \
                                      f"element {int(stray.nonzero()[0])}"
        assert not bool((raw[idx] == SENTINEL).any()), f"{name} [{kernel}]: {what} has unwritten elements"
        got32 = raw.view(torch.float32)[idx]
        got = got32.to(F64)
        ref = ref.to(F64)
        if zero is not None and bool(zero.any()):
            assert bool((got32[zero] == 0).all()), f"{name} [{kernel}]: a masked output of {what} is not 0"
        nan = torch.isnan(ref)
        assert bool(torch.isnan(got[nan]).all()), f"{name} [{kernel}]: {what} must be NaN where the model source is"
        e = (got - ref).abs()
        if exact:
            bad = ~nan & (got32 != ref.to(F32))
        else:
            bound = bound.to(F64).expand_as(ref)
            bad = ~nan & ~(e <= bound)
            live = ~nan & (bound > 0)
            if bool(live.any()):
                self.worst = max(self.worst, float((e[live] / bound[live]).max()))
        if bool(bad.any()):
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(
                f"{name} [{kernel}]: {int(bad.sum())} of {bad.numel()} elements of {what} outside the bound; first {i} "
                f"got {got[i].item():.9g} ref {ref[i].item():.9g} err {e[i].item():.3e} "
                f"bound {0.0 if exact else bound[i].item():.3e}")

    def check_word(self, flag, got_raw, idx):
        """range word: max(start, bits of the largest |output| written) once that reaches 2^14"""
        word = int(flag.cpu()[0])
        amax = got_raw.cpu().view(torch.float32)[idx].abs().max()
        want = max(FLAG0, int(amax.view(torch.int32))) if float(amax) >= 16384.0 else FLAG0
        assert word == want, f"{self.c['name']} [{self.kernel}]: range word {word:#x}, want {want:#x} (max {float(amax)})"
        return word

    def report(self, **kw):
        r = dict(case=self.c['name'], fam=self.c['fam'], kernel=self.kernel, worst=self.worst, **kw)
        print(f"{self.c['name']}: {self.kernel or self.c['fam']}  worst err/bound {self.worst:.3e}"
              + ''.join(f'  {k} {v:.3e}' for k, v in kw.items() if isinstance(v, float)))
        return r


def _ulp32(v):
    a = v.abs().to(F32)
    return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).to(F64)


def _idx2(rows, width, ld):
    return torch.arange(rows)[:, None] * ld + torch.arange(width)[None, :]


def measured_bound(ref64, ref32):
    """the bound of the one-pass statistics: (4 x worst |fp32 formula - float64| / mag) mag + 1 ulp.
    Returns (bound, ratio)."""
    ok = ~torch.isnan(ref64['out']) & (ref64['mag'] > 0)
    ratio = float(((ref32['out'].to(F64) - ref64['out']).abs()[ok] / ref64['mag'][ok]).max()) if bool(ok.any()) else 0.0
    return STD_FACTOR * ratio * ref64['mag'] + _ulp32(ref64['out']), ratio


# ---------------------------------------------------------------------------- time reductions
TC = [(1, 3), (2, 1), (15, 65), (16, 257), (17, 3), (31, 65), (33, 257), (100, 65)]
VMODES = ['none', 'allT', 'all1', 'mixed', 'outside']
LOGITS = ['rand', 'rising', 'falling', 'equal', 'span80', 'spike60']


def _vlen(mode, B, T):
    if mode == 'none':
        return None
    if mode == 'allT':
        return [T] * B
    if mode == 'all1':
        return [1] * B
    if mode == 'mixed':
        return [max(1, (T * (i + 1)) // (B + 1) + (i == 0)) if i < B - 1 else T for i in range(B)]
    return [0, T + 5, -3][:B] + [T] * max(0, B - 3)   # outside [1, T]: the kernels clamp


def _data(ctx, shape, kind):
    """activations [.., T, C] (time is the last but one axis)"""
    g = ctx.gen
    if kind == 'cancel':    # |mean| = 1e4 std: where a one-pass variance loses digits
        return 100.0 + 0.01 * torch.randn(shape, generator=g)
    x = torch.randn(shape, generator=g) + 0.5
    if kind == 'const':
        x[..., 0] = 3.25    # a constant channel: variance exactly 0
    return x


def _logits(ctx, shape, kind, taxis):
    """attention logits, the time axis at `taxis`"""
    T = shape[taxis]
    ramp = torch.arange(T, dtype=torch.float32).reshape([T if i == taxis else 1 for i in range(len(shape))])
    if kind == 'rand':
        return 3.0 * torch.randn(shape, generator=ctx.gen)
    if kind == 'rising':    # every step moves the running maximum
        return (0.37 * ramp).expand(shape).clone()
    if kind == 'falling':
        return (-0.37 * ramp).expand(shape).clone()
    if kind == 'equal':
        return torch.full(shape, 1.5)
    if kind == 'span80':    # weights underflow
        return (160.0 * torch.rand(shape, generator=ctx.gen) - 80.0)
    lg = torch.randn(shape, generator=ctx.gen)   # spike60: one frame carries all the weight
    sel = [slice(None)] * len(shape)
    sel[taxis] = T // 2
    lg[tuple(sel)] += 60.0
    return lg


for _i, (_T, _C) in enumerate(TC):
    for _op in ('time_mean', 'asp_stats', 'stats_pool', 'attn_pool'):
        modes = VMODES if (_T, _C) == (33, 257) else [VMODES[(_i + len(_op)) % 5]]
        for _m in modes:
            case(f'{_op}_T{_T}_C{_C}_{_m}', _op, B=3, T=_T, C=_C, vmode=_m)
    case(f'tstp_W{_T}_C{_C}', 'tstp', B=2, H=1 + 2 * (_i % 2), W=_T, C=_C, parts=1 + _i % 3, unbiased=_i % 2)
    case(f'astp_pool_T{_T}_C{_C}', 'astp_pool', B=2, F=1 + _i % 2, T=_T, C=_C)
for _op in ('asp_stats', 'stats_pool', 'attn_pool', 'time_mean'):
    for _k in ('cancel', 'const'):
        case(f'{_op}_{_k}', _op, B=2, T=100, C=65, vmode='mixed', data=_k)
for _k in ('cancel', 'const'):
    case(f'tstp_{_k}', 'tstp', B=2, H=2, W=100, C=65, parts=3, unbiased=1, data=_k)
    case(f'astp_pool_{_k}', 'astp_pool', B=2, F=2, T=100, C=65, data=_k)
for _p in (1, 2, 3):
    for _u in (0, 1):
        case(f'tstp_parts{_p}_unbiased{_u}', 'tstp', B=2, H=3, W=33, C=65, parts=_p, unbiased=_u)
case('tstp_one_frame_unbiased', 'tstp', B=2, H=2, W=1, C=65, parts=3, unbiased=1)
for _l in LOGITS[1:]:
    case(f'attn_pool_{_l}', 'attn_pool', B=3, T=33, C=65, vmode='mixed', logits=_l)
    case(f'astp_pool_{_l}', 'astp_pool', B=2, F=2, T=33, C=65, logits=_l)

EPS = {'asp_stats': 1e-12, 'attn_pool': 1e-12, 'tstp': 1e-8}


def _const_std(fam, eps):
    if fam == 'stats_pool':
        return 0.0
    if fam == 'astp_pool':
        return float(np.sqrt(np.float32(1e-10)))
    return float(np.sqrt(np.float32(eps)))


def _run_reduction(c, be):
    ctx = Ctx(c, be)
    fam, B, T, C = c['fam'], c['B'], c['T'], c['C']
    x = _data(ctx, (B, T, C), c.get('data', 'rand'))
    vlen = _vlen(c['vmode'], B, T)
    ld = C + 3
    dx = ctx.rows(x, ld)
    dv = None if vlen is None else ctx.up(torch.tensor(vlen, dtype=torch.int32))
    Tb = op_ref.frames(vlen, B, T)
    valid = (torch.arange(T)[None, :] < Tb[:, None])[:, :, None]
    amax = (x.abs().to(F64) * valid).amax(1)
    n = Tb[:, None].to(F64)
    ratio = 0.0
    if fam == 'time_mean':
        ref = op_ref.time_mean(x, vlen)
        ldo = C + 5
        o = ctx.out(B * ldo)
        ctx.launch(fam, dict(x=dx, B=B, T=T, C=C, ld=ld, out=o, ldo=ldo, vlen=dv))
        ctx.check(o, _idx2(B, C, ldo), ref['out'], (ref['n'] + 4) * U * ref['mag'])
        return ctx.report()
    o = ctx.out(B * 2 * C)
    idx = _idx2(B, 2 * C, 2 * C)
    if fam == 'attn_pool':
        lg = _logits(ctx, (B, T, C), c.get('logits', 'rand'), 1)
        ldl = C + 7
        args = (lg, x, EPS[fam], vlen)
        ref, ref32 = op_ref.attn_pool(*args), op_ref.attn_pool(*args, dt=F32)
        ctx.launch(fam, dict(logit=ctx.rows(lg, ldl), ldl=ldl, x=dx, ldx=ld, B=B, T=T, C=C, eps=EPS[fam], out=o, vlen=dv))
        bound, ratio = measured_bound(ref, ref32)
    else:
        if fam == 'asp_stats':
            ref, ref32 = op_ref.asp_stats(x, EPS[fam], vlen), op_ref.asp_stats(x, EPS[fam], vlen, dt=F32)
            ctx.launch(fam, dict(x=dx, B=B, T=T, C=C, ld=ld, eps=EPS[fam], out=o, vlen=dv))
        else:
            ref, ref32 = op_ref.stats_pool(x, vlen), op_ref.stats_pool(x, vlen, dt=F32)
            ctx.launch(fam, dict(x=dx, B=B, T=T, C=C, ld=ld, out=o, vlen=dv))
        bound, ratio = measured_bound(dict(out=ref['out'][:, C:], mag=ref['mag'][:, C:]),
                                      dict(out=ref32['out'][:, C:]))
        bound = torch.cat([(3 * n + 4) * U * amax, bound], 1)
    ctx.check(o, idx, ref['out'], bound)
    if c.get('data') == 'const':   # variance exactly 0: the clamp (or 0) comes out exactly
        want = torch.full((B, 1), _const_std(fam, EPS.get(fam)), dtype=F64)
        live = (Tb > 1)[:, None] | (fam != 'stats_pool')
        ctx.check(o, idx[:, C:C + 1], torch.where(live, want, torch.full_like(want, float('nan'))),
                  _ulp32(want) if be.emu else None, what='std of the constant channel', part=True, exact=not be.emu)
    return ctx.report(formula_ratio=ratio)


def _run_tstp(c, be):
    ctx = Ctx(c, be)
    B, H, W, C, parts, unb = c['B'], c['H'], c['W'], c['C'], c['parts'], c['unbiased']
    x = _data(ctx, (B, H, W, C), c.get('data', 'rand'))
    ld = C + 3
    ref, ref32 = op_ref.tstp(x, EPS['tstp'], unb, parts), op_ref.tstp(x, EPS['tstp'], unb, parts, dt=F32)
    np_ = (parts & 1) + (parts >> 1 & 1)
    o = ctx.out(B * np_ * H * C)
    ctx.launch('tstp', dict(x=ctx.rows(x, ld), B=B, H=H, W=W, C=C, ld=ld, eps=EPS['tstp'], unbiased=unb, out=o,
                            parts=parts))
    hc = H * C
    bounds, ratio = [], 0.0
    if parts & 1:
        bounds.append(((3 * W + 4) * U * x.abs().to(F64).amax(2)).reshape(B, hc))
    if parts & 2:
        s0 = hc * (parts & 1)
        b, ratio = measured_bound(dict(out=ref['out'][:, s0:], mag=ref['mag'][:, s0:]), dict(out=ref32['out'][:, s0:]))
        bounds.append(b)
    idx = _idx2(B, np_ * hc, np_ * hc)
    ctx.check(o, idx, ref['out'], torch.cat(bounds, 1))
    if c.get('data') == 'const' and parts & 2:
        cols = hc * (parts & 1) + torch.arange(H) * C
        want = torch.full((B, H), _const_std('tstp', EPS['tstp']), dtype=F64)
        ctx.check(o, idx[:, cols], want, _ulp32(want) if be.emu else None, what='std of the constant channel', part=True,
                  exact=not be.emu)
    return ctx.report(formula_ratio=ratio)


def _run_astp(c, be):
    ctx = Ctx(c, be)
    B, Fq, T, C = c['B'], c['F'], c['T'], c['C']
    x = _data(ctx, (B, Fq, T, C), c.get('data', 'rand'))
    lg = _logits(ctx, (B, T, Fq * C), c.get('logits', 'rand'), 1)
    ldx, ldl = C + 3, Fq * C + 5
    ref, ref32 = op_ref.astp_pool(lg, x), op_ref.astp_pool(lg, x, dt=F32)
    o = ctx.out(B * 2 * Fq * C)
    ctx.launch('astp_pool', dict(logit=ctx.rows(lg, ldl), ldl=ldl, x=ctx.rows(x, ldx), ldx=ldx, B=B, F=Fq, T=T, C=C, out=o))
    bound, ratio = measured_bound(ref, ref32)
    idx = _idx2(B, 2 * Fq * C, 2 * Fq * C)
    ctx.check(o, idx, ref['out'], bound)
    if c.get('data') == 'const':
        cols = Fq * C + torch.arange(Fq) * C
        want = torch.full((B, Fq), _const_std('astp_pool', None), dtype=F64)
        ctx.check(o, idx[:, cols], want, _ulp32(want) if be.emu else None, what='std of the constant channel', part=True,
                  exact=not be.emu)
    return ctx.report(formula_ratio=ratio)


# ---------------------------------------------------------------------------- se_apply
for _C in (4, 68, 260):
    case(f'se_apply_C{_C}', 'se_apply', B=3, T=17, C=_C, scale=1.0)
case('se_apply_range_at', 'se_apply', B=2, T=9, C=68, scale=16384.0)
case('se_apply_range_below', 'se_apply', B=2, T=9, C=68, scale=16383.0)


def _se_tensors(ctx, c):
    B, T, C = c['B'], c['T'], c['C']
    x = torch.rand(B, T, C, generator=ctx.gen) * 2 - 1
    g = torch.rand(B, C, generator=ctx.gen)
    r = torch.rand(B, T, C, generator=ctx.gen) * 2 - 1
    if c['scale'] != 1.0:   # the largest output is exactly `scale`: x = scale, gate = 1, res = 0 at one element
        x *= 100.0
        x[1, 3, 5], g[1, 5], r[1, 3, 5] = c['scale'], 1.0, 0.0
    return x, g, r


def _se_fields(ctx, c, x, g, r):
    B, T, C = c['B'], c['T'], c['C']
    ldx, ldg, ldr, ldo = C + 4, C + 8, C + 12, C + 16   # four distinct strides; the residual aliases nothing
    o = ctx.out(B * T * ldo)
    return dict(x=ctx.rows(x, ldx), ldx=ldx, gate=ctx.rows(g, ldg), ldg=ldg, res=ctx.rows(r, ldr), ldr=ldr, out=o,
                ldo=ldo, B=B, T=T, C=C, range_flag=ctx.flag()), o


def _run_se_apply(c, be):
    ctx = Ctx(c, be)
    x, g, r = _se_tensors(ctx, c)
    f, o = _se_fields(ctx, c, x, g, r)
    ref = op_ref.se_apply(x, g, r)
    ctx.launch('se_apply', f)
    idx = _idx2(c['B'] * c['T'], c['C'], f['ldo'])
    ctx.check(o, idx, ref['out'].reshape(-1, c['C']), (2 + 4) * U * ref['mag'].reshape(-1, c['C']))
    word = ctx.check_word(f['range_flag'], o, idx)
    assert (word != FLAG0) == (c['scale'] == 16384.0), (c['name'], word)
    return ctx.report()


# ---------------------------------------------------------------------------- stem conv
_STEM_T = [1, 63, 64, 65, 130]
_STEM_CO = [4, 16, 32, 64, 128]
for _i, _F in enumerate([1, 7, 8, 9, 17]):
    case(f'stem_F{_F}_T{_STEM_T[_i]}_co{_STEM_CO[_i]}', 'stem_conv3x3', B=2, F=_F, T=_STEM_T[_i], cout=_STEM_CO[_i],
         relu=_i % 2, vlen=None)
    case(f'stem_F{_F}_T{_STEM_T[-1 - _i]}_co{_STEM_CO[(_i + 2) % 5]}_vlen', 'stem_conv3x3', B=3, F=_F, T=_STEM_T[-1 - _i],
         cout=_STEM_CO[(_i + 2) % 5], relu=1 - _i % 2, vlen='mixed')
case('stem_vlen_past_T', 'stem_conv3x3', B=3, F=9, T=65, cout=32, relu=1, vlen=[65 + 70, 64, 65])
case('stem_range_up', 'stem_conv3x3', B=2, F=9, T=65, cout=32, relu=0, vlen=None, scale=3e4)


def _stem_build(ctx, c):
    B, Fq, T, cout = c['B'], c['F'], c['T'], c['cout']
    feats = torch.randn(B, T, Fq, generator=ctx.gen) * c.get('scale', 1.0)
    w = (torch.rand(cout, 9, generator=ctx.gen) * 2 - 1) / 3
    bias = (torch.rand(cout, generator=ctx.gen) * 2 - 1) * 0.2
    vlen = c['vlen']
    if vlen == 'mixed':
        vlen = [max(1, T - 1 - 7 * i) for i in range(B)]
    if vlen is not None:   # the padding frames hold large values: a frame before the end must see zeros
        past = torch.arange(T)[None, :] >= torch.tensor(vlen)[:, None]
        feats = torch.where(past[:, :, None], 1e4 * (1 + torch.rand(B, T, Fq, generator=ctx.gen)), feats)
    return feats, w, bias, vlen


def _stem_fields(ctx, c, feats, w, bias, vlen):
    B, Fq, T, cout = c['B'], c['F'], c['T'], c['cout']
    wstride, ldo = 32, cout + 4
    wp = torch.full((cout, wstride), PAD)
    wp[:, :9] = w
    o = ctx.out(B * Fq * T * ldo)
    return dict(feats=ctx.up(feats), B=B, T=T, F=Fq, w=ctx.up(wp), bias=ctx.up(bias), cout=cout, act=1 if c['relu'] else 0,
                wstride=wstride, out=o, ldo=ldo, vlen=None if vlen is None else ctx.up(torch.tensor(vlen, dtype=torch.int32)),
                range_flag=ctx.flag()), o


def _run_stem(c, be):
    ctx = Ctx(c, be)
    feats, w, bias, vlen = _stem_build(ctx, c)
    f, o = _stem_fields(ctx, c, feats, w, bias, vlen)
    ref = op_ref.stem(feats, w, bias, c['relu'], vlen)
    ctx.launch('stem', f)
    cout = c['cout']
    idx = _idx2(c['B'] * c['F'] * c['T'], cout, f['ldo'])
    zero = ref['masked'].reshape(-1, 1).expand(-1, cout)
    ctx.check(o, idx, ref['out'].reshape(-1, cout), (10 + 4) * U * ref['mag'].reshape(-1, cout), zero=zero)
    word = ctx.check_word(f['range_flag'], o, idx)
    assert (word != FLAG0) == ('scale' in c), (c['name'], word)
    if vlen is not None and min(vlen) < c['T']:
        assert bool(zero.any()), c['name']
    return ctx.report()


# ---------------------------------------------------------------------------- CAM context and gate
FUSED, PAIR_LEAN, PAIR_LDS = 'cam_gate_fused_kernel', 'cam_segsum_kernel+cam_gate_lean_kernel', \
    'cam_segsum_kernel+cam_gate_kernel'
MODEL_GATE = dict(C=128, red=64, growth=32)
# (name, shape, seg, nseg, T, vlen mode, expected route)
for _nseg, _T, _vm in [(1, 7, 'none'), (4, 40, 'mixed'), (5, 43, 'none'), (9, 83, 'empty')]:
    case(f'cam_gate_fused_nseg{_nseg}', 'cam_gate', B=3, T=_T, seg=10, nseg=_nseg, vmode=_vm, route=FUSED, **MODEL_GATE)
    case(f'cam_context_nseg{_nseg}', 'cam_context', B=3, T=_T, seg=10, nseg=_nseg, vmode=_vm, C=65)
case('cam_gate_fused_T_below_seg', 'cam_gate', B=2, T=7, seg=100, nseg=1, vmode='mixed', route=FUSED, **MODEL_GATE)
case('cam_context_T_below_seg', 'cam_context', B=2, T=7, seg=100, nseg=1, vmode='mixed', C=3)
case('cam_gate_pair_lean', 'cam_gate', B=2, T=229, seg=2, nseg=115, vmode='empty', route=PAIR_LEAN, **MODEL_GATE)
case('cam_gate_pair_lds_C96', 'cam_gate', B=3, T=43, seg=10, nseg=5, vmode='mixed', route=PAIR_LDS, C=96, red=48, growth=24)
case('cam_gate_pair_lds_C1024', 'cam_gate', B=2, T=23, seg=5, nseg=5, vmode='empty', route=PAIR_LDS, C=1024, red=4,
     growth=8)
case('cam_gate_pair_lds_nseg9', 'cam_gate', B=2, T=83, seg=10, nseg=9, vmode='outside', route=PAIR_LDS, C=96, red=48,
     growth=24)
case('cam_context_outside', 'cam_context', B=3, T=43, seg=10, nseg=5, vmode='outside', C=257)


def _cam_vlen(mode, B, T, seg):
    if mode == 'empty':   # trailing segments without a valid frame
        return [max(1, T - 2 * seg - 3 * i) for i in range(B)]
    return _vlen(mode, B, T)


def _cam_build(ctx, c):
    B, T, C = c['B'], c['T'], c['C']
    x = torch.randn(B, T, C, generator=ctx.gen) + 0.3
    vlen = _cam_vlen(c['vmode'], B, T, c['seg'])
    if vlen is not None:
        past = torch.arange(T)[None, :] >= torch.tensor(vlen).clamp(1, T)[:, None]
        x = torch.where(past[:, :, None], torch.full_like(x, 1e4), x)
    return x, vlen


def _run_cam_context(c, be):
    ctx = Ctx(c, be)
    x, vlen = _cam_build(ctx, c)
    B, T, C, seg, nseg = c['B'], c['T'], c['C'], c['seg'], c['nseg']
    ld, ldo = C + 3, C + 5
    o = ctx.out(B * nseg * ldo)
    ref = op_ref.cam_context(x, seg, nseg, vlen)
    ctx.launch('cam_context', dict(x=ctx.rows(x, ld), B=B, T=T, C=C, ld=ld, seg=seg, nseg=nseg, out=o, ldo=ldo,
                                   vlen=None if vlen is None else ctx.up(torch.tensor(vlen, dtype=torch.int32))))
    empty = (ref['n'] == 0).reshape(-1, C)
    ctx.check(o, _idx2(B * nseg, C, ldo), ref['out'].reshape(-1, C), ((ref['n'] + 4) * U * ref['mag']).reshape(-1, C),
              zero=empty)
    if c['vmode'] == 'empty':
        assert bool(empty.any()), c['name']
    return ctx.report()


def _cam_gate_fields(ctx, c, x, vlen, w1, b1, w2, b2):
    B, T, C, seg, nseg, red, growth = c['B'], c['T'], c['C'], c['seg'], c['nseg'], c['red'], c['growth']
    ld, k1p, k2p, ldg = C + 4, round_up(C, 32) + 32, round_up(red, 32) + 32, growth + 4
    gate, segsum = ctx.out(B * nseg * ldg), ctx.out(B * nseg * C)

    def padded(w, kp):   # packed GEMM weights: zero past K
        full = torch.zeros(w.shape[0], kp)
        full[:, :w.shape[1]] = w
        return ctx.up(full)

    return dict(x=ctx.rows(x, ld), B=B, T=T, C=C, ld=ld, seg=seg, nseg=nseg, w1=padded(w1, k1p), k1p=k1p, b1=ctx.up(b1),
                red=red, w2=padded(w2, k2p), k2p=k2p, b2=ctx.up(b2), growth=growth, gate=gate, ldg=ldg, segsum=segsum,
                vlen=None if vlen is None else ctx.up(torch.tensor(vlen, dtype=torch.int32)))


def _cam_weights(ctx, c):
    C, red, growth = c['C'], c['red'], c['growth']
    w1 = (torch.rand(red, C, generator=ctx.gen) * 2 - 1) / math.sqrt(C)
    b1 = torch.rand(red, generator=ctx.gen) * 0.5 - 0.1
    w2 = (torch.rand(growth, red, generator=ctx.gen) * 2 - 1) * 2 / math.sqrt(red)
    b2 = torch.rand(growth, generator=ctx.gen) - 0.5
    return w1, b1, w2, b2


def _run_cam_gate(c, be):
    ctx = Ctx(c, be)
    x, vlen = _cam_build(ctx, c)
    w1, b1, w2, b2 = _cam_weights(ctx, c)
    f = _cam_gate_fields(ctx, c, x, vlen, w1, b1, w2, b2)
    ref = op_ref.cam_gate(x, c['seg'], c['nseg'], w1, b1, w2, b2, vlen)
    kernel = ctx.launch('cam_gate', f, want_kernel=c['route'])
    g = c['growth']
    ctx.check(f['gate'], _idx2(c['B'] * c['nseg'], g, f['ldg']), ref['out'].reshape(-1, g),
              ref['err'].reshape(-1, g) + TRANS_T * ref['out'].reshape(-1, g), what='gate')
    # the scratch: untouched by the fused kernel, the segment sums and nothing past them otherwise
    raw = f['segsum'].cpu()
    n = c['B'] * c['nseg'] * c['C']
    if kernel == FUSED:
        ctx.untouched(raw, 'segsum (the fused kernel keeps the sums in LDS)')
    else:
        assert bool((raw[n:] == SENTINEL).all()), f"{c['name']}: writes past the segment sums"
        assert be.emu or not bool((raw[:n] == SENTINEL).any()), f"{c['name']}: segment sums not written"
    return ctx.report()


# ---------------------------------------------------------------------------- fused AFF
def aff_name(cp, nmid):
    if nmid == 32 and cp <= 128:
        cx = (cp + 31) // 32
        return f'aff_x3p_kernel<{cx}, {1 if cp - 32 * (cx - 1) <= 16 else 2}>'
    return f'aff_x3_kernel<{nmid // 32}>'


_AFF_M = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129]
for _i, _cp in enumerate([8, 16, 24, 32, 40, 48, 64, 72, 80, 96, 104, 112, 128]):
    case(f'aff_p_cp{_cp}', 'aff_x3', cp=_cp, nmid=32, M=_AFF_M[_i % 10], real=32 if _i % 3 else 26 - _i)
for _i, _cp in enumerate([136, 176, 208]):
    case(f'aff_1_cp{_cp}', 'aff_x3', cp=_cp, nmid=32, M=_AFF_M[(3 * _i + 1) % 10], real=32 - 5 * _i)
for _i, _cp in enumerate([8, 104, 208]):
    case(f'aff_2_cp{_cp}', 'aff_x3', cp=_cp, nmid=64, M=_AFF_M[(3 * _i + 5) % 10], real=64 - 7 * _i)
for _i, _m in enumerate(_AFF_M):
    case(f'aff_p_M{_m}', 'aff_x3', cp=40, nmid=32, M=_m, real=32)
    case(f'aff_2_M{_m}', 'aff_x3', cp=24, nmid=64, M=_m, real=52)
case('aff_p_many_tiles', 'aff_x3', cp=8, nmid=32, M='p_tiles', real=32)
case('aff_1_many_blocks', 'aff_x3', cp=136, nmid=32, M='blocks', real=32)
case('aff_p_range_up', 'aff_x3', cp=40, nmid=32, M=33, real=32, scale=1e4)
case('aff_p_range_below', 'aff_x3', cp=40, nmid=32, M=33, real=32, scale=4000.0)
case('aff_2_range_up', 'aff_x3', cp=24, nmid=64, M=33, real=64, scale=1e4)


def _aff_M(c, cus):
    # persistent form: blocks = min(ceil(tiles / 8), 2 CUs) of 8 waves, a wave walks 16-pixel tiles
    # with the stride of the grid: a block takes more than one tile per wave past 16 * 8 * 2 CUs pixels
    if c['M'] == 'p_tiles':
        return 16 * 8 * 2 * cus + 16 * 8 + 5
    if c['M'] == 'blocks':   # the plain form has one 128-pixel block per tile: several blocks, a ragged last one
        return 128 * 3 + 5
    return c['M']


def _aff_build(ctx, c, M):
    cp, nmid, real = c['cp'], c['nmid'], c['real']
    g, sc = ctx.gen, c.get('scale', 1.0)
    x = (torch.rand(M, cp, generator=g) * 2 + 1e-6) * sc
    y = (torch.rand(M, cp, generator=g) * 2 + 1e-6) * sc
    w1 = (torch.rand(nmid, 2 * cp, generator=g) * 2 - 1) / math.sqrt(2 * cp)
    b1 = torch.rand(nmid, generator=g) - 0.3
    w2 = (torch.rand(cp, nmid, generator=g) * 2 - 1) * 2 / math.sqrt(nmid)
    b2 = (torch.rand(cp, generator=g) * 2 - 1) * 0.3
    w1[real:] = 0.0          # a logical bottleneck narrower than nmid: zero rows of W1 and columns of W2,
    w2[:, real:] = 0.0       # and b1 stays non-zero there: SiLU(b1) must not leak
    return x, y, w1, b1, w2, b2


def _aff_fields(ctx, c, M, x, y, w1, b1, w2, b2):
    cp, nmid = c['cp'], c['nmid']
    kp1, kp2 = round_up(2 * cp, 32) + 32, nmid + 32
    ldx, ldy, ldo = cp + 4, cp + 8, cp + 12
    dev = ctx.be.device

    def padded(w, kp):
        full = torch.zeros(w.shape[0], kp)
        full[:, :w.shape[1]] = w
        return ctx.up(full)

    def plane(n):
        p = torch.zeros(n, dtype=torch.int16, device=dev)
        ctx.keep.append(p)
        return p

    o = ctx.out(max(M, 1) * ldo)
    return dict(x=ctx.rows(x, ldx), ldx=ldx, y=ctx.rows(y, ldy), ldy=ldy, out=o, ldo=ldo, M=M, cp=cp, nmid=nmid,
                w1=padded(w1, kp1), w1h=plane(nmid * kp1), w1l=plane(nmid * kp1), b1=ctx.up(b1), kp1=kp1,
                w2=padded(w2, kp2), w2h=plane(cp * kp2), w2l=plane(cp * kp2), b2=ctx.up(b2), kp2=kp2,
                range_flag=ctx.flag()), o


def _run_aff(c, be):
    ctx = Ctx(c, be)
    M = _aff_M(c, be.cus)
    t = _aff_build(ctx, c, M)
    f, o = _aff_fields(ctx, c, M, *t)
    ref = op_ref.aff(*t, C_EMU if be.emu else C_X3)
    ctx.launch('aff', f, want_kernel=aff_name(c['cp'], c['nmid']))
    idx = _idx2(M, c['cp'], f['ldo'])
    ctx.check(o, idx, ref['out'], ref['err'] + TRANS_T * ref['out'].abs())
    word = ctx.check_word(f['range_flag'], o, idx)
    assert (word != FLAG0) == (c.get('scale', 1.0) == 1e4), (c['name'], word)
    return ctx.report()


# ---------------------------------------------------------------------------- fused Res2Net block
R2_NAME = {0: 'res2_block_kernel<128, 128, false>', 1: 'res2_block_kernel<64, 128, true>'}
_R2_H, _R2_W, _R2_WIDTH = [1, 7, 8, 9, 17], [1, 15, 16, 17, 33], [1, 17, 26, 32]
for _i in range(5):
    for _proj in (0, 1):
        _j = (_i + 2 * _proj) % 5
        case(f'res2_{"proj" if _proj else "id"}_{_R2_H[_i]}x{_R2_W[_j]}', 'res2_block', proj=_proj, nimg=1 + 2 * ((_i + _proj) % 2),
             H=_R2_H[_i], W=_R2_W[_j], width=_R2_WIDTH[(_i + _proj + 1) % 4])
case('res2_id_more_tiles_than_grid', 'res2_block', proj=0, nimg='cus', H=9, W=17, width=26)
case('res2_proj_more_tiles_than_grid', 'res2_block', proj=1, nimg='cus', H=8, W=17, width=26)


def _res2_build(ctx, c, nimg):
    proj, H, W, width = c['proj'], c['H'], c['W'], c['width']
    C, Cout, g = (64 if proj else 128), 128, ctx.gen

    def uw(*shape):
        return torch.rand(*shape, generator=g) * 2 - 1

    def ub(n, lo, hi):   # positive biases: Hardtanh(bias) in place of a halo's 0 shows at the border
        return lo + (hi - lo) * torch.rand(n, generator=g)

    x = torch.rand(nimg, H, W, C, generator=g) * 2 + 1e-6
    # scales that spread every stage's pre-activation over (< 0, inside, > 20) of its Hardtanh
    lw = dict(w1=uw(2 * width, C) * (2.4 * math.sqrt(128.0 / C)), b1=ub(2 * width, 2.0, 6.0),
              wa=uw(width, width, 3, 3) * (2.6 / math.sqrt(9 * width)), ba=ub(width, 2.0, 6.0),
              wb=uw(width, width, 3, 3) * (1.6 / math.sqrt(9 * width)), bb=ub(width, 2.0, 6.0),
              w3=uw(Cout, 2 * width) * (2.4 / math.sqrt(2 * width)), b3=uw(Cout) * 2.0 + 4.0)
    if proj:
        lw['wp'] = uw(Cout, C) * (6.0 / math.sqrt(C))
    return x, lw, C, Cout


def _res2_fields(ctx, c, nimg, x, lw, C, Cout):
    p = op_ref.pack_res2(lw, C, Cout, c['width'], c['proj'])
    dev = ctx.be.device
    f = dict(x=ctx.up(x), nimg=nimg, H=c['H'], W=c['W'], C=C, Cout=Cout, stride=1, Hin=0, Win=0, proj=c['proj'],
             width=c['width'])
    for k in ('w1', 'wa', 'wb', 'w3'):
        f[k] = ctx.up(p[k])
        for s in 'hl':
            f[k + s] = torch.zeros(p[k].numel(), dtype=torch.int16, device=dev)
            ctx.keep.append(f[k + s])
        f['b' + k[1]] = ctx.up(p['b' + k[1]])
    o = ctx.out(nimg * c['H'] * c['W'] * Cout)
    f['out'] = o
    return f, o


def _res2_nimg(c, cus):
    if c['nimg'] != 'cus':
        return c['nimg']
    tiles = -(-c['H'] // 8) * -(-c['W'] // 16)   # per image; the grid is at most the CU count
    return cus // tiles + 1


def _run_res2(c, be):
    ctx = Ctx(c, be)
    nimg = _res2_nimg(c, be.cus)
    x, lw, C, Cout = _res2_build(ctx, c, nimg)
    f, o = _res2_fields(ctx, c, nimg, x, lw, C, Cout)
    ref = op_ref.res2_block(x, lw, c['width'], c['proj'], C_EMU if be.emu else C_X3)
    if c['nimg'] == 'cus':
        assert nimg * -(-c['H'] // 8) * -(-c['W'] // 16) > be.cus
    ctx.launch('res2', f, want_kernel=R2_NAME[c['proj']])
    n = nimg * c['H'] * c['W']
    ctx.check(o, _idx2(n, Cout, Cout), ref['out'].reshape(n, Cout), ref['err'].reshape(n, Cout))
    for stage, (lo, mid, hi, count) in ref['clamped'].items():
        # a stage of a handful of values (the 1 x 1 image) cannot show all three, and the nine
        # weights of a one-channel slice decide its sign alone
        assert count < 400 or c['width'] == 1 or min(lo, mid, hi) > 0.0, f"{c['name']}: {stage} has shares {lo:.3f} / {mid:.3f} / {hi:.3f} at 0 / inside / 20"
    return ctx.report()


# ---------------------------------------------------------------------------- exact ops
for _n in (1, 255, 257, 8192 * 256 + 77):
    case(f'split_f16_n{_n}', 'split_f16', n=_n)
for _n in (1, 255, 257, 1024 * 256 + 77):
    for _v in ('2^15', '-2^15', 'below', 'inf', '2^14', 'below14'):
        if _n in (1, 257) or _v == '2^15':
            case(f'range_check_n{_n}_{_v}', 'range_check', n=_n, value=_v)
case('word_reset', 'word_reset')
for _B in (1, 256, 257):
    case(f'derive_len_B{_B}', 'derive_len', B=_B)


def _run_split(c, be):
    ctx = Ctx(c, be)
    n = c['n']
    w = torch.randn(n, generator=ctx.gen)
    k = min(n, 64)
    # lows that land in fp16 subnormals ((w - hi) 2^11 below 2^-14), exact halves, ties, zeros, both signs
    special = torch.tensor([2.0 ** -3 + 2.0 ** -26, 2.0 ** -5 + 3 * 2.0 ** -28, 0.25 - 2.0 ** -26, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,
                            0.0, -0.0, 2.0 ** -14, 2.0 ** -24, 3 * 2.0 ** -25, 1000.0 + 2.0 ** -10, -3.14159, 65000.0,
                            2.0 ** -15 + 2.0 ** -40], dtype=torch.float32)
    w[:k] = special.repeat(5)[:k] * torch.where(torch.arange(k) % 3 == 0, -1.0, 1.0)
    hi = torch.full((n + GUARD,), 0x5A5A, dtype=torch.int16, device=be.device)
    lo = torch.full((n + GUARD,), 0x5A5A, dtype=torch.int16, device=be.device)
    ctx.launch('split_f16', dict(w=ctx.up(w), hi=hi, lo=lo, n=n))
    rh, rl = op_ref.split_f16(w)
    for got, ref, what in ((hi.cpu(), rh, 'hi'), (lo.cpu(), rl, 'lo')):
        assert bool((got[n:] == 0x5A5A).all()), f"{c['name']}: writes past the {what} plane"
        bad = got[:n] != ref
        assert not bool(bad.any()), f"{c['name']}: {int(bad.sum())} {what} halves differ, first at {int(bad.nonzero()[0])}: " \
                                    f"w {float(w[bad][0])!r} got {int(got[:n][bad][0]) & 0xFFFF:#06x} want {int(ref[bad][0]) & 0xFFFF:#06x}"
    sub = (rl.view(torch.float16).abs() < 2.0 ** -14) & (rl.view(torch.float16) != 0)
    assert n < 64 or bool(sub.any()), 'no low half in the fp16 subnormals'
    return ctx.report()


def _run_range_check(c, be):
    ctx = Ctx(c, be)
    n = c['n']
    below = float(np.nextafter(np.float32(2.0 ** 15), np.float32(0)))
    below14 = float(np.nextafter(np.float32(2.0 ** 14), np.float32(0)))
    v = {'2^15': 2.0 ** 15, '-2^15': -2.0 ** 15, 'below': below, 'inf': float('inf'), '2^14': 2.0 ** 14,
         'below14': below14}[c['value']]
    x = torch.rand(n, generator=ctx.gen) * 2000.0 - 1000.0
    x[n - 1] = v   # the maximum at the last element
    flag = ctx.flag()
    ctx.launch('range_check', dict(x=ctx.up(x), n=n, flag=flag))
    word = flag.cpu()
    # common.h: the word takes the bits of the largest |x| once that reaches kRangeLimit = 2^14
    want = int(torch.tensor(abs(v), dtype=torch.float32).view(torch.int32)) if abs(v) >= 2.0 ** 14 else FLAG0
    assert int(word[0]) == want and bool((word[1:] == 0).all()), (c['name'], [hex(int(i)) for i in word])
    return ctx.report()


def _run_word_reset(c, be):
    ctx = Ctx(c, be)
    w = ctx.up(torch.tensor([0x47000000, 7, 7, 7], dtype=torch.int32))
    ctx.launch('word_reset', dict(w=w))
    assert w.cpu().tolist() == [0, 7, 7, 7], w.cpu().tolist()
    return ctx.report()


def _run_derive_len(c, be):
    ctx = Ctx(c, be)
    B = c['B']
    pad, k, stride = 2, 5, 2     # the CAM++ TDNN front (campplus.cpp): lengths the host admits, 1 <= len <= T
    lens = torch.randint(1, 3000, (B,), generator=ctx.gen, dtype=torch.int32)
    lens[0] = 1
    o = ctx.out(B)
    ctx.launch('derive_len', dict(out=o, B=B, pad=pad, k=k, stride=stride, **{'in': ctx.up(lens)}))
    raw = o.cpu()
    assert bool((raw[B:] == SENTINEL).all()), c['name']
    assert bool((raw[:B].long() == op_ref.derive_len(lens, pad, k, stride)).all()), c['name']
    return ctx.report()


RUNNERS = {'time_mean': _run_reduction, 'asp_stats': _run_reduction, 'stats_pool': _run_reduction,
           'attn_pool': _run_reduction, 'tstp': _run_tstp, 'astp_pool': _run_astp, 'se_apply': _run_se_apply,
           'stem_conv3x3': _run_stem, 'cam_context': _run_cam_context, 'cam_gate': _run_cam_gate, 'aff_x3': _run_aff,
           'res2_block': _run_res2, 'split_f16': _run_split, 'range_check': _run_range_check,
           'word_reset': _run_word_reset, 'derive_len': _run_derive_len}
FAMILIES = sorted(RUNNERS)
BY_NAME = {c['name']: c for c in CASES}


def run_case(c, be):
    return RUNNERS[c['fam']](c, be)


# ---------------------------------------------------------------------------- refused descriptors
def _set(**kw):
    return lambda f: f.update(kw)


def _misalign(k):
    return lambda f: f.update({k: f[k].data_ptr() + 4})


def _alias_out(f):
    f['out'] = f['x']


REJECTS = [
    # (name, family, base case, what breaks the descriptor)
    ('aff_cp_mod8', 'aff_x3', 'aff_p_cp40', _set(cp=36)),
    ('aff_cp_216', 'aff_x3', 'aff_1_cp208', _set(cp=216)),
    ('aff_nmid_16', 'aff_x3', 'aff_p_cp40', _set(nmid=16)),
    ('aff_ldx_mod4', 'aff_x3', 'aff_p_cp40', _set(ldx=46)),
    ('aff_ldo_below_cp', 'aff_x3', 'aff_p_cp40', _set(ldo=36)),
    ('aff_x_misaligned', 'aff_x3', 'aff_p_cp40', _misalign('x')),
    ('aff_null_b1', 'aff_x3', 'aff_p_cp40', _set(b1=None)),
    ('aff_kp1_below_2cp', 'aff_x3', 'aff_p_cp40', _set(kp1=72)),
    ('aff_M_zero', 'aff_x3', 'aff_p_cp40', _set(M=0)),
    ('res2_stride2', 'res2_block', 'res2_id_7x15', _set(stride=2)),
    ('res2_C256', 'res2_block', 'res2_id_7x15', _set(C=256, Cout=256)),
    ('res2_width0', 'res2_block', 'res2_id_7x15', _set(width=0)),
    ('res2_width33', 'res2_block', 'res2_id_7x15', _set(width=33)),
    ('res2_x_is_out', 'res2_block', 'res2_id_7x15', _alias_out),
    ('res2_null_plane', 'res2_block', 'res2_id_7x15', _set(wbl=None)),
    ('res2_nimg0', 'res2_block', 'res2_id_7x15', _set(nimg=0)),
    ('se_apply_C_mod4', 'se_apply', 'se_apply_C68', _set(C=66)),
    ('se_apply_ldg_mod4', 'se_apply', 'se_apply_C68', _set(ldg=78)),
    ('cam_gate_C_mod4', 'cam_gate', 'cam_gate_pair_lds_C96', _set(C=94)),
    ('cam_gate_C1028', 'cam_gate', 'cam_gate_pair_lds_C1024', _set(C=1028)),
    ('cam_gate_ld_mod4', 'cam_gate', 'cam_gate_pair_lds_C96', _set(ld=98)),
    ('cam_gate_red0', 'cam_gate', 'cam_gate_pair_lds_C96', _set(red=0)),
    ('cam_gate_red1025', 'cam_gate', 'cam_gate_pair_lds_C96', _set(red=1025)),
    ('cam_gate_B0', 'cam_gate', 'cam_gate_pair_lds_C96', _set(B=0)),
    ('cam_gate_nseg0', 'cam_gate', 'cam_gate_pair_lds_C96', _set(nseg=0)),
    ('cam_gate_lds_over_64k', 'cam_gate', 'cam_gate_pair_lds_C1024', _set(red=20)),   # 1024 * 21 floats alone are 84 KB
    ('stem_cout6', 'stem_conv3x3', 'stem_F7_T65_co64_vlen', _set(cout=6)),
    ('stem_cout12', 'stem_conv3x3', 'stem_F7_T65_co64_vlen', _set(cout=12)),
    ('stem_cout132', 'stem_conv3x3', 'stem_F17_T130_co128', _set(cout=132)),
    ('stem_ldo_mod4', 'stem_conv3x3', 'stem_F7_T65_co64_vlen', _set(ldo=22)),
]
SPK_E_INVALID = -1


def run_reject(name, be):
    """A descriptor the host check must refuse: SPK_E_INVALID comes back, nothing is written."""
    _, fam, base, breakit = next(r for r in REJECTS if r[0] == name)
    c = BY_NAME[base]
    ctx = Ctx(c, be)
    outs = []
    if fam == 'aff_x3':
        M = _aff_M(c, be.cus)
        f, o = _aff_fields(ctx, c, M, *_aff_build(ctx, c, M))
        op, outs = 'aff', [o]
    elif fam == 'res2_block':
        x, lw, C, Cout = _res2_build(ctx, c, c['nimg'])
        f, o = _res2_fields(ctx, c, c['nimg'], x, lw, C, Cout)
        op, outs = 'res2', [o]
    elif fam == 'se_apply':
        f, o = _se_fields(ctx, c, *_se_tensors(ctx, c))
        op, outs = 'se_apply', [o]
    elif fam == 'cam_gate':
        x, vlen = _cam_build(ctx, c)
        f = _cam_gate_fields(ctx, c, x, vlen, *_cam_weights(ctx, c))
        op, outs = 'cam_gate', [f['gate'], f['segsum']]
    else:
        feats, w, bias, vlen = _stem_build(ctx, c)
        f, o = _stem_fields(ctx, c, feats, w, bias, vlen)
        op, outs = 'stem', [o]
    keep_x = f.get('x')
    breakit(f)
    rc, kernel, err = op_diag.launch(be.handle, op, f)
    be.sync()
    assert rc == SPK_E_INVALID, f'{name}: returned {rc} [{kernel}] {err}'
    assert err, name
    for o in outs:
        ctx.untouched(o, 'an output of the refused launch')
    if 'range_flag' in f:
        assert int(f['range_flag'].cpu()[0]) == FLAG0, name
    del keep_x
    print(f'{name}: refused ({rc}): {err}')
