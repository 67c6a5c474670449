"""TEST INFRASTRUCTURE: references of the kernel entries that are not convs (csrc/aff.h,
res2block.h, tdnn_ops.h, misc.h), written from the model source the kernels implement
(speakerlab/models/...: ECAPA_TDNN.py SE / ASP statistics, campplus/layers.py statistics
pooling and CAMLayer context, eres2net/pooling_layers.py TSTP / ASTP, eres2net/fusion.py AFF,
ERes2NetV2.py BasicBlockERes2NetV2) and the header comments, independent of libspk_hip.so and
of the host emulation.

Every function takes `dt`: torch.float64 gives the reference, torch.float32 the model source's
own formula in its own precision (the yardstick of the one-pass standard deviations, see
op_cases.py).  Each returns the expected output and `mag`, a per-element magnitude for the
error bound: sum |terms| for sums; for chained stages the bound itself (`err`), each stage's
c * magnitude carried through the later stages by |W| and the Lipschitz constants of SiLU
(1.1), tanh (1) and Hardtanh (1), as conv_ref.py does for one stage.

WRONG holds the names of deliberate mistakes (the sensitivity test of
test_op_contract_emu.py switches them on one at a time to show that the cases and bounds
discriminate); it is empty otherwise.

Packed layouts of the fused Res2Net block (Res2Desc, res2block.h), built by pack_res2():
the Res2Net slice of `width` <= 32 channels is padded to 32, so
  w1 [64][C]        row n = 32 * slice + j  <- conv1 output channel slice * width + j
  wa, wb [32][9*32] element [n][tap * 32 + c], tap = 3 ky + kx (the tap is the major index)
  w3 [Cout][64(+C)] column 32 * slice + j <- concat channel slice * width + j; with the
                    projection shortcut, columns 64 .. 64 + C are its 1x1 weights
and every padded row, column and bias is zero."""
import torch
import torch.nn.functional as Fn

F64, F32 = torch.float64, torch.float32
WRONG = set()


def frames(vlen, B, T):
    """valid frames per utterance, clamped to [1, T] as the kernels do"""
    if vlen is None or 'ignore_vlen' in WRONG:
        return torch.full((B,), T, dtype=torch.long)
    return torch.as_tensor(vlen, dtype=torch.long).clamp(1, T)


def _mask(Tb, T, dt):
    return (torch.arange(T)[None, :] < Tb[:, None]).to(dt)   # [B, T]


# ------------------------------------------------------------------ time reductions
def time_mean(x, vlen=None, dt=F64):
    """SE squeeze (ECAPA_TDNN.py:209-216): mean over the valid frames.  x [B, T, C]"""
    B, T, _ = x.shape
    Tb = frames(vlen, B, T)
    m = _mask(Tb, T, dt)[:, :, None]
    div = torch.full_like(Tb, T) if 'T_for_Tb' in WRONG else Tb
    x = x.to(dt)
    out = (x * m).sum(1) / div[:, None].to(dt)
    mag = (x.abs() * m).sum(1) / Tb[:, None].to(dt)
    return dict(out=out, mag=mag, n=Tb[:, None].expand_as(out))


def _weighted_stats(x, w, eps, dt):
    """_compute_statistics (ECAPA_TDNN.py:256-270): mean = sum w x, std = sqrt(clamp(sum w (x - mean)^2, eps))"""
    x = x.to(dt)
    mean = (w * x).sum(1)
    var = (w * (x - mean[:, None]).pow(2)).sum(1)
    std = torch.sqrt(var.clamp(min=eps))
    mag = torch.cat([(w * x.abs()).sum(1), torch.sqrt((w * x * x).sum(1))], dim=1)
    return dict(out=torch.cat([mean, std], dim=1), mag=mag)


def asp_stats(x, eps, vlen=None, dt=F64):
    """global-context statistics: weights 1 / Tb on the valid frames.  out [B, 2C]"""
    B, T, _ = x.shape
    Tb = frames(vlen, B, T)
    div = torch.full_like(Tb, T) if 'T_for_Tb' in WRONG else Tb
    w = (_mask(Tb, T, dt) / div[:, None].to(dt))[:, :, None]
    return _weighted_stats(x, w, eps, dt)


def attn_pool(logit, x, eps, vlen=None, dt=F64):
    """attentive statistics (ECAPA_TDNN.py:276-287): softmax over the valid frames of the
    logits (masked_fill(-inf) past them), then the weighted statistics"""
    B, T, _ = x.shape
    Tb = frames(vlen, B, T)
    valid = _mask(Tb, T, dt)[:, :, None] > 0
    w = torch.softmax(logit.to(dt).masked_fill(~valid, float('-inf')), dim=1)
    return _weighted_stats(x, w, eps, dt)


def stats_pool(x, vlen=None, dt=F64):
    """CAM++ statistics pooling (campplus/layers.py:26-37): mean and unbiased std, no eps;
    one frame gives NaN as torch.std does"""
    B, T, C = x.shape
    Tb = frames(vlen, B, T)
    outs, mags = [], []
    for b in range(B):
        xb = x[b, :int(Tb[b])].to(dt)
        mean = xb.mean(0)
        std = xb.std(0, unbiased='biased' not in WRONG) if xb.shape[0] > 1 or 'biased' in WRONG else \
            torch.full((C,), float('nan'), dtype=dt)
        outs.append(torch.cat([mean, std]))
        mags.append(torch.cat([xb.abs().mean(0), torch.sqrt((xb * xb).mean(0))]))
    return dict(out=torch.stack(outs), mag=torch.stack(mags))


def tstp(x, eps, unbiased, parts, dt=F64):
    """TSTP / TAP / TSDP (pooling_layers.py:10-55): x [B, H, W, C] -> [B, np * H * C], the mean
    at h * C + c, then sqrt(var + eps) (torch.var: unbiased, NaN for one frame)"""
    B, H, W, C = x.shape
    x = x.to(dt)
    mean = x.mean(2)
    if unbiased and 'biased' not in WRONG:
        var = x.var(2, unbiased=True) if W > 1 else torch.full_like(mean, float('nan'))
    else:
        var = x.var(2, unbiased=False)
    std = torch.sqrt(var + eps)
    o, m = [], []
    if parts & 1:
        o.append(mean.reshape(B, -1)); m.append(x.abs().mean(2).reshape(B, -1))
    if parts & 2:
        o.append(std.reshape(B, -1)); m.append(torch.sqrt((x * x).mean(2)).reshape(B, -1))
    return dict(out=torch.cat(o, 1), mag=torch.cat(m, 1))


def astp_pool(logit, x, dt=F64):
    """ASTP (pooling_layers.py:93-104): x [B, F, T, C], logits [B, T, F*C] (column f*C + c);
    alpha = softmax_T, mean = sum alpha x, std = sqrt(clamp(sum alpha x^2 - mean^2, 1e-10))"""
    B, Fq, T, C = x.shape
    x = x.to(dt)
    lg = logit.to(dt).reshape(B, T, Fq, C).permute(0, 2, 1, 3)
    a = torch.softmax(lg, dim=2)
    mean = (a * x).sum(2)
    var = (a * x * x).sum(2) - mean * mean
    std = torch.sqrt(var.clamp(min=1e-10))
    mag = torch.cat([(a * x.abs()).sum(2).reshape(B, -1), torch.sqrt((a * x * x).sum(2)).reshape(B, -1)], 1)
    return dict(out=torch.cat([mean.reshape(B, -1), std.reshape(B, -1)], 1), mag=mag)


# ------------------------------------------------------------------ elementwise / small
def se_apply(x, gate, res):
    """out = x * gate[b, c] + residual (ECAPA_TDNN.py:222, 347).  x, res [B, T, C], gate [B, C]"""
    x, g, r = x.to(F64), gate.to(F64)[:, None, :], res.to(F64)
    if 'no_res' in WRONG:
        r = torch.zeros_like(r)
    return dict(out=x * g + r, mag=(x * g).abs() + r.abs())


def stem(feats, w, bias, relu, vlen=None):
    """3x3 conv, 1 -> cout channels, on feats [B, T, F] read as the image [F, T] (ERes2NetV2.py:
    236-238, DTDNN.py:40-41), zero padding, folded BN bias, optional ReLU; with vlen, frames
    >= vlen[b] read as zero and their outputs are zero.  w [cout, 9] (tap = 3 dy + dx, dy along
    F).  out [B, F, T, cout]"""
    B, T, Fq = feats.shape
    Tb = torch.full((B,), T, dtype=torch.long) if vlen is None or 'ignore_vlen' in WRONG else \
        torch.as_tensor(vlen, dtype=torch.long).clamp(max=T)
    keep = (torch.arange(T)[None, :] < Tb[:, None]).to(F64)          # [B, T]
    img = (feats.to(F64) * keep[:, :, None]).permute(0, 2, 1)[:, None]   # [B, 1, F, T]
    wk = w.to(F64).reshape(-1, 1, 3, 3).clone()
    if 'drop_tap' in WRONG:
        wk[:, :, 2, 0] = 0.0
    acc = Fn.conv2d(img, wk, padding=1) + bias.to(F64)[None, :, None, None]
    mag = Fn.conv2d(img.abs(), wk.abs(), padding=1) + bias.to(F64).abs()[None, :, None, None]
    out = acc.clamp(min=0.0) if relu else acc
    out = out * keep[:, None, None, :]
    masked = (keep == 0)[:, None, :].expand(B, Fq, T)
    return dict(out=out.permute(0, 2, 3, 1), mag=mag.permute(0, 2, 3, 1), masked=masked)


def derive_len(lens, pad, k, stride):
    return (torch.as_tensor(lens, dtype=torch.long) + 2 * pad - k) // stride + 1


# ------------------------------------------------------------------ CAM context and gate
def cam_context(x, seg, nseg, vlen=None, dt=F64):
    """CAMLayer context (campplus/layers.py:93-110): mean over the valid frames + the mean of
    the segment's valid frames (avg_pool1d(seg, seg, ceil_mode=True)); a segment without a
    valid frame is written as 0.  x [B, T, C] -> [B, nseg, C]"""
    B, T, C = x.shape
    Tb = frames(vlen, B, T)
    x = x.to(dt)
    out = torch.zeros(B, nseg, C, dtype=dt)
    mag = torch.zeros(B, nseg, C, dtype=dt)
    n = torch.zeros(B, nseg, 1, dtype=dt)
    off = 1 if 'seg_off1' in WRONG else 0
    for b in range(B):
        tb = int(Tb[b])
        mean, amean = x[b, :tb].mean(0), x[b, :tb].abs().mean(0)
        for s in range(nseg):
            t0, t1 = s * seg + off, min(tb, s * seg + seg + off)
            if t1 > t0:
                out[b, s] = mean + x[b, t0:t1].mean(0)
                mag[b, s] = amean + x[b, t0:t1].abs().mean(0)
                n[b, s] = tb + t1 - t0
    return dict(out=out, mag=mag, n=n.expand_as(out))


def cam_gate(x, seg, nseg, w1, b1, w2, b2, vlen=None, u=2.0 ** -24):
    """gate = sigmoid(W2 relu(W1 ctx + b1) + b2) per (utterance, segment); w1 [red, C], w2
    [growth, red].  `err`: the fp32 bound, (n + 4) u sum |terms| per dot product, carried
    through ReLU (1) and the sigmoid (1/4)"""
    c = cam_context(x, seg, nseg, vlen)
    ctx, e_ctx = c['out'], (c['n'] + 4) * u * c['mag']
    W1, W2 = w1.to(F64), w2.to(F64)
    B1 = torch.zeros(W1.shape[0], dtype=F64) if b1 is None else b1.to(F64)
    B2 = torch.zeros(W2.shape[0], dtype=F64) if b2 is None else b2.to(F64)
    a1 = ctx @ W1.t() + B1
    e1 = e_ctx @ W1.abs().t() + (W1.shape[1] + 4) * u * (ctx.abs() @ W1.abs().t() + B1.abs())
    h = a1.clamp(min=0.0)
    a2 = h @ W2.t() + B2
    e2 = e1 @ W2.abs().t() + (W2.shape[1] + 4) * u * (h @ W2.abs().t() + B2.abs())
    out = torch.sigmoid(a2)
    return dict(out=out, err=0.25 * e2 + 4 * u * out)


# ------------------------------------------------------------------ fused AFF
def aff(x, y, w1, b1, w2, b2, c):
    """AFF (eres2net/fusion.py:8-28): h = SiLU(W1 [x | y] + b1), z = W2 h + b2,
    out = x (1 + tanh z) + y (1 - tanh z).  x, y [M, cp]; w1 [nmid, 2 cp]; w2 [cp, nmid];
    c: the per-stage constant of the fp16x3 products"""
    x, y = x.to(F64), y.to(F64)
    if 'swap_xy' in WRONG:
        x, y = y, x
    xy = torch.cat([x, y], 1)
    W1, W2, B1, B2 = w1.to(F64), w2.to(F64), b1.to(F64), b2.to(F64)
    a1 = xy @ W1.t() + B1
    e1 = c * (xy.abs() @ W1.abs().t() + B1.abs())
    h = a1 * torch.sigmoid(a1)
    eh = 1.1 * e1
    z = h @ W2.t() + B2
    ez = c * (h.abs() @ W2.abs().t() + B2.abs()) + eh @ W2.abs().t()
    t = 1.0 + torch.tanh(z)
    out = x * t + y * (2.0 - t)
    err = (x.abs() + y.abs()) * ez + 4 * 2.0 ** -24 * (x.abs() * t + y.abs() * (2.0 - t))
    return dict(out=out, err=err)


# ------------------------------------------------------------------ fused Res2Net block
def pack_res2(lw, C, Cout, width, proj):
    """logical weights (conv1 [2 width, C], convs.0 / convs.1 [width, width, 3, 3], conv3
    [Cout, 2 width], shortcut [Cout, C]; BN folded, biases b1 [2 width], ba, bb [width], b3
    [Cout]) -> the packed fp32 matrices of Res2Desc (layouts in the module docstring)"""
    p = dict(w1=torch.zeros(64, C), b1=torch.zeros(64), wa=torch.zeros(32, 9, 32), ba=torch.zeros(32),
             wb=torch.zeros(32, 9, 32), bb=torch.zeros(32), w3=torch.zeros(Cout, 64 + (C if proj else 0)),
             b3=lw['b3'].clone())
    for s in range(2):
        p['w1'][32 * s:32 * s + width] = lw['w1'][s * width:(s + 1) * width]
        p['b1'][32 * s:32 * s + width] = lw['b1'][s * width:(s + 1) * width]
        p['w3'][:, 32 * s:32 * s + width] = lw['w3'][:, s * width:(s + 1) * width]
    for k in 'ab':
        # [n, c, ky, kx] -> [n, tap, c]
        p['w' + k][:width, :, :width] = lw['w' + k].permute(0, 2, 3, 1).reshape(width, 9, width)
        p['b' + k][:width] = lw['b' + k]
    if proj:
        p['w3'][:, 64:] = lw['wp']
    p['wa'] = p['wa'].reshape(32, 288).contiguous()
    p['wb'] = p['wb'].reshape(32, 288).contiguous()
    return p


def res2_block(x, lw, width, proj, c):
    """BasicBlockERes2NetV2 with scale 2 (ERes2NetV2.py:65-91), BN folded: t = Ht(conv1 x),
    y0 = Ht(convs.0(t[:width])), y1 = Ht(convs.1(y0 + t[width:])), out = Ht(conv3 cat(y0, y1) +
    shortcut(x)); 3x3 convs zero-padded.  x [nimg, H, W, C] -> out [nimg, H, W, Cout], `err` the
    carried bound and `clamped`: per stage the shares (at 0, inside, at 20) of its Hardtanh"""
    X = x.to(F64).permute(0, 3, 1, 2)
    halo = 'halo_bias' in WRONG
    if halo:   # the mistake: halo pixels outside the image computed as pixels with x = 0
        X = Fn.pad(X, (2, 2, 2, 2))
    pad = 0 if halo else 1
    ht = lambda v: v.clamp(0.0, 20.0)
    shares = {}

    def note(name, v):
        shares[name] = (float((v <= 0).double().mean()), float(((v > 0) & (v < 20)).double().mean()),
                        float((v >= 20).double().mean()), v.numel())

    def conv(inp, e_in, w, b, p):
        w, b = w.to(F64), b.to(F64)
        if 'drop_tap' in WRONG and w.shape[-1] == 3:
            w = w.clone(); w[:, :, 0, 2] = 0.0
        acc = Fn.conv2d(inp, w, padding=p) + b[None, :, None, None]
        mag = Fn.conv2d(inp.abs(), w.abs(), padding=p) + b.abs()[None, :, None, None]
        return acc, c * mag + Fn.conv2d(e_in, w.abs(), padding=p)

    def crop(v, k):
        return v[:, :, k:-k, k:-k] if halo else v

    a1, e1 = conv(X, torch.zeros_like(X), lw['w1'][:, :, None, None], lw['b1'], 0)
    note('conv1', a1)
    t1 = ht(a1)
    aa, ea = conv(t1[:, :width], e1[:, :width], lw['wa'], lw['ba'], pad)
    note('convs.0', aa)
    y0 = ht(aa)
    sp = y0 + crop(t1[:, width:], 1)
    esp = ea + crop(e1[:, width:], 1)
    ab, eb = conv(sp, esp, lw['wb'], lw['bb'], pad)
    note('convs.1', ab)
    y1 = ht(ab)
    cat = torch.cat([crop(y0, 1), y1], 1)
    ecat = torch.cat([crop(ea, 1), eb], 1)
    a3, e3 = conv(cat, ecat, lw['w3'][:, :, None, None], lw['b3'], 0)
    Xc = crop(X, 2)
    if proj:
        wp = lw['wp'].to(F64)[:, :, None, None]
        a3 = a3 + Fn.conv2d(Xc, wp)
        e3 = e3 + c * Fn.conv2d(Xc.abs(), wp.abs())
    elif 'no_res' not in WRONG:
        a3 = a3 + Xc
        e3 = e3 + c * Xc.abs()
    note('conv3', a3)
    out = ht(a3)
    return dict(out=out.permute(0, 2, 3, 1), err=(e3 + 4 * 2.0 ** -24 * out).permute(0, 2, 3, 1), clamped=shares)


# ------------------------------------------------------------------ exact ops
def split_f16(w):
    """hi = float16(w) (round to nearest even), lo = float16((w - hi) * 2^11), as bit patterns"""
    import numpy as np
    v = w.numpy().astype(np.float32)
    hi = v.astype(np.float16)
    scale = np.float32(1024.0 if 'lo_2_10' in WRONG else 2048.0)
    lo = ((v - hi.astype(np.float32)) * scale).astype(np.float16)
    return torch.from_numpy(hi.view(np.int16).copy()), torch.from_numpy(lo.view(np.int16).copy())
