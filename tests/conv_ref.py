"""TEST INFRASTRUCTURE: float64 reference of the ConvDesc contract (csrc/common.h), written
from the contract's text and independent of both libspk_hip.so and the host emulation.

    out[m, n] = epi( sum_k A[m, k] * W[n, k] ),  m = (img, ho, wo)

A is gathered channels-last from s0 (stride, zero or 1-D reflect padding, dilation, the p2
addend, the BN-ReLU pre-activation on in-bounds values, vlen) followed by the K-concatenated
1x1 operand s1.  The weights come in logical order, w0[n, tap, c] and w1[n, c]: the packed K
order (ConvDesc::kcb) is the caller's business.  The epilogue order is bias, rowbias, res,
then AFF or act, post affine, act2, gate, and last the rowlen mask.

Besides the expected output, reference() returns per element
    mag = sum_k |A[m,k] W[n,k]| + |bias| + |rowbias| + |res|
and L, the Lipschitz constant of the epilogue with respect to the accumulator, so that a
kernel's rounding error is bounded by c * mag * L."""
import torch

ACT_NONE, ACT_RELU, ACT_HTANH, ACT_SILU, ACT_SIGMOID, ACT_TANH = range(6)
# Lipschitz constants of the activations (SiLU's derivative peaks at 1.0998)
ACT_LIP = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_HTANH: 1.0, ACT_SILU: 1.1, ACT_SIGMOID: 0.25, ACT_TANH: 1.0}
TRANSCENDENTAL = (ACT_SILU, ACT_SIGMOID, ACT_TANH)

F64 = torch.float64


def act(v, a):
    if a == ACT_RELU:
        return v.clamp(min=0.0)
    if a == ACT_HTANH:
        return v.clamp(0.0, 20.0)
    if a == ACT_SILU:
        return v * torch.sigmoid(v)
    if a == ACT_SIGMOID:
        return torch.sigmoid(v)
    if a == ACT_TANH:
        return torch.tanh(v)
    return v


def out_geometry(s, H, W):
    """(Ho, Wo) of a source dict with kh, kw, sh, sw, ph, pw, dh, dw."""
    Ho = (H + 2 * s['ph'] - s['dh'] * (s['kh'] - 1) - 1) // s['sh'] + 1
    Wo = (W + 2 * s['pw'] - s['dw'] * (s['kw'] - 1) - 1) // s['sw'] + 1
    return Ho, Wo


def _plane(x, cin):
    """[nimg, H, W, ld] fp32 -> [nimg*H*W, cin] float64"""
    return x[..., :cin].reshape(-1, cin).to(F64)


def gather_rows(g, t, rows):
    """A[rows, K] in float64 for output rows `rows` (a LongTensor of m indices)."""
    s0 = g['s0']
    H, W, cin = s0['H'], s0['W'], s0['cin']
    Ho, Wo = g['Ho'], g['Wo']
    wo = rows % Wo
    ho = (rows // Wo) % Ho
    img = rows // (Wo * Ho)
    X = _plane(t['x'], cin)
    if t.get('x2') is not None:
        X = X + _plane(t['x2'], cin)
    if t.get('pre_scale') is not None:
        X = (X * t['pre_scale'][:cin].to(F64) + t['pre_shift'][:cin].to(F64)).clamp(min=0.0)
    vlen = None if t.get('vlen') is None else t['vlen'].long()[img]
    cols = []
    for ky in range(s0['kh']):
        for kx in range(s0['kw']):
            hi = ho * s0['sh'] - s0['ph'] + ky * s0['dh']
            wi = wo * s0['sw'] - s0['pw'] + kx * s0['dw']
            if s0.get('reflect'):
                hi = torch.where(hi < 0, -hi, torch.where(hi >= H, 2 * H - 2 - hi, hi))
                wi = torch.where(wi < 0, -wi, torch.where(wi >= W, 2 * W - 2 - wi, wi))
            ok = (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
            if vlen is not None:
                ok = ok & (wi < vlen)
            pix = (img * H + hi.clamp(0, H - 1)) * W + wi.clamp(0, W - 1)
            cols.append(X[pix] * ok.to(F64)[:, None])
    if t.get('xs1') is not None:
        s1 = g['s1']
        pix = (img * s1['H'] + ho * s1['sh']) * s1['W'] + wo * s1['sw']
        cols.append(_plane(t['xs1'], s1['cin'])[pix])
    return torch.cat(cols, dim=1)


def reference(g, t, chunk=16384):
    """g: geometry dict (nimg, Ho, Wo, N, act, act2, gate_seg, s0{...}, s1{...}); t: host
    tensors.  Returns dict(out, mag, L, masked) -- out / mag / L are [M, N] float64, masked is
    a bool [M] (rows the rowlen mask zeroes)."""
    N = g['N']
    Ho, Wo = g['Ho'], g['Wo']
    M = g['nimg'] * Ho * Wo
    Wm = t['w0'][:N].reshape(N, -1).to(F64)
    if t.get('w1') is not None:
        Wm = torch.cat([Wm, t['w1'][:N].to(F64)], dim=1)
    Wt, Wa = Wm.t().contiguous(), Wm.abs().t().contiguous()
    acc = torch.empty(M, N, dtype=F64)
    mag = torch.empty(M, N, dtype=F64)
    for m0 in range(0, M, chunk):
        rows = torch.arange(m0, min(M, m0 + chunk))
        A = gather_rows(g, t, rows)
        acc[m0:m0 + len(rows)] = A @ Wt
        mag[m0:m0 + len(rows)] = A.abs() @ Wa
    m = torch.arange(M)
    img = m // (Ho * Wo)
    wo = m % Wo
    v = acc
    if t.get('bias') is not None:
        b = t['bias'][:N].to(F64)
        v = v + b
        mag += b.abs()
    if t.get('rowbias') is not None:
        rb = t['rowbias'][:, :N].to(F64)[img]
        v = v + rb
        mag += rb.abs()
    if t.get('res') is not None:
        r = t['res'].reshape(M, -1)[:, :N].to(F64)
        v = v + r
        mag += r.abs()
    if t.get('affx') is not None:
        ax = t['affx'].reshape(M, -1)[:, :N].to(F64)
        ay = t['affy'].reshape(M, -1)[:, :N].to(F64)
        th = 1.0 + torch.tanh(v)
        out = ax * th + ay * (2.0 - th)
        L = ax.abs() + ay.abs()
    else:
        L = torch.full((M, N), ACT_LIP[g.get('act', 0)], dtype=F64)
        out = act(v, g.get('act', 0))
        if t.get('post_scale') is not None:
            ps = t['post_scale'][:N].to(F64)
            out = out * ps + t['post_shift'][:N].to(F64)
            L = L * ps.abs()
        out = act(out, g.get('act2', 0))
        L = L * ACT_LIP[g.get('act2', 0)]
        if t.get('gate') is not None:
            gt = t['gate'][:, :, :N].to(F64)[img, wo // g['gate_seg']]
            out = out * gt
            L = L * gt.abs()
    masked = torch.zeros(M, dtype=torch.bool)
    if t.get('rowlen') is not None:
        masked = wo >= t['rowlen'].long()[img]
        out = torch.where(masked[:, None], torch.zeros_like(out), out)
    return dict(out=out, mag=mag, L=L, masked=masked)


def out_index(M, N, ldo, osplit, oplane):
    """Flat float index of every (m, n) in the output buffer (ConvDesc osplit / oplane)."""
    m = torch.arange(M)[:, None]
    n = torch.arange(N)[None, :]
    if osplit:
        return (n // osplit) * oplane + m * ldo + n % osplit
    return m * ldo + n
