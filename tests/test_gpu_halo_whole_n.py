"""The whole-N form of the fp16x3 halo kernel (csrc/conv3x3_halo.hip, 52 -> 52 channels, lean
epilogue: one block computes all 52 output channels from one staged halo), through the entry
point, float64 reference, tolerance and out-of-bounds sentinel check of test_gpu_conv_kernels.py
(conv_cases.run_case: every output element against conv_ref at c = C_X3, nothing written outside
the (m, n) elements of an ldo = N + 4 buffer).  Also: operands next to the synthesised padding
lanes, independence of the grid size (bit equality) and the routes."""
import re

import pytest
import torch

import conv_cases
from conv_ref import ACT_NONE
from speakerlab import _hip

pytestmark = pytest.mark.gpu

# below one tile; one column past every tile width; tile width 16; tile width 32; 280 tiles: more
# than one per block on 256 CUs (the persistent loop and the cross-tile prefetch)
GEO = [(3, 5, 7), (2, 9, 33), (1, 40, 99), (2, 20, 50), (8, 40, 99)]
_BASE = conv_cases.BY_NAME['halo_x3_52to52_g0_plain']   # 52 -> 52, 3x3, bias, Hardtanh


def _name(add, tw=r'\d+', ks=3, lean=1, cin=52):
    return rf'conv3x3_halo_x3_kernel<{cin}, {tw}, {"true" if add else "false"}, 128, {ks}, {"true" if lean else "false"}, 1>'


def _case(name, geo, add, cin_real, **kw):
    nimg, h, w = geo
    return dict(_BASE, name=name, nimg=nimg, H=h, W=w, add=add, cin_real=cin_real, flag=0,
                expect=_name(add, conv_cases.HALO_TW[(h, w)]), **kw)


CASES = [_case(f'whole_n_{h}x{w}x{nimg}_add{add}_c{creal}', (nimg, h, w), add, creal)
         for (nimg, h, w) in GEO for add in (0, 1) for creal in (52, 50)]


@pytest.fixture(autouse=True)
def default_route(monkeypatch):
    monkeypatch.delenv('SPK_HALO_WHOLE_N', raising=False)   # read by the library at every launch
    monkeypatch.delenv('SPK_HALO_GRID_CAP', raising=False)


@pytest.fixture(scope='module')
def backend():
    dev = torch.device('cuda', 0)
    return conv_cases.Backend(_hip.lib(), dev, emu=False, cus=torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_against_fp64(backend, c):
    r = conv_cases.run_case(c, backend)
    assert re.fullmatch(_name(c['add']), r['kernel']), r['kernel']


@pytest.mark.parametrize('add', [0, 1])
def test_padding_lanes(backend, add, monkeypatch):
    """Input channels 52..63 and weight rows 52..63 do not exist in LDS: their lanes read other
    rows (clamped) or zero blocks.  Values near 1e4 in the last real channels (50, 51: the k-block
    that ends in the zero channels 52..55, next to the absent one) and in the last output
    channels' weights make any product with a wrong lane exceed the bound by orders of magnitude;
    no activation, so nothing is clipped.  run_case also checks that the columns past 52 of the
    ldo = 56 output buffer still hold the sentinel."""
    build = conv_cases.build

    def big(c, cus=256):
        g, t = build(c, cus)
        gen = torch.Generator().manual_seed(7)
        for k in ('x', 'x2'):
            if k in t:
                t[k][..., 50:52] = 1e4 * (0.5 + 0.7 * torch.rand(t[k][..., 50:52].shape, generator=gen))
        t['w0'][:, :, 50:52] = 1e4 * (0.5 + 0.5 * torch.rand(t['w0'][:, :, 50:52].shape, generator=gen))
        t['w0'][48:52, :, :50] *= 1e4 / float(t['w0'][48:52, :, :50].abs().max())
        return g, t

    monkeypatch.setattr(conv_cases, 'build', big)
    c = _case(f'whole_n_padding_add{add}', (2, 9, 33), add, 52, act=ACT_NONE)
    r = conv_cases.run_case(c, backend)
    assert re.fullmatch(_name(add), r['kernel']), r['kernel']


def _launch_raw(c, backend):
    g, t = conv_cases.build(c, backend.cus)
    keep = []
    d, out, _, _ = conv_cases.descriptor(c, g, t, backend, keep)
    rc, kernel, err = conv_cases.conv_diag.launch(backend.handle, d)
    torch.cuda.synchronize()
    assert rc == 0, err
    return kernel, out.cpu()


@pytest.mark.parametrize('add', [0, 1])
def test_grid_independence(backend, add, monkeypatch):
    """280 tiles on 8 blocks (35 tiles each) and on the default grid: the same bits."""
    c = _case(f'whole_n_grid_add{add}', (8, 40, 99), add, 52)
    k0, full = _launch_raw(c, backend)
    monkeypatch.setenv('SPK_HALO_GRID_CAP', '8')
    k1, capped = _launch_raw(c, backend)
    assert re.fullmatch(_name(add, 16), k0) and k1 == k0
    assert bool((full != conv_cases.SENTINEL).any())
    assert torch.equal(full, capped)


def test_routes(backend, monkeypatch):
    geo = (3, 5, 7)
    for add in (0, 1):
        c = _case(f'whole_n_route_add{add}', geo, add, 52)
        assert re.fullmatch(_name(add, 8, ks=3), _launch_raw(c, backend)[0])
    # a residual, and 64 -> 64: the sliced form
    res = dict(conv_cases.BY_NAME['halo_x3_52to52_res'], name='whole_n_route_res')
    assert re.fullmatch(_name(0, r'\d+', ks=2, lean=0), _launch_raw(res, backend)[0])
    c64 = dict(conv_cases.BY_NAME['halo_x3_64to64_g0_plain'], name='whole_n_route_64')
    assert re.fullmatch(_name(0, r'\d+', ks=2, cin=64), _launch_raw(c64, backend)[0])
    # the A/B switch: back on the sliced form, and still right
    monkeypatch.setenv('SPK_HALO_WHOLE_N', '0')
    for add in (0, 1):
        c = _case(f'whole_n_route_off_add{add}', geo, add, 52)
        c['expect'] = _name(add, 8, ks=2)
        r = conv_cases.run_case(c, backend)
        assert re.fullmatch(_name(add, 8, ks=2), r['kernel']), r['kernel']
