"""Host side of the GPU resampler (csrc/resample_abi.cpp): the polyphase tap table built in
double, the output length and the error codes, checked without a GPU on the host build of the
executor (tests/emu) and on the built library; and the default path of load_audio / resample,
which the new ``device`` keyword must leave bit-identical."""
import ctypes
import math

import numpy as np
import pytest
import torch

import emu_runner
from speakerlab import _hip
from speakerlab.utils import fileio

PAIRS = [(8000, 16000), (16000, 8000), (44100, 16000), (22050, 16000), (48000, 16000), (16000, 44100),
         (44100, 48000)]
SPK_E_INVALID, SPK_E_UNSUPPORTED = -1, -6


@pytest.fixture(params=['emu', 'native'])
def lib(request):
    return emu_runner.lib() if request.param == 'emu' else _hip.lib()


def closed_formula_fp64(orig, new):
    """h[p][k] of the issue's closed formula in numpy fp64, and (n, K, w)."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    w = math.ceil(6 * o / base)
    K = 2 * w + o
    k = np.arange(K, dtype=np.float64)[None, :]
    p = np.arange(n, dtype=np.float64)[:, None]
    t = np.clip((k - w) / o - p / n, -6 / base, 6 / base) * base
    sinc = np.where(t == 0, 1.0, np.sin(np.pi * t) / np.where(t == 0, 1.0, np.pi * t))
    return sinc * np.cos(np.pi * t / 12) ** 2 * base / o, n, K, w


def query(lib, orig, new, with_taps=True):
    n, K, w = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = lib.spk_resample_taps(orig, new, ctypes.byref(n), ctypes.byref(K), ctypes.byref(w), None, 0)
    if rc != 0 or not with_taps:
        return rc, n.value, K.value, w.value, None
    taps = np.full((n.value, K.value), np.nan, dtype=np.float32)
    rc = lib.spk_resample_taps(orig, new, ctypes.byref(n), ctypes.byref(K), ctypes.byref(w), taps.ctypes.data, taps.size)
    return rc, n.value, K.value, w.value, taps


@pytest.mark.parametrize('orig,new', PAIRS)
def test_tap_table_matches_closed_formula(lib, orig, new):
    ref, n, K, w = closed_formula_fp64(orig, new)
    # sizes only
    rc, qn, qK, qw, _ = query(lib, orig, new, with_taps=False)
    assert (rc, qn, qK, qw) == (0, n, K, w)
    rc, qn, qK, qw, taps = query(lib, orig, new)
    assert (rc, qn, qK, qw) == (0, n, K, w)
    ref32 = ref.astype(np.float32)
    # one fp32 ulp: libm differences in the last double bit may move a tap across a rounding boundary
    ulp = np.spacing(np.maximum(np.abs(ref32), np.abs(taps)))
    assert np.all(np.abs(taps.astype(np.float64) - ref32.astype(np.float64)) <= ulp)
    # a buffer that is too short is refused, not overrun
    short = np.zeros(n * K - 1, dtype=np.float32)
    assert lib.spk_resample_taps(orig, new, None, None, None, short.ctypes.data, short.size) == SPK_E_INVALID


@pytest.mark.parametrize('orig,new', PAIRS)
def test_out_len(lib, orig, new):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    for L in (0, 1, 5, 999, 4410, 4801):
        v = ctypes.c_int64(-1)
        assert lib.spk_resample_out_len(L, orig, new, ctypes.byref(v)) == 0
        assert v.value == -(-n * L // o)


def test_error_codes(lib):
    assert query(lib, 16000, 16000)[0] == SPK_E_INVALID
    assert b'equal' in lib.spk_last_error()
    assert query(lib, 0, 16000)[0] == SPK_E_INVALID
    assert query(lib, 16000, -8000)[0] == SPK_E_INVALID
    assert query(lib, 44101, 16000)[0] == SPK_E_UNSUPPORTED      # 16000 x 44135 taps: above the 8 MiB cap
    assert b'cap' in lib.spk_last_error()
    v = ctypes.c_int64(-1)
    assert lib.spk_resample_out_len(10, 0, 16000, ctypes.byref(v)) == SPK_E_INVALID
    assert lib.spk_resample_out_len(-1, 8000, 16000, ctypes.byref(v)) == SPK_E_INVALID
    # the same through the device entry: refused before anything touches a GPU
    assert lib.spk_resample_f32(None, None, 0, 16000, 16000, None, None, None) == SPK_E_INVALID
    assert lib.spk_resample_f32(None, None, 0, 44101, 16000, None, None, None) == SPK_E_UNSUPPORTED


def test_python_out_len_and_error_code():
    assert _hip.resample_out_len(4410, 44100, 16000) == 1600
    assert _hip.resample_out_len(4801, 48000, 16000) == 1601
    with pytest.raises(_hip.HipError) as e:
        _hip.resample_out_len(10, 0, 16000)
    assert e.value.code == SPK_E_INVALID


def test_load_audio_default_path_unchanged(tmp_path):
    """device=None is today's host path, bit for bit (44.1 kHz file; the expected value is the
    strided conv1d of the fp32 kernel, written out here independently of resample())."""
    rng = np.random.default_rng(7)
    path = str(tmp_path / 'a.wav')
    fileio.write_wav(path, rng.uniform(-0.5, 0.5, 4410), fs=44100)
    wav, fs = fileio.read_wav(path)
    kernel, width = fileio.sinc_resample_kernel(44100, 16000, 100)
    x = torch.nn.functional.pad(wav.mean(dim=0, keepdim=True), (width, width + 441))
    want = torch.nn.functional.conv1d(x[:, None], kernel, stride=441).transpose(1, 2).reshape(1, -1)[:, :1600]
    for got in (fileio.load_audio(path, obj_fs=16000), fileio.load_audio(path, None, 16000, device=None),
                fileio.load_audio(wav[0].numpy(), 44100, 16000, device=None)):
        assert got.dtype == torch.float32 and got.device.type == 'cpu' and got.shape == (1, 1600)
        assert torch.equal(got, want)
    assert torch.equal(fileio.resample(wav, 44100, 16000, device=None), fileio.resample(wav, 44100, 16000))
