"""GPU windowed-sinc resampler (csrc/resample.hip, spk_resample_f32) and its way into ingest:
_hip.resample, fileio.resample / load_audio (device=...), infer_sv_batch --resample_device gpu,
Diarization3Dspeaker(gpu_resample=True).

Reference: the fp64 direct formula (its own copy below).  Bound per output j, derived, not
measured: the kernel's taps are the exact taps rounded once to fp32 (relative error 2^-24) and
an output is one fp32 FMA chain of at most K terms (K roundings of partial sums that never
exceed sum |x h| (1 + small)), so |y[j] - ref[j]| <= (K + 2) 2^-24 sum_k |x_k h_k|.
Measured on MI355X (max over outputs of |y - ref| / bound): see DESIGN.md §7 'GPU resampler'."""
import math

import numpy as np
import pytest
import torch

from speakerlab import _hip
from speakerlab.utils import fileio, synthetic
from speakerlab.utils.fileio import write_wav

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def direct_fp64(x, orig, new):
    """(y, sum |x h|, K): y[j] = sum_i x[i] h(i/o - j/n) over output j's K-tap window, fp64."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    w = math.ceil(6 * o / base)
    K = 2 * w + o
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    xp = np.concatenate([np.zeros(w), x, np.zeros(w + o)])
    M = -(-n * L // o)
    y, mag = np.zeros(M), np.zeros(M)
    k = np.arange(K)
    for p in range(min(n, M)):
        t = np.clip(((k - w) / o - p / n) * base, -6, 6)
        h = np.where(t == 0, 1.0, np.sin(np.pi * t) / np.where(t == 0, 1.0, np.pi * t)) * np.cos(t * np.pi / 12) ** 2
        h *= base / o
        bs = np.arange(p, M, n) // n
        win = xp[bs[:, None] * o + k[None, :]]          # x[b o - w + k], zero outside [0, L)
        y[p::n] = win @ h
        mag[p::n] = np.abs(win) @ np.abs(h)
    return y, mag, K


def check_bound(y, x, orig, new, what=''):
    ref, mag, K = direct_fp64(x, orig, new)
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    if len(ref) == 0:
        return
    err = np.abs(y - ref)
    bound = (K + 2) * 2.0 ** -24 * mag
    print(f'resample {orig}->{new} L={len(x)} {what}: max |y-ref| {err.max():.3e}, '
          f'max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
    assert np.all(err <= bound)
    # the bound of the host fp32 path this stands in for (tests/test_resample.py)
    assert err.max() < 2e-4 * max(1.0, np.abs(ref).max())


def randn(L, seed):
    return np.random.default_rng(seed).standard_normal(L).astype(np.float32)


def gpu(x, orig, new):
    return _hip.resample(torch.from_numpy(x).to(DEV), orig, new).cpu().numpy()


# the pairs / lengths of tests/test_resample.py and an upsampling to 44.1 kHz; then more than one
# tile (and workgroup slice) per utterance, and rate pairs whose table or input span is too
# large for LDS (resample.hip's direct kernel)
CASES = [(8000, 16000, 1000), (44100, 16000, 4410), (16000, 8000, 999), (22050, 16000, 2205), (48000, 16000, 4801),
         (16000, 44100, 800),
         (44100, 16000, 30001), (48000, 16000, 40000), (11025, 16000, 3001),
         (3000, 601, 6001), (44100, 1000, 4410)]


@pytest.mark.parametrize('orig,new,L', CASES)
def test_bound_against_fp64_formula(orig, new, L):
    x = randn(L, orig + L)
    y = gpu(x, orig, new)
    assert len(y) == _hip.resample_out_len(L, orig, new)
    check_bound(y, x, orig, new)
    assert np.array_equal(y, gpu(x, orig, new))          # run to run


def test_ragged_batch_is_bit_identical_and_stays_in_bounds():
    orig, new, G = 44100, 16000, 64
    lens = [4410, 5, 1, 2000, 0]
    xs = [randn(L, 100 + i) for i, L in enumerate(lens)]
    solo = [gpu(x, orig, new) for x in xs]
    outs = [_hip.resample_out_len(L, orig, new) for L in lens]
    assert [len(s) for s in solo] == outs and outs[-1] == 0
    # input: 1e30 in front of the first and behind the last utterance; output: NaN everywhere
    guard = np.full(G, 1e30, dtype=np.float32)
    wav = torch.from_numpy(np.concatenate([guard] + xs + [guard])).to(DEV)
    out = torch.full((2 * G + sum(outs),), float('nan'), dtype=torch.float32, device=DEV)
    in_off = G + np.concatenate([[0], np.cumsum(lens)])
    out_off = G + np.concatenate([[0], np.cumsum(outs)])
    offs = torch.tensor(np.stack([in_off, out_off]), dtype=torch.int64, device=DEV)
    rc = _hip.lib().spk_resample_f32(wav.data_ptr(), offs[0].data_ptr(), len(lens), orig, new, out.data_ptr(),
                                     offs[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _hip.lib().spk_last_error()
    got = out.cpu().numpy()
    assert np.isnan(got[:G]).all() and np.isnan(got[G + sum(outs):]).all()
    body = got[G:G + sum(outs)]
    assert np.isfinite(body).all() and np.abs(body).max() < 100.0     # nothing read across an edge
    for u in range(len(lens)):
        assert np.array_equal(got[out_off[u]:out_off[u + 1]], solo[u]), u
    # the Python ragged forms: list in, list of views out; [B, L] with lengths
    res = _hip.resample([torch.from_numpy(x).to(DEV) for x in xs], orig, new)
    assert [tuple(r.shape) for r in res] == [(m,) for m in outs]
    for u in range(len(lens)):
        assert np.array_equal(res[u].cpu().numpy(), solo[u])
    pad = torch.zeros(len(lens), max(lens))
    for u, x in enumerate(xs):
        pad[u, :len(x)] = torch.from_numpy(x)
    res = _hip.resample(pad.to(DEV), orig, new, lengths=lens)
    for u in range(len(lens)):
        assert np.array_equal(res[u].cpu().numpy(), solo[u])


def test_known_answers():
    # an impulse at input sample 40 (8 kHz) gives the windowed sinc centred at output 80
    x = np.zeros(200, dtype=np.float32)
    x[40] = 1.0
    y = gpu(x, 8000, 16000)
    j = np.arange(len(y))
    t = np.clip((40 / 1 - j / 2) * 0.99, -6, 6)
    h = np.where(t == 0, 1.0, np.sin(np.pi * t) / np.where(t == 0, 1, np.pi * t)) * np.cos(t * np.pi / 12) ** 2 * 0.99
    assert np.abs(y - h).max() < 1e-6
    assert y.argmax() == 80
    # DC passes within 2e-3 in the interior
    y = gpu(np.ones(2000, dtype=np.float32), 8000, 16000)[100:-100]
    assert np.all(np.abs(y - 1) < 2e-3)


def test_non_default_stream_and_two_cached_tables():
    x1, x2 = randn(2205, 1), randn(999, 2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = _hip.resample(torch.from_numpy(x1).to(DEV), 22050, 16000)
        b = _hip.resample(torch.from_numpy(x2).to(DEV), 16000, 8000)
        c = _hip.resample(torch.from_numpy(x1).to(DEV), 22050, 16000)     # the first table again
    s.synchronize()
    check_bound(a.cpu().numpy(), x1, 22050, 16000, 'stream')
    check_bound(b.cpu().numpy(), x2, 16000, 8000, 'stream')
    assert torch.equal(a, c)


def test_2d_form_equals_ragged_form():
    x = torch.from_numpy(randn(3 * 1470, 5).reshape(3, 1470)).to(DEV)
    y = _hip.resample(x, 44100, 48000)
    assert y.shape == (3, 1600) and y.dtype == torch.float32 and y.device.type == 'cuda'
    rows = _hip.resample([x[i] for i in range(3)], 44100, 48000)
    for i in range(3):
        assert torch.equal(y[i], rows[i])
    assert torch.equal(_hip.resample(x[1], 44100, 48000), y[1])
    check_bound(y[2].cpu().numpy(), x[2].cpu().numpy(), 44100, 48000, '2-D')
    with pytest.raises(_hip.HipError):
        _hip.resample(x, 16000, 16000)
    with pytest.raises(_hip.HipError):
        _hip.resample(x.cpu(), 44100, 16000)


def test_over_cap_pair(monkeypatch):
    x = torch.from_numpy(randn(500, 9))
    with pytest.raises(_hip.HipError) as e:
        _hip.resample(x.to(DEV), 44101, 16000)
    assert e.value.code == _hip.E_UNSUPPORTED
    # fileio.resample(device='cuda') takes the host path for it.  The host kernel of this pair is
    # 16000 x 44135 floats (2.8 GB), so the host path is only shown to be entered here ...
    class Entered(Exception):
        pass

    def spy(orig_freq, new_freq, *a, **k):
        raise Entered((orig_freq, new_freq))
    with monkeypatch.context() as m:
        m.setattr(fileio, 'sinc_resample_kernel', spy)
        with pytest.raises(Entered):
            fileio.resample(x, 44101, 16000, device=DEV)
    # ... and its result compared on an over-cap pair with a small host kernel (1999 x 2017 taps, 16 MB)
    with pytest.raises(_hip.HipError) as e:
        _hip.resample(x.to(DEV), 2003, 1999)
    assert e.value.code == _hip.E_UNSUPPORTED
    got = fileio.resample(x, 2003, 1999, device=DEV)
    assert got.device.type == 'cpu' and torch.equal(got, fileio.resample(x, 2003, 1999))


def test_load_audio_on_device(tmp_path):
    path = str(tmp_path / 'a.wav')
    write_wav(path, np.random.default_rng(3).uniform(-0.5, 0.5, 22050), fs=44100)
    wav = fileio.load_audio(path, obj_fs=16000, device=DEV)
    assert wav.device.type == 'cpu' and wav.dtype == torch.float32 and wav.shape == (1, 8000)
    decoded, fs = fileio.read_wav(path)
    assert fs == 44100
    check_bound(wav[0].numpy(), decoded.mean(dim=0).numpy(), 44100, 16000, 'load_audio')
    # the array form, and the host path next to it
    host = fileio.load_audio(path, obj_fs=16000)
    assert np.abs(wav - host).max() < 2e-4
    arr = fileio.load_audio(decoded[0].numpy(), 44100, 16000, device=DEV)
    assert torch.equal(arr, wav)


def test_infer_sv_batch_resample_device(tmp_path):
    from speakerlab.bin import infer_sv_batch as isb
    model_id = 'iic/speech_campplus_sv_zh-cn_16k-common'
    paths = []
    for name, fs, sec in (('tel', 8000, 1.5), ('studio', 44100, 1.2), ('plain', 16000, 1.0)):
        p = tmp_path / f'{name}.wav'
        sig = synthetic.synth_wav(int(sec * 16000), seed=11 + len(paths))
        # the 16 kHz synthetic signal played at fs: a test signal, not a rate conversion
        write_wav(str(p), sig[:int(sec * fs)] if fs <= 16000 else np.resize(sig, int(sec * fs)), fs=fs)
        paths.append(str(p))
    lst = tmp_path / 'wav.list'
    lst.write_text('\n'.join(paths) + '\n')
    embs = {}
    for mode in ('gpu', 'host'):
        out_dir = tmp_path / mode
        isb.main(['--model_id', model_id, '--wavs', str(lst), '--feat_out_dir', str(out_dir), '--synthetic_weights',
                  '--batch_size', '8', '--diable_progress_bar', '--nprocs', '1', '--resample_non16k',
                  '--resample_device', mode])
        embs[mode] = {n: np.load(out_dir / f'{n}.npy') for n in ('tel', 'studio', 'plain')}     # none skipped
        for e in embs[mode].values():
            assert e.shape == (192,) and np.isfinite(e).all()
    # 16 kHz files do not pass through the resampler: same chunks, same embedding
    assert np.allclose(embs['gpu']['plain'], embs['host']['plain'], rtol=0, atol=1e-6)
    # the chunk tensors of the two settings
    items = [isb.load_wav_native(p) for p in paths[:2]]
    assert all(isinstance(it, isb.NativeRateWav) for it in items)
    got = isb.gpu_resample_chunks(items, torch.device(DEV))
    for p, it, g in zip(paths, items, got):
        want = isb.load_wav_chunks(p, resample_other_rates=True)
        assert g.device.type == 'cuda' and tuple(g.shape) == tuple(want.shape) == (it.n_chunks, 160000)
        assert (g.cpu() - want).abs().max() < 2e-4 * max(1.0, float(want.abs().max()))
    # without the new option: today's behaviour
    with pytest.raises(isb.SampleRateSkip):
        isb.load_wav_chunks(paths[0])
    assert isinstance(isb.load_wav_native(paths[2]), torch.Tensor)


def test_diarization_gpu_resample(tmp_path):
    """Same segments with and without gpu_resample on an 8 kHz two-speaker recording.  The segment
    boundaries come from the energy VAD's 16 ms flags (a threshold on frame log energy); the two
    resamplers differ by ~1e-5 relative, i.e. ~1e-4 dB per frame, and the signal is checked below
    to keep every frame at least 0.01 dB (a hundred times that) away from the threshold, so no flag
    can flip."""
    from speakerlab.bin import infer_diarization as idz
    wav16, _ = synthetic.synth_meeting(6.0, 2, seed=3)
    wav8 = wav16[::2].copy()                      # 6 s at 8 kHz (a test signal: aliasing is irrelevant)
    p = tmp_path / 'tel.wav'
    write_wav(str(p), wav8, fs=8000)
    host = fileio.load_audio(str(p), obj_fs=16000)
    fr = np.clip(host[0].numpy(), -1, 1)[:len(host[0]) // 256 * 256].reshape(-1, 256).astype(np.float64)
    db = 10 * np.log10(np.mean(fr ** 2, axis=1) + 1e-12)
    assert np.abs(db - max(np.percentile(db, 95) - 25.0, -60.0)).min() > 0.01
    a = idz.Diarization3Dspeaker(DEV, synthetic_weights=True, vad='energy', gpu_resample=False)
    b = idz.Diarization3Dspeaker(DEV, synthetic_weights=True, vad='energy', gpu_resample=True)
    assert a.resample_device is None and b.resample_device == b.device
    seg_a, seg_b = a(str(p)), b(str(p))
    assert len(seg_a) >= 1 and seg_a == seg_b
    assert idz.parser.parse_args(['--wav', 'x.wav', '--out_dir', 'o', '--gpu_resample']).gpu_resample
