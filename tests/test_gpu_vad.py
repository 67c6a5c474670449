"""Device VAD front end (csrc/vad.hip: spk_vad_energy_f32, spk_vad_apply_intervals_f32) and its
way into the pipeline: _hip.vad_energy / vad_apply_intervals, Diarization3Dspeaker(gpu_vad=True),
infer_diarization.py --gpu_vad.

Bounds: e16 within 4 ulp of numpy's fp64 mean (summation order is the only freedom); e20 within
2^-23 relative of the fp64 mean (two fp32 roundings: the sum, the division).  On audio quantised to
multiples of 2^-7 every sum is exact in fp32 and fp64 alike (tests/test_vad_front_host.py
test_device_arithmetic_on_grid_audio), so there the device tracks, and everything the pipeline
derives from them, must equal the host's to the bit."""
import numpy as np
import pytest
import torch

from speakerlab import _hip
from speakerlab.bin import infer_diarization as idz
from speakerlab.utils import synthetic, vad_post

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# 70001 crosses six of the kernel's 10240-sample tiles and ends 17 samples into a block of 32;
# 10240 / 10400 / 20481 sit on and next to a tile boundary and its one-hop look-ahead
LENGTHS = [0, 100, 255, 256, 257, 319, 320, 321, 479, 480, 16161, 70001, 10240, 10400, 20481]


def _loud(n, seed=7):
    """synth_wav scaled by 1.5.  Its peak is about 0.52, which 1.5 alone would leave below the
    clip, so it is normalised to full scale first: the scaled signal then peaks at 1.5."""
    x = synthetic.synth_wav(max(n, 256), seed)
    return (x / np.abs(x).max() * 1.5).astype(np.float32)[:n]


def _grid(x):
    return np.clip(np.round(x * 128) / 128, -1, 1).astype(np.float32)


def _ref_energies(x):
    c = np.clip(x, -1.0, 1.0).astype(np.float64)
    n16 = len(c) // 256
    e16 = np.mean(c[:n16 * 256].reshape(n16, 256) ** 2, axis=1)
    n20 = (len(c) - 320) // 160 + 1 if len(c) >= 320 else 0
    e20 = np.array([np.mean(c[j * 160:j * 160 + 320] ** 2) for j in range(n20)], dtype=np.float64)
    return e16, e20


def _host_en(x):
    n = (len(x) - 320) // 160 + 1
    if n <= 0:
        return np.zeros(0, np.float32)
    fr = np.lib.stride_tricks.sliding_window_view(x, 320)[::160][:n]
    return np.mean(fr ** 2, axis=1).astype(np.float32)


def _run(x):
    e16, e20 = _hip.vad_energy(torch.from_numpy(x).to(DEV))
    return e16.cpu().numpy(), e20.cpu().numpy()


@pytest.mark.parametrize('L', LENGTHS)
def test_energies_against_fp64(L):
    x = _loud(L)
    if L >= 10000:
        assert np.abs(x).max() > 1.0                      # the clip matters
    e16, e20 = _run(x)
    r16, r20 = _ref_energies(x)
    assert e16.dtype == np.float64 and e20.dtype == np.float32
    assert e16.shape == r16.shape == (_hip.vad_energy_sizes(L)[0],)
    assert e20.shape == r20.shape == (_hip.vad_energy_sizes(L)[1],)
    if len(r16):
        ulp = np.abs(e16 - r16) / np.spacing(r16)
        print(f'L={L}: e16 max {ulp.max():.2f} ulp', end='')
        assert ulp.max() <= 4
    if len(r20):
        rel = np.abs(e20.astype(np.float64) - r20) / r20
        print(f', e20 max rel {rel.max() * 2 ** 23:.3f} x 2^-23')
        assert np.all(np.abs(e20.astype(np.float64) - r20) <= 2.0 ** -23 * r20)


def test_ragged_batch_bits_and_sentinels():
    """One empty utterance, one of 100 samples, two at offsets that are no multiple of 32 (the
    second not even 16-byte aligned: the scalar loads), through the ABI with sentinel-filled
    outputs: every utterance has the bits it has alone and nothing else is written."""
    lens = [0, 100, 16161, 70001]
    xs = [_loud(n, seed=20 + i) for i, n in enumerate(lens)]
    pad = 5                                               # the batch starts 5 floats into its buffer
    flat = torch.zeros(pad + sum(lens) + 64, dtype=torch.float32)
    off, o16, o20 = [pad], [3], [7]                       # the declared ranges start inside the buffers
    for x in xs:
        flat[off[-1]:off[-1] + len(x)] = torch.from_numpy(x)
        n16, n20 = _hip.vad_energy_sizes(len(x))
        off.append(off[-1] + len(x))
        o16.append(o16[-1] + n16)
        o20.append(o20[-1] + n20)
    assert off[2] % 32 and off[3] % 32 and off[3] % 4
    flat = flat.to(DEV)
    offs = torch.tensor([off, o16, o20], dtype=torch.int64, device=DEV)
    e16 = torch.full((o16[-1] + 9,), -7.0, dtype=torch.float64, device=DEV)
    e20 = torch.full((o20[-1] + 9,), -7.0, dtype=torch.float32, device=DEV)
    rc = _hip.lib().spk_vad_energy_f32(flat.data_ptr(), offs[0].data_ptr(), len(lens), e16.data_ptr(),
                                       offs[1].data_ptr(), e20.data_ptr(), offs[2].data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    e16, e20 = e16.cpu().numpy(), e20.cpu().numpy()
    assert np.all(e16[:3] == -7) and np.all(e16[o16[-1]:] == -7)
    assert np.all(e20[:7] == -7) and np.all(e20[o20[-1]:] == -7)
    for i, x in enumerate(xs):
        a16, a20 = _run(x)                                # alone, at an aligned address
        np.testing.assert_array_equal(e16[o16[i]:o16[i + 1]], a16)
        np.testing.assert_array_equal(e20[o20[i]:o20[i + 1]], a20)
    # the list form of the binding: the same batch in one launch
    res = _hip.vad_energy([torch.from_numpy(x).to(DEV) for x in xs])
    for (b16, b20), x in zip(res, xs):
        a16, a20 = _run(x)
        np.testing.assert_array_equal(b16.cpu().numpy(), a16)
        np.testing.assert_array_equal(b20.cpu().numpy(), a20)


@pytest.mark.parametrize('L', [320, 16161, 70001])
def test_energies_on_grid_audio_bit_equal(L):
    x = _grid(_loud(L, seed=9))
    e16, e20 = _run(x)
    np.testing.assert_array_equal(e20, _host_en(x))
    np.testing.assert_array_equal(e16, idz.EnergyVad().frame_energy(x))
    fe, n = vad_post.frame_energy(x)
    np.testing.assert_array_equal(np.maximum.accumulate(e20), fe[:n * 160:160])


@pytest.mark.parametrize('L', [1000, 4096, 4097, 70001])
def test_apply_intervals(L):
    rng = np.random.default_rng(L)
    x = (rng.standard_normal(L) * 0.5).astype(np.float32)      # unclipped, as the pipeline passes it
    xd = torch.from_numpy(x).to(DEV)
    cases = {
        'none': [],
        'all': [[0, L]],
        'holes': [[0, 10], [11, 12], [13, L // 4], [L // 4 + 1, L // 2], [L // 2 + 1, L // 2 + 2]],
        'ends at L': [[5, 6], [L - 300, L]],
        'many': [[a, a + 1 + (a % 7)] for a in range(3, L - 10, 9)],
    }
    for name, iv in cases.items():
        want = vad_post.apply_mask(x, vad_post.intervals_to_mask(iv, L))
        got = _hip.vad_apply_intervals(xd, [a for a, _ in iv], [b for _, b in iv]).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=name)
    # an input that does not start on a 16-byte boundary
    got = _hip.vad_apply_intervals(xd[1:], [0, 50], [7, L - 1]).cpu().numpy()
    np.testing.assert_array_equal(got, vad_post.apply_mask(x[1:], vad_post.intervals_to_mask([[0, 7], [50, L - 1]], L - 1)))
    with pytest.raises(_hip.HipError):
        _hip.vad_apply_intervals(xd, [10, 5], [20, 8])
    with pytest.raises(_hip.HipError):
        _hip.vad_apply_intervals(xd, [0], [L + 1])


def test_front_on_grid_meeting():
    """do_front with gpu_vad against the host front on a 30 s meeting on the 2^-7 grid: every
    last_vad_* field and the chunks are equal.  (Off the grid the host's fp32 pairwise sums and
    the device's fp64 sums may differ in the last bit and an edge may move by a hop: DESIGN.md.)"""
    x = _grid(synthetic.synth_meeting(30, 3, seed=3)[0])
    a = idz.Diarization3Dspeaker(DEV, synthetic_weights=True, vad='energy', gpu_vad=False)
    b = idz.Diarization3Dspeaker(DEV, synthetic_weights=True, vad='energy', gpu_vad=True)
    chunks_a, wav_a = a.do_front(x)
    chunks_b, wav_b = b.do_front(x)
    assert len(chunks_a) > 10 and chunks_a == chunks_b
    assert wav_b.device.type == 'cuda' and wav_b.shape == wav_a.shape
    assert torch.equal(wav_b.cpu(), wav_a)
    assert a.last_vad_time_raw == b.last_vad_time_raw
    assert a.last_vad_time_processed == b.last_vad_time_processed
    assert a.last_vad_time == b.last_vad_time and len(a.last_vad_time) >= 2
    # built on first access only, then kept
    assert callable(vars(b)['last_vad_masked_audio_value'])
    m = b.last_vad_masked_audio
    assert m is b.last_vad_masked_audio and m.shape == a.last_vad_masked_audio.shape
    np.testing.assert_array_equal(m, a.last_vad_masked_audio)
    np.testing.assert_array_equal(b.last_vad_processed_mask, a.last_vad_processed_mask)
    np.testing.assert_array_equal(b.last_vad_refined_mask, a.last_vad_refined_mask)
    # and the embeddings read the device signal in place
    emb_a = a.do_emb_extraction(chunks_a[:4], wav_a)
    emb_b = b.do_emb_extraction(chunks_b[:4], wav_b)
    np.testing.assert_array_equal(emb_a, emb_b)


# ---------------------------------------------------------------------------------- CLI
def _write_grid_wav(path, wav, fs=16000):
    """int16 samples that are multiples of 256: read_wav divides by 32768, i.e. the 2^-7 grid."""
    from scipy.io import wavfile
    q = np.clip(np.round(wav * 128), -128, 127).astype(np.int16) * 256
    wavfile.write(str(path), fs, q)


BASE = ['--out_type', 'rttm', '--synthetic_weights', '--vad', 'energy', '--diable_progress_bar', '--nprocs', '1']


def _same_outputs(tmp_path, names, suffixes=('.rttm', '.vad_info.json', '.vad_masked.wav')):
    for n in names:
        for s in suffixes:
            host = (tmp_path / 'host' / (n + s)).read_bytes()
            assert len(host) > 0 and (tmp_path / 'gpu' / (n + s)).read_bytes() == host, n + s


def test_cli_gpu_vad_same_outputs(tmp_path):
    p = tmp_path / 'meet.wav'
    _write_grid_wav(p, synthetic.synth_meeting(12.0, 2, seed=5)[0])
    idz.main(BASE + ['--wav', str(p), '--out_dir', str(tmp_path / 'host')])
    idz.main(BASE + ['--wav', str(p), '--out_dir', str(tmp_path / 'gpu'), '--gpu_vad'])
    assert len((tmp_path / 'host' / 'meet.rttm').read_text().splitlines()) >= 1
    _same_outputs(tmp_path, ['meet'])


def test_cli_gpu_vad_with_batched_ahc(tmp_path):
    names = ['m1', 'm2']
    for i, n in enumerate(names):
        _write_grid_wav(tmp_path / (n + '.wav'), synthetic.synth_meeting(8.0 + 2 * i, 2, seed=6 + i)[0])
    lst = tmp_path / 'wavs.list'
    lst.write_text(''.join(f'{tmp_path / (n + ".wav")}\n' for n in names))
    args = BASE + ['--wav', str(lst), '--gpu_ahc', '--ahc_batch', '2']
    idz.main(args + ['--out_dir', str(tmp_path / 'host')])
    idz.main(args + ['--out_dir', str(tmp_path / 'gpu'), '--gpu_vad'])
    _same_outputs(tmp_path, names)


def test_cli_gpu_vad_with_gpu_resample(tmp_path):
    """An 8 kHz copy through --gpu_resample: the resampled signal stays on the device and is not on
    the grid (the CLI has no way to write it back onto it), so this test does NOT compare the RTTM
    byte for byte: it asserts that the run completes and that the number of segments is within one
    of the run without --gpu_vad."""
    p = tmp_path / 'tel.wav'
    _write_grid_wav(p, synthetic.synth_meeting(12.0, 2, seed=5)[0][::2].copy(), fs=8000)
    args = BASE + ['--wav', str(p), '--gpu_resample']
    idz.main(args + ['--out_dir', str(tmp_path / 'host')])
    idz.main(args + ['--out_dir', str(tmp_path / 'gpu'), '--gpu_vad'])
    host = (tmp_path / 'host' / 'tel.rttm').read_text().splitlines()
    got = (tmp_path / 'gpu' / 'tel.rttm').read_text().splitlines()
    assert len(host) >= 1 and abs(len(got) - len(host)) <= 1
    assert (tmp_path / 'gpu' / 'tel.vad_masked.wav').stat().st_size == (tmp_path / 'host' / 'tel.vad_masked.wav').stat().st_size


def test_keep_on_device(tmp_path):
    from speakerlab.utils import fileio
    x = torch.from_numpy(synthetic.synth_wav(8000, 1))
    host = fileio.load_audio(x, 8000, 16000, device=DEV)
    kept = fileio.load_audio(x, 8000, 16000, device=DEV, keep_on_device=True)
    assert host.device.type == 'cpu' and kept.device.type == 'cuda' and kept.shape == host.shape == (1, 16000)
    assert torch.equal(kept.cpu(), host)
    # nothing to resample, or no device: as without the flag
    assert fileio.load_audio(x, 16000, 16000, device=DEV, keep_on_device=True).device.type == 'cpu'
    assert fileio.load_audio(x, 8000, 16000, keep_on_device=True).device.type == 'cpu'
