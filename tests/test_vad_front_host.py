"""Host side of the device VAD front end (--gpu_vad), no GPU needed: vad_post.refine_intervals ==
the runs of vad_post.refine_boundaries, vad_post.segments_from_flags == the runs of flags_to_mask,
the EnergyVad split, spk_vad_energy_sizes through the ABI, and the numpy restatement of the device
arithmetic that licenses the exact comparisons of tests/test_gpu_vad.py."""
import ctypes

import numpy as np
import pytest

from speakerlab.bin import infer_diarization as idz
from speakerlab.utils import synthetic, vad_post

FS = 16000


def _markov_flags(n, seed, p_on=0.08, p_off=0.05):
    rng = np.random.default_rng(seed)
    out, state = np.zeros(n, dtype=np.int64), 0
    u = rng.random(n)
    for i in range(n):
        state = (u[i] < p_on) if state == 0 else (u[i] >= p_off)
        out[i] = state
    return out.tolist()


def _audio(n, seed, gain=1.0 / 32768.0):
    return np.clip(synthetic.synth_wav(n, seed) * gain, -1, 1).astype(np.float32)


def _hop_energies(a):
    """The ``en`` of vad_post.frame_energy (its hop values before the running maximum)."""
    n = (len(a) - 320) // 160 + 1
    if n <= 0:
        return np.zeros(0, dtype=np.float32)
    frames = np.lib.stride_tricks.sliding_window_view(a, 320)[::160][:n]
    return np.mean(frames ** 2, axis=1).astype(np.float32)


def _runs_of(mask):
    d = np.diff(np.concatenate(([0], mask, [0])))
    return [[s, e] for s, e in zip(np.where(d > 0)[0].tolist(), np.where(d < 0)[0].tolist())]


def _check_refine(a, mask, floor, exp_ms, pct):
    n = len(a)
    en = _hop_energies(a)
    # the hop values are frame_energy's: its per-sample track is their running maximum
    fe, k = vad_post.frame_energy(a)
    assert k == len(en) or (k <= 0 and len(en) == 0)
    if k > 0:
        np.testing.assert_array_equal(fe[:k * 160:160], np.maximum.accumulate(en))
    want = vad_post.refine_boundaries(a, mask, FS, floor, exp_ms, pct)
    got = vad_post.refine_intervals(en, n, _runs_of(mask), FS, floor, exp_ms, pct)
    np.testing.assert_array_equal(vad_post.intervals_to_mask(got, n), want)
    assert got == _runs_of(want)
    assert vad_post.intervals_to_seconds(got, FS) == vad_post.mask_to_intervals(want, FS)
    return got


GRID = [(10.0, 10.0, 0.05), (0.0, 30.0, 1e-4), (50.0, 5.0, 0.0)]


@pytest.mark.parametrize('seed', range(5))
@pytest.mark.parametrize('exp_ms,pct,floor', GRID)
def test_refine_intervals_grid(seed, exp_ms, pct, floor):
    """The grid of tests/test_diar_host.py::test_refine_boundaries."""
    n = 16000 * 20 + 123 * seed
    a = _audio(n, 10 + seed)
    proc = vad_post.post_process_speech_flags(_markov_flags(n // 256 + 1, seed))
    _check_refine(a, vad_post.flags_to_mask(proc, n, 256), floor, exp_ms, pct)


@pytest.mark.parametrize('seed', range(4))
@pytest.mark.parametrize('exp_ms,pct,floor', GRID + [(10.0, 50.0, 0.01), (3.0, 100.0, 0.0), (10.0, 0.0, 1e-3)])
def test_refine_intervals_loud(seed, exp_ms, pct, floor):
    """Full-scale audio, where the percentile (not the floor) sets the threshold and the
    contractions fire, with short flags so that many segments are shorter than the look window."""
    n = 16000 * 6 + 77 * seed
    a = _audio(n, 20 + seed, gain=1.0)
    flags = _markov_flags(n // 256 + 1, seed, p_on=0.2, p_off=0.15 + 0.1 * (seed % 2))
    _check_refine(a, vad_post.flags_to_mask(flags, n, 256), floor, exp_ms, pct)


@pytest.mark.parametrize('n', [100, 320, 321, 480, 16161])
@pytest.mark.parametrize('exp_ms,pct,floor', GRID)
def test_refine_intervals_short_audio(n, exp_ms, pct, floor):
    a = _audio(n, n, gain=1.0)
    for mask in (np.ones(n, np.float32), np.zeros(n, np.float32),
                 vad_post.flags_to_mask([0, 1, 1, 0, 1] * (n // 1280 + 1), n, 256)):
        _check_refine(a, mask, floor, exp_ms, pct)


@pytest.mark.parametrize('exp_ms,pct,floor', GRID + [(10.0, 10.0, 1e-3)])
def test_refine_intervals_cases(exp_ms, pct, floor):
    n = 16000 * 3 + 155                    # n20 = 299, E = 48000: a zero tail of 155 samples
    a = _audio(n, 5, gain=1.0)
    E = ((n - 320) // 160) * 160 + 320
    assert 0 < n - E < 160

    def mask_of(runs):
        return vad_post.intervals_to_mask(runs, n)

    # a segment ending at L covers the zero tail; one inside the tail only; one starting in the
    # look window in front of it
    _check_refine(a, mask_of([[1000, 9000], [30000, n]]), floor, exp_ms, pct)
    _check_refine(a, mask_of([[E + 3, n]]), floor, exp_ms, pct)
    _check_refine(a, mask_of([[E - 700, n]]), floor, exp_ms, pct)
    _check_refine(a, mask_of([[E - 700, E + 1]]), floor, exp_ms, pct)
    _check_refine(a, mask_of([[n - 1, n]]), floor, exp_ms, pct)
    # segments shorter than 100 ms, down to one and two samples
    _check_refine(a, mask_of([[5000, 5001], [6000, 6002], [7000, 7160], [9000, 10599], [12000, 13601]]),
                  floor, exp_ms, pct)
    # adjacent segments one frame apart
    _check_refine(a, mask_of([[2560, 5120], [5376, 7936], [8192, 8448]]), floor, exp_ms, pct)
    # all ones, all zeros
    got = _check_refine(a, np.ones(n, np.float32), floor, exp_ms, pct)
    assert got and got[0][0] == 0
    assert _check_refine(a, np.zeros(n, np.float32), floor, exp_ms, pct) == []
    # silence in front of speech: the running maximum keeps the contraction at the segment's start
    b = a.copy()
    b[:20000] = 0
    _check_refine(b, mask_of([[100, 30000], [30500, n]]), floor, exp_ms, pct)


def test_refine_intervals_degenerate():
    # no 20 ms window: the segments come back unchanged; empty segments are dropped
    assert vad_post.refine_intervals(np.zeros(0, np.float32), 100, [[10, 60]]) == [[10, 60]]
    assert vad_post.refine_intervals(np.ones(3, np.float32), 640, [[10, 10], [20, 15]]) == []
    assert vad_post.refine_intervals(np.ones(3, np.float32), 640, []) == []


def test_percentile_restatement_matches_numpy():
    """vad_post._slice_percentile has the bits of np.percentile on the materialised slice."""
    rng = np.random.default_rng(0)
    n = 16000 * 4 + 99
    a = _audio(n, 3, gain=1.0)
    en = _hop_energies(a)
    fe, k = vad_post.frame_energy(a)
    c = np.maximum.accumulate(en)
    E = (k - 1) * 160 + 320
    s = rng.integers(0, n - 1, 400)
    e = np.minimum(n, s + 1 + rng.integers(0, 30000, 400) // rng.integers(1, 200, 400))
    for pct in (0.0, 5.0, 10.0, 30.0, 50.0, 99.9, 100.0):
        got = vad_post._slice_percentile(c, k, E, s, e, pct)
        assert got.dtype == np.float32
        want = np.array([np.percentile(fe[i:j], pct) for i, j in zip(s, e)])
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('L', [256 * 40, 256 * 40 + 100, 256 * 37 + 255, 256 * 41])
def test_segments_from_flags(L):
    flags = vad_post.post_process_speech_flags(_markov_flags(40, 1, p_on=0.3, p_off=0.2))
    flags[-1] = 1.0                                  # the last frame is speech: clipped to L where it sticks out
    mask = vad_post.flags_to_mask(flags, L, 256)
    assert vad_post.segments_from_flags(flags, L, 256) == _runs_of(mask)
    assert vad_post.segments_from_flags([], L, 256) == []
    assert vad_post.segments_from_flags([0, 0], L, 256) == []


def test_segments_from_flags_longer_than_audio():
    flags = [0, 1, 1, 0, 1, 1, 1, 1]                 # 8 * 256 = 2048 > L: the last run is cut, a run past L dropped
    for L in (1500, 1024, 1025, 300):
        assert len(flags) * 256 > L
        assert vad_post.segments_from_flags(flags, L, 256) == _runs_of(vad_post.flags_to_mask(flags, L, 256))


def _energy_vad_before(x, hop=256, range_db=25.0, floor_db=-60.0):
    """EnergyVad.__call__ as it was before the split into frame_energy / flags_from_energy."""
    x = np.clip(np.asarray(x).astype(np.float32), -1.0, 1.0)
    if x.size == 0:
        return [], x
    n = len(x) // hop
    if n == 0:
        return [], x
    fr = x[:n * hop].reshape(n, hop).astype(np.float64)
    db = 10 * np.log10(np.mean(fr ** 2, axis=1) + 1e-12)
    return (db > max(np.percentile(db, 95) - range_db, floor_db)).astype(np.int64).tolist(), x


@pytest.mark.parametrize('n', [0, 100, 256, 16161, 80000])
def test_energy_vad_split(n):
    import torch
    wav = synthetic.synth_meeting(5.0, 2, seed=2)[0][:n] * 1.5      # the clip matters
    vad = idz.EnergyVad()
    flags, x = vad(wav)
    want_flags, want_x = _energy_vad_before(wav)
    assert flags == want_flags and isinstance(flags, list)
    np.testing.assert_array_equal(x, want_x)
    assert x.dtype == np.float32
    e16 = vad.frame_energy(wav)
    assert e16.dtype == np.float64 and e16.shape == (n // 256,)
    assert vad.flags_from_energy(e16) == flags
    if n >= 256:
        np.testing.assert_array_equal(e16, np.mean(want_x[:n // 256 * 256].reshape(-1, 256).astype(np.float64) ** 2, axis=1))
    # a torch tensor goes the same way
    flags_t, x_t = vad(torch.from_numpy(wav))
    assert flags_t == flags
    np.testing.assert_array_equal(x_t, x)


def device_energies(x):
    """The arithmetic of spk_vad_energy_f32 in numpy (include/spk_hip.h): fp64 squares of the
    clipped samples, quads of 4, blocks of 8 quads, hops of 5 blocks and frames of 8 blocks, each a
    left-to-right chain; e16 = frame / 256, e20 = float32(h[j] + h[j+1]) / float32(320)."""
    c = np.clip(np.asarray(x, dtype=np.float32), -1.0, 1.0).astype(np.float64)
    nb = len(c) // 32
    sq = (c[:nb * 32] ** 2).reshape(nb, 8, 4)
    quad = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    blk = quad[:, 0]
    for i in range(1, 8):
        blk = blk + quad[:, i]

    def chain(width):
        g = blk[:len(blk) // width * width].reshape(-1, width)
        out = g[:, 0] if len(g) else np.zeros(0)
        for i in range(1, width):
            out = out + g[:, i]
        return out

    e16 = chain(8) / 256.0
    h = chain(5)
    n20 = (len(c) - 320) // 160 + 1 if len(c) >= 320 else 0
    e20 = (h[:n20] + h[1:n20 + 1]).astype(np.float32) / np.float32(320)
    return e16, e20


@pytest.mark.parametrize('n', [0, 100, 320, 16161, 70001])
def test_device_arithmetic_on_grid_audio(n):
    """On audio quantised to multiples of 2^-7 every square is a multiple of 2^-14 and a window sum
    is below 2^9, so every partial sum is exact in fp32 in any order, and both sides end with one
    fp32 division by 320: the device arithmetic equals the host's `en` and EnergyVad's fp64 means
    to the bit.  This is the condition under which tests/test_gpu_vad.py demands equality."""
    x = synthetic.synth_meeting(5.0, 2, seed=4)[0][:n] * 1.5
    x = np.clip(np.round(x * 128) / 128, -1, 1).astype(np.float32)
    e16, e20 = device_energies(x)
    assert e16.dtype == np.float64 and e20.dtype == np.float32
    np.testing.assert_array_equal(e20, _hop_energies(x))
    np.testing.assert_array_equal(e16, idz.EnergyVad().frame_energy(x))
    if n >= 320:
        assert len(e20) == vad_post.frame_energy(x)[1]
        assert e20.max() > 0


@pytest.mark.parametrize('L,want', [(0, (0, 0)), (255, (0, 0)), (256, (1, 0)), (319, (1, 0)), (320, (1, 1)),
                                     (479, (1, 1)), (480, (1, 2)), (16161, (63, 100))])
def test_vad_energy_sizes_abi(L, want):
    from speakerlab import _hip
    lib = _hip.lib()
    n16, n20 = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.spk_vad_energy_sizes(L, ctypes.byref(n16), ctypes.byref(n20)) == 0
    assert (n16.value, n20.value) == want == (L // 256, (L - 320) // 160 + 1 if L >= 320 else 0)
    assert _hip.vad_energy_sizes(L) == want


def test_vad_abi_argument_checks():
    from speakerlab import _hip
    lib = _hip.lib()
    SPK_E_INVALID = -1
    v = ctypes.c_int64()
    assert lib.spk_vad_energy_sizes(-1, ctypes.byref(v), ctypes.byref(v)) == SPK_E_INVALID
    assert lib.spk_vad_energy_sizes(10, None, ctypes.byref(v)) == SPK_E_INVALID
    assert b'spk_vad_energy_sizes' in lib.spk_last_error()
    # checked before anything touches a device
    assert lib.spk_vad_energy_f32(None, None, -1, None, None, None, None, None) == SPK_E_INVALID
    assert lib.spk_vad_energy_f32(None, None, 0, None, None, None, None, None) == 0
    assert lib.spk_vad_energy_f32(None, None, 1, None, None, None, None, None) == SPK_E_INVALID
    assert lib.spk_vad_apply_intervals_f32(None, -1, None, None, 0, None, None) == SPK_E_INVALID
    assert lib.spk_vad_apply_intervals_f32(None, 10, None, None, -1, None, None) == SPK_E_INVALID
    assert lib.spk_vad_apply_intervals_f32(None, 10, None, None, 0, None, None) == SPK_E_INVALID
    assert lib.spk_vad_apply_intervals_f32(None, 0, None, None, 0, None, None) == 0
