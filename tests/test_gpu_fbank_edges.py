"""Edge cases of the Fbank kernels (csrc/fbank.hip) against oracle/fbank_ref in fp64 with the
derived bounds of tests/data_ref.py: every mel count the tables accept (n_mels % 4 != 0 runs
fbank_cmn_kernel<1>, mel blocks that are not 32 wide), one to seven frames and ragged mixes,
batch sizes that make G = 64, 6 and 1 slices per utterance, signals that sit on, across and far
above the FLT_EPSILON floor or in the [0.5, 1) energies where the split log cancels, and the
padded form's zero fill.  Every test prints its worst err / bound."""
import numpy as np
import pytest
import torch

import data_ref as D
from oracle import fbank_ref
from speakerlab import _hip

pytestmark = pytest.mark.gpu

SHORT = 300            # fewer than 400 samples: zero frames


def _ragged(wavs, n_mels, mean_nor):
    """List of 1-D float32 arrays -> list of [T_i, n_mels] arrays (one launch)."""
    L = max(len(w) for w in wavs)
    buf = np.full((len(wavs), L), 1e30, np.float32)       # past each length: never read
    for i, w in enumerate(wavs):
        buf[i, :len(w)] = w
    outs = _hip.fbank(torch.from_numpy(buf).cuda(), n_mels, mean_nor=mean_nor, lengths=[len(w) for w in wavs])
    return [o.cpu().numpy() for o in outs]


def _solo(wav, n_mels, mean_nor):
    return _hip.fbank(torch.from_numpy(wav).cuda()[None], n_mels, mean_nor=mean_nor).cpu().numpy()[0]


def _lengths_batch(B, seed=0):
    lens = [D.FB_LENGTHS[(i * 7 + i // 5) % 5] for i in range(B)]
    return [D.noise(n, 0.1, seed + i) for i, n in enumerate(lens)]


@pytest.mark.parametrize('mean_nor', [False, True])
@pytest.mark.parametrize('n_mels', D.N_MELS)
def test_every_accepted_n_mels(n_mels, mean_nor):
    wavs = [D.noise(n, 0.1, n) for n in D.FB_LENGTHS] + [D.noise(SHORT, 0.1, 1)]
    if not D.fbank_tables_accept(D.N_MELS)[n_mels]:
        with pytest.raises(_hip.HipError):
            _ragged(wavs, n_mels, mean_nor)
        return
    outs = _ragged(wavs, n_mels, mean_nor)
    assert outs[-1].shape == (0, n_mels)
    worst = 0.0
    for w, o in zip(wavs[:-1], outs):
        worst = max(worst, D.fbank_check(o, w, n_mels, mean_nor, (n_mels, len(w))))
        assert np.array_equal(o, _solo(w, n_mels, mean_nor)), (n_mels, len(w))
    print(f'fbank n_mels={n_mels} mean_nor={mean_nor}: max err/bound {worst:.3f}')


@pytest.mark.parametrize('n_mels', [3, 129])
def test_refused_n_mels_write_nothing(n_mels):
    wav = torch.from_numpy(D.noise(720, 0.1, 2)).cuda()
    offs = torch.tensor([[0, 720], [0, 3]], dtype=torch.int64, device='cuda')
    feats = torch.full((3 * 129 + 64,), float('nan'), device='cuda')
    rc = _hip.lib().spk_fbank_f32(wav.data_ptr(), offs[0].data_ptr(), 1, feats.data_ptr(), offs[1].data_ptr(), n_mels,
                                  1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0
    assert torch.isnan(feats).all()
    with pytest.raises(_hip.HipError):
        _hip.fbank(wav[None], n_mels)


@pytest.mark.parametrize('B', [1, 8, 9, 600, 2049])
def test_batch_sizes(B):
    """G = 64 slices per utterance up to 64 utterances, 6 at 600 (not a power of two), 1 at 2049;
    ragged lengths of 1 to 7 frames.  The reference is computed for about 64 rows, spread over all
    utt % 8 and both ends."""
    assert max(1, min(64, 16384 // (4 * B))) == {1: 64, 8: 64, 9: 64, 600: 6, 2049: 1}[B]
    wavs = _lengths_batch(B, seed=B)
    rows = sorted(set(range(min(B, 24))) | set(range(max(0, B - 24), B)) | set(range(0, B, max(1, B // 16))))
    assert B < 64 or {r % 8 for r in rows} == set(range(8))
    worst = 0.0
    for mean_nor in (False, True):
        outs = _ragged(wavs, 80, mean_nor)
        for r in rows:
            worst = max(worst, D.fbank_check(outs[r], wavs[r], 80, mean_nor, (B, r)))
        for r in rows[::4]:
            assert np.array_equal(outs[r], _solo(wavs[r], 80, mean_nor)), (B, r)
    print(f'fbank B={B}: max err/bound {worst:.3f} over {len(rows)} rows')


SIGNALS = D.fbank_signals()


@pytest.mark.parametrize('name', list(SIGNALS))
def test_signals(name):
    wav = SIGNALS[name]
    worst = 0.0
    for n_mels in (80, 23):
        for mean_nor in (False, True):
            out = _solo(wav, n_mels, mean_nor)
            worst = max(worst, D.fbank_check(out, wav, n_mels, mean_nor, (name, n_mels, mean_nor)))
    if name == 'constant':
        assert np.all(_solo(wav, 80, False) == D.FLOOR32)
    print(f'fbank {name}: max err/bound {worst:.3f}')


@pytest.mark.parametrize('B,n_mels', [(5, 80), (6, 23), (2049, 80)])
@pytest.mark.parametrize('mean_nor', [False, True])
def test_padded_form(B, n_mels, mean_nor):
    """spk_fbank_f32_padded through the ABI: output and a guard behind it NaN-filled; valid rows
    inside the bound and bit-equal to the utterance alone, rows [nfr, t_max) exactly 0, the guard
    intact.  One row has fewer than 400 samples (zero frames: all of its rows are 0)."""
    wavs = _lengths_batch(B, seed=3 * B)
    wavs[min(2, B - 1)] = D.noise(SHORT, 0.1, 9)
    lens = [len(w) for w in wavs]
    frames = [fbank_ref.num_frames(n) for n in lens]
    t_max, L, G = max(frames) + 2, max(lens), 4096
    buf = np.zeros((B, L), np.float32)
    for i, w in enumerate(wavs):
        buf[i, :len(w)] = w
    dwav = torch.from_numpy(buf).cuda()
    offs = torch.tensor([[i * L for i in range(B + 1)], np.concatenate([[0], np.cumsum(frames)]).tolist()],
                        dtype=torch.int64, device='cuda')
    feats = torch.full((B * t_max * n_mels + G,), float('nan'), device='cuda')
    rc = _hip.lib().spk_fbank_f32_padded(dwav.data_ptr(), offs[0].data_ptr(), B, feats.data_ptr(), offs[1].data_ptr(),
                                         t_max, n_mels, int(mean_nor), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _hip.lib().spk_last_error()
    got = feats.cpu().numpy()
    assert np.isnan(got[B * t_max * n_mels:]).all()
    got = got[:B * t_max * n_mels].reshape(B, t_max, n_mels)
    for u in range(B):
        assert np.all(got[u, frames[u]:] == 0) and not np.signbit(got[u, frames[u]:]).any(), u
    rows = sorted(set(range(min(B, 16))) | set(range(max(0, B - 16), B)) | set(range(0, B, max(1, B // 16))))
    worst = 0.0
    for u in rows:
        if frames[u] == 0:
            continue
        worst = max(worst, D.fbank_check(got[u, :frames[u]], wavs[u], n_mels, mean_nor, (B, u)))
    for u in rows[::4]:
        if frames[u]:
            assert np.array_equal(got[u, :frames[u]], _solo(wavs[u], n_mels, mean_nor)), (B, u)
    print(f'fbank padded B={B} n_mels={n_mels} mean_nor={mean_nor}: max err/bound {worst:.3f}')
