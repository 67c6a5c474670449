"""``_hip.fbank_chunks`` (spk_fbank_chunks_f32): the Fbank of circle-padded chunks, addressed in
place by the kernel, against ``_hip.fbank`` of the batch gathered with ``torch.remainder`` the way
``Diarization3Dspeaker.embed_batches`` gathers it.  Same kernel and arithmetic, so the comparison
is ``torch.equal``.

Shapes: one frame (pad_len 400), tail samples that belong to no frame (400 + 160 * 3 + 37) and
a 1.5 s chunk (24000); chunk lengths 1, 7, 159 (several wraps inside one 400-sample frame: the
per-lane reduction), 399 / 400 / 401 (around the switch to conditional subtractions),
pad_len - 1 (one wrap, in the last frame) and pad_len (none), all in one call; 1, 9 and 67
chunks (fewer than the 8 utterance groups of the block map, and counts that are no multiple of
8).  The signal is two recordings back to back, with chunks from both, one that starts at
sample 0 and one that ends at the last sample."""
import numpy as np
import pytest
import torch

import data_ref as D
from speakerlab import _hip

pytestmark = pytest.mark.gpu

REC = (30000, 26011)                      # two recordings back to back
TOTAL = sum(REC)
PAD_LENS = (400, 400 + 160 * 3 + 37, 24000)


@pytest.fixture(scope='module')
def pool():
    wav = np.concatenate([D.noise(REC[0], 0.1, 21), D.noise(REC[1], 0.02, 22)])
    return torch.from_numpy(wav).cuda()


def _gathered(wav, starts, lens, pad_len):
    """The [n, pad_len] batch embed_batches builds."""
    ar = torch.arange(pad_len, device=wav.device)
    s, n = starts.to(wav.device)[:, None], lens.to(wav.device)[:, None]
    return wav[s + torch.remainder(ar[None], n)]


def _chunks(n_chunks, pad_len):
    """(starts, lens): the eight lengths in turn; the chunk of length pad_len first starts at
    sample 0 (recording one), the one of pad_len - 1 ends at the last sample (recording two),
    the others are spread over both recordings."""
    kinds = [1, 7, 159, 399, 400, 401, pad_len - 1, pad_len]
    if n_chunks == 1:
        return torch.tensor([TOTAL - 159]), torch.tensor([159])      # ends at the last sample
    starts, lens = [], []
    for k in range(n_chunks):
        ln = kinds[(k + 7) % 8]                                        # k = 0: pad_len at sample 0
        st = 0 if k == 0 else TOTAL - ln if k == 7 else (k * 7919) % (TOTAL - ln + 1)
        starts.append(st)
        lens.append(ln)
    assert set(lens) == set(kinds)
    assert min(starts) < REC[0] < max(starts)                          # chunks from both recordings
    return torch.tensor(starts), torch.tensor(lens)


@pytest.mark.parametrize('mean_nor', [False, True])
@pytest.mark.parametrize('n_chunks', [1, 9, 67])
@pytest.mark.parametrize('pad_len', PAD_LENS)
def test_bits_of_the_gathered_batch(pool, pad_len, n_chunks, mean_nor):
    starts, lens = _chunks(n_chunks, pad_len)
    want = _hip.fbank(_gathered(pool, starts, lens, pad_len), 80, mean_nor=mean_nor)
    got = _hip.fbank_chunks(pool, starts, lens, pad_len, 80, mean_nor=mean_nor)
    assert got.shape == want.shape == (n_chunks, 1 + (pad_len - 400) // 160, 80)
    assert torch.isfinite(want).all()
    bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
    assert torch.equal(got, want), [(c, int(starts[c]), int(lens[c])) for c in bad[:8]]


def test_device_starts_and_longer_than_pad(pool):
    """Start / length tensors already on the device; chunks longer than pad_len never wrap."""
    pad_len = PAD_LENS[1]
    starts = torch.tensor([0, 11, REC[0] - 100, TOTAL - 3 * pad_len]).cuda()
    lens = torch.tensor([pad_len + 5, 2 ** 15, pad_len + 1, 3 * pad_len]).cuda()
    got = _hip.fbank_chunks(pool, starts, lens, pad_len, 80, mean_nor=True)
    assert torch.equal(got, _hip.fbank(_gathered(pool, starts, lens, pad_len), 80, mean_nor=True))


def test_processor_entry(pool):
    from speakerlab.process.processor import FBank
    fb = FBank(80, 16000, mean_nor=True)
    starts, lens = _chunks(9, PAD_LENS[1])
    got = fb.chunks(pool, starts, lens, PAD_LENS[1])
    assert got.is_cuda and torch.equal(got, fb.batch(_gathered(pool, starts, lens, PAD_LENS[1])))


def test_no_chunks(pool):
    e = torch.empty(0, dtype=torch.int64)
    out = _hip.fbank_chunks(pool, e, e, 24000, 80, mean_nor=True)
    assert out.shape == (0, 148, 80) and out.is_cuda
    # through the ABI: SPK_OK without a launch, whatever the pointers
    assert _hip.lib().spk_fbank_chunks_f32(None, TOTAL, None, None, 0, 24000, None, 80, 1, None) == 0


def _raw(pool, **kw):
    """spk_fbank_chunks_f32 on one valid chunk, with arguments replaced by ``kw``."""
    sn = torch.tensor([[0], [500]], dtype=torch.int64, device='cuda')
    feats = torch.full((3 * 128,), float('nan'), device='cuda')
    a = dict(wav=pool.data_ptr(), wav_len=TOTAL, start=sn[0].data_ptr(), len=sn[1].data_ptr(), n=1, pad_len=720,
             feats=feats.data_ptr(), n_mels=80)
    a.update(kw)
    rc = _hip.lib().spk_fbank_chunks_f32(a['wav'], a['wav_len'], a['start'], a['len'], a['n'], a['pad_len'], a['feats'],
                                         a['n_mels'], 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, feats


@pytest.mark.parametrize('kw', [dict(wav=None), dict(start=None), dict(len=None), dict(feats=None), dict(n=-1),
                                dict(pad_len=399), dict(pad_len=0), dict(wav_len=0), dict(wav_len=-5),
                                dict(n_mels=3), dict(n_mels=129), dict(n_mels=0)],
                         ids=lambda kw: '-'.join(f'{k}={v}' for k, v in kw.items()))
def test_invalid_arguments_abi(pool, kw):
    rc, feats = _raw(pool, **kw)
    assert rc == _hip.E_INVALID, (rc, _hip.lib().spk_last_error())
    assert b'spk_fbank_chunks_f32' in _hip.lib().spk_last_error()
    assert torch.isnan(feats).all()                                    # nothing was launched
    rc, feats = _raw(pool)                                             # the same call, valid
    assert rc == 0 and torch.isfinite(feats[:3 * 80]).all() and torch.isnan(feats[3 * 80:]).all()


@pytest.mark.parametrize('starts,lens', [([0, TOTAL - 10], [500, 11]),        # start + length past the signal
                                         ([TOTAL], [1]), ([5], [0]), ([-1], [400]), ([0, 1], [400])])
def test_invalid_chunks_caught_on_the_host(pool, starts, lens):
    for to in (torch.device('cpu'), pool.device):
        with pytest.raises(_hip.HipError) as e:
            _hip.fbank_chunks(pool, torch.tensor(starts).to(to), torch.tensor(lens).to(to), 720, 80)
        assert e.value.code == _hip.E_INVALID


@pytest.mark.parametrize('kw', [dict(pad_len=399), dict(n_mels=3), dict(n_mels=129)], ids=str)
def test_invalid_arguments_binding(pool, kw):
    a = dict(pad_len=720, n_mels=80)
    a.update(kw)
    with pytest.raises(_hip.HipError) as e:
        _hip.fbank_chunks(pool, [0], [500], a['pad_len'], a['n_mels'])
    assert e.value.code == _hip.E_INVALID
    with pytest.raises(_hip.HipError) as e:
        _hip.fbank_chunks(pool[None], [0], [500], 720, 80)              # not a 1-D signal
    assert e.value.code == _hip.E_INVALID


@pytest.mark.parametrize('mean_nor', [False, True])
def test_short_chunk_against_fp64_oracle(pool, mean_nor):
    """One chunk shorter than a frame (250 samples, seven frames of pad_len 1360) against
    oracle/fbank_ref in fp64 on the materialised chunk, inside the derived bounds of data_ref."""
    start, ln, pad_len = REC[0] - 100, 250, 1360
    chunk = pool.cpu().numpy()[start + np.arange(pad_len) % ln]
    out = _hip.fbank_chunks(pool, [start], [ln], pad_len, 80, mean_nor=mean_nor).cpu().numpy()[0]
    worst = D.fbank_check(out, chunk, 80, mean_nor, ('chunk', ln, pad_len))
    print(f'fbank_chunks len {ln} pad {pad_len} mean_nor={mean_nor}: max err/bound {worst:.3f}')
