"""Host side of ``--pool_chunks``: the batch plan of ``speakerlab.utils.chunk_pool`` on hand-made
inputs, and the command line's refusal of the flag without an ``--ahc_batch`` group."""
import numpy as np
import pytest

from speakerlab.utils.chunk_pool import plan_chunk_batches


def _check_plan(lens_per_file, batchsize):
    """Every property the plan promises; returns the batches."""
    batches, inverse = plan_chunk_batches(lens_per_file, batchsize)
    pads = [max(l) if len(l) else None for l in lens_per_file]
    seen = []
    for b in batches:
        assert 1 <= len(b.files) == len(b.chunks) <= batchsize
        assert {pads[f] for f in b.files} == {b.pad_len}            # no batch mixes pad lengths
        seen += list(zip(b.files.tolist(), b.chunks.tolist()))
    want = [(f, c) for f, l in enumerate(lens_per_file) for c in range(len(l))]
    assert sorted(seen) == want and len(set(seen)) == len(seen)     # every (file, chunk) exactly once
    # inside a pad-length group the rows keep (file, chunk) order, and only a group's last batch is short
    for pad in set(p for p in pads if p is not None):
        rows = [fc for b in batches if b.pad_len == pad for fc in zip(b.files.tolist(), b.chunks.tolist())]
        assert rows == sorted(rows)
        sizes = [len(b.files) for b in batches if b.pad_len == pad]
        assert all(s == batchsize for s in sizes[:-1])
    # the inverse map puts the concatenated rows back at (file, chunk)
    assert len(inverse) == len(lens_per_file)
    for f, l in enumerate(lens_per_file):
        assert inverse[f].dtype == np.int64 and inverse[f].shape == (len(l),)
        assert [seen[r] for r in inverse[f]] == [(f, c) for c in range(len(l))]
    return batches


def test_equal_pad_lengths_share_batches():
    batches = _check_plan([[8000, 8000, 3000], [8000] * 4, [5000, 8000]], 4)
    assert [len(b.files) for b in batches] == [4, 4, 1]             # 9 chunks: not a multiple of 4
    assert batches[0].files.tolist() == [0, 0, 0, 1] and batches[1].files.tolist() == [1, 1, 1, 2]
    assert all(b.pad_len == 8000 for b in batches)


def test_different_pad_lengths_never_mix():
    batches = _check_plan([[8000, 2000], [5632, 5120], [8000], [5632]], 8)
    assert [(b.pad_len, b.files.tolist()) for b in batches] == [(8000, [0, 0, 2]), (5632, [1, 1, 3])]


def test_file_without_chunks():
    batches = _check_plan([[], [700, 900], [], [900]], 2)
    assert [b.files.tolist() for b in batches] == [[1, 1], [3]]
    assert plan_chunk_batches([[], []], 4)[0] == []
    assert plan_chunk_batches([], 4) == ([], [])


def test_batchsize_one_and_large():
    batches = _check_plan([[10, 12], [12, 3, 4]], 1)
    assert len(batches) == 5
    assert len(_check_plan([[10, 12], [12, 3, 4]], 64)) == 1


def test_random_plans():
    rng = np.random.default_rng(0)
    for _ in range(20):
        lens = [rng.choice([400, 8000, 8001, 24000], size=rng.integers(0, 12)).tolist() for _ in range(rng.integers(1, 9))]
        _check_plan(lens, int(rng.integers(1, 10)))


def test_bad_arguments():
    with pytest.raises(ValueError):
        plan_chunk_batches([[5]], 0)
    with pytest.raises(ValueError):
        plan_chunk_batches([[5, 0]], 4)


@pytest.mark.parametrize('extra', [[], ['--ahc_batch', '1'], ['--gpu_ahc'], ['--gpu_ahc', '--ahc_batch', '1']])
def test_pool_chunks_needs_an_ahc_batch_group(extra, capsys):
    from speakerlab.bin import infer_diarization as idz
    with pytest.raises(SystemExit) as e:
        idz.main(['--wav', 'a.wav', '--out_dir', 'out', '--pool_chunks'] + extra)
    assert e.value.code == 2
    assert '--pool_chunks' in capsys.readouterr().err


def test_pool_chunks_inherits_the_ahc_batch_rules(capsys):
    """K > 1 itself needs --gpu_ahc and excludes --shard_chunks, with or without pooling."""
    from speakerlab.bin import infer_diarization as idz
    for extra in (['--ahc_batch', '4'], ['--gpu_ahc', '--ahc_batch', '4', '--shard_chunks']):
        with pytest.raises(SystemExit) as e:
            idz.main(['--wav', 'a.wav', '--out_dir', 'out', '--pool_chunks'] + extra)
        assert e.value.code == 2
        assert '--ahc_batch' in capsys.readouterr().err
    args = idz.parser.parse_args(['--wav', 'a.wav', '--out_dir', 'out', '--gpu_ahc', '--ahc_batch', '4', '--pool_chunks'])
    assert args.pool_chunks and not idz.parser.parse_args(['--wav', 'a.wav', '--out_dir', 'out']).pool_chunks
