"""The single-speaker check end to end on the device (``SingleSpeakerChecker`` and the CLI), with
synthetic weights: a group of files checked together against each file on its own, the reported
minimum and mean against the host restatement on per-file embeddings, and the CLI's two output
layouts.

Four recordings of a few seconds: silence (no segment), one burst of synthetic speech (one segment,
no pair) and two with three bursts from two synthetic speakers."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FS = 16000
# name -> (seconds, [(start s, stop s, speaker), ...])
RECORDINGS = {
    'multi_a': (4.0, [(0.3, 1.1, 0), (1.8, 2.5, 1), (3.1, 3.8, 0)]),
    'quiet': (2.0, []),
    'one': (2.0, [(0.5, 1.4, 0)]),
    'multi_b': (4.5, [(0.4, 1.3, 1), (2.0, 2.6, 1), (3.3, 4.2, 0)]),
}
REFERENCE_KEYS = ['wav_path', 'num_segments', 'segments', 'threshold', 'min_pairwise_cosine', 'mean_pairwise_cosine',
                  'is_single_speaker', 'pairwise_similarities']
THRESHOLD = 0.8
# tests/test_gpu_pool_chunks.py holds pooled against per-file embeddings to 1e-4, row by row in the
# 2-norm.  A row within eps of another (relative) is within asin(eps) of it in angle, angles obey
# the triangle inequality and the cosine is 1-Lipschitz in the angle, so a pair's cosine moves by
# at most 2 asin(eps); the device cosine itself is float32 over E = 192 terms, (E + 4) 2^-24 from
# the exact value (the bound of tests/data_ref.py).  The minimum and the mean of values that each
# move by at most that move by at most that.
EMB_TOL = 1e-4
COS_TOL = 2 * math.asin(EMB_TOL) + (192 + 4) * 2.0 ** -24


def _recording(seconds, bursts, seed):
    from speakerlab.utils import synthetic
    wav = np.zeros(int(seconds * FS), dtype=np.float32)
    for k, (st, ed, spk) in enumerate(bursts):
        a, b = int(st * FS), int(ed * FS)
        wav[a:b] = synthetic.synth_wav(b - a, seed=seed + k, speaker=spk)
    return wav


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    from speakerlab.utils.fileio import write_wav
    d = tmp_path_factory.mktemp('single_speaker')
    paths = []
    for q, (name, (seconds, bursts)) in enumerate(RECORDINGS.items()):
        paths.append(str(d / f'{name}.wav'))
        write_wav(paths[-1], _recording(seconds, bursts, 100 * q))
    return paths


@pytest.fixture(scope='module')
def checker():
    from speakerlab.bin.check_single_speaker import SingleSpeakerChecker
    return SingleSpeakerChecker(torch.device('cuda', 0), threshold=THRESHOLD, batch_size=4, vad='energy',
                                synthetic_weights=True)


@pytest.fixture(scope='module')
def results(checker, files):
    """(``check`` of every file, ``check_many`` of all of them): computed once, read by the tests."""
    return [checker.check(f) for f in files], checker.check_many(files)


def test_the_inputs_cover_zero_one_and_several_segments(results):
    one, _ = results
    n = [r['num_segments'] for r in one]
    assert n[1] == 0 and n[2] == 1 and n[0] >= 3 and n[3] >= 3
    assert n[0] + n[3] > 4                                 # more segments than one embedding batch of 4
    for r in one:
        assert list(r) == REFERENCE_KEYS
        assert len(r['pairwise_similarities']) == r['num_segments'] * (r['num_segments'] - 1) // 2 \
            if r['num_segments'] > 1 else r['pairwise_similarities'] == []
    quiet = one[1]
    assert quiet['min_pairwise_cosine'] == 1.0 and quiet['mean_pairwise_cosine'] == 1.0
    assert quiet['is_single_speaker'] is True and quiet['segments'] == []
    assert one[2]['min_pairwise_cosine'] == 1.0 and one[2]['is_single_speaker'] is True


def test_pairs_are_consistent_with_the_summary(results):
    one, _ = results
    for r in (one[0], one[3]):
        cos = [p['cosine'] for p in r['pairwise_similarities']]
        n = r['num_segments']
        assert [(p['i'], p['j']) for p in r['pairwise_similarities']] == \
            [(i, j) for i in range(n) for j in range(i + 1, n)]
        assert all(p['seg_i'] == r['segments'][p['i']] and p['seg_j'] == r['segments'][p['j']]
                   for p in r['pairwise_similarities'])
        assert r['min_pairwise_cosine'] == min(cos)
        assert abs(r['mean_pairwise_cosine'] - sum(cos) / len(cos)) <= 2.0 ** -23
        assert r['is_single_speaker'] == (min(cos) >= THRESHOLD)


def test_check_many_equals_check(results):
    one, many = results
    for q, (a, b) in enumerate(zip(one, many)):
        if a != b and a['num_segments'] > 1:
            d = max(abs(x['cosine'] - y['cosine']) for x, y in zip(a['pairwise_similarities'],
                                                                   b['pairwise_similarities']))
            print(f'file {q}: largest cosine difference {d:.3e}')
    assert many == one


def test_min_and_mean_against_the_host_restatement(checker, files, results):
    from speakerlab.utils import single_speaker as ss
    _, many = results
    for f, r in zip(files, many):
        chunks, wav_data = checker.front.do_front(f)
        assert [[s['start'], s['stop']] for s in r['segments']] == [[float(a), float(b)] for a, b in chunks]
        emb = checker.front.do_emb_extraction(chunks, wav_data) if chunks else None
        ref = ss.pair_stats_host([emb], THRESHOLD)[0]
        dmin = abs(r['min_pairwise_cosine'] - ref['min'])
        dmean = abs(r['mean_pairwise_cosine'] - ref['mean'])
        print(f'{os.path.basename(f)}: {r["num_segments"]} segments, |min - host| {dmin:.3e}, '
              f'|mean - host| {dmean:.3e}, bound {COS_TOL:.3e}')
        assert dmin <= COS_TOL and dmean <= COS_TOL


def test_cli_directory_mode(files, results, tmp_path, capsys):
    from speakerlab.bin import check_single_speaker as css
    _, many = results
    src = os.path.dirname(files[0])
    css.main(['--src_dir', src, '--pattern', '*.wav', '--out_dir', str(tmp_path / 'out'), '--threshold',
              str(THRESHOLD), '--batch_size', '4', '--files_per_batch', '3', '--vad', 'energy',
              '--synthetic_weights'])
    assert f'Wrote {len(files)} results' in capsys.readouterr().out
    written = sorted(os.listdir(tmp_path / 'out'))
    assert written == sorted(f'{name}.single_spk.json' for name in RECORDINGS)
    by_path = {r['wav_path']: r for r in many}
    for f in files:
        name = os.path.basename(f)[:-4]
        res = json.loads((tmp_path / 'out' / f'{name}.single_spk.json').read_text())
        assert list(res) == REFERENCE_KEYS
        want = by_path[f]
        assert res['wav_path'] == f and res['segments'] == want['segments']
        assert res['num_segments'] == want['num_segments'] and res['threshold'] == THRESHOLD
        # groups of 3 and 1 here, one group of 4 in the fixture
        assert abs(res['min_pairwise_cosine'] - want['min_pairwise_cosine']) <= 2 * COS_TOL
        assert abs(res['mean_pairwise_cosine'] - want['mean_pairwise_cosine']) <= 2 * COS_TOL


def test_cli_list_mode_and_no_pairs(files, tmp_path, capsys):
    from speakerlab.bin import check_single_speaker as css
    lst = tmp_path / 'wavs.list'
    lst.write_text(''.join(f'{f}\n' for f in files))
    base = ['--wav', str(lst), '--threshold', str(THRESHOLD), '--batch_size', '4', '--vad', 'energy',
            '--synthetic_weights']
    css.main(base + ['--out', str(tmp_path / 'full' / 'all.json')])
    css.main(base + ['--out', str(tmp_path / 'lean.json'), '--no_pairs'])
    full = json.loads((tmp_path / 'full' / 'all.json').read_text())
    lean = json.loads((tmp_path / 'lean.json').read_text())
    assert isinstance(full, list) and len(full) == len(lean) == len(files)
    for a, b in zip(full, lean):
        assert list(a) == REFERENCE_KEYS and list(b) == REFERENCE_KEYS[:-1]
        assert {k: v for k, v in a.items() if k != 'pairwise_similarities'} == b
    # one wav: a single object, to stdout without --out
    capsys.readouterr()
    css.main(['--wav', files[2], '--vad', 'energy', '--synthetic_weights'])
    res = json.loads(capsys.readouterr().out)
    assert isinstance(res, dict) and res['wav_path'] == files[2] and res['num_segments'] == 1
