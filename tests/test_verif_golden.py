"""The sampled protocol of speakerlab/bin/compute_utterance_similarities.py against the reference
script's own numbers (tests/golden/verif_golden.*, made by tests/golden/make_verif_golden.py): the
pair list is identical, and EER, minDCF and AUC computed from host float32 cosines through the
product code lie in the intervals the maker recorded for a +-2e-6 move of the scores.  Also the CLI's
argument handling."""
import json
import os

import numpy as np
import pytest

from speakerlab.bin import compute_utterance_similarities as cus
from speakerlab.utils import similarity_analysis as sa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden():
    with open(os.path.join(GOLDEN, 'verif_golden.json')) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLDEN, 'verif_golden.npz')))


def in_intervals(result, meta):
    for k, (lo, hi) in meta['interval'].items():
        print(f'{k}: {result[k]!r} in [{lo!r}, {hi!r}], reference {meta["reference"][k]!r}')
    for k, (lo, hi) in meta['interval'].items():
        assert lo <= result[k] <= hi, (k, lo, result[k], hi)


def test_intervals_hold_the_reference_and_are_narrow():
    meta, _ = load_golden()
    for k, (lo, hi) in meta['interval'].items():
        assert lo <= meta['reference'][k] <= hi and hi - lo <= 0.05


def test_pair_list_is_the_reference_one():
    meta, g = load_golden()
    keys = [f'set_spk{s:02d}' for s in g['speaker']]
    pairs = np.asarray(cus.generate_speaker_pairs(keys), np.int64)
    assert np.array_equal(pairs, g['pairs'])
    assert (pairs[:, 2] == 1).sum() == meta['n_target_pairs'] and (pairs[:, 2] == 0).sum() == meta['n_non_target_pairs']


def test_sampled_metrics_from_host_cosines_lie_in_the_intervals():
    meta, g = load_golden()
    cos = sa.host_cosine(g['embeddings'])
    assert cos.dtype == np.float32
    p = g['pairs']
    res = cus.sampled_metrics(p[:, 2], cos[p[:, 0], p[:, 1]].astype(np.float64) - 1.0)
    in_intervals(res, meta)
    assert len(res['y_true']) == len(p) and res['metric'] == 'cosine'


@pytest.mark.parametrize('metric', ['euclidean', 'manhattan'])
def test_other_metrics_are_rejected_naming_the_flag(metric, capsys):
    with pytest.raises(SystemExit) as e:
        cus.parse_args(['--embeddings_dir', 'x', '--distance_metrics', 'cosine', metric])
    assert e.value.code != 0
    err = capsys.readouterr().err
    assert '--distance_metrics' in err and metric in err


def test_pairs_flag_and_ignored_flags():
    a = cus.parse_args(['--embeddings_dir', 'x'])
    assert a.pairs == 'sampled' and a.distance_metrics == ['cosine'] and not a.no_plot
    a = cus.parse_args(['--embeddings_dir', 'x', '--pairs', 'all', '--memory_efficient', '--chunk_size', '17',
                        '--distance_metrics', 'cosine', '--max_speakers', '5', '--max_utterances_per_speaker', '9',
                        '--plot_format', 'pdf', '--dpi', '80', '--num_workers', '2', '--output_dir', 'o',
                        '--utterances_subdir', 'u', '--no_plot'])
    assert a.pairs == 'all' and a.memory_efficient and a.chunk_size == 17 and a.no_plot
    with pytest.raises(SystemExit):
        cus.parse_args(['--embeddings_dir', 'x', '--pairs', 'some'])
