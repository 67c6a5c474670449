"""speakerlab/bin/compute_utterance_similarities.py end to end on the GPU, both ``--pairs`` modes, on small
trees of utterance pickles (tests/verif_cli_tree.py): the output files are present and parse, the
sampled protocol on the golden embeddings lands in the reference's intervals
(tests/golden/verif_golden.*), and the all-pairs results equal the driver run directly."""
import numpy as np
import pytest
import torch

from speakerlab.bin import compute_utterance_similarities as cus
from speakerlab.utils import verification_analysis as va

import test_verif_golden as tg
import verif_cli_tree as tree

pytestmark = pytest.mark.gpu


def test_sampled_mode_on_the_golden_embeddings(tmp_path):
    meta, g = tg.load_golden()
    tree.write_tree(str(tmp_path), g['embeddings'], g['speaker'])
    out = tree.run(str(tmp_path))
    assert set(out) == tree.FILES
    res = out['evaluation_results_cosine.json']
    assert res['pairs'] == 'sampled' and len(res['y_scores']) == len(g['pairs'])
    assert res['y_true'] == g['pairs'][:, 2].tolist()
    tg.in_intervals(res, meta)
    stats = out['speaker_statistics.json']
    assert stats['total_speakers'] == meta['speakers'] and stats['total_utterances'] == meta['n_utterances']
    rep = out['analysis_report.json']
    assert rep['verification_results']['cosine']['eer'] == res['eer'] and rep['analysis_summary']['pairs'] == 'sampled'
    assert '| cosine |' in out['analysis_report.md']


def test_all_pairs_mode_equals_the_driver(tmp_path):
    X, keys = tree.synthetic_tree(str(tmp_path))
    out = tree.run(str(tmp_path), '--pairs', 'all', '--memory_efficient', '--chunk_size', '3')
    assert set(out) == tree.FILES
    res = out['evaluation_results_cosine.json']
    index = {}
    labels = np.array([index.setdefault(k, len(index)) for k in keys], np.int32)
    want = cus.all_pairs_result(va.analyze_device(torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda()))
    assert 'y_true' not in res and 'y_scores' not in res and res['pairs'] == 'all' and res['exact'] is True
    for k in ('eer', 'eer_threshold', 'eer_threshold_cosine', 'min_dcf', 'auc', 'auc_lo', 'auc_hi', 'auc_gap', 'eer_counts',
              'min_dcf_point', 'n_target_pairs', 'n_non_target_pairs', 'passes', 'fpr', 'tpr', 'moments', 'histogram'):
        assert res[k] == want[k], k
    assert res['thresholds'][1:] == want['thresholds'][1:] and len(res['fpr']) == 257
    n = len(keys)
    assert res['n_target_pairs'] + res['n_non_target_pairs'] == n * (n - 1) // 2
    assert abs(res['eer_threshold'] - (res['eer_threshold_cosine'] - 1.0)) < 1e-15
    stats = out['speaker_statistics.json']
    assert stats['total_utterances'] == n and set(stats['datasets']) == {'setA', 'setB'}
    assert 'exact' in out['analysis_report.md'] and out['analysis_report.json']['analysis_summary']['pairs'] == 'all'
