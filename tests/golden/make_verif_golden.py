"""Generate tests/golden/verif_golden.npz and tests/golden/verif_golden.json by running the REFERENCE
egs/mix_adult_kid/sv-eres2netv2/compute_utterance_similarities_analysis.py, read-only from
/root/reference.  Build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_verif_golden.py

12 seeded speakers with 3..9 utterances each, E = 64, clustered float32 embeddings.  The reference's
``generate_speaker_pairs``, ``compute_distance_matrix`` and ``evaluate_speaker_verification`` give
the pair list and its EER, minDCF and AUC.  The device's cosines differ from the host's by at most
2e-6 (the affinity kernel's parity bound, tests/test_gpu_affinity.py), and all three metrics are
monotone when every target score moves one way and every non-target score the other, so the same
three metrics are recomputed, with the reference's own functions, on the reference's scores with
targets lowered and non-targets raised by 2e-6 and the other way round: an interval per metric.
The script asserts that the reference's own values sit inside their intervals and that no interval
is wider than 0.05.  Fixtures are data only: embeddings, speaker indices, the pair list, the numbers.
``seaborn`` (only imported by the reference, never called here) is stubbed when absent."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/egs/mix_adult_kid/sv-eres2netv2/compute_utterance_similarities_analysis.py'
SPEAKERS, E, SEED, SHIFT = 12, 64, 20250611, 2e-6


def main():
    for name in ('seaborn', 'tqdm'):
        try:
            __import__(name)
        except ImportError:
            stub = types.ModuleType(name)
            stub.tqdm = lambda it=None, **kw: it
            sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location('ref_utt', REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rng = np.random.default_rng(SEED)
    centers = rng.standard_normal((SPEAKERS, E))
    speaker, rows = [], []
    for s in range(SPEAKERS):
        for _ in range(3 + int(rng.integers(0, 7))):
            speaker.append(s)
            rows.append(centers[s] + 1.6 * rng.standard_normal(E))
    X = np.asarray(rows, dtype=np.float32)
    speaker = np.asarray(speaker, np.int32)
    utterances = [{'speaker_key': f'set_spk{s:02d}'} for s in speaker]
    pairs = ref.generate_speaker_pairs(utterances)
    dist = ref.compute_distance_matrix(X, 'cosine', 1)
    res = ref.evaluate_speaker_verification(pairs, dist, 'cosine', 1)
    y_true, y_scores = np.asarray(res['y_true']), np.asarray(res['y_scores'], np.float64)

    def metrics(scores):
        fpr, tpr, _ = ref.roc_curve(y_true, scores)
        return {'eer': float(ref.compute_eer(y_true, scores)[0]), 'min_dcf': float(ref.compute_mindcf(y_true, scores)),
                'auc': float(ref.auc(fpr, tpr))}
    sign = np.where(y_true == 1, -1.0, 1.0)
    worse, better = metrics(y_scores + SHIFT * sign), metrics(y_scores - SHIFT * sign)
    own = {k: res[k] for k in ('eer', 'min_dcf', 'auc')}
    interval = {'eer': [better['eer'], worse['eer']], 'min_dcf': [better['min_dcf'], worse['min_dcf']],
                'auc': [worse['auc'], better['auc']]}
    for k, (lo, hi) in interval.items():
        assert lo <= own[k] <= hi, (k, lo, own[k], hi)
        assert hi - lo <= 0.05, (k, lo, hi)
    assert 0.02 < own['eer'] < 0.45, own

    np.savez_compressed(os.path.join(HERE, 'verif_golden.npz'), embeddings=X, speaker=speaker,
                        pairs=np.asarray(pairs, np.int64))
    meta = {'speakers': SPEAKERS, 'e': E, 'seed': SEED, 'shift': SHIFT, 'n_utterances': int(len(X)),
            'n_target_pairs': int((y_true == 1).sum()), 'n_non_target_pairs': int((y_true == 0).sum()),
            'reference': own, 'eer_threshold': res['eer_threshold'], 'interval': interval}
    with open(os.path.join(HERE, 'verif_golden.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print(json.dumps(meta, indent=1))


if __name__ == '__main__':
    main()
