"""The EER search and the minDCF branch and bound of speakerlab/utils/verification_analysis.py against
a numpy-backed digits primitive, checked with the brute force of tests/verif_oracle.py: integers
exactly, floats to 1e-12 relative from the same integers through the same formula.  On tie-free
scores the results are also those of score_metrics; with ties their distance to score_metrics is at
most (largest tie multiplicity) / min(n_tgt, n_non), computed from the data."""
import numpy as np
import pytest

from speakerlab.utils import score_metrics as sm
from speakerlab.utils import verification_analysis as va

import verif_oracle as vo


def two_class(seed, n_tgt=700, n_non=2500, sep=1.2):
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.normal(0.15 * sep + 0.3, 0.12, n_tgt), rng.normal(0.05, 0.1, n_non)]).astype(np.float32)
    c = np.concatenate([np.ones(n_tgt, np.int64), np.zeros(n_non, np.int64)])
    return np.clip(s, -1, 1), c


def tied(seed):
    """About 50 distinct values; value 0.26 straddles the crossing, value 0.5 holds the cost minimum."""
    rng = np.random.default_rng(seed)
    grid = np.round(np.linspace(-0.2, 0.76, 49), 2).astype(np.float32)
    tgt = rng.choice(grid[grid > 0.1], 900)
    non = rng.choice(grid[grid < 0.45], 3000)
    s = np.concatenate([tgt, non, np.full(200, 0.26, np.float32), np.full(300, 0.26, np.float32),
                        np.full(40, 0.5, np.float32), np.full(3, 0.5, np.float32)]).astype(np.float32)
    c = np.concatenate([np.ones(900), np.zeros(3000), np.ones(200), np.zeros(300), np.ones(40), np.zeros(3)]).astype(np.int64)
    return s, c


def run(scores, classes, **kw):
    keys = va.keys_of_scores(scores)
    digits = va.CountingDigits(va.host_digits(keys, classes))
    return keys, va.eer_search(digits), va.min_dcf_search(digits, **kw), digits


def score_metrics_values(scores, classes, p_target, c_miss=1, c_fa=1):
    fnr, fpr = sm.compute_pmiss_pfa_rbst(scores.astype(np.float64), classes)
    return sm.compute_eer(fnr, fpr), sm.compute_c_norm(fnr, fpr, p_target, c_miss, c_fa)


def test_key_map_orders_floats_and_merges_zeros():
    vals = np.array([-1.0, -1e-30, -0.0, 0.0, 1e-30, 0.5, 1.0], np.float32)
    k = va.keys_of_scores(vals)
    assert k[2] == k[3] and np.all(np.diff(k.astype(np.int64)) >= 0) and len(np.unique(k)) == 6
    assert np.array_equal(va.bits_of_key(k).view(np.float32)[[0, 1, 3, 4, 5, 6]], vals[[0, 1, 3, 4, 5, 6]])
    assert va.score_of_key(int(k[2])) == 0.0 and not np.signbit(va.score_of_key(int(k[2])))


@pytest.mark.parametrize('p_target', [0.01, 0.5])
@pytest.mark.parametrize('seed', [1, 2])
def test_random_scores(seed, p_target):
    scores, classes = two_class(seed)
    keys, eer, dcf, digits = run(scores, classes, p_target=p_target)
    assert eer['eer'] > 0 and digits.passes <= 4 + 64
    vo.check_against_brute(eer, dcf, vo.brute(keys, classes, p_target))
    if len(np.unique(keys)) == len(keys):           # tie-free: score_metrics itself
        ref_eer, ref_dcf = score_metrics_values(scores, classes, p_target)
        assert abs(eer['eer'] - ref_eer) <= 1e-12 * ref_eer and abs(dcf['min_dcf'] - ref_dcf) <= 1e-12 * ref_dcf


def test_tie_free_equals_score_metrics():
    rng = np.random.default_rng(7)
    scores = (rng.permutation(4000).astype(np.float32) / 4000 - 0.3).astype(np.float32)   # distinct by construction
    classes = (scores + rng.normal(0, 0.25, 4000) > 0.35).astype(np.int64)
    keys, eer, dcf, _ = run(scores, classes, p_target=0.01)
    assert len(np.unique(keys)) == len(keys)
    ref_eer, ref_dcf = score_metrics_values(scores, classes, 0.01)
    assert abs(eer['eer'] - ref_eer) <= 1e-12 * ref_eer
    assert abs(dcf['min_dcf'] - ref_dcf) <= 1e-12 * ref_dcf
    assert va.score_of_key(eer['key']) == sm.compute_eer(*sm.compute_pmiss_pfa_rbst(scores, classes), scores)[1]


@pytest.mark.parametrize('p_target', [0.01, 0.5])
def test_heavy_ties(p_target):
    scores, classes = tied(3)
    keys, eer, dcf, _ = run(scores, classes, p_target=p_target)
    want = vo.brute(keys, classes, p_target)
    assert len(np.unique(keys)) <= 50 and want['max_tie'] >= 500
    # the tie group of 0.26 holds the crossing: strictly FNR < FPR before it, FNR >= FPR at its end
    assert va.score_of_key(eer['key']) == np.float32(0.26)
    both = [np.sum((scores == np.float32(0.26)) & (classes == c)) for c in (0, 1)]
    assert min(both) >= 200
    vo.check_against_brute(eer, dcf, want)
    # distance to score_metrics (which sees the points inside the tie groups too)
    ref_eer, ref_dcf = score_metrics_values(scores, classes, p_target)
    tie_bound = want['max_tie'] / min(want['n_tgt'], want['n_non'])
    assert abs(eer['eer'] - ref_eer) <= tie_bound
    print(f'p_target {p_target}: EER {eer["eer"]:.6f} vs {ref_eer:.6f}, minDCF {dcf["min_dcf"]:.6f} vs {ref_dcf:.6f}, '
          f'tie bound {tie_bound:.6f}')
    assert abs(dcf['min_dcf'] - ref_dcf) <= tie_bound


def test_tie_group_holds_the_cost_minimum():
    scores, classes = tied(3)
    keys = va.keys_of_scores(scores)
    # a p_target at which the cheapest point is the end of a tie group populated by both classes
    found = False
    for p_target in (0.5, 0.3, 0.2, 0.1, 0.05, 0.01):
        want = vo.brute(keys, classes, p_target)
        sel = keys == np.uint32(want['dcf_key'])
        if sel.sum() > 1 and classes[sel].min() != classes[sel].max():
            found = True
            _, eer, dcf, _ = run(scores, classes, p_target=p_target)
            vo.check_against_brute(eer, dcf, want)
    assert found


def test_crossing_at_the_lowest_score():
    # the lowest score is a tie group that already holds most targets: x1 is the first point, x2 the stand-in
    scores = np.concatenate([np.full(60, -0.5), np.full(5, -0.5), np.linspace(0.0, 0.9, 40)]).astype(np.float32)
    classes = np.concatenate([np.ones(60), np.zeros(5), np.ones(10), np.zeros(30)]).astype(np.int64)
    keys, eer, dcf, _ = run(scores, classes, p_target=0.5)
    want = vo.brute(keys, classes, 0.5)
    assert want['x1'] == 0 and (eer['miss2'], eer['fa2']) == (0, want['n_non'])
    vo.check_against_brute(eer, dcf, want)


def test_reject_everything_is_optimal():
    scores, classes = two_class(5, sep=0.2)
    scores, classes = np.append(scores, np.float32(1.0)), np.append(classes, 0)   # the top score is a non-target
    keys, eer, dcf, _ = run(scores, classes, p_target=0.01, c_miss=1, c_fa=1000)
    want = vo.brute(keys, classes, 0.01, 1, 1000)
    assert want['dcf_fa'] == 0 and want['dcf_key'] == int(keys.max()) and want['dcf_miss'] == want['n_tgt']
    vo.check_against_brute(eer, dcf, want)


@pytest.mark.parametrize('p_target', [0.01, 0.5])
def test_pass_budget_of_one_is_reported_inexact(p_target):
    scores, classes = two_class(11)
    keys = va.keys_of_scores(scores)
    dcf = va.min_dcf_search(va.host_digits(keys, classes), p_target=p_target, max_passes=1)
    want = vo.brute(keys, classes, p_target)
    assert dcf['exact'] is False and dcf['passes'] == 1
    assert dcf['bound'] <= want['min_dcf'] <= dcf['min_dcf']
    # the best point found is a real operating point
    u, miss, fa, *_ = vo.operating_points(keys, classes)
    assert (dcf['miss'], dcf['fa']) in set(zip(miss.tolist(), fa.tolist()))


def test_empty_class_raises_before_any_pass():
    calls = []

    def digits(level, prefixes):
        calls.append(level)
        return np.zeros((len(prefixes), 2, 256), np.int64)
    scores = np.linspace(0, 1, 10).astype(np.float32)
    for classes in (np.zeros(10, np.int64), np.ones(10, np.int64)):
        with pytest.raises(ValueError):
            va.analyze(digits, va.host_moments(scores, classes))
    assert calls == []


def test_analyze_end_to_end_on_the_stand_in():
    scores, classes = two_class(4)
    keys = va.keys_of_scores(scores)
    rep = va.analyze(va.host_digits(keys, classes), va.host_moments(scores, classes))
    want = vo.brute(keys, classes, 0.01)
    assert rep['exact'] and rep['eer_key'] == want['eer_key'] and rep['min_dcf_point']['key'] == want['dcf_key']
    assert rep['eer_counts'] == dict(miss1=want['miss1'], fa1=want['fa1'], miss2=want['miss2'], fa2=want['fa2'])
    # AUC bounds bracket the exact pair count with ties at one half
    t, n = scores[classes == 1].astype(np.float64), scores[classes == 0].astype(np.float64)
    exact = ((t[:, None] > n[None, :]).sum() + 0.5 * (t[:, None] == n[None, :]).sum()) / (len(t) * len(n))
    assert rep['auc_lo'] <= exact <= rep['auc_hi'] and rep['auc_gap'] < 0.02
    assert rep['auc'] == 0.5 * (rep['auc_lo'] + rep['auc_hi'])
    assert rep['passes']['eer'] == 4 and rep['passes']['total'] == rep['passes']['digits'] + 2
    assert len(rep['fpr']) == 257 and rep['fpr'][0] == 0 and rep['fpr'][-1] == 1 and rep['tpr'][-1] == 1
