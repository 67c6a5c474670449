"""The similarity analysis (numpy path) against the reference's compute_speaker_similarities_fast.py
on the fixture of tests/golden/make_sim_golden.py: 160 seeded unit-normal embeddings, E = 64,
top_k = 5.

Float fields agree to 4 * d_ref + 2e-6: d_ref is the reference's own float32 summation error,
measured by the maker (2.9e-9 for this fixture), 2e-6 the affinity kernel's parity bound; the
tolerance is 2.012e-6.  Rankings are compared position by position.  A position is skipped only
when it differs and its score is within the tolerance of a neighbour's, where the reference's order
is unspecified; skipped positions are at most 1 % of the positions compared.  (67 of the 2800
positions are eligible, 2.4 %: the cap is on what is skipped.)  Histogram and threshold counts may
differ from the reference's only by values within the tolerance of an edge or a threshold; those
values are counted and exactly that many are allowed."""
import json
import os

import numpy as np
import pytest

from speakerlab.utils import similarity_analysis as sa

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def golden():
    g = dict(np.load(os.path.join(HERE, 'golden', 'sim_golden.npz')))
    with open(os.path.join(HERE, 'golden', 'sim_golden.json')) as f:
        meta = json.load(f)
    tol = 4 * meta['d_ref'] + meta['affinity_parity']
    keys = [f'spk{i:03d}' for i in range(meta['n'])]
    rep = sa.analyze(g['embeddings'], keys, top_k=meta['top_k'], n_extreme=1000, thresholds=tuple(meta['thresholds']))
    return g, meta, tol, keys, rep


def test_tolerance_comes_from_the_reference(golden):
    g, meta, tol, _, _ = golden
    assert meta['affinity_parity'] == 2e-6 and 0 < meta['d_ref'] < 1e-6 and tol == 4 * meta['d_ref'] + 2e-6
    assert meta['unsure_positions'] <= 0.01 * meta['positions_compared']
    assert g['embeddings'].shape == (160, 64) and g['embeddings'].dtype == np.float32


def test_statistics_and_quartiles(golden):
    g, meta, tol, keys, rep = golden
    for name in ('upper_triangular_statistics', 'similarity_statistics'):
        for key, want in meta[name].items():
            got = rep[name][key]
            if isinstance(want, float):
                assert abs(got - want) <= tol, (name, key, got, want)
            else:
                assert got == want, (name, key)
    tops = rep['speaker_top_similarities']
    for field, arr in (('mean_similarity_to_others', 'row_mean'), ('max_similarity_to_others', 'row_max'),
                       ('min_similarity_to_others', 'row_min')):
        got = np.array([tops[k][field] for k in keys])
        assert np.abs(got - g[arr]).max() <= tol, field


def _compare_ranking(got_ids, got_scores, ref_ids, ref_scores, tol, beyond=None):
    """(positions skipped, positions compared): identities position by position; a differing position
    must be within tol of a neighbour's score in the reference's list."""
    ref_scores = np.asarray(ref_scores, np.float64)
    assert len(got_ids) == len(ref_ids)
    assert np.abs(np.asarray(got_scores, np.float64) - ref_scores).max() <= tol
    ext = np.concatenate([[np.inf], ref_scores, [np.inf if beyond is None else beyond]])
    close = (np.abs(ext[1:-1] - ext[:-2]) <= tol) | (np.abs(ext[1:-1] - ext[2:]) <= tol)
    skipped = 0
    for r, (a, b) in enumerate(zip(got_ids, ref_ids)):
        if a != b:
            assert close[r], (r, a, b)
            skipped += 1
    return skipped, len(ref_ids)


def test_rankings(golden):
    g, meta, tol, keys, rep = golden
    index = {k: i for i, k in enumerate(keys)}
    S = sa.host_cosine(g['embeddings']).astype(np.float64)
    srt = np.sort(S[np.triu_indices(160, 1)])
    skipped = compared = 0
    ext = rep['extreme_similarity_pairs']
    for name, key in (('most', 'most_similar_pairs'), ('least', 'least_similar_pairs')):
        got = [(index[p['speaker1']], index[p['speaker2']]) for p in ext[key]]
        assert [p['rank'] for p in ext[key]] == list(range(1, 1001))
        n = len(got)
        s, c = _compare_ranking(got, [p['similarity'] for p in ext[key]], list(zip(g[name + '_i'], g[name + '_j'])),
                                g[name + '_score'], tol, srt[-n - 1] if name == 'most' else srt[n])
        skipped, compared = skipped + s, compared + c
    tops = rep['speaker_top_similarities']
    for i, k in enumerate(keys):
        t = tops[k]['top_similarities']
        s, c = _compare_ranking([index[e['speaker']] for e in t], [e['similarity'] for e in t], list(g['top_index'][i]),
                                g['top_score'][i], tol, np.sort(np.delete(S[i], i))[-6])
        skipped, compared = skipped + s, compared + c
    assert compared == meta['positions_compared'] == 2800
    assert skipped <= 0.01 * compared, (skipped, compared)


def test_histogram_and_threshold_counts(golden):
    g, meta, tol, keys, rep = golden
    vals = sa.host_cosine(g['embeddings'])[np.triu_indices(160, 1)].astype(np.float64)
    dist = rep['similarity_distribution']
    assert np.abs(np.array(dist['bins']) - g['hist_edges']).max() <= tol
    near = sum(int((np.abs(vals - e) <= tol).sum()) for e in g['hist_edges'][1:-1])
    # a value near an edge moves one count out of a bin and into its neighbour
    assert np.abs(np.array(dist['counts']) - g['hist_counts']).sum() <= 2 * near
    assert sum(dist['counts']) == g['hist_counts'].sum() == 12720
    got = np.array([rep['threshold_statistics'][f'threshold_{t}']['count'] for t in meta['thresholds']])
    for t, a, b in zip(meta['thresholds'], got, g['threshold_counts']):
        assert abs(int(a) - int(b)) <= int((np.abs(vals - t) <= tol).sum()), t
