"""Speaker x speaker similarity analysis of a corpus of embeddings: what the reference's
egs/extract_and_comclude_similarities/compute_speaker_similarities_fast.py reports about the N x N
cosine matrix -- statistics of the upper triangle, the most and least similar pairs, every speaker's
nearest speakers, a histogram, counts at thresholds, quartiles -- from selections and reductions
alone, so that on the device the matrix is never stored (``_hip.cosine_rows_topk``,
``_hip.cosine_triu_stats``).

Definitions, the same on both paths:
  * scores are float32 cosines (sklearn semantics: a zero-norm row divides by 1); -0.0 counts as +0.0;
  * a speaker's nearest: the other speakers by score descending, then index ascending;
  * most similar pairs: the pairs i < j by score descending, then (i, j) ascending; least similar: by
    score ascending, then (i, j) ascending (the reference's argsort leaves the order of equal scores
    unspecified);
  * sums are float64 sums of the float32 scores; threshold counts compare in float32;
  * the histogram has ``nbins`` equal bins over [min, max] of the pairs, edges
    ``np.linspace(float64 min, float64 max, nbins + 1)``; bin b holds edges[b] <= s < edges[b + 1], the
    last bin also s == max (``np.histogram``'s rule);
  * quartiles follow numpy's linear interpolation, computed in float64 from the two neighbouring
    order statistics.

``analyze`` without a device runs the numpy statement of these definitions on a host score matrix;
it is what the device path is tested against.
"""
import math

import numpy as np

THRESHOLDS = (0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9,
              0.95, 0.99)
MAX_TOP_K = 1024       # spk_cosine_rows_topk
MAX_EXTREME = 4096     # spk_cosine_triu_stats
QUANTILES = (0.25, 0.5, 0.75)


def host_cosine(x):
    """float32 [N, N] cosine matrix of the rows of ``x`` on the host (a zero-norm row divides by 1)."""
    x = np.asarray(x, dtype=np.float32)
    n = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    n[n == 0] = 1.0
    xn = (x / n[:, None]).astype(np.float32)
    return (xn @ xn.T).astype(np.float32)


def quantile_ranks(P):
    """For each of QUANTILES over P values: (lower rank, upper rank, weight of the upper), numpy's
    linear rule; and the ascending distinct ranks to ask for."""
    pos = []
    for q in QUANTILES:
        v = q * (P - 1)
        lo = int(math.floor(v))
        hi = min(lo + 1, P - 1)
        pos.append((lo, hi, v - lo))
    return pos, sorted({r for lo, hi, _ in pos for r in (lo, hi)})


def _interp(a, b, t):
    a, b = float(a), float(b)
    return a + (b - a) * t


def pair_of_condensed(q, N):
    """(i, j) of the condensed upper-triangle indices ``q`` (row-major, np.triu_indices(N, 1) order)."""
    i_all = np.arange(N, dtype=np.int64)
    starts = i_all * (2 * N - i_all - 1) // 2
    i = np.searchsorted(starts, q, side='right') - 1
    return i, q - starts[i] + i + 1


def raw_from_scores(S, top_k, n_extreme=1000, nbins=50, thresholds=THRESHOLDS, edges=None, ranks=None):
    """The raw results (the structure ``raw_on_device`` gives) from a float32 score matrix, in numpy."""
    S = np.asarray(S, dtype=np.float32) + np.float32(0)            # -0.0 -> +0.0
    N = S.shape[0]
    k = int(top_k)
    top_s = np.full((N, k), -np.inf, np.float32)
    top_i = np.full((N, k), -1, np.int64)
    rsum, rsq = np.zeros(N), np.zeros(N)
    rmin, rmax = np.full(N, np.nan, np.float32), np.full(N, np.nan, np.float32)
    for i in range(N):
        cols = np.concatenate([np.arange(i), np.arange(i + 1, N)])
        o = S[i, cols]
        order = np.argsort(-o, kind='stable')[:k]                  # score descending, column ascending
        top_s[i, :len(order)] = o[order]
        top_i[i, :len(order)] = cols[order]
        o64 = o.astype(np.float64)
        rsum[i], rsq[i] = o64.sum(), (o64 * o64).sum()
        if N > 1:
            rmin[i], rmax[i] = o.min(), o.max()
    rows = dict(top_scores=top_s, top_index=top_i, sum=rsum, sumsq=rsq, min=rmin, max=rmax,
                self=np.diagonal(S).copy())

    P = N * (N - 1) // 2
    vals = np.concatenate([S[i, i + 1:] for i in range(N)]) if N > 1 else np.zeros(0, np.float32)
    v64 = vals.astype(np.float64)
    if ranks is None:
        ranks = quantile_ranks(P)[1] if P else []
    ranks = [int(r) for r in ranks]
    tri = dict(count=P, sum=float(v64.sum()) if P else float('nan'), sumsq=float((v64 * v64).sum()) if P else float('nan'),
               min=vals.min() if P else np.float32('nan'), max=vals.max() if P else np.float32('nan'),
               count_ge=np.array([int((vals >= np.float32(t)).sum()) for t in thresholds], np.int64),
               order_stats=np.partition(vals, ranks)[ranks] if ranks else np.zeros(0, np.float32))
    if nbins > 0:
        if edges is None:
            lo, hi = (float(tri['min']), float(tri['max'])) if P else (0.0, 1.0)
            if lo == hi:
                lo, hi = lo - 0.5, hi + 0.5
            edges = np.linspace(lo, hi, nbins + 1)
        edges = np.asarray(edges, dtype=np.float64)
        tri['edges'] = edges
        tri['hist'] = np.histogram(v64, bins=edges)[0].astype(np.int64)
    n = min(int(n_extreme), P)
    if n_extreme > 0:
        for name, sign in (('most', -1), ('least', 1)):
            if n == 0:
                tri[name] = (np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
                continue
            w = vals * np.float32(sign)                            # ascending in w = the wanted order
            cut = np.partition(w, n - 1)[n - 1]
            beyond = np.flatnonzero(w < cut)
            ties = np.flatnonzero(w == cut)[:n - len(beyond)]      # the first copies in (i, j) order
            idx = np.concatenate([beyond, ties])
            idx = idx[np.lexsort((idx, w[idx]))]
            i, j = pair_of_condensed(idx, N)
            tri[name] = (vals[idx], i, j)
    return dict(n=N, rows=rows, triu=tri)


def raw_on_device(embeddings, top_k, n_extreme, nbins, thresholds, device):
    import torch
    from speakerlab import _hip
    if not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(f'top_k must be in 1..{MAX_TOP_K} on the device, got {top_k}')
    if not 0 <= n_extreme <= MAX_EXTREME:
        raise ValueError(f'n_extreme must be in 0..{MAX_EXTREME} on the device, got {n_extreme}')
    x = torch.as_tensor(np.ascontiguousarray(embeddings, dtype=np.float32)).to(device)
    N = x.shape[0]
    P = N * (N - 1) // 2
    rows = {k: v.cpu().numpy() for k, v in _hip.cosine_rows_topk(x, top_k).items()}
    tri = _hip.cosine_triu_stats(x, thresholds=thresholds, ranks=quantile_ranks(P)[1] if P else [],
                                 n_ext=n_extreme, nbins=nbins)
    return dict(n=N, rows=rows, triu=tri)


def reports(raw, keys, top_k, thresholds=THRESHOLDS):
    """The reference's dicts (its JSON files' contents, its keys) from the raw results."""
    N, rows, tri = raw['n'], raw['rows'], raw['triu']
    keys = list(keys)
    P = tri['count']
    # the whole matrix with its diagonal, from the rows' moments
    total = float(rows['sum'].sum() + rows['self'].astype(np.float64).sum())
    total_sq = float(rows['sumsq'].sum() + (rows['self'].astype(np.float64) ** 2).sum())
    mean_all = total / (N * N)
    lows = np.concatenate([rows['min'][~np.isnan(rows['min'])], rows['self']])
    highs = np.concatenate([rows['max'][~np.isnan(rows['max'])], rows['self']])
    stats = {'total_speakers': N, 'similarity_matrix_shape': [N, N], 'mean_similarity': mean_all,
             'std_similarity': math.sqrt(max(total_sq / (N * N) - mean_all * mean_all, 0.0)),
             'min_similarity': float(lows.min()), 'max_similarity': float(highs.max())}

    out = {'similarity_statistics': stats, 'speaker_keys_mapping': {i: k for i, k in enumerate(keys)}}
    if P == 0:
        return out
    mean = tri['sum'] / P
    pos, asked = quantile_ranks(P)
    at = {r: float(v) for r, v in zip(asked, tri['order_stats'])}
    q25, med, q75 = (_interp(at[lo], at[hi], t) for lo, hi, t in pos)
    upper = {'total_pairs': int(P), 'mean_similarity': mean,
             'std_similarity': math.sqrt(max(tri['sumsq'] / P - mean * mean, 0.0)),
             'min_similarity': float(tri['min']), 'max_similarity': float(tri['max']), 'median_similarity': med,
             'q25_similarity': q25, 'q75_similarity': q75}

    def pairs(sel):
        s, i, j = sel
        return [{'rank': r + 1, 'speaker1': keys[int(i[r])], 'speaker2': keys[int(j[r])], 'similarity': float(s[r])}
                for r in range(len(s))]

    none = (np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))   # n_extreme == 0
    most, least = pairs(tri.get('most', none)), pairs(tri.get('least', none))
    extreme = {'most_similar_pairs': most, 'least_similar_pairs': least,
               'metadata': {'num_most_similar': len(most), 'num_least_similar': len(least),
                            'total_pairs_analyzed': int(P)}}
    tops = {}
    for i, key in enumerate(keys):
        have = int((rows['top_index'][i] >= 0).sum())
        tops[key] = {'top_similarities': [{'speaker': keys[int(rows['top_index'][i, r])],
                                           'similarity': float(rows['top_scores'][i, r])} for r in range(have)],
                     'mean_similarity_to_others': float(rows['sum'][i]) / (N - 1),
                     'max_similarity_to_others': float(rows['max'][i]),
                     'min_similarity_to_others': float(rows['min'][i])}
    dist = {'bins': [float(e) for e in tri['edges']], 'counts': [int(c) for c in tri['hist']]}
    thr = {f'threshold_{t}': {'count': int(c), 'percentage': float(int(c) / P * 100)}
           for t, c in zip(thresholds, tri['count_ge'])}
    top_bin = int(np.argmax(tri['hist']))
    summary = {'analysis_info': {'total_speakers': N, 'total_speaker_pairs': int(P), 'top_k_analyzed': int(top_k),
                                 'extreme_pairs_analyzed': {'most_similar_count': len(most),
                                                            'least_similar_count': len(least)}},
               'upper_triangular_stats': upper,
               'extreme_pairs_summary': {'most_similar_top1': most[0] if most else None,
                                         'least_similar_top1': least[0] if least else None,
                                         'total_extreme_pairs': len(most) + len(least)},
               'threshold_statistics': thr,
               'distribution_info': {'histogram_bins': len(dist['counts']),
                                     'most_frequent_range': f"{dist['bins'][top_bin]:.3f} - {dist['bins'][top_bin + 1]:.3f}"}}
    out.update({'upper_triangular_statistics': upper, 'extreme_similarity_pairs': extreme,
                'speaker_top_similarities': tops, 'similarity_distribution': dist, 'threshold_statistics': thr,
                'analysis_summary': summary})
    return out


def analyze(embeddings, keys, top_k=100, n_extreme=1000, nbins=50, thresholds=THRESHOLDS, device=None):
    """The analysis of ``embeddings`` [N, E] (one row per entry of ``keys``) as plain dicts named after
    the reference's output files.  With ``device`` (a ROCm device) the kernels run and the matrix is
    never stored; without, the numpy statement of the same definitions on a host matrix."""
    embeddings = np.asarray(embeddings, dtype=np.float32)
    if embeddings.ndim != 2 or embeddings.shape[0] != len(keys) or embeddings.shape[0] < 1:
        raise ValueError(f'expected [N, E] embeddings for {len(keys)} keys, got {embeddings.shape}')
    if top_k < 1 or n_extreme < 0 or nbins < 1:
        raise ValueError('top_k and nbins must be at least 1, n_extreme at least 0')
    if device is None:
        raw = raw_from_scores(host_cosine(embeddings), top_k, n_extreme, nbins, thresholds)
    else:
        raw = raw_on_device(embeddings, top_k, n_extreme, nbins, thresholds, device)
    return reports(raw, keys, top_k, thresholds)
