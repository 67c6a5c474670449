"""Pair-cosine statistics of the single-speaker check (``speakerlab/bin/check_single_speaker.py``).

A file is taken for single-speaker when the smallest cosine between the embeddings of any two of
its speech segments reaches a threshold.  ``pair_stats`` computes every file's pair cosines, their
minimum and mean on the device in one call (``_hip.pair_cosine_stats``) and copies the result back
once; ``pair_stats_host`` is the float64 numpy restatement tests compare it with.  Pairs are kept
in condensed order, ``(0, 1), (0, 2), ..., (1, 2), ...``: the order of ``np.triu_indices(n, 1)``.
"""
import numpy as np

RESULT_KEYS = ('wav_path', 'num_segments', 'segments', 'threshold', 'min_pairwise_cosine', 'mean_pairwise_cosine',
               'is_single_speaker', 'pairwise_similarities')


def pair_count(n):
    """Pairs of ``n`` rows."""
    n = int(n)
    return n * (n - 1) // 2 if n > 1 else 0


def pair_offsets(sizes):
    """Where each group's pairs start in the condensed array of a batch: the prefix sums of
    ``pair_count`` over the group sizes, with the total last (``_hip.pair_cosine_sizes`` on the
    groups' row offsets gives the same list)."""
    out = [0]
    for n in sizes:
        out.append(out[-1] + pair_count(n))
    return out


def condensed_to_ij(n, p):
    """Rows (i, j), i < j, of condensed pair index ``p`` of ``n`` rows.  Row i starts at
    ``i (2n - i - 1) / 2``; the float root proposes i and integer steps settle it."""
    n, p = int(n), int(p)
    if not 0 <= p < pair_count(n):
        raise ValueError(f'condensed_to_ij: pair {p} outside the {pair_count(n)} pairs of {n} rows')

    def start(i):
        return i * (2 * n - i - 1) // 2

    b = 2 * n - 1
    i = min(max(int((b - (b * b - 8 * p) ** 0.5) / 2), 0), n - 2)
    while i > 0 and start(i) > p:
        i -= 1
    while i < n - 2 and start(i + 1) <= p:
        i += 1
    return i, p - start(i) + i + 1


def ij_to_condensed(n, i, j):
    """Inverse of ``condensed_to_ij``."""
    n, i, j = int(n), int(i), int(j)
    if not 0 <= i < j < n:
        raise ValueError(f'ij_to_condensed: need 0 <= i < j < n, got {(i, j, n)}')
    return i * (2 * n - i - 1) // 2 + j - i - 1


def _stats_of(cos, threshold):
    """One group's entry from its condensed cosines (None: fewer than two rows)."""
    if cos is None or len(cos) == 0:
        return {'min': 1.0, 'mean': 1.0, 'argmin': -1, 'n_below': 0}
    return {'min': float(cos.min()), 'mean': float(cos.mean()), 'argmin': int(cos.argmin()),
            'n_below': int((cos < threshold).sum())}


def pair_stats_host(list_of_embeddings, threshold):
    """float64 numpy form of ``pair_stats``: for every [n, E] array a dict with ``cos`` (float64
    condensed pair cosines), ``min``, ``mean``, ``argmin`` (first minimum) and ``n_below`` (cosines
    strictly below ``threshold``).  cos(i, j) = <x_i, x_j> / (|x_i| |x_j|) with the norm of a zero
    row replaced by 1, so such a pair scores 0.  Fewer than two rows: min = mean = 1, argmin = -1,
    n_below = 0, no cosines."""
    out = []
    for emb in list_of_embeddings:
        x = np.zeros((0, 0)) if emb is None else np.asarray(emb, dtype=np.float64)
        n = len(x)
        if n < 2:
            out.append(dict(_stats_of(None, threshold), cos=np.zeros(0)))
            continue
        norm = np.sqrt((x * x).sum(axis=1))
        norm[norm == 0.0] = 1.0
        i, j = np.triu_indices(n, 1)
        cos = (x[i] * x[j]).sum(axis=1) / (norm[i] * norm[j])
        out.append(dict(_stats_of(cos, threshold), cos=cos))
    return out


def pair_stats(list_of_embeddings, threshold, want_cos=True):
    """The same statistics on the device, for all groups in one ``_hip.pair_cosine_stats`` call and
    one copy back.  ``list_of_embeddings``: one [n, E] float32 device tensor per group (None or an
    empty tensor for a group without rows), all on one device; or a pair ``(X, offsets)`` of the
    rows already back to back.  Returns one dict per group with float ``min`` / ``mean`` (the
    float32 results), ``argmin``, ``n_below`` and, with ``want_cos``, ``cos``: float32 numpy
    condensed cosines (absent otherwise)."""
    import torch
    from speakerlab import _hip
    if isinstance(list_of_embeddings, tuple):
        X, offsets = list_of_embeddings
        offsets = [int(v) for v in offsets]
    else:
        groups = [g for g in list_of_embeddings]
        rows = [g for g in groups if g is not None and g.shape[0] > 0]
        offsets = [0]
        for g in groups:
            offsets.append(offsets[-1] + (0 if g is None else int(g.shape[0])))
        if not rows:
            return [dict(_stats_of(None, threshold), **({'cos': np.zeros(0, np.float32)} if want_cos else {}))
                    for _ in groups]
        X = rows[0] if len(rows) == 1 else torch.cat(rows)
    G = len(offsets) - 1
    if G == 0:
        return []
    st = _hip.pair_cosine_stats(X, offsets, threshold, want_cos=want_cos)
    # one buffer, one copy: the statistics (bit patterns kept) in front of the cosines
    parts = [st.min.view(torch.int32), st.mean.view(torch.int32), st.argmin.view(torch.int32),
             st.n_below.view(torch.int32)]
    if want_cos:
        parts.append(st.cos.view(torch.int32))
    host = torch.cat(parts).cpu().numpy()
    mn, mean = host[:G].view(np.float32), host[G:2 * G].view(np.float32)
    argmin, below = host[2 * G:4 * G].view(np.int64), host[4 * G:6 * G].view(np.int64)
    cos = host[6 * G:].view(np.float32)
    out = []
    for g in range(G):
        d = {'min': float(mn[g]), 'mean': float(mean[g]), 'argmin': int(argmin[g]), 'n_below': int(below[g])}
        if want_cos:
            d['cos'] = cos[st.pair_offsets[g]:st.pair_offsets[g + 1]]
        out.append(d)
    return out


def make_result(wav_path, segments, threshold, stats, want_pairs=True):
    """The reference tool's result dict for one file from its VAD segments ``[[start, stop], ...]``
    (seconds) and its entry of ``pair_stats``.  ``is_single_speaker`` is ``min >= threshold`` in
    float32, the comparison the kernel counts ``n_below`` with."""
    segs = [{'start': float(s), 'stop': float(e)} for s, e in segments]
    res = {
        'wav_path': wav_path,
        'num_segments': len(segs),
        'segments': segs,
        'threshold': float(threshold),
        'min_pairwise_cosine': float(stats['min']),
        'mean_pairwise_cosine': float(stats['mean']),
        'is_single_speaker': bool(np.float32(stats['min']) >= np.float32(threshold)),
    }
    if want_pairs:
        pairs = []
        cos = stats.get('cos')
        if cos is not None and len(cos):
            i, j = np.triu_indices(len(segs), 1)
            pairs = [{'i': int(a), 'j': int(b), 'cosine': float(v), 'seg_i': segs[a], 'seg_j': segs[b]}
                     for a, b, v in zip(i, j, cos)]
        res['pairwise_similarities'] = pairs
    return res
