"""Exact verification metrics (EER, minDCF, AUC bounds) over ALL N (N - 1) / 2 labelled pairs of an
embedding set, from two device primitives that never store the N x N score matrix
(``_hip.cosine_verif_digits`` and ``_hip.cosine_verif_moments``).

Everything is decided on integer counts.  A pair's score is the device's own float32 cosine; its key
is the order-preserving 32-bit image of that float (``key_of_bits``; -0.0 shares the key of +0.0).
With n_tgt / n_non the class totals, an operating point is a distinct key u present among the pairs
and rejects every pair with key <= u:

    miss(u) = target pairs with key <= u        FNR = miss / n_tgt
    fa(u)   = non-target pairs with key > u     FPR = fa / n_non

These are the points ``score_metrics.compute_pmiss_pfa_rbst`` yields on tie-free scores; of a group
of tied scores only its last point exists.

The primitive is a callable ``digits(level, prefixes) -> int64 [n_prefix, 2, 256]``: entry [p, c, d]
counts the class-c pairs (c = 1 target) whose key agrees with prefixes[p] in its top ``level`` bytes
and whose next byte is d; up to 16 prefixes per call, one call = one pass over the pairs.  The
searches only ever see this callable, so they run unchanged on the numpy stand-in ``host_digits``.

* EER: FNR - FPR never decreases with u, so x1, the lowest point with FNR >= FPR, is found by four
  one-prefix passes, byte by byte.  x2, the point just below x1, has miss = targets below x1 and
  fa = n_non - non-targets below x1, which the same histograms give; when nothing lies below x1
  these are the accept-everything point (FNR 0, FPR 1).  The EER is ``score_metrics.compute_eer``'s
  interpolation between the two.
* minDCF: branch and bound over key prefixes, pure refinement (no pairs are collected on the
  device).  A prefix node holding keys [a, b] can hold nothing cheaper than
  c_miss p miss(< a) / n_tgt + c_fa (1 - p) fa(> b) / n_non; the highest key present in it is an
  operating point whose cost is known from the counts alone and serves as the incumbent.  Each
  pass refines up to 16 surviving nodes of one level, cheapest bound first, until every survivor is a
  full key.  Among equal costs the lowest key wins.  When ``max_passes`` runs out the result says
  ``exact=False`` and carries the lowest surviving bound: bound <= true minimum <= best.
* AUC: from per-class histograms, ``auc_lo`` counts the non-targets in bins below each target's bin,
  ``auc_hi`` adds those in the same bin; ``auc`` is their midpoint and ``auc_gap`` the difference.
"""
import numpy as np

MAX_PREFIXES = 16


def key_of_bits(bits):
    """uint32 float bits -> uint32 key with the order of the floats (-0.0 -> the key of +0.0)."""
    u = np.asarray(bits, dtype=np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def bits_of_key(key):
    k = np.asarray(key, dtype=np.uint32)
    return np.where((k & np.uint32(0x80000000)) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)


def keys_of_scores(scores):
    return key_of_bits(np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32))


def score_of_key(key):
    return float(bits_of_key(np.array([key], np.uint32)).view(np.float32)[0])


def host_digits(keys, classes):
    """The numpy stand-in of the device primitive over explicit (key uint32, class 0/1) pairs."""
    keys = np.asarray(keys, dtype=np.uint32)
    classes = np.asarray(classes).astype(np.int64)

    def digits(level, prefixes):
        prefixes = np.asarray(prefixes, dtype=np.uint32).reshape(-1)
        out = np.zeros((len(prefixes), 2, 256), np.int64)
        shift = 24 - 8 * level
        nxt = ((keys >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
        for p, pre in enumerate(prefixes):
            m = np.ones(len(keys), bool) if level == 0 else (keys >> np.uint32(32 - 8 * level)) == (pre >> np.uint32(32 - 8 * level))
            for c in (0, 1):
                out[p, c] = np.bincount(nxt[m & (classes == c)], minlength=256)
        return out
    return digits


def host_moments(scores, classes):
    """The numpy stand-in of ``_hip.cosine_verif_moments`` over explicit (score float32, class) pairs."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    classes = np.asarray(classes).astype(np.int64)

    def moments(edges=None):
        out = dict(count=np.zeros(2, np.int64), sum=np.zeros(2), sumsq=np.zeros(2),
                   min=np.full(2, np.nan, np.float32), max=np.full(2, np.nan, np.float32))
        if edges is not None:
            out['edges'] = np.asarray(edges, np.float64)
            out['hist'] = np.zeros((2, len(edges) - 1), np.int64)
        for c in (0, 1):
            s = scores[classes == c].astype(np.float64)
            out['count'][c] = len(s)
            out['sum'][c], out['sumsq'][c] = s.sum(), (s * s).sum()
            if len(s):
                out['min'][c], out['max'][c] = s.min(), s.max()
            if edges is not None:
                out['hist'][c] = np.histogram(s, bins=out['edges'])[0]
        return out
    return moments


class CountingDigits:
    """Wraps a primitive: counts its passes and remembers every (level, prefix) histogram it returned, so
    the searches that share it never ask twice."""

    def __init__(self, digits):
        self._digits, self.passes, self._seen = digits, 0, {}

    @staticmethod
    def _norm(level, prefix):
        return (level, 0 if level == 0 else int(prefix) >> (32 - 8 * level) << (32 - 8 * level))

    def known(self, level, prefix):
        return self._norm(level, prefix) in self._seen

    def __call__(self, level, prefixes):
        keys = [self._norm(level, p) for p in prefixes]
        todo = [k for k in dict.fromkeys(keys) if k not in self._seen]
        if todo:
            if len(todo) > MAX_PREFIXES:
                raise ValueError(f'at most {MAX_PREFIXES} prefixes per pass')
            got = np.asarray(self._digits(level, np.array([k[1] for k in todo], np.uint32)))
            if got.shape != (len(todo), 2, 256):
                raise ValueError(f'the digits primitive returned shape {got.shape}')
            self.passes += 1
            for k, h in zip(todo, got):
                self._seen[k] = h.astype(np.int64)
        return np.stack([self._seen[k] for k in keys])


def class_totals(digits):
    """(n_non, n_tgt) from the level-0 histograms."""
    h = digits(0, [0])[0]
    return int(h[0].sum()), int(h[1].sum())


def _check_totals(n_non, n_tgt):
    if n_tgt <= 0 or n_non <= 0:
        raise ValueError(f'verification metrics need target and non-target pairs (got {n_tgt} target, {n_non} '
                         f'non-target): every speaker has one utterance, or there is one speaker')


def eer_from_counts(miss1, fa1, miss2, fa2, n_tgt, n_non):
    """``score_metrics.compute_eer``'s interpolation between x1 = (miss1, fa1) and x2 = (miss2, fa2)."""
    fnr1, fpr1, fnr2, fpr2 = miss1 / n_tgt, fa1 / n_non, miss2 / n_tgt, fa2 / n_non
    a = (fnr1 - fpr1) / (fpr2 - fpr1 - (fnr2 - fnr1))
    return fnr1 + a * (fnr2 - fnr1)


def eer_search(digits, n_non=None, n_tgt=None):
    """x1 by four one-prefix passes.  Returns dict(eer, key, miss1, fa1, miss2, fa2, n_tgt, n_non)."""
    if n_non is None:
        n_non, n_tgt = class_totals(digits)
    _check_totals(n_non, n_tgt)
    prefix, below = 0, [0, 0]   # pairs per class strictly below the prefix's range
    for level in range(4):
        h = digits(level, [prefix])[0]
        cum = np.cumsum(h, axis=1)
        pick = None
        for d in np.flatnonzero(h[0] + h[1]):   # D at the end of bin d = D at its highest key; first d with D >= 0
            miss = below[1] + int(cum[1, d])
            fa = n_non - below[0] - int(cum[0, d])
            if miss * n_non >= fa * n_tgt:       # FNR >= FPR in integers
                pick = int(d)
                break
        if pick is None:
            raise RuntimeError('the digit histograms do not cover the crossing: the primitive is inconsistent')
        below = [below[c] + int(cum[c, pick]) - int(h[c, pick]) for c in (0, 1)]
        prefix |= pick << (24 - 8 * level)
        last = [int(h[0, pick]), int(h[1, pick])]
    miss1, fa1 = below[1] + last[1], n_non - below[0] - last[0]
    miss2, fa2 = below[1], n_non - below[0]
    return dict(eer=eer_from_counts(miss1, fa1, miss2, fa2, n_tgt, n_non), key=prefix, miss1=miss1, fa1=fa1,
                miss2=miss2, fa2=fa2, n_tgt=n_tgt, n_non=n_non)


def dcf_cost(miss, fa, n_tgt, n_non, p_target, c_miss=1, c_fa=1):
    """The detection cost of an operating point; monotone in miss and fa also in floating point."""
    return c_miss * p_target * (miss / n_tgt) + c_fa * (1 - p_target) * (fa / n_non)


def min_dcf_search(digits, p_target=0.01, c_miss=1, c_fa=1, max_passes=64, n_non=None, n_tgt=None):
    """Branch and bound for the cheapest operating point.  Returns dict(min_dcf (normalised as
    ``compute_c_norm``), cost, key, miss, fa, exact, bound (normalised; == min_dcf when exact), passes,
    key_level).  With ``exact=False`` ``key`` is the highest key of the best node found (its top
    ``key_level`` bytes are known), and bound <= true minimum <= min_dcf."""
    counter = digits if isinstance(digits, CountingDigits) else CountingDigits(digits)
    if n_non is None:
        n_non, n_tgt = class_totals(counter)
    _check_totals(n_non, n_tgt)
    cost = lambda miss, fa: dcf_cost(miss, fa, n_tgt, n_non, p_target, c_miss, c_fa)
    c_def = min(c_miss * p_target, c_fa * (1 - p_target))
    start = counter.passes
    # a node: (bound, prefix, level, non_below, tgt_below); its population is not needed
    nodes = [(cost(0, 0), 0, 0, 0, 0)]
    best_leaf = None                       # (cost, key, miss, fa)
    incumbent = None                       # (cost, prefix, level, miss, fa): the highest key of a node
    spent = 0

    def alive(node):
        b, prefix = node[0], node[1]
        if incumbent is not None and b > incumbent[0]:
            return False
        if best_leaf is not None and (b > best_leaf[0] or (b == best_leaf[0] and prefix > best_leaf[1])):
            return False
        return True

    while nodes:
        nodes = sorted(n for n in nodes if alive(n))
        if not nodes:
            break
        level = nodes[0][2]
        batch = [n for n in nodes if n[2] == level][:MAX_PREFIXES]
        fresh = any(not counter.known(level, n[1]) for n in batch)
        if fresh and spent >= max_passes:
            break
        taken = set(id(n) for n in batch)
        nodes = [n for n in nodes if id(n) not in taken]
        before = counter.passes
        hs = counter(level, [n[1] for n in batch])
        spent += counter.passes - before
        shift = 24 - 8 * level
        for (_, prefix, _, nb, tb), h in zip(batch, hs):
            cum = np.cumsum(h, axis=1)
            for d in np.flatnonzero(h[0] + h[1]):
                d = int(d)
                c_nb, c_tb = nb + int(cum[0, d]) - int(h[0, d]), tb + int(cum[1, d]) - int(h[1, d])
                miss_end, fa_end = tb + int(cum[1, d]), n_non - nb - int(cum[0, d])
                child = prefix | (d << shift)
                end_cost = cost(miss_end, fa_end)        # the cost at the child's highest key
                if incumbent is None or end_cost < incumbent[0]:
                    incumbent = (end_cost, child, level + 1, miss_end, fa_end)
                if level == 3:
                    if best_leaf is None or (end_cost, child) < best_leaf[:2]:
                        best_leaf = (end_cost, child, miss_end, fa_end)
                else:
                    nodes.append((cost(c_tb, fa_end), child, level + 1, c_nb, c_tb))
    nodes = [n for n in nodes if alive(n)]
    passes = counter.passes - start
    if not nodes:
        if best_leaf is None:
            raise RuntimeError('the digit histograms hold no pair: the primitive is inconsistent')
        c, key, miss, fa = best_leaf
        return dict(min_dcf=c / c_def, cost=c, key=key, miss=miss, fa=fa, exact=True, bound=c / c_def, passes=passes,
                    key_level=4)
    c, prefix, lvl, miss, fa = incumbent
    if best_leaf is not None and best_leaf[0] <= c:
        c, prefix, lvl, miss, fa = best_leaf[0], best_leaf[1], 4, best_leaf[2], best_leaf[3]
    bound = min(min(n[0] for n in nodes), c)
    key = prefix | ((1 << (32 - 8 * lvl)) - 1)
    return dict(min_dcf=c / c_def, cost=c, key=key, miss=miss, fa=fa, exact=False, bound=bound / c_def, passes=passes,
                key_level=lvl)


def auc_bounds(hist):
    """(auc_lo, auc_hi) from int64 [2, nbins] class histograms over common edges, in exact integers."""
    non = [int(v) for v in hist[0]]
    tgt = [int(v) for v in hist[1]]
    n_non, n_tgt = sum(non), sum(tgt)
    lo = same = below = 0
    for b in range(len(non)):
        lo += tgt[b] * below
        same += tgt[b] * non[b]
        below += non[b]
    return lo / (n_tgt * n_non), (lo + same) / (n_tgt * n_non)


def roc_from_hist(hist, edges):
    """The nbins-point ROC of thresholds at the bin edges, descending as sklearn's: (fpr, tpr, thresholds),
    accepting scores >= thresholds[k]; a leading (0, 0) point at +inf."""
    non, tgt = np.asarray(hist[0], np.float64), np.asarray(hist[1], np.float64)
    fpr = np.concatenate([[0.0], np.cumsum(non[::-1]) / non.sum()])
    tpr = np.concatenate([[0.0], np.cumsum(tgt[::-1]) / tgt.sum()])
    thr = np.concatenate([[np.inf], np.asarray(edges, np.float64)[-2::-1]])
    return fpr, tpr, thr


def analyze(digits, moments, p_target=0.01, c_miss=1, c_fa=1, nbins=256, max_passes=64):
    """All metrics from the two primitives.  ``moments(edges or None)`` returns the dict of
    ``_hip.cosine_verif_moments``.  Raises ValueError before any digits pass when a class is empty."""
    m = moments(None)
    n_non, n_tgt = int(m['count'][0]), int(m['count'][1])
    _check_totals(n_non, n_tgt)
    lo, hi = float(np.nanmin(m['min'])), float(np.nanmax(m['max']))
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    mh = moments(np.linspace(lo, hi, nbins + 1))
    if [int(v) for v in mh['hist'].sum(axis=1)] != [n_non, n_tgt]:
        raise RuntimeError('the class histograms do not add up to the class counts')
    counter = CountingDigits(digits)
    if class_totals(counter) != (n_non, n_tgt):
        raise RuntimeError('the digit histograms do not add up to the class counts')
    eer = eer_search(counter, n_non, n_tgt)
    eer_passes = counter.passes
    dcf = min_dcf_search(counter, p_target, c_miss, c_fa, max_passes, n_non, n_tgt)
    auc_lo, auc_hi = auc_bounds(mh['hist'])
    fpr, tpr, thr = roc_from_hist(mh['hist'], mh['edges'])
    mean = m['sum'] / m['count']
    var = np.maximum(m['sumsq'] / m['count'] - mean * mean, 0.0)
    return dict(
        n_tgt=n_tgt, n_non=n_non, eer=eer['eer'], eer_key=eer['key'], eer_threshold_cosine=score_of_key(eer['key']),
        eer_counts=dict(miss1=eer['miss1'], fa1=eer['fa1'], miss2=eer['miss2'], fa2=eer['fa2']),
        min_dcf=dcf['min_dcf'], min_dcf_bound=dcf['bound'], exact=dcf['exact'],
        min_dcf_point=dict(miss=dcf['miss'], fa=dcf['fa'], key=dcf['key'], key_level=dcf['key_level'],
                           threshold_cosine=score_of_key(dcf['key'])),
        p_target=p_target, c_miss=c_miss, c_fa=c_fa,
        auc=0.5 * (auc_lo + auc_hi), auc_lo=auc_lo, auc_hi=auc_hi, auc_gap=auc_hi - auc_lo,
        fpr=fpr, tpr=tpr, thresholds=thr, hist=mh['hist'], edges=mh['edges'],
        moments=dict(count=m['count'], mean=mean, std=np.sqrt(var), min=m['min'], max=m['max'], sum=m['sum'],
                     sumsq=m['sumsq']),
        passes=dict(eer=eer_passes, min_dcf=dcf['passes'], digits=counter.passes, moments=2,
                    total=counter.passes + 2))


def analyze_device(x, labels, workspace_bytes=None, **kw):
    """``analyze`` over every pair of the device tensor ``x`` [N, E] with integer ``labels`` [N]."""
    from speakerlab import _hip
    return analyze(lambda level, prefixes: _hip.cosine_verif_digits(x, labels, level, prefixes, workspace_bytes),
                   lambda edges: _hip.cosine_verif_moments(x, labels, edges, workspace_bytes), **kw)
