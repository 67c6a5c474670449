"""spk_cosine_verif_moments / spk_cosine_verif_digits on the GPU: every integer the ABI returns is
compared exactly with numpy applied to the device's own scores (``_hip.cosine_affinity(X)``, strict
upper triangle, the same key map), and the driver's EER / minDCF end to end with the brute force of
tests/verif_oracle.py."""
import numpy as np
import pytest
import torch

from speakerlab import _hip
from speakerlab.utils import verification_analysis as va

import verif_oracle as vo

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def embeddings(n, e, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == 'ternary':                      # entries in {-1, 0, 1}: many tied scores
        return rng.integers(-1, 2, (n, e)).astype(np.float32)
    return rng.standard_normal((n, e)).astype(np.float32)


def labels_of(n, layout, seed):
    rng = np.random.default_rng(seed + 100)
    if layout == 'balanced':
        lab = np.arange(n) % max(2, n // 6)
    elif layout == 'singletons':               # a few pairs of rows share a speaker, the rest are alone
        lab = np.arange(n)
        lab[1::7] = lab[0:n - 1:7][:len(lab[1::7])]
    else:                                      # one speaker holds half the rows
        lab = np.where(np.arange(n) < n // 2, 0, 1 + np.arange(n) % 9)
    return rng.permutation(lab).astype(np.int32) if n > 2 else lab.astype(np.int32)


_cache = {}


def case(n, e, kind='normal', layout='balanced', special=False):
    """(x device, labels device, scores float32 triangle, keys, classes), computed once per case."""
    key = (n, e, kind, layout, special)
    if key not in _cache:
        X = embeddings(n, e, kind, 7 * n + e)
        lab = labels_of(n, layout, n)
        if special and n >= 40:
            X[5] = X[3]; lab[5] = lab[3]       # duplicate rows under the same speaker
            X[11] = X[9]; lab[11] = lab[9] + 1     # and under different ones
            X[20] = 0.0                        # a zero row: scores of exactly 0
            X[30] = -X[3]
        x = torch.from_numpy(X).to(DEV)
        S = _hip.cosine_affinity(x).cpu().numpy()
        iu = np.triu_indices(n, 1)
        s = np.ascontiguousarray(S[iu])
        classes = (lab[iu[0]] == lab[iu[1]]).astype(np.int64)
        _cache[key] = (x, torch.from_numpy(lab).to(DEV), s, va.keys_of_scores(s), classes)
    return _cache[key]


CASES = [(2, 64, 'normal', 'balanced', False), (129, 64, 'normal', 'balanced', True),
         (129, 192, 'ternary', 'half', True), (300, 192, 'normal', 'singletons', True),
         (300, 64, 'ternary', 'balanced', True), (300, 64, 'normal', 'half', False)]


def workspaces(n):
    return [None] if n < 300 else [None, _hip.cosine_verif_workspace_bytes(n)[0]]


def pick_prefixes(keys, level, count):
    """(``count`` prefixes of ``level`` bytes, the index of the one that matches no pair or None): the most
    populated ones, then the absent one."""
    shift = 32 - 8 * level
    present, pop = np.unique(keys >> np.uint32(shift), return_counts=True)
    order = present[np.argsort(-pop, kind='stable')]
    out = [int(p) << shift for p in order[:max(count - 1, 1)]]
    absent = next(p for p in range(1 << (8 * level)) if p not in set(present.tolist()))
    at = None
    if count > 1:
        at = len(out)
        out.append(absent << shift)
    while len(out) < count:                    # fewer distinct prefixes than asked for: repeats are allowed
        out.append(out[0])
    return [p | (0x5A & ((1 << shift) - 1)) for p in out], at   # the low bytes are to be ignored


@pytest.mark.parametrize('n,e,kind,layout,special', CASES)
def test_digits_match_numpy(n, e, kind, layout, special):
    x, lab, s, keys, classes = case(n, e, kind, layout, special)
    want = va.host_digits(keys, classes)
    for ws in workspaces(n):
        got = _hip.cosine_verif_digits(x, lab, 0, [0], workspace_bytes=ws)
        assert got.shape == (1, 2, 256) and got.dtype == np.int64
        assert np.array_equal(got, want(0, [0]))
        assert got.sum() == n * (n - 1) // 2
        for level in (1, 2, 3):
            for count in (1, 2, 16):
                pre, absent = pick_prefixes(keys, level, count)
                got = _hip.cosine_verif_digits(x, lab, level, pre, workspace_bytes=ws)
                assert got.shape == (count, 2, 256)
                assert np.array_equal(got, want(level, pre)), (level, count)
                assert got[0].sum() > 0 and (absent is None or got[absent].sum() == 0)


@pytest.mark.parametrize('n,e,kind,layout,special', CASES)
def test_moments_match_numpy(n, e, kind, layout, special):
    x, lab, s, keys, classes = case(n, e, kind, layout, special)
    d = s.astype(np.float64)
    present = float(s[len(s) // 2])            # an edge equal to a present score
    edges = np.unique(np.concatenate([np.linspace(-1.0, 1.0, 40), [present, 0.0]]))
    for ws in workspaces(n):
        m = _hip.cosine_verif_moments(x, lab, edges=edges, workspace_bytes=ws)
        for c in (0, 1):
            sel = classes == c
            assert m['count'][c] == sel.sum()
            if sel.any():
                assert m['min'][c] == s[sel].min() and m['max'][c] == s[sel].max()
                for got, ref in ((m['sum'][c], d[sel].sum()), (m['sumsq'][c], (d[sel] ** 2).sum())):
                    print(f'n {n} class {c}: {got!r} vs {ref!r}')
                    assert abs(got - ref) <= 1e-12 * abs(ref)
            else:
                assert np.isnan(m['min'][c]) and np.isnan(m['max'][c])
            want = np.histogram(d[sel], bins=edges)[0]
            assert np.array_equal(m['hist'][c], want)
        bare = _hip.cosine_verif_moments(x, lab, workspace_bytes=ws)
        assert 'hist' not in bare and np.array_equal(bare['count'], m['count'])
        assert bare['sum'].tobytes() == m['sum'].tobytes() and bare['sumsq'].tobytes() == m['sumsq'].tobytes()
    if n >= 300:                               # the same bits for every workspace
        a = _hip.cosine_verif_moments(x, lab)
        b = _hip.cosine_verif_moments(x, lab, workspace_bytes=workspaces(n)[1])
        assert a['sum'].tobytes() == b['sum'].tobytes() and a['sumsq'].tobytes() == b['sumsq'].tobytes()


@pytest.mark.parametrize('n,e,kind,layout,special', CASES[1:])
@pytest.mark.parametrize('p_target', [0.01, 0.5])
def test_driver_end_to_end(n, e, kind, layout, special, p_target):
    x, lab, s, keys, classes = case(n, e, kind, layout, special)
    rep = va.analyze_device(x, lab, p_target=p_target)
    want = vo.brute(keys, classes, p_target)
    assert rep['exact'] is True
    assert (rep['n_tgt'], rep['n_non']) == (want['n_tgt'], want['n_non'])
    assert rep['eer_counts'] == dict(miss1=want['miss1'], fa1=want['fa1'], miss2=want['miss2'], fa2=want['fa2'])
    assert rep['eer_key'] == want['eer_key']
    assert np.float32(rep['eer_threshold_cosine']).view(np.uint32) == va.bits_of_key(np.array([want['eer_key']], np.uint32))[0]
    assert abs(rep['eer'] - want['eer']) <= 1e-12 * abs(want['eer'])
    pt = rep['min_dcf_point']
    assert (pt['miss'], pt['fa'], pt['key']) == (want['dcf_miss'], want['dcf_fa'], want['dcf_key'])
    assert abs(rep['min_dcf'] - want['min_dcf']) <= 1e-12 * abs(want['min_dcf'])
    assert rep['passes']['min_dcf'] <= 64 and rep['auc_lo'] <= rep['auc'] <= rep['auc_hi']


def test_cross_class_ties_exist_in_the_special_case():
    _, _, s, keys, classes = case(129, 64, 'normal', 'balanced', True)
    both = np.intersect1d(keys[classes == 0], keys[classes == 1])
    assert len(both) >= 1 and (s == 0).sum() >= 128 and classes[s == 0].min() == 0 and classes[s == 0].max() == 1


def test_errors():
    x, lab, *_ = case(129, 64, 'normal', 'balanced', True)
    n = x.shape[0]
    one = torch.zeros(n, dtype=torch.int32, device=DEV)
    distinct = torch.arange(n, dtype=torch.int32, device=DEV)
    for bad in (one, distinct):
        with pytest.raises(ValueError):
            va.analyze_device(x, bad)
    neg = lab.clone()
    neg[17] = -1
    for call in (lambda: _hip.cosine_verif_digits(x, neg, 0, [0]), lambda: _hip.cosine_verif_moments(x, neg)):
        with pytest.raises(_hip.HipError) as e:
            call()
        assert e.value.code == _hip.E_INVALID
    lo = _hip.cosine_verif_workspace_bytes(n)[0]
    for call in (lambda: _hip.cosine_verif_digits(x, lab, 0, [0], workspace_bytes=lo - 4),
                 lambda: _hip.cosine_verif_moments(x, lab, workspace_bytes=lo - 4)):
        with pytest.raises(_hip.HipError) as e:
            call()
        assert e.value.code == -5              # SPK_E_WORKSPACE
    for level, pre in ((4, [0]), (-1, [0]), (1, list(range(17))), (0, [0, 1]), (2, [])):
        with pytest.raises(_hip.HipError) as e:
            _hip.cosine_verif_digits(x, lab, level, pre)
        assert e.value.code == _hip.E_INVALID
    # the entries still work after the errors
    assert _hip.cosine_verif_digits(x, lab, 0, [0]).sum() == n * (n - 1) // 2
