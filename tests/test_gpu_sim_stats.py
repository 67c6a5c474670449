"""spk_cosine_rows_topk / spk_cosine_triu_stats / spk_cosine_triu_hist on the device.  The reference
of every exact check is numpy applied to ``_hip.cosine_affinity(X).cpu()``, the very scores the
kernels consume, so every selection result matches exactly -- indices, counts, histogram, min / max,
order statistics, extreme pairs -- and the fp64 sums match an np.float64 sum to 1e-12 relative
(only the order of the additions differs)."""
import ctypes

import numpy as np
import pytest
import torch

import sim_inputs
from speakerlab import _hip
from speakerlab.utils import similarity_analysis as sa

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(1, 64), (2, 64), (129, 64), (300, 192)]
KS = [1, 5, 100, 299, 1024]
N_EXT = 60


def _x(n, e):
    if n == 300:
        return sim_inputs.tie_input(n, e)
    return np.random.default_rng(n).standard_normal((n, e)).astype(np.float32)


_cache = {}


def _case(n, e):
    """(device X, the device's own scores on the host, the numpy results from them), computed once."""
    if (n, e) not in _cache:
        x = torch.from_numpy(_x(n, e)).to(DEV)
        S = _hip.cosine_affinity(x).cpu().numpy()
        _cache[(n, e)] = (x, S, {})
    return _cache[(n, e)]


def _ref(n, e, k):
    x, S, refs = _case(n, e)
    if k not in refs:
        refs[k] = sa.raw_from_scores(S, k, N_EXT, 50)
    return refs[k]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) <= 1e-12 * np.maximum(np.abs(b), 1e-300)


def _check_rows(got, ref, n):
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.array_equal(got['top_index'], ref['top_index'])
    assert np.array_equal(got['top_scores'], ref['top_scores'])
    assert np.array_equal(got['self'], ref['self'])
    assert _rel(got['sum'], ref['sum']).all()
    assert _rel(got['sumsq'], ref['sumsq']).all()
    if n > 1:
        assert np.array_equal(got['min'], ref['min']) and np.array_equal(got['max'], ref['max'])
    else:
        assert np.isnan(got['min']).all() and np.isnan(got['max']).all()
    return got


@pytest.mark.parametrize('n,e', SHAPES)
@pytest.mark.parametrize('k', KS)
def test_rows_topk(n, e, k):
    x, S, _ = _case(n, e)
    got = _check_rows(_hip.cosine_rows_topk(x, k), _ref(n, e, k)['rows'], n)
    have = min(k, n - 1)
    assert (got['top_index'][:, have:] == -1).all() and np.isneginf(got['top_scores'][:, have:]).all()
    assert (got['top_index'][:, :have] >= 0).all()


def test_rows_topk_ties_and_the_zero_row():
    x, S, _ = _case(300, 192)
    got = {k: v.cpu().numpy() for k, v in _hip.cosine_rows_topk(x, 2).items()}
    # rows 10, 11, 150, 299 are one vector: the three copies score the same, and the cut at k = 2 falls inside them
    assert S[10, 11] == S[10, 150] == S[10, 299]
    assert list(got['top_index'][10]) == [11, 150] and list(got['top_index'][299]) == [10, 11]
    assert list(got['top_index'][150]) == [10, 11]
    # the zero row scores 0 (either sign) against everything: its nearest are the first columns
    assert (S[42] == 0).all() and list(got['top_index'][42]) == [0, 1] and (got['top_scores'][42] == 0).all()
    assert not np.signbit(got['top_scores'][42]).any() and got['sum'][42] == 0 and got['min'][42] == 0
    # a row whose k-th best is the zero of row 42 among positive and negative scores
    for i in (0, 299):
        pos = int((np.delete(S[i], i) > 0).sum())
        top = _hip.cosine_rows_topk(x, pos + 1)['top_index'][i].cpu().numpy()
        assert top[pos] == 42
    # rows 20 and 21 score -0.0 with each other and +0.0 with row 42: one value, ordered by column
    assert S[20, 21] == 0 and np.signbit(S[20, 21]) and S[20, 42] == 0 and not np.signbit(S[20, 42])
    pos = int((np.delete(S[20], 20) > 0).sum())
    top = _hip.cosine_rows_topk(x, pos + 2)
    assert list(top['top_index'][20, pos:].cpu().numpy()) == [21, 42]
    assert not np.signbit(top['top_scores'][20, pos:].cpu().numpy()).any()


def _check_triu(got, ref):
    for key in ('count', 'min', 'max'):
        assert got[key] == ref[key] or (np.isnan(got[key]) and np.isnan(ref[key])), key
    for key in ('sum', 'sumsq'):
        assert _rel(got[key], ref[key]).all() or (np.isnan(got[key]) and np.isnan(ref[key])), key
    assert np.array_equal(got['count_ge'], ref['count_ge'])
    assert np.array_equal(got['order_stats'], ref['order_stats'])
    assert np.array_equal(got['edges'], ref['edges']) and np.array_equal(got['hist'], ref['hist'])
    for name in ('most', 'least'):
        for a, b in zip(got[name], ref[name]):
            assert a.dtype == b.dtype and np.array_equal(a, b), name


def _triu(x, n, **kw):
    P = n * (n - 1) // 2
    ranks = sa.quantile_ranks(P)[1] if P else []
    ranks = sorted(set(ranks) | ({0, P - 1} if P else set()))
    return ranks, _hip.cosine_triu_stats(x, thresholds=sa.THRESHOLDS, ranks=ranks, n_ext=N_EXT, nbins=50, **kw)


@pytest.mark.parametrize('n,e', SHAPES)
def test_triu_stats(n, e):
    x, S, _ = _case(n, e)
    ranks, got = _triu(x, n)
    ref = sa.raw_from_scores(S, 1, N_EXT, 50, ranks=ranks)['triu']
    _check_triu(got, ref)
    P = n * (n - 1) // 2
    assert got['count'] == P and got['hist'].sum() == P and len(got['most'][0]) == min(N_EXT, P)
    if P:
        vals = np.sort(S[np.triu_indices(n, 1)] + np.float32(0))
        assert np.array_equal(got['order_stats'], vals[ranks])     # ranks 0, P - 1 and the quartiles' neighbours
        assert got['order_stats'][0] == got['min'] and got['order_stats'][-1] == got['max']
        h, edges = np.histogram(vals.astype(np.float64), bins=50)
        assert np.array_equal(got['hist'], h) and np.array_equal(got['edges'], edges)


def test_minimum_and_recommended_workspace_give_the_same_bits():
    x, S, _ = _case(300, 192)
    lo, rec, _ = _hip.cosine_sim_workspace_bytes(300)
    assert (lo, rec) == (128 * 300 * 4, 384 * 300 * 4)             # 3 row blocks, the last one ragged, against 1
    for k in (5, 100):
        a = _hip.cosine_rows_topk(x, k, workspace_bytes=lo)
        _check_rows(a, _ref(300, 192, k)['rows'], 300)
        b = _hip.cosine_rows_topk(x, k, workspace_bytes=rec)
        for key in a:
            assert torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), key
    ranks, a = _triu(x, 300, workspace_bytes=lo)
    _, b = _triu(x, 300, workspace_bytes=rec)
    _check_triu(a, sa.raw_from_scores(S, 1, N_EXT, 50, ranks=ranks)['triu'])
    for key in a:
        for u, v in zip(*(t if isinstance(t, tuple) else (t,) for t in (a[key], b[key]))):
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), key


def test_triu_ties_across_the_extremes_cut():
    x, S, _ = _case(300, 192)
    # the six pairs among rows 10, 11, 150, 299 share the largest score: a cut inside them takes the first in (i, j) order
    for n_ext, want in ((1, [(10, 11)]), (4, [(10, 11), (10, 150), (10, 299), (11, 150)])):
        got = _hip.cosine_triu_stats(x, n_ext=n_ext)
        assert list(zip(got['most'][1], got['most'][2])) == want
        ref = sa.raw_from_scores(S, 1, n_ext, 0)['triu']
        for name in ('most', 'least'):
            for a, b in zip(got[name], ref[name]):
                assert np.array_equal(a, b)
    # 64 rows of the same kind (P = 2016, so that a cut among the zeros is within the 4096 pairs an extreme may
    # have): the 63 pairs of the zero row score +0.0 and the pair (20, 21) scores -0.0 -- one run of equal
    # scores with the cut inside it
    xs = torch.from_numpy(sim_inputs.tie_input(64, 64, copies=(11, 50, 63))).to(DEV)
    Ss = _hip.cosine_affinity(xs).cpu().numpy()
    raw = Ss[np.triu_indices(64, 1)]
    vals = raw + np.float32(0)
    below, zeros = int((vals < 0).sum()), int((vals == 0).sum())
    assert zeros == 64 and np.signbit(raw[raw == 0]).any() and not np.signbit(raw[raw == 0]).all()
    n_ext = below + 22
    got = _hip.cosine_triu_stats(xs, n_ext=n_ext, thresholds=[0.0, -0.0], ranks=[below - 1, below, below + 63, below + 64])
    ref = sa.raw_from_scores(Ss, 1, n_ext, 0, thresholds=[0.0, -0.0], ranks=[below - 1, below, below + 63, below + 64])['triu']
    for name in ('most', 'least'):
        for a, b in zip(got[name], ref[name]):
            assert np.array_equal(a, b), name
    assert (got['least'][0][-22:] == 0).all() and not np.signbit(got['least'][0][-22:]).any()
    assert list(zip(got['least'][1][-22:], got['least'][2][-22:])) == [(r, 42) for r in range(20)] + [(20, 21), (20, 42)]
    assert np.array_equal(got['count_ge'], ref['count_ge']) and got['count_ge'][0] == got['count_ge'][1] == len(vals) - below
    assert np.array_equal(got['order_stats'], ref['order_stats'])
    assert got['order_stats'][0] < 0 and got['order_stats'][1] == got['order_stats'][2] == 0 < got['order_stats'][3]
    # the largest pairs from the other side of the same run
    n_ext = len(vals) - below - 64 + 22
    got = _hip.cosine_triu_stats(xs, n_ext=n_ext)
    ref = sa.raw_from_scores(Ss, 1, n_ext, 0)['triu']
    for a, b in zip(got['most'], ref['most']):
        assert np.array_equal(a, b)
    assert list(zip(got['most'][1][-22:], got['most'][2][-22:])) == [(r, 42) for r in range(20)] + [(20, 21), (20, 42)]


def test_histogram_with_scores_on_the_edges():
    x, S, _ = _case(300, 192)
    vals = np.sort(S[np.triu_indices(300, 1)] + np.float32(0)).astype(np.float64)
    # edges that are scores themselves (so that several scores sit exactly on an edge), unequal widths, the
    # zero run on an edge, the maximum on the closed last edge, and a part of the range left out
    edges = np.array([vals[100], vals[101], vals[5000], 0.0, vals[30000], vals[30001], vals[40000], vals[-1]])
    assert (np.diff(edges) >= 0).all()
    got = _hip.cosine_triu_stats(x, nbins=len(edges) - 1, edges=edges)
    assert np.array_equal(got['hist'], np.histogram(vals, bins=edges)[0])
    assert got['hist'].sum() == len(vals) - 100 and got['hist'][-1] >= 6
    wide = np.linspace(-2.0, 2.0, 257)                             # the most bins; most of them empty
    assert np.array_equal(_hip.cosine_triu_stats(x, nbins=256, edges=wide)['hist'], np.histogram(vals, bins=wide)[0])


def test_error_codes_leave_the_outputs_untouched():
    n, e, k = 129, 64, 5
    x, _, _ = _case(n, e)
    lo, rec, st_bytes = _hip.cosine_sim_workspace_bytes(n)
    ws = torch.empty(rec, dtype=torch.uint8, device=DEV)
    st = torch.empty(st_bytes, dtype=torch.uint8, device=DEV)
    outs = [torch.full((n, k), -7.0, device=DEV), torch.full((n, k), -7, dtype=torch.int64, device=DEV),
            torch.full((n,), -7.0, dtype=torch.float64, device=DEV), torch.full((n,), -7.0, dtype=torch.float64, device=DEV)]
    outs += [torch.full((n,), -7.0, device=DEV) for _ in range(3)]
    lib = _hip.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def rows(x_=x.data_ptr(), N=n, E=e, k_=k, w=ws.data_ptr(), wb=rec, o0=outs[0].data_ptr()):
        return lib.spk_cosine_rows_topk(x_, N, E, k_, o0, *[o.data_ptr() for o in outs[1:]], w, wb, stream)

    for kw, code in ((dict(x_=None), -1), (dict(o0=None), -1), (dict(w=None), -1), (dict(N=0), -1), (dict(E=0), -1),
                     (dict(E=62), -1), (dict(x_=x.data_ptr() + 4), -1), (dict(k_=0), -1), (dict(k_=1025), -1),
                     (dict(wb=lo - 1), -5), (dict(N=2 ** 31, wb=2 ** 62), -6)):
        assert rows(**kw) == code, kw

    P = n * (n - 1) // 2
    a = lambda v: v.ctypes.data
    thr, ranks = np.array([0.1], np.float32), np.array([0, P - 1], np.int64)
    host = dict(count=np.full(1, -7, np.int64), sums=np.full(2, -7.0), mm=np.full(2, -7, np.float32),
                cge=np.full(1, -7, np.int64), order=np.full(2, -7, np.float32), cut=np.full(2, -7, np.float32),
                take=np.full(2, -7, np.int32), hist=np.full(4, -7, np.int64), es=np.full((2, 8), -7, np.float32),
                ei=np.full((2, 8), -7, np.int64), ej=np.full((2, 8), -7, np.int64), found=np.full(2, -7, np.int32))

    def stats(x_=x.data_ptr(), N=n, E=e, r=a(ranks), nr=2, nt=1, ne=8, wb=rec, s=st.data_ptr(), sb=st_bytes):
        return lib.spk_cosine_triu_stats(x_, N, E, a(thr), nt, r, nr, ne, a(host['count']), a(host['sums']),
                                         a(host['sums']) + 8, a(host['mm']), a(host['mm']) + 4, a(host['cge']),
                                         a(host['order']), a(host['cut']), a(host['take']), ws.data_ptr(), wb, s, sb,
                                         stream)

    for kw, code in ((dict(x_=None), -1), (dict(N=0), -1), (dict(E=6), -1), (dict(x_=x.data_ptr() + 8), -1),
                     (dict(ne=4097), -1), (dict(ne=-1), -1), (dict(nt=33), -1), (dict(nr=17), -1),
                     (dict(r=a(np.array([3, 2], np.int64))), -1), (dict(r=a(np.array([0, P], np.int64))), -1),
                     (dict(N=1, nr=1), -1), (dict(s=None), -1), (dict(wb=lo - 1), -5), (dict(sb=st_bytes - 1), -5),
                     (dict(N=2 ** 31, wb=2 ** 62, nr=0), -6)):
        assert stats(**kw) == code, kw

    edges, cut, take = np.linspace(-1, 1, 5), np.array([0.2, -0.2], np.float32), np.array([1, 1], np.int32)

    def hist(x_=x.data_ptr(), N=n, ed=a(edges), nb=4, ne=8, et=a(take), wb=rec, sb=st_bytes):
        return lib.spk_cosine_triu_hist(x_, N, e, ed, nb, ne, a(cut), et, a(host['hist']), a(host['es']), a(host['ei']),
                                        a(host['ej']), a(host['found']), ws.data_ptr(), wb, st.data_ptr(), sb, stream)

    for kw, code in ((dict(x_=None), -1), (dict(N=0), -1), (dict(ed=None), -1), (dict(nb=257), -1), (dict(ne=4097), -1),
                     (dict(ed=a(np.array([0.0, 0.5, 0.4, 0.6, 1.0]))), -1), (dict(et=a(np.array([0, 1], np.int32))), -1),
                     (dict(wb=lo - 1), -5), (dict(sb=st_bytes - 1), -5)):
        assert hist(**kw) == code, kw
    # cuts that are not this input's: found out after the pass, nothing written either
    assert hist() == -1 and b'cuts' in lib.spk_last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert o.eq(-7).all()
    for name, v in host.items():
        assert (v == -7).all(), name
    # N == 1: no pair
    one = _hip.cosine_triu_stats(_case(1, 64)[0], thresholds=[0.0], n_ext=5, nbins=3)
    assert one['count'] == 0 and np.isnan([one['sum'], one['sumsq'], one['min'], one['max']]).all()
    assert one['count_ge'][0] == 0 and (one['hist'] == 0).all() and len(one['most'][0]) == len(one['least'][0]) == 0
    with pytest.raises(_hip.HipError) as ei:
        _hip.cosine_triu_stats(_case(1, 64)[0], ranks=[0])
    assert ei.value.code == -1
