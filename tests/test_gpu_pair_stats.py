"""spk_pair_cosine_stats on the device: the condensed pair cosines against ``_hip.cosine_trials`` bit
for bit, the statistics against numpy on the returned cosines, a group alone against the same group
inside a batch, and the argument errors with the outputs left untouched."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 65, 130]          # 65 rows: 2080 pairs, more than one 1024-thread pass
DIMS = [4, 192, 512]                   # 512: the second float4 pass of a wave
THR = 0.05
E_INVALID, E_UNSUPPORTED = -1, -6


def _dev():
    return torch.device('cuda', 0)


def _offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def _rows(sizes, E, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((int(sum(sizes)), E)).astype(np.float32)


def _host(st):
    """PairStats -> numpy (cos, min, mean, argmin, n_below)."""
    return (None if st.cos is None else st.cos.cpu().numpy(), st.min.cpu().numpy(), st.mean.cpu().numpy(),
            st.argmin.cpu().numpy(), st.n_below.cpu().numpy())


def _trials(X, offsets):
    """Every group's pair cosines by ``cosine_trials`` on the same (i, j) lists, back to back."""
    from speakerlab import _hip
    ia, ib = [], []
    for g in range(len(offsets) - 1):
        i, j = np.triu_indices(offsets[g + 1] - offsets[g], 1)
        ia.append(i + offsets[g])
        ib.append(j + offsets[g])
    ia, ib = np.concatenate(ia).astype(np.int64), np.concatenate(ib).astype(np.int64)
    if ia.size == 0:
        return np.zeros(0, np.float32)
    return _hip.cosine_trials(X, X, torch.from_numpy(ia), torch.from_numpy(ib)).cpu().numpy()


def _check_stats(cos, po, mn, mean, argmin, below, thr):
    """min / argmin / n_below exactly and mean within one ulp, from the returned cosines."""
    for g in range(len(po) - 1):
        c = cos[po[g]:po[g + 1]]
        if c.size == 0:
            assert mn[g] == 1.0 and mean[g] == 1.0 and argmin[g] == -1 and below[g] == 0, g
            continue
        assert argmin[g] == int(np.argmin(c)), g
        assert mn[g].tobytes() == c[argmin[g]].tobytes() and mn[g] == c.min(), g
        assert below[g] == int((c < np.float32(thr)).sum()), g
        ref = np.float32(c.astype(np.float64).sum() / c.size)
        print(f'group {g}: P {c.size}, mean {mean[g]!r}, numpy {ref!r}, diff {abs(float(mean[g]) - float(ref)):.3e}')
        assert abs(float(mean[g]) - float(ref)) <= float(np.spacing(np.abs(ref))), g


@pytest.fixture(scope='module', params=DIMS)
def batch(request):
    """(E, X device, offsets, host results of the whole batch): computed once per E."""
    from speakerlab import _hip
    E = request.param
    X = torch.from_numpy(_rows(SIZES, E, seed=E)).to(_dev())
    offs = _offsets(SIZES)
    st = _hip.pair_cosine_stats(X, offs, THR)
    return E, X, offs, st.pair_offsets, _host(st)


def test_cosines_have_the_bits_of_cosine_trials(batch):
    E, X, offs, po, (cos, *_rest) = batch
    assert po == [0, 0, 0, 1, 4, 4 + 2080, 4 + 2080 + 8385] and cos.shape == (po[-1],) and cos.dtype == np.float32
    ref = _trials(X, offs)
    assert cos.tobytes() == ref.tobytes()
    assert np.abs(cos).max() <= 1.0 + 1e-6 and np.isfinite(cos).all()


def test_statistics_against_the_returned_cosines(batch):
    E, X, offs, po, (cos, mn, mean, argmin, below) = batch
    _check_stats(cos, po, mn, mean, argmin, below, THR)
    assert 0 < below[5] < 8385                       # the threshold cuts through the large group


def test_alone_and_in_a_batch(batch):
    from speakerlab import _hip
    E, X, offs, po, (cos, mn, mean, argmin, below) = batch
    for g, n in enumerate(SIZES):
        c1, m1, a1, i1, b1 = _host(_hip.pair_cosine_stats(X[offs[g]:offs[g + 1]], [0, n], THR))
        assert c1.tobytes() == cos[po[g]:po[g + 1]].tobytes(), g
        for one, many in ((m1, mn), (a1, mean), (i1, argmin), (b1, below)):
            assert one.tobytes() == many[g:g + 1].tobytes(), g
    # the same groups in reverse order: another place in the batch, the same bits
    order = list(range(len(SIZES)))[::-1]
    Xr = torch.cat([X[offs[g]:offs[g + 1]] for g in order])
    cr, mr, ar, ir, br = _host(_hip.pair_cosine_stats(Xr, _offsets([SIZES[g] for g in order]), THR))
    for many, rev in ((mn, mr), (mean, ar), (argmin, ir), (below, br)):
        assert many[order].tobytes() == rev.tobytes()


def test_without_cosines_the_same_statistics(batch):
    from speakerlab import _hip
    E, X, offs, po, (cos, mn, mean, argmin, below) = batch
    st = _hip.pair_cosine_stats(X, offs, THR, want_cos=False)
    assert st.cos is None and st.pair_offsets == po
    _, m2, a2, i2, b2 = _host(st)
    for a, b in ((mn, m2), (mean, a2), (argmin, i2), (below, b2)):
        assert a.tobytes() == b.tobytes()


def test_strided_rows():
    from speakerlab import _hip
    sizes, E = [3, 0, 7], 8
    wide = torch.from_numpy(_rows(sizes, E + 4, seed=1)).to(_dev())
    view = wide[:, :E]
    assert view.stride(0) == E + 4
    a = _host(_hip.pair_cosine_stats(view, _offsets(sizes), THR))
    b = _host(_hip.pair_cosine_stats(view.contiguous(), _offsets(sizes), THR))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[0].tobytes() == _trials(view.contiguous(), _offsets(sizes)).tobytes()


def test_zero_norm_row_scores_zero():
    from speakerlab import _hip
    from speakerlab.utils import single_speaker as ss
    n, E = 6, 16
    x = _rows([n], E, seed=2)
    x[2] = 0
    cos, mn, mean, argmin, below = _host(_hip.pair_cosine_stats(torch.from_numpy(x).to(_dev()), [0, n], -2.0))
    zero = [ss.ij_to_condensed(n, min(2, k), max(2, k)) for k in range(n) if k != 2]
    assert all(cos[p] == 0.0 for p in zero) and np.isfinite(cos).all()
    assert sum(c == 0.0 for c in cos) == len(zero) and below[0] == 0


def test_tied_minima_take_the_smallest_index():
    """Rows alternating between two vectors: every (a, b) pair has the same bits, hundreds of them,
    in every wave and on both sides of the 1024-pair stride; row 0 differs, so the first minimum is
    not pair 0."""
    from speakerlab import _hip
    n, E = 65, 12
    rng = np.random.default_rng(3)
    a = rng.standard_normal(E).astype(np.float32)
    b = (-a + 0.1 * rng.standard_normal(E)).astype(np.float32)
    x = np.stack([a if k % 2 else b for k in range(n)])
    x[0] = np.abs(a)
    X = torch.from_numpy(x).to(_dev())
    for want_cos in (True, False):
        st = _hip.pair_cosine_stats(X, [0, n], THR, want_cos=want_cos)
        cos = _hip.pair_cosine_stats(X, [0, n], THR).cos.cpu().numpy()
        ties = np.flatnonzero(cos == cos.min())
        assert len(ties) > 1000 and ties[0] > 0 and ties[-1] > 1024
        assert int(st.argmin[0]) == int(ties[0]) and float(st.min[0]) == float(cos.min())


def test_threshold_edge():
    from speakerlab import _hip
    from speakerlab.utils import single_speaker as ss
    n, E = 9, 32
    X = torch.from_numpy(_rows([n], E, seed=4)).to(_dev())
    cos = _hip.pair_cosine_stats(X, [0, n], 0.0).cos.cpu().numpy()
    order = np.argsort(cos)
    thr = float(cos[order[10]])                        # exactly a cosine: not below itself
    st = _hip.pair_cosine_stats(X, [0, n], thr)
    assert int(st.n_below[0]) == 10 == int((cos < np.float32(thr)).sum())
    # min == threshold: single-speaker
    lo = float(cos.min())
    res = ss.pair_stats([X], lo)[0]
    assert res['n_below'] == 0 and res['min'] == lo
    assert ss.make_result('w.wav', [[k, k + 0.5] for k in range(n)], lo, res)['is_single_speaker']
    assert not ss.make_result('w.wav', [[k, k + 0.5] for k in range(n)], float(np.nextafter(np.float32(lo), 2)),
                              res)['is_single_speaker']


def test_pair_index_map_at_2049_rows():
    """One group of 2049 rows (2,098,176 pairs): every cosine against ``cosine_trials`` on
    ``np.triu_indices``, the last row's among them, and the statistics with and without ``cos``
    (the second form steps (i, j) along the condensed order inside one workgroup)."""
    from speakerlab import _hip
    n, E = 2049, 8
    X = torch.from_numpy(_rows([n], E, seed=5)).to(_dev())
    st = _hip.pair_cosine_stats(X, [0, n], THR)
    cos, mn, mean, argmin, below = _host(st)
    assert st.pair_offsets == [0, n * (n - 1) // 2]
    ref = _trials(X, [0, n])
    assert cos[-3:].tobytes() == ref[-3:].tobytes()     # rows 2046 and 2047, the last ones with pairs
    assert cos.tobytes() == ref.tobytes()
    _check_stats(cos, st.pair_offsets, mn, mean, argmin, below, THR)
    _, m2, a2, i2, b2 = _host(_hip.pair_cosine_stats(X, [0, n], THR, want_cos=False))
    for a, b in ((mn, m2), (mean, a2), (argmin, i2), (below, b2)):
        assert a.tobytes() == b.tobytes()


def test_a_group_cut_across_two_pair_launches():
    """8200 rows are 33,615,900 pairs, 61,468 more than a pair launch covers (2^25: a grid is a
    32-bit count of work-items), so the group's pair range is cut inside one of its rows.  Cosines on both
    sides of the cut, at both ends and at strided places against ``cosine_trials``; the statistics
    against numpy on all of them."""
    from speakerlab import _hip
    from speakerlab.utils import single_speaker as ss
    n, E, cut = 8200, 4, 1 << 25
    P = n * (n - 1) // 2
    assert _hip.pair_cosine_plan([0, n]) == {'pair_launches': 2, 'stats_launches': 1, 'max_launch_pairs': cut,
                                             'planned_pairs': P}
    X = torch.from_numpy(_rows([n], E, seed=10)).to(_dev())
    st = _hip.pair_cosine_stats(X, [0, n], THR)
    cos, mn, mean, argmin, below = _host(st)
    assert cos.shape == (P,)
    picks = sorted(set(range(0, 300)) | set(range(cut - 300, cut + 300)) | set(range(P - 300, P))
                   | set(range(0, P, 65521)))
    ij = np.array([ss.condensed_to_ij(n, p) for p in picks], dtype=np.int64)
    ref = _hip.cosine_trials(X, X, torch.from_numpy(ij[:, 0].copy()), torch.from_numpy(ij[:, 1].copy())).cpu().numpy()
    assert cos[picks].tobytes() == ref.tobytes()
    _check_stats(cos, st.pair_offsets, mn, mean, argmin, below, THR)
    # without cos this group is above the library's cap for that form: the binding scores it into a
    # scratch array and drops it, the statistics are the same
    assert n > _hip.PAIR_FUSED_MAX_ROWS
    st2 = _hip.pair_cosine_stats(X, [0, n], THR, want_cos=False)
    assert st2.cos is None
    for a, b in zip((mn, mean, argmin, below), _host(st2)[1:]):
        assert a.tobytes() == b.tobytes()


def test_nan_cosines_order_below_every_number():
    """A non-finite row: its pairs' cosines are NaN; min is NaN, argmin the first NaN, the mean NaN
    (numpy's min / argmin / mean of the cosines), and a NaN is not below the threshold."""
    from speakerlab import _hip
    n, E = 70, 8                                       # 2415 pairs: NaNs in several waves and passes
    x = _rows([n], E, seed=11)
    x[5, 3] = np.nan
    x[40, 0] = np.inf
    X = torch.from_numpy(x).to(_dev())
    for want_cos in (True, False):
        st = _hip.pair_cosine_stats(X, [0, n], THR, want_cos=want_cos)
        cos = _hip.pair_cosine_stats(X, [0, n], THR).cos.cpu().numpy()
        assert np.isnan(cos).sum() == 2 * (n - 1) - 1
        assert np.isnan(float(st.min[0])) and np.isnan(float(st.mean[0]))
        assert int(st.argmin[0]) == int(np.argmin(cos)) == 4          # pair (0, 5)
        assert int(st.n_below[0]) == int((cos < np.float32(THR)).sum())


def test_views_the_kernels_cannot_read_in_place_are_copied():
    """A row stride that is no multiple of 4 and rows off a 16-byte boundary: the library rejects
    both (the error table below), the binding copies such a view first."""
    from speakerlab import _hip
    sizes, E = [5, 2], 8
    offs = _offsets(sizes)
    x = _rows(sizes, E, seed=12)
    want = _host(_hip.pair_cosine_stats(torch.from_numpy(x).to(_dev()), offs, THR))
    wide = torch.zeros((7, E + 2), device=_dev())
    wide[:, :E] = torch.from_numpy(x).to(_dev())
    odd_stride = wide[:, :E]
    flat = torch.zeros(7 * E + 1, device=_dev())
    flat[1:] = torch.from_numpy(x).to(_dev()).reshape(-1)
    misaligned = flat[1:].view(7, E)
    assert odd_stride.stride(0) % 4 == 2 and misaligned.data_ptr() % 16 == 4
    for view in (odd_stride, misaligned):
        got = _host(_hip.pair_cosine_stats(view, offs, THR))
        for a, b in zip(want, got):
            assert a.tobytes() == b.tobytes()


def test_more_groups_than_one_launch_takes():
    """150 groups of 0 to 6 rows: three launches of 64 groups' descriptors."""
    from speakerlab import _hip
    sizes = [k % 7 for k in range(150)]
    E = 20
    X = torch.from_numpy(_rows(sizes, E, seed=6)).to(_dev())
    offs = _offsets(sizes)
    st = _hip.pair_cosine_stats(X, offs, THR)
    cos, mn, mean, argmin, below = _host(st)
    assert cos.tobytes() == _trials(X, offs).tobytes()
    _check_stats(cos, st.pair_offsets, mn, mean, argmin, below, THR)
    _, m2, a2, i2, b2 = _host(_hip.pair_cosine_stats(X, offs, THR, want_cos=False))
    for a, b in ((mn, m2), (mean, a2), (argmin, i2), (below, b2)):
        assert a.tobytes() == b.tobytes()


def test_no_pairs_at_all_still_writes_the_statistics():
    from speakerlab import _hip
    X = torch.from_numpy(_rows([1, 1], 4, seed=7)).to(_dev())
    st = _hip.pair_cosine_stats(X, [0, 0, 1, 2], THR)
    cos, mn, mean, argmin, below = _host(st)
    assert cos.size == 0 and list(mn) == [1, 1, 1] and list(mean) == [1, 1, 1]
    assert list(argmin) == [-1, -1, -1] and list(below) == [0, 0, 0]
    empty = _hip.pair_cosine_stats(X[:0], [0], THR)
    assert empty.min.numel() == 0 and empty.pair_offsets == [0]


def test_python_pair_stats_matches_the_host_restatement():
    from speakerlab.utils import single_speaker as ss
    sizes, E = [4, 0, 1, 12], 192
    x = _rows(sizes, E, seed=8)
    offs = _offsets(sizes)
    groups = [torch.from_numpy(x[offs[g]:offs[g + 1]]).to(_dev()) if sizes[g] else None for g in range(len(sizes))]
    dev = ss.pair_stats(groups, THR)
    ref = ss.pair_stats_host([x[offs[g]:offs[g + 1]] for g in range(len(sizes))], THR)
    # fp32 cosine of E = 192 terms: (E + 4) u per the bound of tests/data_ref.py, u = 2^-24
    tol = (E + 4) * 2.0 ** -24
    for d, r in zip(dev, ref):
        assert d['cos'].dtype == np.float32 and len(d['cos']) == len(r['cos'])
        assert np.abs(d['cos'] - r['cos']).max(initial=0.0) <= tol
        assert abs(d['min'] - r['min']) <= tol and abs(d['mean'] - r['mean']) <= tol
        assert d['argmin'] == r['argmin'] and d['n_below'] == r['n_below']
    same = ss.pair_stats((torch.from_numpy(x).to(_dev()), offs), THR, want_cos=False)
    assert all('cos' not in s for s in same)
    assert [(s['min'], s['mean'], s['argmin'], s['n_below']) for s in same] == \
        [(d['min'], d['mean'], d['argmin'], d['n_below']) for d in dev]


def test_error_table_leaves_the_outputs_untouched():
    from speakerlab import _hip
    lib = _hip.lib()
    dev = _dev()
    sizes, E = [3, 4], 8
    X = torch.from_numpy(_rows(sizes, E, seed=9)).to(dev)
    out = {'cos': torch.full((9,), 7.0, device=dev), 'mn': torch.full((2,), 7.0, device=dev),
           'mean': torch.full((2,), 7.0, device=dev), 'argmin': torch.full((2,), 7, dtype=torch.int64, device=dev),
           'below': torch.full((2,), 7, dtype=torch.int64, device=dev)}
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(G=2, E=E, ldx=E, offs=(0, 3, 7), X=X.data_ptr(), **null):
        ptr = {k: (None if k in null else v.data_ptr()) for k, v in out.items()}
        arr = None if offs is None else (ctypes.c_int64 * len(offs))(*offs)
        return lib.spk_pair_cosine_stats(X, ldx, E, arr, G, 0.5, ptr['cos'], ptr['mn'], ptr['mean'], ptr['argmin'],
                                         ptr['below'], stream)

    with torch.cuda.device(dev):
        assert call(G=-1) == E_INVALID
        assert call(offs=None) == E_INVALID
        assert call(X=None) == E_INVALID
        for name in ('mn', 'mean', 'argmin', 'below'):
            assert call(**{name: True}) == E_INVALID, name
        for bad_e in (0, -4, 6):
            assert call(E=bad_e) == E_INVALID, bad_e
        assert call(ldx=E - 4) == E_INVALID
        assert call(ldx=E + 2) == E_INVALID                       # rows are read as float4 ...
        assert call(X=X.data_ptr() + 4) == E_INVALID              # ... from 16-byte boundaries
        assert call(offs=(0, 3, 3 + 4097), cos=True) == E_UNSUPPORTED   # no cos: 4096 rows a group at most
        assert b'4096' in lib.spk_last_error()
        assert call(offs=(0, 5, 3)) == E_INVALID
        assert call(offs=(0, 3, 3 + 32769)) == E_UNSUPPORTED
        assert b'32768' in lib.spk_last_error()
        torch.cuda.synchronize(dev)
        for k, v in out.items():
            assert bool((v == 7).all()), k
        # and the same call with nothing wrong fills them (cos may be left out)
        assert call(cos=True) == 0
        torch.cuda.synchronize(dev)
        assert bool((out['cos'] == 7).all()) and not bool((out['mn'] == 7).any())
        assert call() == 0
        torch.cuda.synchronize(dev)
        assert not bool((out['cos'] == 7).any())
    with pytest.raises(_hip.HipError) as ei:
        _hip.pair_cosine_stats(X, [0, 5, 3], 0.5)
    assert ei.value.code == E_INVALID
