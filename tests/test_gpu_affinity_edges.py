"""Edge cases of the cosine affinity, top-k and trial kernels (csrc/affinity.hip, cosine_pair.h)
against the fp64 references and the derived bounds of tests/data_ref.py: every E % 16 and odd /
even k-tile counts, shapes around the 64-column half and the 128 tile, zero rows anywhere, a
strided output, ties across half / tile / segment boundaries, multi-tile segments, exact counts
and the partial second trip of the trial kernel.  tests/test_data_ref_host.py shows on the host
that each case can fail.  Every test prints its worst err / bound."""
import numpy as np
import pytest
import torch

import data_ref as D
from speakerlab import _hip

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def _scales(n, seed):
    return np.ldexp(np.float32(1), np.random.default_rng(seed).integers(-40, 41, n)).astype(np.float32)


AFF_IDS = [f'{na}x{nb}x{e}-{kind}' for na, nb, e, kind in D.AFF_CASES]


@pytest.mark.parametrize('na,nb,e,kind', D.AFF_CASES, ids=AFF_IDS)
def test_affinity_grid(na, nb, e, kind):
    a, b = D.aff_data(na, nb, e, kind)
    S, mag = D.cos_ref(a, b)
    out = host(_hip.cosine_affinity(dev(a), dev(b)))
    ratio = np.abs(out - S) / np.maximum(D.cos_bound(S, mag, e), 1e-300)
    lv = D.live(a, b)
    print(f'affinity {na}x{nb}x{e} {kind}: max err/bound {ratio[lv].max() if lv.any() else 0:.3f}')
    assert np.all(out[~lv] == 0)                          # zero rows: exactly 0
    assert np.all(ratio[lv] <= 1.0), ratio[lv].max()
    # b=None scores a against itself with the same bits as b=a
    assert np.array_equal(host(_hip.cosine_affinity(dev(a))), host(_hip.cosine_affinity(dev(a), dev(a))))
    # out= a column slice of a wider NaN-filled tensor (ldo > Nb): the NaNs around it survive
    wide = torch.full((na, nb + 7), float('nan'), device='cuda')
    _hip.cosine_affinity(dev(a), dev(b), out=wide[:, 3:3 + nb])
    w = host(wide)
    assert np.isnan(w[:, :3]).all() and np.isnan(w[:, 3 + nb:]).all()
    assert np.array_equal(w[:, 3:3 + nb], out)
    # power-of-two row scaling changes no bit: every product, sum, root and quotient scales exactly
    sa, sb = _scales(na, 1), _scales(nb, 2)
    assert np.array_equal(host(_hip.cosine_affinity(dev(a * sa[:, None]), dev(b * sb[:, None]))), out)


def test_affinity_single_zero_rows():
    z = torch.zeros((1, 8), device='cuda')
    assert host(_hip.cosine_affinity(z)).tolist() == [[0.0]]


def _tie_cases():
    nb, e, groups, offs = D.TIE_SMALL
    yield 'small', nb, e, groups, offs
    nb, e, groups, offs = D.tie_large()
    yield 'large', nb, e, groups, offs


@pytest.mark.parametrize('name', ['small', 'large'])
def test_topk_ties_across_boundaries(name):
    """Columns holding one row tie bit for bit; they straddle the 63|64 half, the 127|128 tile and
    the segment boundaries, and the indices must be the lexicographic reference's exactly."""
    _, nb, e, groups, offs = next(c for c in _tie_cases() if c[0] == name)
    a, b = D.topk_tie_data(nb, e, groups)
    da, db = dev(a), dev(b)
    sa, sb = _scales(len(a), 3), _scales(nb, 4)
    worst = 0.0
    for off in offs:
        for k in (1, 3, 8):
            sc, ix, bound, gap = D.topk_with_bound(a, b, k, off)
            assert np.all((gap == 0) | (gap > 4 * bound))          # the reference decides every index
            gs, gi, _ = _hip.cosine_topk(da, db, k=k, self_offset=off)
            gs, gi = host(gs), host(gi)
            assert np.array_equal(gi, ix), (off, k)
            worst = max(worst, float((np.abs(gs - sc) / bound).max()))
            assert np.all(np.abs(gs - sc) <= bound), (off, k)
            for g, cols in enumerate(groups):                      # the ties are bit-equal on the device
                tied = gs[g][np.isin(gi[g], cols)]
                assert len(set(tied.tolist())) <= 1
            if k == 3:
                s2, i2, _ = _hip.cosine_topk(dev(a * sa[:, None]), dev(b * sb[:, None]), k=k, self_offset=off)
                assert np.array_equal(host(s2), gs) and np.array_equal(host(i2), gi)
    print(f'topk ties {name}: max err/bound {worst:.3f}')


def test_topk_multi_tile_segments():
    na, nb, e, k = D.TOPK_BIG
    tps, nseg = D.topk_tiles_per_seg(na, nb)
    assert tps == 3 and (nb + 127) // 128 - tps * (nseg - 1) == 2
    a, b = D.topk_big_data()
    sc, ix, bound, gap = D.topk_with_bound(a, b, k, None)
    sure = gap > D.TOPK_GAP
    assert (~sure).mean() <= D.TOPK_MASK_CAP                       # on the reference, before the kernel
    gs, gi, _ = _hip.cosine_topk(dev(a), dev(b), k=k)
    gs, gi = host(gs), host(gi)
    ratio = np.abs(gs - sc) / bound
    print(f'topk {na}x{nb}x{e} k={k}: max err/bound {ratio.max():.3f}, masked {(~sure).mean():.5f}')
    assert np.all(ratio <= 1.0), ratio.max()
    assert np.array_equal(gi[sure], ix[sure])
    # everywhere, masked or not: the columns of a row are distinct and each reported score is the
    # score of its reported column
    S, mag = D.cos_ref(a, b)
    assert np.all(np.diff(np.sort(gi, axis=1), axis=1) > 0)
    at = np.take_along_axis(S, gi, 1)
    assert np.all(np.abs(gs - at) <= D.cos_bound(at, np.take_along_axis(mag, gi, 1), e))


def test_topk_exact_counts():
    a, b = D.onehot_data()
    ref = (D.cos_ref(a, b)[0] >= 1.0).sum(1)
    sc, ix, cnt = _hip.cosine_topk(dev(a), dev(b), k=2, threshold=1.0)
    assert np.array_equal(host(cnt), ref)
    rs, ri = D.np_topk(D.cos_ref(a, b)[0], 2, None)
    assert np.array_equal(host(sc), rs.astype(np.float32)) and np.array_equal(host(ix), ri)


def test_topk_fewer_columns_than_k():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((3, 8)).astype(np.float32), rng.standard_normal((2, 8)).astype(np.float32)
    sc, ix, cnt = _hip.cosine_topk(dev(a), dev(b), k=4, threshold=-2.0)
    sc, ix = host(sc), host(ix)
    rs, ri = D.np_topk(D.cos_ref(a, b)[0], 2, None)
    assert np.array_equal(ix[:, :2], ri) and np.all(ix[:, 2:] == -1)
    assert np.all(np.isneginf(sc[:, 2:])) and np.all(np.isfinite(sc[:, :2]))
    assert host(cnt).tolist() == [2, 2, 2]


@pytest.mark.parametrize('e,t', D.TRIAL_CASES)
def test_trials(e, t):
    A, ia, ib = D.trial_data(e, t)
    S, mag = D.cos_ref(A, A)
    ref, bound = S[ia, ib], D.cos_bound(S, mag, e)[ia, ib]
    dA = dev(A)
    got = host(_hip.cosine_trials(dA, dA, torch.from_numpy(ia), torch.from_numpy(ib)))
    ratio = np.abs(got - ref) / bound
    print(f'trials E={e} T={t}: max err/bound {ratio.max():.3f}')
    assert np.all(ratio <= 1.0), ratio.max()
    # each trial is bit-equal to the same pair scored alone
    for q in sorted({0, t // 2, t - 1}):
        alone = host(_hip.cosine_trials(dA, dA, torch.from_numpy(ia[q:q + 1]), torch.from_numpy(ib[q:q + 1])))
        assert alone[0] == got[q]
    # power-of-two row scaling changes no bit
    s = _scales(len(A), 6)
    B = np.ascontiguousarray(A * _scales(len(A), 7)[:, None])
    base = host(_hip.cosine_trials(dA, dev(A.copy()), torch.from_numpy(ia), torch.from_numpy(ib)))
    assert np.array_equal(base, got)
    scaled = host(_hip.cosine_trials(dev(A * s[:, None]), dev(B), torch.from_numpy(ia), torch.from_numpy(ib)))
    assert np.array_equal(scaled, got)
