"""The references, bounds and case inputs of tests/data_ref.py can fail (host only, no GPU).

For every case the GPU edge tests run, a deliberately wrong copy of the fp64 reference must break
the bound the kernel is held to (so the case is able to catch that kind of kernel bug), and a
float32 numpy evaluation of the same formula must stay inside it (so the bound is not too tight
for a correct fp32 implementation)."""
import numpy as np
import pytest

import data_ref as D
from oracle import fbank_ref

AFF_IDS = [f'{na}x{nb}x{e}-{kind}' for na, nb, e, kind in D.AFF_CASES]


# ----------------------------------------------------------------------------- cosine
@pytest.mark.parametrize('na,nb,e,kind', D.AFF_CASES, ids=AFF_IDS)
def test_affinity_cases_can_fail(na, nb, e, kind):
    a, b = D.aff_data(na, nb, e, kind)
    S, mag = D.cos_ref(a, b)
    bound = D.cos_bound(S, mag, e)
    lv = D.live(a, b)                       # zero rows give exact zeros in any implementation
    assert lv.mean() > 0.9
    if kind == 'pos':
        assert np.allclose(mag, S, rtol=1e-14) and S.min() > 0.8
    # a correct fp32 evaluation stays inside
    r32 = np.abs(D.cos_f32(a, b) - S) / np.maximum(bound, 1e-300)
    assert r32[lv].max() <= 1.0 and np.all(D.cos_f32(a, b)[~lv] == 0)
    # the last 4 elements of K left out of the dot product
    bad = np.abs(D.cos_ref(a, b, drop_tail=4)[0] - S) > bound
    assert bad[lv].mean() >= 0.99, bad[lv].mean()
    # one B row displaced by one (needs a second row)
    if nb > 1:
        j = next(c for c in range(nb // 2, nb) if lv[0 if na == 1 else 1, c] and np.any(b[(c + 1) % nb] != 0))
        b2 = b.copy()
        b2[j] = b[(j + 1) % nb]
        bad = np.abs(D.cos_ref(a, b2)[0][:, j] - S[:, j]) > bound[:, j]
        assert bad[lv[:, j]].mean() >= 0.99, bad[lv[:, j]].mean()


@pytest.mark.parametrize('e,t', D.TRIAL_CASES)
def test_trial_cases_can_fail(e, t):
    A, ia, ib = D.trial_data(e, t)
    S, mag = D.cos_ref(A, A)
    ref, bound = S[ia, ib], D.cos_bound(S, mag, e)[ia, ib]
    assert ia[0] == ib[0]
    assert np.all(np.abs(D.cos_f32(A, A)[ia, ib] - ref) <= bound)
    bad = np.abs(D.cos_ref(A, A, drop_tail=4)[0][ia, ib] - ref) > bound
    assert bad.mean() >= 0.99
    bad = np.abs(S[ia, (ib + 1) % len(A)] - ref) > bound         # the B row displaced by one
    assert bad.mean() >= 0.99


def _topk_cases():
    yield 'big', D.topk_big_data(), D.TOPK_BIG[3], None
    nb, e, groups, offs = D.TIE_SMALL
    for off in offs:
        yield f'tie_small_off{off}', D.topk_tie_data(nb, e, groups), 8, off
    nb, e, groups, offs = D.tie_large()
    for off in offs:
        yield f'tie_large_off{off}', D.topk_tie_data(nb, e, groups), 8, off


@pytest.mark.parametrize('name', [c[0] for c in _topk_cases()])
def test_topk_cases_can_fail(name):
    (a, b), k, off = next(c[1:] for c in _topk_cases() if c[0] == name)
    e = a.shape[1]
    sc, ix, bound, gap = D.topk_with_bound(a, b, k, off)
    # fp32 evaluation: its top-k scores stay inside the bound of the reference's
    s32 = D.np_topk(D.cos_f32(a, b).astype(np.float64), k, off)[0]
    assert np.all(np.abs(s32 - sc) <= bound)
    bad = np.abs(D.topk_with_bound(a, b, k, off, drop_tail=4)[0] - sc) > bound
    assert bad.mean() >= 0.99, bad.mean()
    if name == 'big':
        tps, nseg = D.topk_tiles_per_seg(len(a), len(b))
        assert tps == 3 and (len(b) + 127) // 128 - tps * (nseg - 1) == 2
        assert (gap <= D.TOPK_GAP).mean() <= D.TOPK_MASK_CAP
    else:
        # the ties are real (bit-equal fp64 scores inside the top k) and everything else in the
        # top k + 1 is separated by far more than the bound, so exact index equality is decidable
        assert np.any(gap == 0)
        assert np.all((gap == 0) | (gap > 4 * bound))
        # an implementation that breaks ties highest index first gives other indices
        S = D.cos_ref(a, b)[0]
        rev = D.np_topk(S[:, ::-1], k, None)[1] if off is None else None
        if rev is not None:
            assert np.any(len(b) - 1 - rev != ix)


def test_exact_count_case_can_fail():
    a, b, ref = _onehot_counts()
    assert set(np.unique(D.cos_ref(a, b)[0])) == {0.0, 1.0}
    assert ref.min() >= 1 and len(set(ref)) > 3
    assert np.any((D.cos_ref(a, b, drop_tail=4)[0] >= 1.0).sum(1) != ref)


def _onehot_counts():
    a, b = D.onehot_data()
    return a, b, (D.cos_ref(a, b)[0] >= 1.0).sum(1)


# ----------------------------------------------------------------------------- Fbank
def _fbank_cases():
    for name, wav in D.fbank_signals().items():
        yield name, wav
    for n in D.FB_LENGTHS:
        yield f'len{n}', D.noise(n, 0.1, n)


ALL_FLOOR = {'constant', 'noise_2^-30', 'noise_2^-24'}     # every band of every frame is on the floor
# every frame of these signals is the same frame (the tone's period divides the frame shift), so a
# frame swap changes nothing and the mean-normalised features are zero up to fp64 noise
STATIONARY = {'constant', 'nyquist', 'tone_bin_centre'}


@pytest.mark.parametrize('n_mels', D.N_MELS)
@pytest.mark.parametrize('name', [c[0] for c in _fbank_cases()])
def test_fbank_cases_can_fail(name, n_mels):
    wav = dict(_fbank_cases())[name]
    ref = fbank_ref.fbank(wav, n_mels, False, dtype=np.float64)
    en = D.fbank_energies(wav, n_mels)
    assert np.array_equal(np.log(np.maximum(en, D.FLT_EPS)), ref)
    b = D.fbank_bound(ref)
    f32 = D.fbank_log_f32(en)
    assert np.all(np.abs(f32 - ref) <= b)
    assert np.all(f32[D.on_floor(en)] == D.FLOOR32)
    ref_mn = ref - ref.mean(0, keepdims=True)
    f32_mn = (f32.astype(np.float64) - f32.astype(np.float64).mean(0, keepdims=True)).astype(np.float32)
    assert np.all(np.abs(f32_mn - ref_mn) <= D.fbank_mn_bound(ref, ref_mn))
    if name in ALL_FLOOR:
        # no band or frame mutant can show; the check there is exact equality with FLOOR32, which
        # a value one float32 step away fails
        assert D.on_floor(en).all() and np.nextafter(D.FLOOR32, np.float32(0)) != D.FLOOR32
        return
    # band m taken from band m + 1
    assert np.any(np.abs(np.roll(ref, -1, axis=1) - ref) > b)
    if ref.shape[0] >= 2 and name not in STATIONARY:
        # (one frame, or equal frames, normalise to zero: only the form without mean_nor can show it)
        assert np.any(np.abs(np.roll(ref_mn, -1, axis=1) - ref_mn) > D.fbank_mn_bound(ref, ref_mn))
        # the second frame of a pair swapped with the first
        sw = ref.copy()
        sw[[0, 1]] = sw[[1, 0]]
        assert np.any(np.abs(sw - ref) > b)
    else:
        assert ref.shape[0] == 1 or np.abs(ref[0] - ref[1]).max() < 1e-9


def test_fbank_signal_properties():
    sig = D.fbank_signals()
    e = D.fbank_energies(sig['noise_mixed_floor'], 80)
    assert 0.2 <= D.on_floor(e).mean() <= 0.8
    e = D.fbank_energies(sig['noise_half_to_one'], 80)
    assert ((e >= 0.5) & (e < 1.0)).mean() >= 0.10
    assert D.on_floor(D.fbank_energies(sig['noise_2^-30'], 80)).all()
    assert not D.on_floor(D.fbank_energies(sig['noise_2^0'], 80)).any()
    assert [fbank_ref.num_frames(n) for n in D.FB_LENGTHS] == [1, 1, 2, 3, 7]


# ----------------------------------------------------------------------------- Laplacian
@pytest.mark.parametrize('n', [1, 2, 31, 33, 1025])
def test_laplacian_reference_and_bound(n):
    S = D.random_affinity(n, n)
    for ne in D.lap_n_elems(n):
        L, rowabs = D.laplacian_ref(S, ne)
        f32 = D.laplacian_f32(S, ne)
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(f32[off], L[off])
        assert np.all(np.abs(np.diag(f32) - np.diag(L)) <= D.laplacian_diag_bound(n, rowabs))
        assert np.array_equal(L, L.T)
        if 0 < ne < n - 1:
            assert not np.array_equal(D.laplacian_ref(S, ne + 1)[0][off], L[off])      # one more pruned shows


def test_tie_matrix_cut_crosses_chunks():
    """The tie rule matters: at N = 2050 rows have hundreds of ties at the cut, ending past column
    2048, and zeroing the HIGHEST indices first gives another matrix."""
    n = 2050
    S = D.tie_matrix(n, 7)
    ne = int(0.3 * n)
    found = 0
    for row in S:
        thr = np.sort(row, kind='stable')[ne - 1]
        ties = np.flatnonzero(row == thr)
        need = ne - int((row < thr).sum())
        # the cut falls inside the ties, past the first 1024-column chunk, and ties go on past 2048
        found += len(ties) > 200 and 0 < need < len(ties) and ties[-1] >= 2048 and ties[need - 1] >= 1024
    assert found > 10
    L = D.laplacian_ref(S, ne)[0]
    hi = S.copy()
    for i in range(n):
        order = np.lexsort((-np.arange(n), S[i]))                       # ties: highest index first
        hi[i, order[:ne]] = 0
    M = np.float32(0.5) * (hi + hi.T)
    off = ~np.eye(n, dtype=bool)
    assert not np.array_equal(-M[off], L[off])


def test_fbank_tables_accept_the_tested_n_mels():
    acc = D.fbank_tables_accept(D.N_MELS + (3, 129))
    assert [n for n in D.N_MELS if acc[n]] == list(D.N_MELS)      # all six run on the GPU
    assert not acc[3] and not acc[129]


def test_eig_constant_covers_float32_lapack():
    """float32 numpy.linalg.eigh on the eigensolver cases: the figures behind EIG_C (a quarter of
    it at worst when they were recorded; half is allowed for another LAPACK build)."""
    from test_gpu_spectral_edges import EIG_C
    for name, (A, cliques) in D.eig_cases().items():
        w, v = np.linalg.eigh(A)
        assert w.dtype == np.float32
        assert max(D.eig_quantities(A, w, v.T)) <= EIG_C / 2, name
        if cliques:
            assert int((np.abs(w) < 1e-4 * np.abs(w).max()).sum()) == cliques
