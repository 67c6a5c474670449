"""Batched single-launch AHC (``spk_ahc_average_batched``, csrc/ahc_batched.hip) behind
``ahc_labels_gpu_batched`` / ``from_affinities``.  The reference for labels is ``_hip.ahc_average``
(three launches per merge) on the same device affinity, labels and cluster counts equal exactly;
the tie cases compare with the float64 numpy restatement of the greedy loop (``greedy`` below, the
one of tests/test_gpu_ahc.py) instead."""
import ctypes

import numpy as np
import pytest
import torch

from speakerlab import _hip
from speakerlab.process import cluster as C

pytestmark = pytest.mark.gpu


def canon(labels):
    m = {}
    return [m.setdefault(int(v), len(m)) for v in labels]


def embeddings(n, spk, noise, seed, E=192):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((spk, E))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    lab = rng.integers(0, spk, n)
    return (cen[lab] + noise * rng.standard_normal((n, E))).astype(np.float32)


def affinity(n, spk=5, noise=0.08, seed=0):
    return _hip.cosine_affinity(torch.from_numpy(embeddings(n, spk, noise, seed)).cuda())


def greedy(S, thr):
    """The loop of csrc/ahc.hip in float64 numpy: the upper triangle of S mirrored, the largest
    average similarity first (ties: smallest row, then smallest column), the merged cluster keeps
    the smaller index, stop below float32(thr); labels by first occurrence."""
    A = np.array(S, dtype=np.float64)
    n = A.shape[0]
    iu = np.triu_indices(n, 1)
    A[(iu[1], iu[0])] = A[iu]
    upper = np.arange(n)[:, None] < np.arange(n)[None, :]
    size = np.ones(n, dtype=np.int64)
    act = np.ones(n, dtype=bool)
    mem = np.arange(n)
    thr = float(np.float32(thr))
    while act.sum() > 1:
        M = np.where(act[:, None] & act[None, :] & upper, A, -np.inf)
        i, j = divmod(int(np.argmax(M)), n)
        if not M[i, j] >= thr:
            break
        row = (size[i] * A[i] + size[j] * A[j]) / (size[i] + size[j])
        keep = act.copy()
        keep[[i, j]] = False
        A[i, keep] = row[keep]
        A[keep, i] = row[keep]
        size[i] += size[j]
        act[j] = False
        mem[mem == j] = i
    return np.array(canon(mem), dtype=np.int32)


def batched(mats, thrs):
    """(list of label lists, list of counts) of one batched call."""
    labels, counts = _hip.ahc_average_batched([torch.as_tensor(S).cuda() for S in mats], thrs)
    assert all(t.dtype == torch.int32 for t in labels) and counts.dtype == torch.int32
    return [t.cpu().tolist() for t in labels], counts.cpu().tolist()


def single(S, thr):
    labels, count = _hip.ahc_average(torch.as_tensor(S).cuda(), thr, return_count=True)
    return labels.cpu().tolist(), int(count.item())


def assert_same_as_single(mats, thrs):
    got, counts = batched(mats, thrs)
    for S, thr, lab, cnt in zip(mats, thrs, got, counts):
        assert (lab, cnt) == single(S, thr)
    return got


# ---------------------------------------------------------------------------------- sizes
def test_one_row():
    assert batched([np.ones((1, 1), np.float32)], 0.3) == ([[0]], [1])


@pytest.mark.parametrize('thr, want', [(0.4, [0, 0]), (0.6, [0, 1])])
def test_two_rows(thr, want):
    S = np.array([[1.0, 0.5], [0.5, 1.0]], np.float32)
    assert batched([S], thr) == ([want], [max(want) + 1])


@pytest.mark.parametrize('n', [63, 64, 65, 1023, 1024, 1025])
def test_sizes_at_kernel_boundaries(n):
    S = affinity(n, 6, 0.07, 100 + n)
    for thr in (0.2, 0.5):
        lab, = assert_same_as_single([S], [thr])
        assert 1 < max(lab) + 1 < n


# ---------------------------------------------------------------------------------- ties
def tie_matrix(n):
    """Few distinct values: equal maxima in different rows and within one row from the start, and
    ties that averaging two equal rows creates later."""
    rng = np.random.default_rng(7 * n)
    S = rng.choice(np.array([0.1, 0.3, 0.5, 0.7], np.float32), size=(n, n))
    S = np.triu(S, 1) + np.triu(S, 1).T + np.eye(n, dtype=np.float32)
    S[0, 1] = S[1, 0] = S[0, 2] = S[2, 0] = S[3, 4] = S[4, 3] = 0.7   # one row twice, another row once
    S[1, 5] = S[5, 1] = 0.3                                            # merging 0 and 1 makes A[0][5] ...
    S[0, 5] = S[5, 0] = 0.7                                            # ... (0.7 + 0.3) / 2 = 0.5 = A[2][5]
    S[2, 5] = S[5, 2] = 0.5
    return S


@pytest.mark.parametrize('n, thr', [(6, 0.45), (40, 0.45)])
def test_ties_match_numpy_loop(n, thr):
    S = tie_matrix(n)
    up = S[np.triu_indices(n, 1)]
    assert (up == up.max()).sum() > 2 and (S[0, 1:] == up.max()).sum() >= 2
    want = greedy(S, thr)
    assert want.max() + 1 < n
    got, counts = batched([S], thr)
    assert got[0] == want.tolist() and counts[0] == want.max() + 1


# ---------------------------------------------------------------------------------- batches
def test_heterogeneous_batch_and_order():
    sizes = [1, 2, 40, 129, 700]
    thrs = [0.3, 0.45, 0.25, 0.5, 0.35]
    views, wides = [], []
    for q, n in enumerate(sizes):
        S = affinity(n, 5, 0.08, 10 + n)
        wide = torch.full((n, n + 3 + q), 9.0, device='cuda')   # 9: would merge first if it were read
        wide[:, :n] = S
        wides.append(wide)
        views.append(wide[:, :n])
        assert views[-1].stride(0) > n
    before = [w.clone() for w in wides]
    got = assert_same_as_single(views, thrs)
    assert len({max(g) + 1 for g in got}) > 2                   # the problems do differ
    back, back_counts = batched(views[::-1], thrs[::-1])
    assert back[::-1] == got and back_counts[::-1] == [max(g) + 1 for g in got]
    assert all(torch.equal(w, b) for w, b in zip(wides, before))


@pytest.mark.parametrize('n', [2, 65, 257])
def test_threshold_extremes(n):
    S = affinity(n, 4, 0.1, n)
    got, counts = batched([S, S], [2.0, -2.0])
    assert got == [list(range(n)), [0] * n] and counts == [n, 1]


def test_separated_speakers_match_host():
    S = affinity(300, 4, 0.05, 3)
    host = C.ahc_labels(S.cpu().numpy(), 0.3)
    assert host.max() + 1 == 4
    got, = C.ahc_labels_gpu_batched([S], 0.3)
    assert got.dtype == np.int32 and got.tolist() == canon(host)


def test_same_workspace_twice_is_bit_identical():
    mats = [affinity(n, 6, 0.09, n) for n in (300, 65, 130)]
    before = [S.clone() for S in mats]
    first = batched(mats, [0.3, 0.4, 0.5])
    ws = dict(_hip._ahc_ws)
    again = batched(mats, [0.3, 0.4, 0.5])
    assert {k: v.data_ptr() for k, v in _hip._ahc_ws.items()} == {k: v.data_ptr() for k, v in ws.items()}
    assert again == first
    assert all(torch.equal(S, b) for S, b in zip(mats, before))


# ---------------------------------------------------------------------------------- the cap
def two_blocks(n):
    S = torch.full((n, n), 0.1, device='cuda')
    h = n // 3
    S[:h, :h] = 0.9
    S[h:, h:] = 0.8
    S.fill_diagonal_(1.0)
    return S


def test_cap():
    lib = _hip.lib()
    cap = _hip.ahc_batched_max_n()
    assert cap >= 2048
    sizes = (ctypes.c_int64 * 2)(5, cap + 1)
    nbytes = ctypes.c_size_t(7)
    assert lib.spk_ahc_average_batched_workspace_bytes(sizes, 2, ctypes.byref(nbytes)) == _hip.E_UNSUPPORTED
    assert nbytes.value == 7 and b'cap' in lib.spk_last_error()
    S = two_blocks(cap + 1)
    with pytest.raises(_hip.HipError) as ei:
        _hip.ahc_average_batched([S[:5, :5], S], 0.3)
    assert ei.value.code == _hip.E_UNSUPPORTED and 'cap' in str(ei.value)
    # the raw entry: the error comes before any launch, nothing is written
    lab = [torch.full((5,), -7, dtype=torch.int32, device='cuda'), torch.full((cap + 1,), -7, dtype=torch.int32, device='cuda')]
    count = torch.full((2,), -7, dtype=torch.int32, device='cuda')
    ws = torch.zeros(1024, dtype=torch.uint8, device='cuda')
    P = ctypes.c_void_p
    rc = lib.spk_ahc_average_batched((P * 2)(S.data_ptr(), S.data_ptr()), sizes, (ctypes.c_int64 * 2)(cap + 1, cap + 1),
                                     (ctypes.c_float * 2)(0.3, 0.3), 2, (P * 2)(lab[0].data_ptr(), lab[1].data_ptr()),
                                     count.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == _hip.E_UNSUPPORTED and b'cap' in lib.spk_last_error()
    torch.cuda.synchronize()
    assert all(t.eq(-7).all() for t in lab) and count.eq(-7).all() and ws.eq(0).all()


def test_over_cap_problem_falls_back_inside_a_list():
    cap = _hip.ahc_batched_max_n()
    big = two_blocks(cap + 1)
    small = [affinity(65, 4, 0.08, 1), affinity(40, 3, 0.08, 2)]
    got = C.ahc_labels_gpu_batched([small[0], big, small[1]], 0.3)
    h = (cap + 1) // 3
    assert got[1].tolist() == [0] * h + [1] * (cap + 1 - h)
    assert got[0].tolist() == C.ahc_labels_gpu(small[0], 0.3).tolist()
    assert got[2].tolist() == C.ahc_labels_gpu(small[1], 0.3).tolist()


def test_abi_misuse_and_empty_call():
    lib = _hip.lib()
    n = 33
    S = affinity(n, 3, 0.05, 3)
    sizes = (ctypes.c_int64 * 1)(n)
    need = ctypes.c_size_t(0)
    assert lib.spk_ahc_average_batched_workspace_bytes(sizes, 1, ctypes.byref(need)) == 0
    assert need.value >= 8 * n * n
    ws = torch.zeros(need.value, dtype=torch.uint8, device='cuda')
    labels = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    count = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    P = ctypes.c_void_p

    def call(N, lds, ws_bytes, n_prob=1, s=S.data_ptr()):
        return lib.spk_ahc_average_batched((P * 1)(s), (ctypes.c_int64 * 1)(N), (ctypes.c_int64 * 1)(lds),
                                           (ctypes.c_float * 1)(0.3), n_prob, (P * 1)(labels.data_ptr()),
                                           count.data_ptr(), ws.data_ptr(), ws_bytes,
                                           torch.cuda.current_stream().cuda_stream)

    assert call(n, n, need.value - 1) == -5                 # SPK_E_WORKSPACE
    assert call(n, n - 1, need.value) == -1                 # SPK_E_INVALID
    assert call(0, n, need.value) == -1
    assert call(n, n, need.value, s=None) == -1
    assert call(n, n, need.value, n_prob=-1) == -1
    assert call(n, n, need.value, n_prob=0) == 0            # success, launches nothing
    torch.cuda.synchronize()
    assert labels.eq(-7).all() and count.eq(-7).all() and ws.eq(0).all()
    assert call(n, n, need.value) == 0                      # and the same buffers do work
    assert (labels.cpu().tolist(), int(count.item())) == single(S, 0.3)
    assert _hip.ahc_average_batched([], 0.3)[0] == []


def test_more_problems_than_one_launch_takes():
    mats = [affinity(20 + q % 7, 3, 0.08, q) for q in range(70)]   # 64 descriptors travel per launch
    thrs = [0.25 + 0.005 * q for q in range(70)]
    got, counts = batched(mats, thrs)
    for q in (0, 1, 63, 64, 69):
        assert (got[q], counts[q]) == single(mats[q], thrs[q])
    assert [max(g) + 1 for g in got] == counts


# ---------------------------------------------------------------------------------- from_affinities
def test_from_affinities_equals_from_affinity():
    cc = C.CommonClustering('AHC', mer_cos=0.3, min_cluster_size=4, fix_cos_thr=0.3, device='gpu')
    Xs = [embeddings(n, spk, 0.06, 40 + n) for n, spk in ((30, 2), (130, 5), (301, 4))]   # below and above cluster_line
    Ss = [_hip.cosine_affinity(torch.from_numpy(X).cuda()) for X in Xs]
    want = [cc.from_affinity(X.copy(), S) for X, S in zip(Xs, Ss)]
    got = cc.from_affinities([X.copy() for X in Xs], Ss)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    assert len({int(w.max()) for w in want}) > 1
    flat = C.AHCluster(0.3, device='gpu')
    assert [g.tolist() for g in flat.from_affinities(Ss)] == [flat.from_affinity(S).tolist() for S in Ss]
