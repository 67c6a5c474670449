"""Average-linkage AHC on the GPU (``spk_ahc_average``, csrc/ahc.hip) behind
``AHCluster(device='gpu')``: edges, the tie rule against a float64 numpy restatement of the same
greedy loop (labels equal, not merely the partitions), the host path (scipy linkage + fcluster)
on the same device-computed affinity, the reference's AHC fixtures, ABI misuse and the CLI flag.

Host-path cases are conditioned on their inputs: no merge height of the host's float64 linkage
lies within 1e-3 of the threshold (asserted).  The fp64 device update differs from scipy's by
rounding at the 1e-16 level (its NN-chain merges in another order), so a merge can only flip
across the threshold inside that margin."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import squareform

from speakerlab import _hip
from speakerlab.process import cluster as C

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cluster_golden.npz'))
AHC_NAMES = [n for n in json.loads(G['names'].tobytes())
             if json.loads(G[f'{n}/ctor'].tobytes()).get('cluster_type') == 'AHC']


def canon(labels):
    m = {}
    return [m.setdefault(int(v), len(m)) for v in labels]


def embeddings(n, spk, noise, seed, E=192):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((spk, E))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    lab = rng.integers(0, spk, n)
    return (cen[lab] + noise * rng.standard_normal((n, E))).astype(np.float32)


def greedy(S, thr):
    """The loop of csrc/ahc.hip in float64 numpy: the upper triangle of S mirrored, the largest
    average similarity first (ties: smallest row, then smallest column -- argmax over the
    row-major upper triangle), the merged cluster keeps the smaller index, stop below float32(thr);
    labels by first occurrence."""
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


def gpu(S, thr):
    labels, count = _hip.ahc_average(torch.as_tensor(S).cuda(), thr, return_count=True)
    labels = labels.cpu().numpy()
    assert labels.dtype == np.int32 and int(count.item()) == int(labels.max()) + 1
    return labels


# ---------------------------------------------------------------------------------- edges
def test_one_row():
    assert gpu(np.ones((1, 1), np.float32), 0.3).tolist() == [0]
    assert C.ahc_labels_gpu(torch.ones(1, 1, device='cuda'), 0.3).tolist() == [0]


@pytest.mark.parametrize('thr, want', [(0.4, [0, 0]), (0.6, [0, 1])])
def test_two_rows(thr, want):
    S = np.array([[1.0, 0.5], [0.5, 1.0]], np.float32)
    assert gpu(S, thr).tolist() == want


@pytest.mark.parametrize('n', [2, 63, 257])
def test_threshold_extremes(n):
    S = _hip.cosine_affinity(torch.from_numpy(embeddings(n, 4, 0.1, n)).cuda())
    assert gpu(S, -2.0).tolist() == [0] * n            # everything merges
    assert gpu(S, 2.0).tolist() == list(range(n))      # nothing does


def test_row_stride_above_n():
    n = 65
    S = _hip.cosine_affinity(torch.from_numpy(embeddings(n, 5, 0.08, 1)).cuda())
    wide = torch.full((n, n + 7), 9.0, device='cuda')     # 9: would merge first if it were read
    wide[:, :n] = S
    view = wide[:, :n]
    assert view.stride(0) == n + 7
    before = wide.clone()
    assert gpu(view, 0.3).tolist() == gpu(S, 0.3).tolist() == greedy(S.cpu().numpy(), 0.3).tolist()
    assert torch.equal(wide, before)                      # S is not modified


@pytest.mark.parametrize('n', [63, 65, 257])
def test_odd_sizes_match_numpy_loop(n):
    S = _hip.cosine_affinity(torch.from_numpy(embeddings(n, 6, 0.07, 100 + n)).cuda())
    for thr in (0.2, 0.5):
        want = greedy(S.cpu().numpy(), thr)
        assert 1 < want.max() + 1 < n
        assert gpu(S, thr).tolist() == want.tolist()


# ---------------------------------------------------------------------------------- tie rule
@pytest.mark.parametrize('n, thr', [(65, 0.3), (130, 0.45), (257, 0.3)])
def test_ties_duplicated_rows(n, thr):
    X = embeddings(n // 3 + 1, 4, 0.1, n)
    X = np.concatenate([X, X, X])[:n]                      # every row two or three times
    X = X[np.random.default_rng(n).permutation(n)]
    S = _hip.cosine_affinity(torch.from_numpy(X).cuda())
    Sh = S.cpu().numpy()
    vals, counts = np.unique(Sh[np.triu_indices(n, 1)], return_counts=True)
    assert counts.max() > 1                                # the input does contain exact ties
    assert gpu(S, thr).tolist() == greedy(Sh, thr).tolist()


@pytest.mark.parametrize('n, thr', [(64, 0.45), (65, 0.5), (130, 0.45), (257, 0.42)])
def test_ties_few_distinct_values(n, thr):
    rng = np.random.default_rng(7 * n)
    S = rng.choice(np.array([0.1, 0.3, 0.5, 0.7], np.float32), size=(n, n))
    S = np.triu(S, 1) + np.triu(S, 1).T + np.eye(n, dtype=np.float32)
    want = greedy(S, thr)
    assert 1 < want.max() + 1 < n
    assert gpu(S, thr).tolist() == want.tolist()
    lower_garbage = np.triu(S) + np.tril(rng.random((n, n)).astype(np.float32), -1)
    assert gpu(lower_garbage, thr).tolist() == want.tolist()   # only the upper triangle is read


# ---------------------------------------------------------------------------------- host path
# (N, speakers, noise, threshold, seed): seeds and thresholds picked on the CPU for the margin
# below; cluster counts 2, 5, 111, 295, 8, 40 and 286
HOST_CASES = [(41, 2, 0.05, 0.3, 0), (130, 5, 0.06, 0.4, 0), (300, 120, 0.05, 0.4, 0), (300, 8, 0.12, 0.45, 6),
              (1025, 8, 0.05, 0.3, 0), (1025, 40, 0.09, 0.3, 0), (1025, 300, 0.05, 0.4, 0)]
_counts = {}


@pytest.mark.parametrize('n, spk, noise, thr, seed', HOST_CASES)
def test_matches_host_path(n, spk, noise, thr, seed):
    S = _hip.cosine_affinity(torch.from_numpy(embeddings(n, spk, noise, seed)).cuda())
    Sh = S.cpu().numpy()
    heights = linkage(squareform(-Sh, checks=False), method='average')[:, 2]
    margin = np.abs(heights + thr).min()
    assert margin > 1e-3, f'a merge height lies {margin:.2e} from the threshold: pick another seed'
    host = C.ahc_labels(Sh, thr)
    got = C.ahc_labels_gpu(S, thr)
    _counts[(n, spk, noise, thr, seed)] = int(host.max()) + 1
    print(f'N {n}: {int(host.max()) + 1} clusters, margin {margin:.2e}')
    assert canon(got) == got.tolist()                      # already numbered by first occurrence
    assert got.tolist() == canon(host)
    assert C.ahc_labels_gpu(Sh, thr).tolist() == got.tolist()   # an ndarray is accepted too


def test_host_cases_span_cluster_counts():
    counts = []
    for n, spk, noise, thr, seed in HOST_CASES:
        if (n, spk, noise, thr, seed) not in _counts:       # run alone: recompute on the host
            X = embeddings(n, spk, noise, seed)
            _counts[(n, spk, noise, thr, seed)] = int(C.ahc_labels(C._host_cosine(X, X).astype(np.float32), thr).max()) + 1
        counts.append(_counts[(n, spk, noise, thr, seed)])
    assert min(counts) == 2 and max(counts) > 100


# ---------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize('name', AHC_NAMES)
def test_reference_fixtures(name):
    X = G[f'{name}/X']
    ctor = json.loads(G[f'{name}/ctor'].tobytes())
    call = json.loads(G[f'{name}/call'].tobytes())
    cc = C.CommonClustering(**ctor, device='gpu')
    assert cc.cluster.device == 'gpu' and cc.cluster_for_short.device == 'gpu'
    np.random.seed(int(G[f'{name}/seed']))
    assert canon(cc(X.copy(), **call)) == G[f'{name}/canon'].tolist()
    S = _hip.cosine_affinity(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda())
    assert canon(cc.from_affinity(X.copy(), S, **call)) == G[f'{name}/canon'].tolist()


def test_fixture_list_is_not_empty():
    assert len(AHC_NAMES) >= 3


def test_from_affinity_keeps_the_matrix_on_the_device(monkeypatch):
    S = _hip.cosine_affinity(torch.from_numpy(embeddings(50, 3, 0.05, 2)).cuda())
    monkeypatch.setattr(C, 'ahc_labels', lambda *a, **k: pytest.fail('host AHC called'))
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (
        pytest.fail('N x N copy to the host') if self.dim() == 2 else self.to('cpu')))
    labels = C.AHCluster(0.3, device='gpu').from_affinity(S)
    assert labels.max() + 1 == 3


def test_unsupported_falls_back_to_host(monkeypatch):
    S = _hip.cosine_affinity(torch.from_numpy(embeddings(41, 2, 0.05, 0)).cuda())

    def over_cap(*a, **k):
        e = _hip.HipError('over the cap')
        e.code = _hip.E_UNSUPPORTED
        raise e
    monkeypatch.setattr(_hip, 'ahc_average', over_cap)
    assert C.ahc_labels_gpu(S, 0.3).tolist() == C.ahc_labels(S.cpu().numpy(), 0.3).tolist()


# ---------------------------------------------------------------------------------- ABI misuse
def test_abi_misuse_writes_nothing():
    lib = _hip.lib()
    n = 33
    S = _hip.cosine_affinity(torch.from_numpy(embeddings(n, 3, 0.05, 3)).cuda())
    need = _hip.ahc_workspace_bytes(n)
    assert need >= 8 * n * n
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    labels = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    count = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def call(N, lds, ws_bytes, s=S.data_ptr(), lab=labels.data_ptr()):
        return lib.spk_ahc_average(s, N, lds, 0.3, lab, count.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    assert call(n, n, need - 1) == -5                       # SPK_E_WORKSPACE
    assert call(n, n - 1, need) == -1                       # SPK_E_INVALID
    assert call(0, n, need) == -1
    assert call(n, n, need, s=None) == -1
    assert call(n, n, need, lab=None) == -1
    assert call(32769, 32769, need) == -6                   # SPK_E_UNSUPPORTED: over the cap
    nbytes = ctypes.c_size_t(5)
    assert lib.spk_ahc_workspace_bytes(32769, ctypes.byref(nbytes)) == -6 and nbytes.value == 5
    assert lib.spk_ahc_workspace_bytes(0, ctypes.byref(nbytes)) == -1
    assert lib.spk_ahc_workspace_bytes(32768, ctypes.byref(nbytes)) == 0 and nbytes.value >= 8 * 32768 ** 2
    torch.cuda.synchronize()
    assert labels.eq(-7).all() and count.eq(-7).all() and ws.eq(0).all()
    with pytest.raises(_hip.HipError) as ei:
        _hip.ahc_workspace_bytes(32769)
    assert ei.value.code == _hip.E_UNSUPPORTED
    assert call(n, n, need) == 0                            # and the same buffers do work
    assert labels.cpu().tolist() == C.ahc_labels_gpu(S, 0.3).tolist()


# ---------------------------------------------------------------------------------- CLI
def test_cli_gpu_ahc_same_rttm(tmp_path):
    from speakerlab.bin import infer_diarization as idz
    from speakerlab.utils import synthetic
    from speakerlab.utils.fileio import write_wav
    wav, _ = synthetic.synth_meeting(12.0, 2, seed=5)       # the meeting of tests/test_gpu_diarization.py
    p = tmp_path / 'meet.wav'
    write_wav(str(p), wav)
    base = ['--wav', str(p), '--out_type', 'rttm', '--synthetic_weights', '--vad', 'energy', '--diable_progress_bar',
            '--nprocs', '1']
    idz.main(base + ['--out_dir', str(tmp_path / 'host')])
    idz.main(base + ['--out_dir', str(tmp_path / 'gpu'), '--gpu_ahc'])
    host = (tmp_path / 'host' / 'meet.rttm').read_text()
    assert len(host.splitlines()) >= 1
    assert (tmp_path / 'gpu' / 'meet.rttm').read_text() == host
