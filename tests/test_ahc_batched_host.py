"""The batched AHC without a device: the CLI rule of ``--ahc_batch``, the routing and ordering of
``ahc_labels_gpu_batched`` (``_hip`` calls replaced), and the host-only build of the library
(tests/emu, no kernels), which still has to link, load and check its arguments."""
import ctypes

import numpy as np
import pytest
import torch

import emu_runner
from speakerlab import _hip
from speakerlab.bin import infer_diarization as idz
from speakerlab.process import cluster as C


def test_cli_flag_rule(capsys):
    base = ['--wav', 'a.wav', '--out_dir', 'o']
    assert idz.parser.parse_args(base).ahc_batch == 1
    assert idz.parser.parse_args(base + ['--gpu_ahc', '--ahc_batch', '4']).ahc_batch == 4
    for extra in (['--ahc_batch', '2'], ['--gpu_ahc', '--ahc_batch', '0'],
                  ['--gpu_ahc', '--ahc_batch', '2', '--shard_chunks']):
        with pytest.raises(SystemExit) as ei:
            idz.main(base + extra)
        assert ei.value.code == 2                                 # an argparse error
        assert '--ahc_batch' in capsys.readouterr().err


def test_empty_list():
    assert C.ahc_labels_gpu_batched([], 0.3) == []
    assert C.AHCluster(0.3, device='gpu').from_affinities([]) == []
    assert C.CommonClustering('AHC', device='gpu').from_affinities([], []) == []


def test_routing_and_order(monkeypatch):
    """Problems above the cap go to ahc_labels_gpu one by one, the rest through ONE batched call,
    and the results come back in the order of the inputs."""
    calls = {'batched': [], 'single': []}
    monkeypatch.setattr(C, '_require_device', lambda what: None)
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)
    monkeypatch.setattr(_hip, 'ahc_batched_max_n', lambda: 8)

    def fake_batched(mats, thr):
        calls['batched'].append([S.shape[0] for S in mats])
        return [torch.full((S.shape[0],), S.shape[0], dtype=torch.int32) for S in mats], None

    def fake_single(S, thr):
        calls['single'].append(S.shape[0])
        return np.full(S.shape[0], -S.shape[0], dtype=np.int32)

    monkeypatch.setattr(_hip, 'ahc_average_batched', fake_batched)
    monkeypatch.setattr(C, 'ahc_labels_gpu', fake_single)
    sizes = [3, 9, 8, 1, 12, 5]
    out = C.ahc_labels_gpu_batched([np.eye(n, dtype=np.float32) for n in sizes], 0.3)
    assert calls == {'batched': [[3, 8, 1, 5]], 'single': [9, 12]}
    assert [o.tolist() for o in out] == [[n if n <= 8 else -n] * n for n in sizes]
    calls['batched'].clear()
    out = C.ahc_labels_gpu_batched([torch.eye(9), torch.eye(10)], 0.3)   # nothing left for the batched call
    assert calls['batched'] == [] and [o[0] for o in out] == [-9, -10]


def test_from_affinities_host_path_is_per_recording():
    rng = np.random.default_rng(0)
    Xs, Ss = [], []
    for n in (30, 50, 1):
        cen = rng.standard_normal((3, 16))
        X = (cen[rng.integers(0, 3, n)] + 0.05 * rng.standard_normal((n, 16))).astype(np.float32)
        Xs.append(X)
        Ss.append(C._host_cosine(X, X).astype(np.float32))
    cc = C.CommonClustering('AHC', mer_cos=0.3, min_cluster_size=2, fix_cos_thr=0.4)
    got = cc.from_affinities(Xs, Ss)
    assert [g.tolist() for g in got] == [cc.from_affinity(X, S).tolist() for X, S in zip(Xs, Ss)]


def test_emu_library_loads_and_checks_batched_arguments():
    lib = emu_runner.lib()                                        # binds every symbol of _hip.SYMBOLS
    cap = lib.spk_ahc_batched_max_n()
    assert cap >= 2048
    sizes = (ctypes.c_int64 * 2)(5, 7)
    nbytes = ctypes.c_size_t(0)
    assert lib.spk_ahc_average_batched_workspace_bytes(sizes, 2, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= 8 * (25 + 49) and nbytes.value % 256 == 0
    S = torch.eye(7)
    labels = [torch.full((n,), -7, dtype=torch.int32) for n in (5, 7)]
    count = torch.full((2,), -7, dtype=torch.int32)
    ws = torch.zeros(nbytes.value, dtype=torch.uint8)
    P = ctypes.c_void_p

    def call(N, lds=(7, 7), n_prob=2, ws_bytes=nbytes.value):
        return lib.spk_ahc_average_batched((P * 2)(S.data_ptr(), S.data_ptr()), (ctypes.c_int64 * 2)(*N),
                                           (ctypes.c_int64 * 2)(*lds), (ctypes.c_float * 2)(0.3, 0.4), n_prob,
                                           (P * 2)(labels[0].data_ptr(), labels[1].data_ptr()), count.data_ptr(),
                                           ws.data_ptr(), ws_bytes, None)

    assert call((5, 7)) == _hip.E_UNSUPPORTED                     # no kernels in this build
    assert b'no kernels' in lib.spk_last_error()
    assert call((5, 7), n_prob=0) == 0                            # nothing to do is a success
    assert call((5, 7), lds=(7, 6)) == -1                         # argument checks come first
    assert call((0, 7)) == -1
    assert call((5, 7), ws_bytes=nbytes.value - 1) == -5
    assert call((5, cap + 1)) == _hip.E_UNSUPPORTED and b'cap' in lib.spk_last_error()
    assert lib.spk_ahc_average_batched_workspace_bytes((ctypes.c_int64 * 2)(5, cap + 1), 2,
                                                       ctypes.byref(nbytes)) == _hip.E_UNSUPPORTED
    assert all(t.eq(-7).all() for t in labels) and count.eq(-7).all() and ws.eq(0).all()
