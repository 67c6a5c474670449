"""The device AHC is opt-in: without ``device='gpu'`` / ``--gpu_ahc`` every path is the host's,
the option is plumbed from the CLI to the back-end, and the host-only build of the library
(tests/emu, no kernels) answers SPK_E_UNSUPPORTED after its argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import emu_runner
from speakerlab import _hip
from speakerlab.bin import infer_diarization as idz
from speakerlab.process import cluster as C


def _embeddings(n=30, seed=0):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((3, 16))
    return (cen[rng.integers(0, 3, n)] + 0.05 * rng.standard_normal((n, 16))).astype(np.float32)


def test_default_is_the_host_path(monkeypatch):
    X = _embeddings()
    S = C._host_cosine(X, X).astype(np.float32)
    monkeypatch.setattr(C, 'ahc_labels_gpu', lambda *a, **k: pytest.fail('device AHC called without device="gpu"'))
    monkeypatch.setattr(C, 'cosine_affinity', lambda X: S)       # no device here
    want = C.ahc_labels(S, 0.4)
    assert want.max() + 1 == 3
    a = C.AHCluster()
    assert a.device == 'host' and a.fix_cos_thr == 0.4
    assert a(X).tolist() == want.tolist()
    assert a.from_affinity(S).tolist() == want.tolist()
    assert a.from_affinity(torch.from_numpy(S)).tolist() == want.tolist()
    for n in (30, 50):                                            # below and above cluster_line
        X = _embeddings(n, 1)
        S = C._host_cosine(X, X).astype(np.float32)
        cc = C.CommonClustering('AHC', min_cluster_size=0, fix_cos_thr=0.4)
        assert cc.cluster.device == 'host' and cc.cluster_for_short is cc.cluster
        assert cc(X).tolist() == C.ahc_labels(S, 0.4).tolist()
        assert cc.from_affinity(X, S).tolist() == C.ahc_labels(S, 0.4).tolist()
    assert C.CommonClustering('spectral').cluster_for_short.device == 'host'


def test_device_keyword_reaches_both_instances():
    cc = C.CommonClustering('AHC', fix_cos_thr=0.3, device='gpu')
    assert cc.cluster.device == 'gpu' and cc.cluster_for_short.device == 'gpu'
    with pytest.raises(ValueError):
        C.AHCluster(device='tpu')


def test_gpu_without_a_device_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    X = _embeddings()
    S = C._host_cosine(X, X).astype(np.float32)
    with pytest.raises(_hip.HipError):
        C.ahc_labels_gpu(S, 0.3)
    with pytest.raises(_hip.HipError):
        C.AHCluster(0.3, device='gpu')(X)
    with pytest.raises(_hip.HipError):
        C.AHCluster(0.3, device='gpu').from_affinity(S)
    with pytest.raises(_hip.HipError):
        _hip.ahc_average(torch.from_numpy(S), 0.3)


def test_cli_flag_is_plumbed():
    base = ['--wav', 'a.wav', '--out_dir', 'o']
    assert idz.parser.parse_args(base).gpu_ahc is False
    assert idz.parser.parse_args(base + ['--gpu_ahc']).gpu_ahc is True
    assert idz.get_cluster_backend().cluster.device == 'host'
    assert idz.get_cluster_backend(0.3, 0.3, 0).cluster.device == 'host'
    cc = idz.get_cluster_backend(0.3, 0.25, 0, gpu_ahc=True)
    assert cc.cluster.device == 'gpu' and cc.cluster_for_short.device == 'gpu' and cc.cluster.fix_cos_thr == 0.25


def test_emu_library_loads_and_has_no_ahc_kernels():
    lib = emu_runner.lib()                                        # binds every symbol of _hip.SYMBOLS
    assert lib.spk_version() == 2
    n = 5
    nbytes = ctypes.c_size_t(0)
    assert lib.spk_ahc_workspace_bytes(n, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= 8 * n * n + 8 * n + 6 * 4 * n and nbytes.value % 256 == 0
    S = torch.eye(n)
    labels = torch.full((n,), -7, dtype=torch.int32)
    count = torch.full((1,), -7, dtype=torch.int32)
    ws = torch.zeros(nbytes.value, dtype=torch.uint8)

    def call(N, lds, ws_bytes):
        return lib.spk_ahc_average(S.data_ptr(), N, lds, 0.3, labels.data_ptr(), count.data_ptr(), ws.data_ptr(),
                                   ws_bytes, None)

    assert call(n, n, nbytes.value) == _hip.E_UNSUPPORTED         # no kernels in this build
    assert b'no kernels' in lib.spk_last_error()
    assert call(n, n - 1, nbytes.value) == -1                     # argument checks come first
    assert call(n, n, nbytes.value - 1) == -5
    assert call(32769, 32769, nbytes.value) == _hip.E_UNSUPPORTED
    assert lib.spk_ahc_workspace_bytes(32769, ctypes.byref(nbytes)) == _hip.E_UNSUPPORTED
    assert labels.eq(-7).all() and count.eq(-7).all() and ws.eq(0).all()


def test_abi_host_code_under_sanitizers(tmp_path):
    """ahc_abi.cpp's argument checks and workspace arithmetic in a stand-alone program built with
    -fsanitize=address,undefined (tests/sanitize/ahc_abi_main.cpp; no launchers linked)."""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / 'ahc_abi_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-static-libasan', '-static-libubsan', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include', '-w', '-o', exe,
                    os.path.join(here, 'sanitize', 'ahc_abi_main.cpp'),
                    os.path.join(here, '..', '3d-speaker_amd', 'csrc', 'ahc_abi.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'ahc_abi host checks ok' in r.stdout
