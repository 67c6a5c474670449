"""Cohort score normalisation (S-norm / AS-norm), the parts that need no device: the float64 numpy
restatement (speakerlab/utils/score_norm.py) against brute force, the CLI's argument errors, and
the argument checks of the four C entries through ctypes -- on the built library (error paths only:
nothing is launched) and on the host-only build (tests/emu), which has no kernels and answers
SPK_E_UNSUPPORTED once the arguments pass."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import emu_runner
from speakerlab import _hip
from speakerlab.bin import compute_score_metrics as csm
from speakerlab.utils import score_norm

E_INVALID, E_WORKSPACE = -1, -5


def _data(n=13, nc=37, e=24, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, e)).astype(np.float32)
    c = rng.standard_normal((nc, e)).astype(np.float32)
    x[3] = 0                                                       # zero-norm rows: cosine 0 (sklearn)
    c[5] = 0
    return x, c


def _brute_stats(x, c, k):
    mu, sd = [], []
    for a in x.astype(np.float64):
        na = np.linalg.norm(a) or 1.0
        row = [float(a @ b) / (na * (np.linalg.norm(b) or 1.0)) for b in c.astype(np.float64)]
        top = sorted(row)[-k:]
        m = sum(top) / k
        mu.append(m)
        sd.append((sum((v - m) ** 2 for v in top) / k) ** 0.5)
    return np.array(mu), np.array(sd)


@pytest.mark.parametrize('k', [1, 2, 10, 36, 37])
def test_cohort_stats_host_against_brute_force(k):
    x, c = _data()
    mu, sd = score_norm.cohort_stats_host(x, c, k)
    rmu, rsd = _brute_stats(x, c, k)
    assert mu.dtype == np.float64 and mu.shape == (13,) and sd.shape == (13,)
    np.testing.assert_allclose(mu, rmu, rtol=0, atol=1e-14)
    np.testing.assert_allclose(sd, rsd, rtol=0, atol=1e-14)
    assert mu[3] == 0 and sd[3] == 0                               # the zero row scores 0 against everything
    if k == 1:
        assert (sd == 0).all()


def test_topk_stats_host_ties_across_the_cut():
    S = np.array([[0.5, 0.25, 0.25, 0.25, 0.25, -1.0], [3.0, 3.0, 3.0, 3.0, 3.0, 3.0]])
    mu, sd = score_norm.topk_stats_host(S, 3)
    np.testing.assert_allclose(mu, [1.0 / 3, 3.0], atol=1e-15)
    np.testing.assert_allclose(sd, [np.std([0.5, 0.25, 0.25]), 0.0], atol=1e-15)


def test_as_norm_host_is_the_formula():
    rng = np.random.default_rng(1)
    raw, mu_e, mu_t = rng.uniform(-1, 1, (3, 50))
    sd_e, sd_t = rng.uniform(0.01, 0.3, (2, 50))
    sd_e[7] = 0.0                                                  # the floor
    sd_t[9] = 1e-9
    got = score_norm.as_norm_host(raw, mu_e, sd_e, mu_t, sd_t)
    floor = float(np.float32(1e-6))
    for t in range(50):
        want = 0.5 * ((raw[t] - mu_e[t]) / max(sd_e[t], floor) + (raw[t] - mu_t[t]) / max(sd_t[t], floor))
        assert got[t] == pytest.approx(want, rel=1e-15, abs=0)
    assert np.isfinite(got).all()
    assert np.array_equal(score_norm.as_norm_host(raw, np.zeros(50), np.ones(50), np.zeros(50), np.ones(50)), raw)


def test_snorm_is_asnorm_over_the_whole_cohort_and_top_n_is_clipped():
    x, c = _data()
    whole = score_norm.cohort_stats_host(x, c, None)
    for top_n in (37, 38, 10 ** 6):
        got = score_norm.cohort_stats_host(x, c, top_n)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    S = score_norm._host_cosine(x, c)
    np.testing.assert_allclose(whole[0], S.mean(1), atol=1e-15)
    np.testing.assert_allclose(whole[1], S.std(1), atol=1e-15)
    part = score_norm.cohort_stats_host(x, c, 36)
    assert not np.array_equal(part[0], whole[0])
    for bad in (0, -3):
        with pytest.raises(ValueError):
            score_norm.cohort_stats_host(x, c, bad)
    with pytest.raises(ValueError):
        score_norm.cohort_stats_host(x, np.zeros((0, 24)), None)


def test_cli_argument_errors(capsys):
    base = ['--enrol_data', 'e', '--test_data', 't', '--scores_dir', 's', '--trials', 'x']
    args = csm.parse_args(base)
    assert args.score_norm == 'none' and args.cohort_data == '' and args.top_n == 300
    args = csm.parse_args(base + ['--score_norm', 'asnorm', '--cohort_data', 'c', '--top_n', '20'])
    assert (args.score_norm, args.cohort_data, args.top_n) == ('asnorm', 'c', 20)
    assert csm.parse_args(base + ['--score_norm', 'snorm', '--cohort_data', 'c']).score_norm == 'snorm'
    for extra in (['--score_norm', 'asnorm'], ['--score_norm', 'snorm'], ['--score_norm', 'znorm', '--cohort_data', 'c'],
                  ['--score_norm', 'asnorm', '--cohort_data', 'c', '--top_n', '0']):
        with pytest.raises(SystemExit) as ei:
            csm.parse_args(base + extra)
        assert ei.value.code == 2
    with pytest.raises(SystemExit):                                # main() checks before it touches anything
        csm.main(base + ['--score_norm', 'asnorm'])
    capsys.readouterr()


def _abi_cases(lib, kernels_missing):
    """Every SPK_E_INVALID / SPK_E_WORKSPACE case of include/spk_hip.h; outputs keep their sentinel."""
    n, nc, e = 9, 11, 8
    lo, rec = ctypes.c_size_t(77), ctypes.c_size_t(78)
    q = lib.spk_cosine_cohort_stats_workspace_bytes
    assert q(0, nc, ctypes.byref(lo), ctypes.byref(rec)) == E_INVALID
    assert q(n, 0, ctypes.byref(lo), ctypes.byref(rec)) == E_INVALID
    assert q(n, nc, None, ctypes.byref(rec)) == E_INVALID
    assert q(n, nc, ctypes.byref(lo), None) == E_INVALID
    assert q(2 ** 31, nc, ctypes.byref(lo), ctypes.byref(rec)) == _hip.E_UNSUPPORTED
    assert (lo.value, rec.value) == (77, 78)
    assert q(n, nc, ctypes.byref(lo), ctypes.byref(rec)) == 0
    assert lo.value == 128 * nc * 4 and rec.value == lo.value      # 9 rows: one block
    assert q(20000, 20000, ctypes.byref(lo), ctypes.byref(rec)) == 0
    assert lo.value == 128 * 20000 * 4 and lo.value < rec.value <= 128 << 20 and rec.value % lo.value == 0
    assert q(n, nc, ctypes.byref(lo), ctypes.byref(rec)) == 0

    S = torch.full((n, nc), 0.5)
    X, C = torch.ones(n, e), torch.ones(nc, e)
    mean, std, out = (torch.full((n,), -7.0) for _ in range(3))
    ws = torch.zeros(rec.value, dtype=torch.uint8)
    ia = torch.zeros(n, dtype=torch.int64)
    p = lambda t: t.data_ptr()

    def stats(S_=p(S), rows=n, cols=nc, lds=nc, k=3, m=p(mean), s=p(std)):
        return lib.spk_topk_stats(S_, rows, cols, lds, k, m, s, None)

    for kw in (dict(S_=None), dict(m=None), dict(s=None), dict(rows=0), dict(rows=-1), dict(cols=0, k=1),
               dict(lds=nc - 1), dict(k=0), dict(k=-1), dict(k=nc + 1)):
        assert stats(**kw) == E_INVALID, kw
        assert b'spk_topk_stats' in lib.spk_last_error()

    def cohort(x=p(X), N=n, c=p(C), Nc=nc, E=e, k=3, m=p(mean), s=p(std), w=p(ws), wb=rec.value):
        return lib.spk_cosine_cohort_stats(x, N, c, Nc, E, k, m, s, w, wb, None)

    for kw in (dict(x=None), dict(c=None), dict(m=None), dict(s=None), dict(w=None), dict(N=0), dict(Nc=0, k=1),
               dict(k=0), dict(k=nc + 1), dict(E=0), dict(E=-4), dict(E=6)):
        assert cohort(**kw) == E_INVALID, kw
    for kw in (dict(wb=lo.value - 1), dict(wb=0)):
        assert cohort(**kw) == E_WORKSPACE, kw
        assert b'workspace' in lib.spk_last_error()

    def trials(a=p(X), b=p(X), E=e, i=p(ia), j=p(ia), T=n, ma=p(S), sa=p(S), mb=p(S), sb=p(S), o=p(out)):
        return lib.spk_cosine_trials_norm(a, b, E, i, j, T, ma, sa, mb, sb, o, None)

    for kw in (dict(a=None), dict(b=None), dict(i=None), dict(j=None), dict(ma=None), dict(sa=None), dict(mb=None),
               dict(sb=None), dict(o=None), dict(T=0), dict(T=-2), dict(E=0), dict(E=7)):
        assert trials(**kw) == E_INVALID, kw

    if kernels_missing:                                            # valid arguments: only the kernels are missing
        for call in (stats, cohort, trials):
            assert call() == _hip.E_UNSUPPORTED
            assert b'no kernels' in lib.spk_last_error()
        assert cohort(wb=lo.value) == _hip.E_UNSUPPORTED
    assert mean.eq(-7).all() and std.eq(-7).all() and out.eq(-7).all() and ws.eq(0).all()


def _emu_cases():
    lib = emu_runner.lib()                                         # binds every symbol of _hip.SYMBOLS
    assert lib.spk_version() == 2                                  # the entries are additive
    _abi_cases(lib, kernels_missing=True)


def test_emu_library_has_the_entries_and_no_kernels():
    """The host-only build's launchers are unresolved weak symbols.  They stay unresolved only if
    that build is loaded before libspk_hip.so (which _hip loads with RTLD_GLOBAL and which defines
    them): in a process that already holds the real library alone, the calls with valid arguments
    would reach its kernels with host pointers, so that case runs in a fresh interpreter."""
    if emu_runner._lib is None and _hip._lib is not None:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
        r = subprocess.run([sys.executable, '-c', 'import test_score_norm_host as t; t._emu_cases()'], env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        _emu_cases()


def test_abi_argument_checks_on_the_built_library():
    _abi_cases(_hip.lib(), kernels_missing=False)


def test_device_wrappers_need_a_device():
    x, c = _data()
    with pytest.raises(_hip.HipError):
        _hip.topk_stats(torch.from_numpy(x), 3)
    with pytest.raises(_hip.HipError):
        _hip.cosine_cohort_stats(torch.from_numpy(x), torch.from_numpy(c), 3)
    with pytest.raises(_hip.HipError):
        _hip.cosine_trials_norm(torch.from_numpy(x), torch.from_numpy(x), torch.zeros(2, dtype=torch.int64),
                                torch.zeros(2, dtype=torch.int64), (torch.zeros(13), torch.ones(13)),
                                (torch.zeros(13), torch.ones(13)))


def test_abi_host_code_under_sanitizers(tmp_path):
    """score_norm_abi.cpp's argument checks and row-block arithmetic in a stand-alone program built
    with -fsanitize=address,undefined (tests/sanitize/score_norm_abi_main.cpp; no launchers linked)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / 'score_norm_abi_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-static-libasan', '-static-libubsan', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include', '-w', '-o', exe,
                    os.path.join(here, 'sanitize', 'score_norm_abi_main.cpp'),
                    os.path.join(here, '..', '3d-speaker_amd', 'csrc', 'score_norm_abi.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'score_norm_abi host checks ok' in r.stdout
