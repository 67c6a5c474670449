"""Corpus similarity statistics, the parts that need no device: the argument checks of the four C
entries through ctypes -- on the built library (error paths only: nothing is launched) and on the
host-only build (tests/emu), which has no kernels and answers SPK_E_UNSUPPORTED once the arguments
pass --, the workspace arithmetic, the numpy statement of the analysis against brute-force double
loops on the tie input, and the ABI's host code under the sanitizers in a stand-alone program."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import emu_runner
import sim_inputs
from speakerlab import _hip
from speakerlab.utils import similarity_analysis as sa

E_INVALID, E_WORKSPACE = -1, -5


def _sizes(lib, n):
    lo, rec, st = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.spk_cosine_sim_workspace_bytes(n, ctypes.byref(lo), ctypes.byref(rec), ctypes.byref(st)) == 0
    return lo.value, rec.value, st.value


def _abi_cases(lib, kernels_missing):
    lo, rec, st = ctypes.c_size_t(77), ctypes.c_size_t(78), ctypes.c_size_t(79)
    q = lib.spk_cosine_sim_workspace_bytes
    refs = [ctypes.byref(v) for v in (lo, rec, st)]
    assert q(0, *refs) == E_INVALID and q(-3, *refs) == E_INVALID
    for hole in range(3):
        assert q(5, *[None if h == hole else r for h, r in enumerate(refs)]) == E_INVALID
    assert q(2 ** 31, *refs) == _hip.E_UNSUPPORTED
    assert q(2 ** 31 - 1, *refs) == _hip.E_UNSUPPORTED             # one tile of rows is 2^32 work-items of affinity
    assert (lo.value, rec.value, st.value) == (77, 78, 79)
    # the workspace arithmetic: one tile of rows; blocks of about 128 MiB, whole tiles, at most N rows
    assert _sizes(lib, 1)[:2] == (512, 512)
    assert _sizes(lib, 300)[:2] == (128 * 300 * 4, 384 * 300 * 4)
    lo_, rec_, st_ = _sizes(lib, 100000)
    assert lo_ == 128 * 100000 * 4 and rec_ == 256 * 100000 * 4 and rec_ <= 128 << 20 < rec_ + lo_
    assert st_ >= 2 * 8 * 100000 + 2 * 4 * 100000 + 4 * 4096 * 12
    assert _sizes(lib, 20000)[1] == 1664 * 20000 * 4

    n, e, k, next_ = 9, 8, 3, 4
    lo_, rec_, st_ = _sizes(lib, n)
    X = torch.ones(n + 1, e)
    ws = torch.zeros(rec_, dtype=torch.uint8)
    state = torch.zeros(st_, dtype=torch.uint8)
    top_s, top_i = torch.full((n, k), -7.0), torch.full((n, k), -7, dtype=torch.int64)
    d1, d2 = torch.full((n,), -7.0, dtype=torch.float64), torch.full((n,), -7.0, dtype=torch.float64)
    f1, f2, f3 = (torch.full((n,), -7.0) for _ in range(3))
    p = lambda t: t.data_ptr()

    def rows(x=p(X), N=n, E=e, k_=k, a=p(top_s), b=p(top_i), c=p(d1), d=p(d2), f=p(f1), g=p(f2), h=p(f3), w=p(ws),
             wb=rec_):
        return lib.spk_cosine_rows_topk(x, N, E, k_, a, b, c, d, f, g, h, w, wb, None)

    for kw in (dict(x=None), dict(a=None), dict(b=None), dict(c=None), dict(d=None), dict(f=None), dict(g=None),
               dict(h=None), dict(w=None), dict(N=0), dict(N=-1), dict(E=0), dict(E=6), dict(E=-4), dict(k_=0),
               dict(k_=1025), dict(x=p(X) + 4)):
        assert rows(**kw) == E_INVALID, kw
        assert b'spk_cosine_rows_topk' in lib.spk_last_error()
    for kw in (dict(wb=lo_ - 1), dict(wb=0)):
        assert rows(**kw) == E_WORKSPACE, kw
    assert rows(N=2 ** 31, wb=2 ** 62) == _hip.E_UNSUPPORTED

    thr = np.array([0.5, 0.1], np.float32)
    ranks = np.array([0, 35], np.int64)                            # P = 36
    count, sums, mm = np.full(1, -7, np.int64), np.full(2, -7.0), np.full(2, -7, np.float32)
    cge, order = np.full(2, -7, np.int64), np.full(2, -7, np.float32)
    cut, take = np.full(2, -7, np.float32), np.full(2, -7, np.int32)
    a = lambda v: v.ctypes.data

    def stats(x=p(X), N=n, E=e, t=a(thr), nt=2, r=a(ranks), nr=2, ne=next_, c=a(count), s1=a(sums), s2=a(sums) + 8,
              mn=a(mm), mx=a(mm) + 4, cg=a(cge), o=a(order), ec=a(cut), et=a(take), w=p(ws), wb=rec_, s=p(state),
              sb=st_):
        return lib.spk_cosine_triu_stats(x, N, E, t, nt, r, nr, ne, c, s1, s2, mn, mx, cg, o, ec, et, w, wb, s, sb, None)

    for kw in (dict(x=None), dict(t=None), dict(r=None), dict(c=None), dict(s1=None), dict(s2=None), dict(mn=None),
               dict(mx=None), dict(cg=None), dict(o=None), dict(ec=None), dict(et=None), dict(w=None), dict(s=None),
               dict(N=0), dict(E=0), dict(E=10), dict(nt=-1), dict(nt=33), dict(nr=-1), dict(nr=17), dict(ne=-1),
               dict(ne=4097), dict(x=p(X) + 8), dict(r=a(np.array([5, 4], np.int64))),
               dict(r=a(np.array([0, 36], np.int64))), dict(r=a(np.array([-1, 3], np.int64))),
               dict(t=a(np.array([0.5, np.nan], np.float32))), dict(N=1, wb=2 ** 40, nr=1)):
        assert stats(**kw) == E_INVALID, kw
        assert b'spk_cosine_triu_stats' in lib.spk_last_error()
    for kw in (dict(wb=lo_ - 1), dict(sb=st_ - 1), dict(sb=0)):
        assert stats(**kw) == E_WORKSPACE, kw
    assert stats(N=2 ** 31, wb=2 ** 62, nr=0) == _hip.E_UNSUPPORTED

    edges = np.linspace(-1.0, 1.0, 6)
    hist, found = np.full(5, -7, np.int64), np.full(2, -7, np.int32)
    es, ei, ej = np.full((2, next_), -7, np.float32), np.full((2, next_), -7, np.int64), np.full((2, next_), -7, np.int64)
    gcut, gtake = np.array([0.5, -0.5], np.float32), np.array([1, 1], np.int32)

    def hist_(x=p(X), N=n, E=e, ed=a(edges), nb=5, ne=next_, ec=a(gcut), et=a(gtake), h=a(hist), s_=a(es), i_=a(ei),
              j_=a(ej), f=a(found), w=p(ws), wb=rec_, s=p(state), sb=st_):
        return lib.spk_cosine_triu_hist(x, N, E, ed, nb, ne, ec, et, h, s_, i_, j_, f, w, wb, s, sb, None)

    down = np.array([-1.0, 0.0, -0.5, 0.5, 0.7, 1.0])
    for kw in (dict(x=None), dict(ed=None), dict(ec=None), dict(et=None), dict(h=None), dict(s_=None), dict(i_=None),
               dict(j_=None), dict(f=None), dict(w=None), dict(s=None), dict(N=0), dict(E=2), dict(nb=-1), dict(nb=257),
               dict(ne=-1), dict(ne=4097), dict(ed=a(down)), dict(ed=a(np.array([0, 1, 2, 3, 4, np.inf]))),
               dict(et=a(np.array([0, 1], np.int32))), dict(et=a(np.array([1, 5], np.int32))),
               dict(ec=a(np.array([np.nan, 0], np.float32)))):
        assert hist_(**kw) == E_INVALID, kw
        assert b'spk_cosine_triu_hist' in lib.spk_last_error()
    for kw in (dict(wb=lo_ - 1), dict(sb=st_ - 1)):
        assert hist_(**kw) == E_WORKSPACE, kw

    if kernels_missing:                                            # valid arguments: only the kernels are missing
        for call in (rows, stats, hist_):
            assert call() == _hip.E_UNSUPPORTED
            assert b'no kernels' in lib.spk_last_error()
        # N == 1 has no pair: answered on the host
        assert stats(N=1, nr=0) == 0
        assert count[0] == 0 and np.isnan(sums).all() and np.isnan(mm).all() and (cge == 0).all()
        assert np.isnan(cut).all() and (take == 0).all()
        assert hist_(N=1) == 0 and (hist == 0).all() and (found == 0).all()
    else:
        assert count[0] == -7 and (sums == -7).all() and (mm == -7).all() and (cge == -7).all()
        assert (cut == -7).all() and (take == -7).all() and (hist == -7).all() and (found == -7).all()
    assert (order == -7).all() and (es == -7).all() and (ei == -7).all() and (ej == -7).all()
    for t in (top_s, top_i, d1, d2, f1, f2, f3):
        assert t.eq(-7).all()
    assert ws.eq(0).all() and state.eq(0).all()


def _emu_cases():
    lib = emu_runner.lib()
    assert lib.spk_version() == 2                                  # the entries are additive
    _abi_cases(lib, kernels_missing=True)


def test_emu_library_has_the_entries_and_no_kernels():
    """In a process that already holds the real library the weak launchers resolve to its kernels,
    so that case runs in a fresh interpreter (tests/test_score_norm_host.py)."""
    if emu_runner._lib is None and _hip._lib is not None:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
        r = subprocess.run([sys.executable, '-c', 'import test_sim_stats_host as t; t._emu_cases()'], env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        _emu_cases()


def test_abi_argument_checks_on_the_built_library():
    _abi_cases(_hip.lib(), kernels_missing=False)


def test_device_wrappers_need_a_device():
    x = torch.zeros(5, 8)
    with pytest.raises(_hip.HipError):
        _hip.cosine_rows_topk(x, 3)
    with pytest.raises(_hip.HipError):
        _hip.cosine_triu_stats(x, ranks=[0])
    assert _hip.cosine_sim_workspace_bytes(300)[:2] == (128 * 300 * 4, 384 * 300 * 4)


def test_quantile_ranks_follow_numpy():
    rng = np.random.default_rng(3)
    for P in (1, 2, 3, 4, 7, 36, 44850):
        v = np.sort(rng.standard_normal(P))
        pos, asked = sa.quantile_ranks(P)
        assert asked == sorted(set(asked)) and 0 <= asked[0] and asked[-1] < P
        got = [sa._interp(v[lo], v[hi], t) for lo, hi, t in pos]
        np.testing.assert_allclose(got, np.percentile(v, [25, 50, 75]), rtol=0, atol=1e-15)


def test_numpy_path_on_the_tie_input_against_brute_force():
    X = sim_inputs.tie_input(n=120, e=32, copies=(11, 80, 119))
    S = sa.host_cosine(X)
    assert (S[42] == 0).all() and S[10, 11] == S[10, 80] == S[11, 119]
    k, n_ext = 7, 50
    raw = sa.raw_from_scores(S, k, n_ext, 50)
    top_s, top_i = sim_inputs.brute_rows(S, k)
    assert np.array_equal(raw['rows']['top_index'], top_i) and np.array_equal(raw['rows']['top_scores'], top_s)
    N = 120
    P = N * (N - 1) // 2
    vals = np.array([S[i, j] for i in range(N) for j in range(i + 1, N)], np.float32)
    tri = raw['triu']
    assert tri['count'] == P and tri['min'] == vals.min() and tri['max'] == vals.max()
    assert abs(tri['sum'] - sum(float(v) for v in vals)) < 1e-9
    for name, largest in (('most', True), ('least', False)):
        bs, bi, bj = sim_inputs.brute_pairs(S, n_ext, largest)
        assert np.array_equal(tri[name][0], bs) and np.array_equal(tri[name][1], bi) and np.array_equal(tri[name][2], bj)
    # the six copies' pairs score the same: the most similar pairs start with them in (i, j) order
    assert list(zip(tri['most'][1][:3], tri['most'][2][:3])) == [(10, 11), (10, 80), (10, 119)]
    assert tri['hist'].sum() == P and tri['hist'][-1] >= 1        # the maximum is in the closed last bin
    assert np.array_equal(tri['count_ge'], [(vals >= np.float32(t)).sum() for t in sa.THRESHOLDS])
    srt = np.sort(vals)
    assert np.array_equal(tri['order_stats'], srt[sa.quantile_ranks(P)[1]])
    rep = sa.analyze(X, [f's{i}' for i in range(N)], top_k=k, n_extreme=n_ext)
    up = rep['upper_triangular_statistics']
    np.testing.assert_allclose([up['q25_similarity'], up['median_similarity'], up['q75_similarity']],
                               np.percentile(vals.astype(np.float64), [25, 50, 75]), rtol=0, atol=1e-15)
    full = rep['similarity_statistics']
    assert abs(full['mean_similarity'] - S.astype(np.float64).mean()) < 1e-12
    assert abs(full['std_similarity'] - S.astype(np.float64).std()) < 1e-12
    assert full['min_similarity'] == float(S.min()) and full['max_similarity'] == float(S.max())


def test_abi_host_code_under_sanitizers(tmp_path):
    """sim_stats_abi.cpp's argument checks, block arithmetic and state layout in a stand-alone program
    built with -fsanitize=address,undefined (tests/sanitize/sim_stats_abi_main.cpp; no launchers linked)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / 'sim_stats_abi_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-static-libasan', '-static-libubsan', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include', '-w', '-o', exe,
                    os.path.join(here, 'sanitize', 'sim_stats_abi_main.cpp'),
                    os.path.join(here, '..', '3d-speaker_amd', 'csrc', 'sim_stats_abi.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'sim_stats_abi host checks ok' in r.stdout
