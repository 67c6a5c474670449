"""Cohort score normalisation on the device (csrc/score_norm.hip) against float64 numpy: the top-K
statistics kernel on matrices built directly, the row-blocked cohort statistics against
``cohort_stats_host``, the normalising trial gather, and compute_score_metrics' flags.

Bounds of the statistics (derived, not measured), for a row with M = max |s| and K kept entries:
the kernel's fp64 sums carry at most (K - 1) u relative error each (u = 2^-53), so the mean is off by
far less than its final rounding to fp32, 2^-24 |mean| <= 2^-24 M, and sum2 / K - mean^2 is off by at
most delta = 3 K u M^2.  sqrt turns an error delta of the variance into at most
min(sqrt(delta), delta / (2 std)), and the result is rounded to fp32 once more:
    |mean - ref| <= 2^-23 M          |std - ref| <= 2^-23 M + min(sqrt(delta), delta / (2 std_ref)).
"""
import functools
import logging

import numpy as np
import pytest
import torch

from speakerlab import _hip
from speakerlab.bin import compute_score_metrics as csm
from speakerlab.utils import kaldi_io, score_norm

pytestmark = pytest.mark.gpu

U24, U53 = 2.0 ** -24, 2.0 ** -53
AFFINITY_ATOL = 2e-6                       # the cosine affinity's own bound (tests/test_gpu_affinity.py)
GUARD, SENTINEL = 8, -12345.0

SHAPES = [(1, 1, 1), (3, 5, 1), (3, 5, 5), (2, 63, 7), (5, 257, 256), (5, 257, 257), (130, 1000, 300),
          (2, 5003, 1), (2, 5003, 300), (2, 5003, 5002)]
KINDS = ['uniform', 'equal', 'signed_zeros', 'ties', 'negative', 'outlier']


def _matrix(kind, rows, cols, K, rng):
    if kind == 'uniform':
        return rng.uniform(-1, 1, (rows, cols)).astype(np.float32)
    if kind == 'equal':
        return np.full((rows, cols), 0.25, np.float32)
    if kind == 'negative':
        return rng.uniform(-1, -0.01, (rows, cols)).astype(np.float32)
    S = np.empty((rows, cols), np.float32)
    for r in range(rows):
        if kind == 'signed_zeros':                       # half +0.0, half -0.0, a few negatives
            row = np.zeros(cols, np.float32)
            row[::2] = -0.0
            neg = rng.choice(cols, min(3, cols // 2), replace=False)
            row[neg] = rng.uniform(-1, -0.1, len(neg))
        elif kind == 'ties':                             # 2K equal values, the K-th largest inside the block
            b = min(2 * K, cols)
            g = min(K // 2, cols - b)                    # entries above the block: g < K <= g + b
            row = np.concatenate([rng.uniform(0.5, 1, g), np.full(b, 0.3), rng.uniform(-1, 0.2, cols - b - g)])
            row = rng.permutation(row).astype(np.float32)
        else:                                            # one huge outlier among small values
            row = rng.uniform(-1e-3, 1e-3, cols).astype(np.float32)
            row[rng.integers(cols)] = 1e30
        S[r] = row
    return S


def _reference(S, K):
    top = np.sort(S.astype(np.float64), axis=1)[:, S.shape[1] - K:]
    return top.mean(axis=1), top.std(axis=1)


def _bounds(M, K, std_ref):
    delta = 3.0 * K * U53 * M * M
    with np.errstate(divide='ignore', invalid='ignore'):
        slope = np.where(std_ref > 0, delta / (2 * std_ref), np.inf)
    return 2 * U24 * M, 2 * U24 * M + np.minimum(np.sqrt(delta), slope)


def _worst(err, bound):
    """Largest err / bound (0 / 0 counts as 0)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.max(np.where(err > 0, err / bound, 0.0)))


def _run_topk(S, K, pad):
    """One launch on a [rows, cols + pad] buffer whose padding holds +inf; guarded outputs."""
    rows, cols = S.shape
    buf = torch.full((rows, cols + pad), float('inf'), dtype=torch.float32)
    buf[:, :cols] = torch.from_numpy(S)
    buf = buf.cuda()
    outs = [torch.full((rows + 2 * GUARD,), SENTINEL, dtype=torch.float32, device='cuda') for _ in range(2)]
    _hip._check(_hip.lib().spk_topk_stats(buf.data_ptr(), rows, cols, cols + pad, K, outs[0][GUARD:].data_ptr(),
                                          outs[1][GUARD:].data_ptr(), _hip._stream(buf.device)), 'spk_topk_stats')
    outs = [o.cpu().numpy() for o in outs]
    for o in outs:
        assert (o[:GUARD] == SENTINEL).all() and (o[GUARD + rows:] == SENTINEL).all(), 'guard overwritten'
    return outs[0][GUARD:GUARD + rows], outs[1][GUARD:GUARD + rows]


@pytest.mark.parametrize('rows,cols,K', SHAPES)
def test_topk_stats(rows, cols, K):
    rng = np.random.default_rng(rows * 100003 + cols * 101 + K)
    for kind in KINDS:
        S = _matrix(kind, rows, cols, K, rng)
        rmean, rstd = _reference(S, K)
        M = np.abs(S.astype(np.float64)).max(axis=1)
        bmean, bstd = _bounds(M, K, rstd)
        for pad in (0, 3):
            mean, std = _run_topk(S, K, pad)
            emean, estd = np.abs(mean - rmean), np.abs(std - rstd)
            print(f'topk_stats {kind} ({rows},{cols},{K}) pad {pad}: mean err/bound {_worst(emean, bmean):.3g}, '
                  f'std err/bound {_worst(estd, bstd):.3g}')
            assert np.isfinite(mean).all() and np.isfinite(std).all(), (kind, pad)
            assert (emean <= bmean).all(), (kind, pad, emean.max())
            # the outlier row keeps its std bound: the two-pass fp64 reference resolves (s - mean)^2 of
            # every entry to 2^-52 relative, far inside delta, so nothing is lost there
            assert (estd <= bstd).all(), (kind, pad, estd.max())
            if kind == 'equal':
                assert (mean == 0.25).all() and (std == 0).all()
            if K == 1:
                assert (std == 0).all()
            again = _run_topk(S, K, pad)
            assert mean.tobytes() == again[0].tobytes() and std.tobytes() == again[1].tobytes()


COHORT_CASES = [(1, 1, 192, 1), (7, 50, 192, 10), (129, 300, 192, 300), (300, 1100, 256, 64)]


@pytest.mark.parametrize('N,Nc,E,K', COHORT_CASES)
def test_cosine_cohort_stats(N, Nc, E, K):
    rng = np.random.default_rng(N * 7919 + Nc)
    x = rng.standard_normal((N, E)).astype(np.float32)
    c = rng.standard_normal((Nc, E)).astype(np.float32)
    if N >= 3 and Nc >= 5:                               # zero-norm rows: sklearn semantics, cosine 0
        x[2] = 0
        c[4] = 0
    rmean, rstd = score_norm.cohort_stats_host(x, c, K)
    M = np.abs(score_norm._host_cosine(x, c)).max(axis=1)
    bmean, bstd = _bounds(M, K, rstd)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    lo, rec = _hip.cosine_cohort_stats_workspace_bytes(N, Nc)
    assert lo == 128 * Nc * 4 and rec >= lo
    got = {}
    for nbytes in (lo, rec):
        mean, std = _hip.cosine_cohort_stats(xd, cd, K, workspace_bytes=nbytes)
        got[nbytes] = (mean.cpu().numpy(), std.cpu().numpy())
    mean, std = got[rec]
    assert got[lo][0].tobytes() == mean.tobytes() and got[lo][1].tobytes() == std.tobytes()
    emean, estd = np.abs(mean - rmean), np.abs(std - rstd)
    print(f'cohort_stats ({N},{Nc},{E},{K}): mean err {emean.max():.3g} (bound {AFFINITY_ATOL + bmean.min():.3g}), '
          f'std err {estd.max():.3g} (bound {AFFINITY_ATOL + bstd.min():.3g})')
    # order statistics and the standard deviation are 1-Lipschitz in the sup norm of the scores
    assert (emean <= AFFINITY_ATOL + bmean).all(), emean.max()
    assert (estd <= AFFINITY_ATOL + bstd).all(), estd.max()
    if N >= 3 and Nc >= 5:
        assert mean[2] == 0 and std[2] == 0              # the zero row scores 0 against every cohort row
    with pytest.raises(_hip.HipError) as ei:
        _hip.cosine_cohort_stats(xd, cd, K, workspace_bytes=lo - 1)
    assert ei.value.code == -5
    # the wrapper over both: top_n clipped to the cohort, None the whole cohort
    wmean, wstd = score_norm.cohort_stats(x, c, K)
    assert wmean.tobytes() == mean.tobytes() and wstd.tobytes() == std.tobytes()
    if K == Nc:
        for top_n in (None, Nc + 5):
            smean, sstd = score_norm.cohort_stats(x, c, top_n)
            assert smean.tobytes() == mean.tobytes() and sstd.tobytes() == std.tobytes()
    _hip.cohort_release_workspace()


@functools.lru_cache(maxsize=None)
def _trial_setup():
    rng = np.random.default_rng(11)
    E = 192
    enrol = rng.standard_normal((40, E)).astype(np.float32)
    test = rng.standard_normal((60, E)).astype(np.float32)
    cohort = rng.standard_normal((500, E)).astype(np.float32)
    ia, ib = rng.integers(0, 40, 1000), rng.integers(0, 60, 1000)
    a, b, c = (torch.from_numpy(v).cuda() for v in (enrol, test, cohort))
    ta, tb = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
    raw = _hip.cosine_trials(a, b, ta, tb)
    sa = _hip.cosine_cohort_stats(a, c, 50)
    sb = _hip.cosine_cohort_stats(b, c, 50)
    return a, b, ta, tb, ia, ib, raw, sa, sb


def _check_trials(got, raw, ia, ib, sa, sb):
    raw64 = raw.cpu().numpy().astype(np.float64)
    (mu_a, sd_a), (mu_b, sd_b) = ([t.cpu().numpy().astype(np.float64) for t in s] for s in (sa, sb))
    floor = float(np.float32(1e-6))
    za = (raw64 - mu_a[ia]) / np.maximum(sd_a[ia], floor)
    zb = (raw64 - mu_b[ib]) / np.maximum(sd_b[ib], floor)
    ref = 0.5 * (za + zb)
    np.testing.assert_array_equal(ref, score_norm.as_norm_host(raw64, mu_a[ia], sd_a[ia], mu_b[ib], sd_b[ib]))
    got = got.cpu().numpy()
    err, bound = np.abs(got - ref), 6 * U24 * (np.abs(za) + np.abs(zb))
    print(f'trials_norm: max err / bound {_worst(err, bound):.3g}')
    assert np.isfinite(got).all()
    assert (err <= bound).all(), _worst(err, bound)


def test_cosine_trials_norm():
    a, b, ta, tb, ia, ib, raw, sa, sb = _trial_setup()
    assert float(sa[1].min()) > 0 and float(sb[1].min()) > 0
    _check_trials(_hip.cosine_trials_norm(a, b, ta, tb, sa, sb), raw, ia, ib, sa, sb)


def test_cosine_trials_norm_std_floor():
    a, b, ta, tb, ia, ib, raw, sa, sb = _trial_setup()
    sd_a = sa[1].clone()
    sd_a[int(ia[0])] = 0.0                                # a degenerate cohort: the 1e-6 floor
    got = _hip.cosine_trials_norm(a, b, ta, tb, (sa[0], sd_a), sb)
    _check_trials(got, raw, ia, ib, (sa[0], sd_a), sb)
    hit = got.cpu().numpy()[ia == ia[0]]
    assert np.isfinite(hit).all() and np.abs(hit).max() > 1e3


def test_cosine_trials_norm_identity_statistics_return_the_raw_cosine():
    a, b, ta, tb, ia, ib, raw, sa, sb = _trial_setup()
    ident_a = (torch.zeros(40, device='cuda'), torch.ones(40, device='cuda'))
    ident_b = (torch.zeros(60, device='cuda'), torch.ones(60, device='cuda'))
    got = _hip.cosine_trials_norm(a, b, ta, tb, ident_a, ident_b)
    assert torch.equal(got, raw)                          # the shared cosine function, bit for bit
    assert torch.equal(raw, _hip.cosine_trials(a, b, ta, tb))


def _write(d, prefix, embs):
    d.mkdir()
    with kaldi_io.WriteHelper(f'ark,scp:{d}/e.ark,{d}/e.scp') as w:
        for i, e in enumerate(embs):
            w(f'{prefix}{i}', e)


def _scores(path):
    return np.array([float(line.split()[-1]) for line in path.read_text().splitlines()])


@pytest.fixture
def metrics_logger():
    """compute_score_metrics logs through one process-wide logger that keeps the handlers of its first
    call, result.metrics of that run included.  Put it back as it was found, so that the runs of
    this file do not take the file handler of whichever test calls main() next."""
    logger = logging.getLogger('speakerlab.utils.utils')
    before = list(logger.handlers)
    yield
    for h in list(logger.handlers):
        if h not in before:
            logger.removeHandler(h)
            h.close()


def test_score_metrics_cli_score_norm(tmp_path, metrics_logger):
    rng = np.random.default_rng(5)
    E, ne, nt, nc, top_n = 16, 20, 30, 200, 20            # a low dimension spreads the cohort's cosines
    spk = rng.standard_normal((ne, E))
    enrol = np.float32(spk + 0.5 * rng.standard_normal((ne, E)))
    test = np.float32(spk[np.arange(nt) % ne] + 0.5 * rng.standard_normal((nt, E)))
    cohort = np.float32(rng.standard_normal((nc, E)))
    _write(tmp_path / 'enrol', 'e', enrol)
    _write(tmp_path / 'test', 't', test)
    _write(tmp_path / 'cohort', 'c', cohort)
    pairs = [(i, j) for i in range(ne) for j in range(nt) if (i + j) % 3 == 0 or j % ne == i]
    (tmp_path / 'trials').write_text(
        ''.join(f'e{i} t{j} {"target" if j % ne == i else "nontarget"}\n' for i, j in pairs))
    ia, ib = np.array(pairs).T

    metrics = {}

    def run(name, *extra):
        metrics[name] = csm.main(['--enrol_data', str(tmp_path / 'enrol'), '--test_data', str(tmp_path / 'test'),
                                  '--scores_dir', str(tmp_path / name), '--trials', str(tmp_path / 'trials'),
                                  '--no_plot', *extra])['trials']
        return tmp_path / name / 'trials.score'

    plain = run('plain')
    none = run('none', '--score_norm', 'none')
    assert plain.read_bytes() == none.read_bytes()
    assert metrics['plain'] == metrics['none'] and 0 <= metrics['none'][0] < 0.5

    cdir = ['--cohort_data', str(tmp_path / 'cohort')]
    raw = score_norm._host_cosine(enrol, test)[ia, ib]
    eps = AFFINITY_ATOL
    for name, extra, k in (('asnorm', ['--score_norm', 'asnorm', '--top_n', str(top_n)], top_n),
                           ('snorm', ['--score_norm', 'snorm'], None)):
        got = _scores(run(name, *extra, *cdir))
        (mu_e, sd_e), (mu_t, sd_t) = score_norm.cohort_stats_host(enrol, cohort, k), \
            score_norm.cohort_stats_host(test, cohort, k)
        assert sd_e.min() >= 0.02 and sd_t.min() >= 0.02  # the bound below is used only above this
        ref = score_norm.as_norm_host(raw, mu_e[ia], sd_e[ia], mu_t[ib], sd_t[ib])
        side_e = 2 * eps / sd_e[ia] + np.abs(raw - mu_e[ia]) * eps / sd_e[ia] ** 2
        side_t = 2 * eps / sd_t[ib] + np.abs(raw - mu_t[ib]) * eps / sd_t[ib] ** 2
        bound = 0.5 * (side_e + side_t) + 5e-6
        err = np.abs(got - ref)
        print(f'cli {name}: max err {err.max():.3g}, smallest bound {bound.min():.3g}')
        assert (err <= bound).all(), _worst(err, bound)
        assert np.abs(got - _scores(plain)).max() > 0.1  # the normalised scores are what is written
    whole = run('asnorm_all', '--score_norm', 'asnorm', '--top_n', str(nc), *cdir)
    assert whole.read_bytes() == (tmp_path / 'snorm' / 'trials.score').read_bytes()
    assert metrics['asnorm_all'] == metrics['snorm']            # EER / minDCF come from the normalised scores
    clipped = run('asnorm_clip', '--score_norm', 'asnorm', '--top_n', str(nc + 50), *cdir)
    assert clipped.read_bytes() == whole.read_bytes()
