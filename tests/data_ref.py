"""fp64 references, error bounds and case inputs for the kernels around the network: the cosine
affinity / top-k / trials (csrc/affinity.hip, cosine_pair.h), the Fbank (csrc/fbank.hip) and the
spectral Laplacian (csrc/spectral.hip).  Plain numpy, no GPU: ``tests/test_data_ref_host.py``
proves on the host that every case can fail and that a correct fp32 evaluation stays inside every
bound; the ``test_gpu_*_edges.py`` files hold the kernels to the same references and bounds.

All bounds use u = 2^-24 (fp32 unit roundoff) and are worst-case (every rounding at its limit,
all with the same sign), like the resampler's in ``tests/test_gpu_resample.py``; no figure here
was measured on the code under test.
"""
from __future__ import annotations

import numpy as np

from oracle import fbank_ref

U = 2.0 ** -24


# ----------------------------------------------------------------------------- cosine
def _unit_norms(x):
    n = np.sqrt((x * x).sum(1))
    n[n == 0] = 1.0
    return n


def cos_ref(a, b, drop_tail=0):
    """(S, mag) in fp64: S_ij = <a_i, b_j> / (|a_i| |b_j|), mag_ij = sum_k |a_ik b_jk| / (|a_i| |b_j|);
    zero norms are replaced by 1 (sklearn normalize()).  ``drop_tail`` > 0 is the mutant of the
    host tests: the dot product (not the norms) leaves out the last ``drop_tail`` elements of K."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    den = _unit_norms(a)[:, None] * _unit_norms(b)[None, :]
    ke = a.shape[1] - drop_tail
    return (a[:, :ke] @ b[:, :ke].T) / den, (np.abs(a) @ np.abs(b).T) / den


def cos_bound(S, mag, E):
    """|fp32 result - S| <= (E + 2) u mag + (E + 4) u |S|.

    Numerator: one fp32 accumulation of E products, in any order (a chain, the MFMA's pairs, a
    wave reduction): every product carries one rounding and takes part in at most E - 1
    additions, so the error is at most gamma_E sum |a_k b_k| <= (E + 2) u sum |a_k b_k| for
    E u << 1 (the + 2 covers the second-order terms of gamma_E up to E = 10^4).
    Denominator and quotient, relative to |S|: each squared norm is such a sum of E positive
    terms (relative error <= E u), the square root halves that and adds u / 2 (E u / 2 + u / 2
    per norm, E u + u for both), the product of the norms one u, the division one u: E u + 3 u,
    and (E + 4) u with the second-order terms."""
    return (E + 2) * U * mag + (E + 4) * U * np.abs(S)


def cos_f32(a, b):
    """The same formula evaluated in float32 numpy (an independent, correct fp32 implementation)."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)

    def nrm(x):
        n = np.sqrt(np.einsum('ik,ik->i', x, x, dtype=np.float32))
        n[n == 0] = np.float32(1)
        return n
    d = np.einsum('ik,jk->ij', a, b, dtype=np.float32)
    return d / (nrm(a)[:, None] * nrm(b)[None, :])


def np_topk(S, k, self_off):
    """Lexicographic top-k of every row: score descending, column ascending among equal scores;
    column i + self_off of row i is excluded when ``self_off`` is not None.  (scores, columns)."""
    S = S.copy()
    if self_off is not None:
        r = np.arange(S.shape[0])
        ok = (r + self_off >= 0) & (r + self_off < S.shape[1])
        S[r[ok], r[ok] + self_off] = -np.inf
    order = np.lexsort((np.broadcast_to(np.arange(S.shape[1]), S.shape), -S), axis=1)[:, :k]
    return np.take_along_axis(S, order, 1), order


def topk_tiles_per_seg(Na, Nb):
    """(tiles_per_seg, nseg) as launch_cosine_topk (affinity.hip) cuts the 128-column tiles of B
    into segments: about 512 blocks over the row tiles, at most one segment per tile."""
    rt, ct = (Na + 127) // 128, (Nb + 127) // 128
    nseg = max(1, min((512 + rt - 1) // rt, ct))
    tps = (ct + nseg - 1) // nseg
    return tps, (ct + tps - 1) // tps


ZERO_ROWS = (0, 63, 64, 127, 128)

# (Na, Nb, E, kind): every E in {4, 8, 12, 16, 20, 36, 196} (one k-tile; E % 16 in {4, 8, 12, 0};
# nkt = 1, 2, 3, 13: odd and even) and every shape; 'pos' rows are all positive (cos near 1, mag = S),
# 'zeros' has zero rows at ZERO_ROWS of both operands
AFF_CASES = [(1, 1, 4, 'normal'), (1, 1, 196, 'normal'),
             (63, 65, 8, 'normal'), (63, 65, 20, 'normal'), (63, 65, 36, 'zeros'),
             (64, 128, 4, 'normal'), (64, 128, 12, 'zeros'), (64, 128, 16, 'normal'),
             (127, 129, 8, 'zeros'), (127, 129, 20, 'normal'), (127, 129, 196, 'normal'),
             (129, 127, 12, 'normal'), (129, 127, 16, 'zeros'), (129, 127, 36, 'normal'), (129, 127, 20, 'pos'),
             (257, 130, 4, 'zeros'), (257, 130, 8, 'normal'), (257, 130, 12, 'normal'), (257, 130, 16, 'normal'),
             (257, 130, 20, 'zeros'), (257, 130, 36, 'normal'), (257, 130, 196, 'zeros'), (257, 130, 196, 'pos')]


def aff_data(na, nb, e, kind):
    rng = np.random.default_rng(1000 * na + 10 * nb + e)
    if kind == 'pos':
        return (rng.uniform(0.5, 1.5, (na, e)).astype(np.float32), rng.uniform(0.5, 1.5, (nb, e)).astype(np.float32))
    a = rng.standard_normal((na, e)).astype(np.float32)
    b = rng.standard_normal((nb, e)).astype(np.float32)
    if kind == 'zeros':
        a[[i for i in ZERO_ROWS if i < na]] = 0
        b[[i for i in ZERO_ROWS if i < nb]] = 0
    return a, b


def live(a, b):
    """Entries whose two rows are non-zero: the others are exactly 0 in any implementation (the
    edge tests pin that), so no mutant of the arithmetic can move them."""
    return np.any(a != 0, axis=1)[:, None] & np.any(b != 0, axis=1)[None, :]


# the multi-tile-segment top-k case: tiles_per_seg = 3, last segment 2 tiles
TOPK_BIG = (8192, 2176, 16, 4)
TOPK_GAP = 1e-5          # indices are compared where the fp64 gap to both neighbouring scores exceeds this
TOPK_MASK_CAP = 0.005    # ... which may leave out at most this share of the entries

# (E, T) of the trial cases: E > 256 takes the wave's second k += 256 trip, 260 and 516 a partial one
TRIAL_CASES = [(4, 1), (4, 5), (68, 5), (68, 4097), (256, 5), (260, 1), (260, 4097), (516, 5), (516, 4097)]


def trial_data(e, t):
    """(A [211, E], ia, ib) for trials scored on one matrix; trial 0 has ia == ib."""
    rng = np.random.default_rng(7 * e + t)
    A = rng.standard_normal((211, e)).astype(np.float32)
    ia, ib = rng.integers(0, 211, t), rng.integers(0, 211, t)
    ib[0] = ia[0]
    if t > 2:
        ib[t // 2] = ia[t // 2]
    return A, ia, ib


# ----------------------------------------------------------------------------- Fbank
FLT_EPS = fbank_ref.FLT_EPS
FLOOR32 = np.float32(np.log(np.float64(FLT_EPS)))


def fbank_energies(wav, n_mels):
    """The fp64 band energies of oracle/fbank_ref.fbank, before the floor and the log."""
    fr = fbank_ref.windowed_frames(np.asarray(wav), np.float64)
    spec = np.fft.rfft(fr, axis=1)
    return (spec.real ** 2 + spec.imag ** 2) @ fbank_ref.mel_banks(n_mels).T


def ulp32(x):
    """Spacing of float32 at |x| + 2^-22 (the offset keeps a value that the allowed error moves
    across a power of two inside the bound)."""
    return np.spacing((np.abs(np.asarray(x, dtype=np.float64)) + 2.0 ** -22).astype(np.float32)).astype(np.float64)


def fbank_bound(ref):
    """Without mean_nor: |out - ref| <= ulp32(ref) / 2 + 2^-23.

    The kernel works in fp64 up to the band energy e (its error against the fp64 oracle is some
    1e-13 relative, negligible), then takes log e = k ln 2 + logf(m), e = m 2^k, m in [1, 2):
    rounding m to fp32 moves log m by at most 2^-24 (d log m = dm / m, m >= 1), logf is good to
    one ulp of a result in [0, ln 2), at most 2^-24 -- together 2^-23, the same allowance as two
    ulps of logf on [1, 2) -- and the sum is rounded once to fp32 (half an ulp of the result).
    The 2^-23 is absolute: for e in [0.5, 1) the two terms cancel to a small result whose own ulp
    is far smaller."""
    return 0.5 * ulp32(ref) + 2.0 ** -23


def fbank_mn_bound(ref, ref_mn):
    """With mean_nor: b_t + mean_t(b) + ulp32(ref_mn) / 2 per entry: the stored fp32 row (b_t), the
    mean of the stored rows summed in fp64 (the mean of their errors), one rounding of the
    difference."""
    b = fbank_bound(ref)
    return b + b.mean(axis=0, keepdims=True) + 0.5 * ulp32(ref_mn)


def on_floor(energies):
    """Entries safely on the floor (a part in 1e9 below FLT_EPSILON, far above the fp64 noise):
    the result there must be FLOOR32 exactly."""
    return energies <= FLT_EPS * (1.0 - 1e-9)


def fbank_log_f32(energies):
    """The kernel's log formula (fbank.hip log_d2f) in float32 numpy on fp64 energies: the fp32
    evaluation that has to stay inside ``fbank_bound``."""
    e = np.maximum(energies, FLT_EPS)
    m, k = np.frexp(e)                      # e = m 2^k, m in [0.5, 1)
    m, k = 2.0 * m, k - 1
    return (k * np.log(2.0) + np.log(m.astype(np.float32)).astype(np.float64)).astype(np.float32)


def fbank_check(out, wav, n_mels, mean_nor, what=''):
    """Assert one utterance's kernel output against the oracle; returns max err / bound."""
    out = np.asarray(out)
    ref = fbank_ref.fbank(wav, n_mels, False, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    if ref.shape[0] == 0:
        return 0.0
    if mean_nor:
        ref_mn = ref - ref.mean(axis=0, keepdims=True)
        ratio = np.abs(out - ref_mn) / fbank_mn_bound(ref, ref_mn)
    else:
        fl = on_floor(fbank_energies(wav, n_mels))
        assert np.all(out[fl] == FLOOR32), (what, 'floor', out[fl][out[fl] != FLOOR32][:4])
        ratio = np.abs(out - ref) / fbank_bound(ref)
    assert np.all(ratio <= 1.0), (what, float(ratio.max()))
    return float(ratio.max())


N_MELS = (4, 23, 40, 64, 81, 128)
FB_LENGTHS = (400, 559, 560, 720, 1360)     # 1, 1, 2, 3, 7 frames
FB3 = 720                                   # three frames


def noise(n, amp, seed):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _search_amp(pred, n_mels=80):
    """First amplitude 2^(-j/2), j = 0.., whose three-frame white noise satisfies ``pred(energies)``."""
    for j in range(0, 70):
        amp = 2.0 ** (-0.5 * j)
        if pred(fbank_energies(noise(FB3, amp, 5), n_mels)):
            return amp
    raise AssertionError('no amplitude found')


def fbank_signals():
    """name -> three-frame float32 signal (full scale = 1.0)."""
    sig = {f'noise_2^{p}': noise(FB3, 2.0 ** p, 40 + p) for p in (-30, -24, -18, -12, -6, 0)}
    # some bands on the FLT_EPSILON floor and others above it
    amp = _search_amp(lambda e: 0.2 <= on_floor(e).mean() <= 0.8)
    sig['noise_mixed_floor'] = noise(FB3, amp, 5)
    # >= 10 % of the band energies in [0.5, 1): k ln 2 + logf(m) cancels
    amp = _search_amp(lambda e: ((e >= 0.5) & (e < 1.0)).mean() >= 0.10)
    sig['noise_half_to_one'] = noise(FB3, amp, 5)
    sig['dc_plus_noise'] = (np.float32(0.9) + noise(FB3, 1e-4, 6)).astype(np.float32)
    sig['constant'] = np.full(FB3, 0.25, np.float32)
    t = np.arange(FB3)
    sig['tone_bin_centre'] = (0.5 * np.sin(2 * np.pi * 64 * t / 512)).astype(np.float32)   # bin 64 = 2 kHz
    sig['nyquist'] = np.where(t % 2 == 0, 1.0, -1.0).astype(np.float32)
    imp0 = np.zeros(FB3, np.float32)
    imp0[0] = 1.0
    sig['impulse_0'] = imp0
    imp399 = np.zeros(FB3, np.float32)
    imp399[399] = 1.0                         # sample 399 of frame 0 (239 of frame 1, 79 of frame 2)
    sig['impulse_399'] = imp399
    return sig


# ----------------------------------------------------------------------------- Laplacian
def laplacian_ref(S, n_elems):
    """The reference's loops (cluster.py p_pruning + get_laplacian) on float32 S with a STABLE
    argsort, which zeroes the lowest index first among ties; off-diagonals in float32 (exact:
    0.5 (p + q) is one rounding, the same in any correct implementation), the diagonal in fp64.
    (L float64 [N, N], rowabs [N] = sum_j |L_ij| over j != i in fp64)."""
    A = np.array(S, dtype=np.float32, copy=True)
    n = A.shape[0]
    for i in range(n):
        A[i, np.argsort(S[i], kind='stable')[:n_elems]] = 0
    M = np.float32(0.5) * (A + A.T)
    M[np.diag_indices(n)] = 0
    M = M.astype(np.float64)
    rowabs = np.abs(M).sum(1)
    return np.diag(rowabs) - M, rowabs


def laplacian_diag_bound(N, rowabs):
    """|L_ii - sum_j |L_ij|| <= (N / 256 + 10) u sum_j |L_ij|: degree_kernel adds ceil(N / 256)
    terms per thread in a chain, then an 8-level tree over the 256 partial sums: at most
    N / 256 + 8 additions touch any term, plus 2 of slack for the second-order terms."""
    return (N / 256.0 + 10.0) * U * rowabs


def laplacian_f32(S, n_elems):
    """The same in float32 numpy throughout (diagonal by a float32 sum)."""
    A = np.array(S, dtype=np.float32, copy=True)
    n = A.shape[0]
    for i in range(n):
        A[i, np.argsort(S[i], kind='stable')[:n_elems]] = 0
    M = np.float32(0.5) * (A + A.T)
    M[np.diag_indices(n)] = 0
    return np.diag(np.abs(M).sum(1, dtype=np.float32)) - M


def tie_matrix(n, seed):
    """Symmetric, entries from {-0.5, -0.25, 0, 0.25, 0.5}: hundreds of ties at any cut."""
    rng = np.random.default_rng(seed)
    v = np.array([-0.5, -0.25, 0.0, 0.25, 0.5], np.float32)[rng.integers(0, 5, (n, n))]
    S = np.triu(v) + np.triu(v, 1).T
    return np.ascontiguousarray(S, dtype=np.float32)


def random_affinity(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 16))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (x @ x.T).astype(np.float32)


LAP_N = (1, 2, 31, 32, 33, 1023, 1024, 1025)


def lap_n_elems(n):
    return sorted({0, min(1, n), max(n - 1, 0), n})


def clique_laplacian(sizes, seed=0):
    """Unnormalised Laplacian (float32) of disconnected cliques whose edge weights are affinities
    drawn from (0.3, 0.9): eigenvalue 0 has one eigenvector per clique."""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    W = np.zeros((n, n), np.float32)
    o = 0
    for s in sizes:
        w = rng.uniform(0.3, 0.9, (s, s)).astype(np.float32)
        W[o:o + s, o:o + s] = np.triu(w, 1) + np.triu(w, 1).T
        o += s
    return (np.diag(W.sum(1, dtype=np.float32)) - W).astype(np.float32)


def eig_cases():
    """name -> (A float32 symmetric, number of cliques or None)."""
    return {'cliques3_n33': (clique_laplacian([10, 11, 12]), 3),
            'cliques5_n200': (clique_laplacian([20, 30, 40, 50, 60]), 5),
            'diagonal_n64': (np.diag(np.linspace(-3, 5, 64)).astype(np.float32), None),
            'n1': (np.array([[2.5]], np.float32), None),
            'n2': (np.array([[2.0, -0.75], [-0.75, 1.25]], np.float32), None)}


def eig_quantities(A, w, V):
    """(eigenvalue error, residual, orthogonality defect), each divided by N u |A|_2, of computed
    eigenvalues ``w`` and eigenvectors as ROWS of ``V`` against fp64 eigvalsh."""
    A64 = A.astype(np.float64)
    n = A.shape[0]
    ref = np.linalg.eigvalsh(A64)
    scale = n * U * max(np.abs(ref).max(), np.finfo(np.float32).tiny)
    w = np.asarray(w, np.float64)
    V = np.asarray(V, np.float64)
    return (np.abs(w - ref).max() / scale, np.abs(A64 @ V.T - V.T * w[None]).max() / scale,
            np.abs(V @ V.T - np.eye(n)).max() / (n * U))


def topk_with_bound(a, b, k, self_off, drop_tail=0, shift_col=None):
    """(scores, columns, bound at those columns, gap) of the fp64 reference's top-k; ``gap`` is the
    smaller of the fp64 distances to the next and to the previous score of the row: two scores
    closer than rounding may come out in either order, which moves BOTH of their positions, so a
    position's column is decided only when both of its neighbours are clear of it.  ``drop_tail``
    / ``shift_col`` build the host tests' mutants (column ``shift_col`` of B scored with row
    shift_col + 1)."""
    if shift_col is not None:
        b = b.copy()
        b[shift_col] = b[(shift_col + 1) % len(b)]
    S, mag = cos_ref(a, b, drop_tail)
    kk = min(k + 1, S.shape[1])
    sc, ix = np_topk(S, kk, self_off)
    bound = cos_bound(sc, np.take_along_axis(mag, ix, 1), a.shape[1])
    nxt = np.concatenate([sc[:, 1:], np.full((len(sc), 1), -np.inf)], 1)
    prv = np.concatenate([np.full((len(sc), 1), np.inf), sc[:, :-1]], 1)
    k = min(k, S.shape[1])
    return sc[:, :k], ix[:, :k], bound[:, :k], np.minimum(sc - nxt, prv - sc)[:, :k]


def topk_big_data():
    na, nb, e, _ = TOPK_BIG
    rng = np.random.default_rng(8192)
    return rng.standard_normal((na, e)).astype(np.float32), rng.standard_normal((nb, e)).astype(np.float32)


def onehot_data():
    """One-hot rows: every score is exactly 0 or 1, so count(score >= 1.0) is exact.  (a [130, 20],
    b [300, 20]); every hot index occurs in b."""
    rng = np.random.default_rng(20)
    hb = np.concatenate([np.arange(20), rng.integers(0, 20, 280)])
    ha = rng.integers(0, 20, 130)
    return np.eye(20, dtype=np.float32)[ha] * np.float32(3), np.eye(20, dtype=np.float32)[hb] * np.float32(0.5)


# top-k tie cases: (Nb, E, groups of columns that hold one row each, self offsets); row g of A is
# the row of group g, so its best scores are that group's columns, tied bit for bit
TIE_SMALL = (300, 16, [(62, 63, 64, 65), (126, 127, 128, 129), (254, 255, 256, 257), (0, 1, 2, 3),
                       (296, 297, 298, 299)], [None, 0, 62, 127, -1])


def tie_large():
    """Nb large enough for multi-tile segments at a small Na: groups straddle the first, some
    middle and the last segment boundary (tiles_per_seg as launch_cosine_topk computes it)."""
    nb, na = 128 * 600 + 5, 6
    tps, nseg = topk_tiles_per_seg(na, nb)
    assert tps > 1 and nseg > 2
    bnd = [128 * tps * s for s in (1, 2, nseg // 2, nseg - 2, nseg - 1)]
    groups = [(c - 2, c - 1, c, c + 1) for c in bnd] + [(nb - 2, nb - 1)]
    return nb, 16, groups, [None, bnd[0] - 1]


def topk_tie_data(nb, e, groups, seed=3):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((nb, e)).astype(np.float32)
    A = rng.standard_normal((len(groups), e)).astype(np.float32)
    for g, cols in enumerate(groups):
        B[list(cols)] = A[g]
    return A, B


_FT_MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include "fbank.h"
int main(int argc, char** argv) {
  static spk::FbankTables t;
  for (int i = 1; i < argc; ++i)
    std::printf("%d %d\n", std::atoi(argv[i]), spk::build_fbank_tables(&t, std::atoi(argv[i]), 16000.0));
  return 0;
}
'''
_ft_cache = {}


def fbank_tables_accept(n_mels_list):
    """{n_mels: accepted} from build_fbank_tables itself: csrc/fbank_tables.cpp compiled into a
    small host program (once per process) and run on the values."""
    import os
    import subprocess
    import tempfile
    key = tuple(n_mels_list)
    if key not in _ft_cache:
        csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), '3d-speaker_amd', 'csrc')
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, 'main.cpp'), 'w') as f:
                f.write(_FT_MAIN)
            exe = os.path.join(d, 'ft')
            subprocess.run(['g++', '-std=c++17', '-O1', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include', '-I' + csrc,
                            os.path.join(csrc, 'fbank_tables.cpp'), os.path.join(d, 'main.cpp'), '-o', exe], check=True)
            out = subprocess.run([exe] + [str(n) for n in key], check=True, capture_output=True, text=True).stdout
        _ft_cache[key] = {int(l.split()[0]): int(l.split()[1]) >= 0 for l in out.splitlines()}
    return _ft_cache[key]
