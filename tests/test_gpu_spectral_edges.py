"""Edge cases of the spectral kernels (csrc/spectral.hip) against tests/data_ref.py: the tie rule
of p_prune_kernel across its 1024-column chunks, n_elems in {0, 1, N - 1, N}, N at the 32-tile
and 1024-chunk edges, row strides above N through the C ABI, and rocSOLVER's eigenpairs on the
degenerate spectra that Laplacians of separated speakers have."""
import numpy as np
import pytest
import torch

import data_ref as D
from speakerlab import _hip

pytestmark = pytest.mark.gpu


def _gpu_laplacian(S, ne):
    return _hip.spectral_laplacian(torch.from_numpy(S).cuda(), ne).cpu().numpy()


def _check_laplacian(L, S, ne, what):
    n = len(S)
    ref, rowabs = D.laplacian_ref(S, ne)
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(L[off], ref[off]), what
    assert np.array_equal(L, L.T), what
    err = np.abs(np.diag(L) - np.diag(ref))
    bound = D.laplacian_diag_bound(n, rowabs)
    assert np.all(err <= bound), (what, float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize('n', [1030, 2050])
def test_ties_at_the_cut_across_chunks(n):
    """Five distinct values: every row has hundreds of ties at the cut, which the kernel zeroes
    lowest index first with a count carried over the 1024-column chunks."""
    S = D.tie_matrix(n, 7)
    S[3, 5:40:2] = -0.0                       # a row with both zeros at the cut (they compare equal)
    S[5:40:2, 3] = -0.0
    worst = 0.0
    for frac in (0.9, 0.3, 0.5):
        ne = int(frac * n)
        worst = max(worst, _check_laplacian(_gpu_laplacian(S, ne), S, ne, (n, ne)))
    print(f'laplacian ties N={n}: max diag err/bound {worst:.3f}')


@pytest.mark.parametrize('n', D.LAP_N)
def test_random_affinities_every_n_elems(n):
    S = D.random_affinity(n, n)
    worst = 0.0
    for ne in D.lap_n_elems(n):
        worst = max(worst, _check_laplacian(_gpu_laplacian(S, ne), S, ne, (n, ne)))
    print(f'laplacian N={n}: max diag err/bound {worst:.3f}')


@pytest.mark.parametrize('n,ne', [(33, 20), (1025, 700)])
def test_abi_with_row_strides(n, ne):
    """lds = N + 3, ldl = N + 5 through the C ABI, the extra columns NaN: those of L survive,
    those of S never reach the result."""
    S = D.random_affinity(n, n + 1)
    Sw = np.full((n, n + 3), np.nan, np.float32)
    Sw[:, :n] = S
    dS = torch.from_numpy(Sw).cuda()
    dL = torch.full((n, n + 5), float('nan'), device='cuda')
    ws = torch.empty(n * n, dtype=torch.float32, device='cuda')
    rc = _hip.lib().spk_spectral_laplacian(dS.data_ptr(), n, n + 3, ne, dL.data_ptr(), n + 5, ws.data_ptr(),
                                           ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _hip.lib().spk_last_error()
    L = dL.cpu().numpy()
    assert np.isnan(L[:, n:]).all()
    _check_laplacian(L[:, :n], S, ne, (n, ne))
    assert np.array_equal(L[:, :n], _gpu_laplacian(S, ne))


# float32 numpy.linalg.eigh (LAPACK ssyevd, the reference implementation of this step, not the code
# under test) on D.eig_cases(), in units of N u |A|_2 (orthogonality: N u):
#   eigenvalues 0.143, residual 0.154, orthogonality 0.524 at worst (all three at N = 2; 0.024 /
#   0.016 / 0.028 at N = 33, 0.004 / 0.002 / 0.004 at N = 200)  ->  c = 4 * 0.524 = 2.1
# (four times the worst, since an independent LAPACK may differ by a small factor)
EIG_C = 2.1


@pytest.mark.parametrize('name', list(D.eig_cases()))
def test_symmetric_eig_degenerate_spectra(name):
    """Eigenvalues ascending and within c N u |A|_2 of fp64 eigvalsh, residual |A V^T - V^T diag(w)|_max
    within the same, |V V^T - I|_max within c N u.  c cannot be derived for rocSOLVER's divide and
    conquer: it is 4 x the worst of the three for float32 numpy.linalg.eigh on the same matrices
    (0.143 / 0.154 / 0.524 -> c = 2.1).  The number of eigenvalues below 1e-4 |A| is the number of
    cliques."""
    A, cliques = D.eig_cases()[name]
    w, V = _hip.symmetric_eig(torch.from_numpy(A.copy()).cuda())
    w, V = w.cpu().numpy(), V.cpu().numpy()
    assert np.all(np.diff(w) >= 0)
    q = D.eig_quantities(A, w, V)
    print(f'eig {name}: eigenvalue {q[0]:.3f}, residual {q[1]:.3f}, orthogonality {q[2]:.3f} (c = {EIG_C})')
    assert max(q) <= EIG_C, q
    if cliques is not None:
        norm = np.abs(np.linalg.eigvalsh(A.astype(np.float64))).max()
        assert int((np.abs(w) < 1e-4 * norm).sum()) == cliques
