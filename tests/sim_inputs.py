"""Inputs and brute-force references shared by the similarity-statistics tests."""
import numpy as np


def tie_input(n=300, e=192, seed=7, copies=(11, 150, 299)):
    """Rows 10 and ``copies`` (11, 150 and 299) are copies of one vector and row 42 is all zeros: equal
    scores across the cuts of the row top-k and of the extreme pairs, and zeros.  The zero row scores
    +0.0 against everything (a sum that starts at +0.0 never ends at -0.0), so rows 20 and 21 are made
    to score -0.0 with each other: their dot product is -1e-36 and their norms 1e5, and -1e-46
    underflows to -0.0 in float32."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, e)).astype(np.float32)
    for r in copies:
        x[r] = x[10]
    x[42] = 0
    x[20] = 0
    x[21] = 0
    x[20, :2] = (1e-18, 1e5)
    x[21, :3] = (-1e-18, 0, 1e5)
    return x


def brute_rows(S, k):
    """Per row the k best other columns, score descending then column ascending, by a double loop."""
    N = S.shape[0]
    top_s = np.full((N, k), -np.inf, np.float32)
    top_i = np.full((N, k), -1, np.int64)
    for i in range(N):
        best = sorted(((-(float(S[i, j]) + 0.0), j) for j in range(N) if j != i))[:k]
        for r, (ns, j) in enumerate(best):
            top_s[i, r], top_i[i, r] = S[i, j] + np.float32(0), j
    return top_s, top_i


def brute_pairs(S, n, largest):
    """The n largest (smallest) pairs i < j as (score, i, j), ties in (i, j) order, by a double loop."""
    N = S.shape[0]
    sign = -1.0 if largest else 1.0
    allp = sorted((sign * (float(S[i, j]) + 0.0), i, j) for i in range(N) for j in range(i + 1, N))[:n]
    return (np.array([S[i, j] + np.float32(0) for _, i, j in allp], np.float32),
            np.array([i for _, i, _ in allp], np.int64), np.array([j for _, _, j in allp], np.int64))
