"""Cohort score normalisation of verification trials: S-norm and AS-norm (adaptive, top-N).

For a trial (e, t) with raw cosine s, and a cohort of embeddings C,

    score = 0.5 * ((s - mu_e) / sd_e + (s - mu_t) / sd_t)

where mu_e / sd_e are the mean and the population standard deviation (ddof 0) of the ``top_n``
largest cosines of e against C, and mu_t / sd_t the same for t.  ``top_n=None`` uses the whole
cohort (S-norm).  A standard deviation below 1e-6 is replaced by 1e-6, which keeps a degenerate
cohort (all of the top scores equal) finite.

``cohort_stats`` / ``as_norm`` run on the MI355X (``spk_cosine_cohort_stats`` /
``spk_cosine_trials_norm``); ``cohort_stats_host`` / ``as_norm_host`` are the float64 numpy
restatement the device path is tested against, and what the device functions fall back to when the
library was built without the kernels (``E_UNSUPPORTED``), and only then.
"""
import numpy as np

STD_FLOOR = float(np.float32(1e-6))   # the float32 constant of the kernel


def _host_cosine(a, b):
    """sklearn-style cosine in float64: zero-norm rows divide by 1 (process/cluster.py _host_cosine)."""
    def nrm(x):
        x = np.asarray(x, dtype=np.float64)
        n = np.linalg.norm(x, axis=1, keepdims=True)
        n[n == 0] = 1.0
        return x / n
    return nrm(a) @ nrm(b).T


def _clip_top_n(top_n, nc):
    if nc < 1:
        raise ValueError('score normalisation needs a cohort of at least one embedding')
    if top_n is None:
        return nc
    top_n = int(top_n)
    if top_n < 1:
        raise ValueError(f'top_n must be at least 1, got {top_n}')
    return min(top_n, nc)              # as a numpy slice would


def topk_stats_host(S, k):
    """(mean, std) float64 [rows] of the ``k`` largest entries of every row (np.partition)."""
    S = np.asarray(S, dtype=np.float64)
    k = _clip_top_n(k, S.shape[1])
    top = np.partition(S, S.shape[1] - k, axis=1)[:, S.shape[1] - k:]
    return top.mean(axis=1), top.std(axis=1)


def cohort_stats_host(x, cohort, top_n=None):
    """(mean, std) float64 [N] of the ``top_n`` best cosines of every row of ``x`` [N, E] against
    ``cohort`` [Nc, E]; ``top_n=None`` is the whole cohort, ``top_n > Nc`` is clipped to Nc."""
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    cohort = np.asarray(cohort, dtype=np.float64).reshape(len(cohort), -1)
    k = _clip_top_n(top_n, cohort.shape[0])
    if x.shape[0] == 0:
        return np.zeros(0), np.zeros(0)
    return topk_stats_host(_host_cosine(x, cohort), k)


def as_norm_host(raw, mu_e, sd_e, mu_t, sd_t):
    """The normalised scores in float64; every argument is per trial (already gathered)."""
    raw = np.asarray(raw, dtype=np.float64)
    ze = (raw - np.asarray(mu_e, dtype=np.float64)) / np.maximum(np.asarray(sd_e, dtype=np.float64), STD_FLOOR)
    zt = (raw - np.asarray(mu_t, dtype=np.float64)) / np.maximum(np.asarray(sd_t, dtype=np.float64), STD_FLOOR)
    return 0.5 * (ze + zt)


def cohort_stats(x, cohort, top_n=None, device='cuda'):
    """Device form of ``cohort_stats_host``: (mean, std) float32 [N] numpy arrays."""
    import torch
    from speakerlab import _hip
    x = np.asarray(x, dtype=np.float32).reshape(len(x), -1)
    cohort = np.asarray(cohort, dtype=np.float32).reshape(len(cohort), -1)
    k = _clip_top_n(top_n, cohort.shape[0])
    if x.shape[0] == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    try:
        mean, std = _hip.cosine_cohort_stats(torch.from_numpy(x).to(device), torch.from_numpy(cohort).to(device), k)
    except _hip.HipError as e:
        if e.code != _hip.E_UNSUPPORTED:
            raise
        mean, std = cohort_stats_host(x, cohort, k)
        return mean.astype(np.float32), std.astype(np.float32)
    return mean.cpu().numpy(), std.cpu().numpy()


def as_norm(enrol, test, ia, ib, stats_e, stats_t, device='cuda'):
    """Device form of ``as_norm_host`` fused with the trial gather: float32 [n_trials] scores of
    the trials (enrol[ia[t]], test[ib[t]]), ``stats_e`` / ``stats_t`` the (mean, std) of
    ``cohort_stats`` over the rows of ``enrol`` / ``test``."""
    import torch
    from speakerlab import _hip
    enrol = np.asarray(enrol, dtype=np.float32).reshape(len(enrol), -1)
    test = np.asarray(test, dtype=np.float32).reshape(len(test), -1)
    ia = np.asarray(ia, dtype=np.int64)
    ib = np.asarray(ib, dtype=np.int64)
    a, b = torch.from_numpy(enrol).to(device), torch.from_numpy(test).to(device)
    ta, tb = torch.from_numpy(ia), torch.from_numpy(ib)
    try:
        return _hip.cosine_trials_norm(a, b, ta, tb, tuple(torch.as_tensor(np.asarray(v, np.float32)) for v in stats_e),
                                       tuple(torch.as_tensor(np.asarray(v, np.float32)) for v in stats_t)).cpu().numpy()
    except _hip.HipError as e:
        if e.code != _hip.E_UNSUPPORTED:
            raise
    raw = _hip.cosine_trials(a, b, ta, tb).cpu().numpy()
    (mu_e, sd_e), (mu_t, sd_t) = stats_e, stats_t
    return as_norm_host(raw, np.asarray(mu_e)[ia], np.asarray(sd_e)[ia], np.asarray(mu_t)[ib],
                        np.asarray(sd_t)[ib]).astype(np.float32)
