"""Brute-force statement of the all-pairs verification metrics, shared by the verification tests:
``np.unique`` on the keys and per-class cumulative counts, then the same formulas on the same integers
as speakerlab/utils/verification_analysis.py."""
import numpy as np

from speakerlab.utils import verification_analysis as va


def operating_points(keys, classes):
    """(distinct keys ascending, miss, fa, n_tgt, n_non, largest tie multiplicity) as Python-int arrays."""
    keys = np.asarray(keys, np.uint32)
    classes = np.asarray(classes).astype(np.int64)
    u, inv, mult = np.unique(keys, return_inverse=True, return_counts=True)
    tgt = np.bincount(inv, weights=(classes == 1), minlength=len(u)).astype(np.int64)
    non = np.bincount(inv, weights=(classes == 0), minlength=len(u)).astype(np.int64)
    n_tgt, n_non = int(tgt.sum()), int(non.sum())
    miss = np.cumsum(tgt)
    fa = n_non - np.cumsum(non)
    return u, miss, fa, n_tgt, n_non, int(mult.max())


def brute(keys, classes, p_target=0.01, c_miss=1, c_fa=1):
    u, miss, fa, n_tgt, n_non, mult = operating_points(keys, classes)
    x1 = next(q for q in range(len(u)) if int(miss[q]) * n_non >= int(fa[q]) * n_tgt)
    m1, f1 = int(miss[x1]), int(fa[x1])
    m2, f2 = (int(miss[x1 - 1]), int(fa[x1 - 1])) if x1 > 0 else (0, n_non)
    costs = [va.dcf_cost(int(m), int(f), n_tgt, n_non, p_target, c_miss, c_fa) for m, f in zip(miss, fa)]
    best = min(range(len(u)), key=lambda q: (costs[q], q))
    c_def = min(c_miss * p_target, c_fa * (1 - p_target))
    return dict(n_tgt=n_tgt, n_non=n_non, eer=va.eer_from_counts(m1, f1, m2, f2, n_tgt, n_non), eer_key=int(u[x1]),
                miss1=m1, fa1=f1, miss2=m2, fa2=f2, x1=x1, min_dcf=costs[best] / c_def, dcf_key=int(u[best]),
                dcf_miss=int(miss[best]), dcf_fa=int(fa[best]), max_tie=mult,
                fnr=miss / n_tgt, fpr=fa / n_non)


def check_against_brute(res_eer, res_dcf, want):
    """Integers exactly, floats to 1e-12 relative."""
    assert (res_eer['miss1'], res_eer['fa1'], res_eer['miss2'], res_eer['fa2']) == \
        (want['miss1'], want['fa1'], want['miss2'], want['fa2'])
    assert res_eer['key'] == want['eer_key']
    assert abs(res_eer['eer'] - want['eer']) <= 1e-12 * abs(want['eer'])
    assert res_dcf['exact'] is True
    assert (res_dcf['miss'], res_dcf['fa'], res_dcf['key']) == (want['dcf_miss'], want['dcf_fa'], want['dcf_key'])
    assert abs(res_dcf['min_dcf'] - want['min_dcf']) <= 1e-12 * abs(want['min_dcf'])
    assert res_dcf['bound'] == res_dcf['min_dcf']
