"""speakerlab/bin/compute_speaker_similarities.py on the device against its numpy path, on the tiny
tree of tests/sim_cli_tree.py: selection fields exactly equal, float fields to the tolerance of the
golden test (tests/test_sim_golden.py)."""
import json
import os

import numpy as np
import pytest

import sim_cli_tree as tree

pytestmark = pytest.mark.gpu


def _tolerance():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sim_golden.json')) as f:
        g = json.load(f)
    return 4 * g['d_ref'] + g['affinity_parity']


def _same(a, b, tol, path=''):
    if isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], tol, f'{path}/{k}')
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for n, (u, v) in enumerate(zip(a, b)):
            _same(u, v, tol, f'{path}[{n}]')
    elif isinstance(a, float) and not path.endswith('percentage'):
        assert abs(a - b) <= tol, (path, a, b)
    else:
        assert a == b, (path, a, b)


def test_device_run_equals_the_numpy_path(tmp_path):
    host, dev = tmp_path / 'host', tmp_path / 'dev'
    for d in (host, dev):
        d.mkdir()
        tree.make_tree(str(d))
    want = tree.run(str(host), '--save_matrix')
    got = tree.run(str(dev), '--save_matrix', device='cuda')
    assert set(got) == set(want) == tree.ALWAYS | tree.MATRIX
    tol = _tolerance()
    assert 2e-6 <= tol < 1e-4
    # speakers, pair identities, ranks, counts (the random scores have no ties within the tolerance, so the
    # orders are the same): everything that is not a float is compared exactly
    for name in want:
        if name.endswith('.npy'):
            assert got[name].shape == want[name].shape and np.abs(got[name] - want[name]).max() <= tol, name
        else:
            _same(got[name], want[name], tol, name)
