#!/usr/bin/env python
"""Times the corpus similarity analysis (speakerlab/utils/similarity_analysis.analyze: top-100
neighbours per speaker, 1000 extreme pairs, 50-bin histogram, 21 thresholds, quartiles) on synthetic
unit-normal embeddings, E = 192:

  python tools/similarity_bench.py [--sizes 20000,100000] [--host_size 20000]
                                   [--out profiles/similarity_bench.json]

On the device at every N of ``--sizes`` (the N x N matrix is never stored), and at ``--host_size``
also the numpy path on the host, which materialises the matrix; 0 skips it.  The parent of this
tool had no device path, so the host path is the baseline.  One warm-up run at the smallest N, then
the median of ``--repeats`` timed runs per arm with the device synchronised; every time is kept in
the output.  Needs a GPU; not a test."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, '3d-speaker_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='20000,100000')
    ap.add_argument('--host_size', type=int, default=20000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'similarity_bench.json'))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from speakerlab import _hip
    from speakerlab.utils import similarity_analysis as sa
    if not torch.cuda.is_available():
        raise SystemExit('similarity_bench needs a ROCm device')
    dev = torch.device('cuda')
    sizes = [int(s) for s in args.sizes.split(',') if s]
    result = {'e': 192, 'top_k': 100, 'n_extreme': 1000, 'device': torch.cuda.get_device_name(0), 'runs': []}

    def data(n):
        return np.random.default_rng(n).standard_normal((n, 192)).astype(np.float32), [f's{i}' for i in range(n)]

    x, keys = data(min(sizes))
    sa.analyze(x, keys, device=dev)                                # warm-up: library load, workspace allocation
    for n in sizes:
        x, keys = data(n)
        times, parts = [], []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            raw = sa.raw_on_device(x, 100, 1000, 50, sa.THRESHOLDS, dev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            sa.reports(raw, keys, 100)
            t2 = time.perf_counter()
            times.append(t2 - t0)
            parts.append({'kernels_and_copies_s': t1 - t0, 'reports_s': t2 - t1})
        lo, rec, st = _hip.cosine_sim_workspace_bytes(n)
        result['runs'].append({'n': n, 'arm': 'device', 'median_s': statistics.median(times), 'times_s': times,
                               'parts': parts, 'workspace_bytes': rec, 'state_bytes': st, 'pairs': n * (n - 1) // 2})
        print(json.dumps(result['runs'][-1]), flush=True)
        _hip.sim_release_workspace()
    if args.host_size:
        n = args.host_size
        x, keys = data(n)
        times = []
        for _ in range(max(1, min(args.repeats, 2))):
            t0 = time.perf_counter()
            sa.analyze(x, keys)
            times.append(time.perf_counter() - t0)
        result['runs'].append({'n': n, 'arm': 'host_numpy', 'median_s': statistics.median(times), 'times_s': times,
                               'threads': torch.get_num_threads(), 'pairs': n * (n - 1) // 2})
        print(json.dumps(result['runs'][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
