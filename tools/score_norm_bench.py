#!/usr/bin/env python
"""Cohort statistics of AS-norm: the host restatement (cohort_stats_host: float64 cosine matrix +
np.partition, what a user writes today) vs the device path (spk_cosine_cohort_stats), interleaved
in one process on the same fp32 embeddings.

  python tools/score_norm_bench.py [--sizes 5000,20000] [--out profiles/score_norm_bench.json]

For every size N = Nc (E = 192, K = 300) both arms start from host float32 arrays and end with the
statistics on the host: the device arm includes the upload of the embeddings, the row-blocked
affinity + top-K kernels and the download (a device synchronise ends it); ``device_kernels_s`` is
the same call on embeddings already resident, timed to a synchronise.  The host arm runs on
``--threads`` threads.  Median of ``--repeats`` after ``--warmup`` runs of each arm, every time kept
in the output, with the largest difference of the two results."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, '3d-speaker_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='5000,20000')
    ap.add_argument('--embed', type=int, default=192)
    ap.add_argument('--top_n', type=int, default=300)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'score_norm_bench.json'))
    args = ap.parse_args(argv)

    os.environ.setdefault('OMP_NUM_THREADS', str(args.threads))
    import numpy as np
    import torch
    from speakerlab import _hip
    from speakerlab.utils import score_norm
    torch.set_num_threads(args.threads)
    assert torch.cuda.is_available(), 'score_norm_bench needs a ROCm device'

    def write(rows):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'embed': args.embed, 'top_n': args.top_n,
                       'repeats': args.repeats, 'warmup': args.warmup, 'host_threads': args.threads,
                       'host_arm': 'cohort_stats_host (float64 cosine + np.partition)', 'rows': rows}, f, indent=1)
            f.write('\n')

    rows = []
    for n in (int(v) for v in args.sizes.split(',')):
        rng = np.random.default_rng(n)
        spk = rng.standard_normal((n // 10 + 1, args.embed))
        x = (spk[rng.integers(0, len(spk), n)] + 0.8 * rng.standard_normal((n, args.embed))).astype(np.float32)
        c = (spk[rng.integers(0, len(spk), n)] + 0.8 * rng.standard_normal((n, args.embed))).astype(np.float32)
        k = min(args.top_n, n)
        host_s, dev_s, kern_s, host, dev = [], [], [], None, None
        for rep in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            host = score_norm.cohort_stats_host(x, c, k)
            t1 = time.perf_counter()
            dev = score_norm.cohort_stats(x, c, k)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            _hip.cosine_cohort_stats(xd, cd, k)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            print(f'N {n} run {rep}: host {t1 - t0:.4f} s, device {t2 - t1:.4f} s, kernels {t4 - t3:.4f} s', flush=True)
            if rep >= args.warmup:
                host_s.append(t1 - t0)
                dev_s.append(t2 - t1)
                kern_s.append(t4 - t3)
        lo, rec = _hip.cosine_cohort_stats_workspace_bytes(n, n)
        row = {'N': n, 'Nc': n, 'K': k, 'workspace_bytes': rec, 'min_workspace_bytes': lo,
               'row_blocks': -(-n // (rec // (4 * n))),
               'max_abs_diff_mean': float(np.abs(dev[0] - host[0]).max()),
               'max_abs_diff_std': float(np.abs(dev[1] - host[1]).max()),
               'host_s': host_s, 'device_s': dev_s, 'device_kernels_s': kern_s,
               'host_median_s': float(np.median(host_s)), 'device_median_s': float(np.median(dev_s)),
               'device_kernels_median_s': float(np.median(kern_s)),
               'speedup_median': float(np.median(host_s) / np.median(dev_s)),
               'device_faster_beyond_spread': max(dev_s) < min(host_s)}
        rows.append(row)
        write(rows)
        print(json.dumps({k_: v for k_, v in row.items() if not isinstance(v, list)}), flush=True)
        _hip.cohort_release_workspace()
        torch.cuda.empty_cache()
    return 0


if __name__ == '__main__':
    sys.exit(main())
