#!/usr/bin/env python
"""Host AHC (scipy linkage + fcluster, the default) vs the device AHC (spk_ahc_average) on the
same device-resident cosine affinity, interleaved in one process.

  python tools/ahc_bench.py [--sizes 1200,4800,19200] [--out profiles/ahc_bench.json]

For every N (20 min, 1 h and 4 h of 0.75 s hops) synthetic 4- to 8-speaker embeddings (E = 192)
are clustered at fix_cos_thr 0.3.  The host arm is ``ahc_labels(S.cpu().numpy(), thr)`` -- it
includes the device-to-host copy it needs -- on ``--threads`` threads; the device arm is
``ahc_labels_gpu(S, thr)``, labels back on the host.  Median of ``--repeats`` after ``--warmup``
runs of each arm, every time kept in the output, with the merge steps, the launches per step and
the workspace."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, '3d-speaker_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def canon(labels):
    m = {}
    return [m.setdefault(int(v), len(m)) for v in labels]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='1200,4800,19200')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--thr', type=float, default=0.3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ahc_bench.json'))
    args = ap.parse_args(argv)

    os.environ.setdefault('OMP_NUM_THREADS', str(args.threads))
    import numpy as np
    import torch
    from speakerlab import _hip
    from speakerlab.process import cluster as C
    torch.set_num_threads(args.threads)
    assert torch.cuda.is_available(), 'ahc_bench needs a ROCm device'

    def write(rows):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'threshold': args.thr, 'repeats': args.repeats,
                       'warmup': args.warmup, 'host_threads': args.threads, 'launches_per_step': 3,
                       'steps_per_host_read': 256, 'rows': rows}, f, indent=1)
            f.write('\n')

    rows = []
    for idx, n in enumerate(int(v) for v in args.sizes.split(',')):
        spk = (4, 6, 8, 5, 7)[idx % 5]
        rng = np.random.default_rng(n)
        cen = rng.standard_normal((spk, 192))
        cen /= np.linalg.norm(cen, axis=1, keepdims=True)
        X = (cen[rng.integers(0, spk, n)] + 0.05 * rng.standard_normal((n, 192))).astype(np.float32)
        S = _hip.cosine_affinity(torch.from_numpy(X).cuda())
        torch.cuda.synchronize()
        host_s, gpu_s, host_lab, gpu_lab = [], [], None, None
        for rep in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            host_lab = C.ahc_labels(S.cpu().numpy(), args.thr)
            t1 = time.perf_counter()
            gpu_lab = C.ahc_labels_gpu(S, args.thr)
            t2 = time.perf_counter()
            print(f'N {n} run {rep}: host {t1 - t0:.4f} s, device {t2 - t1:.4f} s', flush=True)
            if rep >= args.warmup:
                host_s.append(t1 - t0)
                gpu_s.append(t2 - t1)
        clusters = int(gpu_lab.max()) + 1
        merges = n - clusters
        # steps go out 256 at a time, N - 1 at most; the select after the last merge ends the loop
        enqueued = min(n - 1, -(-(merges + 1) // 256) * 256)
        row = {'N': n, 'speakers': spk, 'clusters': clusters, 'merge_steps': merges,
               'launches_enqueued': 3 * enqueued + 4,      # + convert, state, first repair, labels
               'workspace_bytes': _hip.ahc_workspace_bytes(n),
               'same_partition': canon(host_lab) == gpu_lab.tolist(),
               'host_s': host_s, 'device_s': gpu_s,
               'host_median_s': float(np.median(host_s)), 'device_median_s': float(np.median(gpu_s)),
               'speedup_median': float(np.median(host_s) / np.median(gpu_s)),
               'device_faster_beyond_spread': max(gpu_s) < min(host_s)}
        rows.append(row)
        write(rows)
        print(json.dumps({k: v for k, v in row.items() if k not in ('host_s', 'device_s')}), flush=True)
        _hip.ahc_release_workspace()
        del S
        torch.cuda.empty_cache()
    return 0


if __name__ == '__main__':
    sys.exit(main())
