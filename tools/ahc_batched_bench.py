#!/usr/bin/env python
"""Three AHC paths on the same device-resident cosine affinities, interleaved in one process:
the host (scipy linkage + fcluster, the default), the device AHC with three launches per merge
(spk_ahc_average) and the batched single-launch AHC (spk_ahc_average_batched, one workgroup per
problem).

  python tools/ahc_batched_bench.py [--sizes 300,1200,2000,cap] [--batch 16x600]
                                    [--out profiles/ahc_batched_bench.json]

Setting 1: one problem per call at every N of ``--sizes`` (``cap``: the batched path's largest N).
Setting 2: ``--batch`` BxN, B problems of N rows; the host and the three-launch arms cluster them
one after the other, the batched arm with one call.  Synthetic 4- to 8-speaker embeddings
(E = 192) as tools/ahc_bench.py, fix_cos_thr 0.3.  The host arm includes the device-to-host copy
it needs and runs on ``--threads`` threads; the device arms bring the labels back to the host.
Median of ``--repeats`` after ``--warmup`` runs of each arm, every time kept in the output."""
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
    ap.add_argument('--sizes', default='300,1200,2000,cap')
    ap.add_argument('--batch', default='16x600')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--thr', type=float, default=0.3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ahc_batched_bench.json'))
    args = ap.parse_args(argv)

    os.environ.setdefault('OMP_NUM_THREADS', str(args.threads))
    import numpy as np
    import torch
    from speakerlab import _hip
    from speakerlab.process import cluster as C
    torch.set_num_threads(args.threads)
    assert torch.cuda.is_available(), 'ahc_batched_bench needs a ROCm device'
    cap = _hip.ahc_batched_max_n()

    def affinity(n, idx):
        spk = (4, 6, 8, 5, 7)[idx % 5]
        rng = np.random.default_rng(n + 1000 * (idx // 5))
        cen = rng.standard_normal((spk, 192))
        cen /= np.linalg.norm(cen, axis=1, keepdims=True)
        X = (cen[rng.integers(0, spk, n)] + 0.05 * rng.standard_normal((n, 192))).astype(np.float32)
        return _hip.cosine_affinity(torch.from_numpy(X).cuda())

    def write(rows):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'threshold': args.thr, 'repeats': args.repeats,
                       'warmup': args.warmup, 'host_threads': args.threads, 'batched_cap': cap, 'rows': rows}, f,
                      indent=1)
            f.write('\n')

    cases = [('single', [cap if v == 'cap' else int(v)]) for v in args.sizes.split(',') if v]
    if args.batch:
        b, n = args.batch.split('x')
        cases.append(('batch', [int(n)] * int(b)))
    rows = []
    for ci, (setting, sizes) in enumerate(cases):
        mats = [affinity(n, ci + idx) for idx, n in enumerate(sizes)]
        torch.cuda.synchronize()
        times = {'host': [], 'device': [], 'batched': []}
        labels = {}
        for rep in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            labels['host'] = [C.ahc_labels(S.cpu().numpy(), args.thr) for S in mats]
            t1 = time.perf_counter()
            labels['device'] = [C.ahc_labels_gpu(S, args.thr) for S in mats]
            t2 = time.perf_counter()
            labels['batched'] = C.ahc_labels_gpu_batched(mats, args.thr)
            t3 = time.perf_counter()
            print(f'{setting} {len(sizes)} x N {sizes[0]} run {rep}: host {t1 - t0:.4f} s, device {t2 - t1:.4f} s, '
                  f'batched {t3 - t2:.4f} s', flush=True)
            if rep >= args.warmup:
                for arm, dt in (('host', t1 - t0), ('device', t2 - t1), ('batched', t3 - t2)):
                    times[arm].append(dt)
        merges = sum(n - (int(lab.max()) + 1) for n, lab in zip(sizes, labels['batched']))
        med = {arm: float(np.median(v)) for arm, v in times.items()}
        row = {'setting': setting, 'problems': len(sizes), 'N': sizes[0],
               'clusters': [int(lab.max()) + 1 for lab in labels['batched']], 'merge_steps': merges,
               'batched_launches': 2, 'workspace_bytes': sum(8 * n * n for n in sizes),
               'same_partition_as_host': all(canon(h) == b.tolist() for h, b in zip(labels['host'], labels['batched'])),
               'same_labels_as_device': all(d.tolist() == b.tolist() for d, b in zip(labels['device'], labels['batched'])),
               'host_s': times['host'], 'device_s': times['device'], 'batched_s': times['batched'],
               'host_median_s': med['host'], 'device_median_s': med['device'], 'batched_median_s': med['batched'],
               # the longest problem of a batch bounds its launch: steps of ONE problem for a batch
               'batched_us_per_step': 1e6 * med['batched'] / max(1, merges // len(sizes)),
               'device_us_per_step': 1e6 * med['device'] / max(1, merges),
               'host_over_batched': med['host'] / med['batched'], 'device_over_batched': med['device'] / med['batched'],
               'batched_faster_than_host_beyond_spread': max(times['batched']) < min(times['host']),
               'batched_faster_than_device_beyond_spread': max(times['batched']) < min(times['device'])}
        rows.append(row)
        write(rows)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith('_s') or 'median' in k}), flush=True)
        _hip.ahc_release_workspace()
        del mats
        torch.cuda.empty_cache()
    return 0


if __name__ == '__main__':
    sys.exit(main())
