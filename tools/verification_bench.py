#!/usr/bin/env python
"""Times the all-pairs verification analysis (speakerlab/utils/verification_analysis.analyze_device)
on synthetic clustered embeddings, E = 192, 100 utterances per speaker:

  python tools/verification_bench.py [--sizes 20000,100000] [--repeats 2]
                                     [--out profiles/verification_bench.json]

Per N: seconds per pass of ``cosine_verif_moments`` (without and with a 256-bin histogram) and of
``cosine_verif_digits`` at level 0, at level 3 with 1 prefix and at level 3 with 16 prefixes; the
yardstick, one pass of ``cosine_triu_stats`` (moments only), measured in the same process on the same
input; then the whole analysis end to end with the passes its EER search and its branch and bound
needed, ``exact`` and the bound.  One warm-up run of every arm at the smallest N, then ``--repeats``
timed runs per arm with the device synchronised; the median is reported and every time is kept.
Needs a GPU; not a test."""
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
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--max_passes', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'verification_bench.json'))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from speakerlab import _hip
    from speakerlab.utils import verification_analysis as va
    if not torch.cuda.is_available():
        raise SystemExit('verification_bench needs a ROCm device')
    dev = torch.device('cuda')
    sizes = [int(s) for s in args.sizes.split(',') if s]
    result = {'e': 192, 'utterances_per_speaker': 100, 'device': torch.cuda.get_device_name(0),
              'max_passes': args.max_passes, 'repeats': args.repeats, 'runs': []}

    def data(n):
        rng = np.random.default_rng(n)
        speakers = (n + 99) // 100
        lab = (np.arange(n) // 100).astype(np.int32)
        x = rng.standard_normal((speakers, 192))[lab] + 1.5 * rng.standard_normal((n, 192))
        return torch.from_numpy(x.astype(np.float32)).to(dev), torch.from_numpy(lab).to(dev)

    def timed(fn):
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return {'median_s': statistics.median(times), 'times_s': times}, out

    def arms(x, lab):
        some = _hip.cosine_verif_digits(x, lab, 0, [0])
        top = int(np.argmax(some[0].sum(axis=0)))
        l1 = _hip.cosine_verif_digits(x, lab, 1, [top << 24])[0].sum(axis=0)
        order = np.argsort(-l1, kind='stable')[:16]
        l2 = [(top << 24) | (int(d) << 16) for d in order]
        l3 = []
        for pre, h in zip(l2, _hip.cosine_verif_digits(x, lab, 2, l2)):
            l3.append(pre | (int(np.argmax(h.sum(axis=0))) << 8))
        edges = np.linspace(-1.0, 1.0, 257)
        return {'triu_stats_one_pass': lambda: _hip.cosine_triu_stats(x),
                'verif_moments': lambda: _hip.cosine_verif_moments(x, lab),
                'verif_moments_hist256': lambda: _hip.cosine_verif_moments(x, lab, edges),
                'verif_digits_level0': lambda: _hip.cosine_verif_digits(x, lab, 0, [0]),
                'verif_digits_level3_1_prefix': lambda: _hip.cosine_verif_digits(x, lab, 3, l3[:1]),
                'verif_digits_level3_16_prefixes': lambda: _hip.cosine_verif_digits(x, lab, 3, l3)}

    x, lab = data(min(sizes))
    for fn in arms(x, lab).values():                               # warm-up: library load, workspace allocation
        fn()
    va.analyze_device(x, lab, max_passes=args.max_passes)
    for n in sizes:
        x, lab = data(n)
        run = {'n': n, 'pairs': n * (n - 1) // 2, 'per_pass': {}}
        for name, fn in arms(x, lab).items():
            run['per_pass'][name], _ = timed(fn)
        base = run['per_pass']['triu_stats_one_pass']['median_s']
        run['ratio_to_triu_stats'] = {k: v['median_s'] / base for k, v in run['per_pass'].items()}
        run['end_to_end'], rep = timed(lambda: va.analyze_device(x, lab, max_passes=args.max_passes))
        run['analysis'] = {'passes': rep['passes'], 'exact': bool(rep['exact']), 'eer': rep['eer'], 'min_dcf': rep['min_dcf'],
                           'min_dcf_bound': rep['min_dcf_bound'], 'auc': rep['auc'], 'auc_gap': rep['auc_gap'],
                           'n_tgt': rep['n_tgt'], 'n_non': rep['n_non']}
        lo, rec, st = _hip.cosine_verif_workspace_bytes(n)
        run.update(workspace_bytes=rec, state_bytes=st)
        result['runs'].append(run)
        print(json.dumps(run), flush=True)
        _hip.verif_release_workspace()
        _hip.sim_release_workspace()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
