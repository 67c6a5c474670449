"""Utterance-level speaker verification analysis of a corpus of embeddings: the workflow, the flags and
the output files of the reference's
egs/mix_adult_kid/sv-eres2netv2/compute_utterance_similarities_analysis.py.

The scan (``<utterances>/<dataset>/<speaker>/*.pkl``, pickles holding ``{'embedding': array}``,
utterances with NaN / Inf dropped) and the reports stay on the host.  Directory entries are SORTED
(data sets, speakers, files), so a run is reproducible; the reference takes them in file-system order.

``--pairs sampled`` (default) is the reference protocol: every target pair and twice as many randomly
drawn non-target pairs (``random.seed(42)``, the reference's call sequence, so the same utterance
order gives the same pair list), scored on the device by ``_hip.cosine_trials`` and stored as
``cosine - 1`` as the reference stores them, with the reference's formulas for EER (brentq over the
interpolated ROC), minDCF and AUC.

``--pairs all`` scores every one of the N (N - 1) / 2 pairs with the class-aware HIP kernels
(speakerlab/utils/verification_analysis.py): EER and minDCF exact on the device's own float32 scores,
AUC bracketed by a 256-bin histogram, the N x N matrix never stored.  Thresholds are on the
reference's ``cosine - 1`` scale, ``eer_threshold_cosine`` is the cosine itself; ``fpr`` / ``tpr`` /
``thresholds`` are the 256-bin curve; ``y_true`` / ``y_scores`` are omitted.

Only the ``cosine`` metric exists here; ``--memory_efficient`` and ``--chunk_size`` are accepted and
ignored, since nothing is ever materialised.
"""
import argparse
import json
import logging
import multiprocessing as mp
import os
import pickle
import random
import sys
import time
from collections import defaultdict
from concurrent.futures import ProcessPoolExecutor

import numpy as np

from speakerlab.utils import verification_analysis as va

log = logging.getLogger('compute_utterance_similarities')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Utterance-level speaker similarity analysis')
    p.add_argument('--embeddings_dir', type=str, required=True, help='Base embeddings directory')
    p.add_argument('--utterances_subdir', type=str, default='embeddings_individual/utterances',
                   help='Subdirectory containing utterance embeddings')
    p.add_argument('--output_dir', type=str, default='utterance_analysis', help='Output directory for analysis results')
    p.add_argument('--num_workers', type=int, default=min(16, mp.cpu_count()), help='Number of worker processes')
    p.add_argument('--max_speakers', type=int, default=None, help='Maximum number of speakers to process')
    p.add_argument('--max_utterances_per_speaker', type=int, default=100, help='Maximum utterances per speaker to use')
    p.add_argument('--distance_metrics', nargs='+', default=['cosine'], help='Distance metrics to compute (cosine only)')
    p.add_argument('--plot_format', type=str, default='png', choices=['png', 'pdf', 'svg'], help='Output format for plots')
    p.add_argument('--dpi', type=int, default=300, help='DPI for saved plots')
    p.add_argument('--memory_efficient', action='store_true', help='Accepted and ignored: nothing is materialised')
    p.add_argument('--chunk_size', type=int, default=5000, help='Accepted and ignored')
    p.add_argument('--pairs', choices=['sampled', 'all'], default='sampled',
                   help='sampled: the reference protocol (all target pairs, 2x random non-target pairs); '
                        'all: every pair, exact EER / minDCF on the device')
    p.add_argument('--no_plot', action='store_true', help='Skip the plots')
    args = p.parse_args(argv)
    for m in args.distance_metrics:
        if m != 'cosine':
            p.error(f"--distance_metrics: only 'cosine' is supported here, got '{m}'")
    if args.num_workers < 1 or args.max_utterances_per_speaker < 1:
        p.error('--num_workers and --max_utterances_per_speaker must be at least 1')
    return args


def scan_utterance_files(utterances_dir, max_speakers=None, max_utterances_per_speaker=100):
    """speaker_key -> utterance records; data sets, speakers and files in sorted order."""
    found, n = defaultdict(list), 0
    for dataset in sorted(os.listdir(utterances_dir)):
        ddir = os.path.join(utterances_dir, dataset)
        if not os.path.isdir(ddir):
            continue
        for speaker in sorted(os.listdir(ddir)):
            sdir = os.path.join(ddir, speaker)
            if not os.path.isdir(sdir):
                continue
            if max_speakers and n >= max_speakers:
                break
            key = f'{dataset}_{speaker}'
            for name in sorted(f for f in os.listdir(sdir) if f.endswith('.pkl'))[:max_utterances_per_speaker]:
                found[key].append({'file_path': os.path.join(sdir, name), 'dataset': dataset, 'speaker_id': speaker,
                                   'speaker_key': key, 'utterance_id': name[:-4]})
            n += 1
        if max_speakers and n >= max_speakers:
            break
    return found


def load_batch(batch):
    out = []
    for u in batch:
        try:
            with open(u['file_path'], 'rb') as f:
                e = pickle.load(f).get('embedding')
            e = None if e is None else np.asarray(e, dtype=np.float32).reshape(-1)
        except Exception:
            continue                                                # an unreadable file is skipped
        if e is not None and np.isfinite(e).all():
            out.append(dict(u, embedding=e))
    return out


def load_utterances(found, num_workers):
    """All valid utterances in the order of the scan, whatever order the workers finish in."""
    todo = [u for utts in found.values() for u in utts]
    size = max(1, len(todo) // (num_workers * 4))
    batches = [todo[i:i + size] for i in range(0, len(todo), size)]
    if num_workers <= 1 or len(batches) <= 1:
        return [u for b in batches for u in load_batch(b)]
    with ProcessPoolExecutor(max_workers=num_workers) as pool:
        return [u for res in pool.map(load_batch, batches) for u in res]


def generate_speaker_pairs(speaker_keys):
    """The reference's pair list for utterances with these speaker keys, in their order: every target
    pair, twice as many random non-target pairs, shuffled; (i, j, label) tuples."""
    groups = defaultdict(list)
    for i, k in enumerate(speaker_keys):
        groups[k].append(i)
    positive = []
    for idx in groups.values():
        for a in range(len(idx)):
            for b in range(a + 1, len(idx)):
                positive.append((idx[a], idx[b], 1))
    keys = list(groups)
    if positive and len(keys) < 2:
        raise ValueError('sampled pairs need at least two speakers')
    random.seed(42)
    negative = []
    while len(negative) < 2 * len(positive):
        s1, s2 = random.sample(keys, 2)
        negative.append((random.choice(groups[s1]), random.choice(groups[s2]), 0))
    pairs = positive + negative
    random.shuffle(pairs)
    return pairs


def sampled_metrics(y_true, y_scores):
    """The reference's formulas on its stored scores (``cosine - 1``)."""
    from scipy.interpolate import interp1d
    from scipy.optimize import brentq
    from sklearn.metrics import auc, roc_curve
    y_true, y_scores = np.asarray(y_true), np.asarray(y_scores, dtype=np.float64)
    if y_true.min() == y_true.max():
        raise ValueError('verification metrics need target and non-target pairs')
    fpr, tpr, thresholds = roc_curve(y_true, y_scores)
    eer_threshold = brentq(lambda x: 1. - x - interp1d(fpr, tpr)(x), 0., 1.)
    eer = 1. - interp1d(fpr, tpr)(eer_threshold)
    min_dcf = np.min(1 * (1 - tpr) * 0.01 + 1 * fpr * (1 - 0.01))
    return {'metric': 'cosine', 'eer': float(eer), 'eer_threshold': float(eer_threshold), 'min_dcf': float(min_dcf),
            'auc': float(auc(fpr, tpr)), 'fpr': fpr.tolist(), 'tpr': tpr.tolist(), 'thresholds': thresholds.tolist(),
            'y_true': y_true.tolist(), 'y_scores': y_scores.tolist()}


def evaluate_sampled(X, speaker_keys, device):
    import torch
    from speakerlab import _hip
    pairs = generate_speaker_pairs(speaker_keys)
    if not pairs:
        raise ValueError('verification metrics need target and non-target pairs')
    arr = np.asarray(pairs, dtype=np.int64)
    x = torch.as_tensor(X).to(device)
    cos = _hip.cosine_trials(x, x, torch.as_tensor(arr[:, 0]), torch.as_tensor(arr[:, 1])).cpu().numpy()
    res = sampled_metrics(arr[:, 2], cos.astype(np.float64) - 1.0)
    res['pairs'] = 'sampled'
    return res


def evaluate_all(X, speaker_keys, device):
    import torch
    index = {}
    labels = np.array([index.setdefault(k, len(index)) for k in speaker_keys], np.int32)
    rep = va.analyze_device(torch.as_tensor(X).to(device), torch.as_tensor(labels).to(device))
    return all_pairs_result(rep)


def all_pairs_result(rep):
    """The evaluation_results JSON of ``--pairs all`` from ``verification_analysis.analyze``'s report."""
    thr = rep['thresholds'] - 1.0
    thr[0] = np.inf
    m = rep['moments']
    cls = lambda a, f: {'non_target': f(a[0]), 'target': f(a[1])}
    return {'metric': 'cosine', 'pairs': 'all', 'eer': float(rep['eer']),
            'eer_threshold': rep['eer_threshold_cosine'] - 1.0, 'eer_threshold_cosine': rep['eer_threshold_cosine'],
            'min_dcf': float(rep['min_dcf']), 'auc': float(rep['auc']),
            'fpr': rep['fpr'].tolist(), 'tpr': rep['tpr'].tolist(), 'thresholds': [float(t) for t in thr],
            'exact': bool(rep['exact']), 'min_dcf_bound': float(rep['min_dcf_bound']),
            'min_dcf_point': {k: (float(v) if isinstance(v, float) else int(v)) for k, v in rep['min_dcf_point'].items()},
            'min_dcf_threshold': rep['min_dcf_point']['threshold_cosine'] - 1.0,
            'eer_counts': rep['eer_counts'], 'n_target_pairs': rep['n_tgt'], 'n_non_target_pairs': rep['n_non'],
            'auc_lo': rep['auc_lo'], 'auc_hi': rep['auc_hi'], 'auc_gap': rep['auc_gap'], 'passes': rep['passes'],
            'moments': {'count': cls(m['count'], int), 'mean': cls(m['mean'], float), 'std': cls(m['std'], float),
                        'min': cls(m['min'], float), 'max': cls(m['max'], float)},
            'histogram': {'edges': rep['edges'].tolist(), 'non_target': rep['hist'][0].tolist(),
                          'target': rep['hist'][1].tolist()}}


def speaker_statistics(utterances):
    counts, per_set, set_speakers = defaultdict(int), defaultdict(int), defaultdict(set)
    for u in utterances:
        counts[u['speaker_key']] += 1
        per_set[u['dataset']] += 1
        set_speakers[u['dataset']].add(u['speaker_key'])
    c = list(counts.values())
    return {'total_speakers': len(counts), 'total_utterances': len(utterances),
            'avg_utterances_per_speaker': float(np.mean(c)), 'std_utterances_per_speaker': float(np.std(c)),
            'min_utterances_per_speaker': int(min(c)), 'max_utterances_per_speaker': int(max(c)),
            'datasets': {d: {'utterances': n, 'speakers': len(set_speakers[d])} for d, n in per_set.items()}}


def _dump(out_dir, name, obj):
    with open(os.path.join(out_dir, name + '.json'), 'w', encoding='utf-8') as f:
        json.dump(obj, f, indent=2, ensure_ascii=False)


def markdown_report(report, fmt):
    a, s = report['analysis_summary'], report['speaker_statistics']
    md = (f"# Speaker Verification Analysis Report\n\n## Analysis Summary\n- **Analysis Time**: {a['timestamp']}\n"
          f"- **Total Speakers**: {a['total_speakers']:,}\n- **Total Utterances**: {a['total_utterances']:,}\n"
          f"- **Datasets Analyzed**: {a['datasets_analyzed']}\n- **Pairs**: {a['pairs']}\n\n## Speaker Statistics\n"
          f"- **Average Utterances per Speaker**: {s['avg_utterances_per_speaker']:.2f}\n"
          f"- **Standard Deviation**: {s['std_utterances_per_speaker']:.2f}\n"
          f"- **Min Utterances per Speaker**: {s['min_utterances_per_speaker']}\n"
          f"- **Max Utterances per Speaker**: {s['max_utterances_per_speaker']}\n\n## Dataset Distribution\n")
    for d, info in s['datasets'].items():
        md += f"- **{d}**: {info['utterances']:,} utterances, {info['speakers']:,} speakers\n"
    md += '\n## Verification Results\n\n| Metric | EER | EER Threshold | minDCF | AUC |\n|--------|-----|---------------|--------|-----|\n'
    for metric, r in report['verification_results'].items():
        md += f"| {metric} | {r['eer']:.4f} | {r['eer_threshold']:.4f} | {r['min_dcf']:.4f} | {r['auc']:.4f} |\n"
        if 'auc_gap' in r:
            md += (f"\nAll {r['n_target_pairs'] + r['n_non_target_pairs']:,} pairs were scored "
                   f"({r['n_target_pairs']:,} target, {r['n_non_target_pairs']:,} non-target).  EER is exact; minDCF is "
                   f"{'exact' if r['exact'] else 'NOT exact: the pass budget ran out, lower bound ' + format(r['min_dcf_bound'], '.6f')}"
                   f"; AUC lies in [{r['auc_lo']:.6f}, {r['auc_hi']:.6f}] (gap {r['auc_gap']:.2e}, the pairs "
                   f"that share a histogram bin).  Passes over the pairs: {r['passes']['total']}.\n")
    md += ('\n## Files Generated\n' + ''.join(f'- `{n}.{fmt}`\n' for n in ('roc_curves', 'det_curves', 'score_distribution_cosine',
                                                                          'dataset_distribution', 'speakers_by_dataset'))
           + '- `analysis_report.json` - Detailed analysis results\n')
    return md


def make_plots(result, stats, out_dir, fmt, dpi):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from scipy import stats as sst

    def save(name):
        plt.tight_layout()
        plt.savefig(os.path.join(out_dir, f'{name}.{fmt}'), format=fmt, dpi=dpi, bbox_inches='tight')
        plt.close()
    fpr, tpr = np.asarray(result['fpr']), np.asarray(result['tpr'])
    plt.figure(figsize=(10, 8))
    plt.plot(fpr, tpr, label=f"cosine (AUC = {result['auc']:.3f})", linewidth=2)
    plt.plot([0, 1], [0, 1], 'k--', alpha=0.5, label='Random')
    plt.xlabel('False Positive Rate'); plt.ylabel('True Positive Rate'); plt.title('ROC Curves for Speaker Verification')
    plt.legend(loc='lower right'); plt.grid(True, alpha=0.3)
    save('roc_curves')
    plt.figure(figsize=(10, 8))
    plt.plot(sst.norm.ppf(np.clip(fpr, 1e-8, 1 - 1e-8)), sst.norm.ppf(np.clip(1 - tpr, 1e-8, 1 - 1e-8)),
             label=f"cosine (EER = {result['eer']:.3f})", linewidth=2)
    ticks = [0.1, 0.2, 0.5, 1, 2, 5, 10, 20, 40]
    loc = sst.norm.ppf(np.array(ticks) / 100)
    plt.xticks(loc, ticks); plt.yticks(loc, ticks)
    plt.xlabel('False Positive Rate (%)'); plt.ylabel('False Negative Rate (%)'); plt.title('DET Curves for Speaker Verification')
    plt.legend(); plt.grid(True, alpha=0.3)
    save('det_curves')
    plt.figure(figsize=(12, 6))
    if 'y_scores' in result:
        y, s = np.asarray(result['y_true']), np.asarray(result['y_scores'])
        plt.hist(s[y == 0], bins=50, alpha=0.7, label='Different Speakers', color='red', density=True)
        plt.hist(s[y == 1], bins=50, alpha=0.7, label='Same Speaker', color='blue', density=True)
    else:
        e = np.asarray(result['histogram']['edges']) - 1.0
        for name, label, color in (('non_target', 'Different Speakers', 'red'), ('target', 'Same Speaker', 'blue')):
            h = np.asarray(result['histogram'][name], np.float64)
            plt.stairs(h / max(h.sum(), 1) / np.diff(e), e, fill=True, alpha=0.7, label=label, color=color)
    plt.axvline(x=result['eer_threshold'], color='green', linestyle='--', label=f"EER Threshold ({result['eer_threshold']:.3f})")
    plt.xlabel('Similarity Score'); plt.ylabel('Density'); plt.title('Score Distribution - cosine')
    plt.legend(); plt.grid(True, alpha=0.3)
    save('score_distribution_cosine')
    sets = list(stats['datasets'])
    plt.figure(figsize=(10, 8))
    plt.pie([stats['datasets'][d]['utterances'] for d in sets], labels=sets, autopct='%1.1f%%', startangle=90)
    plt.title('Distribution of Utterances by Dataset'); plt.axis('equal')
    save('dataset_distribution')
    plt.figure(figsize=(12, 6))
    plt.bar(sets, [stats['datasets'][d]['speakers'] for d in sets], color='skyblue', alpha=0.7)
    plt.xlabel('Dataset'); plt.ylabel('Number of Speakers'); plt.title('Number of Speakers by Dataset')
    plt.xticks(rotation=45); plt.grid(True, alpha=0.3)
    save('speakers_by_dataset')


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(levelname)s - %(message)s')
    t0 = time.time()
    utt_dir = os.path.join(args.embeddings_dir, args.utterances_subdir)
    out_dir = os.path.join(args.embeddings_dir, args.output_dir)
    if not os.path.isdir(utt_dir):
        raise SystemExit(f'Utterances directory not found: {utt_dir}')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('compute_utterance_similarities needs a ROCm device')
    device = torch.device('cuda')
    if args.memory_efficient:
        log.info('--memory_efficient / --chunk_size are ignored: no distance matrix is ever stored')

    log.info('=== Stage 1: Scanning utterance files ===')
    found = scan_utterance_files(utt_dir, args.max_speakers, args.max_utterances_per_speaker)
    if not found:
        raise SystemExit('No utterances found')
    log.info('=== Stage 2: Loading utterance embeddings ===')
    utterances = load_utterances(found, args.num_workers)
    if not utterances:
        raise SystemExit('No valid utterances loaded')
    dims = {len(u['embedding']) for u in utterances}
    if len(dims) != 1:
        raise SystemExit(f'Utterance embeddings have different sizes: {sorted(dims)}')
    os.makedirs(out_dir, exist_ok=True)
    log.info('=== Stage 3: Analyzing speaker statistics ===')
    stats = speaker_statistics(utterances)
    _dump(out_dir, 'speaker_statistics', stats)
    log.info('=== Stage 4-5: Scoring %s pairs of %d utterances ===', args.pairs, len(utterances))
    X = np.stack([u['embedding'] for u in utterances]).astype(np.float32)
    keys = [u['speaker_key'] for u in utterances]
    try:
        result = (evaluate_all if args.pairs == 'all' else evaluate_sampled)(X, keys, device)
    except ValueError as e:
        raise SystemExit(str(e))
    _dump(out_dir, 'evaluation_results_cosine', result)
    if not args.no_plot:
        log.info('=== Stage 6: Generating visualizations ===')
        make_plots(result, stats, out_dir, args.plot_format, args.dpi)
    log.info('=== Stage 7: Generating analysis report ===')
    summary = {k: result[k] for k in ('eer', 'eer_threshold', 'min_dcf', 'auc')}
    if args.pairs == 'all':
        summary.update({k: result[k] for k in ('eer_threshold_cosine', 'exact', 'min_dcf_bound', 'auc_lo', 'auc_hi', 'auc_gap',
                                               'n_target_pairs', 'n_non_target_pairs', 'passes', 'moments')})
    report = {'analysis_summary': {'timestamp': time.strftime('%Y-%m-%d %H:%M:%S'), 'total_speakers': stats['total_speakers'],
                                   'total_utterances': stats['total_utterances'], 'datasets_analyzed': len(stats['datasets']),
                                   'pairs': args.pairs},
              'speaker_statistics': stats, 'verification_results': {'cosine': summary}}
    _dump(out_dir, 'analysis_report', report)
    with open(os.path.join(out_dir, 'analysis_report.md'), 'w', encoding='utf-8') as f:
        f.write(markdown_report(report, args.plot_format))
    bar = '=' * 80
    print(f"\n{bar}\nUTTERANCE-LEVEL ANALYSIS COMPLETED\n{bar}\nTotal processing time: {time.time() - t0:.2f} seconds\n"
          f"Results saved to: {out_dir}\n\nVerification Results ({args.pairs} pairs):\n"
          f"  {'cosine':>10}: EER={result['eer']:.4f}, minDCF={result['min_dcf']:.4f}, AUC={result['auc']:.4f}\n{bar}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
