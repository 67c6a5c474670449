"""Speaker embeddings of a corpus and their similarity analysis: the workflow and the output files of
the reference's egs/extract_and_comclude_similarities/compute_speaker_similarities_fast.py.

Stages 1-3 are file I/O and stay on the host: scan ``<utterances>/<dataset>/<speaker>/*.pkl``
(pickles holding ``{'embedding': array}``), drop utterances with NaN / Inf, average each speaker's
embeddings in float32, write ``<speakers>/<dataset>/<speaker>.pkl`` and ``<speaker>_info.json``.
The analysis of the speaker x speaker cosine matrix runs on the device without ever storing the
matrix (speakerlab/utils/similarity_analysis.py); ``--device host`` runs its numpy statement instead.
The three outputs whose size is O(N^2) -- ``speaker_similarities.json``, ``similarity_matrix.npy``,
``upper_triangular_similarities.npy`` -- are written only with ``--save_matrix``.
"""
import argparse
import json
import logging
import multiprocessing as mp
import os
import pickle
import sys
import time
from concurrent.futures import ProcessPoolExecutor, as_completed

import numpy as np

from speakerlab.utils import similarity_analysis as sa

SAVE_MATRIX_MAX = 32768
PROGRESS_FILE = 'processing_progress.json'
ANALYSIS_FILES = ('upper_triangular_statistics', 'extreme_similarity_pairs', 'speaker_top_similarities',
                  'similarity_distribution', 'threshold_statistics', 'analysis_summary')
log = logging.getLogger('compute_speaker_similarities')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Speaker embeddings of a corpus and their similarity analysis')
    p.add_argument('--embeddings_dir', type=str, required=True, help='Base embeddings directory')
    p.add_argument('--utterances_subdir', type=str, default='embeddings_individual/utterances',
                   help='Subdirectory containing utterance embeddings')
    p.add_argument('--speakers_output_subdir', type=str, default='embeddings_individual/speakers',
                   help='Subdirectory for speaker output')
    p.add_argument('--similarities_output_subdir', type=str, default='speaker_similarity_analysis',
                   help='Subdirectory for similarity results')
    p.add_argument('--num_workers', type=int, default=min(32, mp.cpu_count()), help='Number of worker processes')
    p.add_argument('--batch_size', type=int, default=100, help='Batch size for processing speakers')
    p.add_argument('--resume', action='store_true', help='Resume from previous progress')
    p.add_argument('--max_speakers', type=int, default=None, help='Maximum number of speakers to process')
    p.add_argument('--skip_similarity', action='store_true', help='Only process speaker embeddings')
    p.add_argument('--top_k', type=int, default=100, help='Number of top similar speakers per speaker')
    p.add_argument('--n_extreme', type=int, default=1000, help='Number of most / least similar pairs to report')
    p.add_argument('--save_matrix', action='store_true',
                   help=f'Also write the O(N^2) outputs (at most {SAVE_MATRIX_MAX} speakers)')
    p.add_argument('--device', choices=['cuda', 'host'], default='cuda',
                   help='cuda: the HIP kernels; host: the numpy statement of the same analysis')
    args = p.parse_args(argv)
    if args.top_k < 1 or args.n_extreme < 0 or args.batch_size < 1 or args.num_workers < 1:
        p.error('--top_k, --batch_size and --num_workers must be at least 1, --n_extreme at least 0')
    return args


def scan_utterances(utterances_dir, max_speakers=None):
    """speaker -> list of utterance records, datasets and speakers in sorted order."""
    found, n = {}, 0
    for dataset in sorted(os.listdir(utterances_dir)):
        ddir = os.path.join(utterances_dir, dataset)
        if not os.path.isdir(ddir):
            continue
        for speaker in sorted(os.listdir(ddir)):
            sdir = os.path.join(ddir, speaker)
            if not os.path.isdir(sdir):
                continue
            if max_speakers and n >= max_speakers:
                return found
            for name in sorted(os.listdir(sdir)):
                if name.endswith('.pkl'):
                    found.setdefault(speaker, []).append({'file_path': os.path.join(sdir, name), 'dataset': dataset,
                                                          'speaker_id': speaker, 'utterance_id': name[:-4]})
            n += 1
    return found


def _finite(a):
    return bool(np.isfinite(a).all())


def average_batch(batch):
    """(embeddings, info) of a batch of (speaker, utterance records): the float32 mean of the valid ones."""
    embeddings, info = {}, {}
    for speaker, utts in batch:
        good, kept = [], []
        for u in utts:
            try:
                with open(u['file_path'], 'rb') as f:
                    e = pickle.load(f).get('embedding')
                e = None if e is None else np.asarray(e, dtype=np.float32).reshape(-1)
            except Exception:
                continue                                            # an unreadable file is skipped
            if e is None:
                continue
            if not _finite(e):
                log.warning('Utterance %s has an invalid embedding (NaN/Inf), skipping', u['utterance_id'])
                continue
            good.append(e)
            kept.append(u)
        if not good or len({len(e) for e in good}) != 1:
            continue
        avg = np.mean(np.stack(good), axis=0, dtype=np.float32)
        if not _finite(avg):
            continue
        embeddings[speaker] = avg
        info[speaker] = {'dataset': utts[0]['dataset'], 'speaker_id': utts[0]['speaker_id'], 'speaker_key': speaker,
                         'num_utterances': len(kept), 'embedding_dim': int(len(avg)),
                         'utterances': [{'utterance_id': u['utterance_id'], 'file_path': u['file_path']}
                                        for u in kept[:10]]}
    return embeddings, info


def save_progress(embeddings, info, path):
    with open(path, 'w') as f:
        json.dump({'speaker_embeddings': {k: v.tolist() for k, v in embeddings.items()}, 'speaker_info': info,
                   'processed_speakers': list(embeddings)}, f)


def load_progress(path):
    try:
        with open(path) as f:
            d = json.load(f)
        return ({k: np.asarray(v, dtype=np.float32) for k, v in d['speaker_embeddings'].items()}, d['speaker_info'],
                set(d['processed_speakers']))
    except Exception:
        return {}, {}, set()


def speaker_embeddings(found, num_workers, batch_size, progress_file=None):
    embeddings, info, done = {}, {}, set()
    if progress_file and os.path.exists(progress_file):
        embeddings, info, done = load_progress(progress_file)
        log.info('Resumed from progress: %d speakers already processed', len(done))
    todo = [(k, v) for k, v in found.items() if k not in done]
    batches = [todo[i:i + batch_size] for i in range(0, len(todo), batch_size)]

    def take(n_done, result):
        embeddings.update(result[0])
        info.update(result[1])
        if progress_file and n_done % 10 == 0:
            save_progress(embeddings, info, progress_file)

    if num_workers <= 1 or len(batches) <= 1:
        for n, b in enumerate(batches, 1):
            take(n, average_batch(b))
    else:
        with ProcessPoolExecutor(max_workers=num_workers) as pool:
            for n, fut in enumerate(as_completed([pool.submit(average_batch, b) for b in batches]), 1):
                take(n, fut.result())
    if progress_file:
        save_progress(embeddings, info, progress_file)
    # the order of the scan, whatever order the batches finished in
    order = [k for k in found if k in embeddings] + [k for k in embeddings if k not in found]
    return {k: embeddings[k] for k in order}, info


def save_speaker_files(embeddings, info, out_dir):
    for speaker, emb in embeddings.items():
        ddir = os.path.join(out_dir, info[speaker]['dataset'])
        os.makedirs(ddir, exist_ok=True)
        with open(os.path.join(ddir, f"{info[speaker]['speaker_id']}.pkl"), 'wb') as f:
            pickle.dump({'embedding': emb, 'info': info[speaker]}, f)
        with open(os.path.join(ddir, f"{info[speaker]['speaker_id']}_info.json"), 'w', encoding='utf-8') as f:
            json.dump(info[speaker], f, indent=2, ensure_ascii=False)


def _dump(out_dir, name, obj):
    with open(os.path.join(out_dir, name + '.json'), 'w', encoding='utf-8') as f:
        json.dump(obj, f, indent=2, ensure_ascii=False)


def save_matrix(X, keys, out_dir, device):
    """The O(N^2) outputs, through spk_cosine_affinity on the device."""
    if device is None:
        S = sa.host_cosine(X)
    else:
        import torch
        from speakerlab import _hip
        S = _hip.cosine_affinity(torch.as_tensor(X).to(device)).cpu().numpy()
    np.save(os.path.join(out_dir, 'similarity_matrix.npy'), S)
    np.save(os.path.join(out_dir, 'upper_triangular_similarities.npy'), S[np.triu_indices(len(keys), k=1)])
    _dump(out_dir, 'speaker_similarities', {a: {b: float(S[i, j]) for j, b in enumerate(keys)}
                                            for i, a in enumerate(keys)})


def print_summary(rep, n_extreme):
    up, ext, thr = rep['upper_triangular_statistics'], rep['extreme_similarity_pairs'], rep['threshold_statistics']
    bar = '=' * 80
    print(f'\n{bar}\nSIMILARITY MATRIX ANALYSIS SUMMARY\n{bar}')
    print(f"Total speakers: {rep['similarity_statistics']['total_speakers']}")
    print(f"Total speaker pairs (upper triangular): {up['total_pairs']:,}")
    for label, key in (('Mean', 'mean'), ('Std', 'std'), ('Min', 'min'), ('Max', 'max'), ('Median', 'median')):
        print(f"{label} inter-speaker similarity: {up[key + '_similarity']:.4f}")
    for label, name in (('most', 'most_similar_pairs'), ('least', 'least_similar_pairs')):
        print(f"\nTop {n_extreme} {label} similar pairs analyzed: {len(ext[name])}")
        if ext[name]:
            top = ext[name][0]
            print(f"{label.capitalize()} similar pair (Rank #1):\n  {top['speaker1']} <-> {top['speaker2']}\n"
                  f"  Similarity: {top['similarity']:.4f}")
    for label, t in (('High', '0.9'), ('Very high', '0.95'), ('Extremely high', '0.99')):
        c = thr.get('threshold_' + t)
        if c:
            print(('\n' if t == '0.9' else '') + f"{label} similarity pairs (>{t}): {c['count']:,} ({c['percentage']:.2f}%)")
    print(bar)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(levelname)s - %(message)s')
    t0 = time.time()
    utt_dir = os.path.join(args.embeddings_dir, args.utterances_subdir)
    spk_dir = os.path.join(args.embeddings_dir, args.speakers_output_subdir)
    sim_dir = os.path.join(args.embeddings_dir, args.similarities_output_subdir)
    progress = os.path.join(args.embeddings_dir, PROGRESS_FILE)
    if not os.path.isdir(utt_dir):
        raise SystemExit(f'Utterances directory not found: {utt_dir}')
    device = None
    if not args.skip_similarity and args.device == 'cuda':
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('--device cuda needs a ROCm device (use --device host for the numpy path)')
        device = torch.device('cuda')

    log.info('=== Stage 1: Scanning speaker files ===')
    found = scan_utterances(utt_dir, args.max_speakers)
    if not found:
        raise SystemExit('No speaker utterances found')
    log.info('Found %d speakers, %d utterances', len(found), sum(len(v) for v in found.values()))
    log.info('=== Stage 2: Computing speaker embeddings ===')
    embeddings, info = speaker_embeddings(found, args.num_workers, args.batch_size, progress if args.resume else None)
    if not embeddings:
        raise SystemExit('No speaker embeddings computed')
    if not args.skip_similarity and args.save_matrix and len(embeddings) > SAVE_MATRIX_MAX:   # before anything is written
        raise SystemExit(f'--save_matrix writes O(N^2) files and is limited to {SAVE_MATRIX_MAX} speakers; '
                         f'{len(embeddings)} speakers were found. Run without it: the analysis needs no matrix.')
    log.info('=== Stage 3: Saving speaker files ===')
    save_speaker_files(embeddings, info, spk_dir)

    if not args.skip_similarity:
        keys = list(embeddings)
        dims = {len(e) for e in embeddings.values()}
        if len(dims) != 1:
            raise SystemExit(f'Speaker embeddings have different sizes: {sorted(dims)}')
        X = np.stack([embeddings[k] for k in keys]).astype(np.float32)
        log.info('=== Stage 4: Analysing similarities of %d speakers ===', len(keys))
        t1 = time.time()
        rep = sa.analyze(X, keys, top_k=args.top_k, n_extreme=args.n_extreme, device=device)
        log.info('Analysis completed in %.2f seconds', time.time() - t1)
        os.makedirs(sim_dir, exist_ok=True)
        _dump(sim_dir, 'speaker_keys_mapping', rep['speaker_keys_mapping'])
        _dump(sim_dir, 'similarity_statistics', rep['similarity_statistics'])
        if args.save_matrix:
            save_matrix(X, keys, sim_dir, device)
        if 'analysis_summary' in rep:
            for name in ANALYSIS_FILES:
                _dump(sim_dir, name, rep[name])
            print_summary(rep, args.n_extreme)
        else:
            log.warning('A single speaker: no pair to analyse')
        stats, bar = rep['similarity_statistics'], '=' * 60
        print(f"\n{bar}\nSIMILARITY COMPUTATION COMPLETED\n{bar}\nTotal speakers: {stats['total_speakers']}\n"
              f"Mean similarity: {stats['mean_similarity']:.4f}\nMin similarity: {stats['min_similarity']:.4f}\n"
              f"Max similarity: {stats['max_similarity']:.4f}\n{bar}")
    else:
        log.info('Similarity computation skipped as requested')
    if os.path.exists(progress):
        os.remove(progress)
    log.info('TOTAL PROCESSING TIME: %.2f seconds', time.time() - t0)
    return 0


if __name__ == '__main__':
    sys.exit(main())
