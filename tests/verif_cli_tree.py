"""The utterance trees the verification CLI tests run on, and a runner for the tool."""
import json
import os
import pickle

import numpy as np

from speakerlab.bin import compute_utterance_similarities as cus

FILES = {'speaker_statistics.json', 'evaluation_results_cosine.json', 'analysis_report.json', 'analysis_report.md'}


def write_tree(root, embeddings, speaker, dataset_of=lambda s: 'set'):
    """One pickle per row of ``embeddings``: <root>/embeddings_individual/utterances/<dataset>/spkNN/uttNNN.pkl, so
    that the sorted scan returns the rows in their order when ``speaker`` is ascending."""
    count = {}
    for emb, s in zip(embeddings, speaker):
        d = os.path.join(root, 'embeddings_individual', 'utterances', dataset_of(int(s)), f'spk{int(s):02d}')
        os.makedirs(d, exist_ok=True)
        u = count[int(s)] = count.get(int(s), 0) + 1
        with open(os.path.join(d, f'utt{u:03d}.pkl'), 'wb') as f:
            pickle.dump({'embedding': np.asarray(emb)}, f)


def synthetic_tree(root, e=64, seed=9):
    """2 data sets, 14 speakers with 1-6 utterances around a centre each; a NaN utterance and an Inf one are
    dropped by the scan.  Returns (embeddings float32 [N, e], speaker keys) of the valid ones in scan order."""
    rng = np.random.default_rng(seed)
    X, speaker = [], []
    for s in range(14):
        centre = rng.standard_normal(e)
        for _ in range(1 + s % 6):
            X.append((centre + 1.2 * rng.standard_normal(e)).astype(np.float32))
            speaker.append(s)
    bad = [3, 17]
    X[bad[0]] = X[bad[0]].copy(); X[bad[0]][2] = np.nan
    X[bad[1]] = X[bad[1]].copy(); X[bad[1]][5] = np.inf
    dataset_of = lambda s: 'setA' if s < 8 else 'setB'
    write_tree(root, X, speaker, dataset_of)
    keep = [i for i in range(len(X)) if i not in bad]
    return np.stack([X[i] for i in keep]), [f'{dataset_of(speaker[i])}_spk{speaker[i]:02d}' for i in keep]


def run(root, *extra):
    assert cus.main(['--embeddings_dir', str(root), '--num_workers', '1', '--no_plot', *extra]) == 0
    out_dir = os.path.join(root, 'utterance_analysis')
    out = {}
    for name in os.listdir(out_dir):
        with open(os.path.join(out_dir, name), encoding='utf-8') as f:
            out[name] = json.load(f) if name.endswith('.json') else f.read()
    return out
