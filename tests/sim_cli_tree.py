"""The tiny tree of utterance pickles the similarity CLI tests run on, and a runner for the tool."""
import json
import os
import pickle

import numpy as np

from speakerlab.bin import compute_speaker_similarities as css

ALWAYS = {'speaker_keys_mapping.json', 'similarity_statistics.json', 'upper_triangular_statistics.json',
          'extreme_similarity_pairs.json', 'speaker_top_similarities.json', 'similarity_distribution.json',
          'threshold_statistics.json', 'analysis_summary.json'}
MATRIX = {'speaker_similarities.json', 'similarity_matrix.npy', 'upper_triangular_similarities.npy'}
NAN_SPEAKER, PART_NAN_SPEAKER = 'spk007', 'spk003'


def make_tree(root, e=64, seed=5):
    """2 data sets, 40 speakers with 1-4 utterances; one NaN utterance of spk003 (which has others) and
    spk007 with NaN utterances only.  Returns speaker -> the float32 mean of its valid embeddings."""
    rng = np.random.default_rng(seed)
    want = {}
    for s in range(40):
        name, dataset = f'spk{s:03d}', 'setA' if s < 25 else 'setB'
        d = os.path.join(root, 'embeddings_individual', 'utterances', dataset, name)
        os.makedirs(d)
        n_utt = 1 + s % 4
        if name == PART_NAN_SPEAKER:
            n_utt = 3
        good = []
        for u in range(n_utt):
            emb = rng.standard_normal(e).astype(np.float32)
            if name == NAN_SPEAKER or (name == PART_NAN_SPEAKER and u == 1):
                emb[3] = np.nan
            else:
                good.append(emb)
            with open(os.path.join(d, f'utt{u}.pkl'), 'wb') as f:
                pickle.dump({'embedding': emb}, f)
        if good:
            want[name] = np.mean(np.stack(good), axis=0, dtype=np.float32)
    return want


def run(root, *extra, device='host'):
    assert css.main(['--embeddings_dir', str(root), '--num_workers', '1', '--batch_size', '7', '--top_k', '5',
                     '--n_extreme', '30', '--device', device, *extra]) == 0
    sim = os.path.join(root, 'speaker_similarity_analysis')
    out = {}
    if os.path.isdir(sim):
        for name in os.listdir(sim):
            if name.endswith('.json'):
                with open(os.path.join(sim, name)) as f:
                    out[name] = json.load(f)
            else:
                out[name] = np.load(os.path.join(sim, name))
    return out
