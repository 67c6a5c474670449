"""speakerlab/bin/compute_speaker_similarities.py on a tiny tree of pickles, the numpy path: the
file set with and without --save_matrix, the JSON keys of the reference's files, the NaN utterance
and the all-NaN speaker dropped, --resume after a planted progress file, --max_speakers and
--skip_similarity."""
import json
import os
import pickle

import numpy as np
import pytest

import sim_cli_tree as tree
from speakerlab.bin import compute_speaker_similarities as css
from speakerlab.utils import similarity_analysis as sa


@pytest.fixture(scope='module')
def plain(tmp_path_factory):
    root = tmp_path_factory.mktemp('sim_cli')
    want = tree.make_tree(str(root))
    return str(root), want, tree.run(str(root))


def test_file_set_and_json_keys(plain, capsys):
    root, want, out = plain
    assert set(out) == tree.ALWAYS
    assert not os.path.exists(os.path.join(root, css.PROGRESS_FILE))
    keys = sorted(want)
    assert len(keys) == 39 and tree.NAN_SPEAKER not in keys
    assert out['speaker_keys_mapping.json'] == {str(i): k for i, k in enumerate(keys)}
    assert set(out['similarity_statistics.json']) == {'total_speakers', 'similarity_matrix_shape', 'mean_similarity',
                                                      'std_similarity', 'min_similarity', 'max_similarity'}
    assert out['similarity_statistics.json']['similarity_matrix_shape'] == [39, 39]
    up = out['upper_triangular_statistics.json']
    assert set(up) == {'total_pairs', 'mean_similarity', 'std_similarity', 'min_similarity', 'max_similarity',
                       'median_similarity', 'q25_similarity', 'q75_similarity'}
    assert up['total_pairs'] == 39 * 38 // 2
    ext = out['extreme_similarity_pairs.json']
    assert set(ext) == {'most_similar_pairs', 'least_similar_pairs', 'metadata'}
    assert ext['metadata'] == {'num_most_similar': 30, 'num_least_similar': 30, 'total_pairs_analyzed': 741}
    assert set(ext['most_similar_pairs'][0]) == {'rank', 'speaker1', 'speaker2', 'similarity'}
    assert [p['rank'] for p in ext['least_similar_pairs']] == list(range(1, 31))
    tops = out['speaker_top_similarities.json']
    assert sorted(tops) == keys
    assert set(tops[keys[0]]) == {'top_similarities', 'mean_similarity_to_others', 'max_similarity_to_others',
                                  'min_similarity_to_others'}
    assert len(tops[keys[0]]['top_similarities']) == 5 and set(tops[keys[0]]['top_similarities'][0]) == {'speaker', 'similarity'}
    dist = out['similarity_distribution.json']
    assert len(dist['bins']) == 51 and len(dist['counts']) == 50 and sum(dist['counts']) == 741
    thr = out['threshold_statistics.json']
    assert list(thr) == [f'threshold_{t}' for t in sa.THRESHOLDS] and set(thr['threshold_0.9']) == {'count', 'percentage'}
    summary = out['analysis_summary.json']
    assert set(summary) == {'analysis_info', 'upper_triangular_stats', 'extreme_pairs_summary', 'threshold_statistics',
                            'distribution_info'}
    assert summary['analysis_info']['top_k_analyzed'] == 5 and summary['upper_triangular_stats'] == up
    assert summary['extreme_pairs_summary']['most_similar_top1'] == ext['most_similar_pairs'][0]


def test_speaker_files_and_the_nan_cases(plain):
    root, want, _ = plain
    spk = os.path.join(root, 'embeddings_individual', 'speakers')
    assert sorted(os.listdir(spk)) == ['setA', 'setB']
    assert not os.path.exists(os.path.join(spk, 'setA', tree.NAN_SPEAKER + '.pkl'))
    for name, mean in want.items():
        d = os.path.join(spk, 'setA' if int(name[3:]) < 25 else 'setB')
        with open(os.path.join(d, name + '.pkl'), 'rb') as f:
            data = pickle.load(f)
        assert data['embedding'].dtype == np.float32 and np.array_equal(data['embedding'], mean)
        with open(os.path.join(d, name + '_info.json')) as f:
            info = json.load(f)
        assert info == data['info'] and info['speaker_key'] == name and info['embedding_dim'] == 64
    with open(os.path.join(spk, 'setA', tree.PART_NAN_SPEAKER + '_info.json')) as f:
        assert json.load(f)['num_utterances'] == 2                 # the NaN utterance is dropped


def test_analysis_matches_the_numpy_statement(plain):
    root, want, out = plain
    keys = sorted(want)
    rep = sa.analyze(np.stack([want[k] for k in keys]), keys, top_k=5, n_extreme=30)
    for name in tree.ALWAYS - {'speaker_keys_mapping.json'}:
        assert out[name] == json.loads(json.dumps(rep[name[:-5]])), name


def test_save_matrix(tmp_path, plain):
    want = tree.make_tree(str(tmp_path))
    out = tree.run(str(tmp_path), '--save_matrix')
    assert set(out) == tree.ALWAYS | tree.MATRIX
    keys = sorted(want)
    S = sa.host_cosine(np.stack([want[k] for k in keys]))
    assert np.array_equal(out['similarity_matrix.npy'], S)
    assert np.array_equal(out['upper_triangular_similarities.npy'], S[np.triu_indices(39, k=1)])
    assert out['speaker_similarities.json'][keys[3]][keys[9]] == float(S[3, 9])
    for name in tree.ALWAYS:
        assert out[name] == plain[2][name], name


def test_save_matrix_is_refused_above_the_cap(tmp_path, monkeypatch):
    tree.make_tree(str(tmp_path))
    monkeypatch.setattr(css, 'SAVE_MATRIX_MAX', 20)
    with pytest.raises(SystemExit) as ei:
        tree.run(str(tmp_path), '--save_matrix')
    assert '--save_matrix' in str(ei.value) and '39 speakers' in str(ei.value)
    assert css.parse_args(['--embeddings_dir', 'x']).save_matrix is False
    # refused before stage 3: nothing has been written
    assert not os.path.exists(os.path.join(str(tmp_path), 'embeddings_individual', 'speakers'))


def test_resume_after_a_planted_progress_file(tmp_path, plain):
    want = tree.make_tree(str(tmp_path))
    planted = np.full(64, 0.25, np.float32)
    planted[::2] = -0.5
    info = {'dataset': 'setA', 'speaker_id': 'spk000', 'speaker_key': 'spk000', 'num_utterances': 1,
            'embedding_dim': 64, 'utterances': []}
    progress = os.path.join(str(tmp_path), css.PROGRESS_FILE)
    css.save_progress({'spk000': planted}, {'spk000': info}, progress)
    out = tree.run(str(tmp_path), '--resume')
    assert not os.path.exists(progress)                            # removed at the end
    with open(os.path.join(str(tmp_path), 'embeddings_individual', 'speakers', 'setA', 'spk000.pkl'), 'rb') as f:
        assert np.array_equal(pickle.load(f)['embedding'], planted)   # taken from the progress file, not recomputed
    assert out['speaker_keys_mapping.json'] == plain[2]['speaker_keys_mapping.json']
    assert out['upper_triangular_statistics.json'] != plain[2]['upper_triangular_statistics.json']
    # without --resume the planted file is ignored, and removed
    css.save_progress({'spk000': planted}, {'spk000': info}, progress)
    again = tree.run(str(tmp_path))
    assert again['upper_triangular_statistics.json'] == plain[2]['upper_triangular_statistics.json']
    assert not os.path.exists(progress)


def test_max_speakers_and_skip_similarity(tmp_path):
    tree.make_tree(str(tmp_path))
    out = tree.run(str(tmp_path), '--max_speakers', '10')
    assert len(out['speaker_keys_mapping.json']) == 9              # spk007 of the first ten has NaN utterances only
    assert out['upper_triangular_statistics.json']['total_pairs'] == 36
    assert out['extreme_similarity_pairs.json']['metadata']['num_most_similar'] == 30
    other = tmp_path / 'skip'
    other.mkdir()
    tree.make_tree(str(other))
    assert tree.run(str(other), '--skip_similarity') == {}
    assert not os.path.exists(os.path.join(str(other), 'speaker_similarity_analysis'))
    assert len(os.listdir(os.path.join(str(other), 'embeddings_individual', 'speakers', 'setB'))) == 30


def test_argument_errors(tmp_path):
    for extra in (['--top_k', '0'], ['--n_extreme', '-1'], ['--device', 'tpu']):
        with pytest.raises(SystemExit) as ei:
            css.parse_args(['--embeddings_dir', 'x'] + extra)
        assert ei.value.code == 2
    with pytest.raises(SystemExit):
        css.main(['--embeddings_dir', str(tmp_path), '--device', 'host'])   # no utterances directory
