"""Single-speaker check, the parts that need no device: the float64 restatement of the pair
statistics against a double loop, the condensed pair index, the pair-offset helper (Python and the
library's host entry), the CLI's argument handling and the result of a file without speech."""
import ctypes
import os

import numpy as np
import pytest

from speakerlab import _hip
from speakerlab.bin import check_single_speaker as css
from speakerlab.utils import single_speaker as ss

E_INVALID, E_UNSUPPORTED = -1, -6


def _brute(x, thr):
    x = np.asarray(x, dtype=np.float64)
    vals = []
    for i in range(len(x)):
        for j in range(i + 1, len(x)):
            ni = sum(v * v for v in x[i]) ** 0.5 or 1.0
            nj = sum(v * v for v in x[j]) ** 0.5 or 1.0
            vals.append(sum(a * b for a, b in zip(x[i], x[j])) / (ni * nj))
    if not vals:
        return [], 1.0, 1.0, -1, 0
    return vals, min(vals), sum(vals) / len(vals), vals.index(min(vals)), sum(v < thr for v in vals)


def test_pair_stats_host_against_double_loop():
    rng = np.random.default_rng(0)
    groups = [rng.standard_normal((n, 12)).astype(np.float32) for n in (0, 1, 2, 3, 9)]
    groups[4][2] = 0                                  # a zero row: its pairs score 0
    groups[3][2] = groups[3][0]                       # cosine 1 inside a group
    groups.append(None)
    thr = 0.1
    res = ss.pair_stats_host(groups, thr)
    assert len(res) == len(groups)
    for g, r in zip(groups, res):
        vals, mn, mean, arg, below = _brute(np.zeros((0, 12)) if g is None else g, thr)
        assert r['cos'].dtype == np.float64 and len(r['cos']) == len(vals)
        np.testing.assert_allclose(r['cos'], vals, rtol=0, atol=1e-15)
        assert abs(r['min'] - mn) <= 1e-15 and abs(r['mean'] - mean) <= 1e-15
        assert r['argmin'] == arg and r['n_below'] == below
    zero_pairs = [ss.ij_to_condensed(9, min(2, k), max(2, k)) for k in range(9) if k != 2]
    assert all(res[4]['cos'][p] == 0.0 for p in zero_pairs)
    assert res[0]['min'] == res[0]['mean'] == 1.0 and res[1]['argmin'] == -1 and res[5]['n_below'] == 0


def test_pair_stats_host_ties_and_threshold_edge():
    x = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 2.0]])    # cosines 0 1 0 0 1 0
    r = ss.pair_stats_host([x], 0.0)[0]
    assert list(r['cos']) == [0.0, 1.0, 0.0, 0.0, 1.0, 0.0]
    assert r['argmin'] == 0 and r['min'] == 0.0
    assert r['n_below'] == 0                          # a cosine equal to the threshold is not below it
    assert ss.pair_stats_host([x], 1e-9)[0]['n_below'] == 4


@pytest.mark.parametrize('n', [2, 3, 64, 65, 2049])
def test_condensed_round_trip(n):
    i, j = np.triu_indices(n, 1)
    P = ss.pair_count(n)
    assert len(i) == P
    picks = range(P) if n <= 65 else sorted(set(range(0, P, 997)) | set(range(P - 2 * n, P)) | set(range(2 * n)))
    for p in picks:
        assert ss.condensed_to_ij(n, p) == (int(i[p]), int(j[p])), p
        assert ss.ij_to_condensed(n, int(i[p]), int(j[p])) == p
    for bad in (-1, P):
        with pytest.raises(ValueError):
            ss.condensed_to_ij(n, bad)


def test_pair_offsets():
    assert ss.pair_offsets([0, 1, 2, 3]) == [0, 0, 0, 1, 4]
    assert ss.pair_offsets([]) == [0]
    assert ss.pair_offsets([65, 130]) == [0, 2080, 2080 + 8385]
    # the library's host entry on the same groups, given as row offsets
    assert _hip.pair_cosine_sizes([0, 0, 1, 3, 6]) == [0, 0, 0, 1, 4]
    assert _hip.pair_cosine_sizes([0]) == [0]
    assert _hip.pair_cosine_sizes([0, 32768]) == [0, 32768 * 32767 // 2]


def test_pair_cosine_sizes_errors_write_nothing():
    lib = _hip.lib()

    def call(offs, G, out):
        arr = (ctypes.c_int64 * len(offs))(*offs)
        return lib.spk_pair_cosine_sizes(arr, G, out)

    out = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    assert call([0, 3, 2, 5], 3, out) == E_INVALID            # decreasing
    assert call([1, 3, 4, 5], 3, out) == E_INVALID            # does not start at 0
    assert call([0, 3, 4, 5], -1, out) == E_INVALID
    assert call([0, 3, 4, 4 + 32769], 3, out) == E_UNSUPPORTED
    assert lib.spk_pair_cosine_sizes(None, 0, out) == E_INVALID
    assert lib.spk_pair_cosine_sizes((ctypes.c_int64 * 1)(0), 0, None) == E_INVALID
    assert list(out) == [7, 7, 7, 7]
    assert b'spk_pair_cosine_sizes' in lib.spk_last_error()


def test_launch_plan_keeps_every_grid_below_2_32_work_items():
    """A pair takes a wave of 64 work-items and a launch's grid is a 32-bit count of them, so no
    pair launch may cover 2^26 pairs; the plan cuts at 2^25, inside a group where it has to."""
    cap = 1 << 25
    P = 32768 * 32767 // 2                                     # 536,854,528 pairs, the largest group
    plan = _hip.pair_cosine_plan([0, 32768])
    assert plan == {'pair_launches': -(-P // cap), 'stats_launches': 1, 'max_launch_pairs': cap, 'planned_pairs': P}
    assert plan['pair_launches'] == 16 and plan['max_launch_pairs'] * 64 < 2 ** 32
    assert _hip.pair_cosine_plan([0, 32768], with_cos=False) == {
        'pair_launches': 0, 'stats_launches': 1, 'max_launch_pairs': 0, 'planned_pairs': 0}
    # 64 groups of 1500 rows: one chunk of descriptors, 71,952,000 pairs, three launches
    offs = [1500 * k for k in range(65)]
    plan = _hip.pair_cosine_plan(offs)
    assert plan == {'pair_launches': 3, 'stats_launches': 1, 'max_launch_pairs': cap,
                    'planned_pairs': 64 * (1500 * 1499 // 2)}
    # the first group on each side of the cut: 8192 rows are 2^25 - 4096 pairs, 8193 rows 4096 more
    assert _hip.pair_cosine_plan([0, 8192])['pair_launches'] == 1
    plan = _hip.pair_cosine_plan([0, 8193])
    assert plan['pair_launches'] == 2 and plan['max_launch_pairs'] == cap and plan['planned_pairs'] == cap + 4096
    # 150 small groups: three chunks, each with pairs; groups without pairs launch only statistics
    sizes = [k % 7 for k in range(150)]
    plan = _hip.pair_cosine_plan([0] + list(np.cumsum(sizes)))
    assert plan == {'pair_launches': 3, 'stats_launches': 3, 'max_launch_pairs': max(
        sum(ss.pair_count(n) for n in sizes[lo:lo + 64]) for lo in (0, 64, 128)),
        'planned_pairs': sum(ss.pair_count(n) for n in sizes)}
    assert _hip.pair_cosine_plan([0, 1, 1, 2]) == {'pair_launches': 0, 'stats_launches': 1, 'max_launch_pairs': 0,
                                                   'planned_pairs': 0}
    assert _hip.pair_cosine_plan([0])['stats_launches'] == 0
    with pytest.raises(_hip.HipError) as ei:
        _hip.pair_cosine_plan([0, 32769])
    assert ei.value.code == E_UNSUPPORTED


def test_pair_cosine_stats_argument_errors_without_a_device():
    """The checks run before anything is launched, so they answer on a machine without a GPU."""
    lib = _hip.lib()
    offs = (ctypes.c_int64 * 3)(0, 2, 5)
    p = ctypes.c_void_p(4096)                                # never dereferenced: every call fails its checks

    def call(X=p, ldx=8, E=8, offsets=offs, G=2, mn=p, mean=p, argmin=p, below=p):
        return lib.spk_pair_cosine_stats(X, ldx, E, offsets, G, 0.5, None, mn, mean, argmin, below, None)

    assert call(G=-1) == E_INVALID
    assert call(offsets=None) == E_INVALID
    for E in (0, -4, 6):
        assert call(E=E, ldx=8) == E_INVALID
    assert call(ldx=4) == E_INVALID
    assert call(ldx=10) == E_INVALID                         # rows are read as float4
    assert call(X=ctypes.c_void_p(4096 + 4)) == E_INVALID
    # without cos a group is one workgroup's work: capped at 4096 rows (cos is null in every call here)
    assert call(offsets=(ctypes.c_int64 * 3)(0, 2, 2 + 4097)) == E_UNSUPPORTED
    assert b'4096' in lib.spk_last_error()
    assert call(offsets=(ctypes.c_int64 * 3)(0, 5, 2)) == E_INVALID
    assert call(offsets=(ctypes.c_int64 * 3)(0, 2, 2 + 32769)) == E_UNSUPPORTED
    for name in ('X', 'mn', 'mean', 'argmin', 'below'):
        assert call(**{name: None}) == E_INVALID, name
    assert call(G=0) == 0                                    # nothing to do, nothing launched


def test_parser_needs_exactly_one_input():
    parser = css.build_parser()
    for argv in ([], ['--wav', 'a.wav', '--src_dir', 'd']):
        with pytest.raises(SystemExit):
            parser.parse_args(argv)
    a = parser.parse_args(['--wav', 'a.wav'])
    assert (a.threshold, a.files_per_batch, a.batch_size, a.pattern) == (0.8, 16, 64, '*speech_estimate.wav')
    assert not (a.no_pairs or a.gpu_vad or a.gpu_resample or a.synthetic_weights) and a.vad == 'auto'
    a = parser.parse_args(['--src_dir', 'd', '--pattern', '*.wav', '--no_pairs', '--files_per_batch', '4',
                           '--threshold', '0.5', '--gpu_vad', '--vad', 'energy', '--out_dir', 'o'])
    assert a.no_pairs and a.gpu_vad and a.files_per_batch == 4 and a.threshold == 0.5 and a.out_dir == 'o'


def test_input_paths_and_output_names(tmp_path):
    parser = css.build_parser()
    lst = tmp_path / 'wavs.list'
    lst.write_text('a/one.wav\n\n  b/two.wav  \n')
    assert css.input_paths(parser.parse_args(['--wav', 'x/y.wav'])) == (['x/y.wav'], False)
    assert css.input_paths(parser.parse_args(['--wav', str(lst)])) == (['a/one.wav', 'b/two.wav'], False)
    d = tmp_path / 'src'
    d.mkdir()
    for name in ('b_speech_estimate.wav', 'a_speech_estimate.wav', 'c_other.wav'):
        (d / name).write_bytes(b'')
    args = parser.parse_args(['--src_dir', str(d)])
    paths, directory_mode = css.input_paths(args)
    assert directory_mode and [os.path.basename(p) for p in paths] == ['a_speech_estimate.wav',
                                                                      'b_speech_estimate.wav']
    assert css.output_dir(args) == os.path.join(str(d), 'single_spk_check')
    assert css.output_dir(parser.parse_args(['--src_dir', str(d), '--out_dir', 'o'])) == 'o'
    assert css.output_file('o', '/x/a_speech_estimate.wav') == os.path.join('o', 'a_speech_estimate.single_spk.json')
    with pytest.raises(SystemExit):
        css.input_paths(parser.parse_args(['--src_dir', str(d), '--pattern', '*.flac']))


def test_result_of_a_file_without_speech():
    st = ss.pair_stats_host([None], 0.8)[0]
    res = ss.make_result('quiet.wav', [], 0.8, st)
    assert tuple(res) == ss.RESULT_KEYS
    assert res == {'wav_path': 'quiet.wav', 'num_segments': 0, 'segments': [], 'threshold': 0.8,
                   'min_pairwise_cosine': 1.0, 'mean_pairwise_cosine': 1.0, 'is_single_speaker': True,
                   'pairwise_similarities': []}
    assert 'pairwise_similarities' not in ss.make_result('quiet.wav', [], 0.8, st, want_pairs=False)


def test_result_pairs_follow_condensed_order():
    x = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    st = ss.pair_stats_host([x], 0.5)[0]
    res = ss.make_result('w.wav', [[0.0, 1.0], [2.0, 3.0], [4.0, 5.5]], 0.5, st)
    assert [(p['i'], p['j']) for p in res['pairwise_similarities']] == [(0, 1), (0, 2), (1, 2)]
    assert res['pairwise_similarities'][2]['seg_j'] == {'start': 4.0, 'stop': 5.5}
    assert res['min_pairwise_cosine'] == 0.0 and not res['is_single_speaker'] and res['num_segments'] == 3
    # min == threshold counts as single-speaker
    assert ss.make_result('w.wav', [[0, 1], [2, 3], [4, 5]], 0.0, st)['is_single_speaker']
