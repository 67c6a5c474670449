"""Pooled embedding extraction (``Diarization3Dspeaker.defer_many``, ``--pool_chunks``): the
sub-segments of a group of files embedded in shared batches give each file the job ``defer``
gives it, and the CLI writes the same RTTMs with and without the flag.

Four short recordings (bursts of synthetic speech between silences) at chunk_dur 0.5 s, step
0.25 s and batches of 8, so the feature maps stay small and several batches mix files: two
files pad their chunks to the same length, one has no VAD segment as long as chunk_dur (its own,
shorter pad length) and one is pure silence (no chunks at all)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FS = 16000
CHUNK_DUR, CHUNK_STEP, BATCH = 0.5, 0.25, 8
# name -> (seconds, [(start s, stop s, speaker), ...])
RECORDINGS = {
    'two_a': (4.0, [(0.3, 1.7, 0), (2.3, 3.6, 1)]),
    'two_b': (5.0, [(0.5, 2.1, 1), (2.9, 4.5, 0)]),
    'short': (2.0, [(0.6, 0.95, 0), (1.4, 1.72, 1)]),
    'quiet': (3.0, []),
}


def _recording(seconds, bursts, seed):
    from speakerlab.utils import synthetic
    wav = np.zeros(int(seconds * FS), dtype=np.float32)
    for k, (st, ed, spk) in enumerate(bursts):
        a, b = int(st * FS), int(ed * FS)
        wav[a:b] = synthetic.synth_wav(b - a, seed=seed + k, speaker=spk)
    return wav


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    from speakerlab.utils.fileio import write_wav
    d = tmp_path_factory.mktemp('pool_chunks')
    paths = []
    for q, (name, (seconds, bursts)) in enumerate(RECORDINGS.items()):
        paths.append(str(d / f'{name}.wav'))
        write_wav(paths[-1], _recording(seconds, bursts, 100 * q))
    return paths


@pytest.fixture(scope='module')
def diar():
    from speakerlab.bin.infer_diarization import Diarization3Dspeaker
    return Diarization3Dspeaker(torch.device('cuda', 0), synthetic_weights=True, vad='energy', chunk_dur=CHUNK_DUR,
                                chunk_step=CHUNK_STEP, batch_size=BATCH, gpu_ahc=True)


@pytest.fixture(scope='module')
def jobs(diar, files):
    """(one ``defer`` per file, ``defer_many`` of all files): computed once, read by the tests."""
    return [diar.defer(f) for f in files], diar.defer_many(files)


def _pad_len(job):
    return max(min(int(ed * FS), 10 ** 9) - int(st * FS) for st, ed in job['chunks'])


def test_the_inputs_exercise_the_plan(jobs):
    """The properties the recordings were built for: without them the comparison below would not
    cover shared batches, a second pad length or an empty file."""
    one, _ = jobs
    n = [len(j['chunks']) for j in one]
    assert n[3] == 0 and min(n[:3]) >= 1
    pads = [_pad_len(j) for j in one[:3]]
    assert pads[0] == pads[1] != pads[2]
    assert pads[2] < int(CHUNK_DUR * FS)
    assert n[0] % BATCH != 0 and n[0] + n[1] > BATCH        # a batch holds chunks of both files


def test_defer_many_matches_defer(jobs):
    one, many = jobs
    assert len(many) == len(one)
    for q, (a, b) in enumerate(zip(one, many)):
        assert b['chunks'] == a['chunks'], q
        assert set(b) == set(a) and set(b['vad']) == set(a['vad'])
        for k in ('last_vad_time', 'last_vad_time_raw', 'last_vad_time_processed'):
            assert b['vad'][k] == a['vad'][k], (q, k)
        if not a['chunks']:
            assert b['embeddings'] is None and b['affinity'] is None
            continue
        ea, eb = np.asarray(a['embeddings']), np.asarray(b['embeddings'])
        assert eb.shape == ea.shape and eb.dtype == ea.dtype
        # the project's bar for model outputs: 1e-4 relative, as max |difference| over max |value|
        # of the file and row by row in the 2-norm (helpers.rel_err)
        import helpers
        rel = float(np.abs(eb - ea).max() / np.abs(ea).max())
        row = float(helpers.rel_err(eb, ea).max())
        print(f'file {q}: {len(ea)} chunks, embeddings max-abs rel {rel:.3e}, worst row {row:.3e}')
        assert rel < 1e-4, (q, rel)
        assert row < 1e-4, (q, row)
        assert tuple(b['affinity'].shape) == tuple(a['affinity'].shape) and b['affinity'].is_cuda


def test_deferred_jobs_finish_alike(diar, jobs):
    """``finish_deferred`` / ``restore_deferred`` work on the pooled jobs unchanged."""
    one, many = ([dict(j) for j in js] for js in jobs)
    diar.finish_deferred(one)
    diar.finish_deferred(many)
    for a, b in zip(one, many):
        assert b['segments'] == a['segments']
    diar.restore_deferred(many[0])
    assert diar.output_field_labels == many[0]['segments'] and diar.last_vad_time == many[0]['vad']['last_vad_time']


def test_cli_pool_chunks_same_rttm(files, tmp_path):
    import os
    from speakerlab.bin import infer_diarization as idz
    lst = tmp_path / 'wavs.list'
    lst.write_text(''.join(f'{f}\n' for f in files))
    base = ['--wav', str(lst), '--out_type', 'rttm', '--synthetic_weights', '--vad', 'energy', '--diable_progress_bar',
            '--nprocs', '1', '--gpu_ahc', '--chunk_dur', str(CHUNK_DUR), '--chunk_step', str(CHUNK_STEP),
            '--batch_size', str(BATCH)]
    idz.main(base + ['--out_dir', str(tmp_path / 'plain'), '--ahc_batch', '4'])
    idz.main(base + ['--out_dir', str(tmp_path / 'pooled'), '--ahc_batch', '4', '--pool_chunks'])
    # a group of 3 and a remainder of 1
    idz.main(base + ['--out_dir', str(tmp_path / 'pooled3'), '--ahc_batch', '3', '--pool_chunks'])
    some = 0
    for f in files:
        n = os.path.basename(f).rsplit('.', 1)[0]
        want = (tmp_path / 'plain' / f'{n}.rttm').read_bytes()
        some += len(want.splitlines())
        assert (tmp_path / 'pooled' / f'{n}.rttm').read_bytes() == want, n
        assert (tmp_path / 'pooled3' / f'{n}.rttm').read_bytes() == want, n
        # each file's own VAD state was restored before its side files were written
        assert (tmp_path / 'pooled' / f'{n}.vad_info.json').read_bytes() == \
            (tmp_path / 'plain' / f'{n}.vad_info.json').read_bytes(), n
    assert some >= 3
