"""``infer_diarization.py --gpu_ahc --ahc_batch K``: a rank defers the clustering of K files and
clusters them with one batched launch; the outputs are those of ``--gpu_ahc`` alone."""
import pytest

pytestmark = pytest.mark.gpu


def test_cli_ahc_batch_same_rttm(tmp_path):
    from speakerlab.bin import infer_diarization as idz
    from speakerlab.utils import synthetic
    from speakerlab.utils.fileio import write_wav
    names = []
    for q, (dur, spk) in enumerate([(12.0, 2), (9.0, 3), (7.0, 2)]):
        wav, _ = synthetic.synth_meeting(dur, spk, seed=5 + q)
        names.append(f'meet{q}')
        write_wav(str(tmp_path / f'meet{q}.wav'), wav)
    lst = tmp_path / 'wavs.list'
    lst.write_text(''.join(f'{tmp_path / n}.wav\n' for n in names))
    base = ['--wav', str(lst), '--out_type', 'rttm', '--synthetic_weights', '--vad', 'energy', '--diable_progress_bar',
            '--nprocs', '1', '--gpu_ahc']
    idz.main(base + ['--out_dir', str(tmp_path / 'one')])
    idz.main(base + ['--out_dir', str(tmp_path / 'two'), '--ahc_batch', '2'])   # a group of 2, then a remainder of 1
    for n in names:
        want = (tmp_path / 'one' / f'{n}.rttm').read_bytes()
        assert len(want.splitlines()) >= 1
        assert (tmp_path / 'two' / f'{n}.rttm').read_bytes() == want
        for side in ('vad_info.json', 'vad_masked.wav'):      # each file's own VAD state was restored
            assert (tmp_path / 'two' / f'{n}.{side}').read_bytes() == (tmp_path / 'one' / f'{n}.{side}').read_bytes()
