"""bench.py --dump-outputs: a plain run writes the embeddings of its last timed step, and
they are what the timed path (GPU Fbank + ERes2NetV2 forward on the seeded input) computes.
The same run pins the plain result line: the headline keys are there and the legs behind
--full (range-guard count, rooflines, CPU baseline) did not run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 8


@pytest.mark.gpu
def test_plain_run_dumps_last_step_embeddings(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '2',
                          '--warmup', '1', '--batch', str(B), '--dump-outputs', str(tmp_path)],
                         cwd=REPO, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line['steps'] == 2 and line['warmup'] == 1
    assert line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'utt/s' and line['higher_is_better'] is True
    assert line['metric'] and line['dtype']
    assert line['roofline'] is None and line['cpu_baseline'] is None and line['exact_reruns'] is None

    assert os.listdir(tmp_path) == ['embeddings.npy']
    emb = np.load(tmp_path / 'embeddings.npy')
    assert emb.dtype == np.float32 and emb.shape == (B, 192)
    assert np.isfinite(emb).all()

    # the same path in this process: bench.py's seeded input (rank 0) and weights
    import bench
    from speakerlab import _hip
    from speakerlab.utils import synthetic
    dev = torch.device('cuda', 0)
    model = bench.build_model(dev)
    wavs = torch.from_numpy(synthetic.pcm16_batch(B, bench.SAMPLES, seed=1)).to(dev)
    with torch.no_grad():
        ref = model(_hip.fbank(wavs, 80, mean_nor=True)).cpu().numpy()
    # same kernels on the same input: at most summation-order noise, far inside the 1e-4 parity bar
    assert helpers.rel_err(emb, ref).max() < 1e-4
