#!/usr/bin/env python3
"""GPU resampler timing (a GPU script, not a test): spk_resample_f32 against the host
fileio.resample it stands in for, on the shapes of DESIGN §7 'GPU resampler':

  (a) one 3600 s recording, 48 kHz -> 16 kHz and 44.1 kHz -> 16 kHz;
  (b) 256 x 10 s at 44.1 kHz -> 16 kHz as one ragged call.

Device time: HIP events around `--inner` back-to-back calls on resident buffers, `--warmup`
untimed rounds, median of `--runs`.  Bytes are the algorithmic ones (4 B per input sample read
once + 4 B per output written once); `hbm_frac` is their rate over the measured float4-copy rate
of the HBM (6.29 TB/s).  Host time: wall clock of fileio.resample with torch's thread count set
to `--threads`, median of `--host-runs` (0 skips it).  One JSON line; `--out` also writes it.

  python tools/resample_bench.py --out profiles/resample_bench.json
"""
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

import torch  # noqa: E402

from speakerlab import _hip  # noqa: E402
from speakerlab.utils import fileio  # noqa: E402

HBM_COPY_TBS = 6.29


def taps_per_output(orig, new):
    """FMAs per output: the widest non-zero support over the phases (what the kernel loops over)."""
    import ctypes

    import numpy as np
    n, K, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    lib = _hip.lib()
    assert lib.spk_resample_taps(orig, new, ctypes.byref(n), ctypes.byref(K), ctypes.byref(w), None, 0) == 0
    h = np.zeros((n.value, K.value), dtype=np.float32)
    assert lib.spk_resample_taps(orig, new, None, None, None, h.ctypes.data, h.size) == 0
    nz = h != 0
    first, last = nz.argmax(axis=1), K.value - 1 - nz[:, ::-1].argmax(axis=1)
    return int((last - first + 1).max()), K.value


def device_case(name, n_utt, seconds, orig, new, args, dev):
    L = int(seconds * orig)
    M = _hip.resample_out_len(L, orig, new)
    gen = torch.Generator(device='cpu').manual_seed(1)
    wav = (torch.rand(n_utt * L, generator=gen) - 0.5).to(dev)
    out = torch.empty(n_utt * M, dtype=torch.float32, device=dev)
    offs = torch.tensor([[i * L for i in range(n_utt + 1)], [i * M for i in range(n_utt + 1)]], dtype=torch.int64).to(dev)
    lib, stream = _hip.lib(), torch.cuda.current_stream(dev).cuda_stream

    def call():
        rc = lib.spk_resample_f32(wav.data_ptr(), offs[0].data_ptr(), n_utt, orig, new, out.data_ptr(),
                                  offs[1].data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(lib.spk_last_error().decode())

    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / args.inner)
    t = statistics.median(ms)
    nbytes = 4.0 * n_utt * (L + M)
    S, K = taps_per_output(orig, new)
    res = {'case': name, 'orig': orig, 'new': new, 'n_utt': n_utt, 'seconds': seconds, 'in_samples': n_utt * L,
           'out_samples': n_utt * M, 'gpu_ms_median': t, 'gpu_ms_min': min(ms), 'gpu_ms_max': max(ms),
           'algorithmic_bytes': nbytes, 'tb_per_s': nbytes / (t * 1e-3) / 1e12,
           'hbm_frac': nbytes / (t * 1e-3) / 1e12 / HBM_COPY_TBS, 'fma_per_output': S, 'taps_per_phase_K': K,
           'gfma_per_s': n_utt * M * S / (t * 1e-3) / 1e9}
    if args.host_runs > 0:
        x = wav.cpu().view(n_utt, L)
        host = []
        for _ in range(args.host_runs):
            t0 = time.perf_counter()
            y = fileio.resample(x, orig, new)
            host.append((time.perf_counter() - t0) * 1e3)
        res['host_ms_median'] = statistics.median(host)
        res['host_threads'] = torch.get_num_threads()
        res['speedup_vs_host'] = res['host_ms_median'] / t
        res['max_abs_diff_vs_host'] = float((out.cpu().view(n_utt, M) - y).abs().max())
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--host-runs', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--seconds', type=float, default=3600.0, help='length of the long recording of case (a)')
    ap.add_argument('--out', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('resample_bench.py needs a ROCm device')
    torch.set_num_threads(args.threads)
    dev = torch.device('cuda', 0)
    cases = [device_case('a_long_48k', 1, args.seconds, 48000, 16000, args, dev),
             device_case('a_long_44k1', 1, args.seconds, 44100, 16000, args, dev),
             device_case('b_256x10s_44k1', 256, 10.0, 44100, 16000, args, dev)]
    import socket
    res = {'device': torch.cuda.get_device_name(0), 'host': socket.gethostname(), 'hbm_copy_tb_per_s': HBM_COPY_TBS, 'warmup': args.warmup,
           'runs': args.runs, 'inner': args.inner, 'cases': cases}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
