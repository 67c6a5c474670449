"""ctypes binding of ``libspk_hip.so`` (declared in ``include/spk_hip.h``).

This is the only bridge between the drop-in Python surface and the HIP kernels.  There is
no CPU fallback: if the shared library is missing, or a tensor is not on a ROCm device,
the call raises.  (The CPU restatement used to *check* results lives in ``oracle/`` and
is imported by tests only.)
"""
from __future__ import annotations

import collections
import ctypes
import os
import threading
from typing import Dict, Optional

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # .../3d-speaker_amd
LIB_PATH = os.environ.get('SPK_HIP_LIB', os.path.join(_PKG_ROOT, 'lib', 'libspk_hip.so'))

ARCH_ERES2NETV2 = 1
ARCH_ERES2NET = 2
ARCH_ECAPA = 3
ARCH_CAMPPLUS = 4
ARCH_RESNET = 5
ARCH_RES2NET = 6


class spk_weight_t(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char_p), ('data', ctypes.c_void_p), ('ndim', ctypes.c_int32),
                ('shape', ctypes.c_int64 * 4)]


class spk_model_config_t(ctypes.Structure):
    _fields_ = [('arch', ctypes.c_int32), ('feat_dim', ctypes.c_int32), ('embed_dim', ctypes.c_int32),
                ('m_channels', ctypes.c_int32), ('base_width', ctypes.c_int32), ('scale', ctypes.c_int32),
                ('expansion', ctypes.c_int32), ('two_emb_layer', ctypes.c_int32),
                ('channels', ctypes.c_int32 * 5), ('kernel_sizes', ctypes.c_int32 * 5),
                ('dilations', ctypes.c_int32 * 5), ('precision', ctypes.c_int32), ('pooling', ctypes.c_int32), ('reserved', ctypes.c_int32 * 6)]


# spk_model_config_t.precision (include/spk_hip.h)
PRECISIONS = {'fp32': 0, 'fp16': 1}


SPK_CONSUME_TOPK = 1


class spk_affinity_consumer_t(ctypes.Structure):
    _fields_ = [('kind', ctypes.c_int32), ('k', ctypes.c_int32), ('exclude_self', ctypes.c_int32),
                ('self_offset', ctypes.c_int64), ('threshold', ctypes.c_float), ('top_scores', ctypes.c_void_p),
                ('top_index', ctypes.c_void_p), ('count_ge', ctypes.c_void_p), ('workspace', ctypes.c_void_p),
                ('workspace_bytes', ctypes.c_size_t)]


# every entry point of include/spk_hip.h: name -> (restype, argtypes)
_P = ctypes.c_void_p
SYMBOLS = {
    'spk_version': (ctypes.c_int, []),
    'spk_last_error': (ctypes.c_char_p, []),
    'spk_fbank_f32': (ctypes.c_int, [_P, _P, ctypes.c_int32, _P, _P, ctypes.c_int32, ctypes.c_int32, _P]),
    'spk_fbank_f32_padded': (ctypes.c_int, [_P, _P, ctypes.c_int32, _P, _P, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_int32, _P]),
    'spk_fbank_chunks_f32': (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_int32, ctypes.c_int64, _P,
                                            ctypes.c_int32, ctypes.c_int32, _P]),
    'spk_resample_out_len': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.POINTER(ctypes.c_int64)]),
    'spk_resample_taps': (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                         ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), _P,
                                         ctypes.c_size_t]),
    'spk_resample_f32': (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P, _P]),
    'spk_vad_energy_sizes': (ctypes.c_int, [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                                            ctypes.POINTER(ctypes.c_int64)]),
    'spk_vad_energy_f32': (ctypes.c_int, [_P, _P, ctypes.c_int32, _P, _P, _P, _P, _P]),
    'spk_vad_apply_intervals_f32': (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P]),
    'spk_model_create': (ctypes.c_int, [ctypes.POINTER(spk_model_config_t), ctypes.POINTER(spk_weight_t),
                                        ctypes.c_int32, ctypes.POINTER(_P)]),
    'spk_model_destroy': (ctypes.c_int, [_P]),
    'spk_model_workspace_bytes': (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]),
    'spk_model_forward': (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P]),
    'spk_model_workspace_bytes_lengths': (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                         ctypes.POINTER(ctypes.c_size_t)]),
    'spk_model_forward_lengths': (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.c_size_t, _P,
                                                 _P]),
    'spk_model_flops': (ctypes.c_int, [_P, ctypes.c_int32, ctypes.POINTER(ctypes.c_double)]),
    'spk_model_range_check': (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P,
                                             ctypes.POINTER(ctypes.c_int32)]),
    'spk_model_forward_exact': (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.c_size_t, _P,
                                               _P]),
    'spk_model_guard_plan': (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                            ctypes.POINTER(ctypes.c_int32)]),
    'spk_model_plan_size': (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    'spk_model_plan_step': (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p,
                                           ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32,
                                           ctypes.POINTER(ctypes.c_double)]),
    'spk_model_plan_step_bytes': (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                 ctypes.POINTER(ctypes.c_double)]),
    'spk_model_forward_timed': (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_size_t, _P, _P,
                                               _P, ctypes.c_int32]),
    'spk_cosine_affinity': (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, _P,
                                           ctypes.c_int64, _P]),
    'spk_spectral_laplacian': (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_int64,
                                              _P, ctypes.c_size_t, _P]),
    'spk_symmetric_eig': (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int64, _P, _P]),
    'spk_cosine_topk_workspace_bytes': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64,
                                                       ctypes.POINTER(ctypes.c_size_t)]),
    'spk_cosine_topk': (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32,
                                       ctypes.POINTER(spk_affinity_consumer_t), _P]),
    'spk_cosine_trials': (ctypes.c_int, [_P, _P, ctypes.c_int32, _P, _P, ctypes.c_int64, _P, _P]),
    'spk_ahc_workspace_bytes': (ctypes.c_int, [ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]),
    'spk_ahc_average': (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, _P, _P, _P,
                                       ctypes.c_size_t, _P]),
    'spk_ahc_batched_max_n': (ctypes.c_int, []),
    'spk_ahc_average_batched_workspace_bytes': (ctypes.c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32,
                                                               ctypes.POINTER(ctypes.c_size_t)]),
    'spk_ahc_average_batched': (ctypes.c_int, [ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64),
                                               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float),
                                               ctypes.c_int32, ctypes.POINTER(_P), _P, _P, ctypes.c_size_t, _P]),
    'spk_topk_stats': (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, _P, _P, _P]),
    'spk_cosine_cohort_stats_workspace_bytes': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64,
                                                               ctypes.POINTER(ctypes.c_size_t),
                                                               ctypes.POINTER(ctypes.c_size_t)]),
    'spk_cosine_cohort_stats': (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                               _P, _P, _P, ctypes.c_size_t, _P]),
    'spk_cosine_trials_norm': (ctypes.c_int, [_P, _P, ctypes.c_int32, _P, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _P]),
    'spk_pair_cosine_sizes': (ctypes.c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_int64)]),
    'spk_pair_cosine_stats': (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                                             ctypes.c_int32, ctypes.c_float, _P, _P, _P, _P, _P, _P]),
    'spk_pair_cosine_plan': (ctypes.c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, ctypes.c_int32]
                             + [ctypes.POINTER(ctypes.c_int64)] * 4),
    'spk_cosine_sim_workspace_bytes': (ctypes.c_int, [ctypes.c_int64] + [ctypes.POINTER(ctypes.c_size_t)] * 3),
    'spk_cosine_rows_topk': (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P, _P, _P,
                                            _P, _P, ctypes.c_size_t, _P]),
    'spk_cosine_triu_stats': (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_int32, _P, ctypes.c_int32,
                                             ctypes.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t,
                                             _P, ctypes.c_size_t, _P]),
    'spk_cosine_triu_hist': (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_int32, ctypes.c_int32, _P,
                                            _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P, ctypes.c_size_t, _P]),
    'spk_cosine_verif_workspace_bytes': (ctypes.c_int, [ctypes.c_int64] + [ctypes.POINTER(ctypes.c_size_t)] * 3),
    'spk_cosine_verif_moments': (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int32, _P, ctypes.c_int32, _P, _P, _P,
                                                _P, _P, _P, _P, ctypes.c_size_t, _P, ctypes.c_size_t, _P]),
    'spk_cosine_verif_digits': (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _P,
                                               ctypes.c_int32, _P, _P, ctypes.c_size_t, _P, ctypes.c_size_t, _P]),
}

_lib = None
_lock = threading.Lock()


E_INVALID = -1       # SPK_E_INVALID
E_UNSUPPORTED = -6   # SPK_E_UNSUPPORTED


class HipError(RuntimeError):
    code = None   # the SPK_E_* code when the library returned one


def lib():
    """Load libspk_hip.so once (after torch, so it shares torch's HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise HipError(f'libspk_hip.so not found at {LIB_PATH}: build it with '
                               f'`python -c "import __graft_entry__ as g; g.build()"` (or make -C 3d-speaker_amd/csrc)')
            handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
            for name, (res, args) in SYMBOLS.items():
                fn = getattr(handle, name)
                fn.restype = res
                fn.argtypes = args
            _lib = handle
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().spk_last_error()
        err = HipError(f'{what} failed ({rc}): {msg.decode() if msg else ""}')
        err.code = rc
        raise err


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_device_tensor(x: torch.Tensor, what: str):
    if not isinstance(x, torch.Tensor) or x.device.type != 'cuda':
        raise HipError(f'{what}: the MI355X path needs a ROCm device tensor (got '
                       f'{getattr(x, "device", type(x))}); move the input with .to("cuda")')


# ----------------------------------------------------------------------------- Fbank
_frame_offsets_cache: Dict = {}


def num_frames(n_samples: int) -> int:
    return 0 if n_samples < 400 else 1 + (n_samples - 400) // 160


def fbank(wavs: torch.Tensor, n_mels: int = 80, mean_nor: bool = False, lengths=None) -> torch.Tensor:
    """Batched Kaldi Fbank on the GPU.

    ``wavs``: [B, L] float32 device tensor (or [L]).  With ``lengths`` (list of ints) the
    rows are ragged (samples beyond each length are ignored) and the result is a list of
    [T_i, n_mels] views into one buffer; otherwise [B, T, n_mels].
    """
    require_device_tensor(wavs, 'fbank')
    squeeze = wavs.dim() == 1
    if squeeze:
        wavs = wavs.unsqueeze(0)
    wavs = wavs.to(torch.float32).contiguous()
    B, L = wavs.shape
    dev = wavs.device
    if lengths is None:
        lens = [L] * B
    else:
        lens = [int(v) for v in lengths]
    frames = [num_frames(n) for n in lens]
    frame_off = [0]
    for f in frames:
        frame_off.append(frame_off[-1] + f)
    wav_off = [i * L for i in range(B + 1)]
    offs = torch.tensor([wav_off, frame_off], dtype=torch.int64).to(dev, non_blocking=True)
    feats = torch.empty((frame_off[-1], n_mels), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(lib().spk_fbank_f32(wavs.data_ptr(), offs[0].data_ptr(), B, feats.data_ptr(), offs[1].data_ptr(),
                                   n_mels, int(bool(mean_nor)), _stream(dev)), 'spk_fbank_f32')
    if lengths is not None:
        return [feats[frame_off[i]:frame_off[i + 1]] for i in range(B)]
    out = feats.view(B, frames[0], n_mels)
    return out[0] if squeeze else out


def fbank_padded(wavs: torch.Tensor, lengths, n_mels: int = 80, mean_nor: bool = False):
    """Ragged Fbank written straight into a zero-padded [B, T_max, n_mels] batch: returns
    (feats, frames) with ``frames`` a device int32 [B] tensor of valid frames per row, the
    input of the models' ``forward(x, lengths=frames)`` (spk_fbank_f32_padded)."""
    require_device_tensor(wavs, 'fbank_padded')
    wavs = wavs.to(torch.float32).contiguous()
    B, L = wavs.shape
    dev = wavs.device
    lens = [int(v) for v in lengths]
    if len(lens) != B or max(lens) > L or min(lens) < 400:
        raise HipError('fbank_padded: need B lengths in [400, padded length]')
    frames = [num_frames(n) for n in lens]
    tmax = max(frames)
    frame_off = [0]
    for f in frames:
        frame_off.append(frame_off[-1] + f)
    wav_off = [i * L for i in range(B + 1)]
    offs = torch.tensor([wav_off, frame_off], dtype=torch.int64).to(dev, non_blocking=True)
    feats = torch.empty((B, tmax, n_mels), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(lib().spk_fbank_f32_padded(wavs.data_ptr(), offs[0].data_ptr(), B, feats.data_ptr(),
                                          offs[1].data_ptr(), tmax, n_mels, int(bool(mean_nor)), _stream(dev)),
               'spk_fbank_f32_padded')
    return feats, torch.tensor(frames, dtype=torch.int32).to(dev, non_blocking=True)


def _invalid(msg: str):
    err = HipError(msg)
    err.code = E_INVALID
    return err


def fbank_chunks(wav: torch.Tensor, starts, lens, pad_len: int, n_mels: int = 80,
                 mean_nor: bool = False) -> torch.Tensor:
    """Fbank of circle-padded chunks of a device signal, [n, T, n_mels] with T = 1 + (pad_len - 400)
    // 160 (spk_fbank_chunks_f32): chunk c is ``wav[starts[c] + arange(pad_len) % lens[c]]``, read in
    place by the kernel, and the rows have the bits of ``fbank`` on that gathered batch.

    ``wav``: 1-D float32 device tensor (one recording, or several back to back); ``starts`` /
    ``lens``: n int64 values each, sequences or host or device tensors.  Every chunk must lie inside
    the signal (``lens >= 1``, ``0 <= starts``, ``starts + lens <= len(wav)``): checked here on the
    host values (device tensors are copied back for it), ``HipError`` with ``E_INVALID`` otherwise.
    """
    require_device_tensor(wav, 'fbank_chunks')
    if wav.dim() != 1:
        raise _invalid(f'fbank_chunks: expected a 1-D signal, got {tuple(wav.shape)}')
    dev = _dev_of(wav)
    wav = wav.to(torch.float32).contiguous()
    s = torch.as_tensor(starts, dtype=torch.int64).reshape(-1)
    n_ = torch.as_tensor(lens, dtype=torch.int64).reshape(-1)
    n = int(s.numel())
    if int(n_.numel()) != n:
        raise _invalid('fbank_chunks: starts and lens differ in length')
    L, pad_len = int(wav.numel()), int(pad_len)
    if n:
        sh, nh = s.cpu(), n_.cpu()
        if bool((nh < 1).any()) or bool((sh < 0).any()) or bool((sh + nh > L).any()):
            raise _invalid('fbank_chunks: every chunk needs lens >= 1, starts >= 0 and starts + lens <= len(wav)')
    if s.device != n_.device:
        s, n_ = s.to(dev), n_.to(dev)
    sn = torch.stack([s, n_]).to(dev, non_blocking=True)      # host values: one upload
    feats = torch.empty((n, max(num_frames(pad_len), 0), n_mels), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(lib().spk_fbank_chunks_f32(wav.data_ptr(), L, sn[0].data_ptr(), sn[1].data_ptr(), n, pad_len,
                                          feats.data_ptr(), n_mels, int(bool(mean_nor)), _stream(dev)),
               'spk_fbank_chunks_f32')
    return feats


# ----------------------------------------------------------------------------- resampling
def resample_out_len(n_samples: int, orig_freq: int, new_freq: int) -> int:
    """Length of ``n_samples`` at ``orig_freq`` after resampling to ``new_freq``:
    ceil(new * n / orig) in gcd-reduced rates (no GPU needed)."""
    n = ctypes.c_int64()
    _check(lib().spk_resample_out_len(int(n_samples), int(orig_freq), int(new_freq), ctypes.byref(n)),
           'spk_resample_out_len')
    return n.value


def resample(wavs, orig_freq: int, new_freq: int, lengths=None):
    """torchaudio.functional.resample(wavs, orig_freq, new_freq) (default arguments) on the GPU.

    ``wavs``: a [B, L] or [L] float32 device tensor -> [B, L'] / [L']; with ``lengths`` (valid
    samples per row) or as a list of 1-D device tensors the batch is ragged and the result is a
    list of 1-D views into one buffer, which has the layout ``fbank(..., lengths=...)`` reads.
    Every row's result has the bits it has when resampled alone.  Raises HipError (``.code``
    the SPK_E_* value) for equal or non-positive rates and for a rate pair whose polyphase
    table is above the library's cap (E_UNSUPPORTED)."""
    as_list = isinstance(wavs, (list, tuple))
    if as_list and lengths is not None:
        raise HipError('resample: lengths goes with a [B, L] tensor, not with a list')
    squeeze = False
    if not as_list:
        require_device_tensor(wavs, 'resample')
        squeeze = wavs.dim() == 1
        if squeeze:
            wavs = wavs.unsqueeze(0)
        if wavs.dim() != 2:
            raise HipError(f'resample: expected [B, L] or [L], got {tuple(wavs.shape)}')
        if lengths is not None:
            lens = [int(v) for v in lengths]
            if len(lens) != wavs.shape[0] or (lens and (min(lens) < 0 or max(lens) > wavs.shape[1])):
                raise HipError('resample: need B lengths in [0, L]')
            wavs, as_list = [wavs[i, :n] for i, n in enumerate(lens)], True
    if as_list:
        if len(wavs) == 0:
            return []
        for w in wavs:
            require_device_tensor(w, 'resample')
            if w.dim() != 1:
                raise HipError('resample: a ragged batch is a list of 1-D tensors')
        dev = wavs[0].device
        lens = [int(w.numel()) for w in wavs]
        flat = torch.cat([w.to(torch.float32) for w in wavs])
    else:
        dev = wavs.device
        lens = [int(wavs.shape[1])] * int(wavs.shape[0])
        flat = wavs.to(torch.float32).contiguous().view(-1)
    B = len(lens)
    in_off, out_off = [0], [0]
    for n in lens:
        in_off.append(in_off[-1] + n)
        out_off.append(out_off[-1] + resample_out_len(n, orig_freq, new_freq))
    offs = torch.tensor([in_off, out_off], dtype=torch.int64).to(dev, non_blocking=True)
    out = torch.empty(out_off[-1], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(lib().spk_resample_f32(flat.data_ptr(), offs[0].data_ptr(), B, int(orig_freq), int(new_freq),
                                      out.data_ptr(), offs[1].data_ptr(), _stream(dev)), 'spk_resample_f32')
    if as_list:
        return [out[out_off[i]:out_off[i + 1]] for i in range(B)]
    out = out.view(B, -1) if B else out.view(0, 0)
    return out[0] if squeeze else out


# ----------------------------------------------------------------------------- VAD front end
def vad_energy_sizes(n_samples: int):
    """(n16, n20) of ``vad_energy`` for ``n_samples`` at 16 kHz: 16 ms frames and 20 ms / 10 ms
    windows (no GPU needed)."""
    n16, n20 = ctypes.c_int64(), ctypes.c_int64()
    _check(lib().spk_vad_energy_sizes(int(n_samples), ctypes.byref(n16), ctypes.byref(n20)), 'spk_vad_energy_sizes')
    return n16.value, n20.value


def vad_energy(wav):
    """The two mean-square tracks of the VAD front end (spk_vad_energy_f32), samples clipped to
    [-1, 1] first, 16 kHz: ``e16`` float64 [L // 256] (the 16 ms frames of the energy VAD) and
    ``e20`` float32 [(L - 320) // 160 + 1] (the 20 ms / 10 ms windows of ``vad_post.frame_energy``).

    ``wav``: a 1-D float32 device tensor -> (e16, e20) device tensors; a list of 1-D device tensors
    is a ragged batch in one launch -> a list of (e16, e20) pairs of views into two buffers, each
    with the bits it has when run alone.  Non-finite samples are outside the contract."""
    as_list = isinstance(wav, (list, tuple))
    wavs = list(wav) if as_list else [wav]
    if not wavs:
        return []
    for w in wavs:
        require_device_tensor(w, 'vad_energy')
        if w.dim() != 1:
            raise HipError(f'vad_energy: expected 1-D signals, got {tuple(w.shape)}')
    dev = _dev_of(wavs[0])
    if len(wavs) == 1:
        flat = wavs[0].to(torch.float32).contiguous()
    else:
        flat = torch.cat([w.to(torch.float32) for w in wavs])
    off = [[0], [0], [0]]
    for w in wavs:
        for o, n in zip(off, (int(w.numel()),) + vad_energy_sizes(int(w.numel()))):
            o.append(o[-1] + n)
    offs = torch.tensor(off, dtype=torch.int64).to(dev, non_blocking=True)
    e16 = torch.empty(max(off[1][-1], 1), dtype=torch.float64, device=dev)
    e20 = torch.empty(max(off[2][-1], 1), dtype=torch.float32, device=dev)
    if flat.numel() == 0:
        flat = torch.zeros(1, dtype=torch.float32, device=dev)   # no utterance has a sample: nothing is read
    with torch.cuda.device(dev):
        _check(lib().spk_vad_energy_f32(flat.data_ptr(), offs[0].data_ptr(), len(wavs), e16.data_ptr(),
                                        offs[1].data_ptr(), e20.data_ptr(), offs[2].data_ptr(), _stream(dev)),
               'spk_vad_energy_f32')
    res = [(e16[off[1][i]:off[1][i + 1]], e20[off[2][i]:off[2][i + 1]]) for i in range(len(wavs))]
    return res if as_list else res[0]


def vad_apply_intervals(wav: torch.Tensor, starts, ends) -> torch.Tensor:
    """``wav`` (1-D float32 device tensor) with every sample outside the intervals
    [starts[k], ends[k]) zeroed (spk_vad_apply_intervals_f32): ``vad_post.apply_mask`` for the mask
    whose runs are the intervals.  ``starts`` / ``ends``: sorted, disjoint sample indices in
    [0, len(wav)] (sequences or int64 tensors); none gives zeros."""
    require_device_tensor(wav, 'vad_apply_intervals')
    if wav.dim() != 1:
        raise HipError(f'vad_apply_intervals: expected a 1-D signal, got {tuple(wav.shape)}')
    dev = _dev_of(wav)
    wav = wav.to(torch.float32).contiguous()
    L = int(wav.numel())
    s = torch.as_tensor(starts, dtype=torch.int64).reshape(-1)
    e = torch.as_tensor(ends, dtype=torch.int64).reshape(-1)
    n = int(s.numel())
    if int(e.numel()) != n:
        raise HipError('vad_apply_intervals: starts and ends differ in length')
    if n:
        sh, eh = s.cpu(), e.cpu()
        if (int(sh[0]) < 0 or int(eh[-1]) > L or bool((eh <= sh).any()) or bool((sh[1:] < eh[:-1]).any())):
            raise HipError('vad_apply_intervals: intervals must be non-empty, sorted, disjoint and within the signal')
    iv = torch.stack([s, e]).to(dev, non_blocking=True) if n else None
    out = torch.empty_like(wav)
    if L == 0:
        return out
    with torch.cuda.device(dev):
        _check(lib().spk_vad_apply_intervals_f32(wav.data_ptr(), L, iv[0].data_ptr() if n else None,
                                                 iv[1].data_ptr() if n else None, n, out.data_ptr(), _stream(dev)),
               'spk_vad_apply_intervals_f32')
    return out


# ----------------------------------------------------------------------------- models
class NativeModel:
    """One ``spk_model_t`` handle (folded + packed weights on one device)."""

    def __init__(self, arch: int, cfg: dict, state_dict, device: torch.device, precision: str = 'fp32'):
        if precision not in PRECISIONS:
            raise HipError(f'precision must be one of {sorted(PRECISIONS)}, got {precision!r}')
        c = spk_model_config_t()
        c.arch = arch
        c.precision = PRECISIONS[precision]
        self.precision = precision
        for k in ('feat_dim', 'embed_dim', 'm_channels', 'base_width', 'scale', 'expansion', 'two_emb_layer',
                  'pooling'):
            setattr(c, k, int(cfg.get(k, 0)))
        for k in ('channels', 'kernel_sizes', 'dilations'):
            vals = list(cfg.get(k, []))[:5]
            getattr(c, k)[:len(vals)] = vals
        self.embed_dim = int(cfg['embed_dim'])
        self.arch = arch
        self.device = device
        host = []
        ws = (spk_weight_t * len(state_dict))()
        for i, (name, t) in enumerate(state_dict.items()):
            ws[i].name = name.encode()
            ws[i].ndim = t.dim()
            for d in range(min(t.dim(), 4)):
                ws[i].shape[d] = t.shape[d]
            if t.is_floating_point():
                h = t.detach().to('cpu', torch.float32).contiguous()
                host.append(h)
                ws[i].data = h.data_ptr()
            else:
                ws[i].data = None
        handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            _check(lib().spk_model_create(ctypes.byref(c), ws, len(state_dict), ctypes.byref(handle)),
                   'spk_model_create')
        self.handle = handle
        self._ws: Optional[torch.Tensor] = None          # workspace of the last forward
        self._ws_by_stream = {}                           # stream handle -> workspace
        self._last = None                                 # (B, T, ragged, workspace, stream) of the last forward

    def __del__(self):
        h = getattr(self, 'handle', None)
        if h is not None and _lib is not None:
            try:
                _lib.spk_model_destroy(h)
            except Exception:
                pass

    def workspace_bytes(self, B: int, T: int) -> int:
        n = ctypes.c_size_t()
        _check(lib().spk_model_workspace_bytes(self.handle, B, T, ctypes.byref(n)), 'spk_model_workspace_bytes')
        return n.value

    def flops(self, T: int) -> float:
        f = ctypes.c_double()
        _check(lib().spk_model_flops(self.handle, T, ctypes.byref(f)), 'spk_model_flops')
        return f.value

    def plan(self, B: int, T: int):
        """[(step name, kernel name, algorithmic FLOPs)] of the launch plan for [B, T]."""
        n = ctypes.c_int32()
        _check(lib().spk_model_plan_size(self.handle, B, T, ctypes.byref(n)), 'spk_model_plan_size')
        out = []
        for i in range(n.value):
            name = ctypes.create_string_buffer(256)
            kern = ctypes.create_string_buffer(256)
            fl = ctypes.c_double()
            _check(lib().spk_model_plan_step(self.handle, B, T, i, name, 256, kern, 256, ctypes.byref(fl)),
                   'spk_model_plan_step')
            out.append((name.value.decode(), kern.value.decode(), fl.value))
        return out

    def plan_bytes(self, B: int, T: int):
        """Algorithmic HBM bytes of every plan step (0 where a step is not priced)."""
        out = []
        for i in range(len(self.plan(B, T))):
            b = ctypes.c_double()
            _check(lib().spk_model_plan_step_bytes(self.handle, B, T, i, ctypes.byref(b)), 'spk_model_plan_step_bytes')
            out.append(b.value)
        return out

    def _workspace(self, need: int) -> torch.Tensor:
        """The calling stream's workspace (grown on demand).  run_graph stages the inputs
        into the workspace and replays the graph captured for its address, so two forwards
        in flight on different streams must not share one: each stream gets its own.  A
        handle is still not safe for concurrent forwards on ONE stream from several threads
        (they would be serialised on the stream but share the staging space)."""
        key = _stream(self.device)
        ws = self._ws_by_stream.get(key)
        if ws is None or ws.numel() < need:
            if ws is not None and self._ws is ws:
                self._ws = None                 # free the old block before the larger one
            self._ws_by_stream.pop(key, None)
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            self._ws_by_stream[key] = ws
        return ws

    def forward_timed(self, feats: torch.Tensor, out: torch.Tensor):
        """forward() with a HIP event around every plan step; returns per-step ms."""
        B, T, _ = feats.shape
        n = len(self.plan(B, T))
        ms = (ctypes.c_float * n)()
        with torch.cuda.device(self.device):
            self._ws = self._workspace(self.workspace_bytes(B, T))
            _check(lib().spk_model_forward_timed(self.handle, feats.data_ptr(), B, T, self._ws.data_ptr(),
                                                 self._ws.numel(), out.data_ptr(), _stream(self.device), ms, n),
                   'spk_model_forward_timed')
        return list(ms)

    def workspace_bytes_lengths(self, B: int, T: int, ragged: bool) -> int:
        n = ctypes.c_size_t()
        _check(lib().spk_model_workspace_bytes_lengths(self.handle, B, T, int(ragged), ctypes.byref(n)),
               'spk_model_workspace_bytes_lengths')
        return n.value

    def forward(self, feats: torch.Tensor, out: Optional[torch.Tensor] = None, lengths=None) -> torch.Tensor:
        """``lengths`` (optional): valid frames per row (variable-length batch, CAM++)."""
        require_device_tensor(feats, 'embedding forward')
        if feats.device != self.device:
            raise HipError(f'model handle lives on {self.device}, input on {feats.device}')
        if feats.dim() != 3:
            raise HipError(f'expected feats [B, T, F], got {tuple(feats.shape)}')
        feats = feats.to(torch.float32).contiguous()
        B, T, _ = feats.shape
        if lengths is not None:
            lengths = torch.as_tensor(lengths, dtype=torch.int32).to(self.device).contiguous()
            if lengths.numel() != B:
                raise HipError(f'lengths has {lengths.numel()} entries for a batch of {B}')
            # a length past T would read the next utterance's rows (and past the workspace
            # for the last one); CAM++'s unbiased std needs >= 2 frames
            lo = 2 if self.arch == ARCH_CAMPPLUS else 1
            mn, mx = (int(v) for v in torch.aminmax(lengths))
            if mn < lo or mx > T:
                raise HipError(f'lengths must lie in [{lo}, T={T}] (got min {mn}, max {mx})')
        with torch.cuda.device(self.device):
            need = self.workspace_bytes(B, T) if lengths is None else self.workspace_bytes_lengths(B, T, True)
            self._ws = self._workspace(need)
            if out is None:
                out = torch.empty((B, self.embed_dim), dtype=torch.float32, device=self.device)
            if lengths is None:
                _check(lib().spk_model_forward(self.handle, feats.data_ptr(), B, T, self._ws.data_ptr(),
                                               self._ws.numel(), out.data_ptr(), _stream(self.device)),
                       'spk_model_forward')
            else:
                _check(lib().spk_model_forward_lengths(self.handle, feats.data_ptr(), B, T, lengths.data_ptr(),
                                                       self._ws.data_ptr(), self._ws.numel(), out.data_ptr(),
                                                       _stream(self.device)),
                       'spk_model_forward_lengths')
            # the fp16x3 range guard resolves on the device (include/spk_hip.h): no host sync
            self._last = (B, T, int(lengths is not None), self._ws, _stream(self.device))
        return out

    @property
    def last_forward_flagged(self) -> bool:
        """Whether an activation of the last forward reached the fp16x3 range limit (its range
        word is set; synchronises that forward's stream; diagnostics)."""
        if self._last is None:
            return False
        B, T, ragged, ws, stream = self._last
        flag = ctypes.c_int32(0)
        with torch.cuda.device(self.device):
            _check(lib().spk_model_range_check(self.handle, B, T, ragged, ws.data_ptr(), stream, ctypes.byref(flag)),
                   'spk_model_range_check')
        return bool(flag.value)

    @property
    def last_forward_exact(self) -> bool:
        """Whether the last forward was recomputed on the exact-fp32 kernels because an
        activation reached fp16's range: its word is set and its plan has an exact twin
        (ECAPA / CAM++ plans scale the split operands instead and have none)."""
        if not self.last_forward_flagged:
            return False
        B, T, ragged = self._last[:3]
        return self.guard_plan(B, T, bool(ragged))['twin_segments'] > 0

    def guard_plan(self, B: int, T: int, ragged: bool = False) -> dict:
        """How the guarded forward of shape (B, T) is cut into range-guard segments and how
        many exact-plan launches are enqueued behind it (include/spk_hip.h spk_model_guard_plan)."""
        vals = [ctypes.c_int32(0) for _ in range(3)]
        _check(lib().spk_model_guard_plan(self.handle, B, T, int(ragged), *[ctypes.byref(v) for v in vals]),
               'spk_model_guard_plan')
        return dict(zip(('segments', 'twin_segments', 'gated_steps'), (v.value for v in vals)))


class HipModuleMixin:
    """Mixin for the drop-in nn.Modules: lazily builds one native handle per device from
    the module's own state_dict and drops it whenever weights are reloaded or moved."""

    _hip_arch: int = 0

    def _hip_config(self) -> dict:  # pragma: no cover - overridden
        raise NotImplementedError

    def _hip_reset(self, *args, **kwargs):
        self.__dict__['_hip_handles'] = {}

    def set_hip_precision(self, precision: str):
        """'fp32' (default): fp32-accurate forward (fp16x3 split products), embeddings within
        1e-4 of the reference.  'fp16': one fp16 MFMA product per multiply with fp32
        accumulation -- the reduced-precision mode of BASELINE config C3 (cosine >= 0.9999 to
        the reference); layers without a single-product kernel stay fp16x3."""
        if precision not in PRECISIONS:
            raise HipError(f'precision must be one of {sorted(PRECISIONS)}, got {precision!r}')
        self.__dict__['_hip_precision'] = precision
        self._hip_reset()
        return self

    def _hip_handle(self, device: torch.device) -> NativeModel:
        handles = self.__dict__.setdefault('_hip_handles', {})
        key = (device.type, device.index)
        h = handles.get(key)
        if h is None:
            h = NativeModel(self._hip_arch, self._hip_config(), self.state_dict(), device,
                            self.__dict__.get('_hip_precision', 'fp32'))
            handles[key] = h
        return h

    def _hip_forward(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        require_device_tensor(x, type(self).__name__ + '.forward')
        if self.training:
            raise HipError(f'{type(self).__name__}: the MI355X path is inference-only; call .eval()')
        dev = x.device if x.device.index is not None else torch.device('cuda', torch.cuda.current_device())
        return self._hip_handle(dev).forward(x, lengths=lengths)

    def _apply(self, fn, *args, **kwargs):
        self._hip_reset()
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._hip_reset()
        return super()._load_from_state_dict(*args, **kwargs)


def cosine_affinity(a: torch.Tensor, b: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """[Na, E] x [Nb, E] -> [Na, Nb] cosine similarity on the GPU (sklearn semantics)."""
    require_device_tensor(a, 'cosine_affinity')
    b = a if b is None else b
    a = a.to(torch.float32).contiguous()
    b = b.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _check(lib().spk_cosine_affinity(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1],
                                         out.data_ptr(), out.stride(0), _stream(a.device)), 'spk_cosine_affinity')
    return out


def cosine_topk(a: torch.Tensor, b: torch.Tensor, k: int = 1, self_offset: Optional[int] = None,
                threshold: float = float('inf')):
    """Row-block consumer of the cosine affinity (the [Na, Nb] matrix is never written): for
    every row of ``a`` the ``k`` best (score, column) pairs over ``b`` -- score descending,
    column ascending on ties, column ``i + self_offset`` of row ``i`` excluded when
    ``self_offset`` is given -- and the number of columns scoring >= ``threshold``.
    Returns (scores [Na, k] float32, index [Na, k] int64, count [Na] int64)."""
    require_device_tensor(a, 'cosine_topk')
    b = a if b is None else b
    a = a.to(torch.float32).contiguous()
    b = b.to(torch.float32).contiguous()
    if not 1 <= k <= 8:
        raise HipError('cosine_topk: k must be in 1..8')
    Na, Nb, E = a.shape[0], b.shape[0], a.shape[1]
    dev = a.device
    scores = torch.empty((Na, k), dtype=torch.float32, device=dev)
    index = torch.empty((Na, k), dtype=torch.int64, device=dev)
    count = torch.empty(Na, dtype=torch.int64, device=dev)
    nbytes = ctypes.c_size_t(0)
    _check(lib().spk_cosine_topk_workspace_bytes(Na, Nb, ctypes.byref(nbytes)), 'spk_cosine_topk_workspace_bytes')
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=dev)
    c = spk_affinity_consumer_t(SPK_CONSUME_TOPK, k, 0 if self_offset is None else 1,
                                0 if self_offset is None else int(self_offset), float(threshold), scores.data_ptr(),
                                index.data_ptr(), count.data_ptr(), ws.data_ptr(), nbytes.value)
    with torch.cuda.device(dev):
        _check(lib().spk_cosine_topk(a.data_ptr(), Na, b.data_ptr(), Nb, E, ctypes.byref(c), _stream(dev)),
               'spk_cosine_topk')
    return scores, index, count


def cosine_trials(a: torch.Tensor, b: torch.Tensor, ia: torch.Tensor, ib: torch.Tensor) -> torch.Tensor:
    """scores[t] = cosine(a[ia[t]], b[ib[t]]) on the device (compute_score_metrics.py:102-118)."""
    require_device_tensor(a, 'cosine_trials')
    a = a.to(torch.float32).contiguous()
    b = b.to(torch.float32).contiguous()
    ia = ia.to(device=a.device, dtype=torch.int64).contiguous()
    ib = ib.to(device=a.device, dtype=torch.int64).contiguous()
    if ia.numel() and (int(ia.min()) < 0 or int(ia.max()) >= a.shape[0] or int(ib.min()) < 0
                       or int(ib.max()) >= b.shape[0]):
        raise HipError('cosine_trials: trial index out of range')
    out = torch.empty(ia.numel(), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _check(lib().spk_cosine_trials(a.data_ptr(), b.data_ptr(), a.shape[1], ia.data_ptr(), ib.data_ptr(),
                                       ia.numel(), out.data_ptr(), _stream(a.device)), 'spk_cosine_trials')
    return out


def spectral_laplacian(S: torch.Tensor, n_elems: int) -> torch.Tensor:
    """p-pruned, symmetrised unnormalised Laplacian of an N x N affinity (device)."""
    require_device_tensor(S, 'spectral_laplacian')
    S = S.to(torch.float32).contiguous()
    N = S.shape[0]
    L = torch.empty_like(S)
    ws = torch.empty(N * N, dtype=torch.float32, device=S.device)
    with torch.cuda.device(S.device):
        _check(lib().spk_spectral_laplacian(S.data_ptr(), N, S.stride(0), max(0, int(n_elems)), L.data_ptr(),
                                            L.stride(0), ws.data_ptr(), ws.numel() * 4, _stream(S.device)),
               'spk_spectral_laplacian')
    return L


def symmetric_eig(A: torch.Tensor):
    """(eigenvalues ascending [N], eigenvectors as ROWS [N, N]) of a symmetric device matrix;
    A is overwritten."""
    require_device_tensor(A, 'symmetric_eig')
    if A.dtype != torch.float32 or not A.is_contiguous():
        raise HipError('symmetric_eig: float32 contiguous matrix expected')
    N = A.shape[0]
    w = torch.empty(N, dtype=torch.float32, device=A.device)
    with torch.cuda.device(A.device):
        _check(lib().spk_symmetric_eig(A.data_ptr(), N, A.stride(0), w.data_ptr(), _stream(A.device)),
               'spk_symmetric_eig')
    return w, A


# ----------------------------------------------------------------------------- AHC
_ahc_ws: Dict = {}   # (device index, stream handle) -> workspace, grown on demand like the models'


def ahc_workspace_bytes(n: int) -> int:
    """Bytes of workspace ``spk_ahc_average`` needs for an n x n affinity (about 8 n^2: the fp64
    working matrix); raises HipError with ``.code == E_UNSUPPORTED`` above the library's cap."""
    nbytes = ctypes.c_size_t(0)
    _check(lib().spk_ahc_workspace_bytes(int(n), ctypes.byref(nbytes)), 'spk_ahc_workspace_bytes')
    return nbytes.value


def ahc_average(S: torch.Tensor, threshold: float, return_count: bool = False):
    """Average-linkage AHC of an N x N cosine affinity on the device: merge the two clusters with
    the largest average similarity until it is below ``threshold`` (cluster.py:139-156).  Returns
    int32 [N] device labels numbered by first occurrence (with ``return_count`` also the int32 [1]
    device cluster count).  ``S`` may be a view with a row stride above N; it is not modified."""
    require_device_tensor(S, 'ahc_average')
    if S.dim() != 2 or S.shape[0] != S.shape[1]:
        raise HipError(f'ahc_average: expected a square affinity, got {tuple(S.shape)}')
    if S.dtype != torch.float32 or S.stride(1) != 1 or S.stride(0) < S.shape[0]:
        S = S.to(torch.float32).contiguous()
    N = S.shape[0]
    dev = S.device if S.device.index is not None else torch.device('cuda', torch.cuda.current_device())
    if N == 0:
        out = torch.empty(0, dtype=torch.int32, device=dev)
        return (out, torch.zeros(1, dtype=torch.int32, device=dev)) if return_count else out
    need = ahc_workspace_bytes(N)
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        key = (dev.index, _stream(dev))
        ws = _ahc_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = _ahc_ws.pop(key, None)   # free the old block before the larger one
            del ws
            ws = _ahc_ws[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        _check(lib().spk_ahc_average(S.data_ptr(), N, S.stride(0), float(threshold), labels.data_ptr(),
                                     count.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), 'spk_ahc_average')
    return (labels, count) if return_count else labels


def ahc_batched_max_n() -> int:
    """Largest N of a problem ``ahc_average_batched`` takes (``SPK_AHC_BATCH_MAX_N``)."""
    return int(lib().spk_ahc_batched_max_n())


def ahc_average_batched(list_of_S, thresholds):
    """``ahc_average`` of several affinities in one call (``spk_ahc_average_batched``: one workgroup
    per problem, the whole merge loop in one launch).  ``list_of_S``: square device affinities on
    one device, each N in [1, ``ahc_batched_max_n()``]; ``thresholds``: one float, or one per
    problem.  Returns (labels, counts): a list of int32 [N_p] device tensors, each what
    ``ahc_average`` gives for that problem alone, and the int32 [n] device cluster counts.  The
    fp64 working matrices (8 N_p^2 bytes each) share the cached workspace of ``ahc_average``."""
    mats = list(list_of_S)
    n = len(mats)
    thr = [float(thresholds)] * n if not hasattr(thresholds, '__len__') else [float(t) for t in thresholds]
    if len(thr) != n:
        raise HipError(f'ahc_average_batched: {n} affinities, {len(thr)} thresholds')
    if n == 0:
        return [], torch.zeros(0, dtype=torch.int32, device='cuda' if torch.cuda.is_available() else 'cpu')
    for i, S in enumerate(mats):
        require_device_tensor(S, 'ahc_average_batched')
        if S.dim() != 2 or S.shape[0] != S.shape[1] or S.shape[0] < 1:
            raise HipError(f'ahc_average_batched: expected square affinities, got {tuple(S.shape)}')
        if S.device != mats[0].device:
            raise HipError('ahc_average_batched: the affinities must be on one device')
        if S.dtype != torch.float32 or S.stride(1) != 1 or S.stride(0) < S.shape[0]:
            mats[i] = S.to(torch.float32).contiguous()
    dev = _dev_of(mats[0])
    sizes = (ctypes.c_int64 * n)(*[S.shape[0] for S in mats])
    need = ctypes.c_size_t(0)
    _check(lib().spk_ahc_average_batched_workspace_bytes(sizes, n, ctypes.byref(need)),
           'spk_ahc_average_batched_workspace_bytes')
    need = max(need.value, 8)
    labels = [torch.empty(S.shape[0], dtype=torch.int32, device=dev) for S in mats]
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        key = (dev.index, _stream(dev))
        ws = _ahc_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = _ahc_ws.pop(key, None)   # free the old block before the larger one
            del ws
            ws = _ahc_ws[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        _check(lib().spk_ahc_average_batched(
            (_P * n)(*[S.data_ptr() for S in mats]), sizes, (ctypes.c_int64 * n)(*[S.stride(0) for S in mats]),
            (ctypes.c_float * n)(*thr), n, (_P * n)(*[t.data_ptr() for t in labels]), counts.data_ptr(),
            ws.data_ptr(), ws.numel(), _stream(dev)), 'spk_ahc_average_batched')
    return labels, counts


def ahc_release_workspace():
    """Drop the cached AHC workspaces (8 N^2 bytes of the largest N clustered per stream)."""
    _ahc_ws.clear()


# ----------------------------------------------------------------------------- score normalisation
_cohort_ws: Dict = {}   # (device index, stream handle) -> workspace, grown on demand like the AHC's


def _dev_of(t: torch.Tensor) -> torch.device:
    return t.device if t.device.index is not None else torch.device('cuda', torch.cuda.current_device())


def topk_stats(S: torch.Tensor, k: int, out=None):
    """(mean, std) float32 [rows] device tensors: mean and population standard deviation (ddof 0)
    of the ``k`` largest entries of every row of ``S`` (spk_topk_stats; exact selection, ties
    across the cut cannot change the result, the same input gives the same bits).  ``S`` may be a
    view with a row stride above its width: only its own columns are read.  ``out``: a (mean, std)
    pair of contiguous float32 [rows] device tensors (or views) to write into."""
    require_device_tensor(S, 'topk_stats')
    if S.dim() != 2:
        raise HipError(f'topk_stats: expected a matrix, got {tuple(S.shape)}')
    rows, cols = S.shape
    if S.dtype != torch.float32 or (cols > 1 and S.stride(1) != 1) or (rows > 1 and S.stride(0) < cols):
        S = S.to(torch.float32).contiguous()
    lds = S.stride(0) if rows > 1 else max(cols, 1)
    dev = _dev_of(S)
    if out is None:
        mean = torch.empty(rows, dtype=torch.float32, device=dev)
        std = torch.empty(rows, dtype=torch.float32, device=dev)
    else:
        mean, std = out
        for t in (mean, std):
            require_device_tensor(t, 'topk_stats')
            if t.dtype != torch.float32 or t.shape != (rows,) or not t.is_contiguous():
                raise HipError('topk_stats: out must be two contiguous float32 [rows] tensors')
    with torch.cuda.device(dev):
        _check(lib().spk_topk_stats(S.data_ptr(), rows, cols, lds, int(k), mean.data_ptr(), std.data_ptr(),
                                    _stream(dev)), 'spk_topk_stats')
    return mean, std


def cosine_cohort_stats_workspace_bytes(n: int, nc: int):
    """(smallest, recommended) workspace bytes of ``spk_cosine_cohort_stats`` for n rows against a
    cohort of nc: one block of 128 rows of scores, and blocks of about 128 MiB."""
    lo, rec = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(lib().spk_cosine_cohort_stats_workspace_bytes(int(n), int(nc), ctypes.byref(lo), ctypes.byref(rec)),
           'spk_cosine_cohort_stats_workspace_bytes')
    return lo.value, rec.value


def cosine_cohort_stats(x: torch.Tensor, cohort: torch.Tensor, k: int, workspace_bytes: Optional[int] = None):
    """(mean, std) float32 [N] device tensors of the ``k`` best cosine scores of every row of ``x``
    [N, E] against ``cohort`` [Nc, E] (spk_cosine_cohort_stats): the affinity is produced and
    reduced in row blocks inside a cached workspace, never as a whole.  ``workspace_bytes`` overrides
    the recommended workspace size (any size from the smallest up gives the same bits)."""
    require_device_tensor(x, 'cosine_cohort_stats')
    require_device_tensor(cohort, 'cosine_cohort_stats')
    if x.dim() != 2 or cohort.dim() != 2 or x.shape[1] != cohort.shape[1]:
        raise HipError(f'cosine_cohort_stats: expected [N, E] and [Nc, E], got {tuple(x.shape)} and '
                       f'{tuple(cohort.shape)}')
    dev = _dev_of(x)
    x = x.to(torch.float32).contiguous()
    cohort = cohort.to(device=dev, dtype=torch.float32).contiguous()
    N, Nc, E = x.shape[0], cohort.shape[0], x.shape[1]
    mean = torch.empty(N, dtype=torch.float32, device=dev)
    std = torch.empty(N, dtype=torch.float32, device=dev)
    if N == 0:
        return mean, std
    need = cosine_cohort_stats_workspace_bytes(N, Nc)[1] if workspace_bytes is None else int(workspace_bytes)
    with torch.cuda.device(dev):
        key = (dev.index, _stream(dev))
        ws = _cohort_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = _cohort_ws.pop(key, None)   # free the old block before the larger one
            del ws
            ws = _cohort_ws[key] = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        _check(lib().spk_cosine_cohort_stats(x.data_ptr(), N, cohort.data_ptr(), Nc, E, int(k), mean.data_ptr(),
                                             std.data_ptr(), ws.data_ptr(), need, _stream(dev)),
               'spk_cosine_cohort_stats')
    return mean, std


def cohort_release_workspace():
    """Drop the cached cohort-statistics workspaces (up to about 128 MiB per stream)."""
    _cohort_ws.clear()


def cosine_trials_norm(a: torch.Tensor, b: torch.Tensor, ia: torch.Tensor, ib: torch.Tensor, stats_a, stats_b):
    """Normalised trial scores (spk_cosine_trials_norm): with s = cosine(a[ia[t]], b[ib[t]]), the
    bits ``cosine_trials`` gives, and ``stats_a`` = (mean, std) over the rows of ``a``, ``stats_b``
    over those of ``b`` (``cosine_cohort_stats``),
    0.5 * ((s - mean_a) / max(std_a, 1e-6) + (s - mean_b) / max(std_b, 1e-6)) in float32."""
    require_device_tensor(a, 'cosine_trials_norm')
    dev = _dev_of(a)
    a = a.to(torch.float32).contiguous()
    b = b.to(device=dev, dtype=torch.float32).contiguous()
    ia = ia.to(device=dev, dtype=torch.int64).contiguous()
    ib = ib.to(device=dev, dtype=torch.int64).contiguous()
    if ia.numel() != ib.numel():
        raise HipError('cosine_trials_norm: ia and ib differ in length')
    if ia.numel() and (int(ia.min()) < 0 or int(ia.max()) >= a.shape[0] or int(ib.min()) < 0
                       or int(ib.max()) >= b.shape[0]):
        raise HipError('cosine_trials_norm: trial index out of range')
    st = []
    for (m, s), n in ((stats_a, a.shape[0]), (stats_b, b.shape[0])):
        m = torch.as_tensor(m).to(device=dev, dtype=torch.float32).contiguous()
        s = torch.as_tensor(s).to(device=dev, dtype=torch.float32).contiguous()
        if m.shape != (n,) or s.shape != (n,):
            raise HipError('cosine_trials_norm: statistics must be (mean [rows], std [rows]) of each side')
        st += [m, s]
    out = torch.empty(ia.numel(), dtype=torch.float32, device=dev)
    if ia.numel() == 0:
        return out
    with torch.cuda.device(dev):
        _check(lib().spk_cosine_trials_norm(a.data_ptr(), b.data_ptr(), a.shape[1], ia.data_ptr(), ib.data_ptr(),
                                            ia.numel(), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
                                            st[3].data_ptr(), out.data_ptr(), _stream(dev)), 'spk_cosine_trials_norm')
    return out


# ----------------------------------------------------------------------------- pair-cosine statistics
PAIR_MAX_ROWS = 32768         # largest group (kPairMaxRows)
PAIR_FUSED_MAX_ROWS = 4096    # largest group without a cosine array (kPairFusedMaxRows)
PairStats = collections.namedtuple('PairStats', ['cos', 'min', 'mean', 'argmin', 'n_below', 'pair_offsets'])


def pair_cosine_sizes(offsets):
    """Prefix sums of the pair counts n (n - 1) / 2 of the groups ``offsets`` delimits (G + 1 row
    offsets starting at 0): where each group's condensed cosines start in ``pair_cosine_stats``'s
    ``cos`` (spk_pair_cosine_sizes; host arithmetic, no GPU needed)."""
    offs = [int(v) for v in offsets]
    if not offs:
        raise _invalid('pair_cosine_sizes: offsets needs at least the leading 0')
    G = len(offs) - 1
    out = (ctypes.c_int64 * (G + 1))()
    _check(lib().spk_pair_cosine_sizes((ctypes.c_int64 * (G + 1))(*offs), G, out), 'spk_pair_cosine_sizes')
    return list(out)


def pair_cosine_stats(X: torch.Tensor, offsets, threshold: float, want_cos: bool = True) -> PairStats:
    """Statistics of the pair cosines inside every group of rows of ``X`` (spk_pair_cosine_stats).

    ``X``: [N, E] float32 device tensor (a view with a row stride above E is read in place when the
    stride is a multiple of 4); ``offsets``: G + 1 host integers, group g is rows
    ``offsets[g]:offsets[g + 1]``.  Returns ``PairStats`` of device tensors: ``cos`` float32, every
    group's pair cosines in ``np.triu_indices(n, 1)`` order back to back (None without
    ``want_cos``), ``min`` / ``mean`` float32 [G], ``argmin`` int64 [G] (condensed index inside the
    group, smallest among equals, -1 below two rows), ``n_below`` int64 [G] (cosines strictly below
    ``threshold``), and ``pair_offsets``, the host list of where each group starts in ``cos``.  A
    cosine has the bits ``cosine_trials`` gives for the two rows; a group's results have the same
    bits alone and in any batch, with and without ``want_cos``.  A view the kernels cannot read in
    place (a row stride that is no multiple of 4, rows that are not 16-byte aligned, another dtype)
    is copied first.  Without ``want_cos`` the library takes groups of up to
    ``PAIR_FUSED_MAX_ROWS`` rows; for a larger one the cosines go to a scratch array here and are
    dropped (the same statistics)."""
    require_device_tensor(X, 'pair_cosine_stats')
    if X.dim() != 2:
        raise _invalid(f'pair_cosine_stats: expected [N, E], got {tuple(X.shape)}')
    dev = _dev_of(X)
    N, E = int(X.shape[0]), int(X.shape[1])
    if X.dtype != torch.float32 or (N and (X.stride(1) != 1 or X.stride(0) < E or X.stride(0) % 4
                                           or X.data_ptr() % 16)):
        X = X.to(torch.float32).contiguous()
        if X.data_ptr() % 16:
            X = X.clone()               # contiguous already, but off a 16-byte boundary: a fresh block
    ldx = int(X.stride(0)) if N > 1 else E
    offs = [int(v) for v in offsets]
    if not offs or offs[-1] > N:
        raise _invalid(f'pair_cosine_stats: offsets must start at 0 and end within the {N} rows of X')
    G = len(offs) - 1
    po = pair_cosine_sizes(offs)
    with_cos = want_cos or any(b - a > PAIR_FUSED_MAX_ROWS for a, b in zip(offs, offs[1:]))
    cos = torch.empty(po[-1], dtype=torch.float32, device=dev) if with_cos else None
    mn = torch.empty(G, dtype=torch.float32, device=dev)
    mean = torch.empty(G, dtype=torch.float32, device=dev)
    argmin = torch.empty(G, dtype=torch.int64, device=dev)
    below = torch.empty(G, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _check(lib().spk_pair_cosine_stats(X.data_ptr() if N else None, ldx, E, (ctypes.c_int64 * (G + 1))(*offs), G,
                                           float(threshold), cos.data_ptr() if with_cos and po[-1] else None,
                                           mn.data_ptr() if G else None, mean.data_ptr() if G else None,
                                           argmin.data_ptr() if G else None, below.data_ptr() if G else None,
                                           _stream(dev)), 'spk_pair_cosine_stats')
    return PairStats(cos if want_cos else None, mn, mean, argmin, below, po)


def pair_cosine_plan(offsets, with_cos: bool = True) -> dict:
    """The launches ``pair_cosine_stats`` makes for these row offsets (spk_pair_cosine_plan; host
    arithmetic, no GPU needed): ``pair_launches`` and ``stats_launches``, ``max_launch_pairs`` (the
    most pairs one pair launch covers; a pair takes a wave of 64 work-items and a grid holds fewer
    than 2^32) and ``planned_pairs`` (the pairs all pair launches cover together)."""
    offs = [int(v) for v in offsets]
    if not offs:
        raise _invalid('pair_cosine_plan: offsets needs at least the leading 0')
    vals = [ctypes.c_int64() for _ in range(4)]
    _check(lib().spk_pair_cosine_plan((ctypes.c_int64 * len(offs))(*offs), len(offs) - 1, int(bool(with_cos)),
                                      *[ctypes.byref(v) for v in vals]), 'spk_pair_cosine_plan')
    return dict(zip(('pair_launches', 'stats_launches', 'max_launch_pairs', 'planned_pairs'), (v.value for v in vals)))


# ----------------------------------------------------------------------------- corpus similarity statistics
_sim_ws: Dict = {}   # (device index, stream handle) -> (workspace, state), grown on demand like the cohort's


def cosine_sim_workspace_bytes(n: int):
    """(smallest, recommended, state) bytes of the corpus similarity entries for n rows: one block of
    128 rows of scores, blocks of about 128 MiB, and the triangle entries' device state."""
    lo, rec, st = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(lib().spk_cosine_sim_workspace_bytes(int(n), ctypes.byref(lo), ctypes.byref(rec), ctypes.byref(st)),
           'spk_cosine_sim_workspace_bytes')
    return lo.value, rec.value, st.value


def _sim_buffers(dev, n: int, workspace_bytes):
    """The cached (workspace, its size to pass, state) of the current stream of ``dev``."""
    _, rec, st_bytes = cosine_sim_workspace_bytes(n)
    need = rec if workspace_bytes is None else int(workspace_bytes)
    key = (dev.index, _stream(dev))
    ws, st = _sim_ws.get(key, (None, None))
    if ws is None or ws.numel() < need or st.numel() < st_bytes:
        _sim_ws.pop(key, None)   # free the old blocks before the larger ones
        del ws, st
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        st = torch.empty(st_bytes, dtype=torch.uint8, device=dev)
        _sim_ws[key] = (ws, st)
    return ws, need, st


def sim_release_workspace():
    """Drop the cached similarity-statistics workspaces (up to about 128 MiB per stream)."""
    _sim_ws.clear()


def _sim_input(x: torch.Tensor, what: str):
    require_device_tensor(x, what)
    if x.dim() != 2 or x.shape[0] < 1:
        raise _invalid(f'{what}: expected [N, E] with N >= 1, got {tuple(x.shape)}')
    return x.to(torch.float32).contiguous(), _dev_of(x)


def cosine_rows_topk(x: torch.Tensor, k: int, workspace_bytes: Optional[int] = None) -> dict:
    """Per row of the cosine matrix of ``x`` [N, E] against itself, over the other columns
    (spk_cosine_rows_topk; the matrix is produced and consumed in row blocks, never as a whole):
    ``top_scores`` [N, k] float32 and ``top_index`` [N, k] int64, score descending then column
    ascending, -inf / -1 where N - 1 < k; ``sum``, ``sumsq`` float64 [N]; ``min``, ``max``, ``self``
    float32 [N].  Device tensors.  k in 1..1024."""
    x, dev = _sim_input(x, 'cosine_rows_topk')
    N, E = x.shape
    out = dict(top_scores=torch.empty((N, int(k)) if k > 0 else (N, 0), dtype=torch.float32, device=dev),
               top_index=torch.empty((N, int(k)) if k > 0 else (N, 0), dtype=torch.int64, device=dev),
               sum=torch.empty(N, dtype=torch.float64, device=dev), sumsq=torch.empty(N, dtype=torch.float64, device=dev),
               min=torch.empty(N, dtype=torch.float32, device=dev), max=torch.empty(N, dtype=torch.float32, device=dev),
               self=torch.empty(N, dtype=torch.float32, device=dev))
    with torch.cuda.device(dev):
        ws, need, _ = _sim_buffers(dev, N, workspace_bytes)
        _check(lib().spk_cosine_rows_topk(x.data_ptr(), N, E, int(k), out['top_scores'].data_ptr(),
                                          out['top_index'].data_ptr(), out['sum'].data_ptr(), out['sumsq'].data_ptr(),
                                          out['min'].data_ptr(), out['max'].data_ptr(), out['self'].data_ptr(),
                                          ws.data_ptr(), need, _stream(dev)), 'spk_cosine_rows_topk')
    return out


def cosine_triu_stats(x: torch.Tensor, thresholds=(), ranks=(), n_ext: int = 0, nbins: int = 0, edges=None,
                      workspace_bytes: Optional[int] = None) -> dict:
    """Statistics of the P = N (N - 1) / 2 pairs i < j of the cosine matrix of ``x`` [N, E] against
    itself (spk_cosine_triu_stats, then spk_cosine_triu_hist when a histogram or extreme pairs are
    asked for; at most five passes over the scores, which are never stored).  Numpy results:
    ``count``, ``sum``, ``sumsq`` (float64), ``min``, ``max`` (float32), ``count_ge`` int64 per
    threshold (float32 compares), ``order_stats`` float32 at the 0-based ascending ``ranks``;
    with ``nbins`` > 0 ``hist`` int64 over ``edges`` (float64 [nbins + 1]; default
    ``np.linspace(float64 min, float64 max, nbins + 1)``, widened by 0.5 either way when min == max as
    numpy does), bin b holding edges[b] <= s < edges[b + 1] and the last bin closed; with ``n_ext``
    > 0 ``most`` and ``least``: (scores float32, i int64, j int64) of the min(n_ext, P) largest pairs,
    score descending then (i, j) ascending, and the smallest, score ascending then (i, j) ascending.
    Synchronises the stream."""
    import numpy as np
    x, dev = _sim_input(x, 'cosine_triu_stats')
    N, E = x.shape
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
    rk = np.ascontiguousarray(np.asarray(ranks, dtype=np.int64).reshape(-1))
    n_ext, nbins = int(n_ext), int(nbins)
    count = np.zeros(1, np.int64)
    sums = np.zeros(2, np.float64)
    mm = np.zeros(2, np.float32)
    count_ge = np.zeros(max(len(thr), 1), np.int64)
    order = np.zeros(max(len(rk), 1), np.float32)
    cut = np.zeros(2, np.float32)
    take = np.zeros(2, np.int32)
    ptr = lambda a: a.ctypes.data
    with torch.cuda.device(dev):
        ws, need, st = _sim_buffers(dev, N, workspace_bytes)
        _check(lib().spk_cosine_triu_stats(x.data_ptr(), N, E, ptr(thr) if len(thr) else None, len(thr),
                                           ptr(rk) if len(rk) else None, len(rk), n_ext, ptr(count), ptr(sums),
                                           ptr(sums) + 8, ptr(mm), ptr(mm) + 4, ptr(count_ge), ptr(order), ptr(cut),
                                           ptr(take), ws.data_ptr(), need, st.data_ptr(), st.numel(), _stream(dev)),
               'spk_cosine_triu_stats')
        out = dict(count=int(count[0]), sum=float(sums[0]), sumsq=float(sums[1]), min=mm[0], max=mm[1],
                   count_ge=count_ge[:len(thr)].copy(), order_stats=order[:len(rk)].copy())
        if nbins <= 0 and n_ext <= 0:
            return out
        if nbins > 0:
            if edges is None:
                lo, hi = (float(mm[0]), float(mm[1])) if count[0] else (0.0, 1.0)
                if lo == hi:
                    lo, hi = lo - 0.5, hi + 0.5
                edges = np.linspace(lo, hi, nbins + 1)
            edges = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
            if len(edges) != nbins + 1:
                raise _invalid(f'cosine_triu_stats: {nbins} bins need {nbins + 1} edges, got {len(edges)}')
            out['edges'] = edges
        hist = np.zeros(max(nbins, 1), np.int64)
        es = np.zeros((2, max(n_ext, 1)), np.float32)
        ei = np.zeros((2, max(n_ext, 1)), np.int64)
        ej = np.zeros((2, max(n_ext, 1)), np.int64)
        found = np.zeros(2, np.int32)
        _check(lib().spk_cosine_triu_hist(x.data_ptr(), N, E, ptr(edges) if nbins > 0 else None, max(nbins, 0), n_ext,
                                          ptr(cut), ptr(take), ptr(hist), ptr(es), ptr(ei), ptr(ej), ptr(found),
                                          ws.data_ptr(), need, st.data_ptr(), st.numel(), _stream(dev)),
               'spk_cosine_triu_hist')
    if nbins > 0:
        out['hist'] = hist[:nbins].copy()
    if n_ext > 0:
        out['most'] = tuple(a[0, :found[0]].copy() for a in (es, ei, ej))
        out['least'] = tuple(a[1, :found[1]].copy() for a in (es, ei, ej))
    return out


# ----------------------------------------------------------------------------- all-pairs verification statistics
_verif_ws: Dict = {}   # (device index, stream handle) -> (workspace, state), grown on demand like _sim_ws


def cosine_verif_workspace_bytes(n: int):
    """(smallest, recommended, state) bytes of the verification entries for n rows: the workspace as
    for the corpus similarity statistics, and these entries' own device state."""
    lo, rec, st = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(lib().spk_cosine_verif_workspace_bytes(int(n), ctypes.byref(lo), ctypes.byref(rec), ctypes.byref(st)),
           'spk_cosine_verif_workspace_bytes')
    return lo.value, rec.value, st.value


def _verif_buffers(dev, n: int, workspace_bytes):
    """The cached (workspace, its size to pass, state) of the current stream of ``dev``."""
    _, rec, st_bytes = cosine_verif_workspace_bytes(n)
    need = rec if workspace_bytes is None else int(workspace_bytes)
    key = (dev.index, _stream(dev))
    ws, st = _verif_ws.get(key, (None, None))
    if ws is None or ws.numel() < need or st.numel() < st_bytes:
        _verif_ws.pop(key, None)   # free the old blocks before the larger ones
        del ws, st
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        st = torch.empty(st_bytes, dtype=torch.uint8, device=dev)
        _verif_ws[key] = (ws, st)
    return ws, need, st


def verif_release_workspace():
    """Drop the cached verification-statistics workspaces (up to about 128 MiB per stream)."""
    _verif_ws.clear()


def _verif_input(x: torch.Tensor, labels: torch.Tensor, what: str):
    x, dev = _sim_input(x, what)
    require_device_tensor(labels, what)
    if labels.dim() != 1 or labels.shape[0] != x.shape[0] or labels.dtype not in (torch.int32, torch.int64):
        raise _invalid(f'{what}: labels must be an integer tensor of shape [{x.shape[0]}], got '
                       f'{labels.dtype} {tuple(labels.shape)}')
    return x, labels.to(device=dev, dtype=torch.int32).contiguous(), dev


def cosine_verif_moments(x: torch.Tensor, labels: torch.Tensor, edges=None, workspace_bytes: Optional[int] = None) -> dict:
    """Per-class statistics of the pairs i < j of the cosine matrix of ``x`` [N, E] against itself
    (spk_cosine_verif_moments; one pass, the scores are never stored).  Class 1 holds the pairs with
    ``labels[i] == labels[j]``, class 0 the others.  Numpy results indexed by class: ``count`` int64 [2],
    ``sum``, ``sumsq`` float64 [2], ``min``, ``max`` float32 [2] (NaN for an empty class), and with
    ``edges`` (float64 [nbins + 1], nbins <= 256) ``hist`` int64 [2, nbins] with the bins of
    ``cosine_triu_stats``.  Synchronises the stream."""
    import numpy as np
    x, labels, dev = _verif_input(x, labels, 'cosine_verif_moments')
    N, E = x.shape
    nbins = 0
    if edges is not None:
        edges = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
        nbins = len(edges) - 1
        if nbins < 1:
            raise _invalid('cosine_verif_moments: edges need at least two values')
    count = np.zeros(2, np.int64)
    sums = np.zeros((2, 2), np.float64)
    mm = np.zeros((2, 2), np.float32)
    hist = np.zeros((2, max(nbins, 1)), np.int64)
    ptr = lambda a: a.ctypes.data
    with torch.cuda.device(dev):
        ws, need, st = _verif_buffers(dev, N, workspace_bytes)
        _check(lib().spk_cosine_verif_moments(x.data_ptr(), labels.data_ptr(), N, E, ptr(edges) if nbins else None, nbins,
                                              ptr(count), ptr(sums[0]), ptr(sums[1]), ptr(mm[0]), ptr(mm[1]),
                                              ptr(hist) if nbins else None, ws.data_ptr(), need, st.data_ptr(),
                                              st.numel(), _stream(dev)), 'spk_cosine_verif_moments')
    out = dict(count=count, sum=sums[0].copy(), sumsq=sums[1].copy(), min=mm[0].copy(), max=mm[1].copy())
    if nbins:
        out['edges'] = edges
        out['hist'] = hist
    return out


def cosine_verif_digits(x: torch.Tensor, labels: torch.Tensor, level: int, prefixes=(0,),
                        workspace_bytes: Optional[int] = None):
    """int64 [n_prefix, 2, 256]: entry [p, c, d] counts the class-c pairs i < j of ``x`` whose 32-bit
    score key agrees with ``prefixes[p]`` in its top ``level`` bytes (0..3) and whose next byte is d
    (spk_cosine_verif_digits; one pass, up to 16 prefixes, one empty prefix at level 0).  The
    primitive of speakerlab/utils/verification_analysis.py.  Synchronises the stream."""
    import numpy as np
    x, labels, dev = _verif_input(x, labels, 'cosine_verif_digits')
    N, E = x.shape
    pre = np.ascontiguousarray(np.asarray(prefixes, dtype=np.uint32).reshape(-1))
    out = np.zeros((max(len(pre), 1), 2, 256), np.int64)
    with torch.cuda.device(dev):
        ws, need, st = _verif_buffers(dev, N, workspace_bytes)
        _check(lib().spk_cosine_verif_digits(x.data_ptr(), labels.data_ptr(), N, E, int(level),
                                             pre.ctypes.data if len(pre) else None, len(pre), out.ctypes.data,
                                             ws.data_ptr(), need, st.data_ptr(), st.numel(), _stream(dev)),
               'spk_cosine_verif_digits')
    return out
