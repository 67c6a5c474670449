"""TEST INFRASTRUCTURE: ctypes binding of the diagnostics entry csrc/diag_conv.cpp
(spk_diag_conv: one spk::launch_conv from a plain-C mirror of ConvDesc), for libspk_hip.so
and for the host emulation tests/emu/libspk_emu.so alike.  Pointers are taken from torch
tensors; for the emulation the "device" pointers are host pointers, as in emu_runner.py."""
import ctypes

import torch

_P = ctypes.c_void_p
_I = ctypes.c_int32


class spk_diag_src_t(ctypes.Structure):
    _fields_ = [('p', _P), ('p2', _P), ('ld', _I), ('ld2', _I), ('H', _I), ('W', _I), ('cin', _I),
                ('kh', _I), ('kw', _I), ('sh', _I), ('sw', _I), ('ph', _I), ('pw', _I), ('dh', _I), ('dw', _I),
                ('reflect', _I), ('pre_scale', _P), ('pre_shift', _P), ('vlen', _P)]


class spk_diag_conv_t(ctypes.Structure):
    _fields_ = [('s0', spk_diag_src_t), ('s1', spk_diag_src_t),
                ('nimg', _I), ('Ho', _I), ('Wo', _I), ('N', _I), ('K', _I), ('Kp', _I),
                ('w', _P), ('planes', _I), ('wh', _P), ('wl', _P), ('wf', _P),
                ('bias', _P), ('rowbias', _P), ('rowbias_ld', _I),
                ('out', _P), ('ldo', _I), ('osplit', _I), ('oplane', ctypes.c_int64),
                ('act', _I), ('act2', _I), ('res', _P), ('ldr', _I),
                ('post_scale', _P), ('post_shift', _P),
                ('affx', _P), ('ldx', _I), ('affy', _P), ('ldy', _I),
                ('gate', _P), ('gate_ld', _I), ('gate_seg', _I), ('gate_nseg', _I),
                ('ksplit', _I), ('partial', _P), ('rowlen', _P), ('range_flag', _P),
                ('x1', _I), ('wbig', _I), ('kcb', _I), ('range_in', _P)]


_SRC_INTS = ('ld', 'ld2', 'H', 'W', 'cin', 'kh', 'kw', 'sh', 'sw', 'ph', 'pw', 'dh', 'dw', 'reflect')
_SRC_PTRS = ('p', 'p2', 'pre_scale', 'pre_shift', 'vlen')
_PTRS = ('w', 'wh', 'wl', 'wf', 'bias', 'rowbias', 'out', 'res', 'post_scale', 'post_shift', 'affx', 'affy', 'gate',
         'partial', 'rowlen', 'range_flag', 'range_in')

_bound = {}


def bind(handle):
    """Declare the two diagnostics entries on a loaded library (real or emulated)."""
    if id(handle) not in _bound:
        handle.spk_diag_conv.restype = ctypes.c_int
        handle.spk_diag_conv.argtypes = [ctypes.POINTER(spk_diag_conv_t), ctypes.c_char_p, _I, _P]
        handle.spk_diag_frag_halves.restype = ctypes.c_int
        handle.spk_diag_frag_halves.argtypes = [_I, _I, ctypes.POINTER(ctypes.c_size_t)]
        _bound[id(handle)] = handle
    return handle


def frag_halves(handle, N, Kp):
    n = ctypes.c_size_t()
    rc = bind(handle).spk_diag_frag_halves(N, Kp, ctypes.byref(n))
    if rc != 0:
        raise RuntimeError(f'spk_diag_frag_halves({N}, {Kp}) failed ({rc})')
    return n.value


def _ptr(v):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    return int(v)   # a raw address (the misaligned-pointer cases)


def launch(handle, desc, stream=None):
    """desc: dict of the spk_diag_conv_t fields; 's0' / 's1' are dicts of the source fields,
    pointer fields are torch tensors (or None).  Returns (rc, kernel name, last error)."""
    c = spk_diag_conv_t()
    for side in ('s0', 's1'):
        src = desc.get(side) or {}
        s = getattr(c, side)
        # ConvSrc's defaults (common.h)
        for k in ('H', 'W', 'kh', 'kw', 'sh', 'sw', 'dh', 'dw'):
            setattr(s, k, 1)
        for k, v in src.items():
            if k in _SRC_PTRS:
                setattr(s, k, _ptr(v))
            elif k in _SRC_INTS:
                setattr(s, k, int(v))
            else:
                raise KeyError(k)
    c.ksplit = 1
    for k, v in desc.items():
        if k in ('s0', 's1'):
            continue
        if k in _PTRS:
            setattr(c, k, _ptr(v))
        else:
            getattr(spk_diag_conv_t, k)   # KeyError-like guard against typos
            setattr(c, k, int(v))
    name = ctypes.create_string_buffer(256)
    rc = bind(handle).spk_diag_conv(ctypes.byref(c), name, 256, stream)
    err = handle.spk_last_error()
    return rc, name.value.decode(), (err.decode() if err else '')
