"""TEST INFRASTRUCTURE: ctypes binding of the diagnostics entries of csrc/diag_ops.cpp (one
launch of each kernel entry that is not a conv), for libspk_hip.so and for the host emulation
tests/emu/libspk_emu.so alike.  Pointers are taken from torch tensors; for the emulation the
"device" pointers are host pointers, as in emu_runner.py."""
import ctypes

import torch

P, I, F, Z = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t

# field lists in the order of the structs of csrc/diag_ops.cpp
_LAYOUT = {
    'aff': 'x:P ldx:I y:P ldy:I out:P ldo:I M:I cp:I nmid:I w1:P w1h:P w1l:P b1:P kp1:I w2:P w2h:P w2l:P b2:P kp2:I '
           'range_flag:P',
    'res2': 'x:P out:P nimg:I H:I W:I C:I Cout:I stride:I Hin:I Win:I proj:I width:I w1:P w1h:P w1l:P b1:P '
            'wa:P wah:P wal:P ba:P wb:P wbh:P wbl:P bb:P w3:P w3h:P w3l:P b3:P',
    'time_mean': 'x:P B:I T:I C:I ld:I out:P ldo:I vlen:P',
    'asp_stats': 'x:P B:I T:I C:I ld:I eps:F out:P vlen:P',
    'attn_pool': 'logit:P ldl:I x:P ldx:I B:I T:I C:I eps:F out:P vlen:P',
    'se_apply': 'x:P ldx:I gate:P ldg:I res:P ldr:I out:P ldo:I B:I T:I C:I range_flag:P',
    'cam_context': 'x:P B:I T:I C:I ld:I seg:I nseg:I out:P ldo:I vlen:P',
    'cam_gate': 'x:P B:I T:I C:I ld:I seg:I nseg:I w1:P k1p:I b1:P red:I w2:P k2p:I b2:P growth:I gate:P ldg:I '
                'segsum:P vlen:P',
    'stats_pool': 'x:P B:I T:I C:I ld:I out:P vlen:P',
    'derive_len': 'in:P out:P B:I pad:I k:I stride:I',
    'stem': 'feats:P B:I T:I F:I w:P bias:P cout:I act:I wstride:I out:P ldo:I vlen:P range_flag:P',
    'word_reset': 'w:P',
    'range_check': 'x:P n:Z flag:P',
    'split_f16': 'w:P hi:P lo:P n:Z',
    'tstp': 'x:P B:I H:I W:I C:I ld:I eps:F unbiased:I out:P parts:I',
    'astp_pool': 'logit:P ldl:I x:P ldx:I B:I F:I T:I C:I out:P',
}
NAMED = ('aff', 'res2', 'cam_gate')   # entries that report the kernel name
_TYPES = {'P': P, 'I': I, 'F': F, 'Z': Z}
STRUCTS = {}
for _op, _spec in _LAYOUT.items():
    _fields = [(f.split(':')[0], _TYPES[f.split(':')[1]]) for f in _spec.split()]
    STRUCTS[_op] = type(f'spk_diag_{_op}_t', (ctypes.Structure,), {'_fields_': _fields})

_bound = {}


def bind(handle):
    if id(handle) not in _bound:
        for op, st in STRUCTS.items():
            fn = getattr(handle, f'spk_diag_{op}')
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.POINTER(st)] + ([ctypes.c_char_p, I] if op in NAMED else []) + [P]
        handle.spk_last_error.restype = ctypes.c_char_p
        _bound[id(handle)] = handle
    return handle


def _ptr(v):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    return int(v)   # a raw address (the misaligned-pointer cases)


def launch(handle, op, fields, stream=None):
    """fields: dict of the struct's fields (tensors or None for pointers).  Returns
    (rc, kernel name or '', last error)."""
    st = STRUCTS[op]
    c = st()
    known = {n: t for n, t in st._fields_}
    for k, v in fields.items():
        t = known[k]   # KeyError: a typo
        setattr(c, k, _ptr(v) if t is P else (float(v) if t is F else int(v)))
    fn = getattr(bind(handle), f'spk_diag_{op}')
    if op in NAMED:
        name = ctypes.create_string_buffer(256)
        rc = fn(ctypes.byref(c), name, 256, stream)
        kernel = name.value.decode()
    else:
        rc = fn(ctypes.byref(c), stream)
        kernel = ''
    err = handle.spk_last_error()
    return rc, kernel, (err.decode() if err else '')
