"""Every kernel entry that is not a conv -- the fused AFF, the fused Res2Net block, the TDNN
reductions and the small kernels of misc.h -- one launch at a time (csrc/diag_ops.cpp) against
the float64 references of tests/op_ref.py: every case of tests/op_cases.py asserts the kernel
it reached (where the entry has several), every output element, that nothing outside the
output was written, exact zeros where the contract masks, and the range word.  The coverage
test ties the table to the kernels the models' launch plans name and to the launch functions
the four headers declare.

The online-softmax pools (attn_pool, astp_pool) hold their bound (4 x the fp32 PyTorch
formula's own error + 1 ulp) with no allowance for __expf.  Seven of their cases missed it
before the weighted Welford update was rewritten (astp_pool_span80 by 10.7 x: a std of 3.1e-4
came out as 4.3e-4): when a heavy frame follows light ones, w / sw -> 1, mean + d w / sw rounds
at ulp(d) and xv - new mean cancels to rounding noise.  The kernels now take the new mean from
the nearer end and write xv - new mean = d sw0 / sw out.

Not reached: the grid-stride paths of the lane-per-channel reductions and of se_apply, which
need more than 16.7 M elements in one launch."""
import os
import re

import pytest
import torch

import helpers
import op_cases
from speakerlab import _hip

pytestmark = pytest.mark.gpu

_reports = {}
_gpu_error = []   # a HIP error (not a mere mismatch) of an earlier case: nothing more is launched


@pytest.fixture(scope='module')
def backend():
    dev = torch.device('cuda', 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return op_cases.Backend(_hip.lib(), dev, emu=False, cus=cus)


def _guarded(what, fn):
    if _gpu_error:
        pytest.fail(f'not launched: {_gpu_error[0]}')
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:   # a HIP error from a sync, or LaunchError (rc != 0)
        _gpu_error.append(f'{what} raised {type(e).__name__}: {e}')
        raise


def _run(name, backend):
    if name not in _reports:
        _reports[name] = None   # a failing case is not launched a second time by the coverage test
        _reports[name] = _guarded(name, lambda: op_cases.run_case(op_cases.BY_NAME[name], backend))
    return _reports[name]


@pytest.mark.parametrize('name', [c['name'] for c in op_cases.CASES])
def test_case(backend, name):
    assert _run(name, backend) is not None, f'{name} failed in an earlier run of this session'


@pytest.mark.parametrize('name', [r[0] for r in op_cases.REJECTS])
def test_rejected_descriptor(backend, name):
    _guarded(name, lambda: op_cases.run_reject(name, backend))


def test_every_launch_function_has_a_family():
    """every launch_* that tdnn_ops.h, misc.h, aff.h and res2block.h declare has cases"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), '3d-speaker_amd', 'csrc')
    declared = set()
    for h in ('tdnn_ops.h', 'misc.h', 'aff.h', 'res2block.h'):
        with open(os.path.join(csrc, h)) as f:
            declared |= set(re.findall(r'hipError_t\s+launch_(\w+)\s*\(', f.read()))
    assert len(declared) >= 16, declared
    have = {c['fam'] for c in op_cases.CASES}
    assert declared <= have, sorted(declared - have)


def test_table_covers_every_fused_kernel_of_the_models(backend):
    """Every plan kernel name of any model that starts with aff_x3, res2_block or cam_ is
    reached by a case; the names are compared whole."""
    for c in op_cases.CASES:
        if c['fam'] in ('aff_x3', 'res2_block', 'cam_gate'):
            try:
                _run(c['name'], backend)
            except AssertionError:
                pass   # reported by its own test
    if _gpu_error:
        pytest.fail(f'not launched: {_gpu_error[0]}')
    have = {r['kernel'] for r in _reports.values() if r}
    missing = {}
    for arch in helpers.ARCHS + helpers.VARIANTS:
        for prec in ('fp32', 'fp16'):
            m = helpers.loaded_module(arch).to('cuda').set_hip_precision(prec)
            h = m._hip_handle(backend.device)
            for B, T in ((2, 198), (256, 198)):
                for step, kernel, _ in h.plan(B, T):
                    if kernel.startswith(('aff_x3', 'res2_block', 'cam_')) and kernel not in have:
                        missing.setdefault(kernel, []).append(f'{arch}/{prec}/B{B}:{step}')
            del m, h
    for k, where in sorted(missing.items()):
        print(f'no direct case reaches {k}: {where[:4]}')
    assert not missing, sorted(missing)
