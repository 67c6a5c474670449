"""Every conv kernel route of spk::launch_conv, one launch at a time (csrc/diag_conv.cpp),
against the float64 reference of tests/conv_ref.py: every case of tests/conv_cases.py
asserts the kernel it reached, every output element, that nothing outside the output was
written, the ragged mask and the range word.  The coverage test ties the table to the
kernels the models' launch plans name."""
import re

import pytest
import torch

import conv_cases
import helpers
from speakerlab import _hip

pytestmark = pytest.mark.gpu

_reports = {}
_gpu_error = []   # a HIP error (not a mere mismatch) of an earlier case: nothing more is launched


@pytest.fixture(scope='module')
def backend():
    dev = torch.device('cuda', 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count   # hipDeviceAttributeMultiprocessorCount
    return conv_cases.Backend(_hip.lib(), dev, emu=False, cus=cus)


def _guarded(what, fn):
    if _gpu_error:
        pytest.fail(f'not launched: {_gpu_error[0]}')
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:   # a HIP error from a sync, or conv_cases.LaunchError (rc != 0)
        _gpu_error.append(f'{what} raised {type(e).__name__}: {e}')
        raise


def _run(name, backend):
    if name not in _reports:
        _reports[name] = None   # a failing case is not launched a second time by the coverage test
        _reports[name] = _guarded(name, lambda: conv_cases.run_case(conv_cases.BY_NAME[name], backend))
    return _reports[name]


@pytest.mark.parametrize('name', [c['name'] for c in conv_cases.CASES])
def test_case(backend, name):
    assert _run(name, backend) is not None, f'{name} failed in an earlier run of this session'


@pytest.mark.parametrize('name', [r[0] for r in conv_cases.REJECTS])
def test_rejected_descriptor(backend, name):
    _guarded(name, lambda: conv_cases.run_reject(name, backend))


def test_halo_tile_widths_reached(backend):
    """The tile width is a template argument of the fp16x3 and the persistent halo kernel (the
    tile height is a constant of the instantiation): the table reaches all three of each."""
    widths = {'x3': set(), 'persistent': set()}
    for c in conv_cases.CASES:
        if c['fam'].startswith('halo'):
            try:
                r = _run(c['name'], backend)
            except AssertionError:
                continue   # reported by its own test
            m = r and re.match(r'conv3x3_halo_(x3|persistent)_kernel<\d+, (\d+),', r['kernel'])
            if m:
                widths[m.group(1)].add(int(m.group(2)))
    assert widths == {'x3': {8, 16, 32}, 'persistent': {8, 16, 32}}, widths


def test_table_covers_every_conv_kernel_of_the_models(backend):
    """Every conv kernel name in any model's launch plan has a direct case in the table; the
    names are compared whole, the halo kernels' tile width included."""
    for c in conv_cases.CASES:
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
                    if kernel.startswith(('conv_gemm', 'conv3x3_halo', 'pw_gemm')) and kernel not in have:
                        missing.setdefault(kernel, []).append(f'{arch}/{prec}/B{B}:{step}')
            del m, h
    for k, where in sorted(missing.items()):
        print(f'no direct case reaches {k}: {where[:4]}')
    assert not missing, sorted(missing)
