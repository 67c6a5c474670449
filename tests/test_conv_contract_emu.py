"""Every case of tests/conv_cases.py through the host emulation (tests/emu/libspk_emu.so):
the float64 reference (conv_ref.py), the descriptor builder and the emulated ConvDesc
contract (emu_kernels.cpp launch_conv) are three independent statements that must agree,
to c = 1e-6 of the magnitude sum (double accumulation, one rounding).  Runs without a GPU.

Not modelled by the emulation, so not checked here: the kernel name, the split-K partial
slabs (the emulation writes the full sum) and the x1 rounding; the output is checked all
the same."""
import pytest
import torch

import conv_cases
import emu_runner


@pytest.fixture(scope='module')
def backend():
    return conv_cases.Backend(emu_runner.lib(), torch.device('cpu'), emu=True)


@pytest.mark.parametrize('name', [c['name'] for c in conv_cases.CASES])
def test_case_emulated(backend, name):
    conv_cases.run_case(conv_cases.BY_NAME[name], backend)


@pytest.mark.parametrize('name', [r[0] for r in conv_cases.REJECTS])
def test_rejected_descriptor_emulated(backend, name):
    conv_cases.run_reject(name, backend)
