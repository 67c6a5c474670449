"""Every case of tests/op_cases.py through the host emulation (tests/emu/libspk_emu.so): the
float64 references (op_ref.py), the descriptor builders and the emulated kernel contracts
(emu_kernels.cpp) are three independent statements that must agree.  Runs without a GPU.

Relaxed here, since the emulation does not model them: the kernel names (an `emu_` name is
asserted), the scratch of the CAM gate (the emulation writes no segment sums) and the exact
value of a clamped standard deviation (one ulp: the emulation takes the square root in
double).  split_f16 is bit for bit here too.

The sensitivity test shows that the shapes and bounds discriminate: each deliberately wrong
variant of the reference (op_ref.WRONG) must be rejected by the comparator on at least one
case of every family it concerns."""
import pytest
import torch

import emu_runner
import op_cases
import op_ref


@pytest.fixture(scope='module')
def backend():
    return op_cases.Backend(emu_runner.lib(), torch.device('cpu'), emu=True)


@pytest.mark.parametrize('name', [c['name'] for c in op_cases.CASES])
def test_case_emulated(backend, name):
    op_cases.run_case(op_cases.BY_NAME[name], backend)


@pytest.mark.parametrize('name', [r[0] for r in op_cases.REJECTS])
def test_rejected_descriptor_emulated(backend, name):
    op_cases.run_reject(name, backend)


# the wrong variant -> the families whose reference it changes
SENSITIVITY = [
    ('biased', ['stats_pool', 'tstp']),                     # biased for unbiased std
    ('T_for_Tb', ['time_mean', 'asp_stats']),               # T for Tb in a mean
    ('ignore_vlen', ['time_mean', 'asp_stats', 'attn_pool', 'stats_pool', 'stem_conv3x3', 'cam_context', 'cam_gate']),
    ('seg_off1', ['cam_context', 'cam_gate']),              # a segment boundary off by one
    ('swap_xy', ['aff_x3']),                                # AFF with x and y swapped
    ('drop_tap', ['stem_conv3x3', 'res2_block']),           # one 3x3 tap dropped
    ('halo_bias', ['res2_block']),                          # halo = Hardtanh(bias) outside the image
    ('no_res', ['res2_block', 'se_apply']),                 # the residual omitted
    ('lo_2_10', ['split_f16']),                             # lo plane scale 2^10
]


@pytest.mark.parametrize('wrong,fam', [(w, f) for w, fams in SENSITIVITY for f in fams])
def test_comparator_rejects_a_wrong_reference(backend, wrong, fam):
    rejected = []
    op_ref.WRONG.add(wrong)
    try:
        for c in op_cases.CASES:
            # the large cases add nothing here: the mistake shows at the small shapes or not at all
            if c['fam'] != fam or c.get('n', 0) > 1 << 20 or c.get('M') == 'p_tiles' or c.get('nimg') == 'cus':
                continue
            try:
                op_cases.run_case(c, backend)
            except AssertionError:
                rejected.append(c['name'])
    finally:
        op_ref.WRONG.discard(wrong)
    print(f'{wrong} / {fam}: rejected on {len(rejected)} cases: {rejected[:6]}')
    assert rejected, f'no case of {fam} notices the mistake {wrong!r}'
