"""Host check of the whole-N halo form's LDS layout (csrc/halo_whole_n.h, no GPU): the compact
fragment addressing fetches the operands of the padded layout over all lanes, steps, taps and
blocks for 52 and 50 real channels, every ds_read_b128 lane group stays on distinct banks, and
the header's static_assert holds the LDS total at or below 160 KB.  tests/halo_layout_check.cpp
is compiled with the host compiler against the very header the kernel includes."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), '3d-speaker_amd', 'csrc')


def test_compact_addressing_matches_padded_layout(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = str(tmp_path / 'halo_layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-I', CSRC, os.path.join(HERE, 'halo_layout_check.cpp'), '-o', exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.startswith('ok ')
