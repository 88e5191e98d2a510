"""The solo K4 kernel's barrier schedule (nnest_amd/csrc/solo_schedule.h), on the CPU.

The kernel's three roles -- net waves, noise wave, relay wave -- meet at one workgroup barrier; a role that takes one barrier more or
fewer than the others hangs its workgroup, and on the GPU a hang is all there is to see.  The step ranges of the three loops and the
barriers they add up to are constexpr functions of (S, warm, dynamic, exact_all) in a header of plain C++; tests/solo_schedule_main.cpp
restates each role's loops with those bounds and holds the three lists of barriers against each other and against the header's counts,
for S = 1..40, warm in {0, 1, 16, S - 1, S} (clipped as the kernel clips it), under a fixed step, the lagged batch rule and lag 0.
Built with the host compiler and its address and undefined-behaviour sanitizers where it has them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nnest_amd', 'csrc')
MAIN = os.path.join(ROOT, 'tests', 'solo_schedule_main.cpp')


def build(tmp_path, flags):
    cxx = shutil.which(os.environ.get('CXX', 'g++')) or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = str(tmp_path / 'solo_schedule_check')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-I', CSRC] + flags + [MAIN, '-o', exe], capture_output=True, text=True)
    return exe, r


def test_three_roles_take_the_same_barriers(tmp_path):
    exe, r = build(tmp_path, ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    if r.returncode != 0:   # (a host compiler without the sanitizers' runtimes: the plain build checks the same counts)
        exe, r = build(tmp_path, [])
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith('600 cases, 0 failures'), run.stdout[-400:]


def test_kernel_takes_its_bounds_from_the_header():
    """the three loops of mh_kernel_solo are bounded by the header's functions, not by expressions of their own"""
    src = open(os.path.join(CSRC, 'nnest_solo.hip')).read()
    assert '#include "solo_schedule.h"' in src
    for call in ('solo_warm_steps(S, mh_flag_warm(a.flags), dynamic, exact_all)', 'solo_first_lagged_fetch(warm)',
                 'solo_relay_first_iteration(warm)', 'solo_first_straight_step(warm)'):
        assert call in src, call
