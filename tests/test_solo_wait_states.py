"""Static check of the wait states in the hand-scheduled kernel bodies (solo_tile.h), on the CPU.

Inline asm is not padded by hipcc, and a missing wait state shows as wrong values on some waves, not as a fault: a GPU test
that passes is no evidence.  tools/check_wait_states.py walks the disassembly instead.  Here it is first checked against
itself -- fixture listings with a required s_nop shortened or deleted must be reported, compiler-only code must not -- and
then run over the kernels that carry the hand-written bodies: zero findings."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nnest_amd', 'csrc')
FIXTURES = os.path.join(ROOT, 'tests', 'golden', 'wait_states')
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import check_wait_states as cws  # noqa: E402

HAND_SCHEDULED = ('mh_kernel_solo', 'slice_kernel_solo', 'ensemble_kernel', 'train_kernel_rows')
# units whose kernels call no inline asm at all: every instruction and every s_nop in them is hipcc's own
COMPILER_ONLY_UNITS = ('nnest_chol', 'nnest_chain_stats')

def listing(name):
    return cws.parse_listing(open(os.path.join(FIXTURES, name)).read())


def test_fixture_with_all_wait_states_is_clean():
    assert cws.check_kernel(listing('join_ok.s')) == []


@pytest.mark.parametrize('name, rule, reg', [
    ('join_short_swap.s', 'permlane', 'v6'),      # s_nop 1 in front of v_permlane16_swap shortened to s_nop 0
    ('join_no_rcp_wait.s', 'trans', 'v6'),        # the s_nop 0 between v_rcp_f32 and the v_fma_f32 that reads it deleted
    ('join_no_dpp_wait.s', 'dpp', 'v8'),          # the s_nop 0 in front of the first DPP read of the activation deleted
])
def test_fixture_with_a_missing_wait_state_is_reported(name, rule, reg):
    found = cws.check_kernel(listing(name))
    assert [(f[0], f[3]) for f in found] == [(rule, reg)], found
    assert found[0][2] == found[0][1] - 1   # one state short


def test_windows_follow_branches():
    # the producer sits in front of a loop's back edge, the consumer at the loop's head: no path may be assumed away
    text = '\n'.join([
        '\tv_mov_b32_e32 v1, v2                    // 000000001000: 00000000',
        '\ts_nop 1                                 // 000000001004: 00000000',
        '\tv_mov_b32_dpp v3, v1 row_ror:8 row_mask:0xf bank_mask:0xf   // 000000001008: 00000000',
        '\tv_add_f32_e32 v1, v3, v3                // 000000001010: 00000000',
        '\ts_cbranch_scc1 65532                    // 000000001014: 00000000',   # back to 0x1008
        '\ts_endpgm                                // 000000001018: 00000000',
    ])
    found = cws.check_kernel(cws.parse_listing(text))
    assert [(f[0], f[3], f[2]) for f in found] == [('dpp', 'v1', 1)], found


def objects():
    """{unit: path of its object file}: the ones the build left in the source directory, else cross-compiled now"""
    units = ('nnest_solo', 'nnest_ensemble', 'nnest_train') + COMPILER_ONLY_UNITS
    have = {u: os.path.join(CSRC, u + '.o') for u in units}
    if all(os.path.exists(p) for p in have.values()):
        return have, None
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'no built objects and no hipcc to build them'
    import tempfile
    tmp = tempfile.mkdtemp(prefix='nnest_wait_states_')
    out = {}
    for u in units:
        out[u] = os.path.join(tmp, u + '.o')
        subprocess.check_call([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-fno-gpu-rdc', '-Wno-unused-function',
                               '-c', os.path.join(CSRC, u + '.hip'), '-o', out[u]])
    return out, tmp


@pytest.fixture(scope='module')
def built():
    objs, tmp = objects()
    yield objs
    if tmp:
        shutil.rmtree(tmp, ignore_errors=True)


def test_compiler_only_kernels_have_no_findings(built):
    # hipcc pads its own code: a finding here would mean a rule is stated wrong, not that the code is
    n = 0
    for unit in COMPILER_ONLY_UNITS:
        for name, found in cws.check_file(built[unit]).items():
            assert found == [], '\n'.join(cws.format_finding(name, f) for f in found)
            n += 1
    assert n >= 2


def test_hand_scheduled_kernels_have_no_findings(built):
    seen = set()
    for unit in ('nnest_solo', 'nnest_ensemble', 'nnest_train'):
        for name, found in cws.check_file(built[unit], HAND_SCHEDULED).items():
            assert found == [], '\n'.join(cws.format_finding(name, f) for f in found)
            seen.update(k for k in HAND_SCHEDULED if k in name)
    assert seen == set(HAND_SCHEDULED), seen
