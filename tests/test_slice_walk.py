"""The bracket rule of the slice proposal (nnest_amd/csrc/slice_walk.h: the state machine every device kernel runs) on the CPU, bit
for bit in float32 against the oracle's loop form (oracle.slice_bracket), with every branch of the rule reached by construction.
The header is plain C++, so the test compiles it with the host compiler, as nnest_host.o is built."""
import ctypes
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STEPOUT = (0, 1, 2, 8)
MAX_SHRINK = (1, 3, 32)
CASES = 400
MIN_REACHED = 10


@pytest.fixture(scope='module')
def walk(tmp_path_factory):
    """tests/slice_walk_host.cpp as a shared library (no host compiler: the test fails, it does not skip)"""
    so = str(tmp_path_factory.mktemp('slice_walk') / 'libslice_walk_host.so')
    cxx = os.environ.get('CXX') or 'c++'
    cmd = [cxx, '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-fPIC', '-shared', '-I', os.path.join(ROOT, 'nnest_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'slice_walk_host.cpp'), '-o', so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and 'warning' not in r.stdout, '%s\n%s' % (' '.join(cmd), r.stdout)
    lib = ctypes.CDLL(so)
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    lib.slice_walk_update.argtypes = [fp, ctypes.c_int, dp, dp, ctypes.c_int, ctypes.c_int, fp, ctypes.c_int, fp, ctypes.POINTER(ctypes.c_int)]
    lib.slice_walk_update.restype = ctypes.c_int

    def run(u, ivs, max_stepout, max_shrink):
        u = np.ascontiguousarray(u, np.float32)
        lo = np.array([a for a, _ in ivs], np.float64)
        hi = np.array([b for _, b in ivs], np.float64)
        cap = 4 * max_stepout + max_shrink + 8   # (full step-out <= 2 B + 2, split <= B + 2, shrinkage <= max_shrink evaluations)
        cand, out, moved = np.full(cap, np.nan, np.float32), np.zeros(2, np.float32), ctypes.c_int(-1)
        n = lib.slice_walk_update(u.ctypes.data_as(fp), len(ivs), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), max_stepout, max_shrink,
                                  cand.ctypes.data_as(fp), cap, out.ctypes.data_as(fp), ctypes.byref(moved))
        assert 0 < n <= cap
        return cand[:n], out, bool(moved.value)
    return run


def cases():
    """seeded: per (max_stepout, max_shrink) 400 slices and uniform sets.  The slice is 1-3 open intervals in t, the first
    (-10^a, 10^b), a, b ~ U(-2, 1.5), so that it holds t = 0, the others (c, c + 10^w), c ~ U(-12, 12), w ~ U(-1, 0.7); the uniforms
    are 24-bit fractions, as noise_uniform's; every seventh case has u_63 = 0, the next u_63 = 1 - 2^-24 (the ends of the split)."""
    rng = np.random.RandomState(0)
    for m in MAX_STEPOUT:
        for ms in MAX_SHRINK:
            for trial in range(CASES):
                ivs = [(-10 ** rng.uniform(-2, 1.5), 10 ** rng.uniform(-2, 1.5))]
                for _ in range(rng.randint(0, 3)):
                    c = rng.uniform(-12, 12)
                    ivs.append((c, c + 10 ** rng.uniform(-1, 0.7)))
                u = (rng.randint(0, 1 << 24, size=64).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
                if trial % 7 == 0:
                    u[63] = np.float32(0.0)
                if trial % 7 == 1:
                    u[63] = np.float32(1.0 - 2.0 ** -24)
                yield m, ms, ivs, u


def test_state_machine_equals_the_loop_form_bit_for_bit_and_every_branch_is_reached(walk):
    reached, n_cases, bad = Counter(), 0, []
    for m, ms, ivs, u in cases():
        ref = orc.slice_bracket(lambda t: any(lo < float(t) < hi for lo, hi in ivs), u, m, ms)
        cand, bracket, moved = walk(u, ivs, m, ms)
        n_cases += 1
        rc = np.array(ref['candidates'], np.float32)
        same = (len(cand) == len(rc) and cand.tobytes() == rc.tobytes() and moved == ref['moved']
                and bracket.tobytes() == np.array([ref['tl'], ref['tr']], np.float32).tobytes())
        if not same:
            bad.append((m, ms, n_cases - 1, len(cand), len(rc)))
        # which branches of the rule the case takes, read off the REFERENCE alone
        B = 2 * m
        if m == 0:
            reached[m, 'no step-out'] += 1
            assert ref['n_left'] == ref['n_right'] == 0 and not ref['split']
        elif not ref['split']:
            reached[m, 'full step-out within budget'] += 1
            assert ref['n_left'] + ref['n_right'] <= B
        else:
            nl = orc.slice_stepout_split(u[63], m)[0]
            reached[m, 'budget exceeded, nl = 0' if nl == 0 else 'budget exceeded, nl = B' if nl == B else 'budget exceeded, 0 < nl < B'] += 1
            assert ref['n_left'] <= nl and ref['n_right'] <= B - nl
        reached[m, 'moved' if ref['moved'] else 'shrinkage exhausted'] += 1
        reached[(m, ms), 'moved' if ref['moved'] else 'shrinkage exhausted'] += 1
    assert n_cases == len(MAX_STEPOUT) * len(MAX_SHRINK) * CASES
    assert not bad, '%d of %d cases differ, first (max_stepout, max_shrink, case, n_eval, n_eval_ref): %s' % (len(bad), n_cases, bad[:5])
    want = [(m, b) for m in MAX_STEPOUT for b in ('moved', 'shrinkage exhausted')] + [(0, 'no step-out')]
    want += [(m, b) for m in MAX_STEPOUT if m > 0 for b in ('full step-out within budget', 'budget exceeded, nl = 0',
                                                            'budget exceeded, 0 < nl < B', 'budget exceeded, nl = B')]
    want += [((m, ms), 'moved') for m in MAX_STEPOUT for ms in MAX_SHRINK]
    want += [((m, 1), 'shrinkage exhausted') for m in MAX_STEPOUT]   # (32 draws are never exhausted on slices this wide)
    short = {k: reached[k] for k in want if reached[k] < MIN_REACHED}
    assert not short, 'branches reached fewer than %d times: %s' % (MIN_REACHED, short)
    assert reached[0, 'no step-out'] == len(MAX_SHRINK) * CASES


def test_split_of_the_budget_matches_the_oracle_at_every_24_bit_end(walk):
    """u_63 = m / 2^24: the header's integer split against the oracle's float64 floor, at the values where floor(v (B + 1)) steps"""
    for max_stepout in (1, 2, 8, 1 << 24):
        B = 2 * max_stepout
        for j in sorted(set([0, 1, B // 2, B - 1, B])):
            for dm in (-1, 0, 1):
                mm = min(max(-(-(j << 24) // (B + 1)) + dm, 0), (1 << 24) - 1)   # the first m with floor(m (B + 1) / 2^24) = j, and its neighbours
                v = np.float32(mm * 2.0 ** -24)
                nl = orc.slice_stepout_split(v, max_stepout)[0]
                assert nl == min(B, (mm * (B + 1)) >> 24)
                # through the header: a slice nothing leaves, so the full step-out exceeds any budget; count the split's left steps
                if max_stepout <= 8:
                    u = np.zeros(64, np.float32)
                    u[0], u[2], u[63] = 0.5, 0.5, v
                    cand, _, moved = walk(u, [(-1e9, 1e9)], max_stepout, 1)
                    left = cand[B + 1:-1]   # behind the B + 1 candidates of the full step-out, in front of the shrinkage draw
                    assert moved and int(np.sum(left < 0)) == nl and len(left) == B, (max_stepout, mm)
