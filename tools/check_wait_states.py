#!/usr/bin/env python3
"""Static check of the hand-placed wait states of the gfx950 kernels (developer tool; tests/test_solo_wait_states.py runs it).

Inline asm is not padded by hipcc: a wait state missing inside a string gives wrong values on some waves and no fault.  This
tool disassembles every gfx950 kernel of an object file or shared library (as tools/disasm_kernel.py does), follows each
kernel's control flow and reports every (producer, consumer) pair that is closer than the hardware allows, for the rules the
one-walker-per-wave bodies (solo_tile.h) rely on:

  rule          producer                          consumer                                               states between
  dpp           VALU write of a VGPR              DPP read of it (src0: the operand that is permuted)    2
  permlane      VALU write of a VGPR              v_permlane16_swap / v_permlane32_swap operand          2
  readlane      VALU write of a VGPR              v_readlane / v_readfirstlane source                    1
  trans         v_exp / v_log / v_rcp / v_rsq /   any other (non-transcendental) VALU read of the        1
                v_sqrt / v_sin / v_cos result     result
  exec-dpp      VALU write of EXEC (v_cmpx)       any DPP instruction                                    5

`s_nop N` counts N + 1 states, every other instruction one.  The accumulator of a v_fmac_f32_dpp and the destination a
row-masked v_mov_b32_dpp leaves untouched are ordinary register reads, not DPP reads.

Control flow: a kernel is cut into basic blocks at branch targets and behind branches; the state at a block's entry is the
worst (smallest distance) over all its predecessors, iterated to a fixed point, so a window that spans a branch or a loop's
back edge is checked against every way into the block -- nothing is assumed about a path.  A block entered through a
computed jump (s_setpc / s_swappc) counts every register as just written.

  python tools/check_wait_states.py nnest_amd/libnnest_hip.so [name-substring ...]     exit status 1 if there are findings
  python tools/check_wait_states.py --listing kernel.s                                 a text listing (llvm-objdump -d format)"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import code_objects  # noqa: E402

OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'
FAR = 8          # distances are capped here: beyond every rule
TRANS = re.compile(r'^v_(exp|log|rcp|rsq|sqrt|sin|cos)(_iflag|_legacy|_clamp)?_(f16|f32|f64)')
ACCUMULATING = re.compile(r'^v_(fmac|mac|pk_fmac|dot\w*c)_')   # the destination is also a source
BRANCH = re.compile(r'^s_(branch|cbranch_\w+)$')
REG = re.compile(r'\bv(\d+)\b|\bv\[(\d+):(\d+)\]')


class Ins:
    __slots__ = ('addr', 'op', 'ops', 'text', 'target')

    def __init__(self, addr, text):
        self.addr, self.text = addr, text
        head, _, rest = text.partition(' ')
        self.op = head
        # operands are comma separated; modifiers (row_ror:8, op_sel_hi:[1,0], offset:16 ...) follow the last one behind a blank
        ops = [o.strip().split(' ')[0] for o in rest.split(',')] if rest.strip() else []
        self.ops = ops
        self.target = None


def vregs(operand):
    out = []
    for m in REG.finditer(operand):
        if m.group(1) is not None:
            out.append(int(m.group(1)))
        else:
            out.extend(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def parse_listing(body):
    """llvm-objdump -d lines of one kernel -> [Ins].  Lines without an address comment get consecutive addresses."""
    out, addr = [], 0
    for line in body.split('\n'):
        code, _, comment = line.partition('//')
        code = code.strip()
        if not code or code.startswith('<') or code.endswith(':'):
            continue
        m = re.match(r'\s*([0-9A-Fa-f]+):', comment)
        addr = int(m.group(1), 16) if m else addr + 4
        ins = Ins(addr, re.sub(r'\s+', ' ', code))
        if BRANCH.match(ins.op) and ins.ops:
            try:
                off = int(ins.ops[0], 0)
                ins.target = addr + 4 + 4 * (off - 65536 if off >= 32768 else off)
            except ValueError:
                ins.target = -1   # symbolic target: unknown
        out.append(ins)
    return out


def is_valu(op):
    return op.startswith('v_') and op not in ('v_nop',)


def effects(ins):
    """(vgprs written by a VALU, writes EXEC, reads {vgpr: kinds}) of one instruction"""
    op, ops = ins.op, ins.ops
    if not is_valu(op):
        return [], False, {}
    dpp = ' row_' in ins.text or 'quad_perm' in ins.text or ' wave_' in ins.text or ' row_bcast' in ins.text or op.endswith('_dpp')
    swap = op.startswith('v_permlane16_swap') or op.startswith('v_permlane32_swap')
    lane = op.startswith('v_readlane') or op.startswith('v_readfirstlane')
    both = swap or op.startswith('v_swap_')          # both operands are read and written
    writes = [] if lane or not ops else vregs(ops[0]) + (vregs(ops[1]) if both and len(ops) > 1 else [])
    wexec = op.startswith('v_cmpx') or (bool(ops) and ops[0].startswith('exec'))
    reads = {}
    first_src = 0 if both or ACCUMULATING.match(op) else 1   # (the destination of an accumulating form is read as well)
    for k in range(first_src, len(ops)):
        for r in vregs(ops[k]):
            kinds = reads.setdefault(r, set())
            kinds.add('valu')
            if swap:
                kinds.add('permlane')
            if lane:
                kinds.add('readlane')
            if dpp and k == 1:
                kinds.add('dpp')
    return writes, wexec, {'regs': reads, 'dpp': dpp, 'trans': bool(TRANS.match(op))}


def states_of(ins):
    if ins.op == 's_nop' and ins.ops:
        return int(ins.ops[0], 0) + 1
    return 1


def step(state, ins, report):
    """state: {reg or 'exec': (distance, producer Ins, producer is transcendental)}; distance = wait states between"""
    writes, wexec, rd = effects(ins)
    if rd:
        for r, kinds in rd['regs'].items():
            if r not in state:
                continue
            d, prod, ptrans = state[r]
            need, rule = 0, None
            if 'dpp' in kinds and 2 > need:
                need, rule = 2, 'dpp'
            if 'permlane' in kinds and 2 > need:
                need, rule = 2, 'permlane'
            if 'readlane' in kinds and 1 > need:
                need, rule = 1, 'readlane'
            if ptrans and not rd['trans'] and 1 > need:
                need, rule = 1, 'trans'
            if d < need and report is not None:
                report.append((rule, need, d, 'v%d' % r, prod, ins))
        if rd['dpp'] and 'exec' in state and state['exec'][0] < 5 and report is not None:
            report.append(('exec-dpp', 5, state['exec'][0], 'exec', state['exec'][1], ins))
    n = states_of(ins)
    new = {}
    for r, (d, prod, pt) in state.items():
        if d + n < FAR:
            new[r] = (d + n, prod, pt)
    for r in writes:
        new[r] = (0, ins, bool(TRANS.match(ins.op)))
    if wexec:
        new['exec'] = (0, ins, False)
    return new


def merge(a, b):
    """worst case of two entry states; None = not reached yet"""
    if a is None:
        return dict(b), True
    changed = False
    for r, v in b.items():
        if r not in a or v[0] < a[r][0] or (v[0] == a[r][0] and v[2] and not a[r][2]):
            a[r] = v
            changed = True
    return a, changed


def check_kernel(insns):
    """-> findings [(rule, needed, found, register, producer Ins, consumer Ins)]"""
    if not insns:
        return []
    index = {ins.addr: k for k, ins in enumerate(insns)}
    leaders = {0}
    unknown_entry = set()
    for k, ins in enumerate(insns):
        if ins.target is not None:
            if ins.target in index:
                leaders.add(index[ins.target])
            if k + 1 < len(insns):
                leaders.add(k + 1)
        elif ins.op in ('s_endpgm', 's_setpc_b64', 's_swappc_b64', 's_call_b64') and k + 1 < len(insns):
            leaders.add(k + 1)
            if ins.op != 's_endpgm':
                unknown_entry.add(k + 1)
    starts = sorted(leaders)
    blocks = [(s, starts[i + 1] if i + 1 < len(starts) else len(insns)) for i, s in enumerate(starts)]
    block_at = {s: i for i, (s, _) in enumerate(blocks)}
    entry = [None] * len(blocks)
    entry[0] = {}
    everything = None
    for s in unknown_entry:   # entered through a computed jump: every register counts as just written
        if everything is None:
            everything = {r: (0, insns[s - 1], False) for r in range(512)}
        entry[block_at[s]] = dict(everything)
    work = [i for i, e in enumerate(entry) if e is not None]
    while work:
        i = work.pop()
        s, e = blocks[i]
        st = dict(entry[i])
        for k in range(s, e):
            st = step(st, insns[k], None)
        last = insns[e - 1]
        succ = []
        if last.target is not None:
            if last.target in index:
                succ.append(block_at[index[last.target]])
            if last.op != 's_branch' and e < len(insns):
                succ.append(block_at[e])
        elif last.op not in ('s_endpgm', 's_setpc_b64') and e < len(insns):
            succ.append(block_at[e])
        for j in succ:
            entry[j], changed = merge(entry[j], st)
            if changed and j not in work:
                work.append(j)
    report = []
    for i, (s, e) in enumerate(blocks):
        if entry[i] is None:
            continue   # unreachable (padding behind s_endpgm)
        st = dict(entry[i])
        for k in range(s, e):
            st = step(st, insns[k], report)
    seen, out = set(), []
    for f in report:
        key = (f[0], f[3], f[4].addr, f[5].addr)
        if key not in seen:
            seen.add(key)
            out.append(f)
    return out


def kernels_of(path):
    """(demangled name, listing text) of every gfx950 function in an object file / shared library"""
    data = open(path, 'rb').read()
    for co in code_objects(data):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(co)
            f.flush()
            txt = subprocess.run([OBJDUMP, '-d', '--demangle', f.name], capture_output=True, text=True).stdout
        for m in re.finditer(r'^[0-9a-f]+ <(.*?)>:\n(.*?)(?=^\n|\Z)', txt, re.S | re.M):
            if not m.group(1).endswith('.kd'):
                yield m.group(1), m.group(2)


def check_file(path, patterns=()):
    """-> {kernel name: findings} for the kernels whose name contains one of `patterns` (all if none)"""
    out = {}
    for name, body in kernels_of(path):
        if patterns and not any(p in name for p in patterns):
            continue
        out[name] = check_kernel(parse_listing(body))
    return out


def format_finding(name, f):
    rule, need, found, reg, prod, cons = f
    return '%s: %s needs %d state(s), found %d, on %s\n    producer %08x: %s\n    consumer %08x: %s' % (
        name, rule, need, found, reg, prod.addr, prod.text, cons.addr, cons.text)


def main():
    args = sys.argv[1:]
    if not args:
        print(__doc__)
        return 2
    if args[0] == '--listing':
        results = {args[1]: check_kernel(parse_listing(open(args[1]).read()))}
    else:
        results = check_file(args[0], args[1:])
    bad = 0
    for name, fs in results.items():
        for f in fs:
            print(format_finding(name, f))
            bad += 1
    print('%d kernels checked, %d findings' % (len(results), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
