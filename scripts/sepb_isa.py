#!/usr/bin/env python
"""Per sepb kernel of a compile-only listing: VGPRs, scratch and the opcode histogram of the kernel-row loop of stage 2.

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/sepb.hip -o sepb.s
    python scripts/sepb_isa.py sepb.s [label]

The kernel-row loop is the smallest loop (label ... backward branch) that holds a DPP instruction."""
import collections
import re
import sys


def kernels(lines):
    name, start = None, 0
    for i, ln in enumerate(lines):
        m = re.match(r'^(_ZN\S*sepb\S*):', ln)
        if m:
            name, start = m.group(1), i
        elif name and ln.startswith('.Lfunc_end'):
            yield name, start, i
            name = None


def demangle(n):
    m = re.search(r'(sepb_(?:batch_)?kernel)ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E', n)
    return '%s<%s,%s,%s,%s>' % m.groups()


def row_loop(body):
    pos = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r'^(\.LBB\d+_\d+):', ln)] if m}
    best = None
    for j, ln in enumerate(body):
        m = re.match(r'\s+s_c?branch\S*\s+(\.LBB\d+_\d+)', ln)
        if m and pos.get(m.group(1), j) < j:
            i = pos[m.group(1)]
            if any('_dpp' in b for b in body[i:j]) and (best is None or j - i < best[1] - best[0]):
                best = (i, j + 1)
    return best


def main():
    lines = open(sys.argv[1]).read().split('\n')
    label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
    meta = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)', '\n'.join(lines)):
        meta[m.group(1)] = (int(m.group(3)), int(m.group(2)))
    print('## %s' % label)
    for name, a, b in kernels(lines):
        body = lines[a:b]
        lp = row_loop(body)
        ops = collections.Counter(ln.split()[0] for ln in body[lp[0]:lp[1]] if re.match(r'\s+[a-z]', ln) and not ln.strip().startswith(';'))
        vg, scr = meta.get(name, (-1, -1))
        tot = sum(ops.values())
        valu = sum(n for o, n in ops.items() if o.startswith('v_') and not o.startswith('v_mfma'))
        red = sum(n for o, n in ops.items() if o.endswith('_dpp') or o in ('v_pk_add_f32',))
        print('%-34s VGPRs %3d  scratch %d  row loop: %3d instructions, %3d VALU, reduction VALU %3d, s_nop %2d, v_pk_fma_f32 %2d, ds_read_b128 %2d'
              % (demangle(name), vg, scr, tot, valu, red, ops.get('s_nop', 0), ops.get('v_pk_fma_f32', 0), ops.get('ds_read_b128', 0)))
        print('    ' + '  '.join('%s %d' % kv for kv in sorted(ops.items(), key=lambda kv: (-kv[1], kv[0]))))


if __name__ == '__main__':
    main()
