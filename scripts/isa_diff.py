#!/usr/bin/env python
"""Compares the gfx950 kernels of two sets of assembly listings, for refactors that must not change a kernel's instructions.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S old/loss.hip -o old.s          # one listing per unit, before and after
    python scripts/isa_diff.py --old old.s --new loss.s loss_up.s score_up.s label_up.s [--alias OLD_NAME=NEW_NAME]

Per kernel of the old listings (by mangled name; --alias for one whose name had to change) the text from its label to its
.Lfunc_end and its .amdhsa_kernel block are compared after local labels (.LBB<n>_<m>, .Lfunc_end<n>, .L__unnamed..) are renumbered
per function, and the kernel's own name and the names of function-local LDS variables are replaced by placeholders.  One line per kernel:
name, VGPRs / AGPRs / scratch bytes / LDS bytes, `equal` or `DIFFERENT`.  A kernel listed more than once among the new
listings (a template instantiated in two units) must be equal in each.  Exit status 1 on any difference or missing kernel."""
import argparse
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: (normalised text, normalised .amdhsa_kernel block, (vgpr, agpr, scratch, lds))} of one listing"""
    lines = open(path).read().split('\n')
    names = [m.group(1) for m in (re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln) for ln in lines) if m]
    out = {}
    for name in names:
        i0 = next(i for i, ln in enumerate(lines) if ln.startswith(name + ':'))
        i1 = next(i for i in range(i0, len(lines)) if re.match(r'\.Lfunc_end\d+:', lines[i]))
        k0 = next(i for i in range(i0, i1) if re.match(r'\s*\.amdhsa_kernel\s', lines[i]))       # the listing puts the block before .Lfunc_end
        k1 = next(i for i in range(k0, i1) if '.end_amdhsa_kernel' in lines[i])
        res = {}
        for ln in lines[i1:i1 + 60]:
            m = re.match(r';\s*(NumVgprs|NumAgprs|ScratchSize|LDSByteSize):\s*(\d+)', ln)
            if m:
                res.setdefault(m.group(1), int(m.group(2)))
        out.setdefault(name, []).append((_norm(lines[i0:k0] + lines[k1 + 1:i1 + 1], name), _norm(lines[k0:k1 + 1], name),
                                         tuple(res.get(k) for k in ('NumVgprs', 'NumAgprs', 'ScratchSize', 'LDSByteSize'))))
    return out


def _norm(lines, name):
    text = '\n'.join(re.sub(r'\s*;.*$', '', ln) for ln in lines).replace(name, '<kernel>')
    seen = {}
    text = re.sub(r'\.L(?:BB|func_end|tmp|__unnamed_)\d+(?:_\d+)?', lambda m: seen.setdefault(m.group(0), '.L%d' % len(seen)), text)
    lds = {}
    return re.sub(r'_ZZ\w+', lambda m: lds.setdefault(m.group(0), '<lds%d>' % len(lds)), text)


def demangle(name):
    try:
        return subprocess.run(['c++filt', name], capture_output=True, text=True, check=True).stdout.strip().replace('(anonymous namespace)::', '')
    except Exception:
        return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--old', nargs='+', required=True)
    ap.add_argument('--new', nargs='+', required=True)
    ap.add_argument('--alias', action='append', default=[])
    a = ap.parse_args()
    alias = dict(x.split('=') for x in a.alias)
    old, new = {}, {}
    for side, paths in ((old, a.old), (new, a.new)):
        for p in paths:
            for k, v in kernels(p).items():
                side.setdefault(k, []).extend(v)
    bad = 0
    for name, (ref,) in sorted(old.items(), key=lambda kv: demangle(kv[0])):
        got = new.pop(alias.get(name, name), None)
        same = got is not None and all(g[:2] == ref[:2] for g in got)
        bad += not same
        short = re.sub(r'\(.*', '', demangle(name).replace('void ', ''))
        print('%-58s vgpr %3d agpr %3d scratch %3d lds %5d  %s%s' % ((short,) + ref[2] + (
            'missing' if got is None else 'equal' if same else 'DIFFERENT', ' (in %d units)' % len(got) if got and len(got) > 1 else '')))
    for name in sorted(new):
        bad += 1
        print('%-58s only in the new listings' % demangle(name))
    print('%d kernels, %d differ' % (len(old), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
