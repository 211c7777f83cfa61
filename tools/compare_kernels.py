#!/usr/bin/env python3
"""
Compare the device code of two builds of the library, function by function.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC --offload-device-only -S -o before.s badread_amd/csrc/brx_hip.hip
    (the same on the other tree: after.s)
    python tools/compare_kernels.py before.s after.s

A refactor of the host side, or one that moves kernels between headers, changes the order in which the functions are emitted and
nothing else.  So the files are split by symbol: a function's text runs from its `.type SYM,@function` to its `.size SYM`, a kernel's
descriptor from `.amdhsa_kernel SYM` to `.end_amdhsa_kernel` (registers, LDS, scratch, ...).  Local labels (.LBB12_3, .Lfunc_end12,
.Ltmp7, and BB12_3 in the comments on loops) carry the function's ordinal in the file, so inside one function they are renumbered
in order of first appearance.  Everything else is compared as text, byte for byte.  Exit status 0 and one line when both builds
hold the same symbols with the same text.
"""
import re
import sys

TYPE = re.compile(r'^\s*\.type\s+(\S+),@function')
SIZE = re.compile(r'^\s*\.size\s+(\S+),')
KERNEL = re.compile(r'^\s*\.amdhsa_kernel\s+(\S+)')
LOCAL = re.compile(r'\.L[A-Za-z_]+[0-9_]*|\bBB[0-9]+_[0-9]+')


def renumber(lines):
    names = {}
    return [LOCAL.sub(lambda m: names.setdefault(m.group(0), '.L%d' % len(names)), line) for line in lines]


def split(path):
    """{symbol: text} of the functions and {symbol: text} of the kernel descriptors"""
    funcs, descs = {}, {}
    name = kernel = None
    body, desc = [], []
    with open(path) as f:
        for line in f:
            if name is None:
                m = TYPE.match(line)
                if m:
                    name, body = m.group(1), []
                continue
            body.append(line)                                # a kernel's descriptor lies inside its function's .type ... .size
            if kernel is not None:
                desc.append(line)
                if line.strip() == '.end_amdhsa_kernel':
                    descs[kernel], kernel = ''.join(desc), None
            elif KERNEL.match(line):
                kernel, desc = KERNEL.match(line).group(1), []
            elif SIZE.match(line) and SIZE.match(line).group(1) == name:
                funcs[name], name = ''.join(renumber(body)), None
    return funcs, descs


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    (fa, da), (fb, db) = split(argv[1]), split(argv[2])
    bad = []
    for what, a, b in (('function', fa, fb), ('kernel descriptor', da, db)):
        for sym in sorted(set(a) | set(b)):
            if sym not in a or sym not in b:
                bad.append('%s %s: only in %s' % (what, sym, argv[1] if sym in a else argv[2]))
            elif a[sym] != b[sym]:
                bad.append('%s %s: differs' % (what, sym))
    for line in bad:
        print(line)
    print('%d kernels, %d device functions in all: %s' % (len(da), len(fa), '%d differences' % len(bad) if bad else 'identical text and descriptors'))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
