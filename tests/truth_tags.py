"""
--truth-tags: the contract of MD:Z: and SA:Z: restated in plain Python (README, "Truth tags"), shared by tests/test_truth_tags.py
(emulated device) and tests/test_gpu_truth_tags.py (MI355X).

The tagged file is a function of the untagged one and the reference's forward strands (`tagged_sam_from`); `tag_cases` counts
how often a file takes each branch of the writer, and `check_properties` checks what must hold of any tagged file without
that function.
"""
import collections
import functools
import re

import numpy as np

TAG_MD, TAG_SA = 1, 2
MASKS = (TAG_MD, TAG_SA, TAG_MD | TAG_SA)

_CIGAR = re.compile(r'(\d+)([MIDSH])')
_MD = re.compile(r'[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*')


def md_of(parts, seq, ref):              # parts: [(n, op)] of the line's CIGAR; seq: its SEQ; ref: forward strand from POS-1, T long
    out, u, q, t = [], 0, 0, 0
    for n, x in parts:
        if x == 'S': q += n
        elif x == 'M':
            for i in range(n):
                if seq[q + i] == ref[t + i]: u += 1
                else: out.append(f'{u}{ref[t + i]}'); u = 0
            q += n; t += n
        elif x == 'I': q += n
        elif x == 'D': out.append(f'{u}^{ref[t:t + n]}'); u = 0; t += n
    return ''.join(out) + str(u)


@functools.lru_cache(maxsize=8192)
def _md_of(parts, seq, ref):             # the masks of one batch ask for the same lines' MD again
    return md_of(parts, seq, ref)


def sa_element(f):                       # f: the fields of one mapped untagged line
    parts = [(int(n), x) for n, x in _CIGAR.findall(f[5])]
    left = parts[0][0] if parts[0][1] in 'SH' else 0
    right = parts[-1][0] if parts[-1][1] in 'SH' else 0
    Q = sum(n for n, x in parts if x in 'MI'); T = sum(n for n, x in parts if x in 'MD')
    gap = f'{Q - T}I' if Q > T else f'{T - Q}D' if T > Q else ''
    cig = (f'{left}S' if left else '') + f'{min(Q, T)}M' + gap + (f'{right}S' if right else '')
    return f"{f[2]},{f[3]},{'-' if int(f[1]) & 16 else '+'},{cig},60,{f[11][5:]};"


def tagged_sam_from(sam, ref_of, md, sa, md_exempt=None):   # sam: untagged record bytes; ref_of(name) -> forward strand (str)
    """`md_exempt`: None, or a dict line index -> MD text to take instead of md_of's (the long-read test, N in the reference slice)."""
    lines = [l.split('\t') for l in sam.decode('latin-1').splitlines()]
    mapped = collections.defaultdict(list)
    for i, f in enumerate(lines):
        if not int(f[1]) & 4: mapped[f[0]].append(i)
    out = []
    for i, f in enumerate(lines):
        extra = []
        if not int(f[1]) & 4:
            parts = [(int(n), x) for n, x in _CIGAR.findall(f[5])]
            T = sum(n for n, x in parts if x in 'MD')
            if md:
                if md_exempt is not None and i in md_exempt: extra.append('MD:Z:' + md_exempt[i])
                else: extra.append('MD:Z:' + _md_of(tuple(parts), f[9], ref_of(f[2])[int(f[3]) - 1:int(f[3]) - 1 + T]))
            mine = mapped[f[0]]
            if sa and len(mine) > 1:
                prim = next(j for j in mine if not int(lines[j][1]) & 2048)
                order = ([prim] if prim != i else []) + [j for j in mine if j not in (i, prim)]
                extra.append('SA:Z:' + ''.join(sa_element(lines[j]) for j in order))
        out.append('\t'.join(f[:13] + extra + f[13:]) + '\n')      # f[11], f[12] = NM, AS; f[13:] = CO on the primary
    return ''.join(out).encode('latin-1')


def str_strands(seqs):
    """name -> forward strand (str), from (name, text) pairs."""
    return dict(seqs).__getitem__


def _tag(f, name):
    for x in f[11:]:
        if x.startswith(name + ':Z:'):
            return x[5:]
    return None


def tag_cases(sam):
    """How often a tagged (MD|SA) record file takes each branch of the tag writers."""
    c = collections.Counter()
    lines = [l.split('\t') for l in sam.decode('latin-1').splitlines()]
    per_read = collections.defaultdict(list)
    for f in lines:
        if not int(f[1]) & 4:
            per_read[f[0]].append(f)
    for name, fs in per_read.items():
        c['reads_2_lines'] += len(fs) >= 2
        c['reads_3_lines'] += len(fs) >= 3
        c['max_lines'] = max(c['max_lines'], len(fs))
        for f in fs:
            md, sa = _tag(f, 'MD'), _tag(f, 'SA')
            if md is not None:
                minus = bool(int(f[1]) & 16)
                c['md_deletion'] += '^' in md
                c['md_long_deletion'] += re.search(r'\^[A-Z]{2,}', md) is not None
                c['md_deletion_minus'] += minus and '^' in md
                c['md_adjacent_mismatches'] += re.search(r'[A-Z]0[A-Z]', md) is not None
                c['md_deletion_then_mismatch'] += re.search(r'\^[A-Z]+0[A-Z]', md) is not None
                c['md_mismatch_then_deletion'] += re.search(r'[A-Z]0\^', md) is not None
                c['md_starts_0'] += re.match(r'0[A-Z^]', md) is not None
                c['md_ends_0'] += re.search(r'[A-Z]0$', md) is not None
                c['md_all_digits'] += md.isdigit()
                c['md_max_len'] = max(c['md_max_len'], len(md))
            if sa is not None:
                els = sa.split(';')[:-1]
                for e in els:
                    cig = e.split(',')[3]
                    c['sa_with_I'] += 'I' in cig
                    c['sa_with_D'] += 'D' in cig
                    c['sa_plain'] += 'I' not in cig and 'D' not in cig
                    c['sa_minus'] += e.split(',')[2] == '-'
                first, prim = els[0].split(','), next(j for j, g in enumerate(fs) if not int(g[1]) & 2048)
                # the line's SA starts with the primary's element although the primary is not the read's first line
                c['sa_primary_not_first'] += prim != 0 and f is not fs[prim] and (first[0], first[1]) == (fs[prim][2], fs[prim][3])
    return c


ERRORFUL_CASES = ('md_deletion', 'md_long_deletion', 'md_deletion_minus', 'md_adjacent_mismatches', 'md_deletion_then_mismatch',
                  'md_mismatch_then_deletion', 'md_starts_0', 'md_ends_0', 'md_all_digits', 'sa_with_I', 'sa_with_D', 'sa_plain',
                  'reads_2_lines')
FULL_CASES = ('reads_3_lines', 'sa_primary_not_first', 'sa_minus')


def md_properties(f):
    """What holds of one mapped line's MD without md_of: its form, its span, and NM.  NM = X + I + D columns: the letters outside
    '^' runs are the X columns and the letters inside them the D columns, so all letters plus the I lengths make NM."""
    md = _tag(f, 'MD')
    assert md is not None and _MD.fullmatch(md), f[:9]
    parts = [(int(n), x) for n, x in _CIGAR.findall(f[5])]
    numbers = sum(int(x) for x in re.findall(r'[0-9]+', md))
    deleted = sum(len(x) - 1 for x in re.findall(r'\^[A-Z]+', md))
    mismatched = len(re.findall(r'[A-Z]', re.sub(r'\^[A-Z]+', '', md)))
    assert numbers + mismatched + deleted == sum(n for n, x in parts if x in 'MD'), f[:9]
    assert deleted == sum(n for n, x in parts if x == 'D'), f[:9]
    assert mismatched + deleted + sum(n for n, x in parts if x == 'I') == int(f[11][5:]), f[:9]


def check_properties(sam, md=True, sa=True):
    """Test 3: per mapped line, MD's form, span and NM; per read, n - 1 SA elements on each of its n lines, each naming another of
    its lines, and one set of (RNAME, POS, strand) over a line and its SA for the whole read."""
    per_read = collections.defaultdict(list)
    for line in sam.decode('latin-1').splitlines():
        f = line.split('\t')
        if int(f[1]) & 4:
            assert _tag(f, 'MD') is None and _tag(f, 'SA') is None
            continue
        per_read[f[0]].append(f)
        if md:
            md_properties(f)
    if not sa:
        return
    for fs in per_read.values():
        own = [(f[2], f[3], '-' if int(f[1]) & 16 else '+') for f in fs]
        for i, f in enumerate(fs):
            text = _tag(f, 'SA')
            if len(fs) < 2:
                assert text is None
                continue
            assert text is not None and text.endswith(';')
            els = [tuple(e.split(',')) for e in text.split(';')[:-1]]
            assert len(els) == len(fs) - 1 and all(len(e) == 6 and e[4] == '60' for e in els)
            others = collections.Counter(own[:i] + own[i + 1:])
            assert collections.Counter(e[:3] for e in els) == others, f[:9]
            assert sorted([own[i]] + [e[:3] for e in els]) == sorted(own)


def check_offsets(off, data, st):
    n = len(st)
    assert len(off) == n + 1 and int(off[0]) == 0 and int(off[-1]) == len(data) and (np.diff(off.astype(np.int64)) >= 0).all()
    live = st['rec_len'] > 0
    assert all(int(off[r + 1]) > int(off[r]) for r in np.flatnonzero(live)) and all(int(off[r + 1]) == int(off[r]) for r in np.flatnonzero(~live))
