"""
--truth-cs / --truth-eqx: the contract of cs:Z: and of =/X CIGARs restated in plain Python (README, "Truth cs and =/X"), shared by
tests/test_truth_cs.py (emulated device) and tests/test_gpu_truth_cs.py (MI355X).

A line's cs and =/X CIGAR are functions of its CIGAR, its MD and its SEQ alone (`cs_of`, `eqx_of`: what samtools calmd or paftools
would do), so the oracle of a batch is that batch's own SAM with MD and without formats: no reference is read, and a run of N is
exact.  `formatted_sam_from` / `formatted_paf_from` rebuild the files of any fmt and tags from it, `bam_from` / `sam_of_bam` are
tests/bam_codec.py's transforms with the operations MIDNSHP=X, `check_properties` checks what must hold without the restatement and
`cs_cases` counts how often a file takes each branch of the writer.
"""
import collections
import functools
import re
import struct

import bam_codec as BC
import truth_tags as TT

FMT_EQX, FMT_CS, FMT_CS_LONG = 1, 2, 4
FMTS = (0, FMT_EQX, FMT_CS, FMT_CS | FMT_CS_LONG, FMT_EQX | FMT_CS, FMT_EQX | FMT_CS | FMT_CS_LONG)     # the six valid values
TAGGED_FMTS = (FMT_EQX | FMT_CS, FMT_EQX | FMT_CS | FMT_CS_LONG)                                          # those also asked with MD|SA

CIGAR_OPS = 'MIDNSHP=X'
_CIGAR = re.compile(r'(\d+)([MIDNSHP=X])')
_MD_ITEM = re.compile(r'(\d+)|\^([^0-9^]+)|([^0-9^])')
_CS_ITEM = re.compile(r':(\d+)|=([A-Za-z]+)|\*([a-z])([a-z])|\+([a-z]+)|-([a-z]+)')


_LOWER = {c: c | 0x20 for c in range(256)}


def lower(text):
    return text.translate(_LOWER)


def parts_of(cigar):
    return [(int(n), x) for n, x in _CIGAR.findall(cigar)]


def runs_of(cigar, md, seq):
    """The line's alignment in reference-forward order as maximal runs of one op, [(op, r, q)]: op one of '=XID', r the run's reference
    bases (the read's on '=', '' on I), q the read's bases ('' on D).  MD says which M columns are mismatches and what was deleted.
    The walk is by CIGAR runs and MD items, never by column."""
    items = []                                   # ('=', n) | ('X', base) | ('D', bases)
    for num, dele, mis in _MD_ITEM.findall(md):
        if num:
            if int(num): items.append(('=', int(num)))
        elif dele: items.append(('D', dele))
        else: items.append(('X', mis))
    runs = []

    def emit(op, r, q):
        if runs and runs[-1][0] == op:
            runs[-1][1].append(r); runs[-1][2].append(q)
        else: runs.append((op, [r], [q]))

    i, rem, q = 0, (items[0][1] if items and items[0][0] == '=' else 0), 0
    for n, x in parts_of(cigar):
        if x == 'S': q += n
        elif x == 'M':
            while n:
                kind, what = items[i]
                if kind == '=':
                    k = min(rem, n)
                    emit('=', seq[q:q + k], seq[q:q + k])
                    q += k; n -= k; rem -= k
                    if rem: continue
                else:
                    assert kind == 'X', (cigar, md[:80])
                    emit('X', what, seq[q])
                    q += 1; n -= 1
                i += 1
                rem = items[i][1] if i < len(items) and items[i][0] == '=' else 0
        elif x == 'I':
            emit('I', '', seq[q:q + n])
            q += n
        elif x == 'D':
            assert items[i][0] == 'D' and len(items[i][1]) == n, (cigar, md[:80])
            emit('D', items[i][1], '')
            i += 1
            rem = items[i][1] if i < len(items) and items[i][0] == '=' else 0
        else: assert x == 'H', cigar
    assert i == len(items) and q == len(seq), (cigar, md[:80])
    return [(op, ''.join(r), ''.join(q)) for op, r, q in runs]


@functools.lru_cache(maxsize=8192)
def _derive(cigar, md, seq):
    """(cs short, cs long, the =/X CIGAR's runs without clips) of one line: the fmts of one batch ask for the same lines again."""
    short, long, body = [], [], []
    for op, r, q in runs_of(cigar, md, seq):
        if op == '=': short.append(f':{len(r)}'); long.append('=' + r)
        else:
            piece = ''.join('*' + a + b for a, b in zip(lower(r), lower(q))) if op == 'X' else ('+' + lower(q)) if op == 'I' else ('-' + lower(r))
            short.append(piece); long.append(piece)
        body.append(f'{max(len(r), len(q))}{op}')
    return ''.join(short), ''.join(long), ''.join(body)


def cs_of(cigar, md, seq, long):
    return _derive(cigar, md, seq)[1 if long else 0]


def eqx_of(cigar, md, seq=None):
    """The CIGAR with its M runs split into = and X runs; the clips stay.  (SEQ plays no part: without one any base will do.)"""
    parts = parts_of(cigar)
    if seq is None:
        seq = 'N' * sum(n for n, x in parts if x in 'SMI')
    left = f'{parts[0][0]}{parts[0][1]}' if parts[0][1] in 'SH' else ''
    right = f'{parts[-1][0]}{parts[-1][1]}' if parts[-1][1] in 'SH' else ''
    return left + _derive(cigar, md, seq)[2] + right


def _fields(sam):
    return [l.split('\t') for l in bytes(sam).decode('latin-1').splitlines()]


def _md(f):
    assert f[13].startswith('MD:Z:'), f[:9]
    return f[13][5:]


def formatted_sam_from(md_sam, fmt, tags):
    """The SAM of `fmt` and `tags` from the same batch's SAM with MD alone (tags = MD, fmt = 0): NM AS [MD] [cs] [SA] [CO]."""
    lines = _fields(md_sam)
    mapped = collections.defaultdict(list)
    for i, f in enumerate(lines):
        if not int(f[1]) & 4: mapped[f[0]].append(i)
    out = []
    for i, f in enumerate(lines):
        if int(f[1]) & 4:
            out.append('\t'.join(f) + '\n')
            continue
        md, extra = _md(f), []
        if tags & TT.TAG_MD: extra.append(f[13])
        if fmt & FMT_CS: extra.append('cs:Z:' + cs_of(f[5], md, f[9], bool(fmt & FMT_CS_LONG)))
        mine = mapped[f[0]]
        if tags & TT.TAG_SA and len(mine) > 1:
            prim = next(j for j in mine if not int(lines[j][1]) & 2048)
            order = ([prim] if prim != i else []) + [j for j in mine if j not in (i, prim)]
            extra.append('SA:Z:' + ''.join(TT.sa_element(lines[j]) for j in order))
        cigar = eqx_of(f[5], md, f[9]) if fmt & FMT_EQX else f[5]
        out.append('\t'.join(f[:5] + [cigar] + f[6:13] + extra + f[14:]) + '\n')
    return ''.join(out).encode('latin-1')


def formatted_paf_from(paf, md_sam, fmt):
    """The PAF of `fmt` from the untagged PAF text and the same batch's SAM with MD: record i of a read is its mapped line i; cs is
    the line's, cg the line's =/X CIGAR without clips (on '-' that is the record's runs in reverse order, as in the plain PAF)."""
    mapped = collections.defaultdict(list)
    for f in _fields(md_sam):
        if not int(f[1]) & 4: mapped[f[0]].append(f)
    seen, out = collections.Counter(), []
    for line in paf.splitlines():
        p = line.split('\t')
        f = mapped[p[0]][seen[p[0]]]
        seen[p[0]] += 1
        assert (p[4] == '-') == bool(int(f[1]) & 16) and p[5] == f[2] and int(p[7]) + 1 == int(f[3]), (p[:9], f[:9])
        assert p[13].startswith('cg:Z:') and p[15].startswith('AS:i:') and len(p) == 16
        # cg holds the runs in reverse column order on '-', which is the reference-forward order of the SAM line's CIGAR
        assert p[13] == 'cg:Z:' + ''.join(f'{n}{x}' for n, x in parts_of(f[5]) if x not in 'SH'), (p[:9], f[:9])
        if fmt & FMT_EQX:
            p[13] = 'cg:Z:' + ''.join(f'{n}{x}' for n, x in parts_of(eqx_of(f[5], _md(f), f[9])) if x not in 'SH')
        if fmt & FMT_CS: p.append('cs:Z:' + cs_of(f[5], _md(f), f[9], bool(fmt & FMT_CS_LONG)))
        out.append('\t'.join(p) + '\n')
    assert all(seen[k] == len(v) for k, v in mapped.items())
    return ''.join(out)


# ---------------------------------------------------------------------------------------------
# SAM <-> BAM with the operations MIDNSHP=X (tests/bam_codec.py knows MIDNSH)
# ---------------------------------------------------------------------------------------------
def bam_from(sam_records, contig_names, max_cigar_ops=65535):
    """bam_codec.bam_from with = and X: the BAM records of SAM record lines, back to back; reflen counts M D N = X."""
    ref_id = {name: i for i, name in enumerate(contig_names)}
    out = []
    for f in _fields(sam_records):
        name, flag, seq, qual = f[0], int(f[1]), f[9], f[10]
        assert len(name) == 36 and f[6:9] == ['*', '0', '0']
        ops = [(n, CIGAR_OPS.index(x)) for n, x in parts_of(f[5])] if f[5] != '*' else []
        assert ''.join(f'{n}{CIGAR_OPS[x]}' for n, x in ops) == (f[5] if f[5] != '*' else '')
        reflen = sum(n for n, x in ops if x in (0, 2, 3, 7, 8))
        if flag & 4: rid, pos, mapq, bin_ = -1, -1, 0, 4680
        else:
            rid, pos, mapq = ref_id[f[2]], int(f[3]) - 1, int(f[4])
            bin_ = BC.reg2bin(pos, pos + reflen) & 0xFFFF
        tags = b''
        for t in f[11:]:
            if t[2:5] == ':i:': tags += BC.int_tag(t[:2], int(t[5:]))
            else:
                assert t[2:5] == ':Z:'
                tags += t[:2].encode() + b'Z' + t[5:].encode('latin-1') + b'\0'
        cigar = ops
        if len(ops) > max_cigar_ops:
            cigar = [(len(seq), 4), (reflen, 3)]
            tags += b'CGBI' + struct.pack('<I', len(ops)) + b''.join(struct.pack('<I', n << 4 | x) for n, x in ops)
        nib = [BC.SEQ_SET.index(c) if c in BC.SEQ_SET else 15 for c in seq.upper()] + [0]
        packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(seq), 2))
        body = struct.pack('<iiBBHHHIiii', rid, pos, len(name) + 1, mapq, bin_, len(cigar), flag, len(seq), -1, -1, 0)
        body += name.encode() + b'\0' + b''.join(struct.pack('<I', n << 4 | x) for n, x in cigar)
        body += packed + bytes(ord(c) - 33 for c in qual) + tags
        out.append(struct.pack('<I', len(body)) + body)
    return b''.join(out)


def sam_of_bam(raw, contig_names):
    """bam_codec.sam_of_bam with = and X, over its general record decoder; a CG:B:I tag is read back into the CIGAR."""
    lines = []
    for r in BC.records_of_bam(raw):
        cigar, tags = r['cigar'], r['tags']
        cg = [t for t in tags if t[0] == 'CG']
        if cg:
            assert cg[0][1] == 'BI' and tags[-1] is cg[0] and len(cigar) == 2 and cigar[0] == (r['l_seq'], 4) and cigar[1][1] == 3
            cigar, tags = [(w >> 4, w & 15) for w in cg[0][2]], tags[:-1]
        text = ''.join(f'{n}{CIGAR_OPS[x]}' for n, x in cigar) or '*'
        fields = [r['name'], str(r['flag']), '*' if r['rid'] < 0 else contig_names[r['rid']], str(r['pos'] + 1), str(r['mapq']), text, '*', '0', '0']
        assert r['next'] == (-1, -1, 0)
        fields += [r['seq'], ''.join(chr(q + 33) for q in r['qual'])]
        fields += [f'{t}:{"Z" if k == "Z" else "i"}:{v}' for t, k, v in tags]
        lines.append('\t'.join(fields) + '\n')
    return ''.join(lines).encode('latin-1')


# ---------------------------------------------------------------------------------------------
# properties and cases
# ---------------------------------------------------------------------------------------------
def cs_items(cs):
    """[(kind, text)] of a cs value, kind one of ':=*+-' (':' text = the number); the value must be made of such items alone."""
    items, at = [], 0
    for m in _CS_ITEM.finditer(cs):
        assert m.start() == at, cs[:80]
        at = m.end()
        num, eq, r, q, ins, dele = m.groups()
        items.append((':', num) if num else ('=', eq) if eq else ('*', r + q) if r else ('+', ins) if ins else ('-', dele))
    assert at == len(cs) and items and items[0][0] in ':=*' and items[-1][0] in ':=*', cs[:80]
    return items


def ops_of_cs(cs):
    """One letter of '=XID' per column, in reference-forward order."""
    return ''.join({':': lambda t: '=' * int(t), '=': lambda t: '=' * len(t), '*': lambda t: 'X', '+': lambda t: 'I' * len(t),
                    '-': lambda t: 'D' * len(t)}[k](t) for k, t in cs_items(cs))


def check_properties(plain_sam, sam, paf, fmt, ref_of, counts=None):
    """What holds of the files of `fmt` (SAM and PAF of one batch; `plain_sam`: the same batch's SAM without formats) without
    cs_of / eqx_of.  Per mapped line: the reference implied by cs is the forward strand's slice (a line whose slice holds an N is
    exempt, as in the MD tests), the implied query is the aligned SEQ, the '=' columns are the PAF's matches, '*' + inserted +
    deleted letters are NM; the =/X CIGAR collapsed to M is the plain CIGAR and its '=' lengths are the matches.  The PAF record
    carries the line's cs.  Unmapped lines carry no cs."""
    counts = collections.Counter() if counts is None else counts
    pafs = collections.defaultdict(list)
    for line in paf.splitlines():
        p = line.split('\t')
        pafs[p[0]].append(p)
    seen = collections.Counter()
    for f, g in zip(_fields(sam), _fields(plain_sam)):
        assert f[:5] == g[:5] and f[6:11] == g[6:11]
        cs = TT._tag(f, 'cs')
        if int(f[1]) & 4:
            assert cs is None and f[5] == '*'
            continue
        p = pafs[f[0]][seen[f[0]]]
        seen[f[0]] += 1
        matches, nm = int(p[9]), int(f[11][5:])
        parts = parts_of(f[5])
        if fmt & FMT_EQX:
            merged = []
            for n, x in parts:
                x = 'M' if x in '=X' else x
                if merged and merged[-1][1] == x == 'M': merged[-1] = (merged[-1][0] + n, 'M')
                else: merged.append((n, x))
            assert ''.join(f'{n}{x}' for n, x in merged) == g[5], f[:9]
            assert all(a[1] != b[1] for a, b in zip(parts, parts[1:])) and 'M' not in f[5]
            assert sum(n for n, x in parts if x == '=') == matches, f[:9]
            counts['eqx_lines'] += 1
        else: assert f[5] == g[5]
        if not fmt & FMT_CS:
            assert cs is None and not any(x.startswith('cs:Z:') for x in p)
            continue
        assert p[-1] == 'cs:Z:' + cs and p[-2].startswith('AS:i:'), p[:9]
        left = parts[0][0] if parts[0][1] == 'S' else 0
        right = parts[-1][0] if parts[-1][1] == 'S' else 0
        aligned = f[9][left:len(f[9]) - right]
        ref, qry, q, eq, edits = [], [], 0, 0, 0
        for kind, text in cs_items(cs):
            assert (kind == '=') == bool(fmt & FMT_CS_LONG) or kind not in ':=', cs[:80]
            if kind == ':':
                n = int(text); ref.append(aligned[q:q + n]); qry.append(aligned[q:q + n]); q += n; eq += n
            elif kind == '=':
                ref.append(text); qry.append(text); q += len(text); eq += len(text)
            elif kind == '*':
                ref.append(text[0].upper()); qry.append(text[1].upper()); q += 1; edits += 1
            elif kind == '+':
                qry.append(text.upper()); q += len(text); edits += len(text)
            else:
                ref.append(text.upper()); edits += len(text)
        ref, qry = ''.join(ref), ''.join(qry)
        assert qry.upper() == aligned.upper() and q == len(aligned), f[:9]
        assert eq == matches and edits == nm, (f[:9], eq, matches, edits, nm)
        want = ref_of(f[2])[int(f[3]) - 1:int(f[3]) - 1 + len(ref)]
        assert len(ref) == int(p[8]) - int(p[7])
        if 'N' in want.upper(): counts['n_lines'] += 1
        else: assert ref.upper() == want.upper(), f[:9]
        counts['cs_lines'] += 1
    assert all(seen[k] == len(v) for k, v in pafs.items())
    return counts


def cs_cases(text):
    """How often a SAM text with cs (either form) takes each branch of the writer.  The device walks a record's columns 64 per step
    from the record's first column; on a '-' line that order is the reverse of the cs's."""
    c = collections.Counter()
    per_read = collections.Counter()
    for f in _fields(text):
        cs = TT._tag(f, 'cs')
        if cs is None:
            continue
        per_read[f[0]] += 1
        minus = bool(int(f[1]) & 16)
        ops = ops_of_cs(cs)
        dev = ops[::-1] if minus else ops
        c['record_le_64'] += len(dev) <= 64
        c['record_gt_64'] += len(dev) > 64
        for op, key in (('=', 'eq_run_crosses_step'), ('I', 'ins_run_crosses_step'), ('D', 'del_run_crosses_step')):
            c[key] += any(dev[k - 1] == op == dev[k] for k in range(64, len(dev), 64))
        c['x_first_of_step'] += any(dev[k] == 'X' for k in range(0, len(dev), 64))
        c['x_last_of_step'] += any(dev[k] == 'X' for k in range(63, len(dev), 64))
        c['adjacent_xx'] += 'XX' in ops
        c['del_then_ins'] += 'DI' in dev
        c['ins_then_del'] += 'ID' in dev
        c['minus_with_x'] += minus and 'X' in ops
        c['minus_with_ins'] += minus and 'I' in ops
        c['minus_with_del'] += minus and 'D' in ops
        c['only_matches'] += set(ops) == {'='}
        c['not_only_matches'] += set(ops) != {'='}
        c['max_columns'] = max(c['max_columns'], len(dev))
    c['reads_2_records'] = sum(n >= 2 for n in per_read.values())
    return c


# What the two emulated batches of tests/test_truth_cs.py (and the larger GPU ones) must show.  Their alignments hold no I run across a
# 64-column step and no D column next to an I column (ins_run_crosses_step, del_then_ins, ins_then_del: counted, not required here;
# the long reads of tests/test_gpu_truth_cs.py are asked for the first).
ERRORFUL_CASES = ('record_le_64', 'record_gt_64', 'eq_run_crosses_step', 'del_run_crosses_step', 'x_first_of_step', 'x_last_of_step',
                  'adjacent_xx', 'minus_with_x', 'minus_with_ins', 'minus_with_del', 'reads_2_records')
FULL_CASES = ('record_gt_64', 'eq_run_crosses_step', 'reads_2_records', 'only_matches')
