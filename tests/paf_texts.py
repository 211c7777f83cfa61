"""
TEST INFRASTRUCTURE: the device loader (--gpu-loader; include/brx.h: brx_paf_scan, brx_align_pack) against the code it stands in for.
The yardsticks are the host's own loader and packer (alignment.Alignment / load_alignments, model_builder.Job) and, for the lines the
device hands back to the host, the reference itself (tests/golden/paf_lines.json.gz, written by tools/make_paf_golden.py).  Every check
takes the engine as its argument: tests/test_loader.py passes the interpreted kernels (tests/emu_engine.py), tests/test_gpu_loader.py
the MI355X.  Nothing here has a tolerance: every comparison is of integers, bytes or text.
"""
import ctypes
import functools
import gzip
import io
import json
import os
import re

import numpy as np
import pytest

import model_jobs as MJ
import plot_windows as PW
from badread_amd import engine as E
from badread_amd import model_builder as MB
from badread_amd import plot_window_identity as P
from badread_amd.alignment import NO_D, Alignment, DeviceAlignments, load_alignments, load_alignments_device
from badread_amd.misc import load_fasta, load_fastq

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIRS = {name: os.path.join(HERE, 'golden', name) for name in ('model_builder', 'model_builder_edges')}
JOB_FIELDS = ('seq', 'qual', 'ref', 'part_type', 'part_len', 'part_col', 'part_read', 'part_ref', 'align_part_off', 'align_col_off',
              'align_read_off')


# ---- the definition of a regular line, restated (include/brx.h) ----------------------------------------------------------------------
_INT = re.compile(rb'[0-9]{1,18}\Z')
_AS = re.compile(rb'-?[0-9]{1,18}\Z')
_CIGAR = re.compile(rb'([0-9]{1,9}[A-Za-z])+\Z')


def is_regular(line):
    if not line or line[:1] == b'\t' or line[-1:] == b'\t' or any(c != 9 and not 0x21 <= c <= 0x7e for c in line):
        return False
    fields = line.split(b'\t')
    if len(fields) < 11 or len(fields[4]) != 1 or not all(_INT.match(fields[i]) for i in (2, 3, 7, 8, 9, 10)) or int(fields[10]) == 0:
        return False
    cg = [f[5:] for f in fields if f.startswith(b'cg:Z:')]
    scores = [f[5:] for f in fields if f.startswith(b'AS:i:')]
    return bool(cg and scores and all(_AS.match(s) for s in scores) and _CIGAR.match(cg[-1]))


def lines_of(text, max_lines=0):
    """(offset, bytes) of the lines a text file of these bytes has, the first max_lines of them (0: all)."""
    out, at = [], 0
    for piece in text.split(b'\n')[:-1] + ([text.split(b'\n')[-1]] if not text.endswith(b'\n') and text else []):
        out.append((at, piece))
        at += len(piece) + 1
    return out[:max_lines] if max_lines > 0 else out


def expected_record(line):
    """What a record promises for a regular line, from the host's parse of it."""
    a = Alignment(line.decode('ascii') + '\n')
    parts = [(n, t) for n, t in (a.cigar_parts[::-1] if a.strand == '-' else a.cigar_parts) if t in 'MID']
    before_d = [sum(n for n, t in parts[:j] if t != 'D') for j, (_, t) in enumerate(parts) if t == 'D']
    fields = line.split(b'\t')
    at_cigar = line.rindex(b'\tcg:Z:') + 6 if b'\tcg:Z:' in line else 5
    return dict(qname=a.read_name.encode(), tname=a.ref_name.encode(), tname_off=len(b'\t'.join(fields[:5])) + 1, strand=ord(a.strand),
                ints=[a.read_start, a.read_end, a.ref_start, a.ref_end, a.matching_bases, a.num_bases], score=a.alignment_score,
                cigar=a.cigar.encode(), cigar_off=at_cigar, n_parts=len(parts), max_indel=a.max_indel,
                sums=[sum(n for n, t in parts if t == x) for x in 'MID'],
                first_d=before_d[0] if before_d else NO_D, last_d=before_d[-1] if before_d else NO_D)


def upload(engine, data):
    return engine._upload(np.frombuffer(data, dtype=np.uint8))[1][:len(data)]


def check_scan(engine, text, max_lines=0, irregular=None):
    """One record per line; a line is flagged exactly when it is not regular, and a regular line's record equals the host's parse.
    irregular: the number of flagged lines the caller expects."""
    recs = engine.paf_scan(upload(engine, text), max_lines)
    want = lines_of(text, max_lines)
    assert len(recs) == len(want)
    flagged = 0
    for k, (rec, (off, line)) in enumerate(zip(recs, want)):
        where = (k, line[:80])
        assert (int(rec['line_off']), int(rec['line_len'])) == (off, len(line)), where
        assert bool(rec['flags'] & E.PAF_IRREGULAR) == (not is_regular(line)), where
        if rec['flags'] & E.PAF_IRREGULAR:
            flagged += 1
            continue
        x = expected_record(line)
        assert line[:rec['qname_len']] == x['qname'] and int(rec['tname_off']) == x['tname_off'], where
        assert line[rec['tname_off']:rec['tname_off'] + rec['tname_len']] == x['tname'] and int(rec['strand']) == x['strand'], where
        assert rec['ints'].tolist() == x['ints'] and int(rec['as']) == x['score'], where
        assert int(rec['cigar_off']) == x['cigar_off'] and line[rec['cigar_off']:rec['cigar_off'] + rec['cigar_len']] == x['cigar'], where
        assert (int(rec['n_parts']), int(rec['max_indel'])) == (x['n_parts'], x['max_indel']), where
        assert [int(rec[f]) for f in ('sum_m', 'sum_i', 'sum_d')] == x['sums'], where
        assert (int(rec['first_d']), int(rec['last_d'])) == (x['first_d'], x['last_d']), where
    assert irregular is None or flagged == irregular
    return recs


# ---- texts -----------------------------------------------------------------------------------------------------------------------------
def paf_line(name='r', cigar='120M', score='5', strand='+', tags_before=('tp:A:P',), tags_after=(), ints=(0, 200, 10, 210, 190, 200), tname='ctg'):
    return '\t'.join([name, '300', str(ints[0]), str(ints[1]), strand, tname, '9000', str(ints[2]), str(ints[3]), str(ints[4]), str(ints[5]), '60',
                      *tags_before, *([f'AS:i:{score}'] if score is not None else []), *([f'cg:Z:{cigar}'] if cigar is not None else []),
                      *tags_after])


@functools.lru_cache(maxsize=None)
def synthetic_text():
    """The shapes at which the lexer can go wrong (the issue's list), more than 1024 lines and 1024 bytes; ends WITHOUT a newline."""
    nine, two = '123456789M', '1M1I' * 16                            # a nine-digit length; 32 two-byte parts: 64 bytes
    cigars = ['7M', '10S', '120M', nine, two, two + two + '3D', '1M' * 30 + nine + '2D',      # 60 bytes, then nine digits over the border
              '1M' * 31 + '9D', '1M' * 31 + '1I' + '77D', '1M' * 31 + '12D' + '1I',            # 63 / 64 / 65 bytes ... and the same
              '1M' * 28 + '123456I', '1M' * 28 + '12345D' + '1M', '1M' * 28 + '12345D' + '10M',
              '5S3M2H4I1N6D2P7M1X8m9M4S', '3H10M5S', '4D10M', '10M4D', '4D', '3D2I5D', '2I9D4M1D', '1M2D' * 40 + '900000000I' + '1D3M' * 40]
    lines = []
    for k in range(1, 71):                                           # the CIGAR's first byte meets every position of a 64-byte step
        for c in (cigars[k % len(cigars)], cigars[(3 * k + 1) % len(cigars)]):
            lines.append(paf_line('q' * k, c, strand='+-'[k & 1]))
    for c in cigars:
        lines.append(paf_line('c', c))
        lines.append(paf_line('c', c, strand='-', tags_after=('NM:i:3',)))
    # cg before and after AS, each given twice (the last wins); cg:Z: as the read name
    lines.append(paf_line('two', None, None, tags_before=('cg:Z:5M', 'AS:i:-3', 'cg:Z:6M2D1M', 'AS:i:44')))
    lines.append(paf_line('two', None, None, tags_before=('AS:i:1', 'cg:Z:5M', 'AS:i:2', 'cg:Z:8M1D')))
    lines.append(paf_line('cg:Z:3M4I', None, '7'))
    lines.append(paf_line('cg:Z:3M4I', '9D1M', '7'))
    lines.append(paf_line('AS:i:12', '5M', None))                    # ... and AS:i: as the read name
    for score in ('-1', '0', '-0', '999999999999999999', '-999999999999999999'):
        lines.append(paf_line('s', '5M', score))
    lines.append(paf_line('big', '5M', '1', ints=(0, 999999999999999999, 7, 123456789012345678, 1, 1)))
    lines += [paf_line(f'f{k}', f'{k + 1}M{k % 7}D{k % 5 + 1}I', str(k - 500)) for k in range(1000)]
    assert len(lines) > 1024
    return '\n'.join(lines).encode('ascii')


def check_synthetic(engine):
    text = synthetic_text()
    n = len(lines_of(text))
    check_scan(engine, text, irregular=0)
    check_scan(engine, text + b'\n', irregular=0)                  # the last line with its newline: the same lines
    for max_lines in (1, n, n + 5):
        assert len(check_scan(engine, text[:40000], max_lines)) == min(max_lines, len(lines_of(text[:40000])))
    one = paf_line('one', '5M2D').encode()
    assert len(check_scan(engine, one, irregular=0)) == 1 and len(check_scan(engine, one + b'\n', irregular=0)) == 1
    assert len(engine.paf_scan(upload(engine, b''))) == 0
    # a line that is not regular beyond max_lines flags nothing and is not counted
    assert len(check_scan(engine, one + b'\n\nx\n', 1, irregular=0)) == 1 and len(check_scan(engine, one + b'\n\nx\n', irregular=2)) == 3


def big_text():
    """1.1 MB of short lines: more than 1024 tiles of line starts, the second level of the scan (GPU only)."""
    lines = [paf_line(f'b{k}', f'{k % 90 + 1}M{k % 3}D', str(k)) for k in range(18000)]
    text = ('\n'.join(lines) + '\n').encode()
    assert len(text) > 1024 * E.DEPTH_TILE * 1.05
    return text


def check_committed(engine):
    """The committed PAFs: every line regular (a lexer that flags everything cannot pass), every record the host's parse."""
    for name, n_lines in (('model_builder', 60), ('model_builder_edges', 109)):
        with open(os.path.join(GOLDEN_DIRS[name], 'aln.paf'), 'rb') as f:
            text = f.read()
        assert len(check_scan(engine, text, irregular=0)) == n_lines


@functools.lru_cache(maxsize=None)
def made_jobs():
    return {'edges_files': MJ.edges(files=True), 'mixed': MJ.mixed()}


def check_made_files(engine, name):
    text = ('\n'.join(made_jobs()[name][3]) + '\n').encode()
    check_scan(engine, text, irregular=0)


# ---- the lines the host parses -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    with gzip.open(os.path.join(HERE, 'golden', 'paf_lines.json.gz'), 'rt') as f:
        return json.load(f)


ODD_NAMES = ('leading_blank', 'trailing_tab', 'blank_in_name', 'empty_line', 'ten_fields', 'no_cg', 'no_as', 'strand_plus_minus',
             'strand_plus_five', 'integer_19_digits', 'num_bases_zero', 'cg_empty', 'cigar_eq_x', 'cigar_trailing_digits',
             'cigar_two_letters', 'cigar_underscore', 'cigar_10_digit_length', 'cigar_minus_strand')


def check_odd_line(engine, tmp_path, name):
    """The line is flagged, lines around it are not, and the loader gives what the reference gave for it: its attributes or its end."""
    fx = fixture()
    entry = next(e for e in fx['odd'] if e['name'] == name)
    good = fx['regular']['line'].replace('odd\t', 'good\t', 1)
    text = (good + '\n' + entry['line'] + '\n' + good.replace('good', 'good2') + '\n').encode()
    recs = check_scan(engine, text, irregular=1)
    assert recs['flags'].tolist() == [0, E.PAF_IRREGULAR, 0]
    path = tmp_path / f'{name}.paf'
    path.write_bytes(text)
    out = io.StringIO()
    if 'exit' in entry:
        with pytest.raises(SystemExit) as e:
            load_alignments_device(str(path), engine, output=out)
        assert str(e.value.code) == entry['exit'] and out.getvalue() == 'Loading alignments'
        return None
    if 'exception' in entry:
        with pytest.raises(Exception) as e:
            load_alignments_device(str(path), engine, output=out)
        assert type(e.value).__name__ == entry['exception']
        return None
    kept = load_alignments_device(str(path), engine, output=out)
    assert isinstance(kept, DeviceAlignments) and [a.read_name for a in kept] == ['good', entry['attributes']['read_name'], 'good2']
    a = kept[1]
    for field, value in entry['attributes'].items():
        got = getattr(a, field)
        got = repr(got) if field == 'percent_identity' else [f'{n}{t}' for n, t in got] if field == 'cigar_parts' else got
        assert got == value, field
    assert repr(a) == entry['repr']
    return kept


def check_host_route(engine, tmp_path):
    """A file with a carriage return, or a byte of 0x80 or more, takes the host loader whole: plain Alignment objects."""
    line = fixture()['regular']['line']
    for k, text in enumerate(((line + '\r\n' + line.replace('odd', 'odd2') + '\r\n').encode(), (line.replace('odd', 'odé') + '\n').encode('utf-8'))):
        path = tmp_path / f'host_{k}.paf'
        path.write_bytes(text)
        o1, o2 = io.StringIO(), io.StringIO()
        got, want = load_alignments_device(str(path), engine, output=o1), load_alignments(str(path), output=o2)
        assert not isinstance(got, DeviceAlignments) and all(type(a) is Alignment for a in got)
        assert [vars(a) for a in got] == [vars(a) for a in want] and len(got) == 2 - k
        assert o1.getvalue() == o2.getvalue()


# ---- load_alignments_device == load_alignments -------------------------------------------------------------------------------------------
ATTRIBUTES = ('read_name', 'read_start', 'read_end', 'strand', 'ref_name', 'ref_start', 'ref_end', 'matching_bases', 'num_bases',
              'percent_identity', 'cigar', 'alignment_score', 'cigar_parts', 'max_indel')


def assert_same_alignments(got, want):
    assert [repr(a) for a in got] == [repr(a) for a in want]
    for a, b in zip(got, want):
        for field in ATTRIBUTES:
            assert getattr(a, field) == getattr(b, field) and type(getattr(a, field)) is type(getattr(b, field)), (repr(b), field)


def both_loaders(engine, path, max_alignments=None, dot_interval=1000):
    o1, o2 = io.StringIO(), io.StringIO()
    got = load_alignments_device(str(path), engine, max_alignments, output=o1, dot_interval=dot_interval)
    want = load_alignments(str(path), max_alignments, output=o2, dot_interval=dot_interval)
    assert o1.getvalue() == o2.getvalue()
    assert_same_alignments(got, want)
    return got


def selection_text():
    """Equal scores (the last wins), interleaved reads, the two filters at their borders, a kept irregular line among them."""
    L = lambda name, score, m, n, cigar='150M', **kw: paf_line(name, cigar, str(score), ints=(0, 200, 10, 210, m, n), **kw)
    lines = [L('a', 5, 190, 200, '150M1D'), L('b', 9, 190, 200), L('a', 5, 191, 200, '149M2I'), L('c', -4, 190, 200), L('b', 8, 100, 200),
             L('a', 4, 199, 200), L('short', 1, 100, 100), L('long', 1, 101, 101), L('poor', 1, 80, 100 + 1), L('edge80', 1, 160, 200),
             L('above80', 1, 161, 200), L('c', -4, 160, 200), L('c', -5, 200, 200), L('d', 0, 190, 200, '100M5MM', strand='-'),
             L('e', 2, 190, 200, '20M3D130M', strand='-'), L('d', 0, 150, 200, '10M'), L('g', 3, 190, 200, '100M5MM')]
    lines += [L(f'n{k % 37}', k % 11, 150 + k % 50, 200, f'{100 + k % 9}M{k % 4}I') for k in range(90)]
    return ('\n'.join(lines) + '\n').encode()


def check_selection(engine, tmp_path):
    path = tmp_path / 'selection.paf'
    path.write_bytes(selection_text())
    kept = both_loaders(engine, path)
    names = [a.read_name for a in kept]
    assert names[:2] == ['a', 'b'] and 'short' not in names and 'long' in names and 'edge80' not in names and 'above80' in names
    assert kept[0].matching_bases == 191 and kept[0].cigar == '149M2I' and 'e' in names and 'g' in names
    assert 'c' not in names and 'd' not in names and 'poor' not in names       # the last of c's and d's equal scores is at 80.0 % and 75 %
    n_lines = len(lines_of(selection_text()))
    for max_alignments in (0, -3, 1, 4, 13, n_lines, n_lines + 1):
        both_loaders(engine, path, max_alignments)
    for dot_interval in (1, 7):                                     # the dots of both progress lines
        both_loaders(engine, path, dot_interval=dot_interval)
    for name, folder in GOLDEN_DIRS.items():
        both_loaders(engine, os.path.join(folder, 'aln.paf'), dot_interval=10)
    path.write_bytes(b'')                                           # an empty file: no alignment, the two progress lines
    assert both_loaders(engine, path) == []
    # the first bad line ends the command, with the dots of the lines before it
    bad = selection_text() + b'bad line\n' + selection_text() + b'\n'
    path.write_bytes(bad)
    ends = []
    for load in (lambda o: load_alignments_device(str(path), engine, output=o, dot_interval=10), lambda o: load_alignments(str(path), output=o, dot_interval=10)):
        o = io.StringIO()
        with pytest.raises(SystemExit) as e:
            load(o)
        ends.append((str(e.value.code), o.getvalue()))
    assert ends[0] == ends[1] and ends[0][0] == 'Error: alignment file does not seem to be in PAF format' and ends[0][1].count('.') == 10


# ---- Job.packed == Job --------------------------------------------------------------------------------------------------------------------
def line_of(a, reads, refs, matching=1000, bases=1001):
    """A PAF line of an alignment that passes the loader's filters, whatever its size."""
    return '\t'.join([a.read_name, str(len(reads[a.read_name][0])), str(a.read_start), str(a.read_end), a.strand, a.ref_name,
                      str(len(refs[a.ref_name])), str(a.ref_start), str(a.ref_end), str(matching), str(bases), '60', f'AS:i:{a.alignment_score}',
                      f'cg:Z:{a.cigar}'])


def shapes_job():
    """What the other jobs do not hold: '-' alignments of 1, 2 and 3 parts, slices clipped by the contig's and by the read's end, a contig
    with IUPAC codes and a '*', CIGARs with letters that are dropped, an alignment without parts, kept irregular lines."""
    refs = {'ctg': 'ACGTTGCAAGGCTTAACCGGTTAGCATCGA' * 4, 'odd': 'ACGTRYSWKMBVDHN*acgtn.-?XZ' * 3}
    reads = {f'r{k}': ('TTGACCAGTAGGACATTAGACCATAGGACAT' * 3, ''.join(chr(33 + (7 * k + i) % 90) for i in range(93))) for k in range(16)}
    L = lambda k, rs, re_, strand, ref, fs, fe, cigar, extra=(): '\t'.join(
        [f'r{k}', '93', str(rs), str(re_), strand, ref, '120', str(fs), str(fe), '1000', '1001', '60', 'AS:i:1', f'cg:Z:{cigar}', *extra])
    lines = [L(0, 0, 40, '-', 'ctg', 5, 45, '40M'), L(1, 0, 40, '-', 'ctg', 5, 47, '30M2D10M'), L(2, 3, 45, '-', 'ctg', 5, 43, '30M4I2D6M'),
             L(3, 0, 30, '+', 'ctg', 100, 140, '20M'), L(4, 0, 30, '-', 'ctg', 100, 140, '5M2D13M'),       # the contig ends at 120
             L(5, 80, 120, '+', 'ctg', 0, 10, '9M1I1M'), L(6, 80, 120, '-', 'ctg', 0, 13, '3D9M1I1M'),       # the read ends at 93
             L(7, 0, 78, '-', 'odd', 0, 78, '78M'), L(8, 0, 60, '+', 'odd', 10, 70, '30M1D29M1I'),
             L(9, 0, 50, '+', 'ctg', 0, 50, '5S3M2H4I1N6D2P7M1X8m9M4S'), L(10, 0, 50, '-', 'ctg', 0, 50, '5S3M2H4I1N6D2P7M1X8m9M4S'),
             L(11, 0, 50, '+', 'ctg', 0, 50, '10S'), L(12, 50, 40, '+', 'ctg', 60, 50, '7H'),
             L(13, 0, 50, '-', 'ctg', 0, 50, '10M3D5MM20M'), L(14, 0, 50, '+', 'ctg', 0, 50, '10M2I5_7D20M3'), L(15, 0, 50, '-', 'ctg', 0, 50, '30M', ('',))]
    return refs, reads, lines


@functools.lru_cache(maxsize=None)
def packed_cases():
    """name -> (refs, reads, PAF lines)"""
    cases = {'shapes': shapes_job()}
    for name, ((refs, reads, alignments), _) in PW.synthetic_jobs().items():
        if alignments:
            cases['plot_' + name] = (refs, reads, [line_of(a, reads, refs) for a in alignments])
    for name, made in made_jobs().items():
        fields = [line.split('\t') for line in made[3]]                # the small alignments of `mixed` pass the loader's filters too
        cases[name] = (made[0], made[1], ['\t'.join(f[:9] + ['1000', '1001'] + f[11:]) for f in fields])
    for name, folder in GOLDEN_DIRS.items():
        with open(os.path.join(folder, 'aln.paf')) as f:
            lines = f.read().splitlines()
        cases[name] = (load_fasta(os.path.join(folder, 'ref.fasta'))[0], load_fastq(os.path.join(folder, 'reads.fastq'), output=io.StringIO()), lines)
    return cases


def host_array(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def assert_same_job(got, want, where):
    for field in JOB_FIELDS:
        a, b = host_array(getattr(got, field)), getattr(want, field)
        assert a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes(), (where, field)
    assert (got.n_align, got.n_cols) == (want.n_align, want.n_cols) and len(got.slices) == len(want.slices), where
    for k in range(want.n_align):
        assert got.slices[k] == want.slices[k] and got.gapped(k, '-') == want.gapped(k, '-'), (where, k)


def check_packed_job(engine, tmp_path, name):
    """Every array of Job.packed, copied back, is the host Job's byte for byte: of the whole file and of every range a chunk border can
    make between two alignments (each split in two; for small jobs every range)."""
    refs, reads, lines = packed_cases()[name]
    path = tmp_path / 'aln.paf'
    path.write_text('\n'.join(lines) + '\n')
    packed = both_loaders(engine, path)
    host = load_alignments(str(path), output=io.StringIO())
    n = len(host)
    assert n > 0
    if name == 'shapes':
        assert n == 16 and int((packed.rec['cigar_off'] >= len('\n'.join(lines)) + 1).sum()) == 3      # the canonical side text
    assert_same_job(MB.Job.packed(engine, refs, reads, packed, 0, n), MB.Job(refs, reads, host), (name, 0, n))
    ranges = [(a, b) for a in range(n) for b in range(a, n + 1)] if n <= 6 else [(0, k) for k in range(1, n, max(n // 7, 1))] + [(k, n) for k in range(1, n, max(n // 7, 1))]
    for first, end in ranges:
        assert_same_job(MB.Job.packed(engine, refs, reads, packed, first, end), MB.Job(refs, reads, host[first:end]), (name, first, end))


def check_plot_chunks(engine, tmp_path, monkeypatch):
    """window_means over a DeviceAlignments gives what it gives over the host's list, with a chunk border between any two alignments
    (PLOT_CHUNK_BASES 3000) and without one; the reference text is uploaded once."""
    refs, reads, lines = packed_cases()['mixed']
    lines = lines[:60]
    path = tmp_path / 'aln.paf'
    path.write_text('\n'.join(lines) + '\n')
    packed, host = both_loaders(engine, path), load_alignments(str(path), output=io.StringIO())
    uploads = []
    inner = MB._device_reference
    monkeypatch.setattr(MB, '_device_reference', lambda e, r, p: uploads.append(getattr(p, '_reference', None) is None) or inner(e, r, p))
    for limit in (1 << 40, 3000, 1):
        monkeypatch.setattr(P, 'PLOT_CHUNK_BASES', limit)
        got = [(s.tolist(), e.tolist(), q.tolist()) for s, e, q in P.window_means(engine, refs, reads, packed, 33, True, values=True)]
        want = [(s.tolist(), e.tolist(), q.tolist()) for s, e, q in P.window_means(engine, refs, reads, host, 33, True, values=True)]
        assert got == want and len(got) == len(host)
    assert len(uploads) > len(host) and sum(uploads) == 1


def check_exits(engine, tmp_path):
    """The exits of the checks keep their messages and their order, also where one input triggers two of them."""
    refs, reads, lines = shapes_job()
    L = lambda k, cigar, rs=0, re_=50, fs=0, fe=50, name=None, ref='ctg', strand='+': '\t'.join(
        [name or f'r{k}', '93', str(rs), str(re_), strand, ref, '120', str(fs), str(fe), '1000', '1001', '60', 'AS:i:1', f'cg:Z:{cigar}'])
    deletion, past = 'ends in a deletion with no read base after it', 'runs past its read or reference range'
    cases = {                                                      # what `plot` ends with, what the model commands end with
        'trailing deletion, then past its range': ([lines[0], L(1, '50M4D', fe=20)], deletion, past),
        'trailing deletion on the minus strand': ([lines[0], L(1, '4D50M', strand='-', fe=54)], deletion, None),
        'no trailing deletion on the minus strand': ([lines[0], L(1, '50M4D', strand='-', fe=54)], None, None),
        'a deletion in front of the last base': ([lines[0], L(1, '49M4D1M', fe=54)], None, None),
        'past its read range': ([lines[0], L(1, '60M', fe=60)], past, past),
        'past its reference range': ([lines[0], L(1, '40M20D', fe=50)], past, past),
        'an unknown read before a trailing deletion': ([L(1, '50M4D', fe=54), L(2, '50M', name='nobody')], deletion, 'could not find read nobody'),
        'an unknown contig': ([lines[0], L(1, '50M', ref='nowhere')], 'could not find reference nowhere', 'could not find reference nowhere'),
        'past its range behind two good alignments': ([lines[0], lines[1], L(2, '70M', re_=60, fe=70)], past, past),
    }
    for what, (case, plot_end, model_end) in cases.items():
        path = tmp_path / 'exits.paf'
        path.write_text('\n'.join(case) + '\n')
        packed, host = both_loaders(engine, path), load_alignments(str(path), output=io.StringIO())
        for run, end in ((lambda al: list(P.window_means(engine, refs, reads, al, 10, True)), plot_end), (lambda al: MB._job(engine, refs, reads, al), model_end)):
            ends = []
            for al in (packed, host):
                try:
                    run(al)
                    ends.append(None)
                except SystemExit as e:
                    ends.append(str(e.code))
            assert ends[0] == ends[1] and (ends[0] is None if end is None else end in (ends[0] or '')), (what, ends)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def check_abi(engine):
    """NULL arrays, a line_cap that is too small (BRX_E_OUTPUT, the needed size, then success), zero bytes and zero alignments."""
    lib, torch = engine.lib, engine.torch
    text = (paf_line('a', '5M') + '\n' + paf_line('b', '6M1D') + '\n' + paf_line('c', '7M')).encode()
    d_text = upload(engine, text)
    n = ctypes.c_uint64(99)
    scratch = torch.zeros(int(lib.brx_paf_scan_scratch(len(text))), dtype=torch.uint8, device=engine.device)
    lines = torch.zeros(3 * E.PAF_LINE_DTYPE.itemsize, dtype=torch.uint8, device=engine.device)
    scan = lambda t, nb, out, cap, nl, scr, scr_n: lib.brx_paf_scan(engine.ctx, t, nb, 0, out, cap, nl, scr, scr_n, engine._stream())
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    assert scan(None, 0, None, 0, ctypes.byref(n), None, 0) == 0 and n.value == 0                        # zero bytes: a valid call
    assert scan(ptr(d_text), len(text), ptr(lines), 3, None, ptr(scratch), scratch.numel()) == -1
    assert scan(None, len(text), ptr(lines), 3, ctypes.byref(n), ptr(scratch), scratch.numel()) == -1 and b'NULL' in lib.brx_last_error(engine.ctx)
    assert scan(ptr(d_text), len(text), ptr(lines), 3, ctypes.byref(n), None, 0) == -3 and lib.brx_scratch_needed(engine.ctx) == scratch.numel()
    assert scan(ptr(d_text), len(text), ptr(lines), 3, ctypes.byref(n), ptr(scratch), 64) == -3
    assert scan(ptr(d_text), len(text), ptr(lines), 2, ctypes.byref(n), ptr(scratch), scratch.numel()) == -4          # BRX_E_OUTPUT
    assert lib.brx_output_needed(engine.ctx) == 3 and n.value == 0 and not lines.any()                   # ... and nothing written
    assert scan(ptr(d_text), len(text), None, 0, ctypes.byref(n), ptr(scratch), scratch.numel()) == -4 and lib.brx_output_needed(engine.ctx) == 3
    assert scan(ptr(d_text), len(text), ptr(lines), 3, ctypes.byref(n), ptr(scratch), scratch.numel()) == 0 and n.value == 3
    assert len(engine.paf_scan(d_text, cap=1)) == 3 and engine.paf_scan(d_text, cap=1).tobytes() == engine.paf_scan(d_text).tobytes()
    assert len(engine.paf_scan(d_text, 2, cap=1)) == 2
    # brx_align_pack
    pack = lambda job: lib.brx_align_pack(engine.ctx, ctypes.byref(job), engine._stream())
    job = E.BrxPackJob()
    assert pack(job) == 0                                                                                 # no alignment: nothing to do
    job.n_align = 1
    assert pack(job) == -1 and b'NULL' in lib.brx_last_error(engine.ctx)
    recs = engine.paf_scan(d_text)
    comp = upload(engine, bytes(range(256)))
    desc = np.zeros(1, dtype=E.PACK_ALIGN_DTYPE)
    for field in ('cigar_len', 'n_parts', 'sum_m', 'sum_i', 'sum_d'):
        desc[field] = recs[field][1]
    desc['cigar_off'], desc['ref_len'] = recs['line_off'][1] + recs['cigar_off'][1], 7
    off = lambda x: np.array([0, x], dtype=np.uint64)
    args = (d_text, upload(engine, b'ACGTACGTAC'), comp, desc, off(2), off(7), off(6), off(7))
    out = engine.align_pack(*args)
    assert host_array(out['part_len']).tolist() == [6, 1] and host_array(out['ref']).tobytes() == b'ACGTACG'
    for field, value in (('n_parts', 1), ('sum_m', 5), ('cigar_len', 3), ('cigar_off', len(text)), ('ref_off', 4), ('ref_len', 6)):
        wrong = desc.copy()
        wrong[field] = value
        with pytest.raises(E.BrxError) as e:                      # a descriptor that does not fit: refused, nothing out of range
            engine.align_pack(args[0], args[1], args[2], wrong, *args[4:])
        assert e.value.code == -1, field
    none = engine.align_pack(d_text, args[1], comp, desc[:0], off(0)[:1], off(0)[:1], off(0)[:1], off(0)[:1])
    assert all(host_array(t).tolist() == [0] for t in none.values())


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
MODEL_ARGS = {'error_model': ['--k_size', '4', '--max_alt', '3'], 'qscore_model': ['--k_size', '5', '--max_del', '2', '--min_occur', '2', '--max_output', '20']}


def check_cli(run, tmp_path, command, extra=(), folder='model_builder'):
    """run(command, argv) -> (exit status, stdout, the text on `output`): the same with and without --gpu-loader, the summary file too."""
    files = [x for k in ('reference', 'reads', 'alignment') for x in ('--' + k, os.path.join(GOLDEN_DIRS[folder], {'reference': 'ref.fasta', 'reads': 'reads.fastq', 'alignment': 'aln.paf'}[k]))]
    results = []
    for flag in ([], ['--gpu-loader']):
        argv = files + list(extra) + flag
        summary = None
        if command == 'plot':
            summary = tmp_path / f'summary{len(flag)}.tsv'
            argv += ['--no_plot', '--summary', str(summary)]
        else:
            argv += MODEL_ARGS[command]
        status, out, err = run(command, argv)
        # a child process shares its stderr with the GPU driver, which may print a line of its own when the device is opened -- and the
        # flag opens it earlier: of that stream only the command's own lines are compared
        err = ''.join(line for line in err.splitlines(True) if line.startswith(('Loading ', 'Choosing ', 'Processing ', 'Error')))
        results.append((status, out, err, summary.read_text() if summary else None))
    for k, what in enumerate(('exit status', 'stdout', 'the text on output', 'the summary')):
        assert results[0][k] == results[1][k], (what, results[0][k][-600:] if k else results[0][k], results[1][k][-600:] if k else results[1][k])
    assert results[0][0] == 0 and results[0][1]
    assert 'Loading alignments' in results[0][1] + results[0][2]


def check_help(run):
    for command in ('error_model', 'qscore_model', 'plot'):
        status, out, _ = run(command, ['--help'])
        assert status == 0 and '--gpu-loader' in out and 'MI355X' in out
        assert "Parse the PAF's CIGARs and pack the alignments on the GPU (same output)" in ' '.join(out.split())
