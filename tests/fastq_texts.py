"""
TEST INFRASTRUCTURE: the device read loader (--gpu-reads; include/brx.h: brx_fastq_scan, brx_reads_pack) against the code it stands in
for.  The yardsticks are the reference itself (tests/golden/fastq_texts.json.gz, written by tools/make_fastq_golden.py from the running
reference's load_fastq), a plain-Python restatement of its state machine (records_of), the host's own loader (misc.load_fastq) and packer
(model_builder.Job).  Every check takes the engine as its argument: tests/test_reads_loader.py passes the interpreted kernels
(tests/emu_engine.py), tests/test_gpu_reads_loader.py the MI355X.  Nothing here has a tolerance: every comparison is of integers, bytes
or text.
"""
import base64
import ctypes
import functools
import gzip
import io
import json
import os
import random

import numpy as np
import pytest

import paf_texts as PT
from badread_amd import engine as E
from badread_amd import model_builder as MB
from badread_amd import plot_window_identity as P
from badread_amd.alignment import load_alignments, load_alignments_device
from badread_amd.misc import load_fastq
from badread_amd.reads import DeviceReads, load_fastq_device

HERE = PT.HERE
BLANKS = b' \t\n\r\x0b\x0c'


# ---- the record rule, restated (the reference's load_fastq, misc.py:97-119) -------------------------------------------------------------
def lines_of(text):
    """(offset, bytes with the '\\n') of the lines a file of these bytes has"""
    out, at = [], 0
    for piece in text.split(b'\n'):
        out.append((at, piece + b'\n'))
        at += len(piece) + 1
    last_off, last = out.pop()                             # what lies behind the last '\n': a line only if it holds a byte
    if last != b'\n':
        out.append((last_off, last[:-1]))
    return out


def stripped_span(off, line):
    """(where the stripped line begins, its length); a line of blanks alone: (where the line ends, 0)"""
    core = line.strip(BLANKS)
    if not core:
        return off + len(line), 0
    return off + len(line) - len(line.lstrip(BLANKS)), len(core)


def records_of(text):
    """The reference's state machine over the lines: (the records as dicts of brx_fastq_rec's fields, the index of each header line).
    Raises what the reference raises: StopIteration for a record cut short, IndexError for a bare '@'."""
    lines = lines_of(text)
    recs, heads, i = [], [], 0
    while i < len(lines):
        off, line = lines[i]
        core = line.strip(BLANKS)
        if not core.startswith(b'@'):
            i += 1
            continue
        name = core[1:].split()[0]                         # IndexError: a bare '@'
        if i + 3 >= len(lines):
            raise StopIteration
        at, _ = stripped_span(off, line)
        name_at = at + 1 + (len(core[1:]) - len(core[1:].lstrip(BLANKS)))
        assert text[name_at:name_at + len(name)] == name
        seq_off, seq_len = stripped_span(*lines[i + 1])
        qual_off, qual_len = stripped_span(*lines[i + 3])
        recs.append(dict(head_off=off, name_off=name_at - off, name_len=len(name), seq_off=seq_off, seq_len=seq_len, qual_off=qual_off,
                         qual_len=qual_len, flags=0, reserved=0))
        heads.append(i)
        i += 4
    return recs, heads


def items_of(text):
    """What the reference's loader returns for these bytes, from the restated records: the dict's items in order."""
    reads = {}
    for r in records_of(text)[0]:
        name_at = r['head_off'] + r['name_off']
        reads[text[name_at:name_at + r['name_len']].decode()] = (text[r['seq_off']:r['seq_off'] + r['seq_len']].upper().decode(),
                                                                 text[r['qual_off']:r['qual_off'] + r['qual_len']].decode())
    return [[k, v[0], v[1]] for k, v in reads.items()]


def expected_layout(text):
    """The layout word include/brx.h promises for these bytes."""
    lines = lines_of(text)
    if len(lines) % 4:
        return E.FQ_LINES
    opens = lambda line: line.strip(BLANKS).startswith(b'@') and bool(line.strip(BLANKS)[1:].split())
    return (0 if all(opens(line) for _, line in lines[::4]) else E.FQ_HEADER) | (E.FQ_HIGH if any(c >= 0x80 for c in text) else 0)


def upload(engine, data):
    return PT.upload(engine, data)


def check_scan(engine, text, layout=None):
    """The layout word is the one the rule gives; with 0 the records are those of the restated state machine, whose headers then lie on
    the lines 0, 4, 8, ...; otherwise no record comes back.  layout: what the caller expects."""
    recs, got = engine.fastq_scan(upload(engine, text))
    assert got == expected_layout(text) and (layout is None or got == layout), (got, expected_layout(text), layout)
    if got:
        assert len(recs) == 0
        return recs
    want, heads = records_of(text)
    assert heads == list(range(0, 4 * len(want), 4)) and len(recs) == len(want) == len(lines_of(text)) // 4
    for field in E.FASTQ_REC_DTYPE.names:
        assert recs[field].tolist() == [r[field] for r in want], field
    return recs


# ---- the fixture from the running reference ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    with gzip.open(os.path.join(HERE, 'golden', 'fastq_texts.json.gz'), 'rt') as f:
        doc = json.load(f)
    for entry in doc['texts']:
        entry['bytes'] = base64.b64decode(entry['text'])
    return doc['texts']


REGULAR_NAMES = ('single', 'crlf', 'quality_begins_with_at', 'plus_line_with_text', 'header_forms', 'blanks_of_all_kinds', 'lower_case',
                 'empty_lines', 'repeated_name', 'no_final_newline', 'quality_longer_and_shorter', 'seven_records')
HOST_LAYOUT = {'blank_line_between_records': E.FQ_LINES, 'trailing_blank_line': E.FQ_LINES, 'four_trailing_blank_lines': E.FQ_HEADER,
               'three_lines': E.FQ_LINES, 'five_lines': E.FQ_LINES, 'six_lines': E.FQ_LINES, 'bare_at': E.FQ_HEADER,
               'bare_at_with_blanks': E.FQ_HEADER, 'line_4k_opens_no_record': E.FQ_HEADER, 'record_opens_off_the_grid': E.FQ_HEADER,
               'high_byte_in_name': E.FQ_HIGH, 'high_byte_in_sequence': E.FQ_HIGH, 'high_byte_in_plus_line': E.FQ_HIGH,
               'high_byte_in_quality': E.FQ_HIGH}
FIXTURE_NAMES = REGULAR_NAMES + tuple(HOST_LAYOUT)


def check_fixture_text(engine, tmp_path, name):
    """A text of the regular layout: layout 0, the records of the restatement, a DeviceReads with the reference's items.  Any other text:
    its layout bit, no record, and the host's loader with the reference's items or the reference's exception type.  Both: the
    reference's text on `output`."""
    assert [e['name'] for e in fixture()] == list(FIXTURE_NAMES)
    entry = next(e for e in fixture() if e['name'] == name)
    text = entry['bytes']
    regular = name in REGULAR_NAMES
    assert (entry['kind'] == 'regular') == regular
    check_scan(engine, text, 0 if regular else HOST_LAYOUT[name])
    try:                                                   # the restatement itself against the reference
        assert items_of(text) == entry['items']
    except (StopIteration, IndexError) as e:
        assert type(e).__name__ == entry['exception']
    path = tmp_path / 'reads.fastq'
    path.write_bytes(text)
    out = io.StringIO()
    if 'exception' in entry:
        with pytest.raises(BaseException) as e:
            load_fastq_device(str(path), engine, output=out, dot_interval=3)
        assert type(e.value).__name__ == entry['exception']
        assert out.getvalue() == entry['output']
        return
    reads = load_fastq_device(str(path), engine, output=out, dot_interval=3)
    assert isinstance(reads, DeviceReads) == regular and (regular or type(reads) is dict)
    assert [[k, reads[k][0], reads[k][1]] for k in reads.keys()] == entry['items'] and len(reads) == len(entry['items'])
    assert out.getvalue() == entry['output']


# ---- scan records against the restatement -----------------------------------------------------------------------------------------------
def check_committed(engine):
    for name, folder in PT.GOLDEN_DIRS.items():
        with open(os.path.join(folder, 'reads.fastq'), 'rb') as f:
            text = f.read()
        assert len(check_scan(engine, text, 0)) == text.count(b'\n') // 4 > 0


def nine_byte_text():
    """40.5 KB of 9-byte records: up to two line starts per 16-byte group, starts at every offset of a group, three tiles of the scan, and
    26 times the lines the first scratch holds (BRX_E_SCRATCH and the retry)."""
    return b'@a\nA\n+\n!\n' * 4500


def long_line_text():
    """One sequence line and one quality line of 40 KB: tiles of the scan without a line start."""
    return b'@s\nAC\n+\n!!\n@long one\n' + b'ACGT' * 10000 + b'\n+\n' + b'!#' * 20000 + b'\n@t\nG\n+\n#'


def check_synthetic(engine):
    text = nine_byte_text()
    starts = {off % 16 for off, _ in lines_of(text)}
    assert len(text) > 2 * 16 * E.DEPTH_TILE and starts == set(range(16))
    assert len(check_scan(engine, text, 0)) == 4500
    assert len(check_scan(engine, text[:-1], 0)) == 4500              # the last line without its newline: the same records
    check_scan(engine, text + b'\n', E.FQ_LINES)
    assert len(check_scan(engine, long_line_text(), 0)) == 3
    assert engine.fastq_scan(upload(engine, b''))[1] == 0


def big_text():
    """2 200 records of 2 kb from a seeded generator, 8.8 MB: more than 256 tiles of groups, so that the one workgroup that scans the tile
    sums takes more than one trip (GPU only)."""
    rng = random.Random(11)
    parts = []
    for k in range(2200):
        n = 1900 + rng.randrange(200)
        parts.append(b'@big%d len=%d\n%s\n+\n%s\n' % (k, n, bytes(rng.choice(b'ACGTacgtN') for _ in range(n)), bytes(33 + rng.randrange(60) for _ in range(n))))
    text = b''.join(parts)
    assert len(text) > 4 << 20 and len(text) / 16 / E.DEPTH_TILE > 256
    return text


# ---- load_fastq_device == load_fastq ----------------------------------------------------------------------------------------------------
def assert_same_reads(got, want):
    assert isinstance(got, DeviceReads) and list(got.keys()) == list(want.keys()) and len(got) == len(want)
    for name, pair in want.items():
        assert name in got and got[name] == pair and type(got[name]) is tuple and got.length(name) == len(pair[0]), name
    assert 'no such read' not in got
    with pytest.raises(KeyError):
        got['no such read']


def both_loaders(engine, path, dot_interval=1000):
    o1, o2 = io.StringIO(), io.StringIO()
    got, want = load_fastq_device(str(path), engine, output=o1, dot_interval=dot_interval), load_fastq(str(path), output=o2, dot_interval=dot_interval)
    assert o1.getvalue() == o2.getvalue()
    assert_same_reads(got, want)
    return got


def check_loader(engine, tmp_path):
    for name, folder in PT.GOLDEN_DIRS.items():
        for dot_interval in (7, 1000):
            both_loaders(engine, os.path.join(folder, 'reads.fastq'), dot_interval)
    text = next(e for e in fixture() if e['name'] == 'repeated_name')['bytes'] * 5
    path = tmp_path / 'reads.fastq'
    path.write_bytes(text)
    for dot_interval in (1, 7, 1000):
        assert len(both_loaders(engine, path, dot_interval)) == 3
    packed = tmp_path / 'reads.fastq.gz'
    with gzip.open(packed, 'wb') as f:
        f.write(text)
    assert len(both_loaders(engine, packed, 7)) == 3
    fasta = tmp_path / 'ref.fasta'
    fasta.write_text('>c\nACGT\n')
    for load in (load_fastq_device, lambda p, e, output: load_fastq(p, output=output)):
        out = io.StringIO()
        with pytest.raises(SystemExit) as e:
            load(str(fasta), engine, output=out)
        assert str(e.value.code) == f'Error: {fasta} is not FASTQ format' and out.getvalue() == ''


# ---- Job.packed with a DeviceReads == Job with load_fastq's dict --------------------------------------------------------------------------
def write_fastq(path, reads):
    """The reads as FASTQ, every third base lower-cased.  Some made jobs hold quality characters no FASTQ of the regular layout can
    (blanks, 0x80 and more): those are folded into '!'..'~', for both routes alike."""
    fold = lambda c: c if 33 <= ord(c) <= 126 else chr(33 + ord(c) % 94)
    with open(path, 'w', encoding='ascii', newline='') as f:
        for name, (seq, qual) in reads.items():
            f.write('@%s\n%s\n+\n%s\n' % (name, ''.join(c.lower() if i % 3 == 0 else c for i, c in enumerate(seq)), ''.join(map(fold, qual))))


def borders_case():
    """Read slices of 0, 1, 15, 16 and 17 bases that begin at every offset 0..16 of their reads, several slices inside one 16-byte group of
    the output, a 4096-byte tile border inside a slice and one exactly between two slices, a quality line longer than its sequence."""
    refs = {'ctg': 'ACGTTGCAAGGCTTAACCGGTTAGCATCGA' * 200}
    reads, lines, total, ends = {}, [], 0, []
    bases = lambda n, k: ''.join('ACGT'[(i * i + k) % 4] for i in range(n))
    quals = lambda n, k: ''.join(chr(33 + (i + 5 * k) % 90) for i in range(n))

    def add(n_seq, start, length, n_qual=None, end=None):
        nonlocal total
        k = len(reads)
        reads[f'b{k}'] = (bases(n_seq, k), quals(n_seq if n_qual is None else n_qual, k))
        end = start + length if end is None else end
        lines.append('\t'.join([f'b{k}', str(n_seq), str(start), str(end), '+-'[k & 1], 'ctg', '6000', '0', str(max(length, 1)), '1000', '1001', '60',
                                'AS:i:1', f'cg:Z:{length}M' if length else 'cg:Z:3S']))
        total += length
        ends.append(total)
    for start in range(17):
        add(40, start, (0, 1, 15, 16, 17)[start % 5])
    for _ in range(6):
        add(9, 2, 3)                                       # 18 bytes: several slices in one 16-byte group
    add(5000, 7, 4200 - total)                             # the first tile border inside a slice
    add(5000, 1000, 8192 - total)                          # the second exactly behind this one
    add(30, 0, 17)
    add(30, 4, 0)
    add(30, 29, 1)
    add(20, 3, 17, n_qual=26, end=40)                      # the quality line longer than its sequence, both clipped at their own end
    assert 4096 not in ends and 8192 in ends and total > 8192 and total % 16
    return refs, reads, lines


@functools.lru_cache(maxsize=None)
def packed_cases():
    return dict(PT.packed_cases(), borders=borders_case())


def both_kinds(engine, tmp_path, reads, lines):
    """(the DeviceReads, the dict, the DeviceAlignments, the host's list) of a job's reads and PAF lines written to files"""
    fastq, paf = tmp_path / 'reads.fastq', tmp_path / 'aln.paf'
    write_fastq(fastq, reads)
    paf.write_text('\n'.join(lines) + '\n')
    device_reads = both_loaders(engine, fastq)
    host_reads = load_fastq(str(fastq), output=io.StringIO())
    return device_reads, host_reads, load_alignments_device(str(paf), engine, output=io.StringIO()), load_alignments(str(paf), output=io.StringIO())


def check_packed_job(engine, tmp_path, name):
    """Every array of Job.packed over a DeviceReads, copied back, is the host Job's byte for byte: of the whole file and of the ranges
    paf_texts.check_packed_job takes."""
    refs, reads, lines = packed_cases()[name]
    device_reads, host_reads, packed, host = both_kinds(engine, tmp_path, reads, lines)
    n = len(host)
    assert n > 0 and len(packed) == n
    job = MB.Job.packed(engine, refs, device_reads, packed, 0, n)
    assert not isinstance(job.seq, np.ndarray) and not isinstance(job.qual, np.ndarray)                   # written on the device
    PT.assert_same_job(job, MB.Job(refs, host_reads, host), (name, 0, n))
    if name == 'borders':
        assert n == 29 and int(job.align_read_off[-1]) > 8192 and np.diff(job.align_read_off.astype(np.int64)).tolist()[:5] == [0, 1, 15, 16, 17]
    ranges = [(a, b) for a in range(n) for b in range(a, n + 1)] if n <= 6 else [(0, k) for k in range(1, n, max(n // 7, 1))] + [(k, n) for k in range(1, n, max(n // 7, 1))]
    for first, end in ranges:
        PT.assert_same_job(MB.Job.packed(engine, refs, device_reads, packed, first, end), MB.Job(refs, host_reads, host[first:end]), (name, first, end))


def check_plot_chunks(engine, tmp_path, monkeypatch):
    """paf_texts.check_plot_chunks' comparison with a DeviceReads: window_means over (DeviceReads, DeviceAlignments) gives what it gives
    over the host's dict and list, with a chunk border between any two alignments and without one."""
    refs, reads, lines = PT.packed_cases()['mixed']
    device_reads, host_reads, packed, host = both_kinds(engine, tmp_path, reads, lines[:60])
    for limit in (1 << 40, 3000, 1):
        monkeypatch.setattr(P, 'PLOT_CHUNK_BASES', limit)
        got = [(s.tolist(), e.tolist(), q.tolist()) for s, e, q in P.window_means(engine, refs, device_reads, packed, 33, True, values=True)]
        want = [(s.tolist(), e.tolist(), q.tolist()) for s, e, q in P.window_means(engine, refs, host_reads, host, 33, True, values=True)]
        assert got == want and len(got) == len(host)


# ---- exits ----------------------------------------------------------------------------------------------------------------------------------
def check_exits(engine, tmp_path, monkeypatch):
    """The cases of paf_texts.check_exits with a DeviceReads in place of the dict: the same messages in the same order.  Then a quality
    line shorter than its sequence and an unknown read, with the DeviceReads and with the dict."""
    refs, reads, lines = PT.shapes_job()
    fastq = tmp_path / 'shapes.fastq'
    write_fastq(fastq, reads)
    device_reads = both_loaders(engine, fastq)
    monkeypatch.setattr(PT, 'shapes_job', lambda: (refs, device_reads, lines))
    PT.check_exits(engine, tmp_path)
    monkeypatch.undo()
    reads = dict(reads, short=(reads['r0'][0], reads['r0'][1][:40]))
    write_fastq(fastq, reads)
    device_reads, host_reads = both_loaders(engine, fastq), load_fastq(str(fastq), output=io.StringIO())
    L = lambda name, re_: '\t'.join([name, '93', '0', str(re_), '+', 'ctg', '120', '0', '50', '1000', '1001', '60', 'AS:i:1', 'cg:Z:30M'])
    cases = {'a quality line shorter than its sequence': ([lines[0], L('short', 50)], 'runs past its read or reference range'),
             'a quality line shorter than its sequence, the slice inside it': ([lines[0], L('short', 40)], None),
             'an unknown read': ([lines[0], L('nobody', 50)], 'could not find read nobody')}
    for what, (case, end) in cases.items():
        path = tmp_path / 'exits.paf'
        path.write_text('\n'.join(case) + '\n')
        packed = load_alignments_device(str(path), engine, output=io.StringIO())
        for run in (lambda r: list(P.window_means(engine, refs, r, packed, 10, True)), lambda r: MB._job(engine, refs, r, packed)):
            ends = []
            for r in (device_reads, host_reads):
                try:
                    run(r)
                    ends.append(None)
                except SystemExit as e:
                    ends.append(str(e.code))
            assert ends[0] == ends[1] and (ends[0] is None if end is None else end in (ends[0] or '')), (what, ends)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def check_abi(engine):
    lib, torch = engine.lib, engine.torch
    text = b'@a\nACGT\n+\n!!!!\n@b x\nacgtacgt\n+\n########\n@c\nG\n+\n$'
    d_text = upload(engine, text)
    n, layout = ctypes.c_uint64(99), ctypes.c_uint32(99)
    room = int(lib.brx_fastq_scan_scratch(len(text)))
    scratch = torch.zeros(room, dtype=torch.uint8, device=engine.device)
    recs = torch.zeros(3 * E.FASTQ_REC_DTYPE.itemsize, dtype=torch.uint8, device=engine.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    scan = lambda t, nb, out, cap, nr, lay, scr, scr_n: lib.brx_fastq_scan(engine.ctx, t, nb, out, cap, nr, lay, scr, scr_n, engine._stream())
    nr, lay = ctypes.byref(n), ctypes.byref(layout)
    assert scan(None, 0, None, 0, nr, lay, None, 0) == 0 and (n.value, layout.value) == (0, 0)          # zero bytes: a valid call
    assert scan(ptr(d_text), len(text), ptr(recs), 3, None, lay, ptr(scratch), room) == -1
    assert scan(ptr(d_text), len(text), ptr(recs), 3, nr, None, ptr(scratch), room) == -1
    assert scan(None, len(text), ptr(recs), 3, nr, lay, ptr(scratch), room) == -1 and b'NULL' in lib.brx_last_error(engine.ctx)
    assert scan(ptr(d_text), len(text), ptr(recs), 3, nr, lay, None, 0) == -3 and lib.brx_scratch_needed(engine.ctx) == room
    assert scan(ptr(d_text), len(text), ptr(recs), 3, nr, lay, ptr(scratch), 64) == -3 and lib.brx_scratch_needed(engine.ctx) == room
    assert str(room).encode() in lib.brx_last_error(engine.ctx)                                         # ... with the size named
    assert scan(ptr(d_text), len(text), ptr(recs), 2, nr, lay, ptr(scratch), room) == -4                 # BRX_E_OUTPUT
    assert lib.brx_output_needed(engine.ctx) == 3 and n.value == 0 and not recs.any()                    # ... and nothing written
    assert scan(ptr(d_text), len(text), None, 0, nr, lay, ptr(scratch), room) == -4 and lib.brx_output_needed(engine.ctx) == 3
    assert scan(ptr(d_text), len(text), ptr(recs), 3, nr, lay, ptr(scratch), room) == 0 and (n.value, layout.value) == (3, 0)
    assert scan(ptr(d_text), 1 << 42, ptr(recs), 3, nr, lay, ptr(scratch), room) == -1
    got, word = engine.fastq_scan(d_text, cap=1)
    assert word == 0 and got.tobytes() == engine.fastq_scan(d_text)[0].tobytes() and got.tobytes() == recs.cpu().numpy().tobytes()
    assert [text[o:o + q] for o, q in zip((got['head_off'] + got['name_off']).tolist(), got['name_len'].tolist())] == [b'a', b'b', b'c']
    # a file of more lines than the first scratch holds: the size named, then success with it
    many = nine_byte_text()
    d_many, least = upload(engine, many), int(lib.brx_fastq_scan_scratch(len(many)))
    small = torch.zeros(least, dtype=torch.uint8, device=engine.device)
    out = torch.zeros(4500 * E.FASTQ_REC_DTYPE.itemsize, dtype=torch.uint8, device=engine.device)
    assert scan(ptr(d_many), len(many), ptr(out), 4500, nr, lay, ptr(small), least) == -3 and not out.any()
    more = int(lib.brx_scratch_needed(engine.ctx))
    assert more > least
    large = torch.zeros(more, dtype=torch.uint8, device=engine.device)
    assert scan(ptr(d_many), len(many), ptr(out), 4500, nr, lay, ptr(large), more) == 0 and (n.value, layout.value) == (4500, 0)
    # brx_reads_pack
    pack = lambda job: lib.brx_reads_pack(engine.ctx, ctypes.byref(job), engine._stream())
    job = E.BrxReadsJob()
    assert pack(job) == 0                                                                                 # no alignment: nothing to do
    job.n_align = 1
    assert pack(job) == -1 and b'NULL' in lib.brx_last_error(engine.ctx)
    u64 = lambda *x: np.array(x, dtype=np.uint64)
    seq, qual = engine.reads_pack(d_text, u64(got['seq_off'][1] + 2, got['seq_off'][0]), u64(got['qual_off'][1] + 2, got['qual_off'][0]), u64(0, 5, 9))
    assert PT.host_array(seq).tobytes() == b'GTACGACGT' and PT.host_array(qual).tobytes() == b'#####!!!!'
    for at in range(len(text) - 40, len(text) - 15):                # 16 bytes up to the last of the text: the wide loads stop in front of its end
        seq, qual = engine.reads_pack(d_text, u64(at), u64(at), u64(0, 16))
        assert PT.host_array(seq).tobytes() == text[at:at + 16].upper() and PT.host_array(qual).tobytes() == text[at:at + 16], at
    none = engine.reads_pack(d_text, u64(), u64(), u64(0))
    assert all(PT.host_array(t).tolist() == [0] for t in none)
    assert all(PT.host_array(t).tolist() == [0] for t in engine.reads_pack(d_text, u64(3), u64(3), u64(0, 0)))
    # a source past the text, offsets that descend: refused before a byte is written
    keep = [torch.from_numpy(x.view(np.int64).copy()).to(engine.device) for x in (u64(0, 3), u64(0, 3), u64(0, 4, 8))]
    outs = [torch.full((8,), 7, dtype=torch.uint8, device=engine.device) for _ in range(2)]
    flags = torch.zeros(4, dtype=torch.int32, device=engine.device)
    job.n_align, job.d_text, job.n_text = 2, d_text.data_ptr(), len(text)
    job.d_seq_src, job.d_qual_src, job.d_align_read_off = (t.data_ptr() for t in keep)
    job.d_seq, job.d_qual, job.d_flags = outs[0].data_ptr(), outs[1].data_ptr(), flags.data_ptr()
    assert pack(job) == 0 and PT.host_array(outs[0]).tobytes() == text[0:4].upper() + text[3:7].upper()
    for which, k, value in ((0, 1, len(text) - 3), (1, 1, len(text) - 3), (0, 0, len(text) + 1), (1, 0, 1 << 63), (2, 1, 9), (2, 0, 1), (2, 2, 3)):
        for t in outs:
            t.fill_(7)
        flags.zero_()
        held = int(keep[which][k])
        keep[which][k] = value if value < 1 << 63 else value - (1 << 64)
        assert pack(job) == -1 and int(flags[0]) == 1, (which, k, value)
        assert all(PT.host_array(t).tolist() == [7] * 8 for t in outs), (which, k, value)                # outputs untouched
        keep[which][k] = held
    flags.zero_()
    assert pack(job) == 0
    ms = engine.reads_last()
    assert set(ms) == {'scan', 'pack'}


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
READS_HELP = 'Parse the FASTQ and pack the read slices on the GPU (same output; needs --gpu-loader)'


def check_cli(run, tmp_path, command, extra=(), folder='model_builder'):
    """run(command, argv) -> (exit status, stdout, the text on `output`): the same with --gpu-loader --gpu-reads as with no flag, the
    summary file too."""
    files = [x for k in ('reference', 'reads', 'alignment') for x in ('--' + k, os.path.join(PT.GOLDEN_DIRS[folder], {'reference': 'ref.fasta', 'reads': 'reads.fastq', 'alignment': 'aln.paf'}[k]))]
    results = []
    for flag in ([], ['--gpu-loader', '--gpu-reads']):
        argv = files + list(extra) + flag
        summary = None
        if command == 'plot':
            summary = tmp_path / f'summary{len(flag)}.tsv'
            argv += ['--no_plot', '--summary', str(summary)]
        else:
            argv += PT.MODEL_ARGS[command]
        status, out, err = run(command, argv)
        err = ''.join(line for line in err.splitlines(True) if line.startswith(('Loading ', 'Choosing ', 'Processing ', 'Error')))     # as paf_texts.check_cli
        results.append((status, out, err, summary.read_text() if summary else None))
    for k, what in enumerate(('exit status', 'stdout', 'the text on output', 'the summary')):
        assert results[0][k] == results[1][k], (what, results[0][k][-600:] if k else results[0][k], results[1][k][-600:] if k else results[1][k])
    assert results[0][0] == 0 and results[0][1]
    assert 'Loading reads' in results[0][1] + results[0][2]


def check_flag_alone(run, command):
    files = [x for k in ('reference', 'reads', 'alignment') for x in ('--' + k, os.path.join(PT.GOLDEN_DIRS['model_builder'], {'reference': 'ref.fasta', 'reads': 'reads.fastq', 'alignment': 'aln.paf'}[k]))]
    status, out, err = run(command, files + ['--gpu-reads'] + (['--no_plot'] if command == 'plot' else []))
    assert status == 1 and 'Loading' not in out + err
    return out + err


def check_help(run):
    for command in ('error_model', 'qscore_model', 'plot'):
        status, out, _ = run(command, ['--help'])
        words = ' '.join(out.split())
        assert status == 0 and '--gpu-reads' in out and '--gpu-loader' in out and 'MI355X' in out
        assert READS_HELP in words and "Parse the PAF's CIGARs and pack the alignments on the GPU (same output)" in words
