"""
TEST INFRASTRUCTURE: --truth-bam-sorted in plain Python and numpy, for tests/test_bam_sorted.py (the emulated device) and
tests/test_gpu_bam_sorted.py (the MI355X).

The restatement of the contract (README, --truth-bam-sorted; include/brx.h, brx_bam_sort and brx_bam_index): `sort_records`, the stable
sort of decoded records by ((uint32) refID, pos); `reflen`; `table_of`, the lines of brx_bam_rec; `bai_of`, the bytes of the index from
a complete sorted BAM file and its own BGZF blocks.  `Reader` answers region queries through an index the way the standard reader does
(reg2bins, the linear index as a lower bound, a scan of the chunks that are left), and `self_check` holds it against brute force.

Record sets are made of SAM lines through bam_codec.bam_from (`lines`, `raw_of`); the `check_*` functions take a make_engine, so that one
body serves the emulator and the GPU.
"""
import bisect
import ctypes
import random
import struct

import numpy as np

import bam_codec as BC

BLOCK = 32768                       # BRX_BGZF_BLOCK
REF_OPS = (0, 2, 3, 7, 8)           # M D N = X
TILE = 1024                         # BRX_DEPTH_TILE
SPAN = 4096                         # the output bytes of a workgroup of the gather


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def split(raw):
    """The records of uncompressed BAM bytes, each with its block_size."""
    raw, at, out = bytes(raw), 0, []
    while at < len(raw):
        size = struct.unpack_from('<I', raw, at)[0] + 4
        out.append(raw[at:at + size])
        at += size
    assert at == len(raw)
    return out


def key_of(rec):
    rid, pos = struct.unpack_from('<ii', rec, 4)
    return (rid & 0xFFFFFFFF, pos)


def sort_records(raw):
    """The records in the order of the sorted file: by ((uint32) refID, pos); Python's sort is stable."""
    return b''.join(sorted(split(raw), key=key_of))


def reflen(rec):
    """The reference bases of the CIGAR field, 0 counting as 1."""
    l_name, n_cigar = rec[12], struct.unpack_from('<H', rec, 16)[0]
    words = struct.unpack_from(f'<{n_cigar}I', rec, 36 + l_name)
    return sum(w >> 4 for w in words if (w & 15) in REF_OPS) or 1


def table_of(sorted_raw):
    """The lines of brx_bam_rec of a sorted record stream (engine.BAM_REC_DTYPE)."""
    from badread_amd import engine as E
    recs, at = split(sorted_raw), 0
    table = np.zeros(len(recs), dtype=E.BAM_REC_DTYPE)
    for i, rec in enumerate(recs):
        rid, pos = struct.unpack_from('<ii', rec, 4)
        table[i] = (at, rid, pos, 0 if rid < 0 else pos + reflen(rec), struct.unpack_from('<H', rec, 14)[0])
        at += len(rec)
    return table


def block_walk(blob):
    """(compressed offset, payload) of every BGZF block of `blob`, by its BSIZE field; bam_codec.bgzf_blocks checks the framing."""
    payloads, offs, at = BC.bgzf_blocks(blob), [], 0
    for _ in payloads:
        offs.append(at)
        at += struct.unpack_from('<H', blob, at + 16)[0] + 1
    assert at == len(blob)
    return list(zip(offs, payloads))


def header_bytes(stream):
    """The length of the BAM header at the head of an uncompressed BAM stream, and n_ref."""
    assert stream[:4] == b'BAM\1'
    at = 8 + struct.unpack_from('<i', stream, 4)[0]
    n_ref = struct.unpack_from('<i', stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from('<i', stream, at)[0]
    return at, n_ref


class File(object):
    """A complete sorted BAM file taken apart: its header text, n_ref, its records (rid, pos, end, bin) with their virtual offsets.  The
    header fills blocks of its own; the record stream behind it is cut into blocks of 32768 bytes, the last what is left, so byte u of
    the stream has the virtual offset (the file offset of block u // 32768) << 16 | u % 32768 -- the EOF block's where u is the stream's
    length and a multiple of 32768."""

    def __init__(self, blob):
        blocks = block_walk(blob)
        assert blocks and blocks[-1][1] == b'' and all(p for _, p in blocks[:-1]), 'the EOF block ends the file, and only it is empty'
        self.stream = b''.join(p for _, p in blocks)
        head, self.n_ref = header_bytes(self.stream)
        self.text = self.stream[8:8 + struct.unpack_from('<i', self.stream, 4)[0]]
        self.raw = self.stream[head:]
        at, first = 0, None
        for i, (_, payload) in enumerate(blocks):
            if at == head:
                first = i
                break
            at += len(payload)
        assert first is not None, 'the records begin with a block of their own'
        assert all(len(p) == BLOCK for _, p in blocks[first:-2]) and len(blocks) - 1 - first == -(-len(self.raw) // BLOCK)
        self.coff = [off for off, _ in blocks[first:]]
        self.recs, at = [], 0
        for rec in split(self.raw):
            rid, pos = struct.unpack_from('<ii', rec, 4)
            self.recs.append(dict(rid=rid, pos=pos, end=0 if rid < 0 else pos + reflen(rec), bin=struct.unpack_from('<H', rec, 14)[0],
                                  voff=self.voff(at), vend=self.voff(at + len(rec)), raw=rec))
            at += len(rec)
        self.voffs = [r['voff'] for r in self.recs]
        assert self.voffs == sorted(self.voffs)

    def voff(self, u):
        return self.coff[u // BLOCK] << 16 | u % BLOCK


def bai_of(blob):
    """The .bai bytes of a complete, sorted BAM file, from its own blocks and records (README, --truth-bam-sorted: the .bai bytes)."""
    f = File(blob)
    out = [b'BAI\1', struct.pack('<i', f.n_ref)]
    for rid in range(f.n_ref):
        mine = [r for r in f.recs if r['rid'] == rid]
        bins, prev = {}, None
        for r in f.recs:                                        # chunks: runs consecutive in the file, on one contig, in one bin
            if r['rid'] == rid:
                if prev is not None and prev['rid'] == rid and prev['bin'] == r['bin']:
                    bins[r['bin']][-1][1] = r['vend']
                else:
                    bins.setdefault(r['bin'], []).append([r['voff'], r['vend']])
            prev = r
        out.append(struct.pack('<i', len(bins)))
        for b in sorted(bins):
            out.append(struct.pack('<Ii', b, len(bins[b])) + b''.join(struct.pack('<QQ', beg, end) for beg, end in bins[b]))
        n_intv = ((max(r['end'] for r in mine) - 1) >> 14) + 1 if mine else 0
        linear = [None] * n_intv
        for w in range(n_intv):
            hit = [r for r in mine if r['pos'] < (w + 1) << 14 and r['end'] > w << 14]
            linear[w] = hit[0]['voff'] if hit else None
        for w in range(n_intv - 2, -1, -1):                     # a window no record overlaps: the next one that has one
            if linear[w] is None:
                linear[w] = linear[w + 1]
        assert all(x is not None for x in linear)
        out.append(struct.pack('<i', n_intv) + b''.join(struct.pack('<Q', x) for x in linear))
    out.append(struct.pack('<Q', sum(r['rid'] < 0 for r in f.recs)))
    return b''.join(out)


# ---------------------------------------------------------------------------------------------
# a reader
# ---------------------------------------------------------------------------------------------
def reg2bins(beg, end):
    """SAM spec v1 section 5.3: the bins that may hold records overlapping [beg, end)."""
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += range(first + (beg >> shift), first + (end >> shift) + 1)
    return bins


class Reader(object):
    """Region queries through a .bai: the chunks of reg2bins, those dropped that end at or before ioffset[beg >> 14], the rest scanned."""

    def __init__(self, bai, file):
        self.file = file
        assert bai[:4] == b'BAI\1'
        n_ref, at = struct.unpack_from('<i', bai, 4)[0], 8
        self.refs = []
        for _ in range(n_ref):
            n_bin, bins = struct.unpack_from('<i', bai, at)[0], {}
            at += 4
            order = []
            for _ in range(n_bin):
                b, n_chunk = struct.unpack_from('<Ii', bai, at)
                at += 8
                bins[b] = [struct.unpack_from('<QQ', bai, at + 16 * i) for i in range(n_chunk)]
                at += 16 * n_chunk
                order.append(b)
            assert order == sorted(set(order))
            n_intv = struct.unpack_from('<i', bai, at)[0]
            linear = list(struct.unpack_from(f'<{n_intv}Q', bai, at + 4))
            at += 4 + 8 * n_intv
            self.refs.append((bins, linear))
        self.n_no_coor = struct.unpack_from('<Q', bai, at)[0]
        assert at + 8 == len(bai)

    def query(self, rid, beg, end):
        """The numbers (in file order) of the records of contig rid that overlap [beg, end)."""
        bins, linear = self.refs[rid]
        if not linear:
            return []
        floor = linear[min(beg >> 14, len(linear) - 1)] if (beg >> 14) < len(linear) else None
        if floor is None:                                       # behind the contig's last window: nothing ends there
            return []
        found, voffs, recs = set(), self.file.voffs, self.file.recs
        for b in reg2bins(beg, end):
            for c_beg, c_end in bins.get(b, ()):
                if c_end <= floor:
                    continue
                for i in range(bisect.bisect_left(voffs, c_beg), bisect.bisect_left(voffs, c_end)):
                    if recs[i]['rid'] == rid and recs[i]['pos'] < end and recs[i]['end'] > beg:
                        found.add(i)
        return sorted(found)


def brute(file, rid, beg, end):
    return [i for i, r in enumerate(file.recs) if r['rid'] == rid and r['pos'] < end and r['end'] > beg]


def queries(file, lengths, seed, count=200):
    """A fixed random set of regions: short and long, at window and bin borders, and every record's own span and its neighbours."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        rid = rng.randrange(len(lengths))
        span = rng.choice((1, 2, 100, 16384, 16385, 1 << 17, 1 << 20, lengths[rid]))
        beg = rng.choice((rng.randrange(max(lengths[rid], 1)), (rng.randrange(max(lengths[rid], 1)) >> 14) << 14))
        out.append((rid, beg, min(beg + span, max(lengths[rid], beg + 1))))
    for r in file.recs:
        if r['rid'] >= 0:
            out += [(r['rid'], r['pos'], r['end']), (r['rid'], r['end'], r['end'] + 1), (r['rid'], max(r['pos'] - 1, 0), max(r['pos'], 1)),
                    (r['rid'], r['end'] - 1, r['end']), (r['rid'], r['pos'], r['pos'] + 1)]
    return out


def check_queries(bai, blob, lengths, seed=7):
    file = File(blob)
    reader = Reader(bai, file)
    assert reader.n_no_coor == sum(r['rid'] < 0 for r in file.recs)
    for rid, beg, end in queries(file, lengths, seed):
        assert reader.query(rid, beg, end) == brute(file, rid, beg, end), (rid, beg, end)


# ---------------------------------------------------------------------------------------------
# record sets
# ---------------------------------------------------------------------------------------------
def line(i, rid, pos, cigar='10M', l_seq=None, names=None, flag=0, tags='NM:i:0\tAS:i:0'):
    """One SAM line for bam_from: read number i on contig rid (None: unmapped) at 0-based pos; SEQ of l_seq bases."""
    n = l_seq if l_seq is not None else sum(int(x) for x, op in BC._CIGAR.findall(cigar) if op in 'MIS') or 1
    seq, qual = ('ACGT' * (n // 4 + 1))[:n], ('5' * n)
    if rid is None:
        return f'{i:036d}\t4\t*\t0\t0\t*\t*\t0\t0\t{seq}\t{qual}\tCO:Z:u\n'
    return f'{i:036d}\t{flag}\t{names[rid]}\t{pos + 1}\t60\t{cigar}\t*\t0\t0\t{seq}\t{qual}\t{tags}\n'


def raw_of(lines, names, limit=65535):
    """(the BAM records of the lines, the offsets of a segment per line)."""
    recs = [BC.bam_from(x.encode(), names, limit) for x in lines]
    off = np.concatenate(([0], np.cumsum([len(r) for r in recs]))).astype(np.uint64)
    return b''.join(recs), off


def names_of(n):
    return [f'c{i}' for i in range(n)]


def random_set(rng, n, n_ref, length, unmapped=0.1, l_seq=(1, 40), reach=(1, 400)):
    """n lines over n_ref contigs of `length` bases: random positions and spans, some unmapped."""
    names, out = names_of(n_ref), []
    for i in range(n):
        if rng.random() < unmapped:
            out.append(line(i, None, 0, l_seq=rng.randint(*l_seq)))
        else:
            span = rng.randint(*reach)
            pos = rng.randrange(max(length - span, 1))
            out.append(line(i, rng.randrange(n_ref), pos, f'{span}M', l_seq=rng.randint(*l_seq), names=names))
    return out, names


def sort_cases():
    """(label, lines, names, max_pos, segments or None: one per line, max_cigar_ops) of the sort and gather checks."""
    rng = random.Random(11)
    cases = []
    for n in (0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 3073):          # thread, tile and multi-tile borders of BRX_DEPTH_TILE
        lines, names = random_set(rng, n, 3, 70000, l_seq=(1, 6))
        cases.append((f'count_{n}', lines, names, 70000, None, 65535))
    names = names_of(1)
    cases.append(('all_equal', [line(i, 0, 777, l_seq=1 + i % 5, names=names) for i in range(300)], names, 1000, None, 65535))
    cases.append(('ascending', [line(i, 0, 3 * i, names=names) for i in range(300)], names, 1000, None, 65535))
    cases.append(('descending', [line(i, 0, 3 * (299 - i), names=names) for i in range(300)], names, 1000, None, 65535))
    cases.append(('alternating', [line(i, 0, (500, 20)[i & 1], l_seq=1 + i % 7, names=names) for i in range(300)], names, 1000, None, 65535))
    names = names_of(3)                                                  # the middle contig empty
    cases.append(('three_contigs', [line(i, (0, 2)[rng.randrange(2)], rng.randrange(900), names=names) for i in range(200)], names, 1000, None, 65535))
    names = names_of(257)                                                # a second contig digit
    cases.append(('257_contigs', [line(i, rng.randrange(257), rng.randrange(900), names=names) for i in range(600)], names, 1000, None, 65535))
    names = names_of(2)                                                  # the top position digit
    top = 2 ** 29 - 100
    cases.append(('top_digit', [line(i, i & 1, rng.choice((rng.randrange(top), top - 1 - rng.randrange(1 << 24))), '50M', l_seq=3, names=names)
                                for i in range(300)], names, 2 ** 29, None, 65535))
    cases.append(('no_unmapped', random_set(rng, 200, 2, 5000, unmapped=0.0)[0], names, 5000, None, 65535))
    cases.append(('all_unmapped', [line(i, None, 0, l_seq=1 + i % 9) for i in range(200)], names, 5000, None, 65535))
    cases.append(('interleaved', [line(i, None, 0, l_seq=2) if i & 1 else line(i, 0, 4000 - i, names=names) for i in range(200)], names, 5000, None, 65535))
    lines = random_set(rng, 120, 2, 5000)[0]                             # segments of 0, 1 and several records
    cases.append(('segments', lines, names, 5000, [0, 0, 1, 1, 4, 4, 4, 9, 50, 119, 120, 120], 65535))
    # sizes: records that straddle the gather's span border and its 16-byte lanes, the smallest record between two large ones, and one
    # record of more than 64 KB
    sizes = [line(0, 0, 900, l_seq=2600, names=names), line(1, 1, 5, l_seq=1, names=names), line(2, 0, 100, l_seq=2700, names=names),
             line(3, 0, 50, l_seq=50000, names=names), line(4, None, 0, l_seq=1), line(5, 1, 4, l_seq=2731, names=names),
             line(200, 1, 6, l_seq=2900, names=names)]
    sizes += [line(6 + i, i & 1, 3000 - 7 * i, l_seq=1 + (i * 37) % 23, names=names) for i in range(150)]
    cases.append(('sizes', sizes, names, 5000, None, 65535))
    # a long-CIGAR record among short ones: reflen from the placeholder's N
    longc = [line(i, 0, 10 * i, '3S' + '2M1I1M1D' * 6 + '2S', names=names) for i in range(20)]
    cases.append(('long_cigar', longc, names, 5000, None, 8))
    return cases


def index_cases():
    """(label, lines, names, lengths, max_cigar_ops) of the index checks; the lines in any order, the check sorts them."""
    rng = random.Random(5)
    names, lengths = names_of(3), [2 ** 27 + 5000, 50000, 300000]
    edges = [line(0, 0, 16383, '1M', names=names), line(1, 0, 16384, '1M', names=names), line(2, 0, 16000, '384M', names=names),     # end 16384
             line(3, 0, 16000, '385M', names=names)]                                                                                 # end 16385
    for i, border in enumerate((2 ** 17, 2 ** 20, 2 ** 23, 2 ** 26)):
        edges.append(line(4 + i, 0, border - 30, '60M', l_seq=3, names=names))
    edges.append(line(8, 0, 2 ** 26 - 10, f'{2 ** 26 + 20}M', l_seq=3, names=names))                     # bin 0
    edges.append(line(9, 0, 40 * 16384 + 5, '3M', names=names))                                          # empty windows before, between and after
    edges.append(line(10, 0, 90 * 16384 + 5, '3M', names=names))
    edges.append(line(11, 2, 5 * 16384, f'{10 * 16384}M', l_seq=2, names=names))                         # a long record, short ones inside it
    edges += [line(12 + i, 2, 6 * 16384 + 1000 * i, '20M', names=names) for i in range(30)]
    edges += [line(50 + i, None, 0, l_seq=4) for i in range(3)]                                          # contig 1 without records
    cases = [('edges', edges, names, lengths, 65535)]
    lines = random_set(rng, 300, 3, 200000, reach=(1, 70000))[0]
    cases.append(('random', lines, names, [200000] * 3, 65535))
    longc = [line(i, 0, 1000 * i, '3S' + '200M1I100M1D' * 6 + '2S', l_seq=20, names=names) for i in range(40)]
    longc += [line(40 + i, 0, 500 * i, '30M', names=names) for i in range(40)]
    cases.append(('long_cigar', longc, names, lengths, 8))
    cases.append(('nothing', [], names, lengths, 65535))
    cases.append(('only_unmapped', [line(i, None, 0, l_seq=3) for i in range(5)], names, lengths, 65535))
    return cases


class Ref(object):
    """What output.bam_header reads of a reference."""

    def __init__(self, names, lengths):
        self.names, self.lengths = names, lengths


SORTED_TEXT = b'@HD\tVN:1.6\tSO:coordinate\n'


def file_of(sorted_blob, names, lengths):
    """A complete BAM file around the BGZF blocks of a sorted record stream: (its bytes, the compressed length of its header)."""
    from badread_amd import output as O
    head = O.bgzf_host(O.bam_header(Ref(names, lengths), SORTED_TEXT))
    return head + sorted_blob + O.BGZF_EOF, len(head)


def python_blocks(data, block=BLOCK):
    """`data` as BGZF blocks of `block` input bytes, by zlib; (the blob, the offsets of the blocks and of its end)."""
    from badread_amd import output as O
    parts = [O.bgzf_block(data[at:at + block]) for at in range(0, len(data), block)]
    return b''.join(parts), np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.uint64)


def self_check(rounds=300, seed=3):
    """Reader against brute force on random record sets, through bai_of: the construction of the index is one a standard reader can use."""
    rng = random.Random(seed)
    for k in range(rounds):
        n_ref = rng.randint(1, 3)
        length = rng.choice((40000, 300000, 2 ** 21))
        lines, names = random_set(rng, rng.randint(0, 40), n_ref, length, reach=(1, rng.choice((50, 20000, length // 2))), l_seq=(1, rng.choice((4, 3000))))
        raw = sort_records(raw_of(lines, names)[0])
        blob, _ = file_of(python_blocks(raw)[0], names, [length] * n_ref)
        check_queries(bai_of(blob), blob, [length] * n_ref, seed=k)


# ---------------------------------------------------------------------------------------------
# the checks, shared by the emulator's file and the GPU's
# ---------------------------------------------------------------------------------------------
def up(eng, data):
    return eng.torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(eng.device)


def down(t):
    return bytes(t.cpu().numpy())


def check_sort_case(eng, case):
    """brx_bam_sort against the restatement, byte for byte: the sorted stream, the table and the two counts."""
    from badread_amd import engine as E
    label, lines, names, max_pos, segments, limit = case
    raw, off = raw_of(lines, names, limit)
    if segments is not None:
        off = off[np.array(segments)]
    want = sort_records(raw)
    got, table, n, unmapped = eng.bam_sort(up(eng, raw), off, len(names), max_pos)
    assert down(got) == want, label
    want_table = table_of(want)
    assert n == len(want_table) and unmapped == int((want_table['refID'] < 0).sum()), label
    assert np.array_equal(np.frombuffer(down(table), dtype=E.BAM_REC_DTYPE), want_table), label
    return want


def check_sizes_case_is_what_it_says():
    """The record set 'sizes' does what its comment claims, for the spans and lanes of the gather."""
    case = [c for c in sort_cases() if c[0] == 'sizes'][0]
    raw, _ = raw_of(case[1], case[2])
    recs = split(sort_records(raw))
    ends = np.cumsum([len(r) for r in recs])
    assert max(len(r) for r in recs) > 65536 and min(len(r) for r in recs) < 100
    assert any((e - len(r)) // SPAN != (e - 1) // SPAN for r, e in zip(recs, ends))              # a record over a span border
    assert any(e % 16 for e in ends) and any(len(r) < 16 * 7 for r in recs)                       # borders inside 16-byte lanes
    small = [i for i, r in enumerate(recs) if len(r) < 100]
    assert any(0 < i < len(recs) - 1 and len(recs[i - 1]) > 3000 and len(recs[i + 1]) > 3000 for i in small)


def sized_line(i, pos, size, names):
    """A mapped line whose BAM record has exactly `size` bytes: SEQ and QUAL take l + ceil(l / 2) bytes, NM:i:300 one more than NM:i:0."""
    base = len(raw_of([line(0, 0, 0, l_seq=1, names=names)], names)[0]) - 2
    for tags, extra in (('NM:i:0\tAS:i:0', 0), ('NM:i:300\tAS:i:0', 1)):
        guess = 2 * (size - base - extra) // 3
        for l_seq in range(max(guess - 2, 1), guess + 3):
            if base + extra + l_seq + (l_seq + 1) // 2 == size:
                return line(i, 0, pos, '1M', l_seq=l_seq, names=names, tags=tags)
    raise AssertionError(size)


def grid_cases():
    """(label, lines, names, lengths, max_cigar_ops), sorted record streams for the BGZF grid: lengths 32767, 32768, 32769 and an exact
    multiple of 32768, a record that begins exactly on a block border and one that spans three blocks."""
    names = names_of(1)

    def stream(total, first=()):
        lines, at = [], 0
        for size in first:
            lines.append(sized_line(len(lines), len(lines), size, names))
            at += size
        while total - at > 700:
            size = 150 + 37 * (len(lines) % 11)
            lines.append(sized_line(len(lines), len(lines), size, names))
            at += size
        if total - at:
            assert total - at > 120
            lines.append(sized_line(len(lines), len(lines), total - at, names))
        assert len(raw_of(lines, names)[0]) == total
        return lines
    cases = [(f'len_{total}', stream(total), names, [100000], 65535) for total in (32767, 32768, 32769, 3 * 32768)]
    cases.append(('on_a_border', stream(2 * 32768 + 999, (20000, 12768, 200)), names, [100000], 65535))
    cases.append(('three_blocks', stream(4 * 32768, (30000, 70000)), names, [100000], 65535))
    return cases


def check_grid_case(eng, case):
    """brx_bgzf_device_off on a record stream: the blob is brx_bgzf_device's, the offsets are the walk of its BSIZE fields, the blocks hold
    32768 input bytes each, the last what is left.  Then the index over these blocks (check_index_case)."""
    label, lines, names = case[:3]
    raw = raw_of(lines, names)[0]
    assert raw == sort_records(raw)
    src = up(eng, raw)
    blob, off = eng.bgzf_device(src, offsets=True)
    blob = down(blob)
    assert blob == down(eng.bgzf_device(src)), label
    walk = block_walk(blob)
    assert [int(x) for x in off] == [o for o, _ in walk] + [len(blob)], label
    assert b''.join(p for _, p in walk) == raw and all(len(p) == BLOCK for _, p in walk[:-1]) and len(walk) == -(-len(raw) // BLOCK), label
    check_index_case(eng, case)


def check_index_case(eng, case):
    """brx_bam_index against the restatement, byte for byte, on the table and the blocks the device made; every query of the fixed set
    answered as brute force answers it."""
    label, lines, names, lengths, limit = case
    raw, off = raw_of(lines, names, limit)
    want = sort_records(raw)
    got, table, n, unmapped = eng.bam_sort(up(eng, raw), off, len(names), 2 ** 29)
    assert down(got) == want, label
    blob, block_off = eng.bgzf_device(got, offsets=True) if n else (eng.torch.zeros(0, dtype=eng.torch.uint8), np.zeros(1, dtype=np.uint64))
    whole, base = file_of(down(blob), names, lengths)
    bai = down(eng.bam_index(table, len(names), len(want), block_off, base))
    assert bai == bai_of(whole), label
    check_queries(bai, whole, lengths)
    return whole, bai


# ---- the ABI: every refusal returns its code, writes nothing and leaves the context usable --------------------------------------------
def _sort_call(eng, raw, off, n_ref, max_pos, rec_cap=None, scratch=None, fill=0xAB):
    """brx_bam_sort called by hand: (rc, the sorted buffer, the table buffer, n, unmapped).  The buffers are preset to `fill`."""
    torch = eng.torch
    src, d_off = up(eng, raw if len(raw) else b'\0'), eng.torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64).copy()).to(eng.device)
    cap = rec_cap if rec_cap is not None else len(raw) // 36 + 1
    out = torch.full((max(len(raw), 1),), fill, dtype=torch.uint8, device=eng.device)
    table = torch.full((max(cap, 1) * 24,), fill, dtype=torch.uint8, device=eng.device)
    need = int(eng.lib.brx_bam_sort_scratch(len(raw), len(off) - 1))
    scr = torch.empty(max(scratch if scratch is not None else 64 * need, 8), dtype=torch.uint8, device=eng.device)
    n, unmapped = ctypes.c_uint64(99), ctypes.c_uint64(99)
    rc = eng.lib.brx_bam_sort(eng.ctx, ctypes.c_void_p(src.data_ptr()), len(raw), ctypes.c_void_p(d_off.data_ptr()), len(off) - 1, n_ref, max_pos,
                              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(table.data_ptr()), cap, ctypes.byref(n), ctypes.byref(unmapped),
                              ctypes.c_void_p(scr.data_ptr()), scr.numel(), eng._stream())
    return rc, down(out), down(table), n.value, unmapped.value


def check_sort_abi(eng):
    from badread_amd import engine as E
    names = names_of(2)
    lines = [line(i, i & 1, 100 - i, l_seq=5, names=names) for i in range(40)] + [line(40, None, 0, l_seq=3)]
    raw, off = raw_of(lines, names)
    untouched = lambda got: set(got[1]) == {0xAB} and set(got[2]) == {0xAB} and got[3] == 0 and got[4] == 0
    good = lambda: check_sort_case(eng, ('after a refusal', lines, names, 1000, None, 65535))
    good()
    size = struct.unpack_from('<I', raw, 0)[0]
    # a chain that overruns its segment: the first record claims one byte more than its segment holds; and one that ends inside it
    for claimed in (size + 1, size - 1, len(raw)):
        bad = struct.pack('<I', claimed) + raw[4:]
        got = _sort_call(eng, bad, off, 2, 1000)
        assert got[0] == -1 and untouched(got), claimed
        good()
    # a block_size of 0, and one below the fixed fields and the name
    for claimed in (0, 31, 32 + 36):
        got = _sort_call(eng, struct.pack('<I', claimed) + raw[4:], off, 2, 1000)
        assert got[0] == -1 and untouched(got), claimed
    good()
    # a segment of fewer than 36 bytes that is not empty
    short = np.array([0, 20, len(raw)], dtype=np.uint64)
    assert _sort_call(eng, raw, short, 2, 1000)[0] == -1
    # offsets that descend, that do not begin at 0, that do not end at n_bytes or run past it
    for wrong in (off[[0, 5, 3, -1]], off[[1, 5, -1]], off[[0, 5, -2]], np.append(off[:-1], off[-1] + 100)):
        got = _sort_call(eng, raw, wrong, 2, 1000)
        assert got[0] == -1 and untouched(got), wrong
    good()
    # refID out of range: the records name contig 1 of a reference of one; refID -2; a position the keys cannot hold
    assert _sort_call(eng, raw, off, 1, 1000)[0] == -1
    assert _sort_call(eng, raw[:4] + struct.pack('<i', -2) + raw[8:], off, 2, 1000)[0] == -1
    got = _sort_call(eng, raw, off, 2, 100)                                  # pos 100 with max_pos 100
    assert got[0] == -1 and untouched(got)
    good()
    # NULLs
    assert eng.lib.brx_bam_sort(eng.ctx, None, len(raw), None, 1, 2, 1000, None, None, 0, None, None, None, 0, eng._stream()) == -1
    # a small rec_cap: BRX_E_OUTPUT and the records needed; a small scratch: BRX_E_SCRATCH and the bytes needed
    got = _sort_call(eng, raw, off, 2, 1000, rec_cap=40)
    assert got[0] == E.E_OUTPUT and int(eng.lib.brx_output_needed(eng.ctx)) == 41 and untouched(got)
    got = _sort_call(eng, raw, off, 2, 1000, scratch=1000)
    assert got[0] == E.E_SCRATCH and int(eng.lib.brx_scratch_needed(eng.ctx)) == int(eng.lib.brx_bam_sort_scratch(len(raw), 41)) and untouched(got)
    # more records than brx_bam_sort_scratch assumes: the size for the count found
    many = [line(i, 0, i, l_seq=1, names=names) for i in range(3000)]
    raw_many, off_many = raw_of(many, names)
    one = np.array([0, len(raw_many)], dtype=np.uint64)
    least = int(eng.lib.brx_bam_sort_scratch(len(raw_many), 1))
    got = _sort_call(eng, raw_many, one, 2, 5000, scratch=least)
    assert got[0] == E.E_SCRATCH and int(eng.lib.brx_scratch_needed(eng.ctx)) > least and untouched(got)
    got = _sort_call(eng, raw_many, one, 2, 5000, scratch=int(eng.lib.brx_scratch_needed(eng.ctx)))
    assert got[0] == 0 and got[1] == raw_many and got[3] == 3000 and got[4] == 0
    # zero bytes is a valid call
    got = _sort_call(eng, b'', np.zeros(1, dtype=np.uint64), 2, 1000)
    assert got[0] == 0 and got[3] == 0 and got[4] == 0
    good()


def _index_call(eng, table, n_ref, n_bytes, block_off, base, out_cap=None, scratch=None):
    torch = eng.torch
    n = len(table)
    d_table = up(eng, table.tobytes() if n else b'\0' * 24)
    d_off = torch.from_numpy(np.ascontiguousarray(block_off, dtype=np.uint64).view(np.int64).copy()).to(eng.device)
    cap = out_cap if out_cap is not None else 1 << 20
    out = torch.full((max(cap, 8),), 0xAB, dtype=torch.uint8, device=eng.device)
    need = int(eng.lib.brx_bam_index_scratch(n, n_ref))
    scr = torch.empty(max(scratch if scratch is not None else need, 8), dtype=torch.uint8, device=eng.device)
    got = ctypes.c_size_t(99)
    rc = eng.lib.brx_bam_index(eng.ctx, ctypes.c_void_p(d_table.data_ptr()), n, n_ref, n_bytes, ctypes.c_void_p(d_off.data_ptr()), len(block_off) - 1, base,
                               ctypes.c_void_p(out.data_ptr()), cap, ctypes.byref(got), ctypes.c_void_p(scr.data_ptr()), scr.numel(), eng._stream())
    return rc, down(out), got.value


def check_index_abi(eng):
    from badread_amd import engine as E
    names, lengths = names_of(2), [100000, 100000]
    lines = [line(i, i & 1, 700 * i, '900M', l_seq=4, names=names) for i in range(60)] + [line(60, None, 0, l_seq=3)]
    want = sort_records(raw_of(lines, names)[0])
    table = table_of(want)
    blob, block_off = python_blocks(want)
    whole, base = file_of(blob, names, lengths)
    right = bai_of(whole)
    untouched = lambda got: set(got[1]) == {0xAB} and got[2] == 0

    def good():
        got = _index_call(eng, table, 2, len(want), block_off, base)
        assert got[0] == 0 and got[1][:got[2]] == right and set(got[1][got[2]:]) == {0xAB}
    good()
    # an unsorted table: two records swapped (by position, and by contig); offsets that do not ascend
    for a, b in ((3, 4), (0, 40)):
        t = table.copy()
        for name in ('refID', 'pos', 'end', 'bin'):
            t[name][a], t[name][b] = table[name][b], table[name][a]
        got = _index_call(eng, t, 2, len(want), block_off, base)
        assert got[0] == -1 and untouched(got), (a, b)
    t = table.copy()
    t['off'][5] = t['off'][4]
    assert _index_call(eng, t, 2, len(want), block_off, base)[0] == -1
    good()
    # refID out of range; pos below 0; end above 2^29; an offset behind the stream
    for field, at, value in (('refID', 59, 2), ('refID', 0, -2), ('pos', 0, -1), ('end', 59, 2 ** 29 + 1), ('off', 60, len(want))):
        t = table.copy()
        t[field][at] = value
        got = _index_call(eng, t, 2, len(want), block_off, base)
        assert got[0] == -1 and untouched(got), (field, at)
    assert _index_call(eng, table, 1, len(want), block_off, base)[0] == -1
    good()
    # the blocks: a count that does not fit the stream, offsets that descend, an offset of 2^48
    assert _index_call(eng, table, 2, len(want), block_off[:-1], base)[0] == -1
    wrong = block_off.copy()
    wrong[0] = wrong[1] + 1
    assert _index_call(eng, table, 2, len(want), wrong, base)[0] == -1
    assert _index_call(eng, table, 2, len(want), block_off, 2 ** 48 - int(block_off[-1]))[0] == -1
    got = _index_call(eng, table, 2, len(want), block_off, 2 ** 48 - int(block_off[-1]) - 1)
    assert got[0] == 0
    # small output and small scratch
    got = _index_call(eng, table, 2, len(want), block_off, base, out_cap=len(right) - 1)
    assert got[0] == E.E_OUTPUT and int(eng.lib.brx_output_needed(eng.ctx)) == len(right) and untouched(got)
    got = _index_call(eng, table, 2, len(want), block_off, base, scratch=512)
    assert got[0] == E.E_SCRATCH and int(eng.lib.brx_scratch_needed(eng.ctx)) == int(eng.lib.brx_bam_index_scratch(len(table), 2)) and untouched(got)
    good()
    # no records: every contig empty
    got = _index_call(eng, table[:0], 2, 0, np.zeros(1, dtype=np.uint64), base)
    assert got[0] == 0 and got[1][:got[2]] == b'BAI\1' + struct.pack('<iiiiiQ', 2, 0, 0, 0, 0, 0)


# ---- from simulated batches, and whole files ------------------------------------------------------------------------------------------------
def check_batches(make_engine, n_full, n_err, n_low=1):
    """The records brx_emit_bam writes for a batch, sorted: the small configurations of test_truth_bam (full identity, errorful, low
    identity), with tags and cs / eqx once and with a small max_cigar_ops once (reflen from the placeholder of a long CIGAR)."""
    import helpers as H
    import test_truth_bam as TB
    import test_truth_paf as T
    import test_truth_sam as TS
    from badread_amd import engine as E
    pref, _ = TS.small()
    n_ref, max_pos = len(pref.names), max(int(x) for x in pref.lengths)
    runs = ((T.full_identity_params(), 11, 0, n_full, dict()),
            (H.SimParams(frag_mean=400, frag_stdev=300), 5, 0, n_err, dict(tags=E.TAG_MD | E.TAG_SA, fmt=E.FMT_EQX | E.FMT_CS)),
            (H.SimParams(frag_mean=400, frag_stdev=300), 5, 0, n_err, dict(max_cigar_ops=8)),
            (H.SimParams(**TB.LOW_IDENTITY), 3, 4, n_low, dict()))
    seen = dict(unmapped=0, long=0, records=0)
    for params, seed, first, n, kw in runs:
        eng = H.configure(make_engine(), pref, 'nanopore2023', 'nanopore2023', params)
        eng.simulate_batch(seed, first, n)
        data, off = eng.emit_bam_device(n, **kw)
        raw = down(data)
        want = sort_records(raw)
        got, table, n_rec, unmapped = eng.bam_sort(data, off, n_ref, max_pos)
        want_table = table_of(want)
        assert down(got) == want and n_rec == len(want_table) and unmapped == int((want_table['refID'] < 0).sum())
        assert np.array_equal(np.frombuffer(down(table), dtype=E.BAM_REC_DTYPE), want_table)
        decoded = BC.records_of_bam(want)
        # what the table says of a record is what the decoded record says: end from the real CIGAR, also where it sits in a CG tag
        for r, t in zip(decoded, want_table):
            ops = r['cigar']
            cg = [x for x in r['tags'] if x[0] == 'CG']
            if cg:
                ops = [(w >> 4, w & 15) for w in cg[0][2]]
                seen['long'] += 1
            if r['rid'] >= 0:
                assert int(t['end']) == r['pos'] + (sum(n_ for n_, op in ops if op in REF_OPS) or 1) and BC.reg2bin(r['pos'], int(t['end'])) == r['bin']
        seen['unmapped'] += unmapped
        seen['records'] += n_rec
    print('bam_sorted_batches', seen)
    assert seen['long'] >= 1 and seen['records'] > n_full + n_err


def check_file_pair(blob, bai, pref, unsorted_records=None):
    """What holds of a PATH / PATH.bai pair: the header says SO:coordinate, the EOF block once and at the end, the records sorted -- the
    stable sort of `unsorted_records` where given --, the index the restatement from the file itself, the queries answered."""
    from badread_amd import output as O
    f = File(blob)
    assert blob.endswith(O.BGZF_EOF) and blob.count(O.BGZF_EOF) == 1
    assert f.text.startswith(b'@HD\tVN:1.6\tSO:coordinate\n@SQ') and b'GO:' not in f.text.split(b'\n')[0]
    assert f.stream.startswith(O.bam_header(pref, text=f.text))
    assert f.raw == sort_records(f.raw)
    if unsorted_records is not None:
        assert f.raw == sort_records(unsorted_records)
    assert bai == bai_of(blob)
    check_queries(bai, blob, [int(x) for x in pref.lengths])
    return f
