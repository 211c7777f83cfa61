"""
PAF alignments for the model builders: the reference's `Alignment` / `load_alignments`
(/root/reference/badread/alignment.py:24-98) -- same fields, same filters (best alignment per read by AS:i, more than
100 aligned bases, identity above 80 %), same messages and exits.  CIGAR parts are kept as (length, letter) pairs,
reversed for '-' strand alignments (alignment.py:61-64).
"""
import re
import sys

from .misc import get_open_func

_PART = re.compile(r'(\d+)(\w)')


class Alignment(object):

    def __init__(self, paf_line):
        fields = paf_line.strip().split('\t')
        if len(fields) < 11:
            sys.exit('Error: alignment file does not seem to be in PAF format')
        self.read_name = fields[0]
        self.read_start, self.read_end = int(fields[2]), int(fields[3])
        self.strand = fields[4]
        self.ref_name = fields[5]
        self.ref_start, self.ref_end = int(fields[7]), int(fields[8])
        self.matching_bases, self.num_bases = int(fields[9]), int(fields[10])
        self.percent_identity = 100.0 * self.matching_bases / self.num_bases
        self.cigar = self.alignment_score = None
        for field in fields:
            if field.startswith('cg:Z:'):
                self.cigar = field[5:]
            if field.startswith('AS:i:'):
                self.alignment_score = int(field[5:])
        if self.cigar is None:
            sys.exit('Error: no CIGAR string found')
        if self.alignment_score is None:
            sys.exit('Error: no alignment score')
        self.cigar_parts = [(int(n), letter) for n, letter in _PART.findall(self.cigar)]
        self.max_indel = max([n for n, letter in self.cigar_parts if letter in 'ID'], default=0)
        if self.strand == '-':
            self.cigar_parts = self.cigar_parts[::-1]

    def __repr__(self):
        return (f'{self.read_name}:{self.read_start}-{self.read_end}({self.strand}),'
                f'{self.ref_name}:{self.ref_start}-{self.ref_end}({self.percent_identity:.3f}%)')


def _paf_records(filename, limit):
    """Alignment objects of the first `limit` PAF lines (all of them when limit is None)."""
    with get_open_func(filename)(filename, 'rt') as paf:
        for n, line in enumerate(paf):
            if limit is not None and limit > 0 and n >= limit:
                return
            yield Alignment(line)


def load_alignments(filename, max_alignments=None, output=sys.stderr, dot_interval=1000):
    """One alignment per read -- its highest AS:i, the LAST of equals (the reference sorts a read's alignments by score and
    takes the final one, alignment.py:89) -- in order of the reads' first appearance, filtered like alignment.py:90.  The PAF is
    streamed: a read keeps one candidate at a time instead of the list of all its alignments."""
    def progress(count):
        if count % dot_interval == 0:
            print('.', end='', file=output, flush=True)

    print('Loading alignments', end='', file=output, flush=True)
    candidate = {}                                        # read name -> best so far; dicts keep first-insertion order
    for seen, a in enumerate(_paf_records(filename, max_alignments), 1):
        held = candidate.get(a.read_name)
        if held is None or a.alignment_score >= held.alignment_score:
            candidate[a.read_name] = a
        progress(seen)
    print('', file=output, flush=True)
    print('Choosing best alignment per read', end='', file=output, flush=True)
    kept = []
    for a in candidate.values():
        if a.num_bases <= 100 or a.percent_identity <= 80.0:
            continue
        kept.append(a)
        progress(len(kept))
    print('', file=output, flush=True)
    return kept


# ---- --gpu-loader: the same list, the PAF parsed by brx_paf_scan (include/brx.h; README: The device loader) -----------------------------
NO_D = 0xFFFFFFFFFFFFFFFF                                 # first_d / last_d of a CIGAR without a D part


class DeviceAlignment(object):
    """An alignment whose fields came from a scan record: the attributes and the repr of Alignment, the CIGAR text cut from the file's
    bytes and its parts parsed only when somebody asks (the spill paths of the model builders)."""
    __slots__ = ('read_name', 'read_start', 'read_end', 'strand', 'ref_name', 'ref_start', 'ref_end', 'matching_bases', 'num_bases',
                 'percent_identity', 'alignment_score', 'max_indel', '_data', '_span', '_parts')

    @property
    def cigar(self):
        return self._data[self._span[0]:self._span[1]].decode('ascii')

    @property
    def cigar_parts(self):
        if self._parts is None:
            parts = [(int(n), letter) for n, letter in _PART.findall(self.cigar)]
            self._parts = parts[::-1] if self.strand == '-' else parts
        return self._parts

    __repr__ = Alignment.__repr__


class DeviceAlignments(list):
    """What load_alignments_device returns: the alignments, and beside them what model_builder.Job.packed ships.  rec: one record per
    alignment (REC_DTYPE; cigar_off is absolute in `text`); text: the PAF's bytes on the engine's device, with the canonical CIGARs of
    the kept irregular lines behind them."""
    REC_DTYPE = [('cigar_off', '<u8'), ('cigar_len', '<u4'), ('n_parts', '<u4'), ('sum_m', '<u8'), ('sum_i', '<u8'), ('sum_d', '<u8'),
                 ('first_d', '<u8'), ('last_d', '<u8'), ('reversed', '<u4')]
    rec = text = engine = None


def _out_of_memory(engine):
    return getattr(engine.torch, 'OutOfMemoryError', None) or engine.torch.cuda.OutOfMemoryError


def _does_not_fit(engine, n_bytes):
    need = n_bytes + engine.lib.brx_paf_scan_scratch(n_bytes) + 144 * (n_bytes // 256 + 64)
    sys.exit(f'Error: --gpu-loader: the alignment file needs {need / 1e9:.1f} GB on the device')


def load_alignments_device(filename, engine, max_alignments=None, output=sys.stderr, dot_interval=1000):
    """load_alignments with the per-part work on the device: the same alignments in the same order, the same text on `output`, the
    same exits.  The host touches a line once (its name, its score) and parses only the lines the device flags as irregular -- in
    file order and before anything else, so that the first bad line of the file ends the command as it does in load_alignments."""
    import numpy as np
    from .engine import PAF_IRREGULAR
    with get_open_func(filename)(filename, 'rb') as paf:
        data = paf.read()
    if b'\r' in data or not data.isascii():               # universal newlines, decoding: the host loader's business
        return load_alignments(filename, max_alignments, output=output, dot_interval=dot_interval)
    print('Loading alignments', end='', file=output, flush=True)
    limit = max_alignments if max_alignments is not None and max_alignments > 0 else 0
    try:
        text = engine._upload(np.frombuffer(data, dtype=np.uint8))[1][:len(data)]          # an empty file: no byte, no line
        recs = engine.paf_scan(text, limit)
    except _out_of_memory(engine):
        _does_not_fit(engine, len(data))
    n = len(recs)
    offs, lens = recs['line_off'].tolist(), recs['line_len'].tolist()
    dots = 0
    parsed = {}                                           # line -> Alignment, for the irregular ones
    for i in np.flatnonzero(recs['flags'] & PAF_IRREGULAR).tolist():
        owed = i // dot_interval                          # the dots of the lines in front of this one, should it end the command
        print('.' * (owed - dots), end='', file=output, flush=True)
        dots = owed
        parsed[i] = Alignment(data[offs[i]:offs[i] + lens[i]].decode('ascii') + '\n')
    print('.' * (n // dot_interval - dots), end='', file=output, flush=True)
    print('', file=output, flush=True)
    print('Choosing best alignment per read', end='', file=output, flush=True)
    names = [data[o:o + q] for o, q in zip(offs, recs['qname_len'].tolist())]
    scores = recs['as'].tolist()
    for i, a in parsed.items():
        names[i], scores[i] = a.read_name.encode('ascii'), a.alignment_score
    candidate = {}                                        # read name -> line of its best so far; dicts keep first-insertion order
    for i, (name, score) in enumerate(zip(names, scores)):
        held = candidate.get(name)
        if held is None or score >= scores[held]:
            candidate[name] = i
    ints = recs['ints'].tolist()
    kept = DeviceAlignments()
    lines = []
    for i in candidate.values():
        a = parsed.get(i)
        matching, bases = (a.matching_bases, a.num_bases) if a is not None else ints[i][4:6]
        if bases <= 100 or 100.0 * matching / bases <= 80.0:
            continue
        lines.append(i)
    print('.' * (len(lines) // dot_interval), end='', file=output, flush=True)
    print('', file=output, flush=True)
    rec = np.zeros(len(lines), dtype=DeviceAlignments.REC_DTYPE)
    at = np.array(lines, dtype=np.int64)
    for field in ('cigar_len', 'n_parts', 'sum_m', 'sum_i', 'sum_d', 'first_d', 'last_d'):
        rec[field] = recs[field][at]
    rec['cigar_off'] = recs['line_off'][at] + recs['cigar_off'][at]
    rec['reversed'] = recs['strand'][at] == ord('-')
    tname = list(zip((recs['line_off'] + recs['tname_off'])[at].tolist(), recs['tname_len'][at].tolist()))
    strands, max_indels = recs['strand'][at].tolist(), recs['max_indel'][at].tolist()
    side = []                                             # the canonical CIGARs of the kept irregular lines
    side_at = len(data)
    for k, i in enumerate(lines):
        a = parsed.get(i)
        d = DeviceAlignment()
        if a is None:
            v = ints[i]
            d.read_name, d.strand = names[i].decode('ascii'), chr(strands[k])
            d.ref_name = data[tname[k][0]:tname[k][0] + tname[k][1]].decode('ascii')
            d.read_start, d.read_end, d.ref_start, d.ref_end, d.matching_bases, d.num_bases = v
            d.percent_identity = 100.0 * d.matching_bases / d.num_bases
            d.alignment_score, d.max_indel = scores[i], max_indels[k]
            d._data, d._span, d._parts = data, (int(rec['cigar_off'][k]), int(rec['cigar_off'][k]) + int(rec['cigar_len'][k])), None
        else:
            for field in ('read_name', 'read_start', 'read_end', 'strand', 'ref_name', 'ref_start', 'ref_end', 'matching_bases',
                          'num_bases', 'percent_identity', 'alignment_score', 'max_indel'):
                setattr(d, field, getattr(a, field))
            d._data, d._span, d._parts = a.cigar.encode('ascii'), (0, len(a.cigar)), a.cigar_parts
            parts = [(n, t) for n, t in (a.cigar_parts[::-1] if a.strand == '-' else a.cigar_parts) if t in ('M', 'I', 'D')]
            if any(n >= 1 << 32 for n, _ in parts):
                sys.exit(f'Error: the CIGAR of {a!r} has a part of 2^32 or more bases')
            canonical = ''.join(f'{n}{t}' for n, t in parts).encode('ascii')
            before_d = [sum(m for m, u in parts[:j] if u != 'D') for j, (_, t) in enumerate(parts) if t == 'D']
            rec[k] = (side_at, len(canonical), len(parts), sum(n for n, t in parts if t == 'M'), sum(n for n, t in parts if t == 'I'),
                      sum(n for n, t in parts if t == 'D'), before_d[0] if before_d else NO_D, before_d[-1] if before_d else NO_D,
                      a.strand == '-')
            side.append(canonical)
            side_at += len(canonical)
        kept.append(d)
    if side:
        try:
            text = engine.torch.cat([text[:len(data)], engine._upload(np.frombuffer(b''.join(side), dtype=np.uint8))[1][:side_at - len(data)]])
        except _out_of_memory(engine):
            _does_not_fit(engine, len(data))
    kept.rec, kept.text, kept.engine = rec, text, engine
    return kept
