"""
`badread error_model` and `badread qscore_model` on the GPU: the reference's
make_error_model (/root/reference/badread/error_model.py:31-83) and make_qscore_model (qscore_model.py:78-162) with the
per-alignment Python loops replaced by brx_model_count (include/brx.h; kernels in csrc/brx_model.h).

Host side, as the reference: load_fasta, load_fastq, load_alignments (best alignment per read, > 100 bases, > 80 %),
check_alignment_matches_read_and_refs, the slices and the strand flip of every alignment.  What goes to the device: the
slices as bytes and the CIGAR parts with the prefix sums of their column / read / reference offsets.  What comes back: a
hash table of (key, count, earliest window) and the few windows a 64-bit key cannot hold, which are counted here.  The
text written to stdout is the reference's, byte for byte: alternatives and cigars with equal counts keep the order in
which the reference's loops would first have met them (Python dict order + stable sort), reproduced from the earliest
window recorded per key.

With --gpu-loader (README: The device loader) the PAF is parsed by brx_paf_scan (alignment.load_alignments_device) and the part arrays and
reference slices are written by brx_align_pack (Job.packed); the host then only joins the read slices.  Same text, same exits.
With --gpu-reads on top (README: The device read loader) the FASTQ is parsed by brx_fastq_scan (reads.load_fastq_device) and stays on
the device, and the read slices are cut out of it by brx_reads_pack: no join either.
"""
import collections
import itertools
import re
import sys

import numpy as np

from .alignment import DeviceAlignments, load_alignments, load_alignments_device
from .misc import _COMPLEMENT, float_to_str, load_fasta, load_fastq, only_acgt, reverse_complement
from .reads import DeviceReads, load_fastq_device

_TYPE = {'M': 0, 'I': 1, 'D': 2}
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def check_alignment_matches_read_and_refs(a, reads, refs):
    if a.read_name not in reads:
        sys.exit(f'\nError: could not find read {a.read_name}\nare you sure your read file and alignment file match?')
    if a.ref_name not in refs:
        sys.exit(f'\nError: could not find reference {a.ref_name}\nare you sure your reference file and alignment file match?')


def clipped(start, end, length):
    """The indices x[start:end] takes of a sequence of `length` items: Python's clipping rule without the sequence."""
    return range(*slice(start, end).indices(length))


def cut(a, refs, reads):
    """(read slice, its qualities, reference slice on the read's strand, M / I / D parts) of alignment a: what align_sequences
    (alignment.py:101-132) works on; it ignores every other CIGAR letter."""
    read_seq, read_qual = (x[a.read_start:a.read_end] for x in reads[a.read_name])
    ref_seq = refs[a.ref_name][a.ref_start:a.ref_end]
    if a.strand == '-':
        ref_seq = reverse_complement(ref_seq)
    return read_seq, read_qual, ref_seq, [(n, t) for n, t in a.cigar_parts if t in _TYPE]


class Job(object):
    """The alignments as flat arrays (what brx_model_job points at) + the per-alignment strings for the spilled windows."""

    def __init__(self, refs, reads, alignments):
        seqs, quals, refsl = [], [], []
        ptype, plen, pcol, pread, pref = [], [], [], [], []
        a_part, a_col, a_read = [0], [0], [0]
        col = rpos = fpos = 0
        self.slices = []
        for a in alignments:
            check_alignment_matches_read_and_refs(a, reads, refs)
            read_seq, read_qual, ref_seq, parts = cut(a, refs, reads)
            used_read = sum(n for n, t in parts if t != 'D')
            used_ref = sum(n for n, t in parts if t != 'I')
            if used_read > len(read_seq) or used_ref > len(ref_seq) or len(read_qual) < len(read_seq):
                sys.exit(f'Error: the CIGAR of {a!r} runs past its read or reference range')
            r0, f0 = rpos, fpos
            for n, t in parts:
                ptype.append(_TYPE[t]); plen.append(n); pcol.append(col); pread.append(rpos); pref.append(fpos)
                col += n
                if t != 'D':
                    rpos += n
                if t != 'I':
                    fpos += n
            rpos, fpos = r0 + len(read_seq), f0 + len(ref_seq)
            seqs.append(read_seq); quals.append(read_qual[:len(read_seq)]); refsl.append(ref_seq)
            a_part.append(len(ptype)); a_col.append(col); a_read.append(rpos)
            self.slices.append((read_seq, read_qual, ref_seq, parts))
        enc = lambda parts_: np.frombuffer(''.join(parts_).encode('latin-1') or b'\0', dtype=np.uint8)
        self.seq, self.qual, self.ref = enc(seqs), enc(quals), enc(refsl)
        self.part_type = np.array(ptype or [0], dtype=np.uint8)
        self.part_len = np.array(plen or [0], dtype=np.uint32)
        self.part_col, self.part_read, self.part_ref = (np.array(x or [0], dtype=np.uint64) for x in (pcol, pread, pref))
        self.align_part_off = np.array(a_part, dtype=np.uint64)
        self.align_col_off = np.array(a_col, dtype=np.uint64)
        self.align_read_off = np.array(a_read, dtype=np.uint64)      # where each alignment's read slice begins in seq / qual
        self.n_align, self.n_cols = len(alignments), col

    @classmethod
    def packed(cls, engine, refs, reads, packed, first, end):
        """The same job for packed[first:end] of a DeviceAlignments (--gpu-loader): seq and qual joined here as above, the part arrays
        and ref written on the device by brx_align_pack from the CIGAR text that already lies there -- tensors, which model_count and
        window_means take as they are.  The checks read the scan records (sum_m / sum_i / sum_d) instead of walking parts; slices is
        made per alignment when a spill path asks for one.  With a DeviceReads (--gpu-reads) seq and qual are tensors too: the host
        only says where every slice lies in the FASTQ text (Python's clipping rule on the record's lengths) and brx_reads_pack copies."""
        self = cls.__new__(cls)
        on_device = isinstance(reads, DeviceReads)
        alignments, rec = list.__getitem__(packed, slice(first, end)), packed.rec[first:end]
        reftext, ref_at = _device_reference(engine, refs, packed)
        n = len(alignments)
        seqs, quals = [], []
        read_len, ref_off, ref_len, seq_src, qual_src = (np.zeros(n, dtype=np.uint64) for _ in range(5))
        used_read, used_ref = (rec['sum_m'] + rec['sum_i']).tolist(), (rec['sum_m'] + rec['sum_d']).tolist()
        for k, a in enumerate(alignments):
            check_alignment_matches_read_and_refs(a, reads, refs)
            if on_device:                                   # ranges stand in for the two strings: only their lengths are asked for
                seq_at, seq_n, qual_at, qual_n = reads.spans(a.read_name)
                read_seq, read_qual = clipped(a.read_start, a.read_end, seq_n), clipped(a.read_start, a.read_end, qual_n)
                seq_src[k], qual_src[k] = seq_at + read_seq.start, qual_at + read_qual.start
            else:
                read_seq, read_qual = (x[a.read_start:a.read_end] for x in reads[a.read_name])
            ref_seq = clipped(a.ref_start, a.ref_end, len(refs[a.ref_name]))
            if used_read[k] > len(read_seq) or used_ref[k] > len(ref_seq) or len(read_qual) < len(read_seq):
                sys.exit(f'Error: the CIGAR of {a!r} runs past its read or reference range')
            if not on_device:
                seqs.append(read_seq); quals.append(read_qual[:len(read_seq)])
            read_len[k], ref_off[k], ref_len[k] = len(read_seq), ref_at[a.ref_name] + ref_seq.start, len(ref_seq)
        offsets = lambda x: np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(x, dtype=np.uint64)))
        self.align_part_off = offsets(rec['n_parts'])
        self.align_col_off = offsets(rec['sum_m'] + rec['sum_i'] + rec['sum_d'])
        self.align_read_off = offsets(read_len)
        if on_device:
            self.seq, self.qual = engine.reads_pack(reads.text, seq_src, qual_src, self.align_read_off)
        else:
            enc = lambda parts_: np.frombuffer(''.join(parts_).encode('latin-1') or b'\0', dtype=np.uint8)
            self.seq, self.qual = enc(seqs), enc(quals)
        self.align_ref_off = offsets(ref_len)
        from .engine import PACK_ALIGN_DTYPE
        desc = np.zeros(n, dtype=PACK_ALIGN_DTYPE)
        for field in ('cigar_off', 'cigar_len', 'n_parts', 'sum_m', 'sum_i', 'sum_d', 'reversed'):
            desc[field] = rec[field]
        desc['ref_off'], desc['ref_len'] = ref_off, ref_len
        out = engine.align_pack(packed.text, reftext, _device_complement(engine, packed), desc, self.align_part_off, self.align_col_off,
                                self.align_read_off, self.align_ref_off)
        self.part_type, self.part_len, self.ref = out['part_type'], out['part_len'], out['ref']
        self.part_col, self.part_read, self.part_ref = out['part_col'], out['part_read'], out['part_ref']
        self.n_align, self.n_cols = n, int(self.align_col_off[-1])
        self.slices = _LazySlices(refs, reads, alignments)
        return self

    def gapped(self, a, gap):
        """align_sequences (alignment.py:101-132) for alignment a: gapped read, quality, reference strings."""
        read_seq, read_qual, ref_seq, parts = self.slices[a]
        read, qual, ref = [], [], []
        rp = fp = 0
        for n, t in parts:
            read.append(read_seq[rp:rp + n] if t != 'D' else gap * n)
            qual.append(read_qual[rp:rp + n] if t != 'D' else gap * n)
            ref.append(ref_seq[fp:fp + n] if t != 'I' else gap * n)
            if t != 'D':
                rp += n
            if t != 'I':
                fp += n
        return ''.join(read), ''.join(qual), ''.join(ref)


class _LazySlices(object):
    """Job.slices of a packed job: an entry is made when it is asked for."""

    def __init__(self, refs, reads, alignments):
        self.refs, self.reads, self.alignments = refs, reads, alignments

    def __len__(self):
        return len(self.alignments)

    def __getitem__(self, k):
        return cut(self.alignments[k], self.refs, self.reads)


def _device_reference(engine, refs, packed):
    """(the contigs' text back to back on the device, {contig: where it begins}): uploaded once per command, kept on `packed`."""
    held = getattr(packed, '_reference', None)
    if held is None or held[0] is not refs:
        at, total = {}, 0
        for name, seq in refs.items():
            at[name] = total
            total += len(seq)
        text = np.frombuffer(''.join(refs.values()).encode('latin-1') or b'\0', dtype=np.uint8)
        held = packed._reference = (refs, engine._upload(text)[1], at)
    return held[1], held[2]


def _device_complement(engine, packed):
    """misc._COMPLEMENT as the 256 bytes brx_align_pack reads: N for every byte it does not name (reverse_complement)."""
    held = getattr(packed, '_complement', None)
    if held is None:
        table = np.full(256, ord('N'), dtype=np.uint8)
        for base, other in _COMPLEMENT.items():
            table[ord(base)] = ord(other)
        held = packed._complement = engine._upload(table)[1]
    return held


def _job(engine, refs, reads, alignments):
    if isinstance(alignments, DeviceAlignments):
        return Job.packed(engine, refs, reads, alignments, 0, len(alignments))
    return Job(refs, reads, alignments)


def _default_engine(engine=None):
    """`engine`, or the process's own: the one place where a command opens the device (the driver then prints to stderr)."""
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    return engine


def load_inputs(args, engine, output, order):
    """(refs, reads, alignments, engine) of a command, loaded in `order` ('reference', 'reads', 'alignments' in the command's own
    sequence) with their "Loading ..." lines on `output`.  --gpu-reads / --gpu-loader take the device twins of load_fastq /
    load_alignments, and the engine is made just before the first of them that needs it; without either flag it comes back as it
    came (None: the caller opens the device where it starts to compute, after its own checks and exits)."""
    gpu_loader, gpu_reads = getattr(args, 'gpu_loader', False), getattr(args, 'gpu_reads', False)
    if gpu_reads and not gpu_loader:
        sys.exit('Error: --gpu-reads needs --gpu-loader')
    max_alignments = getattr(args, 'max_alignments', None)
    got = {}
    for what in order:
        if what == 'reference':
            got[what] = load_fasta(args.reference)[0]
        elif what == 'reads' and gpu_reads:
            engine = _default_engine(engine)
            got[what] = load_fastq_device(args.reads, engine, output=output)
        elif what == 'reads':
            got[what] = load_fastq(args.reads, output=output)
        elif gpu_loader:
            engine = _default_engine(engine)
            got[what] = load_alignments_device(args.alignment, engine, max_alignments, output=output)
        else:
            got[what] = load_alignments(args.alignment, max_alignments, output=output)
    return got['reference'], got['reads'], got['alignments'], engine


MODEL_ORDER = ('reference', 'reads', 'alignments')


def _table(engine, kind, job, k, max_del, n_ksizes, first_bits=16):
    """The counted table of a job.  The first table has 2^first_bits slots, raised to four times the keys the job is expected to hold;
    a first_bits below the default is taken as it is, so the growth below is what finds the size."""
    bits = first_bits
    need = max(job.n_cols * (n_ksizes if kind else 1) // 2, 1)
    while first_bits >= 16 and (1 << bits) < 4 * need and bits < 28:
        bits += 1
    while True:
        res = engine.model_count(kind, job, k, max_del, n_ksizes, bits)
        if res is not None:
            return res
        bits += 2                                   # table full: the engine returned None
        if bits > 30:
            sys.exit('Error: model builder hash table does not fit')


def _spilled(spill, shift, strings_of):
    """(word, strings_of(its alignment)) for every distinct spilled word, ascending; the alignment index is the word's top bits, so
    the words of one alignment follow each other and its strings are built once, not once per word."""
    held, strings = -1, None
    for word in sorted(set(spill.tolist())):
        if word >> shift != held:
            held = word >> shift
            strings = strings_of(held)
        yield word, strings


def count_error_model(engine, job, k, first_bits=16):
    """(ref k-mer, read k-mer) -> [count, earliest window (alignment << 32 | start column)]: the device table with the spilled
    windows merged in."""
    keys, counts, first, spill = _table(engine, 0, job, k, 0, 1, first_bits)
    found = {}
    mask_k = (1 << (2 * k)) - 1
    for key, n, rank in zip(keys.tolist(), counts.tolist(), first.tolist()):
        refk = key & mask_k
        length = (key >> (2 * k)) & 31
        bits = key >> (2 * k + 5)
        ref_kmer = ''.join('ACGT'[(refk >> (2 * (k - 1 - i))) & 3] for i in range(k))
        read_kmer = ''.join('ACGT'[(bits >> (2 * i)) & 3] for i in range(length))
        found[(ref_kmer, read_kmer)] = [n, rank]
    for word, (read_g, _, ref_g) in _spilled(spill, 32, lambda a: job.gapped(a, '-')):       # read k-mers of more than 21 bases: counted here
        pair = _error_window(read_g, ref_g, word & 0xFFFFFFFF, k)
        if pair is not None:
            entry = found.setdefault(pair, [0, word])
            entry[0] += 1
            entry[1] = min(entry[1], word)
    return found


def make_error_model(args, output=sys.stderr, dot_interval=1000, engine=None, stdout=None):
    stdout = stdout or sys.stdout
    refs, reads, alignments, engine = load_inputs(args, engine, output, MODEL_ORDER)
    if len(alignments) == 0:
        sys.exit('Error: no usable alignments')
    k = args.k_size
    if not 2 <= k <= 8:
        sys.exit('Error: the GPU error-model builder supports --k_size 2 to 8')
    engine = _default_engine(engine)
    print('Processing alignments', end='', file=output, flush=True)
    found = count_error_model(engine, _job(engine, refs, reads, alignments), k)
    print('.' * (len(alignments) // dot_interval), file=output, flush=True)
    by_kmer = collections.defaultdict(list)
    for (ref_kmer, read_kmer), (n, rank) in found.items():
        by_kmer[ref_kmer].append((rank, read_kmer, n))
    for kmer in (''.join(x) for x in itertools.product('ACGT', repeat=k)):
        alts = sorted(by_kmer.get(kmer, ()))        # first-insertion order of the reference's dictionary
        if not alts:
            continue
        total = sum(n for _, _, n in alts)
        same = sum(n for _, alt, n in alts if alt == kmer)
        print(f'{kmer},{same / total:.6f}', end=';', file=stdout)
        fracs = sorted(((alt, n / total) for _, alt, n in alts if alt != kmer), reverse=True, key=lambda x: x[1])
        for alt, frac in fracs[:args.max_alt]:
            print(f'{alt},{frac:.6f}', end=';', file=stdout)
        print(file=stdout)


def _error_window(read_g, ref_g, start, k):
    """One window of error_model.py:47-62 on the gapped strings: (ref k-mer, read k-mer) or None."""
    end = start
    while len(ref_g[start:end].replace('-', '')) < k:
        end += 1
        if end > len(ref_g):
            return None
    ref_kmer, read_kmer = ref_g[start:end].replace('-', ''), read_g[start:end].replace('-', '')
    if len(read_kmer) > 1 and ref_kmer[0] == read_kmer[0] and ref_kmer[-1] == read_kmer[-1] and \
            only_acgt(ref_kmer) and only_acgt(read_kmer):
        return ref_kmer, read_kmer
    return None


def count_qscore_model(engine, job, k_size, max_del, first_bits=16):
    """cigar -> [earliest window (alignment << 40 | size index << 36 | start column), {q: count}]: the device table with the
    spilled windows merged in."""
    keys, counts, first, spill = _table(engine, 1, job, k_size, max_del, (k_size + 1) // 2, first_bits)
    per_cigar = {}
    for key, n, rank in zip(keys.tolist(), counts.tolist(), first.tolist()):
        q, ki, ops = key & 127, (key >> 7) & 15, key >> 11
        cigar, shift = [], 0
        for i in range(2 * ki + 1):
            if i:
                cigar.append('D' * ((ops >> shift) & 15)); shift += 4
            cigar.append('=XI'[(ops >> shift) & 3]); shift += 2
        entry = per_cigar.setdefault(''.join(cigar), [rank, collections.Counter()])
        entry[0] = min(entry[0], rank)
        entry[1][q] += n
    # windows a key cannot hold (k_mb_qscore names each: alignment, size index, start)
    long_run = re.compile('D{' + str(max_del) + ',}')

    def strings_of(a):                               # gapped read and quality, and the alignment's columns as cigar letters
        read_g, qual_g, ref_g = job.gapped(a, ' ')
        return read_g, qual_g, ''.join('=' if r == f else 'D' if r == ' ' else 'I' if f == ' ' else 'X' for r, f in zip(read_g, ref_g))

    for word, (read_g, qual_g, ops_g) in _spilled(spill, 36, strings_of):
        a, ki, start = word >> 36, (word >> 32) & 15, word & 0xFFFFFFFF
        hit = _qscore_window(read_g, qual_g, ops_g, start, 2 * ki + 1, long_run, 'D' * max_del)
        if hit is None:
            continue
        rank = (a << 40) | (ki << 36) | start
        entry = per_cigar.get(hit[0])
        if entry is None:
            entry = per_cigar[hit[0]] = [rank, collections.Counter()]
        entry[0] = min(entry[0], rank)
        entry[1][hit[1]] += 1
    return per_cigar


def make_qscore_model(args, output=sys.stderr, dot_interval=1000, engine=None, stdout=None):
    stdout = stdout or sys.stdout
    refs, reads, alignments, engine = load_inputs(args, engine, output, MODEL_ORDER)
    if len(alignments) == 0:
        sys.exit('Error: no usable alignments')
    assert args.k_size % 2 == 1
    n_ksizes = (args.k_size + 1) // 2
    if n_ksizes > 16 or args.max_del > 15:
        sys.exit('Error: the GPU qscore-model builder supports --k_size up to 31 and --max_del up to 15')
    engine = _default_engine(engine)
    print('Processing alignments', end='', file=output, flush=True)
    per_cigar = count_qscore_model(engine, _job(engine, refs, reads, alignments), args.k_size, args.max_del)
    print('.' * (len(alignments) // dot_interval), file=output, flush=True)
    overall = collections.Counter()
    for cigar, (_, qs) in per_cigar.items():
        if len(cigar.replace('D', '')) == 1:         # every window of one read base (qscore_model.py:141-142)
            overall.update(qs)
    print_qscore_fractions('overall', overall, 0, stdout)
    ordered = sorted(per_cigar, key=lambda c: per_cigar[c][0])                       # first-insertion order
    ordered = sorted(ordered, reverse=True, key=lambda c: sum(per_cigar[c][1].values()))
    for i, cigar in enumerate(ordered, 1):
        print_qscore_fractions(cigar, per_cigar[cigar][1], args.min_occur, stdout)
        if i >= args.max_output:
            break


def _qscore_window(read_g, qual_g, ops_g, start, k_size, long_run, run_cap):
    """One window of qscore_model.py:104-143 on the gapped strings (ops_g: the columns as = X I D): (cigar, qscore) or None."""
    end = start + k_size
    if end > len(read_g):
        return None
    have = k_size - read_g.count(' ', start, end)
    while have < k_size:
        if end >= len(read_g):
            return None
        have += read_g[end] != ' '
        end += 1
    qual = qual_g[start:end].replace(' ', '')
    return long_run.sub(run_cap, ops_g[start:end]), ord(qual[(k_size - 1) // 2]) - 33


def print_qscore_fractions(cigar, qscores, min_occur, stdout):
    total = sum(qscores.values())
    if total < min_occur:
        return
    print(f'{cigar};{total};', end='', file=stdout)
    for q in sorted(qscores.keys()):
        print(f'{q}:{float_to_str(qscores[q] / total, decimals=6, trim_zeros=True)},', end='', file=stdout)
    print(file=stdout)
