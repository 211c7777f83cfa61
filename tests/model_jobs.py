"""
TEST INFRASTRUCTURE: seeded synthetic jobs for the model builders (badread_amd/model_builder.py, csrc/brx_model.h).

job(kind) -> (refs, reads, alignments): {contig: sequence}, {read name: (bases, qualities)} and a list of
badread_amd.alignment.Alignment built straight from PAF lines, so no file is involved and the loader's filters (more than 100
bases, above 80 %) do not apply: alignments of one base exist here.  What the reference's loops need is kept: every CIGAR begins
and ends on M, and no quality character is 0x20 (the reference's gap character for qualities).

  edges      reference spans of 1..33, 255, 256, 257, 511, 512, 600 bases with alignment starts on columns = 0, 1 and 255 (mod 256),
             both strands; insertions that make read k-mers of exactly 21 and 22 bases for k = 2, 3, 7, 8 (the last length a key
             holds and the first that spills); deletions around every max_del under test, 16 and 30; an insertion / deletion right
             behind the first M base and right before the last; N and IUPAC letters in reads and reference; qualities '!', '~',
             0x7F, 0xA0, 0xA1 and 0x05; some alignments twice, so that a spilled key is met by two alignments
  hot        reference A...A, 64 perfect reads of 256 bases, 256M, quality 'I': one key per window size
  two_keys   the same with reads ACAC...: closed forms with two keys per qscore size
  mixed      alignments of 20 to 600 bases at 5 to 15 % edits

write_files(folder, job) stores a job as ref.fasta / reads.fastq / aln.paf (tools/make_golden.py: edges(files=True), the form of
`edges` that passes the loader and holds ASCII only).
"""
import os

import numpy as np

from badread_amd.alignment import Alignment
from badread_amd.misc import reverse_complement

ERROR_KS = (2, 3, 7, 8)
MAX_DELS = (1, 2, 6, 15)
_ODD_QUALS = '!~\x7f\x05\xa0\xa1'
_ODD_QUALS_ASCII = '!~\x7f\x05'


class _Builder(object):

    def __init__(self, seed, odd_quals=_ODD_QUALS):
        self.rng = np.random.default_rng(seed)
        self.ref, self.ref_len = [], 0
        self.reads, self.lines, self.cols = {}, [], 0
        self.odd_quals = odd_quals

    def dna(self, n, letters='ACGT'):
        return ''.join(np.array(list(letters))[self.rng.integers(0, len(letters), n)]) if n else ''

    def quals(self, n):
        q = self.rng.integers(34, 126, n)
        odd = np.flatnonzero(self.rng.random(n) < 0.06)
        q[odd] = [ord(self.odd_quals[i]) for i in self.rng.integers(0, len(self.odd_quals), len(odd))]
        return ''.join(map(chr, q.tolist()))

    def add(self, target, parts, strand='+', sub=0.0, letters='ACGT', quals=None, clip=True, copies=1):
        """One alignment of a new read against `target` (given in the read's orientation) along `parts`; M columns are
        substituted at rate `sub` with one of `letters`, inserted bases are drawn from `letters`."""
        assert parts[0][1] == 'M' and parts[-1][1] == 'M' and sum(n for n, t in parts if t != 'I') == len(target)
        read, tp, matches = [], 0, 0
        for n, t in parts:
            if t == 'M':
                piece = list(target[tp:tp + n])
                for i in np.flatnonzero(self.rng.random(n) < sub).tolist():
                    piece[i] = letters[int(self.rng.integers(0, len(letters)))]
                matches += sum(a == b for a, b in zip(piece, target[tp:tp + n]))
                read.append(''.join(piece))
            elif t == 'I':
                read.append(self.dna(n, letters))
            if t != 'I':
                tp += n
        read = ''.join(read)
        c5, c3 = (int(x) for x in self.rng.integers(0, 4, 2)) if clip else (0, 0)
        seq = self.dna(c5) + read + self.dna(c3)
        qual = quals * len(seq) if quals else self.quals(len(seq))
        fwd = target if strand == '+' else reverse_complement(target)
        start = self.ref_len
        self.ref.append(fwd)
        self.ref_len += len(fwd)
        columns = sum(n for n, _ in parts)
        cigar = ''.join(f'{n}{t}' for n, t in (parts if strand == '+' else parts[::-1]))
        for _ in range(copies):
            name = f'r{len(self.reads)}'
            self.reads[name] = (seq, qual)
            self.lines.append('\t'.join([name, str(len(seq)), str(c5), str(c5 + len(read)), strand, 'ctg', '0', str(start),
                                         str(start + len(fwd)), str(matches), str(columns), '60', 'AS:i:0', f'cg:Z:{cigar}']))
            self.cols += columns

    def pad_to(self, residue):
        """A filler alignment (substitutions only) that puts the next alignment's first column on `residue` (mod 256)."""
        n = (residue - self.cols) % 256
        if n:
            self.add(self.dna(n), [(n, 'M')], '+-'[n & 1], sub=0.1)

    def job(self):
        ref = ''.join(self.ref)
        lines = [line.replace('\tctg\t0\t', f'\tctg\t{len(ref)}\t') for line in self.lines]
        return {'ctg': ref}, self.reads, [Alignment(line) for line in lines], lines


def edges(files=False):
    """files=True: the form that passes load_alignments and a text file: every alignment longer than 100 columns and above 80 %,
    no quality character above 0x7F."""
    b = _Builder(2024, _ODD_QUALS_ASCII if files else _ODD_QUALS)
    flank = 100 if files else 20
    spans = [1, 2, 3, 4, 5, 6, 7, 8, 9, 30, 255, 256, 257, 511, 512, 600]
    for span in (s for s in spans if not files or s > 100):
        for residue in (0, 1, 255):
            for strand in '+-':
                if not files:
                    b.pad_to(residue)
                b.add(b.dna(span), [(span, 'M')], strand, sub=0.08)
    if not files:
        for span in range(10, 34):                       # around every qscore window size up to 31 (+ 2)
            b.add(b.dna(span), [(span, 'M')], '+-'[span & 1], sub=0.05)
    ins = sorted({1, 2, 3, 40} | {21 - k for k in ERROR_KS} | {22 - k for k in ERROR_KS})
    for i, n in enumerate(ins):                          # exact flanks: the windows over the insertion count for the error model
        for strand in '+-':
            b.add(b.dna(2 * flank), [(flank, 'M'), (n, 'I'), (flank, 'M')], strand, copies=2)
    dels = sorted({1, 16, 30} | {d + x for d in MAX_DELS for x in (-1, 0, 1) if d + x > 0})
    for n in dels:
        for strand in '+-':
            b.add(b.dna(2 * flank + n), [(flank, 'M'), (n, 'D'), (flank, 'M')], strand, sub=0.03)
    # a deletion inside a homopolymer: windows whose read k-mer is a single base, equal at both ends (k = 2)
    b.add('ACGT' * (flank // 4) + 'AAAA' + 'CCCC' + 'ACGT' * (flank // 4), [(flank + 1, 'M'), (1, 'D'), (2, 'M'), (1, 'M'), (2, 'D'), (1 + flank, 'M')], '+')
    tail = 2 * flank
    for strand in '+-':
        b.add(b.dna(21 + tail), [(1, 'M'), (3, 'I'), (20 + tail, 'M')], strand)           # right behind the first M base
        b.add(b.dna(21 + tail), [(20 + tail, 'M'), (3, 'I'), (1, 'M')], strand)           # right before the last
        b.add(b.dna(23 + tail), [(1, 'M'), (2, 'D'), (20 + tail, 'M')], strand)
        b.add(b.dna(23 + tail), [(20 + tail, 'M'), (2, 'D'), (1, 'M')], strand)
        b.add(b.dna(12 + tail), [(tail // 2, 'M'), (1, 'I'), (1, 'M'), (1, 'D'), (1, 'M'), (2, 'I'), (2, 'M'), (3, 'D'), (1, 'M'), (12, 'I'),
                                 (1, 'M'), (1, 'D'), (1, 'M'), (tail // 2, 'M')], strand, sub=0.05)
        # N and IUPAC letters on both sides
        t = b.dna(40 + tail, 'ACGTACGTACGTN')
        t = t[:10] + 'NNNRYKM' + t[17:]
        b.add(t, [(15 + tail // 2, 'M'), (2, 'I'), (10, 'M'), (4, 'D'), (11 + tail // 2, 'M')], strand, sub=0.06, letters='ACGTNR')
    return b.job()


def homopolymer(alternate):
    """hot (alternate=False) and two_keys (True): 64 reads of 256 bases, 256M on an all-A reference, every quality 'I'."""
    b = _Builder(1)
    for _ in range(64):
        b.ref.append('A' * 256)
        b.ref_len += 256
    read = 'AC' * 128 if alternate else 'A' * 256
    for r in range(64):
        b.reads[f'r{r}'] = (read, 'I' * 256)
        b.lines.append('\t'.join([f'r{r}', '256', '0', '256', '+', 'ctg', '0', str(256 * r), str(256 * r + 256),
                                  '128' if alternate else '256', '256', '60', 'AS:i:0', 'cg:Z:256M']))
    return b.job()


def mixed(n_align=400):
    b = _Builder(77)
    ins_len = [1, 1, 1, 1, 2, 2, 3, 5, 12, 25, 40]
    del_len = [1, 1, 1, 1, 2, 2, 3, 5, 7, 16, 30]
    for i in range(n_align):
        length = 20 + int(580 * b.rng.random() ** 2.2)
        rate = float(b.rng.uniform(0.05, 0.15))
        parts = [[1, 'M']]
        left = length - 2                                # reference bases between the first and the last, both M
        while left > 0:
            u = b.rng.random()
            if u < rate / 4:
                n, t = int(b.rng.choice(ins_len)), 'I'
            elif u < rate / 2:
                n, t = min(int(b.rng.choice(del_len)), left), 'D'
            else:
                n, t = 1, 'M'
            if parts[-1][1] == t:
                parts[-1][0] += n
            else:
                parts.append([n, t])
            left -= n if t != 'I' else 0
        if parts[-1][1] == 'M':
            parts[-1][0] += 1
        else:
            parts.append([1, 'M'])
        parts = [(n, t) for n, t in parts]
        letters = 'ACGTN' if i % 9 == 0 else 'ACGT'
        b.add(b.dna(sum(n for n, t in parts if t != 'I'), letters * 3 + 'ACGT'), parts, '+-'[int(b.rng.integers(0, 2))],
              sub=rate / 2, letters=letters)
    return b.job()


_JOBS = {}


def job(kind, **kw):
    """(refs, reads, alignments) of a named job, made once and shared (nothing changes them)."""
    key = (kind, tuple(sorted(kw.items())))
    if key not in _JOBS:
        made = {'edges': edges, 'hot': lambda: homopolymer(False), 'two_keys': lambda: homopolymer(True), 'mixed': mixed}[kind](**kw)
        _JOBS[key] = made[:3]
    return _JOBS[key]


def write_files(folder, made):
    refs, reads, _, lines = made
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, 'ref.fasta'), 'w') as f:
        for name, seq in refs.items():
            f.write(f'>{name}\n')
            for i in range(0, len(seq), 80):
                f.write(seq[i:i + 80] + '\n')
    with open(os.path.join(folder, 'reads.fastq'), 'w', encoding='ascii', newline='\n') as f:
        for name, (seq, qual) in reads.items():
            f.write(f'@{name}\n{seq}\n+\n{qual}\n')
    with open(os.path.join(folder, 'aln.paf'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
