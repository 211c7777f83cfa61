#!/usr/bin/env python3
"""
Generate tests/golden/plot_windows.json.gz by RUNNING THE UNMODIFIED REFERENCE (/root/reference, Badread 0.4.2): its `plot --no_plot`
on the committed tests/golden/model_builder/{ref.fasta,reads.fastq,aln.paf}.  The reference's modules import edlib (absent here;
oracle/shim/edlib stands in, plot does not call it) and matplotlib (MPLBACKEND=Agg: nothing is drawn with --no_plot).

For every window size W of WINDOWS, without and with --qual, the fixture records
  stdout         what the reference's plot_window_identity prints (the loaders' lines and one line per alignment)
  alignments     per alignment, in the reference's order: n (the number of windows), position[0] (null where n = 0) and the sha256 of
                 the float64 little-endian bytes of the identities and (with --qual) of the qualities, from the reference's own
                 align_sequences + get_window_means, called as plot_window_identity calls them
and, for W = 100 with --qual, the full positions, identities and qualities of three alignments: the first on '+', the first on '-'
and the one with the longest insertion.  Floats are stored as repr() text, which round-trips exactly.

Deterministic: a second run changes no byte.  Run:  python tools/make_plot_golden.py   (needs /root/reference; seconds)
"""
import argparse
import contextlib
import gzip
import hashlib
import io
import json
import os
import struct
import sys

os.environ.setdefault('MPLBACKEND', 'Agg')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = '/root/reference'
for p in (os.path.join(REPO, 'oracle', 'shim'), REFERENCE):
    if p not in sys.path:
        sys.path.insert(0, p)

import badread.alignment as ref_alignment                  # noqa: E402  (the reference)
import badread.misc as ref_misc                            # noqa: E402
import badread.plot_window_identity as ref_plot            # noqa: E402
import badread.qscore_model as ref_qm                      # noqa: E402
import badread.version as ref_version                      # noqa: E402

INPUTS = os.path.join(REPO, 'tests', 'golden', 'model_builder')
OUT = os.path.join(REPO, 'tests', 'golden', 'plot_windows.json.gz')
WINDOWS = (1, 2, 100, 312, 313, 5000)


def digest(values):
    return hashlib.sha256(b''.join(struct.pack('<d', v) for v in values)).hexdigest()


def arguments(window, qual):
    return argparse.Namespace(reference=os.path.join(INPUTS, 'ref.fasta'), reads=os.path.join(INPUTS, 'reads.fastq'),
                              alignment=os.path.join(INPUTS, 'aln.paf'), window=window, qual=qual, no_plot=True)


def stdout_of(window, qual):
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        ref_plot.plot_window_identity(arguments(window, qual), output=text)
    return text.getvalue()


def values_of(reads, refs, a, window):
    """positions, identities, qualities of one alignment: the calls of plot_window_identity.py:34-45"""
    read_seq, read_qual = (x[a.read_start:a.read_end] for x in reads[a.read_name])
    ref_seq = refs[a.ref_name][a.ref_start:a.ref_end]
    if a.strand == '-':
        ref_seq = ref_misc.reverse_complement(ref_seq)
    _, _, _, errors = ref_alignment.align_sequences(read_seq, read_qual, ref_seq, a)
    positions, identities = ref_plot.get_window_means(errors, window, a.read_start, convert_to_identity=True)
    quals = [ref_qm.qscore_char_to_val(q) for q in read_qual]
    _, qualities = ref_plot.get_window_means(quals, window, a.read_start, convert_to_identity=False)
    return positions, identities, qualities


def main():
    null = io.StringIO()
    args = arguments(100, True)
    reads = ref_misc.load_fastq(args.reads, output=null)
    refs = ref_misc.load_fasta(args.reference)[0]
    alignments = ref_alignment.load_alignments(args.alignment, output=null)
    longest_ins = max(range(len(alignments)), key=lambda i: max([int(c[:-1]) for c in alignments[i].cigar_parts if c[-1] == 'I'], default=0))
    full_of = sorted({next(i for i, a in enumerate(alignments) if a.strand == '+'),
                      next(i for i, a in enumerate(alignments) if a.strand == '-'), longest_ins})
    fixture = {'reference': f'rrwick/Badread {ref_version.__version__}', 'generator': 'tools/make_plot_golden.py',
               'inputs': 'tests/golden/model_builder', 'windows': list(WINDOWS), 'names': [repr(a) for a in alignments],
               'cases': [], 'full': []}
    for window in WINDOWS:
        for qual in (False, True):
            rows = []
            for a in alignments:
                positions, identities, qualities = values_of(reads, refs, a, window)
                rows.append({'n': len(identities), 'position0': positions[0] if positions else None, 'identities': digest(identities),
                             'qualities': digest(qualities) if qual else None})
            fixture['cases'].append({'window': window, 'qual': qual, 'stdout': stdout_of(window, qual), 'alignments': rows})
    for i in full_of:
        positions, identities, qualities = values_of(reads, refs, alignments[i], 100)
        fixture['full'].append({'index': i, 'window': 100, 'positions': positions, 'identities': [repr(v) for v in identities],
                                'qualities': [repr(v) for v in qualities]})
    data = json.dumps(fixture, separators=(',', ':'), sort_keys=True).encode()
    with open(OUT, 'wb') as raw, gzip.GzipFile(filename='', mode='wb', fileobj=raw, mtime=0) as f:
        f.write(data)
    print(f'{OUT}: {len(alignments)} alignments, full lists of {full_of}, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
