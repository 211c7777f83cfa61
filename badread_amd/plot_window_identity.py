"""
`badread plot` on the GPU: the identity (and, with --qual, the mean quality) of every window of W read bases of every read's best
alignment -- the reference's plot_window_identity (/root/reference/badread/plot_window_identity.py:27-70 over align_sequences,
alignment.py:103-132) with the per-base and per-window Python loops replaced by brx_window_means (include/brx.h; kernels in
csrc/brx_window.h).

Host side, as the reference: load_fastq, load_fasta, load_alignments (best alignment per read, > 100 bases, > 80 %), in that order
and with their "Loading ..." lines on `output` (stdout, as the reference has it), one repr(alignment) line per alignment.  What
goes to the device is model_builder.Job, in chunks of at most PLOT_CHUNK_BASES read bases.  What comes back is integers: per
alignment the number of windows and the smallest, largest and total window sum, and the sums themselves only where a plot needs them.
The doubles are made from those here with the reference's own expressions, so they are bit-equal to its values:

    n = max(L - W, 0) windows (not L - W + 1: the reference's loop leaves the last one out)
    position[i] = read_start + i + W // 2     identity[i] = 100.0 * (1.0 - S[i] / W)     quality[i] = Q[i] / W

Additive: --summary PATH (one TSV line per alignment, no window values leave the device), --save DIR (one PNG per alignment) and
--max_alignments N.  Drawing needs matplotlib, which is imported only where a plot is drawn.  --gpu-loader: the PAF parsed and every
chunk packed on the device (alignment.load_alignments_device, model_builder.Job.packed), the same output.  --gpu-reads on top of it: the
FASTQ parsed on the device too and the read slices cut out of it there (reads.load_fastq_device).
"""
import contextlib
import itertools
import os
import pathlib
import sys

import numpy as np

from .alignment import NO_D, DeviceAlignments
from .model_builder import Job, _default_engine, check_alignment_matches_read_and_refs, clipped, load_inputs
from .reads import read_length as read_length_of

PLOT_CHUNK_BASES = 1 << 26                 # read bases per device call: 20 bytes of scratch each, 28 with --qual
SUMMARY_COLUMNS = ('read_name', 'read_length', 'read_start', 'read_end', 'strand', 'ref_name', 'ref_start', 'ref_end',
                   'alignment_identity', 'windows', 'min_identity', 'min_position', 'max_identity', 'mean_identity')
SUMMARY_QUAL_COLUMNS = ('min_quality', 'max_quality', 'mean_quality')


def get_window_means(errors_per_read_pos, window_size, read_start, convert_to_identity=True):
    """The reference's host function (plot_window_identity.py:54-70): (positions, means) of the len - window_size windows of a list
    of integers, the means as identities (100 * (1 - sum / size)) or as they are."""
    prefix = list(itertools.accumulate(errors_per_read_pos, initial=0))
    positions, means = [], []
    for i in range(len(errors_per_read_pos) - window_size):
        mean = (prefix[i + window_size] - prefix[i]) / window_size
        means.append(100.0 * (1.0 - mean) if convert_to_identity else mean)
        positions.append(read_start + i + window_size // 2)
    return positions, means


def identities_of(err_sum, window):
    """float64 identities of window sums: the reference's 100.0 * (1.0 - S / W), every operation correctly rounded as in Python."""
    return 100.0 * (1.0 - np.asarray(err_sum).astype(np.float64) / np.float64(window))


def qualities_of(qual_sum, window):
    return np.asarray(qual_sum).astype(np.float64) / np.float64(window)


def _check_alignment(a, reads, refs, qual):
    """What must hold before an alignment is shipped; returns the length of its read slice."""
    check_alignment_matches_read_and_refs(a, reads, refs)
    length = len(reads[a.read_name][0][a.read_start:a.read_end])
    rp = 0
    for n, t in a.cigar_parts:
        if t == 'D' and rp >= length:         # the reference: IndexError at errors_per_read_pos[read_pos]
            sys.exit(f'Error: the CIGAR of {a!r} ends in a deletion with no read base after it')
        if t in 'MI':
            rp += n
    if sum(n for n, t in a.cigar_parts if t in 'MID') >= 1 << 31:
        sys.exit(f'Error: the CIGAR of {a!r} has 2^31 or more columns')
    if qual and 223 * length >= 1 << 31:
        sys.exit(f'Error: the read slice of {a!r} is too long for --qual (32-bit quality sums)')
    return length


def _check_packed(a, rec, reads, refs, qual):
    """_check_alignment from the scan record of a (--gpu-loader): the same exits in the same order.  A D part with no read base behind
    it: the D with the most read bases in front of it is the last one in file order for '+' and, the list being read backwards, the
    first one for '-'."""
    check_alignment_matches_read_and_refs(a, reads, refs)
    length = len(clipped(a.read_start, a.read_end, read_length_of(reads, a.read_name)))
    first_d, last_d, used_read = int(rec['first_d']), int(rec['last_d']), int(rec['sum_m']) + int(rec['sum_i'])
    if first_d != NO_D and (used_read - first_d >= length if a.strand == '-' else last_d >= length):
        sys.exit(f'Error: the CIGAR of {a!r} ends in a deletion with no read base after it')
    if used_read + int(rec['sum_d']) >= 1 << 31:
        sys.exit(f'Error: the CIGAR of {a!r} has 2^31 or more columns')
    if qual and 223 * length >= 1 << 31:
        sys.exit(f'Error: the read slice of {a!r} is too long for --qual (32-bit quality sums)')
    return length


def check_alignments(alignments, reads, refs, qual):
    """The lengths of the read slices of all alignments, every alignment checked on the way."""
    if isinstance(alignments, DeviceAlignments):
        return [_check_packed(a, rec, reads, refs, qual) for a, rec in zip(alignments, alignments.rec)]
    return [_check_alignment(a, reads, refs, qual) for a in alignments]


def chunks(lengths, limit):
    """(first, end) index ranges: as many consecutive alignments as hold at most `limit` read bases, at least one."""
    first, held = 0, 0
    for i, length in enumerate(lengths):
        if i > first and held + length > limit:
            yield first, i
            first, held = i, 0
        held += length
    if first < len(lengths):
        yield first, len(lengths)


def window_means(engine, refs, reads, alignments, window, qual, values=False, lengths=None):
    """brx_window_means over all alignments, chunk by chunk: yields (stat, err_sum, qual_sum) per alignment, stat a record of
    engine.WINDOW_STAT_DTYPE, the sums arrays of stat['n'] integers or None (values=False; qual_sum also without qual).  Every
    alignment is checked before the first chunk is shipped."""
    if lengths is None:
        lengths = check_alignments(alignments, reads, refs, qual)
    device = isinstance(alignments, DeviceAlignments)
    for first, end in chunks(lengths, PLOT_CHUNK_BASES):
        job = Job.packed(engine, refs, reads, alignments, first, end) if device else Job(refs, reads, alignments[first:end])
        stats, err_sum, qual_sum = engine.window_means(job, window, qual, values)
        off = np.concatenate(([0], np.cumsum(stats['n'].astype(np.int64))))
        for k in range(end - first):
            lo, hi = int(off[k]), int(off[k + 1])
            yield stats[k], err_sum[lo:hi] if err_sum is not None else None, qual_sum[lo:hi] if qual_sum is not None else None


def summary_line(a, read_length, stat, window, qual):
    """One line of --summary (without the newline)."""
    n = int(stat['n'])
    fields = [a.read_name, str(read_length), str(a.read_start), str(a.read_end), a.strand, a.ref_name, str(a.ref_start), str(a.ref_end),
              '%.3f' % a.percent_identity, str(n)]
    if n == 0:
        return '\t'.join(fields + ['NA'] * (4 + (3 if qual else 0)))
    fields += ['%.3f' % (100.0 * (1.0 - int(stat['err_max']) / window)), str(a.read_start + int(stat['err_argmax']) + window // 2),
               '%.3f' % (100.0 * (1.0 - int(stat['err_min']) / window)), '%.3f' % (100.0 * (1.0 - int(stat['err_total']) / (window * n)))]
    if qual:
        fields += ['%.3f' % (int(stat['qual_min']) / window), '%.3f' % (int(stat['qual_max']) / window),
                   '%.3f' % (int(stat['qual_total']) / (window * n))]
    return '\t'.join(fields)


def _pyplot(save):
    try:
        import matplotlib
        if save:
            matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        sys.exit('Error: plot needs matplotlib to display or save plots (use --no_plot)')
    return plt


def plot_one_alignment(plt, positions, identities, qualities, window, a, read_length, save_path=None):
    """The identity of every window against its centre's position in the read; with qualities, their means on a second axis."""
    fig, ax = plt.subplots(1, 1, figsize=(12, 3))
    ax.plot(positions, identities, '-', color='firebrick')
    ax.set_xlabel('read position')
    ax.set_ylabel(f'% identity ({window} bp windows)')
    ax.set_title(f'{a.read_name} ({read_length} bp, {a.percent_identity:.1f}% identity)')
    ax.set_xlim(0, max(read_length, 1))
    ax.set_ylim(min(50.0, float(np.min(identities))) if len(identities) else 50.0, 100.0)
    if qualities is not None:
        ax2 = ax.twinx()
        ax2.plot(positions, qualities, '-', color='navy')
        ax2.set_ylabel('mean qscore')
    fig.tight_layout()
    if save_path is not None:
        fig.savefig(save_path)
    else:
        plt.show()
    plt.close(fig)


def plot_window_identity(args, output=sys.stdout, engine=None, stdout=None):
    stdout = stdout or sys.stdout
    window, qual = args.window, bool(args.qual)
    summary, save = getattr(args, 'summary', None), getattr(args, 'save', None)
    if window < 1:
        sys.exit('Error: --window must be at least 1')
    if summary is not None and not pathlib.Path(summary).resolve().parent.is_dir():
        sys.exit(f'Error: the directory of --summary {summary} does not exist')
    refs, reads, alignments, engine = load_inputs(args, engine, output, ('reads', 'reference', 'alignments'))
    lengths = check_alignments(alignments, reads, refs, qual)
    draw = save is not None or not args.no_plot
    plt = _pyplot(save is not None) if draw else None
    if save is not None:
        os.makedirs(save, exist_ok=True)
    engine = _default_engine(engine)
    with open(summary, 'w') if summary is not None else contextlib.nullcontext() as table:
        if summary is not None:
            table.write('#' + '\t'.join(SUMMARY_COLUMNS + (SUMMARY_QUAL_COLUMNS if qual else ())) + '\n')
        results = window_means(engine, refs, reads, alignments, window, qual, values=draw, lengths=lengths)
        for index, (a, (stat, err_sum, qual_sum)) in enumerate(zip(alignments, results)):
            print(a, file=stdout)
            read_length = read_length_of(reads, a.read_name)
            if summary is not None:
                table.write(summary_line(a, read_length, stat, window, qual) + '\n')
            if draw:
                positions = a.read_start + window // 2 + np.arange(int(stat['n']), dtype=np.int64)
                name = f'{index}_{a.read_name.replace("/", "_")}.png'
                plot_one_alignment(plt, positions, identities_of(err_sum, window), qualities_of(qual_sum, window) if qual else None,
                                   window, a, read_length, os.path.join(save, name) if save is not None else None)
