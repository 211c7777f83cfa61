"""
Cost of `badread plot --no_plot --summary` on reads of the project's own simulate: what profiles/plot_windows.md records.

    python tools/plot_windows_cost.py [--quantity 150M] [--ref-bases 2000000] [--repeats 5] [--out plot_windows_cost.json]

A random one-contig reference, `simulate --quantity Q --seed 7 --truth-paf` at the default lengths, then, separately: the three loaders,
the checks and the packing (model_builder.Job) of every chunk, and brx_window_means on every chunk -- one warm-up call, then `--repeats`
calls under brx_set_kernel_timing: the median ms of each kernel group between HIP events (engine.window_last) and of the whole call
(uploads and the copy back included), without and with --qual and with the window values.  Beside every kernel the bytes it must move
and the rate that gives.  Last, the whole command as a child process.
"""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quantity', default='150M')
    ap.add_argument('--ref-bases', type=int, default=2000000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    from badread_amd import plot_window_identity as P
    from badread_amd.alignment import load_alignments
    from badread_amd.engine import default_engine
    from badread_amd.misc import load_fasta, load_fastq
    from badread_amd.model_builder import Job

    work = tempfile.mkdtemp(prefix='plot_cost_')
    ref, fastq, paf = (os.path.join(work, x) for x in ('ref.fasta', 'reads.fastq', 'truth.paf'))
    seq = np.frombuffer(b'ACGT', dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, args.ref_bases)].tobytes().decode()
    with open(ref, 'w') as f:
        f.write('>contig\n' + '\n'.join(seq[i:i + 80] for i in range(0, len(seq), 80)) + '\n')
    res = {'quantity': args.quantity, 'ref_bases': args.ref_bases, 'window': args.window, 'repeats': args.repeats}
    t = time.perf_counter()
    with open(fastq, 'wb') as out:
        subprocess.run([sys.executable, '-m', 'badread_amd', 'simulate', '--reference', ref, '--quantity', args.quantity, '--seed', '7',
                        '--truth-paf', paf], cwd=REPO, stdout=out, stderr=subprocess.DEVNULL, check=True, timeout=900)
    res['simulate_s'] = time.perf_counter() - t
    res['fastq_bytes'], res['paf_bytes'] = os.path.getsize(fastq), os.path.getsize(paf)
    say('simulated', res)

    null = io.StringIO()
    t0 = time.perf_counter()
    reads = load_fastq(fastq, output=null)
    t1 = time.perf_counter()
    refs = load_fasta(ref)[0]
    t2 = time.perf_counter()
    alignments = load_alignments(paf, output=null)
    t3 = time.perf_counter()
    lengths = [P._check_alignment(a, reads, refs, True) for a in alignments]
    t4 = time.perf_counter()
    res.update(load_fastq_s=t1 - t0, load_fasta_s=t2 - t1, load_alignments_s=t3 - t2, checks_s=t4 - t3, reads=len(reads), alignments=len(alignments))
    say('loaded', res)

    engine = default_engine()
    engine.set_kernel_timing(True)
    res['chunks'] = []
    for first, end in P.chunks(lengths, P.PLOT_CHUNK_BASES):
        t = time.perf_counter()
        job = Job(refs, reads, alignments[first:end])
        row = {'alignments': end - first, 'bases': int(job.align_read_off[-1]), 'parts': int(job.align_part_off[-1]), 'pack_s': time.perf_counter() - t}
        for label, qual, values in (('plain', False, False), ('qual', True, False), ('qual_values', True, True)):
            kernels, wall = [], []
            for i in range(args.repeats + 1):
                t = time.perf_counter()
                stats = engine.window_means(job, args.window, qual, values)[0]
                if i:
                    wall.append((time.perf_counter() - t) * 1e3)
                    kernels.append(engine.window_last())
            row['windows'] = int(stats['n'].sum())
            row[label] = {'wall_ms': statistics.median(wall), **{k + '_ms': statistics.median(x[k] for x in kernels) for k in kernels[0]}}
        # what each kernel must move: read + reference byte and 4 bytes of E per base; the scans read E twice and write 8 (with qualities:
        # the quality byte twice and 8 more); the statistics read both ends of every window; the values write 4 more per sum
        b, w = row['bases'], row['windows']
        row['bytes'] = {'errors': 6 * b, 'scans_plain': 16 * b, 'scans_qual': 26 * b, 'stats_plain': 16 * w, 'stats_qual': 32 * w, 'values_qual': 40 * w}
        row['gb_per_s'] = {'errors': 6 * b / row['plain']['errors_ms'] / 1e6, 'scans_plain': 16 * b / row['plain']['scans_ms'] / 1e6,
                           'scans_qual': 26 * b / row['qual']['scans_ms'] / 1e6, 'stats_plain': 16 * w / row['plain']['stats_ms'] / 1e6,
                           'stats_qual': 32 * w / row['qual']['stats_ms'] / 1e6, 'values_qual': 40 * w / row['qual_values']['values_ms'] / 1e6}
        res['chunks'].append(row)
        say('chunk', row)
        del job
    t = time.perf_counter()
    subprocess.run([sys.executable, '-m', 'badread_amd', 'plot', '--reference', ref, '--reads', fastq, '--alignment', paf, '--no_plot',
                    '--summary', os.devnull], cwd=REPO, stdout=subprocess.DEVNULL, check=True, timeout=1800)
    res['command_s'] = time.perf_counter() - t
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    for path in (ref, fastq, paf):
        os.remove(path)
    for name in os.listdir(work):                       # the packed-reference sidecar of simulate
        os.remove(os.path.join(work, name))
    os.rmdir(work)


if __name__ == '__main__':
    main()
