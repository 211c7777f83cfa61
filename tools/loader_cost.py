"""
Cost of reading the PAF back with and without --gpu-loader, on reads of the project's own simulate: what profiles/gpu_loader.md records.

    python tools/loader_cost.py [--quantity 1500M] [--ref-bases 2000000] [--runs 3] [--out loader_cost.json]

The input of tools/plot_windows_cost.py: a random one-contig reference, `simulate --quantity Q --seed 7 --truth-paf` at the default lengths.
Then `--runs` times per route, the routes taking turns (the host's load_alignments + model_builder.Job, and load_alignments_device +
Job.packed), the three host steps of `plot` with the host's clock: loading the alignments, the checks per alignment, packing every chunk; on the device route under
brx_set_kernel_timing, so that the HIP-event times of brx_paf_scan and of every brx_align_pack are there too, with the bytes they move.
Last, `plot --no_plot --summary /dev/null` as a child process, `--runs` times per route, the routes taking turns.
"""
import argparse
import io
import json
import os
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
    ap.add_argument('--quantity', default='1500M')
    ap.add_argument('--ref-bases', type=int, default=2000000)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    from badread_amd import plot_window_identity as P
    from badread_amd.alignment import load_alignments, load_alignments_device
    from badread_amd.engine import default_engine
    from badread_amd.misc import load_fasta, load_fastq
    from badread_amd.model_builder import Job

    work = tempfile.mkdtemp(prefix='loader_cost_')
    ref, fastq, paf = (os.path.join(work, x) for x in ('ref.fasta', 'reads.fastq', 'truth.paf'))
    seq = np.frombuffer(b'ACGT', dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, args.ref_bases)].tobytes().decode()
    with open(ref, 'w') as f:
        f.write('>contig\n' + '\n'.join(seq[i:i + 80] for i in range(0, len(seq), 80)) + '\n')
    try:
        res = {'quantity': args.quantity, 'ref_bases': args.ref_bases}
        with open(fastq, 'wb') as out:
            subprocess.run([sys.executable, '-m', 'badread_amd', 'simulate', '--reference', ref, '--quantity', args.quantity, '--seed', '7',
                            '--truth-paf', paf], cwd=REPO, stdout=out, stderr=subprocess.DEVNULL, check=True, timeout=900)
        res['fastq_bytes'], res['paf_bytes'] = os.path.getsize(fastq), os.path.getsize(paf)
        say('simulated', res)

        null = io.StringIO()
        t = time.perf_counter()
        reads = load_fastq(fastq, output=null)
        res['load_fastq_s'] = time.perf_counter() - t
        refs = load_fasta(ref)[0]
        engine = default_engine()
        engine.set_kernel_timing(True)
        engine.paf_scan(engine._upload(np.frombuffer(b'a\tb\n', dtype=np.uint8))[1][:4])              # the first launch of a process
        res['host'], res['device'] = [], []
        for route in ('host', 'device') * args.runs:                         # the routes take turns
            t0 = time.perf_counter()
            alignments = load_alignments_device(paf, engine, output=null) if route == 'device' else load_alignments(paf, output=null)
            t1 = time.perf_counter()
            row = {'load_s': t1 - t0, 'alignments': len(alignments)}
            if route == 'device':
                row['scan_ms'] = engine.loader_last()['scan']
                row['scan_gb_per_s'] = res['paf_bytes'] / row['scan_ms'] / 1e6
            lengths = P.check_alignments(alignments, reads, refs, True)
            t2 = time.perf_counter()
            row['checks_s'] = t2 - t1
            pack_s = join_s = pack_ms = 0.0
            parts = ref_bases = cigar_bytes = chunks = 0
            for first, end in P.chunks(lengths, P.PLOT_CHUNK_BASES):
                t = time.perf_counter()
                job = Job.packed(engine, refs, reads, alignments, first, end) if route == 'device' else Job(refs, reads, alignments[first:end])
                pack_s += time.perf_counter() - t
                chunks += 1
                parts += int(job.align_part_off[-1])
                if route == 'device':
                    pack_ms += engine.loader_last()['pack']
                    ref_bases += int(job.align_ref_off[-1])
                    cigar_bytes += int(alignments.rec['cigar_len'][first:end].sum())
                    t = time.perf_counter()                                  # what of the packing is the join of the read slices
                    ''.join(reads[a.read_name][0][a.read_start:a.read_end] for a in alignments[first:end]).encode('latin-1')
                    ''.join(reads[a.read_name][1][a.read_start:a.read_end] for a in alignments[first:end]).encode('latin-1')
                    join_s += time.perf_counter() - t
                del job
            row.update(pack_s=pack_s, chunks=chunks, parts=parts, sum_s=row['load_s'] + row['checks_s'] + pack_s)
            if route == 'device':
                moved = cigar_bytes + 29 * parts + 2 * ref_bases                # the CIGAR text, 29 bytes per part written, each slice read and written
                row.update(pack_ms=pack_ms, pack_bytes=moved, pack_gb_per_s=moved / pack_ms / 1e6, join_of_read_slices_s=join_s)
            res[route].append(row)
            say(route, row)
            del alignments
        del reads, refs
        engine.close()
        res['command_s'] = {'host': [], 'device': []}
        for _ in range(args.runs):
            for route, flag in (('host', []), ('device', ['--gpu-loader'])):
                t = time.perf_counter()
                subprocess.run([sys.executable, '-m', 'badread_amd', 'plot', '--reference', ref, '--reads', fastq, '--alignment', paf, '--no_plot',
                                '--summary', os.devnull] + flag, cwd=REPO, stdout=subprocess.DEVNULL, check=True, timeout=1800)
                res['command_s'][route].append(time.perf_counter() - t)
                say(route, res['command_s'][route][-1])
        text = json.dumps(res, indent=1)
        print(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text + '\n')
    finally:
        for name in os.listdir(work):                   # the inputs and the packed-reference sidecar of simulate
            os.remove(os.path.join(work, name))
        os.rmdir(work)


if __name__ == '__main__':
    main()
