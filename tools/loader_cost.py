"""
Cost of reading the PAF back with and without --gpu-loader, and the FASTQ with and without --gpu-reads, on reads of the project's own
simulate: what profiles/gpu_loader.md and profiles/gpu_reads.md record.

    python tools/loader_cost.py [--quantity 1500M] [--ref-bases 2000000] [--runs 3] [--routes host,device,reads] [--out loader_cost.json]

The input of tools/plot_windows_cost.py: a random one-contig reference, `simulate --quantity Q --seed 7 --truth-paf` at the default lengths.
Then `--runs` times per route, the routes taking turns (the host's load_alignments + model_builder.Job, and load_alignments_device +
Job.packed), the three host steps of `plot` with the host's clock: loading the alignments, the checks per alignment, packing every chunk; on the device route under
brx_set_kernel_timing, so that the HIP-event times of brx_paf_scan and of every brx_align_pack are there too, with the bytes they move.
Last, `plot --no_plot --summary /dev/null` as a child process, `--runs` times per route, the routes taking turns.
The route `reads` is `device` with --gpu-reads on top: load_fastq_device in place of load_fastq and Job.packed over its DeviceReads, with
the HIP-event times of brx_fastq_scan and of every brx_reads_pack and, beside each pack, a device-to-device copy of the bytes it wrote.
Every route loads its reads in every run (`reads_s`), and `total_s` = reads_s + sum_s is what profiles/gpu_reads.md compares.
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
    ap.add_argument('--routes', default='host,device,reads')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    routes = tuple(args.routes.split(','))
    assert routes and set(routes) <= {'host', 'device', 'reads'}
    import numpy as np
    from badread_amd import plot_window_identity as P
    from badread_amd.alignment import load_alignments, load_alignments_device
    from badread_amd.engine import default_engine
    from badread_amd.misc import load_fasta, load_fastq
    from badread_amd.model_builder import Job
    from badread_amd.reads import load_fastq_device

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
        refs = load_fasta(ref)[0]
        engine = default_engine()
        torch = engine.torch
        engine.set_kernel_timing(True)
        engine.paf_scan(engine._upload(np.frombuffer(b'a\tb\n', dtype=np.uint8))[1][:4])              # the first launch of a process
        engine.fastq_scan(engine._upload(np.frombuffer(b'@a\nA\n+\n!\n', dtype=np.uint8))[1][:9])
        for route in routes:
            res[route] = []
        for route in routes * args.runs:                                     # the routes take turns
            t0 = time.perf_counter()
            reads = load_fastq_device(fastq, engine, output=null) if route == 'reads' else load_fastq(fastq, output=null)
            reads_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            alignments = load_alignments(paf, output=null) if route == 'host' else load_alignments_device(paf, engine, output=null)
            t1 = time.perf_counter()
            row = {'reads_s': reads_s, 'load_s': t1 - t0, 'alignments': len(alignments)}
            if route == 'reads':
                row['fastq_scan_ms'] = engine.reads_last()['scan']
                row['fastq_scan_gb_per_s'] = res['fastq_bytes'] / row['fastq_scan_ms'] / 1e6
            if route != 'host':
                row['scan_ms'] = engine.loader_last()['scan']
                row['scan_gb_per_s'] = res['paf_bytes'] / row['scan_ms'] / 1e6
            lengths = P.check_alignments(alignments, reads, refs, True)
            t2 = time.perf_counter()
            row['checks_s'] = t2 - t1
            pack_s = join_s = pack_ms = reads_pack_ms = copy_ms = 0.0
            parts = ref_bases = cigar_bytes = chunks = read_bases = 0
            for first, end in P.chunks(lengths, P.PLOT_CHUNK_BASES):
                t = time.perf_counter()
                job = Job(refs, reads, alignments[first:end]) if route == 'host' else Job.packed(engine, refs, reads, alignments, first, end)
                pack_s += time.perf_counter() - t
                chunks += 1
                parts += int(job.align_part_off[-1])
                if route != 'host':
                    pack_ms += engine.loader_last()['pack']
                    ref_bases += int(job.align_ref_off[-1])
                    cigar_bytes += int(alignments.rec['cigar_len'][first:end].sum())
                if route == 'reads':                                         # beside the pack: hipMemcpyAsync of what it wrote, device to device
                    reads_pack_ms += engine.reads_last()['pack']
                    read_bases += int(job.align_read_off[-1])
                    spare = [torch.empty_like(job.seq), torch.empty_like(job.qual)]
                    marks = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    marks[0].record()
                    spare[0].copy_(job.seq, non_blocking=True)
                    spare[1].copy_(job.qual, non_blocking=True)
                    marks[1].record()
                    marks[1].synchronize()
                    copy_ms += marks[0].elapsed_time(marks[1])
                    del spare
                if route == 'device':
                    t = time.perf_counter()                                  # what of the packing is the join of the read slices
                    ''.join(reads[a.read_name][0][a.read_start:a.read_end] for a in alignments[first:end]).encode('latin-1')
                    ''.join(reads[a.read_name][1][a.read_start:a.read_end] for a in alignments[first:end]).encode('latin-1')
                    join_s += time.perf_counter() - t
                del job
            row.update(pack_s=pack_s, chunks=chunks, parts=parts, sum_s=row['load_s'] + row['checks_s'] + pack_s)
            row['total_s'] = row['reads_s'] + row['sum_s']
            if route != 'host':
                moved = cigar_bytes + 29 * parts + 2 * ref_bases                # the CIGAR text, 29 bytes per part written, each slice read and written
                row.update(pack_ms=pack_ms, pack_bytes=moved, pack_gb_per_s=moved / pack_ms / 1e6)
            if route == 'device':
                row.update(join_of_read_slices_s=join_s)
            if route == 'reads':                                             # seq and qual: every base read once and written once, twice
                row.update(reads_pack_ms=reads_pack_ms, reads_pack_bytes=4 * read_bases, reads_pack_gb_per_s=4 * read_bases / reads_pack_ms / 1e6,
                           copy_ms=copy_ms, copy_gb_per_s=4 * read_bases / copy_ms / 1e6)
            res[route].append(row)
            say(route, row)
            del alignments, reads
        del refs
        engine.close()
        flags = {'host': [], 'device': ['--gpu-loader'], 'reads': ['--gpu-loader', '--gpu-reads']}
        res['command_s'] = {route: [] for route in routes}
        for _ in range(args.runs):
            for route, flag in ((route, flags[route]) for route in routes):
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
