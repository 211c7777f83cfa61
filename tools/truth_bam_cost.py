"""
Cost of brx_emit_bam and brx_bgzf_device (and brx_emit_sam beside them) per device batch of configs[3] at the shipped geometry:
what profiles/truth_bam.md records.

    python tools/truth_bam_cost.py [--batches 3] [--reads 65536] [--zlib-sample 64] [--out truth_bam_cost.json]

One HipEngine with the bench's arena; every batch is simulate_batch_device, then emit_sam_device, emit_bam_device and bgzf_device
of the BAM records, each with a device synchronize around it.  Per batch: wall ms of the calls, the bytes each wrote, their
ratios to the batch's FASTQ bytes (BAM_SHARE comes from bam_per_fastq), and the ratio zlib level 1 reaches on a sample of the
same BAM bytes (`--zlib-sample` MB from the middle of the batch; one host core, not timed).
"""
import argparse
import io
import json
import os
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--reads', type=int, default=65536)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--zlib-sample', type=int, default=64, help='MB of the BAM records given to zlib level 1 for comparison')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import bench
    from badread_amd.engine import HipEngine
    wl = bench.build_workload(io.StringIO(), 'human', bench.default_ref_dir())
    eng = bench.configure(HipEngine(0, scratch_bytes=int(bench.SCRATCH_GB_DEFAULT * (1 << 30))), wl)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        return res, (time.perf_counter() - t0) * 1e3

    rows = []
    for b in range(args.batches):
        (out, st), batch_ms = timed(lambda: eng.simulate_batch_device(args.seed, b * args.reads, args.reads))
        fastq_bytes, bases = int(out.numel()), int(st['seq_len'].sum())
        (sam, _), sam_ms = timed(lambda: eng.emit_sam_device(args.reads))
        sam_bytes = int(sam.numel())
        del sam
        (bam, off), bam_ms = timed(lambda: eng.emit_bam_device(args.reads))
        bam_bytes = int(bam.numel())
        blocks, bgzf_ms = timed(lambda: eng.bgzf_device(bam))
        bgzf_bytes = int(blocks.numel())
        del blocks
        n = min(args.zlib_sample << 20, bam_bytes)
        lo = (bam_bytes - n) // 2
        sample = bytes(bam[lo:lo + n].cpu().numpy())
        (sample_blocks, _) = timed(lambda: eng.bgzf_device(bam[lo:lo + n]))
        zlib1 = sum(len(zlib.compress(sample[at:at + 65280], 1)) for at in range(0, n, 65280))
        rows.append(dict(batch=b, batch_ms=round(batch_ms, 1), emit_sam_ms=round(sam_ms, 1), emit_bam_ms=round(bam_ms, 1), bgzf_ms=round(bgzf_ms, 1),
                         fastq_bytes=fastq_bytes, sam_bytes=sam_bytes, bam_bytes=bam_bytes, bgzf_bytes=bgzf_bytes, read_bases=bases,
                         sam_per_fastq=round(sam_bytes / fastq_bytes, 4), bam_per_fastq=round(bam_bytes / fastq_bytes, 4),
                         bgzf_per_fastq=round(bgzf_bytes / fastq_bytes, 4), bgzf_per_bam=round(bgzf_bytes / bam_bytes, 4),
                         sample_bytes=n, sample_bgzf_per_bam=round(int(sample_blocks.numel()) / n, 4), sample_zlib1_per_bam=round(zlib1 / n, 4),
                         bam_bytes_per_ms=round(bam_bytes / bam_ms), sam_bytes_per_ms=round(sam_bytes / sam_ms),
                         bgzf_in_bytes_per_ms=round(bam_bytes / bgzf_ms), engine_retries=getattr(eng, 'retries', 0)))
        del bam, sample_blocks
        print(json.dumps(rows[-1]), flush=True)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
