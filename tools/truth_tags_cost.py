"""
Cost of MD:Z: and SA:Z: (--truth-tags) per device batch of configs[3] at the shipped geometry: what profiles/truth_tags.md records.

    python tools/truth_tags_cost.py [--batches 3] [--reads 65536] [--repeats 3] [--out truth_tags_cost.json]

One HipEngine with the bench's arena; every batch is simulate_batch_device, then emit_sam_device and emit_bam_device at tags 0, MD,
SA and MD|SA, `--repeats` times each with a device synchronize around every call (the median is reported; the first call of a
kind also sizes its buffer), and bgzf_device of the BAM records with both tags.  Per batch: the ms and bytes of every call, what the
tags add per FASTQ byte (engine.MD_SHARE and SA_SHARE come from md_per_fastq and sa_per_fastq) and the BGZF ratio of the tagged BAM.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]

MASKS = ((0, 'none'), (1, 'md'), (2, 'sa'), (3, 'md_sa'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--reads', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seed', type=int, default=42)
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

    def median_of(call):
        """(bytes, median ms, every ms) of `repeats` calls; the tensors are dropped at once."""
        ms, nbytes = [], 0
        for _ in range(args.repeats):
            (data, _), t = timed(call)
            nbytes = int(data.numel())
            del data
            ms.append(round(t, 2))
        return nbytes, round(statistics.median(ms), 2), ms

    rows = []
    for b in range(args.batches):
        (out, st), batch_ms = timed(lambda: eng.simulate_batch_device(args.seed, b * args.reads, args.reads))
        fastq_bytes = int(out.numel())
        row = dict(batch=b, batch_ms=round(batch_ms, 1), fastq_bytes=fastq_bytes, read_bases=int(st['seq_len'].sum()))
        for tags, name in MASKS:
            row[f'sam_{name}_bytes'], row[f'sam_{name}_ms'], row[f'sam_{name}_all_ms'] = median_of(lambda: eng.emit_sam_device(args.reads, tags))
            row[f'bam_{name}_bytes'], row[f'bam_{name}_ms'], row[f'bam_{name}_all_ms'] = median_of(lambda: eng.emit_bam_device(args.reads, 65535, tags))
        (bam, _), _ = timed(lambda: eng.emit_bam_device(args.reads, 65535, 3))
        blocks, bgzf_ms = timed(lambda: eng.bgzf_device(bam))
        row.update(bgzf_ms=round(bgzf_ms, 1), bgzf_bytes=int(blocks.numel()), bgzf_per_bam=round(int(blocks.numel()) / int(bam.numel()), 4))
        del bam, blocks
        (plain, _), _ = timed(lambda: eng.emit_bam_device(args.reads))
        plain_blocks, plain_ms = timed(lambda: eng.bgzf_device(plain))
        row.update(bgzf_untagged_ms=round(plain_ms, 1), bgzf_untagged_per_bam=round(int(plain_blocks.numel()) / int(plain.numel()), 4))
        del plain, plain_blocks
        row.update(md_per_fastq=round((row['sam_md_bytes'] - row['sam_none_bytes']) / fastq_bytes, 4),
                   sa_per_fastq=round((row['sam_sa_bytes'] - row['sam_none_bytes']) / fastq_bytes, 4),
                   bam_md_per_fastq=round((row['bam_md_bytes'] - row['bam_none_bytes']) / fastq_bytes, 4),
                   bam_sa_per_fastq=round((row['bam_sa_bytes'] - row['bam_none_bytes']) / fastq_bytes, 4),
                   engine_retries=getattr(eng, 'retries', 0))
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
