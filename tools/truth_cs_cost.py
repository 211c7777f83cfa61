"""
Cost of cs:Z: and =/X CIGARs (--truth-cs, --truth-eqx) per device batch of configs[3] at the shipped geometry: what
profiles/truth_cs.md records.

    python tools/truth_cs_cost.py [--batches 3] [--reads 65536] [--repeats 3] [--out truth_cs_cost.json]
    python tools/truth_cs_cost.py --plain-only                                 # the fmt = 0 emitters alone, for the parent comparison

One HipEngine with the bench's arena; every batch is simulate_batch_device, then emit_paf_device, emit_sam_device and emit_bam_device
at fmt 0, EQX, CS, CS|LONG and EQX|CS, and emit_sam_device / emit_bam_device with MD beside them, `--repeats` times each with a device
synchronize around every call (the median is reported; the first call of a kind also sizes its buffer).  Per batch: the ms and bytes
of every call and what each option adds per FASTQ byte and per file (engine.EQX_SHARE, CS_SHORT_SHARE and CS_LONG_SHARE come from
*_per_fastq), and the retries of the first buffers.

--plain-only calls only the emitters without formats (six calls each per batch, the first dropped, median of the rest) through
nothing newer than emit_*_device(n), so a copy of this file runs in a checkout of the parent commit as well.
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

FMTS = ((0, 'none'), (1, 'eqx'), (2, 'cs'), (6, 'cs_long'), (3, 'eqx_cs'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--reads', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import bench
    from badread_amd import engine as E
    wl = bench.build_workload(io.StringIO(), 'human', bench.default_ref_dir())
    eng = bench.configure(E.HipEngine(0, scratch_bytes=int(bench.SCRATCH_GB_DEFAULT * (1 << 30))), wl)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        return res, (time.perf_counter() - t0) * 1e3

    def median_of(call, repeats, drop=0):
        """(bytes, median ms, every ms) of `repeats` calls, the first `drop` left out of the median; the tensors are dropped at once."""
        ms, nbytes = [], 0
        for _ in range(repeats):
            (data, _), t = timed(call)
            nbytes = int(data.numel())
            del data
            ms.append(round(t, 2))
        return nbytes, round(statistics.median(ms[drop:]), 2), ms

    rows = []
    for b in range(args.batches):
        (out, st), batch_ms = timed(lambda: eng.simulate_batch_device(args.seed, b * args.reads, args.reads))
        fastq_bytes = int(out.numel())
        row = dict(batch=b, batch_ms=round(batch_ms, 1), fastq_bytes=fastq_bytes, read_bases=int(st['seq_len'].sum()))
        if args.plain_only:
            for kind, call in (('sam', lambda: eng.emit_sam_device(args.reads)), ('bam', lambda: eng.emit_bam_device(args.reads)),
                               ('paf', lambda: eng.emit_paf_device(args.reads))):
                row[f'{kind}_bytes'], row[f'{kind}_ms'], row[f'{kind}_all_ms'] = median_of(call, 6, drop=1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            continue
        retries = 0
        for fmt, name in FMTS:
            for kind, call in (('paf', lambda: eng.emit_paf_device(args.reads, fmt)), ('sam', lambda: eng.emit_sam_device(args.reads, 0, fmt)),
                               ('bam', lambda: eng.emit_bam_device(args.reads, 65535, 0, fmt))):
                row[f'{kind}_{name}_bytes'], row[f'{kind}_{name}_ms'], row[f'{kind}_{name}_all_ms'] = median_of(call, args.repeats)
        for kind, call in (('sam', lambda: eng.emit_sam_device(args.reads, E.TAG_MD)), ('bam', lambda: eng.emit_bam_device(args.reads, 65535, E.TAG_MD))):
            row[f'{kind}_md_bytes'], row[f'{kind}_md_ms'], row[f'{kind}_md_all_ms'] = median_of(call, args.repeats)
        for kind in ('paf', 'sam', 'bam'):
            base = row[f'{kind}_none_bytes']
            for name in ('eqx', 'cs', 'cs_long'):
                row[f'{kind}_{name}_per_fastq'] = round((row[f'{kind}_{name}_bytes'] - base) / fastq_bytes, 4)
                row[f'{kind}_{name}_add_ms'] = round(row[f'{kind}_{name}_ms'] - row[f'{kind}_none_ms'], 2)
            if kind != 'paf':
                row[f'{kind}_md_per_fastq'] = round((row[f'{kind}_md_bytes'] - base) / fastq_bytes, 4)
                row[f'{kind}_md_add_ms'] = round(row[f'{kind}_md_ms'] - row[f'{kind}_none_ms'], 2)
            # a first buffer that was too small: the share of this option, times the bytes expected, against what was written
            cap = lambda share: int(args.reads * share * eng.expected_record_bytes()) + (1 << 16)
            plain = dict(paf=E.PAF_SHARE, sam=E.SAM_SHARE, bam=E.BAM_SHARE)[kind]
            for fmt, name in FMTS[1:]:
                retries += row[f'{kind}_{name}_bytes'] > cap(plain + E.fmt_share(fmt, kind))
        row['first_buffers_too_small'] = retries
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
