"""
Cost of brx_emit_sam (and brx_emit_paf beside it) per device batch of configs[3] at the shipped geometry: what
profiles/truth_sam.md records.

    python tools/truth_sam_cost.py [--batches 3] [--reads 65536] [--out truth_sam_cost.json]

One HipEngine with the bench's arena; every batch is simulate_batch_device, then emit_paf_device, then emit_sam_device, each
with a device synchronize around it.  Per batch: wall ms of the three calls, BRX_STAGE_EMIT (k_recsize + k_scan_rec + k_emit
of the same batch, by HIP events), the bytes each wrote, SAM lines, and the bytes per ms of the SAM pass and of the emit stage.
"""
import argparse
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--reads', type=int, default=65536)
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

    rows = []
    for b in range(args.batches):
        (out, st), batch_ms = timed(lambda: eng.simulate_batch_device(args.seed, b * args.reads, args.reads))
        emit_ms = eng.stage_ms()['emit']
        fastq_bytes, bases = int(out.numel()), int(st['seq_len'].sum())
        (paf, _), paf_ms = timed(lambda: eng.emit_paf_device(args.reads))
        paf_bytes = int(paf.numel())
        del paf
        (sam, _), sam_ms = timed(lambda: eng.emit_sam_device(args.reads))
        sam_bytes = int(sam.numel())
        lines = int((sam == 10).sum())
        del sam
        retries = getattr(eng, 'retries', 0)
        rows.append(dict(batch=b, batch_ms=round(batch_ms, 1), stage_emit_ms=round(emit_ms, 2), emit_paf_ms=round(paf_ms, 1),
                         emit_sam_ms=round(sam_ms, 1), fastq_bytes=fastq_bytes, paf_bytes=paf_bytes, sam_bytes=sam_bytes, sam_lines=lines,
                         read_bases=bases, sam_per_fastq=round(sam_bytes / fastq_bytes, 4),
                         sam_bytes_per_ms=round(sam_bytes / sam_ms), emit_bytes_per_ms=round(fastq_bytes / max(emit_ms, 1e-9)),
                         sam_slower_per_byte=round((sam_ms / sam_bytes) / (max(emit_ms, 1e-9) / fastq_bytes), 2), engine_retries=retries))
        print(json.dumps(rows[-1]), flush=True)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
