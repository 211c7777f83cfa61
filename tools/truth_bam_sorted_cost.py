"""
Cost of --truth-bam-sorted at the end of a job: what profiles/truth_bam_sorted.md records.

    python tools/truth_bam_sorted_cost.py [--job-batches 16] [--reads 65536] [--repeats 3] [--workload human] [--out cost.json]

One HipEngine with the bench's arena and the workload's geometry (human: configs[3]).  `--job-batches` batches of `--reads` reads leave
their BAM records on the device (emit_bam_device), every read a segment.  Then, `--repeats` times each with a device synchronize around
every call: bam_sort (wall ms and, from HIP events, its stages: walk, sort, table, gather), a device-to-device copy of the same bytes
beside the gather, bgzf_device with offsets over the sorted stream in the spans the driver uses, bam_index (wall ms and stages).  Records,
bytes, scratch sizes, the peak of the device allocator and of the process's resident set.  --check: the host sorts the table's keys and
compares (numpy, stable).
"""
import argparse
import io
import json
import os
import resource
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--job-batches', type=int, default=16)
    ap.add_argument('--reads', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--workload', default='human')
    ap.add_argument('--check', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from badread_amd import engine as E
    from badread_amd import simulate as S
    wl = bench.build_workload(io.StringIO(), args.workload, bench.default_ref_dir())
    pref = wl[0]
    eng = bench.configure(E.HipEngine(0, scratch_bytes=int(bench.SCRATCH_GB_DEFAULT * (1 << 30))), wl)
    eng.set_kernel_timing(True)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        return res, (time.perf_counter() - t0) * 1e3

    parts, lens = [], []
    for b in range(args.job_batches):
        eng.simulate_batch_device(args.seed, b * args.reads, args.reads)
        data, off = eng.emit_bam_device(args.reads)
        parts.append(data)
        lens.append(np.diff(off.astype(np.int64)))
    records = torch.cat(parts)
    del parts
    seg_off = np.concatenate(([0], np.cumsum(np.concatenate(lens)))).astype(np.uint64)
    n_bytes, n_ref, max_pos = int(records.numel()), len(pref.names), max(int(x) for x in pref.lengths)
    torch.cuda.reset_peak_memory_stats()
    job = dict(workload=args.workload, batches=args.job_batches, reads=args.job_batches * args.reads, bytes=n_bytes, n_ref=n_ref,
               sort_scratch_bytes=int(eng.lib.brx_bam_sort_scratch(n_bytes, len(seg_off) - 1)))
    sort_ms, sort_stages, out = [], [], None
    for _ in range(args.repeats):
        del out
        out, t = timed(lambda: eng.bam_sort(records, seg_off, n_ref, max_pos))
        sort_ms.append(round(t, 2))
        sort_stages.append({k: round(v, 3) for k, v in list(eng.bamsort_last().items())[:4]})
    ordered, table, n, unmapped = out
    job.update(records=n, unmapped=unmapped, sort_wall_ms=sort_ms, sort_stages_ms=sort_stages)
    copy_ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dst = torch.empty_like(records)
        a.record()
        dst.copy_(records)
        b.record()
        torch.cuda.synchronize()
        copy_ms.append(round(a.elapsed_time(b), 3))
        del dst
    job['device_copy_of_the_same_bytes_ms'] = copy_ms
    if args.check:
        t = np.frombuffer(table.cpu().numpy().tobytes(), dtype=E.BAM_REC_DTYPE)
        key = (t['refID'].astype(np.uint32).astype(np.uint64) << np.uint64(32)) | t['pos'].astype(np.uint32).astype(np.uint64)
        assert (np.diff(key.astype(np.float64)) >= 0).all() and int((t['refID'] < 0).sum()) == unmapped and int(t['off'][-1]) < n_bytes
        job['checked'] = True
    del records
    bgzf_ms, block_off, total = [], None, 0
    for _ in range(args.repeats):
        block_off, total, ms = [], 0, 0.0
        for at in range(0, n_bytes, S.SORTED_SPAN):
            (blocks, off), t = timed(lambda: eng.bgzf_device(ordered[at:at + S.SORTED_SPAN], offsets=True))
            ms += t
            block_off.append(off[:-1] + np.uint64(total))
            total += int(off[-1])
            del blocks
        bgzf_ms.append(round(ms, 2))
    block_off = np.concatenate(block_off + [np.array([total], dtype=np.uint64)])
    job.update(bgzf_wall_ms=bgzf_ms, compressed_bytes=total, blocks=len(block_off) - 1)
    index_ms, index_stages, bai = [], [], None
    for _ in range(args.repeats):
        bai, t = timed(lambda: eng.bam_index(table, n_ref, n_bytes, block_off, 1000))
        index_ms.append(round(t, 2))
        index_stages.append({k: round(v, 3) for k, v in list(eng.bamsort_last().items())[4:]})
    job.update(index_wall_ms=index_ms, index_stages_ms=index_stages, bai_bytes=int(bai.numel()),
               index_scratch_bytes=int(eng.lib.brx_bam_index_scratch(n, n_ref)),
               peak_device_bytes_beside_the_arena=int(torch.cuda.max_memory_allocated()) - int(bench.SCRATCH_GB_DEFAULT * (1 << 30)),
               peak_host_rss_bytes=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024)
    job['medians_ms'] = dict(sort=statistics.median(sort_ms), copy=statistics.median(copy_ms), bgzf=statistics.median(bgzf_ms), index=statistics.median(index_ms))
    print(json.dumps(job), flush=True)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(job, f, indent=1)


if __name__ == '__main__':
    main()
