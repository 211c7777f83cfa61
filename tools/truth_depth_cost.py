"""
Cost of --truth-depth on configs[3] at the shipped geometry: what profiles/truth_depth.md records.

    python tools/truth_depth_cost.py [--batches 3] [--reads 65536] [--repeats 3] [--job-batches 94] [--check] [--out truth_depth_cost.json]

One HipEngine with the bench's arena.  Per batch: simulate_batch_device, then emit_paf_device and emit_truth_device('depth') `--repeats`
times each with a device synchronize around every call (the median is reported), the records and the bytes of both.  Then the job:
`--job-batches` batches in all (94 of 65 536 reads are the 30x product command's 6.16 M reads; the timed ones count) leave their events on
the device, and depth_bedgraph runs `--repeats` times on all of them: wall ms, the stages' ms (engine.depth_last), the sort passes, the
events and the bytes of text; with --check the text is read on the host line by line (every contig tiled, neighbours differ, covered
bases = the events' spans).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--reads', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--job-batches', type=int, default=94)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--check', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from badread_amd import engine as E
    wl = bench.build_workload(io.StringIO(), 'human', bench.default_ref_dir())
    pref = wl[0]
    eng = bench.configure(E.HipEngine(0, scratch_bytes=int(bench.SCRATCH_GB_DEFAULT * (1 << 30))), wl)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        return res, (time.perf_counter() - t0) * 1e3

    def median_of(call, repeats):
        ms, data = [], None
        for _ in range(repeats):
            del data
            (data, _), t = timed(call)
            ms.append(round(t, 2))
        return data, round(statistics.median(ms), 2), ms

    rows, events = [], []
    for b in range(max(args.batches, args.job_batches)):
        (out, st), batch_ms = timed(lambda: eng.simulate_batch_device(args.seed, b * args.reads, args.reads))
        if b >= args.batches:
            events.append(eng.emit_truth_device('depth', args.reads)[0])
            continue
        row = dict(batch=b, batch_ms=round(batch_ms, 1), fastq_bytes=int(out.numel()), read_bases=int(st['seq_len'].sum()))
        paf, row['paf_ms'], row['paf_all_ms'] = median_of(lambda: eng.emit_paf_device(args.reads), args.repeats)
        row['paf_bytes'] = int(paf.numel())
        del paf
        ev, row['depth_ms'], row['depth_all_ms'] = median_of(lambda: eng.emit_truth_device('depth', args.reads), args.repeats)
        row['depth_bytes'], row['records'] = int(ev.numel()), int(ev.numel()) // 16
        row['depth_per_fastq'] = round(row['depth_bytes'] / row['fastq_bytes'], 6)
        row['first_buffer_too_small'] = row['depth_bytes'] > int(args.reads * E.DEPTH_SHARE * eng.expected_record_bytes()) + (1 << 16)
        events.append(ev)
        rows.append(row)
        print(json.dumps(row), flush=True)
    all_events = torch.cat(events)
    del events
    text, wall_ms, wall_all = None, None, []
    stages = []
    for _ in range(args.repeats):
        del text
        text, t = timed(lambda: eng.depth_bedgraph(all_events))
        wall_all.append(round(t, 2))
        passes, ms = eng.depth_last()
        stages.append({k: round(v, 2) for k, v in ms.items()})
    job = dict(job_batches=max(args.batches, args.job_batches), events=int(all_events.numel()) // 8, sort_passes=passes, text_bytes=int(text.numel()),
               wall_ms=round(statistics.median(wall_all), 2), wall_all_ms=wall_all, stages_ms=stages,
               scratch_bytes=int(eng.lib.brx_depth_bedgraph_scratch(int(all_events.numel()) // 8)))
    if args.check:
        # the shape of the text, on the host
        host = text.cpu().numpy().tobytes().decode()
        ev = all_events.cpu().numpy().view(np.uint64)
        pos = ((ev >> np.uint64(1)) & np.uint64((1 << 39) - 1)).astype(np.int64)
        spans = int(np.where(ev & np.uint64(1), -pos, pos).sum())
        covered, at, lines = 0, 0, host.split('\n')[:-1]
        for name, length in zip(pref.names, pref.lengths):
            p, last = 0, None
            while at < len(lines) and p < int(length):
                n, s, e, d = lines[at].split('\t')
                assert n == str(name) and int(s) == p and int(e) > p and int(d) != last and int(d) >= 0, lines[at]
                covered += int(d) * (int(e) - int(s))
                p, last, at = int(e), int(d), at + 1
            assert p == int(length), (name, p)
        assert at == len(lines) and covered == spans, (at, len(lines), covered, spans)
        job.update(lines=len(lines), covered_bases=covered, mean_depth=round(covered / float(pref.n_bases), 3))
    print(json.dumps(job), flush=True)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(dict(batches=rows, job=job), f, indent=1)


if __name__ == '__main__':
    main()
