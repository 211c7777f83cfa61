"""
GPU: --truth-bam on the MI355X.  The emulated-device checks of tests/test_truth_bam.py on the HIP engine (the BAM records equal
the plain-Python transform of the batch's SAM lines, byte for byte, and decode back to them; every branch shown), the BGZF
cases, long reads on the repeat-rich reference, one read whose CIGAR has more than 65535 operations, the command line (the
decompressed BAM independent of streams and batch sizes, FASTQ and SAM unchanged by the flag) and two ranks on one GPU.
"""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bam_codec as BC
import helpers as H
import test_truth_bam as TB
import test_truth_paf as T
import test_truth_sam as TS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_truth_bam_of_the_batches_on_the_gpu():
    TB.check_batches(H.hip_engine, 400, 512, low=(0, 64))


def test_hip_kernels_write_valid_bgzf_blocks():
    TB.check_bgzf(H.hip_engine())


def test_truth_bam_of_long_reads_on_the_gpu():
    """--length 15000,13000 on the 3.4 Mb repeat-rich reference: many 128-base steps and many records per read."""
    import lowcomplexity as L
    eng = L.configure_case(H.hip_engine(), 'default')
    pref = L.packed_reference('large')
    n = 512
    st, sam, bams = TB.emit_sam_and_bams(eng, 7, n, (65535,))
    bam, off = bams[65535]
    TB.check_bam(pref, st, sam, bam, off, 65535)
    per_read = np.array([len(BC.records_of_bam(bam[int(off[r]):int(off[r + 1])])) for r in range(n)])
    print('truth_bam_long_reads', dict(records=int(per_read.sum()), longest=int(st['seq_len'].max()), most_records=int(per_read.max()),
                                       bam_bytes=len(bam), sam_bytes=len(sam)))
    assert int(st['seq_len'].max()) > 30000 and int(per_read.max()) >= 4 and len(bam) < 0.8 * len(sam)


def test_a_cigar_of_more_than_65535_operations_goes_into_the_cg_tag():
    """One read of 179 kb at 53.8 % identity, alone in its batch, with the real limit: 80 110 operations in one record.

    The configuration is the wide-path workload of tests/test_gpu_fullsize.py (bench.py 'wide': the configs[1] reference, nanopore2023,
    --identity 60,75,8) with --length 200000,10000 --glitches 0,0,0, read 1.  That file's own witness, read 50 of the unchanged workload
    (155 kb, target identity 53 %), does NOT pass 65535: a glitch ends a record, so under the workload's glitches (one per 10 kb) its truth
    is 13 records of at most 12 989 operations each, and without glitches it is one record of 48 145 (M covers = and X; 0.33 operations
    per base at this identity, 0.45 at a target of 51 %).  So the read is longer and its target identity lower; measured on an MI355X."""
    import bench
    from badread_amd.engine import HipEngine
    wl = bench.build_workload(io.StringIO(), 'wide', bench.default_ref_dir())
    pref, p = wl[0], wl[4]
    p.glitch_rate = p.glitch_size = p.glitch_skip = 0.0
    p.frag_mean, p.frag_stdev = 200000.0, 10000.0
    p.gamma_k, p.gamma_t = p.frag_mean ** 2 / p.frag_stdev ** 2, p.frag_stdev ** 2 / p.frag_mean
    eng = bench.configure(HipEngine(0, scratch_bytes=16 << 30), wl)
    _, st = eng.simulate_batch(42, 1, 1)
    identity = float(st['n_match'][0]) / float(st['n_cols'][0])
    sam = bytes(eng.emit_sam_device(1)[0].cpu().numpy())
    bam = bytes(eng.emit_bam_device(1)[0].cpu().numpy())
    eng.close()
    names = list(pref.names)
    lines = sam.decode('latin-1').splitlines()
    n_ops = [len(re.findall(r'\d+[MIDSH]', line.split('\t')[5])) for line in lines]
    print('truth_bam_long_cigar', dict(lines=len(lines), ops=n_ops, bases=int(st['seq_len'][0]), identity=round(identity, 4), bam_bytes=len(bam)))
    assert int(st['status'][0]) == 0 and int(st['seq_len'][0]) >= 150000 and 0.5 < identity < 0.56
    assert max(n_ops) > 65535
    assert bam == BC.bam_from(sam, names) and BC.sam_of_bam(bam, names) == sam
    recs = BC.records_of_bam(bam)
    assert len(recs) == len(lines)
    for rec, line, n in zip(recs, lines, n_ops):
        if n > 65535:
            cg = rec['tags'][-1]
            assert len(rec['cigar']) == 2 and rec['cigar'][0] == (rec['l_seq'], 4) and rec['cigar'][1][1] == 3
            assert cg[0] == 'CG' and cg[1] == 'BI' and len(cg[2]) == n
            assert ''.join(f'{w >> 4}{BC.CIGAR_OPS[w & 15]}' for w in cg[2]) == line.split('\t')[5]
        else:
            assert len(rec['cigar']) == n and all(t[0] != 'CG' for t in rec['tags'])


def run_cli(tmp_path, name, *extra, sam=None):
    bam = tmp_path / (name or 'unused.bam')
    cmd = [sys.executable, '-m', 'badread_amd', 'simulate', '--reference', T.SMALL_REF, '--quantity', '40x', '--length', '400,300',
           '--seed', '11'] + list(extra)
    if name:
        cmd += ['--truth-bam', str(bam)]
    if sam:
        cmd += ['--truth-sam', str(tmp_path / sam)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, (bam.read_bytes() if name else None), ((tmp_path / sam).read_bytes() if sam else None)


def test_truth_bam_from_the_cli(tmp_path):
    import concurrent.futures
    pref, _ = TS.small()
    sam_head = TS.expected_header(pref)
    runs = dict(plain=((None,), dict(sam='alone.sam')), b0=(('b0.bam', '--gpu-streams', '1'), {}),
                b1=(('b1.bam', '--gpu-streams', '6', '--gpu-batch', '64'), {}), b2=(('b2.bam', '--gpu-batch', '200'), {}),
                c=(('c.bam',), dict(sam='c.sam')))
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:       # independent processes: four at a time
        futures = {k: pool.submit(run_cli, tmp_path, *a, **kw) for k, (a, kw) in runs.items()}
        got = {k: f.result() for k, f in futures.items()}
    plain, _, sam = got['plain']
    _, records = TB.split_bam(got['c'][1], pref)
    assert got['c'][0] == plain and got['c'][2] == sam                       # stdout and the SAM are unchanged by the flag
    assert records == BC.bam_from(sam[len(sam_head):], list(pref.names)) and len(BC.records_of_bam(records)) > 100
    for k in ('b0', 'b1', 'b2'):
        assert got[k][0] == plain and TB.split_bam(got[k][1], pref)[1] == records, runs[k]


def test_truth_bam_of_two_ranks_on_one_gpu(tmp_path):
    import test_gpu_cli as C
    import test_host_simulate as THS
    pref, _ = TS.small()
    single_fq, single, _ = run_cli(tmp_path, 'single.bam')
    _, records = TB.split_bam(single, pref)
    bam = tmp_path / 'ranks.bam'
    out = C._launch_ranks(tmp_path, 2, ['--truth-bam', str(bam)], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'))
    assert open(out, 'rb').read() == single_fq and TB.split_bam(bam.read_bytes(), pref)[1] == records
    prefix = str(tmp_path / 'shard')
    sbam = str(tmp_path / 'shard.bam')
    C._launch_ranks(tmp_path, 2, ['--output-shards', prefix, '--truth-bam', sbam], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'),
                    out_name='unused.fastq')
    got, _ = THS.reassemble(prefix, 2)
    assert got == single_fq
    names, _ = T.parse_fastq_names(got)
    pos = {n: j for j, n in enumerate(names)}
    recs = []
    for r in range(2):
        _, mine = TB.split_bam(open(f'{sbam}.{r}', 'rb').read(), pref)          # each shard a complete BAM file
        at = 0
        while at < len(mine):
            size = 4 + int.from_bytes(mine[at:at + 4], 'little')
            recs.append(mine[at:at + size])
            at += size
    recs.sort(key=lambda rec: pos[rec[36:72].decode()])                       # stable: a read's records keep their order
    assert b''.join(recs) == records
