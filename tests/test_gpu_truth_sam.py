"""
GPU: --truth-sam on the MI355X.  The emulated-device checks of tests/test_truth_sam.py on the HIP engine (the SAM equals the
plain-Python transform of the batch's FASTQ and PAF, byte for byte, with every branch of the writer shown by the batch), long
reads on the repeat-rich reference, the command line (SAM independent of streams and batch sizes, FASTQ and PAF unchanged by
the flag) and two ranks on one GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import test_truth_paf as T
import test_truth_sam as TS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_truth_sam_of_a_full_identity_batch_on_the_gpu():
    pref, seqs = TS.small()
    eng = H.configure(H.hip_engine(), pref, 'nanopore2023', 'nanopore2023', T.full_identity_params())
    TS.check_batch(eng, pref, seqs, 11, 400)


def test_truth_sam_of_an_errorful_batch_on_the_gpu():
    pref, seqs = TS.small()
    eng = H.configure(H.hip_engine(), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    TS.check_batch(eng, pref, seqs, 5, 512)


class _Forward(object):
    """A contig's forward strand by name, decoded from the packed reference when first asked for."""

    def __init__(self, pref):
        import test_gpu_truth_paf as G
        self.packed, self.pref, self.seen = G._PackedSeq(pref), pref, {}
        self.index = {n: j for j, n in enumerate(pref.names)}

    def __call__(self, name):
        if name not in self.seen:
            j = self.index[name]
            self.seen[name] = self.packed.target(j, 0, int(self.pref.lengths[j]), False)
        return self.seen[name]


def test_truth_sam_of_long_reads_on_the_gpu():
    """--length 15000,13000 on the 3.4 Mb repeat-rich reference: many 64-column steps and records per read, several routes of the
    final alignment, read offsets far past one 64-read group."""
    import lowcomplexity as L
    eng = L.configure_case(H.hip_engine(), 'default')
    pref = L.packed_reference('large')
    n = 512
    fastq, st, paf, sam, off = TS.emit_both(eng, 7, n)
    assert sam == TS.sam_from(fastq, paf, pref.sym, pref.comp)
    assert len(off) == n + 1 and int(off[0]) == 0 and int(off[-1]) == len(sam) and (np.diff(off.astype(np.int64)) >= 0).all()
    n_lines, n_reads = TS.check_invariants(sam, _Forward(pref), int((st['rec_len'] > 0).sum()))
    per_read = np.array([sam[int(off[r]):int(off[r + 1])].count(b'\n') for r in range(n)])
    print('truth_sam_long_reads', dict(lines=n_lines, reads=n_reads, longest=int(st['seq_len'].max()), most_lines=int(per_read.max()),
                                       sam_bytes=len(sam), fastq_bytes=len(fastq)))
    assert int(st['seq_len'].max()) > 30000 and int(per_read.max()) >= 4


def run_cli(tmp_path, name, *extra, paf=None):
    sam = tmp_path / (name or 'unused.sam')
    cmd = [sys.executable, '-m', 'badread_amd', 'simulate', '--reference', T.SMALL_REF, '--quantity', '40x', '--length', '400,300',
           '--seed', '11'] + list(extra)
    if name:
        cmd += ['--truth-sam', str(sam)]
    if paf:
        cmd += ['--truth-paf', str(tmp_path / paf)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, (sam.read_bytes() if name else None), ((tmp_path / paf).read_bytes() if paf else None)


def test_truth_sam_from_the_cli(tmp_path):
    import concurrent.futures
    pref, seqs = TS.small()
    head = TS.expected_header(pref)
    runs = dict(plain=((None,), {}), paf_alone=((None,), dict(paf='alone.paf')), a=(('a.sam',), {}),
                b0=(('b0.sam', '--gpu-streams', '1'), {}), b1=(('b1.sam', '--gpu-streams', '6', '--gpu-batch', '64'), {}),
                b2=(('b2.sam', '--gpu-batch', '200'), {}), c=(('c.sam',), dict(paf='c.paf')))
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:       # independent processes: four at a time
        futures = {k: pool.submit(run_cli, tmp_path, *a, **kw) for k, (a, kw) in runs.items()}
        got = {k: f.result() for k, f in futures.items()}
    plain, sam = got['plain'][0], got['a'][1]
    assert got['a'][0] == plain and sam.startswith(head) and sam.count(b'\n') > 100
    for k in ('b0', 'b1', 'b2'):
        assert got[k][0] == plain and got[k][1] == sam, runs[k]
    fq3, sam3, paf3 = got['c']
    assert fq3 == plain and sam3 == sam and paf3 == got['paf_alone'][2]
    assert head + TS.sam_from(plain, paf3.decode(), pref.sym, pref.comp) == sam
    names, _ = T.parse_fastq_names(plain)
    TS.check_invariants(sam[len(head):], TS.forward_strands(seqs), len(names))


def test_truth_sam_of_two_ranks_on_one_gpu(tmp_path):
    import test_gpu_cli as C
    import test_host_simulate as THS
    pref, _ = TS.small()
    head = TS.expected_header(pref)
    single_fq, single, _ = run_cli(tmp_path, 'single.sam')
    sam = tmp_path / 'ranks.sam'
    out = C._launch_ranks(tmp_path, 2, ['--truth-sam', str(sam)], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'))
    assert open(out, 'rb').read() == single_fq and sam.read_bytes() == single
    prefix = str(tmp_path / 'shard')
    ssam = str(tmp_path / 'shard.sam')
    C._launch_ranks(tmp_path, 2, ['--output-shards', prefix, '--truth-sam', ssam], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'),
                    out_name='unused.fastq')
    got, _ = THS.reassemble(prefix, 2)
    assert got == single_fq
    names, _ = T.parse_fastq_names(got)
    pos = {n: j for j, n in enumerate(names)}
    lines = []
    for r in range(2):
        data = open(f'{ssam}.{r}', 'rb').read()
        assert data.startswith(head)
        lines += data[len(head):].splitlines(keepends=True)
    lines.sort(key=lambda line: pos[line.split(b'\t')[0].decode()])          # stable: a read's lines keep their order
    assert head + b''.join(lines) == single
