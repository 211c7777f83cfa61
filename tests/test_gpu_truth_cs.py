"""
GPU: --truth-cs and --truth-eqx on the MI355X.  The emulated-device checks of tests/test_truth_cs.py on the HIP engine (PAF and SAM
of every valid fmt equal the plain-Python restatement over the same batch's MD-tagged SAM, the BAM is the codec's transform of the
formatted SAM, the properties, the branches of the writer), the ABI round trip, long reads on the repeat-rich reference, the command
line (files independent of streams and batch sizes, FASTQ unchanged by the options) and two ranks on one GPU.
"""
import collections
import ctypes
import os
import subprocess
import sys

import pytest

import bam_codec as BC
import helpers as H
import test_truth_cs as TG
import test_truth_paf as T
import test_truth_sam as TS
import truth_cs as TC
import truth_tags as TT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BOTH, EQX_CS, EQX_CS_LONG = TG.BOTH, TC.FMT_EQX | TC.FMT_CS, TC.FMT_EQX | TC.FMT_CS | TC.FMT_CS_LONG
_batches = {}


def batch(kind):
    """The two batches of tests/test_gpu_truth_tags.py, each simulated and emitted once for the tests below."""
    if kind not in _batches:
        pref, _ = TS.small()
        params, seed, n = (T.full_identity_params(), 11, 400) if kind == 'full' else (H.SimParams(frag_mean=400, frag_stdev=300), 5, 512)
        eng = H.configure(H.hip_engine(), pref, 'nanopore2023', 'nanopore2023', params)
        _batches[kind] = TG.formatted_batch(eng, seed, n)
    return _batches[kind]


@pytest.mark.parametrize('kind', ['errorful', 'full'])
def test_formatted_paf_sam_and_bam_of_a_batch_on_the_gpu(kind):
    pref, seqs = TS.small()
    b = batch(kind)
    TG.check_exact(b)
    TG.check_bams(b, list(pref.names), eqx_only=kind == 'errorful')
    counts = TG.check_properties(b, TT.str_strands(seqs))
    assert counts['cs_lines'] > 100 and counts['eqx_lines'] > 100


def test_the_batches_show_the_branches_of_the_cs_writer_on_the_gpu():
    TG.check_cases(batch('errorful'), TC.ERRORFUL_CASES, 'errorful')
    cases = TG.check_cases(batch('full'), TC.FULL_CASES, 'full_identity')
    assert cases['not_only_matches'] == 0


def test_brx_emit_fmt_abi_on_the_gpu():
    from badread_amd import engine as E
    pref, _ = TS.small()
    eng = H.configure(H.hip_engine(), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    with pytest.raises(E.BrxError) as ex:                   # BRX_E_STATE: new parameters, no batch since
        eng.emit_paf_device(48, E.FMT_CS)
    assert ex.value.code == -6
    n = 48
    eng.simulate_batch(21, 0, n)
    for call in (lambda: eng.emit_sam_device(n, 0, 8), lambda: eng.emit_bam_device(n, 65535, 0, E.FMT_CS_LONG), lambda: eng.emit_paf_device(n, 4)):
        with pytest.raises(E.BrxError) as ex:               # BRX_E_ARG: an unknown bit, CS_LONG alone
            call()
        assert ex.value.code == -1
    torch = eng.torch
    for want, emit in ((bytes(eng.emit_sam_device(n, BOTH, EQX_CS)[0].cpu().numpy()), lambda *a: eng.lib.brx_emit_sam_fmt(eng.ctx, EQX_CS, BOTH, *a)),
                       (bytes(eng.emit_bam_device(n, 8, BOTH, EQX_CS)[0].cpu().numpy()), lambda *a: eng.lib.brx_emit_bam_fmt(eng.ctx, EQX_CS, BOTH, 8, *a)),
                       (bytes(eng.emit_paf_device(n, EQX_CS_LONG)[0].cpu().numpy()), lambda *a: eng.lib.brx_emit_paf_fmt(eng.ctx, EQX_CS_LONG, *a))):
        assert want.count(b'cs') >= n // 2
        got = ctypes.c_size_t(0)
        buf = torch.zeros(64, dtype=torch.uint8, device=eng.device)
        assert emit(ctypes.c_void_p(buf.data_ptr()), 64, None, ctypes.byref(got), eng._stream()) == E.E_OUTPUT
        need = int(eng.lib.brx_output_needed(eng.ctx))
        assert need == len(want) and not buf.any() and got.value == 0
        full = torch.zeros(need, dtype=torch.uint8, device=eng.device)
        assert emit(ctypes.c_void_p(full.data_ptr()), need, None, ctypes.byref(got), eng._stream()) == 0
        assert got.value == need and bytes(full.cpu().numpy()) == want


def test_truth_cs_of_long_reads_on_the_gpu():
    """--length 15000,13000 on the 3.4 Mb repeat-rich reference: records of tens of thousands of columns, reads of many lines, one
    reference slice with an N.  EQX|CS and EQX|CS|CS_LONG with MD|SA equal the restatement over the batch's MD-tagged SAM (exact in N
    runs: it reads no reference), the BAM is the formatted SAM, and the properties hold against the reference's forward strands."""
    import lowcomplexity as L
    import test_gpu_truth_sam as GS
    eng = L.configure_case(H.hip_engine(), 'default')
    pref = L.packed_reference('large')
    n = 512
    fastq, st, paf, sam, off = TS.emit_both(eng, 7, n)
    md_sam = TG._bytes(eng.emit_sam_device(n, TT.TAG_MD))[0]
    got = {fmt: TG._bytes(eng.emit_sam_device(n, BOTH, fmt)) for fmt in (EQX_CS, EQX_CS_LONG)}
    pafs = {fmt: TG._bytes(eng.emit_paf_device(n, fmt))[0].decode() for fmt in (EQX_CS, EQX_CS_LONG)}
    bam, boff = TG._bytes(eng.emit_bam_device(n, 65535, BOTH, EQX_CS))
    assert TG._bytes(eng.emit_sam_device(n))[0] == sam
    for fmt, (data, foff) in got.items():
        assert data == TC.formatted_sam_from(md_sam, fmt, BOTH), fmt
        TT.check_offsets(foff, data, st)
        assert pafs[fmt] == TC.formatted_paf_from(paf, md_sam, fmt), fmt
    names = list(pref.names)
    assert bam == TC.bam_from(got[EQX_CS][0], names) and TC.sam_of_bam(bam, names) == got[EQX_CS][0]
    TT.check_offsets(boff, bam, st)
    forward, texts = GS._Forward(pref), {}

    def ref_of(name):
        if name not in texts:
            texts[name] = forward(name).tobytes().decode('latin-1')
        return texts[name]

    counts = collections.Counter()
    plain_tagged = TG._bytes(eng.emit_sam_device(n, BOTH))[0]
    for fmt in (EQX_CS, EQX_CS_LONG):
        TC.check_properties(plain_tagged, got[fmt][0], pafs[fmt], fmt, ref_of, counts)
    cases = TC.cs_cases(got[EQX_CS][0])
    print('truth_cs_long_reads', dict(counts), dict(cases), dict(longest=int(st['seq_len'].max()), sam=len(sam), eqx_cs=len(got[EQX_CS][0]),
                                                                  eqx_cs_long=len(got[EQX_CS_LONG][0]), fastq=len(fastq)))
    assert counts['n_lines'] >= 2 and 5 * counts['n_lines'] <= counts['cs_lines']          # two fmts: the line with an N twice
    assert int(st['seq_len'].max()) > 30000 and cases['max_columns'] > 20000 and cases['reads_2_records'] >= 4
    assert cases['ins_run_crosses_step'] >= 1 and cases['del_run_crosses_step'] >= 1          # what the small batches may not show


def run_cli(tmp_path, name, *extra, fmt=('--truth-cs', 'short', '--truth-eqx'), tags='MD,SA'):
    """One command-line run writing NAME.sam, NAME.bam and NAME.paf: (stdout, SAM, BAM, PAF)."""
    cmd = [sys.executable, '-m', 'badread_amd', 'simulate', '--reference', T.SMALL_REF, '--quantity', '40x', '--length', '400,300',
           '--seed', '11', '--truth-sam', str(tmp_path / f'{name}.sam'), '--truth-bam', str(tmp_path / f'{name}.bam'),
           '--truth-paf', str(tmp_path / f'{name}.paf')] + (['--truth-tags', tags] if tags else []) + list(fmt) + list(extra)
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return (r.stdout,) + tuple((tmp_path / f'{name}.{x}').read_bytes() for x in ('sam', 'bam', 'paf'))


def test_truth_cs_and_eqx_from_the_cli(tmp_path):
    import concurrent.futures
    import test_truth_bam as TB
    pref, seqs = TS.small()
    head = TS.expected_header(pref)
    runs = dict(plain=(('plain',), dict(fmt=(), tags='MD')), a=(('a',), {}), b0=(('b0', '--gpu-streams', '1'), {}),
                b1=(('b1', '--gpu-batch', '64'), {}), long=(('long',), dict(fmt=('--truth-cs', 'long'), tags=None)))
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:       # independent processes: four at a time
        futures = {k: pool.submit(run_cli, tmp_path, *a, **kw) for k, (a, kw) in runs.items()}
        got = {k: f.result() for k, f in futures.items()}
    plain, md_sam, _, paf = got['plain']
    fq, sam, bam, paf_a = got['a']
    assert fq == plain and md_sam.startswith(head) and sam.startswith(head)  # the FASTQ is unchanged by the options
    want = TC.formatted_sam_from(md_sam[len(head):], 3, 3)
    assert sam[len(head):] == want and want.count(b'\tcs:Z:') > 100 and want.count(b'\tSA:Z:') > 10
    assert paf_a.decode() == TC.formatted_paf_from(paf.decode(), md_sam[len(head):], 3)
    records = TB.split_bam(bam, pref)[1]                                     # host zlib per BGZF block (BC.bgzf_blocks)
    assert records == TC.bam_from(want, list(pref.names)) and TC.sam_of_bam(records, list(pref.names)) == want
    for k in ('b0', 'b1'):
        assert got[k][0] == plain and got[k][1] == sam and got[k][3] == paf_a, runs[k]
        assert TB.split_bam(got[k][2], pref)[1] == records, runs[k]
    fq, sam, bam, paf_l = got['long']
    want = TC.formatted_sam_from(md_sam[len(head):], 6, 0)
    assert fq == plain and sam[len(head):] == want and paf_l.decode() == TC.formatted_paf_from(paf.decode(), md_sam[len(head):], 6)
    assert TB.split_bam(bam, pref)[1] == TC.bam_from(want, list(pref.names))


def test_truth_cs_and_eqx_of_two_ranks_on_one_gpu(tmp_path):
    import test_gpu_cli as C
    import test_host_simulate as THS
    import test_truth_bam as TB
    pref, _ = TS.small()
    head = TS.expected_header(pref)
    single_fq, single, single_bam, single_paf = run_cli(tmp_path, 'single')
    records = TB.split_bam(single_bam, pref)[1]
    assert single.count(b'\tcs:Z:') > 100
    opts = ['--truth-tags', 'MD,SA', '--truth-cs', 'short', '--truth-eqx']
    prefix, ssam, sbam, spaf = (str(tmp_path / x) for x in ('shard', 'shard.sam', 'shard.bam', 'shard.paf'))
    env = dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0')
    C._launch_ranks(tmp_path, 2, ['--output-shards', prefix, '--truth-sam', ssam, '--truth-bam', sbam, '--truth-paf', spaf] + opts, env,
                    out_name='unused.fastq')
    got, _ = THS.reassemble(prefix, 2)
    assert got == single_fq
    names, _ = T.parse_fastq_names(got)
    pos = {n: j for j, n in enumerate(names)}
    lines, recs, pafs = [], [], []
    for r in range(2):
        data = open(f'{ssam}.{r}', 'rb').read()
        assert data.startswith(head)
        lines += data[len(head):].splitlines(keepends=True)
        pafs += open(f'{spaf}.{r}', 'rb').read().splitlines(keepends=True)
        mine, at = TB.split_bam(open(f'{sbam}.{r}', 'rb').read(), pref)[1], 0          # each shard a complete BAM file
        while at < len(mine):
            size = 4 + int.from_bytes(mine[at:at + 4], 'little')
            recs.append(mine[at:at + size])
            at += size
    lines.sort(key=lambda line: pos[line.split(b'\t')[0].decode()])          # stable: a read's lines keep their order
    pafs.sort(key=lambda line: pos[line.split(b'\t')[0].decode()])
    recs.sort(key=lambda rec: pos[rec[36:72].decode()])
    assert head + b''.join(lines) == single and b''.join(recs) == records and b''.join(pafs) == single_paf
