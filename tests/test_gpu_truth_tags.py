"""
GPU: --truth-tags on the MI355X.  The emulated-device checks of tests/test_truth_tags.py on the HIP engine (every mask's SAM equals
the plain-Python restatement over the same batch's untagged SAM, the BAM is the codec's transform of it, every branch of the two
writers shown), long reads on the repeat-rich reference, the command line (tagged files independent of streams and batch sizes,
FASTQ and PAF unchanged by the option) and two ranks on one GPU.
"""
import collections
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bam_codec as BC
import helpers as H
import test_truth_paf as T
import test_truth_sam as TS
import test_truth_tags as TG
import truth_tags as TT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
_batches = {}


def batch(kind):
    """The two batches of tests/test_gpu_truth_sam.py, each simulated and emitted once for the tests below (everything emitted at once:
    the tests share one engine, which the next configure takes over)."""
    if kind not in _batches:
        pref, _ = TS.small()
        params, seed, n = (T.full_identity_params(), 11, 400) if kind == 'full' else (H.SimParams(frag_mean=400, frag_stdev=300), 5, 512)
        eng = H.configure(H.hip_engine(), pref, 'nanopore2023', 'nanopore2023', params)
        _batches[kind] = TG.tagged_batch(eng, seed, n)
    return _batches[kind]


@pytest.mark.parametrize('kind', ['errorful', 'full'])
def test_tagged_sam_and_bam_of_a_batch_on_the_gpu(kind):
    pref, seqs = TS.small()
    b = batch(kind)
    TG.check_exact(b, TT.str_strands(seqs))
    TG.check_bams(b, list(pref.names), long_cigars=kind == 'errorful')
    TT.check_properties(b['tagged'][TT.TAG_MD | TT.TAG_SA][0])
    TT.check_properties(b['tagged'][TT.TAG_MD][0], sa=False)
    TT.check_properties(b['tagged'][TT.TAG_SA][0], md=False)


def test_the_batches_show_every_branch_of_the_tag_writers_on_the_gpu():
    TG.check_cases(batch('errorful'), TT.ERRORFUL_CASES, 'errorful')
    cases = TG.check_cases(batch('full'), TT.FULL_CASES, 'full_identity')
    assert cases['max_lines'] >= 4


def test_brx_emit_tags_abi_on_the_gpu():
    import ctypes
    from badread_amd import engine as E
    pref, _ = TS.small()
    eng = H.configure(H.hip_engine(), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    with pytest.raises(E.BrxError) as ex:                   # BRX_E_STATE: new parameters, no batch since
        eng.emit_sam_device(48, E.TAG_MD | E.TAG_SA)
    assert ex.value.code == -6
    n = 48
    eng.simulate_batch(21, 0, n)
    with pytest.raises(E.BrxError) as ex:                   # BRX_E_ARG: a bit that is no tag
        eng.emit_bam_device(n, 65535, 4)
    assert ex.value.code == -1
    tags, torch = E.TAG_MD | E.TAG_SA, eng.torch
    want = bytes(eng.emit_sam_device(n, tags)[0].cpu().numpy())
    assert want.count(b'\tSA:Z:') >= 2 and want.count(b'\tMD:Z:') >= n // 2
    got = ctypes.c_size_t(0)
    buf = torch.zeros(64, dtype=torch.uint8, device=eng.device)
    assert eng.lib.brx_emit_sam_tags(eng.ctx, tags, ctypes.c_void_p(buf.data_ptr()), 64, None, ctypes.byref(got), eng._stream()) == E.E_OUTPUT
    need = int(eng.lib.brx_output_needed(eng.ctx))
    assert need == len(want) and not buf.any() and got.value == 0
    full = torch.zeros(need, dtype=torch.uint8, device=eng.device)
    assert eng.lib.brx_emit_sam_tags(eng.ctx, tags, ctypes.c_void_p(full.data_ptr()), need, None, ctypes.byref(got), eng._stream()) == 0
    assert got.value == need and bytes(full.cpu().numpy()) == want


def test_truth_tags_of_long_reads_on_the_gpu():
    """--length 15000,13000 on the 3.4 Mb repeat-rich reference: MD texts of many 64-column steps, reads of many lines.  A line whose
    reference slice holds an N is checked by its properties (TT.md_properties) instead of the exact MD, as TS.check_invariants skips
    such a line's NM; every other line, and every SA, is exact."""
    import lowcomplexity as L
    import test_gpu_truth_sam as GS
    eng = L.configure_case(H.hip_engine(), 'default')
    pref = L.packed_reference('large')
    n = 512
    b = TG.tagged_batch(eng, 7, n, limits=(65535,))
    forward, texts = GS._Forward(pref), {}

    def ref_of(name):
        if name not in texts:
            texts[name] = forward(name).tobytes().decode('latin-1')
        return texts[name]

    stats = collections.Counter()

    def exempt(tagged):
        """line index -> the device's MD, for the mapped lines whose reference slice holds an N (their properties checked here)."""
        out = {}
        want = TT.tagged_sam_from(b['sam'], ref_of, True, False).decode('latin-1').splitlines()
        for i, line in enumerate(tagged.decode('latin-1').splitlines()):
            f = line.split('\t')
            if int(f[1]) & 4:
                continue
            stats['mapped'] += 1
            span = sum(int(x) for x, op in re.findall(r'(\d+)([MIDSH])', f[5]) if op in 'MD')
            if 'N' in ref_of(f[2])[int(f[3]) - 1:int(f[3]) - 1 + span]:
                TT.md_properties(f)
                out[i] = TT._tag(f, 'MD')
                stats['n_lines'] += 1
                stats['n_lines_exact'] += 'MD:Z:' + out[i] in want[i].split('\t')
        return out

    TG.check_exact(b, ref_of, md_exempt=exempt)
    both = b['tagged'][TT.TAG_MD | TT.TAG_SA][0]
    TT.check_properties(both)
    TG.check_bams(b, list(pref.names), limits=(65535,), long_cigars=False)
    cases = TT.tag_cases(both)
    mapped, n_lines = stats['mapped'] // 2, stats['n_lines'] // 2          # two of the three masks carry MD
    print('truth_tags_long_reads', dict(mapped=mapped, n_lines=n_lines, n_lines_exact=stats['n_lines_exact'] // 2,
                                        longest=int(b['st']['seq_len'].max()), most_lines=cases['max_lines'], longest_md=cases['md_max_len'],
                                        tagged=len(both), untagged=len(b['sam']), fastq=len(b['fastq'])))
    assert 5 * n_lines <= mapped
    assert int(b['st']['seq_len'].max()) > 30000 and cases['max_lines'] >= 4 and cases['md_max_len'] > 4096


def run_cli(tmp_path, name, *extra, tags='MD,SA'):
    """One command-line run writing NAME.sam, NAME.bam and NAME.paf: (stdout, SAM, BAM, PAF)."""
    cmd = [sys.executable, '-m', 'badread_amd', 'simulate', '--reference', T.SMALL_REF, '--quantity', '40x', '--length', '400,300',
           '--seed', '11', '--truth-sam', str(tmp_path / f'{name}.sam'), '--truth-bam', str(tmp_path / f'{name}.bam'),
           '--truth-paf', str(tmp_path / f'{name}.paf')] + (['--truth-tags', tags] if tags else []) + list(extra)
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return (r.stdout,) + tuple((tmp_path / f'{name}.{x}').read_bytes() for x in ('sam', 'bam', 'paf'))


def test_truth_tags_from_the_cli(tmp_path):
    import concurrent.futures
    import test_truth_bam as TB
    pref, seqs = TS.small()
    head = TS.expected_header(pref)
    runs = dict(plain=(('plain',), dict(tags=None)), a=(('a',), {}), b0=(('b0', '--gpu-streams', '1'), {}),
                b1=(('b1', '--gpu-batch', '64'), {}), b2=(('b2', '--gpu-batch', '200'), {}))
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:       # independent processes: four at a time
        futures = {k: pool.submit(run_cli, tmp_path, *a, **kw) for k, (a, kw) in runs.items()}
        got = {k: f.result() for k, f in futures.items()}
    plain, untagged, _, paf = got['plain']
    fq, sam, bam, paf_a = got['a']
    assert fq == plain and paf_a == paf                                      # FASTQ and PAF are unchanged by the option
    assert untagged.startswith(head) and sam.startswith(head)
    want = TT.tagged_sam_from(untagged[len(head):], TT.str_strands(seqs), True, True)
    assert sam[len(head):] == want and want.count(b'\tSA:Z:') > 10 and want.count(b'\tMD:Z:') > 100
    records = TB.split_bam(bam, pref)[1]                                     # host zlib per BGZF block (BC.bgzf_blocks)
    assert records == BC.bam_from(want, list(pref.names)) and BC.sam_of_bam(records, list(pref.names)) == want
    for k in ('b0', 'b1', 'b2'):
        assert got[k][0] == plain and got[k][1] == sam and got[k][3] == paf, runs[k]
        assert TB.split_bam(got[k][2], pref)[1] == records, runs[k]


def test_truth_tags_of_two_ranks_on_one_gpu(tmp_path):
    import test_gpu_cli as C
    import test_host_simulate as THS
    import test_truth_bam as TB
    pref, _ = TS.small()
    head = TS.expected_header(pref)
    single_fq, single, single_bam, _ = run_cli(tmp_path, 'single')
    records = TB.split_bam(single_bam, pref)[1]
    sam, bam = tmp_path / 'ranks.sam', tmp_path / 'ranks.bam'
    env = dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0')
    out = C._launch_ranks(tmp_path, 2, ['--truth-sam', str(sam), '--truth-bam', str(bam), '--truth-tags', 'MD,SA'], env)
    assert open(out, 'rb').read() == single_fq and sam.read_bytes() == single and TB.split_bam(bam.read_bytes(), pref)[1] == records
    prefix, ssam, sbam = str(tmp_path / 'shard'), str(tmp_path / 'shard.sam'), str(tmp_path / 'shard.bam')
    C._launch_ranks(tmp_path, 2, ['--output-shards', prefix, '--truth-sam', ssam, '--truth-bam', sbam, '--truth-tags', 'MD,SA'], env,
                    out_name='unused.fastq')
    got, _ = THS.reassemble(prefix, 2)
    assert got == single_fq
    names, _ = T.parse_fastq_names(got)
    pos = {n: j for j, n in enumerate(names)}
    lines, recs = [], []
    for r in range(2):
        data = open(f'{ssam}.{r}', 'rb').read()
        assert data.startswith(head)
        lines += data[len(head):].splitlines(keepends=True)
        mine, at = TB.split_bam(open(f'{sbam}.{r}', 'rb').read(), pref)[1], 0          # each shard a complete BAM file
        while at < len(mine):
            size = 4 + int.from_bytes(mine[at:at + 4], 'little')
            recs.append(mine[at:at + size])
            at += size
    lines.sort(key=lambda line: pos[line.split(b'\t')[0].decode()])          # stable: a read's lines keep their order
    recs.sort(key=lambda rec: pos[rec[36:72].decode()])
    assert head + b''.join(lines) == single and b''.join(recs) == records
