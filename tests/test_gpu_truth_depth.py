"""
GPU: --truth-depth on the MI355X.  The emulated-device checks of tests/test_truth_depth.py on the HIP engine (the events are the end points
of the same batch's PAF records, the text is the plain-Python restatement's for the batches and for synthetic events around the tile
borders and at 200 000 events), long reads on the repeat-rich reference, the command line (the file independent of streams and batch
sizes, FASTQ and PAF unchanged by the option, gzip with --gzip) and two ranks on one GPU.
"""
import gzip
import os

import numpy as np
import pytest

import helpers as H
import test_gpu_truth_paf as GP
import test_truth_depth as TDT
import test_truth_paf as T
import test_truth_sam as TS
import truth_depth as TD

pytestmark = pytest.mark.gpu
_batches = {}


def batch(kind):
    """The two batches of tests/test_gpu_truth_tags.py, each simulated and emitted once."""
    if kind not in _batches:
        pref, _ = TS.small()
        params, seed, n = (T.full_identity_params(), 11, 400) if kind == 'full' else (H.SimParams(frag_mean=400, frag_stdev=300), 5, 512)
        eng = H.configure(H.hip_engine(), pref, 'nanopore2023', 'nanopore2023', params)
        _batches[kind] = (TDT.depth_batch(eng, seed, n), n)
    return _batches[kind]


@pytest.mark.parametrize('kind', ['errorful', 'full'])
def test_events_and_bedgraph_of_a_batch_on_the_gpu(kind):
    pref, _ = TS.small()
    b, n = batch(kind)
    eng = H.hip_engine()
    eng.set_reference(pref)
    TDT.check_batch(eng, b, pref)
    assert 2 <= eng.depth_last()[0] <= 3


def test_bedgraph_of_synthetic_events_on_the_gpu():
    eng = H.hip_engine()
    eng.set_reference(TDT.synthetic_reference())
    for n_events in TDT.counts(TDT.tile()):
        assert TDT.check_synthetic(eng, n_events) < 8
    assert TDT.bedgraph_of(eng, np.zeros(0, dtype=np.uint64)) == 'one\t0\t1\t0\nmid\t0\t300\t0\nlong\t0\t70000\t0\n'
    # many tiles, and a depth of six digits: 100 000 identical intervals
    TDT.check_synthetic(eng, 200000, mixes=('identical', 'whole', 'nested', 'uniform', 'one_digit'))
    text = TDT.bedgraph_of(eng, TDT.synthetic_events('identical', 200000, 1))
    assert text == 'one\t0\t1\t0\nmid\t0\t300\t0\nlong\t0\t1234\t0\nlong\t1234\t50001\t100000\nlong\t50001\t70000\t0\n'


def test_brx_depth_abi_on_the_gpu():
    pref, _ = TS.small()
    b, n = batch('errorful')
    eng = H.configure(H.hip_engine(), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    eng.simulate_batch(5, 0, n)                          # the batch of `b` again: another test may have used the engine since
    fresh = eng.clone(1 << 20)
    try:
        TDT.check_abi(eng, fresh, b, n, pref)
    finally:
        fresh.close()


def test_long_reads_on_the_repeat_rich_reference():
    import lowcomplexity as LC
    eng = LC.configure_case(H.hip_engine(), 'default')
    pref = LC.packed_reference('large')
    n = 512
    eng.simulate_batch_device(3, 0, n)
    paf = bytes(eng.emit_paf_device(n)[0].cpu().numpy()).decode()
    data, off = eng.emit_truth_device('depth', n)
    ev = np.frombuffer(bytes(data.cpu().numpy()), dtype='<u8')
    names = list(pref.names)
    assert (ev == TD.events_from_paf(paf, names)).all() and len(ev) >= 2 * 400 and int(off[-1]) == 8 * len(ev)
    got = TDT.bedgraph_of(eng, ev)
    assert got == TD.bedgraph_from_paf(paf, names, pref.lengths)
    covered = TD.check_bedgraph(got, names, pref.lengths, paf)
    assert covered > 2_000_000 and max(r[3] for r in TD.parse_bedgraph(got)) >= 3
    assert TDT.bedgraph_of(eng, np.random.default_rng(2).permutation(ev)) == got


def test_truth_depth_from_the_cli(tmp_path):
    pref, _ = TS.small()
    names = list(pref.names)
    depth = lambda name: ['--truth-depth', str(tmp_path / name)]
    read = lambda name: (tmp_path / name).read_bytes()
    plain, plain_paf = GP.run_cli(tmp_path, 'plain.paf')
    fq, paf = GP.run_cli(tmp_path, 'a.paf', *depth('a.bedgraph'))
    assert fq == plain and paf == plain_paf
    want = TD.bedgraph_from_paf(paf.decode(), names, pref.lengths)
    assert read('a.bedgraph').decode() == want
    TD.check_bedgraph(want, names, pref.lengths, paf.decode())
    fq, _ = GP.run_cli(tmp_path, None, '--gpu-streams', '1', '--gpu-batch', '64', *depth('b.bedgraph'))       # the option alone
    assert fq == plain and read('b.bedgraph').decode() == want
    fq, _ = GP.run_cli(tmp_path, None, '--gpu-streams', '3', '--gzip', '1', *depth('c.bedgraph.gz'))
    assert gzip.decompress(fq) == plain and gzip.decompress(read('c.bedgraph.gz')).decode() == want and read('c.bedgraph.gz')[:2] == b'\x1f\x8b'


def test_truth_depth_of_two_ranks_on_one_gpu(tmp_path):
    import test_gpu_cli as C
    pref, _ = TS.small()
    names = list(pref.names)
    single_fq, _ = GP.run_cli(tmp_path, None, '--truth-depth', str(tmp_path / 'single.bedgraph'), quantity='40x')
    single = (tmp_path / 'single.bedgraph').read_text()
    path = tmp_path / 'ranks.bedgraph'
    out = C._launch_ranks(tmp_path, 2, ['--truth-depth', str(path)], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'))
    assert open(out, 'rb').read() == single_fq and path.read_text() == single
    prefix, spath = str(tmp_path / 'shard'), str(tmp_path / 'shard.bedgraph')
    C._launch_ranks(tmp_path, 2, ['--output-shards', prefix, '--truth-depth', spath], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'),
                    out_name='unused.fastq')
    parts = [open(f'{spath}.{r}').read() for r in range(2)]
    total = TD.per_base(single, names, pref.lengths)
    for text in parts:
        assert TD.check_bedgraph(text, names, pref.lengths) > 0
    mine = [TD.per_base(text, names, pref.lengths) for text in parts]
    for name in names:
        assert (mine[0][name] + mine[1][name] == total[name]).all(), name
    assert not os.path.exists(spath)
