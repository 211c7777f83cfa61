"""
--truth-depth: the true coverage of the reference as bedGraph (brx_emit_depth, brx_depth_bedgraph, badread_amd/csrc/brx_depth.h), on the
emulated device.

The file is a function of the job's PAF records (README, "True coverage"), restated in plain Python in tests/truth_depth.py.  On the two
batches of tests/test_truth_tags.py at the sizes of its GPU file, the device's events must be the end points of the same batch's PAF
records and its text the restatement's; on synthetic events over a three-contig reference (lengths 1, 300 and 70 000) the text must be
the restatement's at every count around the borders of the kernels' tiles and for every mix of intervals below.
tests/test_gpu_truth_depth.py runs the same checks on the MI355X.
"""
import ctypes
import functools
import io

import numpy as np
import pytest

import emu_engine as EE
import helpers as H
import test_truth_paf as T
import test_truth_sam as TS
import truth_depth as TD

SYN_NAMES, SYN_LENGTHS = ('one', 'mid', 'long'), (1, 300, 70000)
OWN_KEYS = 4 * len(SYN_NAMES)          # the keys brx_depth_bedgraph adds to the events: four per contig


def tile():
    from badread_amd import engine as E
    return E.DEPTH_TILE


def counts(t):
    """Event counts around the tile borders of the sort and scan kernels: of the events themselves and of the events with the library's own keys."""
    return sorted({0, 2, t - 2, t, t + 2, 3 * t + 6, t - 2 - OWN_KEYS, t - OWN_KEYS, t + 2 - OWN_KEYS})


def synthetic_reference():
    from badread_amd.reference import PackedReference
    import collections
    rng = np.random.default_rng(3)
    seqs = collections.OrderedDict((n, H.random_dna(rng, l)) for n, l in zip(SYN_NAMES, SYN_LENGTHS))
    flat = {n: False for n in seqs}
    return PackedReference.from_seqs(seqs, {n: 1.0 for n in seqs}, dict(flat), dict(flat), dict(flat))


MIXES = ('identical', 'abutting', 'whole', 'nested', 'uniform', 'one_digit')


def synthetic_events(mix, n_events, seed, empty_mid=False):
    """n_events events (n_events / 2 intervals) of one mix on the synthetic reference, shuffled; `empty_mid` keeps the middle contig free."""
    rng = np.random.default_rng(seed)
    n = n_events // 2
    ivs = []
    if mix == 'identical':                      # one change point up, one down, depth n
        ivs = [(2, 1234, 50001)] * n
    elif mix == 'abutting':                     # end == the next start: the depth stays 1 over the chain
        c, step = (2, 7) if empty_mid or n > 100 else (1, 2)
        ivs = [(c, 5 + step * i, 5 + step * (i + 1)) for i in range(n)]
    elif mix == 'whole':                        # from 0 to the contig's length
        cs = [0, 2] if empty_mid else [0, 1, 2]
        ivs = [(c, 0, SYN_LENGTHS[c]) for c in (cs[i % len(cs)] for i in range(n))]
    elif mix == 'nested':                       # a stack: every interval inside the one before, then the same stack again
        c, L = (2, 70000) if empty_mid else (1, 300)
        ivs = [(c, i % (L // 2), L - i % (L // 2)) for i in range(n)]
    elif mix == 'uniform':
        for _ in range(n):
            c = int(rng.choice([0, 2] if empty_mid else [0, 1, 2], p=[0.05, 0.95] if empty_mid else [0.05, 0.25, 0.7]))
            s = int(rng.integers(0, SYN_LENGTHS[c]))
            ivs.append((c, s, int(rng.integers(s + 1, SYN_LENGTHS[c] + 1))))
    elif mix == 'one_digit':                    # the start keys differ in their second byte alone, the end keys not at all
        ivs = [(2, 128 * (i % 256), 65536) for i in range(n)]
    ev = np.array([TD.event(c, p, st) for c, s, e in ivs for p, st in ((s, 1), (e, 0))], dtype=np.uint64)
    assert len(ev) == n_events
    return rng.permutation(ev)


def bedgraph_of(eng, events, cap=None):
    import torch
    ev = torch.from_numpy(np.ascontiguousarray(events, dtype=np.uint64).view(np.int64).copy()).to(eng.device)
    return bytes(eng.depth_bedgraph(ev, cap).cpu().numpy()).decode()


def check_synthetic(eng, n_events, mixes=MIXES):
    """brx_depth_bedgraph == bedgraph_from_events for every mix at this count, the middle contig empty in every other case."""
    for j, mix in enumerate(mixes):
        empty_mid = (j + n_events // 2) % 2 == 1
        ev = synthetic_events(mix, n_events, 100 + j, empty_mid)
        got = bedgraph_of(eng, ev)
        assert got == TD.bedgraph_from_events(ev, SYN_NAMES, SYN_LENGTHS), (mix, n_events)
        TD.check_bedgraph(got, SYN_NAMES, SYN_LENGTHS)
        if empty_mid:
            assert 'mid\t0\t300\t0\n' in got
    return eng.depth_last()[0]


def depth_batch(eng, seed, n_reads):
    """One batch (shared with the GPU file): FASTQ, PAF and SAM (TS.emit_both), then the events, then PAF and SAM again, which must not
    have moved: the events are emitted behind the first pair and before the second."""
    fastq, st, paf, sam, off = TS.emit_both(eng, seed, n_reads)
    data, eoff = eng.emit_truth_device('depth', n_reads)
    ev = np.frombuffer(bytes(data.cpu().numpy()), dtype='<u8')
    paf2, paf_off = eng.emit_paf_device(n_reads)
    assert bytes(paf2.cpu().numpy()).decode() == paf
    sam2, off2 = eng.emit_sam_device(n_reads)
    assert bytes(sam2.cpu().numpy()) == sam and (off2 == off).all()
    return dict(fastq=fastq, st=st, paf=paf, events=ev, off=eoff, paf_off=paf_off)


def check_batch(eng, batch, pref):
    """The events are the end points of the batch's PAF records, read by read; their text is the restatement's, in any order of the events."""
    names, paf, ev, off = list(pref.names), batch['paf'], batch['events'], batch['off']
    assert (ev == TD.events_from_paf(paf, names)).all() and len(ev) == 2 * paf.count('\n') and len(ev) > 200
    assert len(off) == len(batch['st']) + 1 and int(off[0]) == 0 and int(off[-1]) == 8 * len(ev) and (np.diff(off.astype(np.int64)) >= 0).all()
    # a read's events are those of its own PAF lines
    lines_before = np.array([paf[:int(o)].count('\n') for o in batch['paf_off'][::16]])
    assert (off[::16].astype(np.int64) == 16 * lines_before).all()
    want = TD.bedgraph_from_paf(paf, names, pref.lengths)
    got = bedgraph_of(eng, ev)
    assert got == want
    TD.check_bedgraph(got, names, pref.lengths, paf)
    assert bedgraph_of(eng, np.random.default_rng(1).permutation(ev)) == want
    assert bedgraph_of(eng, ev[::-1].copy()) == want
    return got


def check_abi(eng, fresh, batch, n_reads, pref):
    """BRX_E_STATE without a batch; BRX_E_OUTPUT on 64 bytes with nothing written and the exact size, then success, for both entries;
    BRX_E_ARG of brx_depth_bedgraph with the buffer untouched."""
    from badread_amd import engine as E
    torch = eng.torch
    with pytest.raises(E.BrxError) as ex:
        fresh.emit_truth_device('depth', 48)
    assert ex.value.code == -6
    got = ctypes.c_size_t(0)
    want = batch['events'].tobytes()
    buf = torch.zeros(64, dtype=torch.uint8, device=eng.device)
    stream = eng._stream()
    assert eng.lib.brx_emit_depth(eng.ctx, ctypes.c_void_p(buf.data_ptr()), 64, None, ctypes.byref(got), stream) == E.E_OUTPUT
    need = int(eng.lib.brx_output_needed(eng.ctx))
    assert need == len(want) and not buf.any() and got.value == 0
    full = torch.zeros(need, dtype=torch.uint8, device=eng.device)
    off = torch.zeros(n_reads + 1, dtype=torch.int64, device=eng.device)
    assert eng.lib.brx_emit_depth(eng.ctx, ctypes.c_void_p(full.data_ptr()), need, ctypes.c_void_p(off.data_ptr()), ctypes.byref(got), stream) == 0
    assert got.value == need and int(off[-1]) == need and bytes(full.cpu().numpy()) == want
    # the text: a short buffer, then the exact one
    ev = torch.from_numpy(batch['events'].view(np.int64).copy()).to(eng.device)
    scratch = torch.empty(int(eng.lib.brx_depth_bedgraph_scratch(len(ev))), dtype=torch.uint8, device=eng.device)

    def text_into(events, n, out):
        return eng.lib.brx_depth_bedgraph(eng.ctx, ctypes.c_void_p(events.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(got),
                                          ctypes.c_void_p(scratch.data_ptr()), scratch.numel(), stream)
    text = TD.bedgraph_from_paf(batch['paf'], list(pref.names), pref.lengths).encode()
    assert text_into(ev, len(ev), buf) == E.E_OUTPUT
    assert int(eng.lib.brx_output_needed(eng.ctx)) == len(text) and not buf.any() and got.value == 0
    exact = torch.zeros(len(text), dtype=torch.uint8, device=eng.device)
    assert text_into(ev, len(ev), exact) == 0 and got.value == len(text) and bytes(exact.cpu().numpy()) == text
    # bad events: BRX_E_ARG, nothing written
    n_contigs, last = len(pref.names), len(pref.names) - 1
    L = int(pref.lengths[last])
    good = [TD.event(last, 2, 1), TD.event(last, 9, 0)]
    for label, events, n in (('odd count', good + [TD.event(last, 3, 1)], 3),
                             ('contig = n_contigs', good + [TD.event(n_contigs, 0, 1), TD.event(n_contigs, 1, 0)], 4),
                             ('position = length + 1', good + [TD.event(last, 1, 1), TD.event(last, L + 1, 0)], 4),
                             ('end before start', good + [TD.event(last, 20, 0), TD.event(last, 25, 1)], 4),
                             ('unmatched start', good + [TD.event(last, 4, 1), TD.event(last, 5, 1)], 4)):
        out = torch.zeros(4096, dtype=torch.uint8, device=eng.device)
        bad = torch.from_numpy(np.array(events, dtype=np.uint64).view(np.int64)).to(eng.device)
        assert text_into(bad, n, out) == -1, label
        assert not out.any() and got.value == 0, label
    out = torch.zeros(4096, dtype=torch.uint8, device=eng.device)
    assert text_into(torch.from_numpy(np.array(good, dtype=np.uint64).view(np.int64)).to(eng.device), 2, out) == 0 and got.value > 0


@functools.lru_cache(maxsize=None)
def errorful():
    pref, seqs = TS.small()
    eng = H.configure(EE.EmuEngine(1 << 28), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    return eng, depth_batch(eng, 5, 512)


@functools.lru_cache(maxsize=None)
def full_identity():
    pref, seqs = TS.small()
    eng = H.configure(EE.EmuEngine(1 << 28), pref, 'nanopore2023', 'nanopore2023', T.full_identity_params())
    return eng, depth_batch(eng, 11, 400)


@functools.lru_cache(maxsize=None)
def synthetic_engine():
    eng = EE.EmuEngine(1 << 20)
    eng.set_reference(synthetic_reference())
    return eng


@pytest.mark.parametrize('make', [errorful, full_identity])
def test_events_and_bedgraph_of_a_batch_equal_the_restatement(make):
    pref, _ = TS.small()
    eng, batch = make()
    text = check_batch(eng, batch, pref)
    passes = eng.depth_last()[0]
    print('truth_depth_sort_passes small_ref', passes)
    assert 2 <= passes <= 3
    assert text.startswith('circ_chrom\t0\t') and text.splitlines()[-1].startswith('tiny\t') and text.splitlines()[-1].split('\t')[2] == '31'


@pytest.mark.parametrize('n_events', counts(1024))
def test_bedgraph_of_synthetic_events_at_the_tile_borders(n_events):
    assert tile() == 1024
    passes = check_synthetic(synthetic_engine(), n_events)
    print('truth_depth_sort_passes synthetic', passes)
    assert passes < 8


def test_no_events_give_one_zero_line_per_contig():
    assert bedgraph_of(synthetic_engine(), np.zeros(0, dtype=np.uint64)) == 'one\t0\t1\t0\nmid\t0\t300\t0\nlong\t0\t70000\t0\n'


def test_the_restatement_on_hand_made_intervals():
    names, lengths = ('a', 'b'), (10, 4)
    paf = ''.join('\t'.join(['q', '9', '0', '5', '+', n, str(l), str(s), str(e), '5', '5', '60']) + '\n'
                  for n, l, s, e in (('a', 10, 2, 6), ('a', 10, 6, 8), ('a', 10, 3, 5), ('a', 10, 0, 1)))
    text = TD.bedgraph_from_paf(paf, names, lengths)
    assert text == 'a\t0\t1\t1\na\t1\t2\t0\na\t2\t3\t1\na\t3\t5\t2\na\t5\t8\t1\na\t8\t10\t0\nb\t0\t4\t0\n'
    assert TD.check_bedgraph(text, names, lengths, paf) == 9
    assert (TD.per_base(text, names, lengths)['a'] == [1, 0, 1, 2, 2, 1, 1, 1, 0, 0]).all()
    with pytest.raises(AssertionError):
        TD.check_bedgraph(text.replace('a\t5\t8\t1\n', 'a\t5\t7\t1\na\t7\t8\t1\n'), names, lengths)


def test_brx_depth_abi():
    pref, _ = TS.small()
    fresh = H.configure(EE.EmuEngine(1 << 24), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    eng, batch = errorful()
    check_abi(eng, fresh, batch, len(batch['st']), pref)


# ---- host ------------------------------------------------------------------------------------------------------------------------------
def _cli_args(*extra):
    from badread_amd.__main__ import parse_args
    return parse_args(['simulate', '--reference', T.SMALL_REF, '--quantity', '1x'] + list(extra))


def test_truth_depth_alone_passes_the_argument_check(tmp_path):
    from badread_amd.__main__ import check_simulate_args
    from badread_amd import simulate as S
    args = _cli_args('--truth-depth', str(tmp_path / 'x.bedgraph'))
    check_simulate_args(args)
    assert args.truth_depth.endswith('x.bedgraph') and args.truth_tags == 0 and args.truth_fmt == 0
    assert S.TruthSpec.from_args(args).kinds == ('depth',)
    with pytest.raises(SystemExit) as ex:
        check_simulate_args(_cli_args('--truth-depth', str(tmp_path / 'nope' / 'x')))
    assert 'truth-depth' in ex.value.code and 'does not exist' in ex.value.code


def test_the_other_truth_options_still_need_a_file_of_records(tmp_path):
    from badread_amd.__main__ import check_simulate_args
    for extra, flag, files in ((('--truth-cs', 'short'), '--truth-cs', '--truth-paf, --truth-sam or --truth-bam'),
                               (('--truth-eqx',), '--truth-eqx', '--truth-paf, --truth-sam or --truth-bam'),
                               (('--truth-tags', 'MD'), '--truth-tags', '--truth-sam or --truth-bam')):
        with pytest.raises(SystemExit) as ex:
            check_simulate_args(_cli_args('--truth-depth', str(tmp_path / 'x'), *extra))
        assert ex.value.code == f'Error: {flag} needs {files}'


def test_the_spec_puts_depth_last_with_its_own_share_only():
    from badread_amd import engine as E
    from badread_amd import simulate as S
    assert E.TRUTH_KINDS[-1] == 'depth' and E.TRUTH_SHARE['depth'] == E.DEPTH_SHARE
    # 16 bytes per record, the records per FASTQ byte of profiles/truth_paf.md
    assert 16 * 161766 / 1981458140 < E.DEPTH_SHARE < 2 * 16 * 161766 / 1981458140
    spec = S.TruthSpec.from_args(T._Args(truth_depth='d', truth_sam='s', truth_paf='p', truth_tags=3, truth_fmt=3))
    assert spec.kinds == ('paf', 'sam', 'depth')
    without = S.TruthSpec(('paf', 'sam'), 3, 3)
    assert spec.share() == pytest.approx(without.share() + E.DEPTH_SHARE)
    assert S.TruthSpec(('depth',), 3, 7).share() == E.DEPTH_SHARE == S.TruthSpec(('depth',)).share()
    base = 1000 * (2.1 * 15000.0 + 400.0)
    assert S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(('depth',), 3, 7)) == pytest.approx(base * (1.0 + E.DEPTH_SHARE), abs=1.5)


class _FakeRef(object):
    def __init__(self, names, lengths):
        self.names, self.lengths = names, lengths


def test_a_reference_an_event_cannot_hold_is_refused(tmp_path):
    from badread_amd import simulate as S
    assert S.depth_limits(_FakeRef(['a', 'b'], [2 ** 39 - 1, 5])) is None
    assert 'contig b' in S.depth_limits(_FakeRef(['a', 'b'], [5, 2 ** 39]))
    assert '2^24' in S.depth_limits(_FakeRef(range(2 ** 24), [1] * 2 ** 24))
    args = T._Args(truth_depth=str(tmp_path / 'x.bedgraph'))
    with pytest.raises(SystemExit) as ex:
        S.open_outputs(args, S.Shard(), synthetic_engine(), io.BytesIO(), _FakeRef(['a', 'b'], [5, 2 ** 39]))
    assert ex.value.code.startswith('Error: --truth-depth: contig b')
    with pytest.raises(SystemExit) as ex:                      # an engine without the device entry points
        S.open_outputs(args, S.Shard(), H.oracle_engine(), io.BytesIO(), _FakeRef(['a'], [5]))
    assert ex.value.code == 'Error: --truth-depth needs the GPU engine'


def test_the_option_is_in_the_help_and_the_readme(capsys):
    import os
    from badread_amd.__main__ import parse_args
    with pytest.raises(SystemExit):
        parse_args(['simulate', '--help'])
    assert '--truth-depth PATH' in capsys.readouterr().out
    readme = open(os.path.join(os.path.dirname(TS.__file__), '..', 'README.md')).read()
    assert '--truth-depth PATH' in readme.split('\n## ')[0] and '\n## True coverage (`--truth-depth PATH`)\n' in readme


def test_truth_depth_through_the_host_driver(tmp_path, monkeypatch):
    """simulate() with --truth-depth alone and beside --truth-paf: the same file whatever the batch size and the streams, FASTQ, PAF and
    return value those of the run without it, the file the restatement of that run's PAF; gzip of the same text with a --gzip level."""
    import gzip
    from badread_amd import simulate as S
    pref, _ = TS.small()
    args = dict(quantity='5x', mean_frag_length=300.0, frag_length_stdev=200.0, error_model='nanopore2023', qscore_model='nanopore2023',
                mean_identity=92.0, max_identity=98.0, identity_stdev=3.0, seed=3)
    monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', 12)
    plain, plain_paf = io.BytesIO(), str(tmp_path / 'plain.paf')
    base = S.simulate(T._Args(truth_paf=plain_paf, **args), output=io.StringIO(), engine=EE.EmuEngine(1 << 28), stdout=plain, shard=S.Shard())
    want = TD.bedgraph_from_paf(open(plain_paf).read(), list(pref.names), pref.lengths)
    for i, (max_batch, streams, extra) in enumerate(((12, 1, {}), (7, 2, dict(truth_paf=str(tmp_path / 'b.paf'))), (12, 2, dict(gzip_level=1)))):
        monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', max_batch)
        fq, path = io.BytesIO(), str(tmp_path / f'd{i}.bedgraph')
        got = S.simulate(T._Args(truth_depth=path, gpu_streams=streams, **extra, **args), output=io.StringIO(), engine=EE.EmuEngine(1 << 28),
                         stdout=fq, shard=S.Shard())
        assert got == base
        data = open(path, 'rb').read()
        if 'gzip_level' in extra:
            assert gzip.decompress(fq.getvalue()) == plain.getvalue() and data[:2] == b'\x1f\x8b' and gzip.decompress(data).decode() == want
        else:
            assert fq.getvalue() == plain.getvalue() and data.decode() == want
        if 'truth_paf' in extra:
            assert open(extra['truth_paf'], 'rb').read() == open(plain_paf, 'rb').read()
    TD.check_bedgraph(want, list(pref.names), pref.lengths, open(plain_paf).read())
