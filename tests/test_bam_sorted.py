"""
--truth-bam-sorted: the truth BAM in coordinate order with its BAI index (brx_bam_sort, brx_bgzf_device_off, brx_bam_index:
badread_amd/csrc/brx_bamsort.h), on the emulated device, and the host driver around them.

The contract is restated in plain Python in tests/bam_sorted.py: the stable sort of the decoded records, the bytes of the index from the
sorted file's own blocks, and a reader that answers region queries through an index as the standard reader does.  The device's bytes
must equal the restatement's, and the reader must answer every query of a fixed set as brute force does.
tests/test_gpu_bam_sorted.py runs the same bodies on the MI355X.
"""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bam_codec as BC
import bam_sorted as BS
import emu_engine as EE
import helpers as H
import test_truth_bam as TB
import test_truth_paf as T
import test_truth_sam as TS


@pytest.fixture(scope='module')
def eng():
    return EE.EmuEngine(1 << 26)


def test_the_reader_finds_what_brute_force_finds_through_the_restated_index():
    BS.self_check()


def test_the_restatement_on_a_table_worked_out_by_hand():
    names = BS.names_of(2)
    lines = [BS.line(0, 1, 5, '10M', names=names), BS.line(1, None, 0, l_seq=3), BS.line(2, 0, 16383, '2M', names=names),
             BS.line(3, 0, 16383, '1M', names=names), BS.line(4, 0, 7, '3M2D1I4M', names=names)]
    raw, off = BS.raw_of(lines, names)
    recs = BS.split(raw)
    want = recs[4] + recs[2] + recs[3] + recs[0] + recs[1]              # contig 0 by position, ties in input order, contig 1, unmapped
    assert BS.sort_records(raw) == want
    table = BS.table_of(want)
    assert [BS.reflen(r) for r in recs] == [10, 1, 2, 1, 9]
    assert table['refID'].tolist() == [0, 0, 0, 1, -1] and table['pos'].tolist() == [7, 16383, 16383, 5, -1]
    assert table['end'].tolist() == [16, 16385, 16384, 15, 0] and table['bin'].tolist() == [4681, 585, 4681, 4681, 4680]
    assert table['off'].tolist() == [0] + np.cumsum([len(recs[i]) for i in (4, 2, 3, 0)]).tolist()
    blob, block_off = BS.python_blocks(want)
    whole, base = BS.file_of(blob, names, [40000, 100])
    bai = BS.bai_of(whole)
    v = [(base << 16) | int(x) for x in table['off']] + [(base + len(blob)) << 16]
    # contig 0: bin 585 with one chunk, bin 4681 with two (the run is cut by the record of bin 585); two windows
    c0 = struct.pack('<i', 2) + struct.pack('<IiQQ', 585, 1, v[1], v[2]) + struct.pack('<IiQQQQ', 4681, 2, v[0], v[1], v[2], v[3]) + struct.pack('<iQQ', 2, v[0], v[1])
    c1 = struct.pack('<i', 1) + struct.pack('<IiQQ', 4681, 1, v[3], v[4]) + struct.pack('<iQ', 1, v[3])
    assert bai == b'BAI\1' + struct.pack('<i', 2) + c0 + c1 + struct.pack('<Q', 1)
    assert BS.Reader(bai, BS.File(whole)).query(0, 16384, 16385) == [1]


def test_the_record_set_of_sizes_straddles_spans_and_lanes():
    BS.check_sizes_case_is_what_it_says()


@pytest.mark.parametrize('case', BS.sort_cases(), ids=lambda c: c[0])
def test_sort_and_gather_equal_the_stable_sort(eng, case):
    BS.check_sort_case(eng, case)


@pytest.mark.parametrize('case', BS.grid_cases(), ids=lambda c: c[0])
def test_the_blocks_hold_32768_bytes_and_the_offsets_walk_them(eng, case):
    BS.check_grid_case(eng, case)


@pytest.mark.parametrize('case', BS.index_cases(), ids=lambda c: c[0])
def test_the_index_equals_the_restatement_and_answers_queries(eng, case):
    BS.check_index_case(eng, case)


def test_brx_bam_sort_abi(eng):
    BS.check_sort_abi(eng)


def test_brx_bam_index_abi(eng):
    BS.check_index_abi(eng)


def test_the_records_of_simulated_batches_sorted():
    BS.check_batches(lambda: EE.EmuEngine(1 << 28), 24, 40)


# ---- host ------------------------------------------------------------------------------------------------------------------------------
ARGS = dict(quantity='5x', mean_frag_length=300.0, frag_length_stdev=200.0, error_model='nanopore2023', qscore_model='nanopore2023',
            mean_identity=92.0, max_identity=98.0, identity_stdev=3.0, seed=3)


def test_truth_bam_sorted_through_the_host_driver(tmp_path, monkeypatch):
    """simulate() with --truth-bam-sorted beside --truth-bam and alone: both files the same whatever the batch size and the streams, FASTQ,
    --truth-bam and return value those of the run without it, the records the stable sort of --truth-bam's, the index the restatement."""
    from badread_amd import simulate as S
    pref, _ = TS.small()
    runs = []
    for i, (max_batch, streams, bam, ordered) in enumerate(((12, 1, True, False), (12, 1, True, True), (7, 2, False, True))):
        monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', max_batch)
        fq = io.BytesIO()
        bam_path, sorted_path = str(tmp_path / f'u{i}.bam'), str(tmp_path / f's{i}.bam')
        got = S.simulate(T._Args(truth_bam=bam_path if bam else None, truth_bam_sorted=sorted_path if ordered else None, gpu_streams=streams, **ARGS),
                         output=io.StringIO(), engine=EE.EmuEngine(1 << 28), stdout=fq, shard=S.Shard())
        read = lambda path, on: open(path, 'rb').read() if on else None
        runs.append((got, fq.getvalue(), read(bam_path, bam), read(sorted_path, ordered), read(sorted_path + '.bai', ordered)))
        assert os.path.exists(sorted_path) == os.path.exists(sorted_path + '.bai') == ordered
    base, both, alone = runs
    assert both[:2] == base[:2] == alone[:2]
    _, records = TB.split_bam(base[2], pref)
    assert TB.split_bam(both[2], pref)[1] == records and len(BS.split(records)) > 20       # --truth-bam's records do not depend on the option
    BS.check_file_pair(both[3], both[4], pref, records)
    assert alone[3:] == both[3:]


def test_the_sink_finds_its_frames_however_the_bytes_were_cut(tmp_path):
    import torch
    from badread_amd import simulate as S
    names = BS.names_of(1)
    raw_a, off_a = BS.raw_of([BS.line(i, 0, 50 - i, l_seq=3 + i, names=names) for i in range(5)], names)
    raw_b, off_b = BS.raw_of([BS.line(9, 0, 7, names=names)], names)
    off_a = np.insert(off_a, 2, off_a[2])                                       # a read without a record
    parts = [S.sorted_frame(torch, (torch.from_numpy(np.frombuffer(r, dtype=np.uint8).copy()), o, False), keep)
             for r, o, keep in ((raw_a, off_a, 6), (raw_b, off_b, 1), (raw_a, off_a, 2))]
    assert S.sorted_frame(torch, None, 3) is None and S.sorted_frame(torch, (None, off_a, False), 0) is None
    whole = b''.join(bytes(p.numpy()) for p in parts)
    for cuts in ((), (1,), (24, 25, 100), tuple(range(0, len(whole), 7))):
        sink = S._SortedBamFile(str(tmp_path / 'x.bam'), TS.small()[0])
        for a, b in zip((0,) + cuts, cuts + (len(whole),)):
            sink.write(memoryview(whole[a:b]))
        lens, pieces = sink.frames()
        assert lens.tolist() == np.diff(off_a.astype(np.int64)).tolist() + [len(raw_b)] + np.diff(off_a[:3].astype(np.int64)).tolist()
        assert b''.join(bytes(p) for p in pieces) == raw_a + raw_b + raw_a[:int(off_a[2])]
    with pytest.raises(OSError):
        S._SortedBamFile(str(tmp_path / 'nope' / 'x.bam'), TS.small()[0])


def test_a_job_that_does_not_fit_the_device_says_so_and_writes_neither_file(tmp_path, monkeypatch):
    from badread_amd import simulate as S
    monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', 12)
    eng = EE.EmuEngine(1 << 28)

    def no_room(*a, **k):
        raise MemoryError
    eng.bam_sort = no_room
    path = str(tmp_path / 's.bam')
    with pytest.raises(SystemExit) as ex:
        S.simulate(T._Args(truth_bam_sorted=path, **ARGS), output=io.StringIO(), engine=eng, stdout=io.BytesIO(), shard=S.Shard())
    import re
    assert re.fullmatch(r'Error: --truth-bam-sorted: \d+ records \(\d+\.\d GB\) need \d+\.\d GB on the device', str(ex.value.code)), ex.value.code
    assert int(str(ex.value.code).split()[2]) > 20
    assert not os.path.exists(path) and not os.path.exists(path + '.bai')
    # a failure after the first file was begun takes it away again
    eng = EE.EmuEngine(1 << 28)

    def broken(*a, **k):
        raise RuntimeError('the index failed')
    eng.bam_index = broken
    with pytest.raises(RuntimeError):
        S.simulate(T._Args(truth_bam_sorted=path, **ARGS), output=io.StringIO(), engine=eng, stdout=io.BytesIO(), shard=S.Shard())
    assert not os.path.exists(path) and not os.path.exists(path + '.bai')


def test_truth_bam_sorted_missing_directory_is_an_error(tmp_path):
    r = subprocess.run([sys.executable, '-m', 'badread_amd', 'simulate', '--reference', T.SMALL_REF, '--quantity', '1x',
                        '--truth-bam-sorted', str(tmp_path / 'nope' / 'x.bam')], capture_output=True, text=True, cwd=os.path.dirname(T.HERE))
    assert r.returncode == 1 and r.stderr.startswith('Error: ') and 'truth-bam-sorted' in r.stderr and 'does not exist' in r.stderr


class _FakeRef(object):
    def __init__(self, names, lengths):
        self.names, self.lengths = names, lengths


def test_what_open_outputs_refuses(tmp_path):
    from badread_amd import simulate as S

    class NoTruth(object):
        pass
    args = T._Args(truth_bam_sorted=str(tmp_path / 'x.bam'), quantity='1x', seed=1)
    with pytest.raises(SystemExit) as ex:
        S.open_outputs(args, S.Shard(), NoTruth(), io.BytesIO(), TS.small()[0])
    assert str(ex.value) == 'Error: --truth-bam-sorted needs the GPU engine'
    with pytest.raises(SystemExit) as ex:
        S.open_outputs(args, S.Shard(), H.oracle_engine(), io.BytesIO(), TS.small()[0])
    assert str(ex.value) == 'Error: --truth-bam-sorted needs the GPU engine'
    eng = EE.EmuEngine(1 << 20)
    with pytest.raises(SystemExit) as ex:
        S.open_outputs(args, S.Shard(), eng, io.BytesIO(), _FakeRef(['a', 'b'], [5, 2 ** 29]))
    assert str(ex.value) == 'Error: --truth-bam-sorted: contig b is too long for a BAI index'
    with pytest.raises(SystemExit) as ex:                                      # as --truth-bam refuses it
        S.open_outputs(args, S.Shard(), eng, io.BytesIO(), _FakeRef(['a', 'b'], [2 ** 31, 5]))
    with pytest.raises(SystemExit) as ex_bam:
        S.open_outputs(T._Args(truth_bam=str(tmp_path / 'y.bam'), quantity='1x', seed=1), S.Shard(), eng, io.BytesIO(), _FakeRef(['a', 'b'], [2 ** 31, 5]))
    assert str(ex.value) == str(ex_bam.value).replace('--truth-bam', '--truth-bam-sorted') and 'contig a' in str(ex.value)
    outs = S.open_outputs(args, S.Shard(), eng, io.BytesIO(), _FakeRef(['a', 'b'], [5, 2 ** 29 - 1]))
    assert outs.sorted_bam is not None and outs.truth_write['bam_sorted'] == outs.sorted_bam.write and not os.path.exists(args.truth_bam_sorted)
    outs.close()


def _cli_args(*extra):
    from badread_amd.__main__ import parse_args
    return parse_args(['simulate', '--reference', T.SMALL_REF, '--quantity', '1x'] + list(extra))


def test_the_option_alone_with_tags_and_formats_passes_the_argument_check(tmp_path, capsys):
    from badread_amd import engine as E
    from badread_amd import simulate as S
    from badread_amd.__main__ import check_simulate_args, parse_args
    args = _cli_args('--truth-bam-sorted', str(tmp_path / 'x.bam'), '--truth-tags', 'MD,SA', '--truth-cs', 'short', '--truth-eqx')
    check_simulate_args(args)
    spec = S.TruthSpec.from_args(args)
    assert spec == (('bam_sorted',), E.TAG_MD | E.TAG_SA, E.FMT_EQX | E.FMT_CS)
    assert spec.share() == pytest.approx(E.BAM_SHARE + E.MD_SHARE + E.SA_SHARE + E.EQX_SHARE['bam'] + E.CS_SHORT_SHARE['bam'])
    assert S.TruthSpec(('depth', 'bam_sorted', 'bam', 'paf')).kinds == ('paf', 'bam', 'bam_sorted', 'depth')
    assert S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(['bam_sorted'])) == int(1000 * (2.1 * 15000.0 + 400.0) * (1.0 + S.BAM_SHARE))
    with pytest.raises(SystemExit):
        parse_args(['simulate', '--help'])
    assert '--truth-bam-sorted PATH' in capsys.readouterr().out
    readme = open(os.path.join(os.path.dirname(T.HERE), 'README.md')).read()
    assert '--truth-bam-sorted PATH' in readme.split('\n## ')[0] and '\n## Sorted truth BAM with its index (`--truth-bam-sorted PATH`)\n' in readme


def test_a_worker_emits_the_bam_records_once_for_both_files():
    import torch
    from badread_amd import simulate as S
    calls = []

    class Eng(object):
        stats_dtype = np.dtype([('x', 'u4')])

        def simulate_batch(self, seed, first, n, allow_nofrag=True):
            return np.zeros(4, dtype=np.uint8), np.zeros(n, dtype=self.stats_dtype)

        def emit_truth_device(self, kind, n, tags=0, fmt=0, max_cigar_ops=65535):
            calls.append(kind)
            return torch.tensor(list(kind.encode()), dtype=torch.uint8), np.array([0, 1, 3], dtype=np.uint64)

        def bgzf_device(self, data):
            return torch.cat([torch.tensor([31, 139], dtype=torch.uint8), data])
    pool = S._BatchPool(Eng(), 1, truth=S.TruthSpec(('bam', 'bam_sorted', 'paf')))
    truth = pool.submit(1, 0, 2, pack=True).result().truth
    assert calls == ['paf', 'bam'] and list(truth) == ['paf', 'bam', 'bam_sorted']
    assert bytes(truth['bam'][0].numpy()) == b'\x1f\x8bbam' and truth['bam'][2] is True
    assert bytes(truth['bam_sorted'][0].numpy()) == b'bam' and truth['bam_sorted'][2] is False
    pool.close()
    calls.clear()
    pool = S._BatchPool(Eng(), 1, truth=S.TruthSpec(('bam_sorted',)))
    assert bytes(pool.submit(1, 0, 2).result().truth['bam_sorted'][0].numpy()) == b'bam' and calls == ['bam']
    pool.close()
