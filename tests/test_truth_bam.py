"""
--truth-bam: the truth alignments as BGZF-compressed BAM (brx_emit_bam, badread_amd/csrc/brx_bam.h; brx_bgzf_device,
brx_gzip_dev.h), on the emulated device.

A batch's BAM records are a function of its SAM lines (README, --truth-bam), restated in plain Python in tests/bam_codec.py
(`bam_from`); the device's bytes must equal it, and an independent decoder (`sam_of_bam`) must give the SAM back.  The SAM
itself is checked in tests/test_truth_sam.py.  BGZF: whatever the kernels write must pass a block-by-block walk of the
framing and inflate, CRC and length verified, to the input.  tests/test_gpu_truth_bam.py runs the same checks on the MI355X.
"""
import collections
import ctypes
import gzip
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bam_codec as BC
import emu_engine as EE
import helpers as H
import test_gzip_device as GZ
import test_truth_paf as T
import test_truth_sam as TS

BAM_CASES = ('odd_minus', 'negative_as', 'nm_above_255')


def bam_coverage(sam):
    """What the BAM writer adds to the SAM writer's branches (TS.coverage): an odd SEQ read backwards, a signed tag, a two-byte one."""
    c = collections.Counter()
    for line in sam.decode('latin-1').splitlines():
        f = line.split('\t')
        if int(f[1]) & 4:
            continue
        c['odd_minus'] += bool(int(f[1]) & 16) and len(f[9]) % 2 == 1
        c['negative_as'] += int(f[12][5:]) < 0
        c['nm_above_255'] += int(f[11][5:]) > 255
    return c


def emit_sam_and_bams(eng, seed, n_reads, limits, first=0):
    """One batch: its statistics, its SAM bytes, and (BAM bytes, read offsets) for every max_cigar_ops of `limits`."""
    _, st = eng.simulate_batch(seed, first, n_reads)
    st = st.copy()
    sam = bytes(eng.emit_sam_device(n_reads)[0].cpu().numpy())
    bams = {}
    for limit in limits:
        data, off = eng.emit_bam_device(n_reads, limit)
        bams[limit] = (bytes(data.cpu().numpy()), off)
    assert bytes(eng.emit_sam_device(n_reads)[0].cpu().numpy()) == sam          # brx_emit_bam in between leaves the SAM as it was
    return st, sam, bams


def check_bam(pref, st, sam, bam, off, limit):
    """The two equalities and the offsets of one batch's BAM records."""
    names = list(pref.names)
    assert bam == BC.bam_from(sam, names, limit)
    assert BC.sam_of_bam(bam, names) == sam
    n = len(st)
    assert len(off) == n + 1 and int(off[0]) == 0 and int(off[-1]) == len(bam) and (np.diff(off.astype(np.int64)) >= 0).all()
    live = st['rec_len'] > 0
    assert all(int(off[r + 1]) > int(off[r]) for r in np.flatnonzero(live)) and all(int(off[r + 1]) == int(off[r]) for r in np.flatnonzero(~live))


def check_coverage(sam, wanted):
    cases = TS.coverage(sam)
    cases.update(bam_coverage(sam))
    print('truth_bam_cases', dict(cases))
    assert all(cases[k] >= 1 for k in wanted), dict(cases)


def check_long_cigars(bam, limit):
    """With a small limit the batch shows both forms, and the long one on a primary and on a supplementary record."""
    recs = BC.records_of_bam(bam)
    long_ones = [r for r in recs if any(t[0] == 'CG' for t in r['tags'])]
    assert long_ones and len(long_ones) < len(recs)
    assert all(len(r['cigar']) == 2 and len(r['tags'][-1][2]) > limit for r in long_ones)
    assert all(len(r['cigar']) <= limit for r in recs)
    flags = {r['flag'] & 2048 for r in long_ones}
    print('truth_bam_long_cigars', dict(records=len(recs), long=len(long_ones)))
    assert flags == {0, 2048}


LOW_IDENTITY = dict(frag_mean=900, frag_stdev=300, id_a=6, id_b=5)      # identities around 55 %: NM above 255, records that are one mismatch


def check_batches(make_engine, n_full, n_err, low=(4, 1)):
    """The batch checks, shared with the GPU file: full identity; errorful with the real limit and with a limit of 8; each must show every
    case of the SAM writer.  Reads of 400 bases at 90 % identity show neither an NM above 255 nor a negative AS, whatever the seed, so a
    third batch at LOW_IDENTITY (seed 3, reads [low[0], low[0] + low[1]): read 4 is the witness) shows these two."""
    pref, _ = TS.small()
    eng = H.configure(make_engine(), pref, 'nanopore2023', 'nanopore2023', T.full_identity_params())
    st, sam_full, bams = emit_sam_and_bams(eng, 11, n_full, (65535,))
    check_bam(pref, st, sam_full, *bams[65535], 65535)
    eng = H.configure(make_engine(), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    st, sam_err, bams = emit_sam_and_bams(eng, 5, n_err, (65535, 8))
    check_bam(pref, st, sam_err, *bams[65535], 65535)
    check_bam(pref, st, sam_err, *bams[8], 8)
    check_long_cigars(bams[8][0], 8)
    assert not any(t[0] == 'CG' for r in BC.records_of_bam(bams[65535][0]) for t in r['tags'])
    check_coverage(sam_full, TS.CASES)
    check_coverage(sam_err, TS.CASES + ('odd_minus',))
    eng = H.configure(make_engine(), pref, 'nanopore2023', 'nanopore2023', H.SimParams(**LOW_IDENTITY))
    st, sam_low, bams = emit_sam_and_bams(eng, 3, low[1], (65535, 8), first=low[0])
    check_bam(pref, st, sam_low, *bams[65535], 65535)
    check_bam(pref, st, sam_low, *bams[8], 8)
    check_coverage(sam_low, ('negative_as', 'nm_above_255'))
    return sam_full, sam_err, sam_low


def test_truth_bam_of_a_full_identity_an_errorful_and_a_low_identity_batch():
    check_batches(lambda: EE.EmuEngine(1 << 28), 160, 256)


def test_the_codec_round_trips_what_the_contract_says_about_tags_and_bins():
    assert BC.int_tag('NM', 255) == b'NMC\xff' and BC.int_tag('NM', 256) == b'NMS\x00\x01' and BC.int_tag('NM', 65536) == b'NMI\x00\x00\x01\x00'
    assert BC.int_tag('AS', -128) == b'ASc\x80' and BC.int_tag('AS', -129) == b'ASs\x7f\xff' and BC.int_tag('AS', -32769)[2:3] == b'i'
    assert BC.reg2bin(0, 1) == 4681 and BC.reg2bin(-1, 0) == 4680 and BC.reg2bin(0, 1 << 14) == 4681 and BC.reg2bin(0, (1 << 14) + 1) == 585
    assert BC.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0
    name = '0' * 36
    line = f'{name}\t16\tc\t7\t60\t2S3M1I1D1M1S\t*\t0\t0\tACGTNAca\t!!!!!!!!\tNM:i:300\tAS:i:-5\tCO:Z:x y\n'.encode()
    for limit in (65535, 3):
        assert BC.sam_of_bam(BC.bam_from(line, ['b', 'c'], limit), ['b', 'c']) == line.replace(b'ca\t', b'CA\t')


def test_brx_emit_bam_abi():
    from badread_amd import engine as E
    pref, _ = TS.small()
    eng = EE.EmuEngine(1 << 28)
    H.configure(eng, pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    with pytest.raises(E.BrxError) as ex:                   # BRX_E_STATE: no batch yet
        eng.emit_bam_device(48)
    assert ex.value.code == -6
    get = lambda emit, *a: bytes(emit(48, *a)[0].numpy())
    eng.simulate_batch(21, 0, 48)
    paf, sam = get(eng.emit_paf_device), get(eng.emit_sam_device)
    eng.simulate_batch(21, 0, 48)                            # the same batch again: BAM first, then the others in both orders
    bam = get(eng.emit_bam_device)
    assert get(eng.emit_sam_device) == sam and get(eng.emit_paf_device) == paf and get(eng.emit_bam_device) == bam
    assert get(eng.emit_paf_device) == paf and get(eng.emit_bam_device, 0) == bam and get(eng.emit_sam_device) == sam
    assert bam == BC.bam_from(sam, list(pref.names))
    # a buffer that is too small: BRX_E_OUTPUT, nothing written, and the size to come back with
    got = ctypes.c_size_t(0)
    buf = eng.torch.zeros(64, dtype=eng.torch.uint8)
    assert eng.lib.brx_emit_bam(eng.ctx, 65535, ctypes.c_void_p(buf.data_ptr()), 64, None, ctypes.byref(got), None) == E.E_OUTPUT
    need = int(eng.lib.brx_output_needed(eng.ctx))
    assert need == len(bam) and not buf.any() and got.value == 0
    full = eng.torch.zeros(need, dtype=eng.torch.uint8)
    off = eng.torch.zeros(49, dtype=eng.torch.int64)
    rc = eng.lib.brx_emit_bam(eng.ctx, 65535, ctypes.c_void_p(full.data_ptr()), need, ctypes.c_void_p(off.data_ptr()), ctypes.byref(got), None)
    assert rc == 0 and got.value == need and int(off[-1]) == need and bytes(full.numpy()) == bam
    # a CIGAR field of the long form holds two operations: no smaller limit
    assert eng.lib.brx_emit_bam(eng.ctx, 1, ctypes.c_void_p(full.data_ptr()), need, None, ctypes.byref(got), None) == -1
    assert bytes(full.numpy()) == bam and got.value in (0, need)
    # after brx_sequence_fragments the arena holds something else
    eng.sequence_fragments(3, 0, [np.array([0, 1, 2, 3] * 20, dtype=np.uint8)], [0.9])
    with pytest.raises(E.BrxError) as ex:
        eng.emit_bam_device(48)
    assert ex.value.code == -6


BGZF_CASES = [('fastq', n) for n in (0, 1, 32767, 32768, 32769, 65537, 200001)] + [('bytes', 70000), ('one', 5000), ('skew', 131072)]


def check_bgzf(engine):
    """brx_bgzf_device on text, on bytes that do not compress, on one symbol and on the histogram that forces 15-bit codes (shared
    with the GPU file)."""
    import torch
    from badread_amd import output as O
    for kind, n in BGZF_CASES:
        data = GZ.make_case(kind, n) if n else b''
        src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(engine.device)
        blob = bytes(engine.bgzf_device(src).cpu().numpy())
        payloads = BC.bgzf_blocks(blob)
        assert b''.join(payloads) == data, (kind, n)
        assert len(payloads) == -(-n // 32768) and all(len(p) == 32768 for p in payloads[:-1]), (kind, n)
        assert (gzip.decompress(blob) if blob else b'') == data
        host = O.bgzf_host(data)
        assert b''.join(BC.bgzf_blocks(host)) == data and len(BC.bgzf_blocks(host)) == -(-n // 0xff00)
    assert O.BGZF_EOF == bytes.fromhex('1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00')
    assert BC.bgzf_blocks(O.BGZF_EOF) == [b'']


def test_interpreted_kernels_write_valid_bgzf_blocks():
    check_bgzf(EE.EmuEngine(1 << 26))


def test_the_header_is_the_sam_header_and_the_contigs():
    from badread_amd import output as O
    from badread_amd import simulate as S
    pref, _ = TS.small()
    raw = O.bam_header(pref)
    text = S.sam_header(pref)
    assert raw[:4] == b'BAM\x01' and struct.unpack_from('<i', raw, 4)[0] == len(text) and raw[8:8 + len(text)] == text
    at = 8 + len(text)
    assert struct.unpack_from('<i', raw, at)[0] == len(pref.names)
    at += 4
    for name, length in zip(pref.names, pref.lengths):
        l_name = struct.unpack_from('<i', raw, at)[0]
        assert raw[at + 4:at + 4 + l_name] == name.encode() + b'\0' and struct.unpack_from('<i', raw, at + 4 + l_name)[0] == int(length)
        at += 8 + l_name
    assert at == len(raw)
    # thousands of contigs: several blocks; a contig BAM cannot address: refused
    Many = collections.namedtuple('Many', 'names lengths')
    many = Many([f'contig_{i:05d}' for i in range(6000)], [1000 + i for i in range(6000)])
    big = O.bam_header(many, b'@HD\tVN:1.6\n')
    assert len(BC.bgzf_blocks(O.bgzf_host(big))) == -(-len(big) // 0xff00) > 1 and b''.join(BC.bgzf_blocks(O.bgzf_host(big))) == big
    with pytest.raises(ValueError):
        O.bam_header(Many(['a', 'b'], [5, 2 ** 31]), b'')
    O.bam_header(Many(['a'], [2 ** 31 - 1]), b'')


def split_bam(blob, pref):
    """(header bytes, record bytes) of a complete BAM file: every block checked, the EOF block last and only there."""
    from badread_amd import output as O
    payloads = BC.bgzf_blocks(blob)
    assert blob.endswith(O.BGZF_EOF) and payloads[-1] == b'' and all(payloads[:-1])
    raw, head = b''.join(payloads), O.bam_header(pref)
    assert raw.startswith(head)
    return head, raw[len(head):]


def test_truth_bam_through_the_host_driver(tmp_path, monkeypatch):
    from badread_amd import simulate as S
    pref, _ = TS.small()
    args = dict(quantity='5x', mean_frag_length=300.0, frag_length_stdev=200.0, error_model='nanopore2023', qscore_model='nanopore2023',
                mean_identity=92.0, max_identity=98.0, identity_stdev=3.0, seed=3)
    runs = []
    for max_batch, streams, bam in ((12, 1, False), (12, 1, True), (7, 2, True)):
        monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', max_batch)
        fq = io.BytesIO()
        sam_path, bam_path = str(tmp_path / f'truth{max_batch}{bam}.sam'), str(tmp_path / f'truth{max_batch}.bam')
        got = S.simulate(T._Args(truth_sam=sam_path, truth_bam=bam_path if bam else None, gpu_streams=streams, **args), output=io.StringIO(),
                         engine=EE.EmuEngine(1 << 28), stdout=fq, shard=S.Shard())
        timing = dict(S.run_batches.last_timing)
        runs.append((got, fq.getvalue(), open(sam_path, 'rb').read(), open(bam_path, 'rb').read() if bam else None, timing))
    (base, plain, sam, _, _), with_12, with_7 = runs
    for got, fq, sam_again, _, _ in (with_12, with_7):
        assert got == base and fq == plain and sam_again == sam                # the flag changes neither the FASTQ nor the SAM
    head12, records12 = split_bam(with_12[3], pref)
    head7, records7 = split_bam(with_7[3], pref)
    assert records12 == records7 and len(records12) > 0
    sam_head = TS.expected_header(pref)
    assert records12 == BC.bam_from(sam[len(sam_head):], list(pref.names))
    assert sam_head + BC.sam_of_bam(records12, list(pref.names)) == sam
    # both ways of compressing were taken: whole batches by their workers, the job's last batches by the consumer
    assert with_12[4]['bam_batches_packed_by_their_worker'] >= 1 and with_12[4]['batches'] > with_12[4]['bam_batches_packed_by_their_worker']


def test_a_packed_batch_that_is_cut_after_all_is_unpacked_and_packed_again():
    """_Run.pack_bam on a batch its worker compressed whole, of which the stop rule keeps a prefix."""
    import torch
    from badread_amd import simulate as S
    eng = EE.EmuEngine(1 << 26)
    records = GZ.make_case('fastq', 90000)
    off = np.array([0, 40000, 70001, 90000], dtype=np.uint64)
    whole = eng.bgzf_device(torch.from_numpy(np.frombuffer(records, dtype=np.uint8).copy()))
    run = S._Run.__new__(S._Run)
    run.torch, run.timing, run.gz_engine = torch, collections.Counter(), eng
    assert run.pack_bam((whole, off, True), 3) is whole and run.pack_bam(None, 0) is None
    for keep in (2, 1):
        cut = bytes(run.pack_bam((whole, off, True), keep).numpy())
        assert b''.join(BC.bgzf_blocks(cut)) == records[:int(off[keep])]
    raw = torch.from_numpy(np.frombuffer(records, dtype=np.uint8).copy())
    assert b''.join(BC.bgzf_blocks(bytes(run.pack_bam((raw, off, False), 2).numpy()))) == records[:70001]
    assert int(run.pack_bam((raw, off, False), 0).numel()) == 0


def test_truth_bam_missing_directory_is_an_error(tmp_path):
    r = subprocess.run([sys.executable, '-m', 'badread_amd', 'simulate', '--reference', T.SMALL_REF, '--quantity', '1x',
                        '--truth-bam', str(tmp_path / 'nope' / 'x.bam')], capture_output=True, text=True, cwd=os.path.dirname(T.HERE))
    assert r.returncode == 1 and r.stderr.startswith('Error: ') and 'truth-bam' in r.stderr


def test_truth_bam_needs_the_gpu_engine(tmp_path):
    from badread_amd import simulate as S

    class NoTruth(object):
        pass
    args = T._Args(truth_bam=str(tmp_path / 'x.bam'), quantity='1x', seed=1)
    with pytest.raises(SystemExit) as ex:
        S.open_outputs(args, S.Shard(), NoTruth(), io.BytesIO(), TS.small()[0])
    assert str(ex.value) == 'Error: --truth-bam needs the GPU engine'


def test_the_bam_share_is_counted_into_the_expected_bytes():
    from badread_amd import simulate as S
    assert S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(['bam'])) == int(1000 * (2.1 * 15000.0 + 400.0) * (1.0 + S.BAM_SHARE))
    assert S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(['paf', 'sam', 'bam'])) == int(1000 * (2.1 * 15000.0 + 400.0) * (1.0 + S.PAF_SHARE + S.SAM_SHARE + S.BAM_SHARE))
