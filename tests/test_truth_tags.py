"""
--truth-tags: MD:Z: and SA:Z: on the truth SAM and BAM records (brx_emit_sam_tags / brx_emit_bam_tags, badread_amd/csrc/brx_sam.h,
brx_bam.h), on the emulated device.

The tagged records are a function of the untagged ones and the reference's forward strands (README, "Truth tags"), restated in
plain Python in tests/truth_tags.py; the device's bytes must equal it for every mask, on the two batches of
tests/test_truth_sam.py, which between them must show every branch of the two writers (`tag_cases`).  `check_properties` checks
the tags without that restatement.  tests/test_gpu_truth_tags.py runs the same checks on the MI355X.
"""
import ctypes
import functools
import io

import pytest

import bam_codec as BC
import emu_engine as EE
import helpers as H
import test_truth_paf as T
import test_truth_sam as TS
import truth_tags as TT


def limits_of(tags, limits):
    """Both CIGAR limits with both tags, the first alone with one tag: the long form does not depend on which tags precede CG."""
    return limits if tags == TT.TAG_MD | TT.TAG_SA else limits[:1]


def tagged_batch(eng, seed, n_reads, limits=(65535, 8)):
    """One batch (shared with the GPU file): untagged FASTQ / PAF / SAM (TS.emit_both), the tagged SAM of every mask with its offsets,
    the tagged BAM of every mask and limit; tags = 0 and the untagged emitters before and after must not move."""
    fastq, st, paf, sam, off = TS.emit_both(eng, seed, n_reads)
    got = dict(fastq=fastq, st=st, paf=paf, sam=sam, off=off, tagged={}, bam={})
    for tags in TT.MASKS:
        data, toff = eng.emit_sam_device(n_reads, tags)
        got['tagged'][tags] = (bytes(data.cpu().numpy()), toff)
        for limit in limits_of(tags, limits):
            data, boff = eng.emit_bam_device(n_reads, limit, tags)
            got['bam'][tags, limit] = (bytes(data.cpu().numpy()), boff)
    zero, zoff = eng.emit_sam_device(n_reads, 0)
    assert bytes(zero.cpu().numpy()) == sam and (zoff == off).all()
    assert bytes(eng.emit_paf_device(n_reads)[0].cpu().numpy()).decode() == paf
    return got


def check_exact(batch, ref_of, md_exempt=None):
    """Test 1: every mask's SAM equals the restatement over the same batch's untagged SAM; the read offsets."""
    for tags in TT.MASKS:
        data, off = batch['tagged'][tags]
        exempt = md_exempt(data) if md_exempt is not None and tags & TT.TAG_MD else None
        assert data == TT.tagged_sam_from(batch['sam'], ref_of, tags & TT.TAG_MD, tags & TT.TAG_SA, exempt), tags
        TT.check_offsets(off, data, batch['st'])


def check_bams(batch, names, limits=(65535, 8), long_cigars=True):
    """Test 4: the BAM of every mask is the codec's transform of the tagged SAM (CG behind the new tags), and decodes back to it."""
    for tags in TT.MASKS:
        sam = batch['tagged'][tags][0]
        for limit in limits_of(tags, limits):
            bam, off = batch['bam'][tags, limit]
            assert bam == BC.bam_from(sam, names, limit), (tags, limit)
            assert BC.sam_of_bam(bam, names) == sam
            TT.check_offsets(off, bam, batch['st'])
    if not long_cigars:
        return
    both = BC.records_of_bam(batch['bam'][TT.TAG_MD | TT.TAG_SA, min(limits)][0])
    long_ones = [r for r in both if any(t[0] == 'CG' for t in r['tags'])]
    assert any(t[0] == 'SA' for r in long_ones for t in r['tags'])
    assert long_ones and all(r['tags'][-1][0] == 'CG' and [t[0] for t in r['tags']][:3] == ['NM', 'AS', 'MD'] for r in long_ones)


def check_cases(batch, wanted, label):
    """Test 2: the batch shows every branch it is there for."""
    cases = TT.tag_cases(batch['tagged'][TT.TAG_MD | TT.TAG_SA][0])
    print('truth_tags_cases', label, dict(cases))
    assert all(cases[k] >= 1 for k in wanted), dict(cases)
    return cases


@functools.lru_cache(maxsize=None)
def errorful():
    pref, seqs = TS.small()
    eng = H.configure(EE.EmuEngine(1 << 28), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    return eng, tagged_batch(eng, 5, 256)


@functools.lru_cache(maxsize=None)
def full_identity():
    pref, seqs = TS.small()
    eng = H.configure(EE.EmuEngine(1 << 28), pref, 'nanopore2023', 'nanopore2023', T.full_identity_params())
    return eng, tagged_batch(eng, 11, 160)


@pytest.mark.parametrize('make', [errorful, full_identity])
def test_tagged_sam_equals_the_restatement_for_every_mask(make):
    pref, seqs = TS.small()
    check_exact(make()[1], TT.str_strands(seqs))


def test_the_batches_show_every_branch_of_the_tag_writers():
    cases = check_cases(errorful()[1], TT.ERRORFUL_CASES, 'errorful')
    assert cases['reads_2_lines'] >= 1
    cases = check_cases(full_identity()[1], TT.FULL_CASES, 'full_identity')
    assert cases['max_lines'] >= 4


@pytest.mark.parametrize('make', [errorful, full_identity])
def test_the_tags_hold_their_properties_without_the_restatement(make):
    batch = make()[1]
    TT.check_properties(batch['tagged'][TT.TAG_MD | TT.TAG_SA][0])
    TT.check_properties(batch['tagged'][TT.TAG_MD][0], sa=False)
    TT.check_properties(batch['tagged'][TT.TAG_SA][0], md=False)


@pytest.mark.parametrize('make', [errorful, full_identity])
def test_tagged_bam_is_the_tagged_sam(make):
    pref, _ = TS.small()
    check_bams(make()[1], list(pref.names), long_cigars=make is errorful)


def test_the_restatement_on_a_hand_made_line():
    parts = [(2, 'S'), (3, 'M'), (1, 'I'), (2, 'D'), (2, 'M'), (1, 'S')]
    assert TT.md_of(parts, 'NNACGTTAN', 'ACTGGTC') == '2T0^GG1C0'          # X, then a deletion, a 0 behind a final mismatch
    assert TT.md_of([(3, 'M')], 'CCC', 'ACC') == '0A2' and TT.md_of([(3, 'M')], 'ACC', 'ACC') == '3'
    f = ['r', '2064', 'c1', '7', '60', '2H3M1I2D2M1H', '*', '0', '0', 'ACGTTA', '!!!!!!', 'NM:i:5', 'AS:i:0']
    assert TT.sa_element(f) == 'c1,7,-,2S6M1D1S,60,5;'


def test_brx_emit_tags_abi():
    from badread_amd import engine as E
    assert (E.TAG_MD, E.TAG_SA) == (1, 2)
    pref, _ = TS.small()
    fresh = H.configure(EE.EmuEngine(1 << 24), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    for call in (lambda: fresh.emit_sam_device(48, E.TAG_MD), lambda: fresh.emit_bam_device(48, 65535, E.TAG_SA)):
        with pytest.raises(E.BrxError) as ex:               # BRX_E_STATE: no batch yet
            call()
        assert ex.value.code == -6
    eng, batch = errorful()
    n = len(batch['st'])
    for call in (lambda: eng.emit_sam_device(n, 4), lambda: eng.emit_bam_device(n, 65535, 8 | E.TAG_MD)):
        with pytest.raises(E.BrxError) as ex:               # BRX_E_ARG: a bit that is no tag
            call()
        assert ex.value.code == -1
    # a buffer that is too small: BRX_E_OUTPUT, nothing written, the exact size to come back with; the repeat succeeds
    tags = E.TAG_MD | E.TAG_SA
    for want, emit in ((batch['tagged'][tags][0], lambda *a: eng.lib.brx_emit_sam_tags(eng.ctx, tags, *a)),
                       (batch['bam'][tags, 8][0], lambda *a: eng.lib.brx_emit_bam_tags(eng.ctx, tags, 8, *a))):
        got = ctypes.c_size_t(0)
        buf = eng.torch.zeros(64, dtype=eng.torch.uint8)
        assert emit(ctypes.c_void_p(buf.data_ptr()), 64, None, ctypes.byref(got), None) == E.E_OUTPUT
        need = int(eng.lib.brx_output_needed(eng.ctx))
        assert need == len(want) and not buf.any() and got.value == 0
        full = eng.torch.zeros(need, dtype=eng.torch.uint8)
        off = eng.torch.zeros(n + 1, dtype=eng.torch.int64)
        assert emit(ctypes.c_void_p(full.data_ptr()), need, ctypes.c_void_p(off.data_ptr()), ctypes.byref(got), None) == 0
        assert got.value == need and int(off[-1]) == need and bytes(full.numpy()) == want
    assert bytes(eng.emit_sam_device(n)[0].numpy()) == batch['sam']


def _cli_args(*extra):
    from badread_amd.__main__ import parse_args
    return parse_args(['simulate', '--reference', T.SMALL_REF, '--quantity', '1x'] + list(extra))


@pytest.mark.parametrize('text', ['md', 'MD,', '', 'MD;SA', 'MD, SA', 'NM'])
def test_truth_tags_spelt_otherwise_is_an_error(tmp_path, text, capsys):
    from badread_amd.__main__ import check_simulate_args
    with pytest.raises(SystemExit) as ex:
        check_simulate_args(_cli_args('--truth-sam', str(tmp_path / 'x.sam'), '--truth-tags', text))
    assert ex.value.code == 'Error: --truth-tags must be a comma-separated list of MD and SA'


def test_truth_tags_without_a_file_is_an_error(tmp_path):
    from badread_amd.__main__ import check_simulate_args
    with pytest.raises(SystemExit) as ex:
        check_simulate_args(_cli_args('--truth-tags', 'MD', '--truth-paf', str(tmp_path / 'x.paf')))
    assert ex.value.code == 'Error: --truth-tags needs --truth-sam or --truth-bam'


def test_truth_tags_becomes_the_mask(tmp_path):
    from badread_amd.__main__ import check_simulate_args
    for text, mask in (('MD', 1), ('SA', 2), ('MD,SA', 3), ('SA,MD', 3)):
        args = _cli_args('--truth-bam', str(tmp_path / 'x.bam'), '--truth-tags', text)
        check_simulate_args(args)
        assert args.truth_tags == mask
    args = _cli_args('--truth-bam', str(tmp_path / 'x.bam'))
    check_simulate_args(args)
    assert args.truth_tags == 0


def test_the_first_buffer_counts_the_tags_once_per_file():
    from badread_amd import engine as E
    from badread_amd import simulate as S
    base = 1000 * (2.1 * 15000.0 + 400.0)
    assert S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(['sam'], 3)) == int(base * (1.0 + S.SAM_SHARE + E.MD_SHARE + E.SA_SHARE))
    assert S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(['sam', 'bam'], 1)) == int(base * (1.0 + S.SAM_SHARE + S.BAM_SHARE + 2 * E.MD_SHARE))
    assert S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(['paf'], 3)) == int(base * (1.0 + S.PAF_SHARE))


def test_truth_tags_through_the_host_driver(tmp_path, monkeypatch):
    """simulate() with both files and both tags: the same files whatever the batch size and the streams, FASTQ and PAF untouched, the
    SAM the restatement of the untagged run's, the BAM's blocks the tagged records."""
    from badread_amd import simulate as S
    import test_truth_bam as TB
    pref, seqs = TS.small()
    args = dict(quantity='5x', mean_frag_length=300.0, frag_length_stdev=200.0, error_model='nanopore2023', qscore_model='nanopore2023',
                mean_identity=92.0, max_identity=98.0, identity_stdev=3.0, seed=3)
    monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', 12)
    plain = io.BytesIO()
    plain_sam, plain_paf = str(tmp_path / 'plain.sam'), str(tmp_path / 'plain.paf')
    base = S.simulate(T._Args(truth_sam=plain_sam, truth_paf=plain_paf, **args), output=io.StringIO(), engine=EE.EmuEngine(1 << 28),
                      stdout=plain, shard=S.Shard())
    files = []
    for max_batch, streams in ((12, 1), (7, 2)):
        monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', max_batch)
        fq = io.BytesIO()
        sam_path, bam_path, paf_path = (str(tmp_path / f'tagged{max_batch}.{x}') for x in ('sam', 'bam', 'paf'))
        got = S.simulate(T._Args(truth_sam=sam_path, truth_bam=bam_path, truth_paf=paf_path, truth_tags=3, gpu_streams=streams, **args),
                         output=io.StringIO(), engine=EE.EmuEngine(1 << 28), stdout=fq, shard=S.Shard())
        assert got == base and fq.getvalue() == plain.getvalue()
        assert open(paf_path, 'rb').read() == open(plain_paf, 'rb').read()
        files.append((open(sam_path, 'rb').read(), TB.split_bam(open(bam_path, 'rb').read(), pref)[1]))
    assert files[0] == files[1]
    head = TS.expected_header(pref)
    untagged = open(plain_sam, 'rb').read()
    assert untagged.startswith(head) and files[0][0].startswith(head)
    want = TT.tagged_sam_from(untagged[len(head):], TT.str_strands(seqs), True, True)
    assert files[0][0][len(head):] == want and want != untagged[len(head):]
    assert files[0][1] == BC.bam_from(want, list(pref.names))
