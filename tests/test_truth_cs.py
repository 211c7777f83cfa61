"""
--truth-cs / --truth-eqx: cs:Z: and =/X CIGARs on the truth PAF, SAM and BAM (brx_emit_paf_fmt / brx_emit_sam_fmt / brx_emit_bam_fmt,
badread_amd/csrc/brx_paf.h, brx_sam.h, brx_bam.h), on the emulated device.

A line's cs and =/X CIGAR are functions of its CIGAR, MD and SEQ (README, "Truth cs and =/X"), restated in plain Python in
tests/truth_cs.py; the device's bytes must equal that restatement over the same batch's MD-tagged SAM for every valid fmt, on the two
batches of tests/test_truth_tags.py, which must show the branches of the writer that `cs_cases` counts.  `check_properties` checks the
files without the restatement.  tests/test_gpu_truth_cs.py runs the same checks on the MI355X.
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
import truth_cs as TC
import truth_tags as TT

BOTH = TT.TAG_MD | TT.TAG_SA
BAM_FMT = TC.FMT_EQX | TC.FMT_CS


def _bytes(pair):
    return bytes(pair[0].cpu().numpy()), pair[1]


def ops_counts(md_sam):
    """Per mapped line of an MD-tagged SAM: (CIGAR operations as written, operations of its =/X form), clips included."""
    out = []
    for f in TC._fields(md_sam):
        if not int(f[1]) & 4:
            out.append((len(TC.parts_of(f[5])), len(TC.parts_of(TC.eqx_of(f[5], f[13][5:], f[9])))))
    return out


def eqx_only_limit(md_sam):
    """A max_cigar_ops at which some line is long only in its =/X form: M-form operations <= L < =/X-form operations; None if no line
    allows one.  The smallest such L of the batch."""
    fits = [m for m, e in ops_counts(md_sam) if 2 <= m < e]
    return min(fits) if fits else None


def formatted_batch(eng, seed, n_reads, limits=(65535, 8)):
    """One batch (shared with the GPU file): untagged FASTQ / PAF / SAM (TS.emit_both), the SAM with MD (the oracle's input), the PAF
    and SAM of every valid fmt with tags 0, of the two tagged fmts with MD|SA, the BAM of EQX|CS with MD|SA at every limit and at the
    limit that only =/X lines exceed; fmt = 0 through the new functions and the old emitters before and after must not move."""
    fastq, st, paf, sam, off = TS.emit_both(eng, seed, n_reads)
    got = dict(fastq=fastq, st=st, paf=paf, sam=sam, off=off, fsam={}, fpaf={}, bam={})
    got['md_sam'] = _bytes(eng.emit_sam_device(n_reads, TT.TAG_MD))[0]
    for fmt in TC.FMTS[1:]:
        got['fpaf'][fmt] = _bytes(eng.emit_paf_device(n_reads, fmt))
        got['fsam'][fmt, 0] = _bytes(eng.emit_sam_device(n_reads, 0, fmt))
    for fmt in TC.TAGGED_FMTS:
        got['fsam'][fmt, BOTH] = _bytes(eng.emit_sam_device(n_reads, BOTH, fmt))
    got['limit'] = eqx_only_limit(got['md_sam'])
    for limit in tuple(limits) + ((got['limit'],) if got['limit'] else ()):
        got['bam'][limit] = _bytes(eng.emit_bam_device(n_reads, limit, BOTH, BAM_FMT))
    # fmt = 0 through the new functions: the bytes of the old ones
    zero = {}
    for name, emit in (('paf', lambda ctx, *a: eng.lib.brx_emit_paf_fmt(ctx, 0, *a)), ('sam', lambda ctx, *a: eng.lib.brx_emit_sam_fmt(ctx, 0, 0, *a)),
                       ('md_sam', lambda ctx, *a: eng.lib.brx_emit_sam_fmt(ctx, 0, TT.TAG_MD, *a)),
                       ('bam8', lambda ctx, *a: eng.lib.brx_emit_bam_fmt(ctx, 0, BOTH, 8, *a))):
        zero[name] = _bytes(eng._emit_truth(emit, 2.0, n_reads))
    assert zero['paf'][0].decode() == paf and zero['sam'][0] == sam and (zero['sam'][1] == off).all() and zero['md_sam'][0] == got['md_sam']
    assert zero['bam8'][0] == _bytes(eng.emit_bam_device(n_reads, 8, BOTH))[0]
    assert _bytes(eng.emit_sam_device(n_reads))[0] == sam and _bytes(eng.emit_paf_device(n_reads))[0].decode() == paf
    return got


def check_exact(batch):
    """Test 1: PAF and SAM of every fmt equal the restatement over the batch's MD-tagged SAM; the read offsets."""
    for fmt in TC.FMTS[1:]:
        data, off = batch['fpaf'][fmt]
        assert data.decode() == TC.formatted_paf_from(batch['paf'], batch['md_sam'], fmt), fmt
        assert len(off) == len(batch['st']) + 1 and int(off[0]) == 0 and int(off[-1]) == len(data)      # a live read may have no record
    for (fmt, tags), (data, off) in batch['fsam'].items():
        assert data == TC.formatted_sam_from(batch['md_sam'], fmt, tags), (fmt, tags)
        TT.check_offsets(off, data, batch['st'])
    assert TC.formatted_sam_from(batch['md_sam'], 0, 0) == batch['sam'] and TC.formatted_paf_from(batch['paf'], batch['md_sam'], 0) == batch['paf']


def check_bams(batch, names, limits=(65535, 8), eqx_only=True):
    """Test 2: the BAM is the codec's transform of the formatted SAM at every limit and decodes back to it; at the searched limit a
    record is long whose M form would not be; long records end ... MD cs SA ... CG."""
    sam = batch['fsam'][BAM_FMT, BOTH][0]
    for limit, (bam, off) in batch['bam'].items():
        assert bam == TC.bam_from(sam, names, limit), limit
        assert TC.sam_of_bam(bam, names) == sam
        TT.check_offsets(off, bam, batch['st'])
    if not eqx_only:
        return
    L = batch['limit']
    assert L is not None and L >= 2
    m_form = {i for i, (m, e) in enumerate(ops_counts(batch['md_sam'])) if m > L}
    recs = [r for r in BC.records_of_bam(batch['bam'][L][0]) if not r['flag'] & 4]
    long_ones = {i for i, r in enumerate(recs) if any(t[0] == 'CG' for t in r['tags'])}
    assert long_ones - m_form and m_form <= long_ones
    for limit in (L, min(limits)):
        longs = [r for r in BC.records_of_bam(batch['bam'][limit][0]) if any(t[0] == 'CG' for t in r['tags'])]
        assert longs and all(r['tags'][-1][0] == 'CG' and [t[0] for t in r['tags']][:4] == ['NM', 'AS', 'MD', 'cs'] for r in longs)
        assert any(t[0] == 'SA' for r in longs for t in r['tags'])
        assert all([t[0] for t in r['tags'] if t[0] in ('cs', 'SA')] in (['cs'], ['cs', 'SA']) for r in longs)


def check_properties(batch, ref_of):
    """Test 3, without the restatement."""
    counts = None
    for fmt in TC.FMTS[1:]:
        counts = TC.check_properties(batch['sam'], batch['fsam'][fmt, 0][0], batch['fpaf'][fmt][0].decode(), fmt, ref_of, counts)
    return counts


def check_cases(batch, wanted, label):
    cases = TC.cs_cases(batch['fsam'][BAM_FMT, 0][0])
    assert cases == TC.cs_cases(batch['fsam'][TC.FMT_CS | TC.FMT_CS_LONG, 0][0])        # both forms say the same of the columns
    print('truth_cs_cases', label, dict(cases))
    assert all(cases[k] >= 1 for k in wanted), dict(cases)
    return cases


@functools.lru_cache(maxsize=None)
def errorful():
    pref, seqs = TS.small()
    eng = H.configure(EE.EmuEngine(1 << 28), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    return eng, formatted_batch(eng, 5, 256)


@functools.lru_cache(maxsize=None)
def full_identity():
    pref, seqs = TS.small()
    eng = H.configure(EE.EmuEngine(1 << 28), pref, 'nanopore2023', 'nanopore2023', T.full_identity_params())
    return eng, formatted_batch(eng, 11, 160)


@pytest.mark.parametrize('make', [errorful, full_identity])
def test_formatted_paf_and_sam_equal_the_restatement_for_every_fmt(make):
    check_exact(make()[1])


@pytest.mark.parametrize('make', [errorful, full_identity])
def test_formatted_bam_is_the_formatted_sam(make):
    pref, _ = TS.small()
    check_bams(make()[1], list(pref.names), eqx_only=make is errorful)


@pytest.mark.parametrize('make', [errorful, full_identity])
def test_cs_and_eqx_hold_their_properties_without_the_restatement(make):
    pref, seqs = TS.small()
    counts = check_properties(make()[1], TT.str_strands(seqs))
    assert counts['cs_lines'] > 100 and counts['eqx_lines'] > 100


def test_the_batches_show_the_branches_of_the_cs_writer():
    check_cases(errorful()[1], TC.ERRORFUL_CASES, 'errorful')
    cases = check_cases(full_identity()[1], TC.FULL_CASES, 'full_identity')
    assert cases['not_only_matches'] == 0                 # full identity: nothing but :n / =ACGT values
    sam = full_identity()[1]['fsam'][TC.FMT_EQX, 0][0].decode()
    assert 'X' not in ''.join(l.split('\t')[5] for l in sam.splitlines())


def test_the_restatement_on_a_hand_made_line():
    """The line of tests/test_truth_tags.py::test_the_restatement_on_a_hand_made_line."""
    cigar, seq, md = '2S3M1I2D2M1S', 'NNACGTTAN', '2T0^GG1C0'
    assert TT.md_of(TC.parts_of(cigar), seq, 'ACTGGTC') == md
    assert TC.cs_of(cigar, md, seq, False) == ':2*tg+t-gg:1*ca'
    assert TC.cs_of(cigar, md, seq, True) == '=AC*tg+t-gg=T*ca'
    assert TC.eqx_of(cigar, md) == '2S2=1X1I2D1=1X1S'
    assert TC.ops_of_cs(':2*tg+t-gg:1*ca') == TC.ops_of_cs('=AC*tg+t-gg=T*ca') == '==XIDD=X'
    line = '\t'.join(['0' * 36, '0', 'c', '1', '60', '2S2=1X1I2D1=1X1S', '*', '0', '0', seq, '!' * 9, 'NM:i:5', 'AS:i:-2', 'cs:Z::2*tg+t-gg:1*ca'])
    bam = TC.bam_from((line + '\n').encode(), ['c'])
    assert [x for _, x in BC.records_of_bam(bam)[0]['cigar']] == [4, 7, 8, 1, 2, 7, 8, 4]
    assert TC.sam_of_bam(bam, ['c']).decode() == line + '\n'


def test_brx_emit_fmt_abi():
    from badread_amd import engine as E
    assert (E.FMT_EQX, E.FMT_CS, E.FMT_CS_LONG) == (1, 2, 4)
    pref, _ = TS.small()
    fresh = H.configure(EE.EmuEngine(1 << 24), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    for call in (lambda: fresh.emit_paf_device(48, E.FMT_CS), lambda: fresh.emit_sam_device(48, 0, E.FMT_EQX),
                 lambda: fresh.emit_bam_device(48, 65535, E.TAG_MD, E.FMT_CS)):
        with pytest.raises(E.BrxError) as ex:               # BRX_E_STATE: no batch yet
            call()
        assert ex.value.code == -6
    eng, batch = errorful()
    n = len(batch['st'])
    for fmt in (8, E.FMT_CS_LONG, E.FMT_CS_LONG | E.FMT_EQX, 16 | E.FMT_CS):
        for call in (lambda: eng.emit_paf_device(n, fmt), lambda: eng.emit_sam_device(n, 0, fmt), lambda: eng.emit_bam_device(n, 65535, 0, fmt)):
            with pytest.raises(E.BrxError) as ex:           # BRX_E_ARG: an unknown bit, or CS_LONG without CS
                call()
            assert ex.value.code == -1
    with pytest.raises(E.BrxError) as ex:                   # the tags' own check stands
        eng.emit_sam_device(n, 4, E.FMT_CS)
    assert ex.value.code == -1
    # a buffer that is too small: BRX_E_OUTPUT, nothing written, the exact size to come back with; the repeat succeeds
    for want, emit in ((batch['fsam'][BAM_FMT, BOTH][0], lambda *a: eng.lib.brx_emit_sam_fmt(eng.ctx, BAM_FMT, BOTH, *a)),
                       (batch['bam'][8][0], lambda *a: eng.lib.brx_emit_bam_fmt(eng.ctx, BAM_FMT, BOTH, 8, *a)),
                       (batch['fpaf'][BAM_FMT][0], lambda *a: eng.lib.brx_emit_paf_fmt(eng.ctx, BAM_FMT, *a))):
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


@pytest.mark.parametrize('text', ['Short', 'both', '', 'short,long', 'cs'])
def test_truth_cs_spelt_otherwise_is_an_error(tmp_path, text):
    from badread_amd.__main__ import check_simulate_args
    with pytest.raises(SystemExit) as ex:
        check_simulate_args(_cli_args('--truth-paf', str(tmp_path / 'x.paf'), '--truth-cs', text))
    assert ex.value.code == 'Error: --truth-cs must be short or long'


def test_truth_cs_and_eqx_without_a_file_are_errors():
    from badread_amd.__main__ import check_simulate_args
    with pytest.raises(SystemExit) as ex:
        check_simulate_args(_cli_args('--truth-cs', 'short'))
    assert ex.value.code == 'Error: --truth-cs needs --truth-paf, --truth-sam or --truth-bam'
    with pytest.raises(SystemExit) as ex:
        check_simulate_args(_cli_args('--truth-eqx'))
    assert ex.value.code == 'Error: --truth-eqx needs --truth-paf, --truth-sam or --truth-bam'


def test_truth_cs_and_eqx_become_the_mask(tmp_path):
    from badread_amd.__main__ import check_simulate_args
    for file_flag in ('--truth-paf', '--truth-sam', '--truth-bam'):
        for extra, mask in (((), 0), (('--truth-eqx',), 1), (('--truth-cs', 'short'), 2), (('--truth-cs', 'long'), 6),
                            (('--truth-cs', 'short', '--truth-eqx'), 3), (('--truth-eqx', '--truth-cs', 'long'), 7)):
            args = _cli_args(file_flag, str(tmp_path / 'x'), *extra)
            check_simulate_args(args)
            assert args.truth_fmt == mask and args.truth_tags == 0
    args = _cli_args()
    check_simulate_args(args)
    assert args.truth_fmt == 0


def test_the_options_are_in_the_help_and_the_readme(capsys):
    import os
    from badread_amd.__main__ import parse_args
    with pytest.raises(SystemExit):
        parse_args(['simulate', '--help'])
    text = capsys.readouterr().out
    assert '--truth-cs MODE' in text and '--truth-eqx' in text
    readme = open(os.path.join(os.path.dirname(TS.__file__), '..', 'README.md')).read()
    assert '--truth-cs short|long' in readme.split('\n## ')[0] and '--truth-eqx' in readme.split('\n## ')[0]


def test_the_first_buffer_counts_every_share_once_per_file():
    from badread_amd import engine as E
    from badread_amd import simulate as S
    base = 1000 * (2.1 * 15000.0 + 400.0)
    for share in (E.EQX_SHARE, E.CS_SHORT_SHARE, E.CS_LONG_SHARE):
        assert sorted(share) == ['bam', 'paf', 'sam'] and all(v > 0 for v in share.values())
    def bytes_of(paf, sam, bam, tags, fmt=0, truth_fmt=0):             # the flags as the driver reads them off its arguments
        kinds = [k for k, on in (('paf', paf), ('sam', sam), ('bam', bam)) if on]
        return S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(kinds, tags, fmt or truth_fmt))
    near = lambda share: pytest.approx(base * (1.0 + share), abs=1.5)       # int() of a sum of doubles taken in another order
    assert bytes_of(True, True, True, 3) == bytes_of(True, True, True, 3, truth_fmt=0) == bytes_of(True, True, True, 3, 0)
    assert bytes_of(False, True, False, 3, truth_fmt=3) == near(S.SAM_SHARE + E.MD_SHARE + E.SA_SHARE + E.EQX_SHARE['sam'] + E.CS_SHORT_SHARE['sam'])
    assert bytes_of(True, False, True, 0, truth_fmt=6) == near(S.PAF_SHARE + S.BAM_SHARE + E.CS_LONG_SHARE['paf'] + E.CS_LONG_SHARE['bam'])
    assert bytes_of(True, True, True, 0, truth_fmt=1) == near(S.PAF_SHARE + S.SAM_SHARE + S.BAM_SHARE + sum(E.EQX_SHARE.values()))
    assert bytes_of(False, False, False, 0, truth_fmt=7) == int(base)


def test_truth_cs_and_eqx_through_the_host_driver(tmp_path, monkeypatch):
    """simulate() with the three files, --truth-cs short --truth-eqx and --truth-tags MD,SA: the same files whatever the batch size and
    the streams, FASTQ and return value those of the plain run, the SAM and the PAF the restatement of the plain MD-tagged run's, the
    BAM's blocks those records."""
    from badread_amd import simulate as S
    import test_truth_bam as TB
    pref, seqs = TS.small()
    args = dict(quantity='5x', mean_frag_length=300.0, frag_length_stdev=200.0, error_model='nanopore2023', qscore_model='nanopore2023',
                mean_identity=92.0, max_identity=98.0, identity_stdev=3.0, seed=3)
    monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', 12)
    plain = io.BytesIO()
    plain_sam, plain_paf = str(tmp_path / 'plain.sam'), str(tmp_path / 'plain.paf')
    base = S.simulate(T._Args(truth_sam=plain_sam, truth_paf=plain_paf, truth_tags=TT.TAG_MD, **args), output=io.StringIO(),
                      engine=EE.EmuEngine(1 << 28), stdout=plain, shard=S.Shard())
    files = []
    for max_batch, streams in ((12, 1), (7, 2)):
        monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', max_batch)
        fq = io.BytesIO()
        sam_path, bam_path, paf_path = (str(tmp_path / f'fmt{max_batch}.{x}') for x in ('sam', 'bam', 'paf'))
        got = S.simulate(T._Args(truth_sam=sam_path, truth_bam=bam_path, truth_paf=paf_path, truth_tags=3, truth_fmt=3, gpu_streams=streams, **args),
                         output=io.StringIO(), engine=EE.EmuEngine(1 << 28), stdout=fq, shard=S.Shard())
        assert got == base and fq.getvalue() == plain.getvalue()
        files.append((open(sam_path, 'rb').read(), TB.split_bam(open(bam_path, 'rb').read(), pref)[1], open(paf_path, 'rb').read()))
    assert files[0] == files[1]
    head = TS.expected_header(pref)
    md_sam = open(plain_sam, 'rb').read()
    assert md_sam.startswith(head) and files[0][0].startswith(head)
    want = TC.formatted_sam_from(md_sam[len(head):], 3, 3)
    assert files[0][0][len(head):] == want and want.count(b'\tcs:Z:') > 10 and b'X' in b''.join(l.split(b'\t')[5] for l in want.splitlines())
    assert files[0][1] == TC.bam_from(want, list(pref.names))
    assert files[0][2].decode() == TC.formatted_paf_from(open(plain_paf).read(), md_sam[len(head):], 3)
