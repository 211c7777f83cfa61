"""
--truth-sam: the true alignment of every simulated read as SAM (brx_emit_sam, badread_amd/csrc/brx_sam.h), on the emulated device.

A read's SAM lines are a function of its FASTQ record and its truth-PAF records (README, --truth-sam).  That function is restated
here in plain Python (`sam_from`) and the device's bytes must equal it; PAF and SAM come from one batch, so errorful reads are
exact too.  `check_invariants` checks what must hold of any such file without that function (field counts, flags, CIGAR
lengths, clips, one primary or unmapped line per read, NM recomputed from SEQ against the reference).
tests/test_gpu_truth_sam.py runs the same checks on the MI355X.
"""
import collections
import ctypes
import functools
import io
import re

import numpy as np
import pytest

import emu_engine as EE
import helpers as H
import test_truth_paf as T

_CIGAR = re.compile(r'(\d+)([MIDSH])')
MATE = ['*', '0', '0']


def sam_from(fastq, paf_text, sym, comp):
    """The SAM records (no header) of the reads of `fastq` whose truth alignments are `paf_text`: the contract of --truth-sam."""
    sym, comp = [int(x) for x in sym], [int(x) for x in comp]
    code_of = {}
    for code, ch in enumerate(sym):
        code_of.setdefault(ch, code)
    flip = bytes(sym[comp[code_of[b]]] if b in code_of else b for b in range(256))      # the complement, through the codes
    by_read = collections.defaultdict(list)
    for line in paf_text.splitlines():
        f = line.split('\t')
        by_read[f[0]].append(f)
    lines = bytes(fastq).decode('latin-1').split('\n')
    out = []
    for i in range(0, len(lines) - 1, 4):
        name, _, comment = lines[i][1:].partition(' ')
        seq, qual = lines[i + 1], lines[i + 3]
        L = len(seq)
        if name not in by_read:
            out.append([name, '4', '*', '0', '0', '*'] + MATE + [seq, qual, 'CO:Z:' + comment])
            continue
        for f in by_read[name]:
            qs, qe, minus, ts = int(f[2]), int(f[3]), f[4] == '-', int(f[7])
            primary = f[12] == 'tp:A:P'
            left, right = (L - qe, qs) if minus else (qs, L - qe)
            clip = 'S' if primary else 'H'
            cigar = (f'{left}{clip}' if left else '') + f[13][5:] + (f'{right}{clip}' if right else '')
            s, q = (seq, qual) if primary else (seq[qs:qe], qual[qs:qe])
            if minus:
                s, q = s.encode('latin-1').translate(flip)[::-1].decode('latin-1'), q[::-1]
            flag = (16 if minus else 0) | (0 if primary else 2048)
            out.append([name, str(flag), f[5], str(ts + 1), '60', cigar] + MATE + [s, q, f[14], f[15]] + (['CO:Z:' + comment] if primary else []))
    return ''.join('\t'.join(x) + '\n' for x in out).encode('latin-1')


def expected_header(pref):
    from badread_amd.version import __version__
    sq = ''.join(f'@SQ\tSN:{n}\tLN:{int(x)}\n' for n, x in zip(pref.names, pref.lengths))
    return ('@HD\tVN:1.6\tSO:unsorted\tGO:query\n' + sq + f'@PG\tID:badread_amd\tPN:badread_amd\tVN:{__version__}\n').encode()


def coverage(sam):
    """How often the batch takes each branch of the writer: a test passes only on an input that shows every one."""
    c = collections.Counter()
    reads = {}
    for line in sam.decode('latin-1').splitlines():
        f = line.split('\t')
        flag, parts = int(f[1]), _CIGAR.findall(f[5])
        if not flag & 2048:
            reads[f[0]] = len(f[9])
        if flag & 4:
            c['unmapped'] += 1
            continue
        left, right = parts[0][1] in 'SH', parts[-1][1] in 'SH'
        c['minus'] += bool(flag & 16)
        c['supplementary'] += bool(flag & 2048)
        c['supplementary_minus'] += flag & 2064 == 2064
        c['long_primary_minus'] += flag == 16 and len(f[9]) > 64
        c['no_left_clip'] += not left
        c['no_right_clip'] += not right
        c['no_clip'] += not left and not right
    c['short_reads'] = sum(1 for n in reads.values() if n <= 64)
    return c


CASES = ('minus', 'supplementary', 'supplementary_minus', 'long_primary_minus', 'unmapped', 'no_left_clip', 'no_right_clip', 'no_clip',
         'short_reads')


def _nm(parts, q, t):
    """NM of a SAM CIGAR walked over SEQ q against the reference slice t (uint8 symbols): mismatches in M, plus I and D."""
    lens = np.array([n for n, _ in parts], dtype=np.int64)
    ops = np.array([x for _, x in parts])
    m = ops == 'M'
    qadv, tadv = lens * ((ops != 'D') & (ops != 'H')), lens * (m | (ops == 'D'))
    q0, t0 = np.cumsum(qadv) - qadv, np.cumsum(tadv) - tadv
    ml = lens[m]
    within = np.arange(int(ml.sum())) - np.repeat(np.cumsum(ml) - ml, ml)
    differ = int((q[np.repeat(q0[m], ml) + within] != t[np.repeat(t0[m], ml) + within]).sum())
    return differ + int(lens[ops == 'I'].sum()) + int(lens[ops == 'D'].sum())


def forward_strands(seqs):
    """name -> the contig's forward strand as uint8 symbols, from (name, text) pairs."""
    table = {n: np.frombuffer(t.encode(), dtype=np.uint8) for n, t in seqs}
    return table.__getitem__


def check_invariants(sam, ref_of, n_fastq_reads=None):
    """What holds of every --truth-sam record file, without sam_from; ref_of(name) = a contig's forward strand (uint8 symbols).
    Returns (lines, reads)."""
    per_read = collections.Counter()
    n_lines = 0
    for line in sam.decode('latin-1').splitlines():
        f = line.split('\t')
        n_lines += 1
        assert len(f) >= 11, f[:9]
        flag, seq, qual = int(f[1]), f[9], f[10]
        assert flag in (0, 4, 16, 2048, 2064), flag
        assert len(seq) == len(qual) and len(seq) > 0
        tags = [x[:5] for x in f[11:]]
        per_read[f[0]] += not flag & 2048
        assert ('CO:Z:' in tags) == (not flag & 2048), f[:9]
        if flag & 4:
            assert f[2:9] == ['*', '0', '0', '*', '*', '0', '0'] and tags == ['CO:Z:']
            continue
        assert f[4] == '60' and f[6:9] == MATE and tags[:2] == ['NM:i:', 'AS:i:']
        parts = [(int(n), x) for n, x in _CIGAR.findall(f[5])]
        assert ''.join(f'{n}{x}' for n, x in parts) == f[5] and all(n > 0 for n, _ in parts)
        assert sum(n for n, x in parts if x in 'MIS') == len(seq), f[:9]
        clips = {x for _, x in parts if x in 'SH'}
        assert clips <= ({'H'} if flag & 2048 else {'S'}), f[:9]
        assert all(x not in 'SH' for _, x in parts[1:-1])
        # NM from SEQ as it stands (a '-' line is stored reverse-complemented, i.e. on the reference's forward strand)
        pos, ref = int(f[3]) - 1, ref_of(f[2])
        span = sum(n for n, x in parts if x in 'MD')
        assert 0 <= pos and pos + span <= len(ref), f[:9]
        target = ref[pos:pos + span]
        if (target == ord('N')).any():
            continue
        assert _nm(parts, np.frombuffer(seq.encode('latin-1'), dtype=np.uint8), target) == int(f[11][5:]), f[:9]
    assert all(v == 1 for v in per_read.values())
    if n_fastq_reads is not None:
        assert len(per_read) == n_fastq_reads
    return n_lines, len(per_read)


def emit_both(eng, seed, n_reads):
    """One batch: its FASTQ, its PAF text, its SAM bytes and the SAM's read offsets."""
    fastq, st = eng.simulate_batch(seed, 0, n_reads)
    fastq = bytes(fastq[:int(st['rec_off'][-1] + st['rec_len'][-1])])
    paf, _ = eng.emit_paf_device(n_reads)
    paf = bytes(paf.cpu().numpy())
    sam, off = eng.emit_sam_device(n_reads)
    sam = bytes(sam.cpu().numpy())
    paf_again, _ = eng.emit_paf_device(n_reads)
    assert bytes(paf_again.cpu().numpy()) == paf            # brx_emit_sam in between leaves the PAF as it was
    return fastq, st.copy(), paf.decode(), sam, off


def check_batch(eng, pref, seqs, seed, n_reads):
    """Checks 1-4 of one configured engine's batch (shared with the GPU file); `seqs`: (name, forward strand) pairs, or a function
    from a contig's name to its forward strand as uint8 symbols.  Returns (fastq, stats, sam)."""
    fastq, st, paf, sam, off = emit_both(eng, seed, n_reads)
    want = sam_from(fastq, paf, pref.sym, pref.comp)
    assert sam == want
    assert len(off) == n_reads + 1 and int(off[0]) == 0 and int(off[-1]) == len(sam) and (np.diff(off.astype(np.int64)) >= 0).all()
    live = st['rec_len'] > 0
    assert all(int(off[r + 1]) > int(off[r]) for r in np.flatnonzero(live)) and all(int(off[r + 1]) == int(off[r]) for r in np.flatnonzero(~live))
    cases = coverage(sam)
    print('truth_sam_cases', dict(cases))
    assert all(cases[k] >= 1 for k in CASES), dict(cases)
    check_invariants(sam, forward_strands(seqs) if isinstance(seqs, list) else seqs, int(live.sum()))
    return fastq, st, sam


@functools.lru_cache(maxsize=None)
def small():
    return T.small_ref()


def test_truth_sam_of_a_full_identity_batch():
    pref, seqs = small()
    eng = H.configure(EE.EmuEngine(1 << 28), pref, 'nanopore2023', 'nanopore2023', T.full_identity_params())
    check_batch(eng, pref, seqs, 11, 160)


def test_truth_sam_of_an_errorful_batch():
    pref, seqs = small()
    eng = H.configure(EE.EmuEngine(1 << 28), pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    check_batch(eng, pref, seqs, 5, 256)


def test_brx_emit_sam_abi():
    from badread_amd import engine as E
    pref, seqs = small()
    eng = EE.EmuEngine(1 << 28)
    H.configure(eng, pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    with pytest.raises(E.BrxError) as ex:                   # BRX_E_STATE: no batch yet
        eng.emit_sam_device(48)
    assert ex.value.code == -6
    eng.simulate_batch(21, 0, 48)
    paf_alone = bytes(eng.emit_paf_device(48)[0].numpy())
    eng.simulate_batch(21, 0, 48)                            # the same batch again: SAM first, then PAF, then SAM
    sam_first = bytes(eng.emit_sam_device(48)[0].numpy())
    assert bytes(eng.emit_paf_device(48)[0].numpy()) == paf_alone
    assert bytes(eng.emit_sam_device(48)[0].numpy()) == sam_first and len(sam_first) > len(paf_alone)
    # a buffer that is too small: BRX_E_OUTPUT, nothing written, and the size to come back with
    got = ctypes.c_size_t(0)
    buf = eng.torch.zeros(64, dtype=eng.torch.uint8)
    assert eng.lib.brx_emit_sam(eng.ctx, ctypes.c_void_p(buf.data_ptr()), 64, None, ctypes.byref(got), None) == E.E_OUTPUT
    need = int(eng.lib.brx_output_needed(eng.ctx))
    assert need == len(sam_first) and not buf.any() and got.value == 0
    full = eng.torch.zeros(need, dtype=eng.torch.uint8)
    off = eng.torch.zeros(49, dtype=eng.torch.int64)
    rc = eng.lib.brx_emit_sam(eng.ctx, ctypes.c_void_p(full.data_ptr()), need, ctypes.c_void_p(off.data_ptr()), ctypes.byref(got), None)
    assert rc == 0 and got.value == need and int(off[-1]) == need and bytes(full.numpy()) == sam_first
    # after brx_sequence_fragments the arena holds something else
    eng.sequence_fragments(3, 0, [np.array([0, 1, 2, 3] * 20, dtype=np.uint8)], [0.9])
    with pytest.raises(E.BrxError) as ex:
        eng.emit_sam_device(48)
    assert ex.value.code == -6


def _records_of(names, sam_records):
    """The record lines of `sam_records` in the order of the FASTQ names: all of a read's lines, each read once."""
    order = [line.split(b'\t')[0].decode() for line in sam_records.splitlines()]
    firsts = [n for j, n in enumerate(order) if j == 0 or order[j - 1] != n]
    assert firsts == names


def test_truth_sam_through_the_host_driver(tmp_path, monkeypatch):
    from badread_amd import simulate as S
    pref, seqs = small()
    args = dict(quantity='5x', mean_frag_length=300.0, frag_length_stdev=200.0, error_model='nanopore2023', qscore_model='nanopore2023',
                mean_identity=92.0, max_identity=98.0, identity_stdev=3.0, seed=3)
    plain = io.BytesIO()
    monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', 12)
    base = S.simulate(T._Args(**args), output=io.StringIO(), engine=EE.EmuEngine(1 << 28), stdout=plain, shard=S.Shard())
    files = []
    for max_batch, streams in ((12, 1), (7, 2)):
        monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', max_batch)
        fq = io.BytesIO()
        sam_path, paf_path = str(tmp_path / f'truth{max_batch}.sam'), str(tmp_path / f'truth{max_batch}.paf')
        got = S.simulate(T._Args(truth_sam=sam_path, truth_paf=paf_path, gpu_streams=streams, **args), output=io.StringIO(),
                         engine=EE.EmuEngine(1 << 28), stdout=fq, shard=S.Shard())
        assert got == base and fq.getvalue() == plain.getvalue()
        files.append(open(sam_path, 'rb').read())
        paf = open(paf_path).read()
    assert files[0] == files[1]
    head = expected_header(pref)
    assert files[0].startswith(head)
    records = files[0][len(head):]
    names, _ = T.parse_fastq_names(plain.getvalue())
    _records_of(names, records)                              # exactly the FASTQ's reads: the stop rule cuts both at the same one
    assert records == sam_from(plain.getvalue(), paf, pref.sym, pref.comp)
    check_invariants(records, forward_strands(seqs), len(names))


def test_truth_sam_missing_directory_is_an_error(tmp_path):
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, '-m', 'badread_amd', 'simulate', '--reference', T.SMALL_REF, '--quantity', '1x',
                        '--truth-sam', str(tmp_path / 'nope' / 'x.sam')], capture_output=True, text=True, cwd=os.path.dirname(T.HERE))
    assert r.returncode == 1 and r.stderr.startswith('Error: ') and 'truth-sam' in r.stderr


def test_byte_counts_beyond_32_bits_are_exchanged_whole():
    from badread_amd import simulate as S
    assert S.Shard().gather_word64(5 * 2 ** 32 + 7) == [5 * 2 ** 32 + 7]
    assert S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(['sam'])) == int(1000 * (2.1 * 15000.0 + 400.0) * (1.0 + S.SAM_SHARE))
    assert S.expected_out_bytes(None, 1000, 15000.0, S.TruthSpec(['paf', 'sam'])) == int(1000 * (2.1 * 15000.0 + 400.0) * (1.0 + S.PAF_SHARE + S.SAM_SHARE))
