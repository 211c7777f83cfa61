"""
--truth-paf: the true alignment of every simulated read (brx_emit_paf, badread_amd/csrc/brx_paf.h), on the emulated device.

The record rules (README, --truth-paf) are restated here in plain Python (`expected_records`) and checked against the kernels:
exactly at 100 % identity, where the final alignment of a read is all '=' and the expected PAF follows from the oracle's plan
alone; and by properties on errorful reads (CIGAR lengths, NM against an optimal alignment, provenance, overlaps).
tests/test_gpu_truth_paf.py runs the same checks on the MI355X.
"""
import io
import os
import re
import sys

import numpy as np
import pytest

import emu_engine as EE
import helpers as H

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_REF = os.path.join(HERE, 'golden', 'small_ref.fasta')
COMP = str.maketrans('ACGTNMKRYSWBVDHacgtn', 'TGCANKMYRSWVBHDtgcan')      # IUPAC symbols the packed reference keeps


def small_ref():
    """(packed reference, {name: forward sequence}): the sequence the fragments are cut from, N runs resolved as the
    packed reference holds them (PackedReference.decode), not the FASTA text."""
    from badread_amd.misc import load_fasta
    from badread_amd.reference import PackedReference
    pref = PackedReference.from_seqs(*load_fasta(SMALL_REF))
    return pref, [(n, pref.decode(i, '+', 0, int(L))) for i, (n, L) in enumerate(zip(pref.names, pref.lengths))]


def revcomp(s):
    return s.translate(COMP)[::-1]


def parse_fastq_names(fastq):
    lines = bytes(fastq).decode().split('\n')
    return [lines[i][1:].split(' ')[0] for i in range(0, len(lines) - 1, 4)], [lines[i + 1] for i in range(0, len(lines) - 1, 4)]


def expected_records(ops, segs, k, lo, hi, seq_len, qname, names, lengths):
    """The PAF lines of one read by the contract: ops = its final alignment (0 '=' 1 'X' 2 'I' 3 'D'), segs = oracle plan()
    segments (type, contig, strand, start, len), [lo, hi) = the kept read indices."""
    origin, dst = {}, 0
    for t, a, b, start, ln in segs:
        if t == 0:
            for i in range(int(ln)):
                origin[dst + i] = (int(a), int(b), int(start) + i)
        dst += int(ln)
    runs, cur, last_t = [], [], None
    r = f = 0
    for op in ops:
        q, t = op != 3, op != 2
        o = origin.get(f - k) if t else None
        good = (not t or o is not None) and (not q or lo <= r < hi)
        col = (int(op), r, o)
        r += q
        f += t
        if not good:
            runs.append(cur)
            cur, last_t = [], None
            continue
        if o is not None:
            if last_t is not None and not (last_t[:2] == o[:2] and last_t[2] + 1 == o[2]):
                runs.append(cur)
                cur = []
            last_t = o
        cur.append(col)
    runs.append(cur)
    recs = []
    for run in runs:
        m = [i for i, c in enumerate(run) if c[0] <= 1]
        if not m:
            continue
        cols = run[m[0]:m[-1] + 1]
        qcols = [c for c in cols if c[0] != 3]
        tpos = [c[2] for c in cols if c[0] != 2]
        contig, strand = tpos[0][0], tpos[0][1]
        L = lengths[contig]
        p0, p1 = tpos[0][2], tpos[-1][2]
        ts, te = (p0, p1 + 1) if strand == 0 else (L - 1 - p1, L - p0)
        cig = []
        for c in cols:
            letter = 'M' if c[0] <= 1 else 'I' if c[0] == 2 else 'D'
            if cig and cig[-1][1] == letter:
                cig[-1][0] += 1
            else:
                cig.append([1, letter])
        if strand == 1:
            cig = cig[::-1]
        n_eq = sum(1 for c in cols if c[0] == 0)
        nm = len(cols) - n_eq
        recs.append([qname, seq_len, qcols[0][1] - lo, qcols[-1][1] + 1 - lo, '+-'[strand], names[contig], L, ts, te, n_eq,
                     len(cols), 60, None, ''.join(f'{n}{x}' for n, x in cig), nm, n_eq - nm])
    if recs:
        best = max(range(len(recs)), key=lambda i: (recs[i][-1], -i))
        for i, rec in enumerate(recs):
            rec[12] = 'P' if i == best else 'S'
    return ['\t'.join(str(x) for x in rec[:12]) + f'\ttp:A:{rec[12]}\tcg:Z:{rec[13]}\tNM:i:{rec[14]}\tAS:i:{rec[15]}\n'
            for rec in recs]


def full_identity_params():
    return H.SimParams(frag_mean=300, frag_stdev=250, identity_mode=0, id_max=1.0, chimera_rate=0.3, glitch_rate=200,
                       glitch_size=5, glitch_skip=5, junk_rate=0.05, random_rate=0.05)


def check_full_identity(eng, pref, seed, n_reads):
    """Test 1 (shared with the GPU file): the PAF of a batch at 100 % identity equals the one the rules give, byte for byte."""
    from pyoracle import OracleEngine
    fastq, st = eng.simulate_batch(seed, 0, n_reads)
    paf, off = eng.emit_paf_device(n_reads)
    got = bytes(paf.cpu().numpy()).decode()
    orc = H.configure(OracleEngine(), pref, 'nanopore2023', 'nanopore2023', full_identity_params())
    qnames, _ = parse_fastq_names(fastq[:int(st['rec_off'][-1] + st['rec_len'][-1])])
    live = st['rec_len'] > 0
    k = int(st['padded_len'][live][0] - st['seq_len'][live][0]) // 2      # the pads: the error model's k on both ends
    names, lengths = list(pref.names), [int(x) for x in pref.lengths]
    want, features, name_at = [], dict(wrap=0, hairpin=0, glitch=0, chimera=0), 0
    for i in range(n_reads):
        if st['rec_len'][i] == 0:
            continue
        qn = qnames[name_at]
        name_at += 1
        plan = orc.plan(seed, i)
        assert st['seq_len'][i] == plan['frag_len'] and st['n_cols'][i] == plan['frag_len'] + 2 * k
        assert st['n_match'][i] == st['n_cols'][i]                      # all '=': the read is its padded fragment
        segs = plan['segs']
        ops = np.zeros(int(st['n_cols'][i]), dtype=np.uint8)
        recs = expected_records(ops, segs, k, k, int(st['padded_len'][i]) - k, int(st['seq_len'][i]), qn, names, lengths)
        want += recs
        ref = [s for s in segs if s[0] == 0]
        for a, b in zip(ref, ref[1:]):
            if a[1] == b[1] and a[2] != b[2]:
                features['hairpin'] += 1
            elif a[1] == b[1] and a[2] == b[2] and b[3] == 0 and a[3] + a[4] == lengths[int(a[1])]:
                features['wrap'] += 1
        features['glitch'] += int(any(s[0] == 2 and s[1] >= 2 for s in segs) or len(recs) > len(plan['pieces']))
        features['chimera'] += int(len(plan['pieces']) > 1 and len(recs) > 1)
    assert name_at == len(qnames)
    assert got == ''.join(want)
    assert [int(x) for x in off[1:]] == sorted(int(x) for x in off[1:]) and int(off[-1]) == len(got)
    return features


def test_truth_paf_is_exact_at_full_identity():
    pref, _ = small_ref()
    eng = H.configure(EE.EmuEngine(1 << 28), pref, 'nanopore2023', 'nanopore2023', full_identity_params())
    feats = check_full_identity(eng, pref, 11, 160)
    assert all(v >= 1 for v in feats.values()), feats


def check_errorful(seqs_by_name, fastq, st, paf_text, plans, contig_names, lengths_by_name):
    """Test 2 (shared with the GPU file): every record of errorful reads is a consistent, optimal, in-provenance alignment.
    plans: read index -> oracle plan (or None to skip the provenance check); contig_names: the plan's contig index -> name.
    Returns the fraction of SEG_REF bases covered."""
    from pyoracle import align
    names, reads = parse_fastq_names(fastq)
    live = [i for i in range(len(st)) if st['rec_len'][i] > 0]
    assert len(live) == len(names)
    read_of = dict(zip(names, zip(live, reads)))
    by_read, order = {}, []
    for line in paf_text.splitlines():
        f = line.split('\t')
        assert len(f) == 16
        by_read.setdefault(f[0], []).append(f)
        if not order or order[-1] != f[0]:
            order.append(f[0])
    assert len(order) == len(by_read)                    # a read's records are together
    pos = {n: j for j, n in enumerate(names)}
    assert [pos[n] for n in order] == sorted(pos[n] for n in order)        # in FASTQ order
    covered = ref_bases = 0
    for name, recs in by_read.items():
        i, read = read_of[name]
        assert sum(1 for f in recs if f[12] == 'tp:A:P') == 1
        assert [int(f[2]) for f in recs] == sorted(int(f[2]) for f in recs)
        for a, b in zip(recs, recs[1:]):
            assert int(a[3]) <= int(b[2])                 # no overlap in the read
        for f in recs:
            qs, qe, ts, te = int(f[2]), int(f[3]), int(f[7]), int(f[8])
            assert int(f[1]) == len(read) and 0 <= qs < qe <= len(read)
            assert int(f[6]) == lengths_by_name[f[5]] and 0 <= ts < te <= int(f[6])
            parts = [(int(n), x) for n, x in re.findall(r'(\d+)([MID])', f[13][5:])]
            if f[4] == '-':
                parts = parts[::-1]
            assert sum(n for n, x in parts if x != 'D') == qe - qs and sum(n for n, x in parts if x != 'I') == te - ts
            assert sum(n for n, _ in parts) == int(f[10]) and parts[0][1] == 'M' and parts[-1][1] == 'M'
            tseq = seqs_by_name[f[5]][ts:te]
            if f[4] == '-':
                tseq = revcomp(tseq)
            qseq = read[qs:qe]
            x = y = eq = nm = 0
            for n, op in parts:
                if op == 'M':
                    same = sum(1 for d in range(n) if qseq[x + d] == tseq[y + d])
                    eq += same
                    nm += n - same
                    x += n
                    y += n
                elif op == 'I':
                    x += n
                    nm += n
                else:
                    y += n
                    nm += n
            covered += te - ts
            if plans is not None and i in plans:
                ok = False
                for s in plans[i]['segs']:
                    if s[0] != 0 or contig_names[int(s[1])] != f[5] or '+-'[int(s[2])] != f[4]:
                        continue
                    L = lengths_by_name[f[5]]
                    lo, hi = (int(s[3]), int(s[3]) + int(s[4])) if f[4] == '+' else (L - int(s[3]) - int(s[4]), L - int(s[3]))
                    if lo <= ts and te <= hi:
                        ok = True
                assert ok or record_spans_adjacent_segments(plans[i]['segs'], f, contig_names, lengths_by_name), (name, f[:12])
            assert int(f[15][5:]) == int(f[9]) - int(f[14][5:])
            if 'N' in tseq:
                # the fragment carries a random base where the reference has an N: the read's alignment may call it '='
                assert 0 <= int(f[9]) - eq <= tseq.count('N'), (name, f[:12])
                continue
            assert eq == int(f[9]) and nm == int(f[14][5:]), (name, f[:12])
            dist, _ = align(qseq.encode(), tseq.encode(), want_ops=False)
            assert nm == dist, (name, f[:12], nm, dist)
    if plans is not None:
        for i, p in plans.items():
            if st['rec_len'][i] > 0:
                ref_bases += sum(int(s[4]) for s in p['segs'] if s[0] == 0)
        return covered / max(ref_bases, 1)
    return None




def record_spans_adjacent_segments(segs, f, contig_names, lengths_by_name):
    """A record may cover consecutive SEG_REF segments that continue each other on the same strand (a glitch that inserted and
    skipped nothing): merge such neighbours and look again."""
    L = lengths_by_name[f[5]]
    merged = []
    for s in segs:
        s = [int(x) for x in s]
        if merged and s[0] == 0 and merged[-1][0] == 0 and merged[-1][1:3] == s[1:3] and merged[-1][3] + merged[-1][4] == s[3]:
            merged[-1][4] += s[4]
        else:
            merged.append(s)
    for s in merged:
        if s[0] != 0 or contig_names[s[1]] != f[5] or '+-'[s[2]] != f[4]:
            continue
        lo, hi = (s[3], s[3] + s[4]) if f[4] == '+' else (L - s[3] - s[4], L - s[3])
        if lo <= int(f[7]) and int(f[8]) <= hi:
            return True
    return False


def errorful_batch(eng, pref, seed, n_reads):
    from pyoracle import OracleEngine
    p = H.SimParams(frag_mean=400, frag_stdev=300)
    H.configure(eng, pref, 'nanopore2023', 'nanopore2023', p)
    fastq, st = eng.simulate_batch(seed, 0, n_reads)
    paf, off = eng.emit_paf_device(n_reads)
    orc = H.configure(OracleEngine(), pref, 'nanopore2023', 'nanopore2023', p)
    plans = {i: orc.plan(seed, i) for i in range(n_reads)}
    return fastq[:int(st['rec_off'][-1] + st['rec_len'][-1])], st, bytes(paf.cpu().numpy()).decode(), plans


def test_truth_paf_records_of_errorful_reads():
    pref, seqs = small_ref()
    eng = EE.EmuEngine(1 << 28)
    fastq, st, paf, plans = errorful_batch(eng, pref, 5, 256)
    seqs_by_name = dict(seqs)
    lengths = {n: int(x) for n, x in zip(pref.names, pref.lengths)}
    frac = check_errorful(seqs_by_name, fastq, st, paf, plans, list(pref.names), lengths)
    # an estimate, not a derived bound: measured 0.99957 of the SEG_REF bases in a record on this batch (what is lost: the
    # ends of a stretch that the alignment opens or closes with an indel, which a record trims away)
    assert frac >= 0.99, frac


class _Args(object):
    def __init__(self, **kw):
        from test_host_simulate import Args
        self.__dict__.update(Args(**kw).__dict__)


@pytest.mark.parametrize('max_batch,streams', [(12, 1), (12, 3), (64, 2), (7, 1)])
def test_truth_paf_leaves_the_fastq_unchanged(tmp_path, monkeypatch, max_batch, streams):
    from badread_amd import simulate as S
    monkeypatch.setattr(S, 'DEFAULT_MAX_BATCH', max_batch)
    args = dict(quantity='5x', mean_frag_length=300.0, frag_length_stdev=200.0, error_model='nanopore2023',
                qscore_model='nanopore2023', mean_identity=92.0, max_identity=98.0, identity_stdev=3.0, seed=3, gpu_streams=streams)
    a, b = io.BytesIO(), io.BytesIO()
    path = str(tmp_path / 'truth.paf')
    ra = S.simulate(_Args(**args), output=io.StringIO(), engine=EE.EmuEngine(1 << 28), stdout=a, shard=S.Shard())
    rb = S.simulate(_Args(truth_paf=path, **args), output=io.StringIO(), engine=EE.EmuEngine(1 << 28), stdout=b, shard=S.Shard())
    assert ra == rb and a.getvalue() == b.getvalue()
    names, reads = parse_fastq_names(a.getvalue())
    paf = open(path).read()
    qn = [line.split('\t')[0] for line in paf.splitlines()]
    firsts = [n for j, n in enumerate(qn) if j == 0 or qn[j - 1] != n]
    pos = {n: j for j, n in enumerate(names)}
    assert all(n in pos for n in firsts) and [pos[n] for n in firsts] == sorted(pos[n] for n in firsts)
    headers = [line for line in a.getvalue().decode().split('\n')[0::4] if line]
    with_ref = [h[1:].split(' ')[0] for h in headers if 'strand,' in h]
    assert set(with_ref) <= set(firsts)                  # every read with reference bases has a record (measured: all 76 of them)
    if max_batch == 7:
        assert len(firsts) >= 10


def test_brx_emit_paf_abi(tmp_path):
    import ctypes
    from badread_amd import engine as E
    from badread_amd.alignment import load_alignments
    from pyoracle import align
    pref, seqs = small_ref()
    eng = EE.EmuEngine(1 << 28)
    H.configure(eng, pref, 'nanopore2023', 'nanopore2023', H.SimParams(frag_mean=400, frag_stdev=300))
    got = ctypes.c_size_t(0)
    buf = eng.torch.zeros(1, dtype=eng.torch.uint8)
    assert eng.lib.brx_emit_paf(eng.ctx, ctypes.c_void_p(buf.data_ptr()), 1, None, ctypes.byref(got), None) == -6                      # BRX_E_STATE: no batch yet
    fastq, st = eng.simulate_batch(21, 0, 48)
    rc = eng.lib.brx_emit_paf(eng.ctx, ctypes.c_void_p(buf.data_ptr()), 1, None, ctypes.byref(got), None)
    assert rc == E.E_OUTPUT
    need = int(eng.lib.brx_output_needed(eng.ctx))
    assert need > 1
    full = eng.torch.zeros(need, dtype=eng.torch.uint8)
    off = eng.torch.zeros(49, dtype=eng.torch.int64)
    rc = eng.lib.brx_emit_paf(eng.ctx, ctypes.c_void_p(full.data_ptr()), need, ctypes.c_void_p(off.data_ptr()), ctypes.byref(got), None)
    assert rc == 0 and got.value == need and int(off[-1]) == need
    paf, off2 = eng.emit_paf_device(48)
    assert bytes(paf.numpy()) == bytes(full.numpy()) and list(off2) == [int(x) for x in off]
    path = tmp_path / 'x.paf'
    path.write_bytes(bytes(full.numpy()))
    names, reads = parse_fastq_names(fastq[:int(st['rec_off'][-1] + st['rec_len'][-1])])
    read_of = dict(zip(names, reads))
    seqs_by_name = dict(seqs)
    alns = load_alignments(str(path), output=io.StringIO())
    assert len(alns) >= 10
    for a in alns:
        t = seqs_by_name[a.ref_name][a.ref_start:a.ref_end]
        if a.strand == '-':
            t = revcomp(t)
        d, _ = align(read_of[a.read_name][a.read_start:a.read_end].encode(), t.encode(), want_ops=False)
        assert a.num_bases - a.matching_bases == d        # NM: every column that is not '='
    # after brx_align_batch the arena holds something else
    eng.align_batch([b'ACGTACGT'], [b'ACGTTACGT'])
    rc = eng.lib.brx_emit_paf(eng.ctx, ctypes.c_void_p(full.data_ptr()), need, None, ctypes.byref(got), None)
    assert rc == -6


def test_truth_paf_missing_directory_is_an_error(tmp_path):
    import subprocess
    r = subprocess.run([sys.executable, '-m', 'badread_amd', 'simulate', '--reference', SMALL_REF, '--quantity', '1x',
                        '--truth-paf', str(tmp_path / 'nope' / 'x.paf')], capture_output=True, text=True,
                       cwd=os.path.dirname(HERE))
    assert r.returncode == 1 and r.stderr.startswith('Error: ') and 'truth-paf' in r.stderr


PAF_FAIL_WORKER = r'''
import io, os, sys
sys.path[:0] = [{repo!r}, {repo!r} + '/oracle', {repo!r} + '/tests']
import emu_engine as EE
from badread_amd import simulate as S
from test_host_simulate import Args
S.DEFAULT_MAX_BATCH = 8
shard = S.Shard.from_env()
try:
    S.simulate(Args(quantity='60x', truth_paf='/dev/full'), output=io.StringIO(), engine=EE.EmuEngine(1 << 26), stdout=io.BytesIO(),
               shard=shard)
except OSError as ex:
    assert shard.rank == 0 and ex.errno == 28
    open({marker!r} + '.0', 'w').write('oserror')
except SystemExit as ex:
    assert shard.rank != 0 and 'rank 0' in str(ex.code)
    open({marker!r} + '.%d' % shard.rank, 'w').write('exit')
else:
    raise AssertionError('the run went on after its PAF file had failed')
'''


@pytest.mark.skipif(not os.path.exists('/dev/full'), reason='needs /dev/full (a file whose writes fail with ENOSPC)')
def test_a_failed_truth_paf_file_stops_every_rank_at_the_same_batch(tmp_path):
    """A PAF file that fails on rank 0 mid-run is reported in the per-batch exchange like a failed FASTQ sink: rank 0 raises its
    error and the other ranks exit with a message at the same batch, instead of the job writing on to its end."""
    from test_host_simulate import _free_port, _torchrun
    marker = str(tmp_path / 'stopped')
    script = tmp_path / 'worker.py'
    script.write_text(PAF_FAIL_WORKER.format(repo=os.path.dirname(HERE), marker=marker))
    r = _torchrun(script, 2, _free_port(), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(marker + '.0').read() == 'oserror' and open(marker + '.1').read() == 'exit'
