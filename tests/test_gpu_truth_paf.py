"""
GPU: --truth-paf on the MI355X.  The emulated-device checks of tests/test_truth_paf.py on the HIP engine (exact PAF at 100 %
identity, properties of errorful records), the command line (PAF independent of streams, batch sizes and ranks; FASTQ
unchanged by the flag), the round trip through the model builders, and the builders' text on a 60x truth PAF against the plain
restatement of the reference's counting loops.
"""
import collections
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import test_truth_paf as T

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SMALL_REF = T.SMALL_REF


def test_truth_paf_is_exact_at_full_identity_on_the_gpu():
    pref, _ = T.small_ref()
    eng = H.configure(H.hip_engine(), pref, 'nanopore2023', 'nanopore2023', T.full_identity_params())
    feats = T.check_full_identity(eng, pref, 11, 400)
    assert all(v >= 1 for v in feats.values()), feats


def test_truth_paf_records_of_errorful_reads_on_the_gpu():
    pref, seqs = T.small_ref()
    eng = H.hip_engine()
    fastq, st, paf, plans = T.errorful_batch(eng, pref, 5, 512)
    frac = T.check_errorful(dict(seqs), fastq, st, paf, plans, list(pref.names), {n: int(x) for n, x in zip(pref.names, pref.lengths)})
    print('truth_paf_ref_fraction', frac)
    assert frac >= 0.99, frac


def run_cli(tmp_path, name, *extra, quantity='15x', length='400,300'):
    paf = tmp_path / (name or 'unused.paf')
    cmd = [sys.executable, '-m', 'badread_amd', 'simulate', '--reference', SMALL_REF, '--quantity', quantity,
           '--length', length, '--seed', '11'] + list(extra)
    if name:
        cmd += ['--truth-paf', str(paf)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, (paf.read_bytes() if name else None)


def test_truth_paf_from_the_cli(tmp_path):
    plain, _ = run_cli(tmp_path, None, quantity='40x')
    fq, paf = run_cli(tmp_path, 'a.paf', quantity='40x')
    assert fq == plain and paf.count(b'\n') > 100
    for i, extra in enumerate((['--gpu-streams', '1'], ['--gpu-streams', '6', '--gpu-batch', '64'], ['--gpu-batch', '200'])):
        fq2, paf2 = run_cli(tmp_path, f'b{i}.paf', *extra, quantity='40x')
        assert fq2 == plain and paf2 == paf, extra
    names, _ = T.parse_fastq_names(plain)
    pos = {n: j for j, n in enumerate(names)}
    firsts = [line.split(b'\t')[0].decode() for line in paf.splitlines()]
    assert [pos[n] for n in firsts] == sorted(pos[n] for n in firsts)


def test_truth_paf_of_two_ranks_on_one_gpu(tmp_path):
    import test_gpu_cli as C
    import test_host_simulate as THS
    single_fq, single = run_cli(tmp_path, 'single.paf', quantity='40x')
    paf = tmp_path / 'ranks.paf'
    out = C._launch_ranks(tmp_path, 2, ['--truth-paf', str(paf)], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'))
    assert open(out, 'rb').read() == single_fq and paf.read_bytes() == single
    prefix = str(tmp_path / 'shard')
    spaf = str(tmp_path / 'shard.paf')
    C._launch_ranks(tmp_path, 2, ['--output-shards', prefix, '--truth-paf', spaf], dict(BRX_DIST_BACKEND='gloo', BRX_DEVICE='0'),
                    out_name='unused.fastq')
    got, _ = THS.reassemble(prefix, 2)
    assert got == single_fq
    names, _ = T.parse_fastq_names(got)
    pos = {n: j for j, n in enumerate(names)}
    lines = []
    for r in range(2):
        lines += open(f'{spaf}.{r}', 'rb').read().splitlines(keepends=True)
    lines.sort(key=lambda line: pos[line.split(b'\t')[0].decode()])          # stable: a read's records keep their order
    assert b''.join(lines) == single


def test_truth_paf_builds_models(tmp_path):
    """Round trip: the truth PAF of simulated reads feeds the model builders, and the error model they build from it comes back
    close to the one the reads were simulated with."""
    from badread_amd.error_model import ErrorModel
    # (--length 3000,1500 draws fragments that none of small_ref's short contigs can give often enough: NOFRAG)
    fq, paf = run_cli(tmp_path, 'rt.paf', quantity='300x', length='1000,500')
    (tmp_path / 'rt.fastq').write_bytes(fq)
    args = ['--reference', SMALL_REF, '--reads', str(tmp_path / 'rt.fastq'), '--alignment', str(tmp_path / 'rt.paf')]
    for kind in ('error_model', 'qscore_model'):
        r = subprocess.run([sys.executable, '-m', 'badread_amd', kind] + args, cwd=REPO, capture_output=True, timeout=900)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert len(r.stdout.splitlines()) > 10
        (tmp_path / f'{kind}.txt').write_bytes(r.stdout)
    built = ErrorModel(str(tmp_path / 'error_model.txt'), io.StringIO(), use_cache=False)
    ref = ErrorModel('nanopore2023', io.StringIO())
    b = dict(zip(built._kmers, (p[0] for p in built._probs)))
    a = dict(zip(ref._kmers, (p[0] for p in ref._probs)))
    _, seqs = T.small_ref()
    counts = collections.Counter(s[i:i + 7] for _, s in seqs for i in range(len(s) - 6))
    top = [km for km, _ in counts.most_common() if set(km) <= set('ACGT') and km in b][:50]
    assert len(top) == 50
    diff = max(abs(a[km] - b[km]) for km in top)
    print('truth_paf_model_max_diff', diff)
    # tolerance set from one run on the MI355X: max |difference| 0.219 (a 3.6 kb reference sees each of these 7-mers only a
    # few hundred times over the job, so the built probabilities are noisy); 0.3 leaves room for that noise, not for a bias
    assert diff < 0.3, diff


def test_truth_paf_models_equal_the_restatement_at_scale(tmp_path):
    """The builder commands on a truth PAF of 60x: thousands of windows per key, '-' strands, and reads with several records of which
    the loader keeps one.  Their stdout (the commands' default arguments) equals the text the plain restatement
    (oracle/model_builder_ref.py) gives for the same files, read through the product's loaders."""
    sys.path.insert(0, os.path.join(REPO, 'oracle'))
    import model_builder_ref as R
    from badread_amd.alignment import load_alignments
    from badread_amd.misc import load_fasta, load_fastq, reverse_complement
    fq, paf = run_cli(tmp_path, 'sc.paf', quantity='60x', length='1000,500')
    (tmp_path / 'sc.fastq').write_bytes(fq)
    files = dict(reference=SMALL_REF, reads=str(tmp_path / 'sc.fastq'), alignment=str(tmp_path / 'sc.paf'))
    refs = load_fasta(files['reference'])[0]
    reads = load_fastq(files['reads'], output=io.StringIO())
    al = load_alignments(files['alignment'], None, output=io.StringIO())
    records = collections.Counter(line.split(b'\t')[0] for line in paf.splitlines())
    assert len(al) > 100 and {a.strand for a in al} == {'+', '-'} and max(records.values()) > 1 and len(al) < sum(records.values())
    want = {'error_model': R.error_model_text(refs, reads, al, 7, 25, reverse_complement),
            'qscore_model': R.qscore_model_text(refs, reads, al, 9, 6, 100, 10000, reverse_complement)}
    args = [x for key, value in files.items() for x in ('--' + key, value)]
    for kind in ('error_model', 'qscore_model'):
        r = subprocess.run([sys.executable, '-m', 'badread_amd', kind] + args, cwd=REPO, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        got = r.stdout.decode()
        print('truth_paf_scale', kind, dict(alignments=len(al), lines=got.count('\n'), first_diff=next((i for i, (x, y) in enumerate(zip(got, want[kind])) if x != y), -1)))
        assert got == want[kind], kind


# ---------------------------------------------------------------------------------------------------------------------------------
# one full device batch of configs[3] at the shipped geometry (tests/test_gpu_fullsize.py builds it the same way): long reads,
# many 64-column steps and records per read, every band class and route of the final stage, k_truth_scan over 65 536 reads

_CIGAR = re.compile(rb'(\d+)([MID])')


class _PackedSeq(object):
    """Reference symbols straight from the packed genome (numpy), N runs and other exceptions as the packed reference holds them."""

    def __init__(self, pref):
        self.pref = pref
        self.packed = np.asarray(pref.packed)
        self.sym = np.asarray(pref.sym, dtype=np.uint8)
        self.comp = np.asarray(pref.comp, dtype=np.uint8)
        self.ex = np.asarray(pref.exceptions)

    def target(self, contig, ts, te, minus):
        """Symbols of the read's strand string over forward [ts, te): reverse complement for '-'."""
        ct = self.pref.contigs[contig]
        g = int(ct['base_off']) + np.arange(ts, te, dtype=np.uint64)
        codes = ((self.packed[(g >> np.uint64(4)).astype(np.int64)] >> (2 * (g & np.uint64(15))).astype(np.uint32)) & 3).astype(np.uint8)
        g0, g1 = int(ct['base_off']) + ts, int(ct['base_off']) + te
        for e in self.ex:
            if int(e['start']) < g1 and int(e['end']) > g0:
                lo, hi = max(int(e['start']), g0) - g0, min(int(e['end']), g1) - g0
                codes[lo:hi] = int(e['code'])
        if minus:
            codes = self.comp[codes][::-1]
        return self.sym[codes]


def _walk(parts, q, t):
    """(= columns, NM) of a CIGAR in column order over query q and target t (uint8 symbols)."""
    lens = np.array([n for n, _ in parts], dtype=np.int64)
    ops = np.array([x for _, x in parts])
    m, i, d = ops == 'M', ops == 'I', ops == 'D'
    qadv, tadv = lens * (m | i), lens * (m | d)
    q0, t0 = np.cumsum(qadv) - qadv, np.cumsum(tadv) - tadv
    ml = lens[m]
    within = np.arange(int(ml.sum())) - np.repeat(np.cumsum(ml) - ml, ml)
    eq = int((q[np.repeat(q0[m], ml) + within] == t[np.repeat(t0[m], ml) + within]).sum())
    return eq, int(ml.sum()) - eq + int(lens[i].sum()) + int(lens[d].sum())


def test_truth_paf_of_a_full_configs3_batch():
    import bench
    from badread_amd.engine import HipEngine
    from pyoracle import OracleEngine, align
    n, seed = 65536, 42
    wl = bench.build_workload(io.StringIO(), 'human', bench.default_ref_dir())
    pref = wl[0]
    eng = bench.configure(HipEngine(0, scratch_bytes=int(bench.SCRATCH_GB_DEFAULT * (1 << 30))), wl)
    out, st = eng.simulate_batch(seed, 0, n)
    out, st = out.copy(), st.copy()
    route = eng.read_cycles(n)[:, 7] & np.uint64(0x3FFFF)            # words per lane | four per wave | one per lane
    paf_t, off = eng.emit_paf_device(n)
    paf = bytes(paf_t.cpu().numpy())
    eng.close()
    assert len(off) == n + 1 and int(off[0]) == 0 and int(off[-1]) == len(paf) and (np.diff(off.astype(np.int64)) >= 0).all()
    orc = bench.configure(OracleEngine(), wl)
    ref = _PackedSeq(pref)
    names = list(pref.names)
    cidx = {nm: j for j, nm in enumerate(names)}
    raw = np.frombuffer(out, dtype=np.uint8)
    # a fixed sample of >= 2000 reads for the NM-optimality check: up to 200 of every route (band words x kernel), then every k-th read
    keys = collections.defaultdict(list)
    for r in range(n):
        if st['rec_len'][r]:
            keys[int(route[r])].append(r)
    sample = set()
    for rs in keys.values():
        sample.update(rs[:200])
    live = [r for rs in keys.values() for r in rs]
    sample.update(sorted(live)[::max(len(live) // 1500, 1)])
    assert len(sample) >= 2000 and len(keys) >= 4, (len(sample), sorted(keys))
    covered = ref_bases = n_records = n_aligned = no_record = 0
    for r in range(n):
        chunk = paf[int(off[r]):int(off[r + 1])]
        if not st['rec_len'][r]:
            assert not chunk
            continue
        rec = raw[int(st['rec_off'][r]):int(st['rec_off'][r]) + int(st['rec_len'][r])]
        L = int(st['seq_len'][r])
        hdr = int(st['rec_len'][r]) - 2 * L - 4
        name = bytes(rec[1:hdr]).split(b' ')[0]
        read = rec[hdr:hdr + L]
        plan = orc.plan(seed, r)
        segs = [[int(x) for x in s] for s in plan['segs']]
        ref_bases += sum(s[4] for s in segs if s[0] == 0)
        merged = []                                          # neighbours that continue each other (a glitch of no size and no skip)
        for s in segs:
            if merged and s[0] == 0 and merged[-1][0] == 0 and merged[-1][1:3] == s[1:3] and merged[-1][3] + merged[-1][4] == s[3]:
                merged[-1][4] += s[4]
            else:
                merged.append(list(s))
        lines = chunk.split(b'\n')
        assert lines[-1] == b'', r
        lines = lines[:-1]
        if not lines:                                        # only a read with (almost) no reference bases has no record
            assert sum(s[4] for s in segs if s[0] == 0) < 50, (r, segs)
            no_record += 1
        assert sum(1 for f in lines if b'\ttp:A:P\t' in f) == (1 if lines else 0), r
        last_qe = 0
        for line in lines:
            f = line.split(b'\t')
            assert len(f) == 16 and f[0] == name and int(f[1]) == L and f[11] == b'60', (r, f[:12])
            qs, qe, ts, te = int(f[2]), int(f[3]), int(f[7]), int(f[8])
            assert last_qe <= qs < qe <= L, (r, f[:12])             # in increasing qstart, no overlap
            last_qe = qe
            contig, minus = cidx[f[5].decode()], f[4] == b'-'
            clen = int(pref.contigs[contig]['length'])
            assert int(f[6]) == clen and 0 <= ts < te <= clen, (r, f[:12])
            parts = [(int(a), b.decode()) for a, b in _CIGAR.findall(f[13][5:])]
            if minus:
                parts = parts[::-1]
            assert parts[0][1] == 'M' and parts[-1][1] == 'M' and sum(a for a, _ in parts) == int(f[10])
            assert sum(a for a, x in parts if x != 'D') == qe - qs and sum(a for a, x in parts if x != 'I') == te - ts, (r, f[:12])
            t = ref.target(contig, ts, te, minus)
            eq, nm = _walk(parts, read[qs:qe], t)
            n_eq, rec_nm = int(f[9]), int(f[14][5:])
            assert int(f[15][5:]) == n_eq - rec_nm
            n_N = int((t == ord('N')).sum())
            # where the reference has an N the fragment carries the packed reference's stand-in base: a '=' may stand against it
            assert (eq == n_eq and nm == rec_nm) if not n_N else (0 <= n_eq - eq <= n_N and 0 <= nm - rec_nm <= n_N), (r, f[:12])
            strand = 1 if minus else 0
            assert any(s[0] == 0 and s[1] == contig and s[2] == strand and
                       ((s[3] <= ts and te <= s[3] + s[4]) if not minus else (clen - s[3] - s[4] <= ts and te <= clen - s[3]))
                       for s in merged), (r, f[:12])
            if r in sample and not n_N:
                dist, _ = align(bytes(read[qs:qe]), bytes(t), want_ops=False)
                assert rec_nm == dist, (r, f[:12], rec_nm, dist)
                n_aligned += 1
            covered += te - ts
            n_records += 1
    frac = covered / ref_bases
    print('truth_paf_full_batch', dict(records=n_records, aligned=n_aligned, sample=len(sample), routes=len(keys), no_record=no_record,
                                       ref_fraction=round(frac, 6), paf_bytes=len(paf)))
    assert n_records > 100000 and n_aligned >= 2000
    assert frac >= 0.99, frac

