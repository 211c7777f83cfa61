"""
TEST INFRASTRUCTURE: the window identities of `badread plot` (README, "Window identities"; include/brx.h: brx_window_means) restated in
plain Python from their definition, the fixture recorded from the running reference (tests/golden/plot_windows.json.gz, written by
tools/make_plot_golden.py), synthetic jobs at the shapes where each kernel can go wrong, and one check_* function per property.  Every
check takes the engine as its argument: tests/test_plot.py passes the interpreted kernels (tests/emu_engine.py), tests/test_gpu_plot.py
the MI355X.  Nothing here has a tolerance: the device returns integers and the doubles made from them are the reference's bit for bit.
"""
import functools
import gzip
import hashlib
import io
import json
import os

import numpy as np
import pytest

import model_jobs as MJ
from badread_amd import plot_window_identity as P
from badread_amd.alignment import Alignment, load_alignments
from badread_amd.engine import DEPTH_TILE
from badread_amd.misc import load_fasta, load_fastq, reverse_complement
from badread_amd.model_builder import Job

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, 'golden', 'model_builder')
FILES = {'reference': os.path.join(INPUTS, 'ref.fasta'), 'reads': os.path.join(INPUTS, 'reads.fastq'), 'alignment': os.path.join(INPUTS, 'aln.paf')}
FILE_ARGS = [x for k, v in FILES.items() for x in ('--' + k, v)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
class TrailingDeletion(Exception):
    pass


def errors_per_position(read, ref, parts):
    """E[0..L): the walk of the definition over the parts in read order."""
    errors = [0] * len(read)
    rp = fp = 0
    for n, t in parts:
        if t == 'M':
            for i in range(n):
                errors[rp + i] += read[rp + i] != ref[fp + i]
            rp, fp = rp + n, fp + n
        elif t == 'I':
            for i in range(n):
                errors[rp + i] += 1
            rp += n
        elif t == 'D':
            if rp == len(read):
                raise TrailingDeletion()
            errors[rp] += n
            fp += n
    return errors


def window_sums(values, window):
    """S[i] = values[i] + .. + values[i + W - 1] for 0 <= i < max(L - W, 0): the last window is left out"""
    return [sum(values[i:i + window]) for i in range(max(len(values) - window, 0))]


def restate(slices, window, read_start):
    """Everything the definition names for one alignment (slices: an entry of Job.slices)."""
    read, qual, ref, parts = slices
    S = window_sums(errors_per_position(read, ref, parts), window)
    Q = window_sums([ord(c) - 33 for c in qual[:len(read)]], window)
    n = len(S)
    out = dict(n=n, S=S, Q=Q, positions=[read_start + i + window // 2 for i in range(n)],
               identities=[100.0 * (1.0 - s / window) for s in S], qualities=[q / window for q in Q])
    if n:
        out.update(Smin=min(S), Smax=max(S), imax=S.index(max(S)), Stot=sum(S), Qmin=min(Q), Qmax=max(Q), Qtot=sum(Q))
    else:
        out.update(Smin=0, Smax=0, imax=0, Stot=0, Qmin=0, Qmax=0, Qtot=0)
    return out


def expected_summary(job3, window, qual):
    """The text of --summary from the restatement."""
    refs, reads, alignments = job3
    cols = ['read_name', 'read_length', 'read_start', 'read_end', 'strand', 'ref_name', 'ref_start', 'ref_end', 'alignment_identity', 'windows',
            'min_identity', 'min_position', 'max_identity', 'mean_identity'] + (['min_quality', 'max_quality', 'mean_quality'] if qual else [])
    lines = ['#' + '\t'.join(cols)]
    for a, sl in zip(alignments, Job(refs, reads, alignments).slices):
        r = restate(sl, window, a.read_start)
        f = [a.read_name, str(len(reads[a.read_name][0])), str(a.read_start), str(a.read_end), a.strand, a.ref_name, str(a.ref_start), str(a.ref_end),
             '%.3f' % a.percent_identity, str(r['n'])]
        if r['n'] == 0:
            f += ['NA'] * (len(cols) - len(f))
        else:
            f += ['%.3f' % (100.0 * (1.0 - r['Smax'] / window)), str(a.read_start + r['imax'] + window // 2),
                  '%.3f' % (100.0 * (1.0 - r['Smin'] / window)), '%.3f' % (100.0 * (1.0 - r['Stot'] / (window * r['n'])))]
            if qual:
                f += ['%.3f' % (r['Qmin'] / window), '%.3f' % (r['Qmax'] / window), '%.3f' % (r['Qtot'] / (window * r['n']))]
        lines.append('\t'.join(f))
    return '\n'.join(lines) + '\n'


def digest(values):
    return hashlib.sha256(np.asarray(values, dtype='<f8').tobytes()).hexdigest()


# ---- the fixture and its inputs --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    with gzip.open(os.path.join(HERE, 'golden', 'plot_windows.json.gz'), 'rt') as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def inputs():
    """(refs, reads, alignments) of the committed files, through the product's loaders."""
    null = io.StringIO()
    return load_fasta(FILES['reference'])[0], load_fastq(FILES['reads'], output=null), load_alignments(FILES['alignment'], output=null)


def case(window, qual):
    return next(c for c in fixture()['cases'] if c['window'] == window and c['qual'] == qual)


# ---- synthetic jobs --------------------------------------------------------------------------------------------------------------------
class Synth(object):
    """Alignments built from PAF lines (no file, so the loader's filters do not apply) on one contig that grows with them."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.ref, self.ref_len, self.reads, self.lines = [], 0, {}, []

    def dna(self, n):
        return ''.join(np.array(list('ACGT'))[self.rng.integers(0, 4, n)]) if n else ''

    def add(self, parts, strand='+', read_len=None, sub=0.1, qual=None, start=0, errors_at=None):
        """A read along `parts` (read order) over a new stretch of the contig; M columns differ at rate `sub`, or exactly at the read
        positions `errors_at`.  read_len: the length of the read slice [start, start + read_len), longer than the CIGAR's if given."""
        used_read = sum(n for n, t in parts if t != 'D')
        used_ref = sum(n for n, t in parts if t != 'I')
        target = self.dna(used_ref)                                 # in the read's orientation
        read, tp = [], 0
        for n, t in parts:
            if t == 'M':
                piece = list(target[tp:tp + n])
                rp = sum(len(x) for x in read)
                for i in range(n):
                    if (rp + i in errors_at) if errors_at is not None else self.rng.random() < sub:
                        piece[i] = 'ACGT'[('ACGT'.index(piece[i]) + 1) % 4]
                read.append(''.join(piece))
            elif t == 'I':
                read.append(self.dna(n))
            if t != 'I':
                tp += n
        read = ''.join(read)
        read_len = used_read if read_len is None else read_len
        seq = self.dna(start) + read + self.dna(read_len - used_read) + self.dna(2)
        q = qual if qual is not None else ''.join(map(chr, self.rng.integers(33, 127, len(seq)).tolist()))
        q = (q * (len(seq) // max(len(q), 1) + 1))[:len(seq)]
        fwd = target if strand == '+' else reverse_complement(target)
        name = f's{len(self.reads)}'
        self.reads[name] = (seq, q)
        cigar = ''.join(f'{n}{t}' for n, t in (parts if strand == '+' else parts[::-1]))
        self.lines.append('\t'.join([name, str(len(seq)), str(start), str(start + read_len), strand, 'ctg', '0', str(self.ref_len),
                                     str(self.ref_len + len(fwd)), '1', str(max(sum(n for n, _ in parts), 1)), '60', 'AS:i:0', f'cg:Z:{cigar}']))
        self.ref.append(fwd)
        self.ref_len += len(fwd)
        return self

    def job(self):
        return {'ctg': ''.join(self.ref)}, self.reads, [Alignment(line) for line in self.lines]


@functools.lru_cache(maxsize=None)
def synthetic_jobs():
    """name -> ((refs, reads, alignments), windows): the shapes at which each kernel can go wrong."""
    t = DEPTH_TILE
    jobs = {}
    # read lengths around the scan's tile; together the read bases cross three tiles, and every alignment begins inside another tile
    jobs['tiles'] = (Synth(1).add([(t - 1, 'M')]).add([(t, 'M')], '-').add([(t // 2, 'M'), (3, 'D'), (t - t // 2 + 1, 'M')]).job(),
                     (1, 2, 100, t - 2, t - 1, t, t + 1))
    s = Synth(2)
    s.add([(4, 'D'), (40, 'M')])                                     # begins with D
    s.add([(20, 'M'), (5, 'D'), (3, 'I'), (20, 'M')])                # D directly before I
    s.add([(20, 'M'), (5, 'D'), (3, 'I'), (20, 'M')], '-')           # ... on '-': I directly before D in read order
    s.add([(20, 'M'), (2, 'D'), (7, 'D'), (20, 'M')])                # two consecutive D parts
    s.add([(3, 'D'), (2, 'D'), (1, 'I'), (4, 'D'), (9, 'M')])        # D D I D M
    s.add([(30, 'M')], read_len=45)                                  # a CIGAR shorter than its read slice
    s.add([(30, 'M'), (6, 'D')], read_len=45, start=3)               # ... and a trailing D there: it lands on the first base behind
    s.add([(30, 'M'), (6, 'D'), (2, 'D')], read_len=31)              # ... on the slice's last base
    s.add([(10, 'M'), (3, 'D'), (0, 'M'), (2, 'I'), (10, 'M')])      # an empty part between a deletion and the base it lands on
    s.add([(1, 'M')])                                                # one column
    s.add([(1, 'M')], sub=1.0)
    jobs['parts'] = (s.job(), (1, 2, 3, 9, 30, 44, 45, 46))
    # one alignment of L = 50: W = 1, L - 1 (one window), L and L + 1 (none)
    jobs['window_sizes'] = (Synth(3).add([(25, 'M'), (1, 'I'), (24, 'M')]).job(), (1, 49, 50, 51))
    # a deletion of 70 000: window sums beyond 16 bits
    jobs['long_deletion'] = (Synth(4).add([(150, 'M'), (70000, 'D'), (150, 'M')]).add([(300, 'M')]).job(), (1, 100, 299))
    # equal maxima: two lone errors 150 apart give two plateaus of W windows each; the first window of the first one is the answer
    jobs['plateau'] = (Synth(5).add([(600, 'M')], errors_at={50, 200}).add([(600, 'M')], errors_at=set()).add([(700, 'M')], errors_at={699, 0}).job(),
                       (1, 10, 100, 256, 300))
    # quality bytes below '!' and above '~': q from -33 to 222
    odd = ''.join(map(chr, [0, 5, 32, 33, 126, 127, 160, 255]))
    jobs['odd_qualities'] = (Synth(6).add([(300, 'M')], qual=odd).add([(100, 'M'), (2, 'I'), (98, 'M')], '-', qual='\x00\xff\xff').job(), (1, 3, 100))
    jobs['edges'] = (MJ.job('edges'), (1, 100))
    jobs['mixed'] = (MJ.job('mixed', n_align=40), (1, 33, 100))
    jobs['none'] = (({'ctg': 'ACGT'}, {}, []), (1, 100))
    return jobs


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def product(engine, job3, window, qual, values=True):
    refs, reads, alignments = job3
    return list(P.window_means(engine, refs, reads, alignments, window, qual, values=values))


def assert_stat(stat, r, qual, where):
    got = tuple(int(stat[k]) for k in ('n', 'err_min', 'err_max', 'err_argmax', 'err_total'))
    assert got == (r['n'], r['Smin'], r['Smax'], r['imax'], r['Stot']), where
    got = tuple(int(stat[k]) for k in ('qual_min', 'qual_max', 'qual_total'))
    assert got == ((r['Qmin'], r['Qmax'], r['Qtot']) if qual else (0, 0, 0)), where


def check_against_restatement(engine, job3, windows):
    """Stats and values of the product == the restatement's, for every window size, with qualities and once without."""
    refs, reads, alignments = job3
    slices = Job(refs, reads, alignments).slices
    for window in windows:
        for qual in ((True, False) if window == windows[0] else (True,)):
            got = product(engine, job3, window, qual)
            assert len(got) == len(alignments)
            for k, (a, (stat, err_sum, qual_sum)) in enumerate(zip(alignments, got)):
                r = restate(slices[k], window, a.read_start)
                where = (k, repr(a), window, qual)
                assert err_sum.tolist() == r['S'], where
                assert (qual_sum.tolist() == r['Q']) if qual else qual_sum is None, where
                assert_stat(stat, r, qual, where)
            if window == windows[0]:                                # without the values the stats are the same
                for (stat, _, _), (stat2, err_sum, qual_sum) in zip(got, product(engine, job3, window, qual, values=False)):
                    assert stat2 == stat and err_sum is None and qual_sum is None


def check_restatement_against_fixture():
    """The restatement on the committed inputs == what the running reference gave: n, position[0], the digests, the full lists."""
    refs, reads, alignments = inputs()
    fx = fixture()
    assert [repr(a) for a in alignments] == fx['names']
    slices = Job(refs, reads, alignments).slices
    for c in fx['cases']:
        for a, sl, row in zip(alignments, slices, c['alignments']):
            r = restate(sl, c['window'], a.read_start)
            assert (r['n'], r['positions'][0] if r['n'] else None) == (row['n'], row['position0'])
            assert digest(r['identities']) == row['identities']
            assert row['qualities'] is None or digest(r['qualities']) == row['qualities']
    assert len(fx['full']) == 3
    for full in fx['full']:
        a, r = alignments[full['index']], restate(slices[full['index']], full['window'], alignments[full['index']].read_start)
        assert r['positions'] == full['positions']
        assert r['identities'] == [float(x) for x in full['identities']] and r['qualities'] == [float(x) for x in full['qualities']]
    assert P.get_window_means([0, 3, 1, 0, 2], 2, 10) == ([11, 12, 13], [-50.0, -100.0, 50.0])
    assert P.get_window_means([4, 8, 2], 2, 0, convert_to_identity=False) == ([1], [6.0]) and P.get_window_means([1], 5, 0) == ([], [])


def check_fixture(engine, windows=None):
    """The product on the committed inputs, turned into doubles, == the reference's digests; its stats == those of the same values."""
    fx = fixture()
    for window in windows or fx['windows']:
        rows = case(window, True)['alignments']
        got = product(engine, inputs(), window, True)
        assert len(got) == len(rows)
        for a, row, (stat, err_sum, qual_sum) in zip(inputs()[2], rows, got):
            assert (int(stat['n']), len(err_sum), len(qual_sum)) == (row['n'],) * 3
            assert digest(P.identities_of(err_sum, window)) == row['identities'] and digest(P.qualities_of(qual_sum, window)) == row['qualities']
            if row['n']:
                assert a.read_start + window // 2 == row['position0']
                S, Q = err_sum.astype(np.int64), qual_sum.astype(np.int64)
                want = (int(S.min()), int(S.max()), int(np.argmax(S)), int(S.sum()), int(Q.min()), int(Q.max()), int(Q.sum()))
            else:
                want = (0,) * 7
            assert tuple(int(stat[k]) for k in ('err_min', 'err_max', 'err_argmax', 'err_total', 'qual_min', 'qual_max', 'qual_total')) == want
    for full in fx['full']:                                            # the doubles themselves, for the three recorded alignments
        stat, err_sum, qual_sum = product(engine, (inputs()[0], inputs()[1], [inputs()[2][full['index']]]), full['window'], True)[0]
        assert P.identities_of(err_sum, full['window']).tolist() == [float(x) for x in full['identities']]
        assert P.qualities_of(qual_sum, full['window']).tolist() == [float(x) for x in full['qualities']]


def check_chunking(engine, monkeypatch):
    """PLOT_CHUNK_BASES = 1 (one alignment per call) and a value between give what one call gives."""
    job3 = synthetic_jobs()['mixed'][0]
    calls = []
    inner = engine.window_means
    monkeypatch.setattr(engine, 'window_means', lambda job, *a, **k: calls.append(job.n_align) or inner(job, *a, **k), raising=False)
    results = {}
    for limit in (1 << 40, 1, 1500):
        monkeypatch.setattr(P, 'PLOT_CHUNK_BASES', limit)
        del calls[:]
        results[limit] = [(s.tolist(), e.tolist(), q.tolist()) for s, e, q in product(engine, job3, 33, True)]
        n = len(job3[2])
        assert sum(calls) == n and (calls == [n] if limit > 1500 else calls == [1] * n if limit == 1 else 1 < len(calls) < n)
    assert results[1] == results[1 << 40] == results[1500]


def check_abi(engine, monkeypatch):
    """The error codes of brx_window_means: window 0, NULL arrays, a scratch that is too small; zero alignments are a valid call."""
    import ctypes
    from badread_amd import engine as E
    lib, call = engine.lib, lambda job: engine.lib.brx_window_means(engine.ctx, ctypes.byref(job), engine._stream())
    s = E.BrxWindowJob()
    assert call(s) == -1 and b'window 0' in lib.brx_last_error(engine.ctx)                 # BRX_E_ARG
    s.window = 5
    assert call(s) == 0                                                                   # no alignment: nothing to do
    s.n_align = 1
    assert call(s) == -1 and b'NULL' in lib.brx_last_error(engine.ctx)
    refs, reads, alignments = Synth(8).add([(30, 'M')]).job()
    job = Job(refs, reads, alignments)
    need = lib.brx_window_scratch(30, 1)
    assert need >= 30 * 4 + 2 * 31 * 8 and lib.brx_window_scratch(30, 0) < need
    real = lib.brx_window_scratch
    monkeypatch.setattr(lib, 'brx_window_scratch', lambda n_bases, qual: 16, raising=False)
    with pytest.raises(E.BrxError) as e:
        engine.window_means(job, 5, True)
    assert e.value.code == -3 and 'scratch too small' in str(e.value) and lib.brx_scratch_needed(engine.ctx) == need
    monkeypatch.setattr(lib, 'brx_window_scratch', real, raising=False)
    stats = engine.window_means(job, 5, True)[0]
    assert int(stats['n'][0]) == 25


class NoDevice(object):
    def window_means(self, *args, **kwargs):
        raise AssertionError('the device was called')


def check_trailing_deletion():
    """A D part with no read base behind it: the message of the definition, before anything is shipped (a good alignment comes first)."""
    s = Synth(7).add([(30, 'M')]).add([(30, 'M'), (6, 'D')])
    refs, reads, alignments = s.job()
    read, _, ref, parts = Job(refs, reads, alignments).slices[1]
    with pytest.raises(TrailingDeletion):
        errors_per_position(read, ref, parts)
    with pytest.raises(SystemExit) as e:
        list(P.window_means(NoDevice(), refs, reads, alignments, 10, False))
    assert str(e.value) == f'Error: the CIGAR of {alignments[1]!r} ends in a deletion with no read base after it'


CLI_CASES = ((100, False), (100, True), (5000, True))


def check_cli(run, tmp_path, chunked=None, cases=CLI_CASES):
    """run(argv) -> (exit status, stdout, message): the command line of `plot` on the committed inputs; with --no_plot the stdout is the
    reference's, whatever else is asked for, and --summary is the restatement's.  chunked(argv): the same with a small PLOT_CHUNK_BASES,
    where the caller can lower it."""
    for window, qual in cases:
        path = str(tmp_path / f'summary_{window}_{qual}.tsv')
        argv = FILE_ARGS + ['--no_plot', '--summary', path] + (['--window', str(window)] if window != 100 else []) + (['--qual'] if qual else [])
        status, out, _ = run(argv)
        assert status == 0 and out == case(window, qual)['stdout']
        text = open(path).read()
        assert text == expected_summary(inputs(), window, qual)
        if window == 5000:
            assert all(line.split('\t')[9:] == ['0'] + ['NA'] * 7 for line in text.splitlines()[1:]) and len(text.splitlines()) == 34
        if chunked is not None:
            os.remove(path)
            assert chunked(argv)[:2] == (0, out) and open(path).read() == text


def check_cli_errors(run, tmp_path):
    status, _, message = run(FILE_ARGS + ['--no_plot', '--window', '0'])
    assert status != 0 and message.strip() == 'Error: --window must be at least 1'
    missing = str(tmp_path / 'no_such_dir' / 'summary.tsv')
    status, _, message = run(FILE_ARGS + ['--no_plot', '--summary', missing])
    assert status != 0 and message.strip() == f'Error: the directory of --summary {missing} does not exist'


def check_cli_save(run, tmp_path):
    """--save: one PNG per alignment, named by its index and read name."""
    null = io.StringIO()
    kept = load_alignments(FILES['alignment'], 4, output=null)     # the first four PAF lines: three reads pass the filters
    assert len(kept) == 3
    folder = tmp_path / 'plots'
    status, out, message = run(FILE_ARGS + ['--max_alignments', '4', '--qual', '--save', str(folder)])
    assert status == 0, message
    assert sorted(os.listdir(folder)) == sorted(f'{i}_{a.read_name}.png' for i, a in enumerate(kept))
    for name in os.listdir(folder):
        with open(folder / name, 'rb') as f:
            assert f.read(8) == b'\x89PNG\r\n\x1a\n'
