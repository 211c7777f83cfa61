"""
SURVEY.md section 8f row f4: `badread error_model` / `badread qscore_model` on the device (badread_amd/model_builder.py,
csrc/brx_model.h, C-ABI brx_model_count) against tests/golden/model_builder.json.gz -- the text the REFERENCE's own
make_error_model (error_model.py:31-83) and make_qscore_model (qscore_model.py:78-162) print for the committed inputs
(tests/golden/model_builder/: reference, reads and PAF alignments made by tools/make_golden.py), seven argument sets.

  not gpu:  the oracle's plain-Python restatement (oracle/model_builder_ref.py) == the reference's text;
            the product kernels, interpreted on the CPU, == the reference's text; loader filters; spilled windows
  gpu:      the HIP kernels through the C-ABI == the reference's text, and the command line writes it to stdout

Below these: the merged TABLES (model_builder.count_error_model / count_qscore_model: key set, counts, earliest-window ranks) against
the restatement's error_table / qscore_table on the synthetic jobs of tests/model_jobs.py -- the printed text rounds counts to six
decimals, cuts rare entries and shows a rank only where two counts tie.  Every check is written once as a function of the engine
(check_*) and run on the interpreted kernels (not gpu) and on the HIP kernels (gpu): parity at both ends of the key's bit budget,
closed forms on one-key and two-key jobs (many atomics on one slot), the spill and regrow routes asserted from what the engine
returns, and tests/golden/model_builder_edges.json.gz, the reference's own text for a file form of the `edges` job.
"""
import collections
import gzip
import io
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import helpers as H  # noqa: F401  (sys.path)
import model_jobs as J

HERE = os.path.dirname(os.path.abspath(__file__))
FOLDER = os.path.join(HERE, 'golden', 'model_builder')
with gzip.open(os.path.join(HERE, 'golden', 'model_builder.json.gz'), 'rt') as _f:
    GOLDEN = json.load(_f)


def namespace(case):
    return types.SimpleNamespace(reference=os.path.join(FOLDER, 'ref.fasta'), reads=os.path.join(FOLDER, 'reads.fastq'),
                                 alignment=os.path.join(FOLDER, 'aln.paf'), **case)


def run_product(kind, case, engine):
    from badread_amd import model_builder as MB
    out = io.StringIO()
    fn = MB.make_error_model if kind == 'error' else MB.make_qscore_model
    fn(namespace(case), output=io.StringIO(), engine=engine, stdout=out)
    return out.getvalue()


def test_loader_keeps_the_best_alignment_per_read_and_drops_short_and_poor_ones():
    from badread_amd.alignment import load_alignments
    al = load_alignments(os.path.join(FOLDER, 'aln.paf'), output=io.StringIO())
    names = [a.read_name for a in al]
    assert 25 <= len(names) == len(set(names)) < 48 and 'read_short' not in names and 'read_bad' not in names      # the 17 %-error reads fall below 80 % identity
    assert all(a.num_bases > 100 and a.percent_identity > 80.0 for a in al)
    minus = [a for a in al if a.strand == '-']
    assert minus and all(a.cigar_parts == [(int(n), t) for n, t in __import__('re').findall(r'(\d+)(\w)', a.cigar)][::-1] for a in minus)
    assert len(load_alignments(os.path.join(FOLDER, 'aln.paf'), 5, output=io.StringIO())) <= 5


def test_oracle_restatement_reproduces_the_reference_text():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
    import model_builder_ref as R
    from badread_amd.alignment import load_alignments
    from badread_amd.misc import load_fasta, load_fastq, reverse_complement
    refs = load_fasta(os.path.join(FOLDER, 'ref.fasta'))[0]
    reads = load_fastq(os.path.join(FOLDER, 'reads.fastq'), output=io.StringIO())
    for entry in GOLDEN['error']:
        a = entry['args']
        al = load_alignments(os.path.join(FOLDER, 'aln.paf'), a['max_alignments'], output=io.StringIO())
        assert R.error_model_text(refs, reads, al, a['k_size'], a['max_alt'], reverse_complement) == entry['text'], a
    for entry in GOLDEN['qscore']:
        a = entry['args']
        al = load_alignments(os.path.join(FOLDER, 'aln.paf'), a['max_alignments'], output=io.StringIO())
        assert R.qscore_model_text(refs, reads, al, a['k_size'], a['max_del'], a['min_occur'], a['max_output'],
                                   reverse_complement) == entry['text'], a


@pytest.mark.parametrize('kind', ['error', 'qscore'])
def test_interpreted_kernels_reproduce_the_reference_text(kind):
    import emu_engine as EE
    eng = EE.EmuEngine(1 << 26)
    for entry in GOLDEN[kind]:
        assert run_product(kind, entry['args'], eng) == entry['text'], entry['args']


def test_windows_a_key_cannot_hold_are_counted_on_the_host():
    """The inputs hold 30-base insertions: read k-mers of more than 21 bases leave the 64-bit key (error model), and
    nothing may be lost or counted twice -- the text equality above covers it; here: the spill path really ran."""
    import emu_engine as EE
    from badread_amd import model_builder as MB
    from badread_amd.alignment import load_alignments
    from badread_amd.misc import load_fasta, load_fastq
    refs = load_fasta(os.path.join(FOLDER, 'ref.fasta'))[0]
    reads = load_fastq(os.path.join(FOLDER, 'reads.fastq'), output=io.StringIO())
    al = load_alignments(os.path.join(FOLDER, 'aln.paf'), output=io.StringIO())
    job = MB.Job(refs, reads, al)
    keys, counts, first, spill = EE.EmuEngine(1 << 26).model_count(0, job, 7, 0, 1, 18)
    assert len(spill) > 0 and int(counts.sum()) > 10000
    assert EE.EmuEngine(1 << 26).model_count(0, job, 7, 0, 1, 8) is None          # a 256-slot table is full: the caller grows it


def test_quality_characters_outside_the_phred_range_are_counted_like_the_reference(tmp_path):
    """A quality character below '!' (q < 0) or above chr(160) (q > 127) does not fit the 7 bits a key gives the score: k_mb_qscore
    hands such windows to the host with their size index in the spill word, and the host counts them with the reference's own
    arithmetic (qscore_model.py:137-138: ord(c) - 33, whatever it is).  Product (interpreted kernels) == the oracle's
    restatement == the reference's own text for these files (tests/golden/model_builder_quals_out_of_range.txt.gz)."""
    import shutil
    import emu_engine as EE
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
    import model_builder_ref as R
    from badread_amd.alignment import load_alignments
    from badread_amd.misc import load_fasta, load_fastq, reverse_complement
    folder = tmp_path / 'mb'
    shutil.copytree(FOLDER, folder)
    lines = open(folder / 'reads.fastq').read().split('\n')
    changed = 0
    for i in range(3, len(lines), 4):                # every quality line: a control character and a DEL every 97 / 131 bases
        q = list(lines[i])
        for j in range(40, len(q), 97):
            q[j] = '\x05'; changed += 1              # q = -28
        for j in range(71, len(q), 131):
            q[j] = '\x7f'                            # q = 94: inside the key's range, above the phred range
        lines[i] = ''.join(q)
    assert changed > 200
    open(folder / 'reads.fastq', 'w').write('\n'.join(lines))
    case = dict(GOLDEN['qscore'][0]['args'])
    ns = types.SimpleNamespace(reference=str(folder / 'ref.fasta'), reads=str(folder / 'reads.fastq'), alignment=str(folder / 'aln.paf'), **case)
    from badread_amd import model_builder as MB
    out = io.StringIO()
    MB.make_qscore_model(ns, output=io.StringIO(), engine=EE.EmuEngine(1 << 26), stdout=out)
    refs = load_fasta(ns.reference)[0]
    reads = load_fastq(ns.reads, output=io.StringIO())
    al = load_alignments(ns.alignment, case['max_alignments'], output=io.StringIO())
    want = R.qscore_model_text(refs, reads, al, case['k_size'], case['max_del'], case['min_occur'], case['max_output'], reverse_complement)
    assert out.getvalue() == want
    assert '-28:' in want and '94:' in want
    # the reference itself on the same files: the text its make_qscore_model printed for them, stored
    with gzip.open(os.path.join(HERE, 'golden', 'model_builder_quals_out_of_range.txt.gz'), 'rt') as f:
        assert f.read() == want


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['error', 'qscore'])
def test_hip_kernels_reproduce_the_reference_text(kind):
    eng = H.hip_engine()
    for entry in GOLDEN[kind]:
        assert run_product(kind, entry['args'], eng) == entry['text'], entry['args']


@pytest.mark.gpu
def test_command_line_writes_the_model_to_stdout():
    repo = os.path.dirname(HERE)
    for cmd, entry, extra in (('error_model', GOLDEN['error'][1], ['--k_size', '4', '--max_alt', '3']),
                              ('qscore_model', GOLDEN['qscore'][2], ['--k_size', '5', '--max_del', '2', '--min_occur', '2', '--max_output', '20'])):
        r = subprocess.run([sys.executable, '-m', 'badread_amd', cmd, '--reference', os.path.join(FOLDER, 'ref.fasta'),
                            '--reads', os.path.join(FOLDER, 'reads.fastq'), '--alignment', os.path.join(FOLDER, 'aln.paf')] + extra,
                           cwd=repo, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == entry['text']
        assert 'Loading alignments' in r.stderr and 'Processing alignments' in r.stderr


# ---------------------------------------------------------------------------------------------------------------------------------
# raw tables on synthetic jobs (tests/model_jobs.py)

ERROR_KS = (2, 3, 7, 8)                       # 8: the key is 2k + 5 + 42 = 63 bits
QSCORE_CASES = ((1, 1), (9, 6), (9, 15), (11, 1), (15, 6), (31, 2))      # from k_size 11 on a key no longer holds the largest windows
PARITY_JOBS = ('edges', 'mixed')
FOLDER_EDGES = os.path.join(HERE, 'golden', 'model_builder_edges')
_CACHE = {}


def restatement():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
    import model_builder_ref as R
    return R


def emu():
    import emu_engine as EE
    if 'emu' not in _CACHE:
        _CACHE['emu'] = EE.EmuEngine(1 << 26)
    return _CACHE['emu']


def job_kw(name, k_size=0):
    """The windows of k_size 11 and more are counted on the host one by one (and by the restatement): the two largest qscore
    cases run on the first 120 alignments of `mixed`, which keeps a case at a few seconds; every other case takes the whole job."""
    return dict(n_align=120) if name == 'mixed' and k_size >= 15 else {}


def product_job(name, **kw):
    from badread_amd import model_builder as MB
    key = ('job', name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = MB.Job(*J.job(name, **kw))
    return _CACHE[key]


def want_error(name, k, **kw):
    """error_table of the restatement, computed once per (job, k) and shared by the interpreted and the HIP checks."""
    from badread_amd.misc import reverse_complement
    key = ('error', name, k, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = restatement().error_table(*J.job(name, **kw), k, reverse_complement)
    return _CACHE[key]


def want_qscore(name, k_size, max_del, **kw):
    from badread_amd.misc import reverse_complement
    key = ('qscore', name, k_size, max_del, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = restatement().qscore_table(*J.job(name, **kw), k_size, max_del, reverse_complement)
    return _CACHE[key]


def got_error(engine, job, k, **kw):
    from badread_amd import model_builder as MB
    return {pair: [n, (rank >> 32, rank & 0xFFFFFFFF)] for pair, (n, rank) in MB.count_error_model(engine, job, k, **kw).items()}


def got_qscore(engine, job, k_size, max_del, **kw):
    from badread_amd import model_builder as MB
    return {cigar: [(rank >> 40, (rank >> 36) & 15, rank & 0xFFFFFFFF), dict(qs)]
            for cigar, (rank, qs) in MB.count_qscore_model(engine, job, k_size, max_del, **kw).items()}


def assert_same_table(got, want, what):
    """Exact equality, with the first few differences named (the dicts hold up to 250 000 entries)."""
    if got == want:
        return
    missing = [key for key in want if key not in got][:3]
    extra = [key for key in got if key not in want][:3]
    wrong = [(key, got[key], want[key]) for key in want if key in got and got[key] != want[key]][:3]
    raise AssertionError(f'{what}: missing {missing}, extra {extra}, (key, got, want) {wrong}; {len(got)} / {len(want)} entries')


def check_error_parity(engine, name, k):
    want = want_error(name, k)
    assert len(want) > 40
    assert_same_table(got_error(engine, product_job(name), k), want, (name, k))


def check_qscore_parity(engine, name, k_size, max_del):
    kw = job_kw(name, k_size)
    want = want_qscore(name, k_size, max_del, **kw)
    sizes = {len(cigar.replace('D', '')) for cigar in want}
    assert sizes == set(range(1, k_size + 2, 2))
    runs = [len(run) for cigar in want for run in __import__('re').findall('D+', cigar)]
    assert k_size == 1 or max(runs) == max_del                    # the jobs hold deletions longer than every max_del: the clamp ran
    assert_same_table(got_qscore(engine, product_job(name, **kw), k_size, max_del), want, (name, k_size, max_del))


def check_closed_forms(engine):
    """hot: 64 reads A^256 on A^256, 256M, quality 'I': every window of a size has one key, so all 64 * (256 - k + 1) windows add to one
    slot.  two_keys: reads (AC)^128: an error window counts only when it starts and ends on a match, so for odd k the (256 - k) / 2 + 1
    even starts give (A^k, ACA..A) and an even k counts nothing; a qscore size has the keys =X=.. (even starts, first at column 0)
    and X=X.. (odd starts, first at column 1), (257 - ks) / 2 windows each."""
    hot, two = product_job('hot'), product_job('two_keys')
    for k in ERROR_KS:
        assert got_error(engine, hot, k) == {('A' * k, 'A' * k): [64 * (256 - k + 1), (0, 0)]}, k
        want = {('A' * k, ('AC' * k)[:k]): [64 * ((256 - k) // 2 + 1), (0, 0)]} if k % 2 else {}
        assert got_error(engine, two, k) == want, k
    spilled = []
    for k_size in (9, 31):
        sizes = range(1, k_size + 2, 2)
        assert got_qscore(engine, hot, k_size, 6) == {'=' * ks: [(0, ks // 2, 0), {40: 64 * (256 - ks + 1)}] for ks in sizes}, k_size
        want = {}
        for ks in sizes:
            want[('=X' * ks)[:ks]] = [(0, ks // 2, 0), {40: 64 * (257 - ks) // 2}]
            want[('X=' * ks)[:ks]] = [(0, ks // 2, 1), {40: 64 * (257 - ks) // 2}]
        assert got_qscore(engine, two, k_size, 6) == want, k_size
        spilled.append(len(engine.model_count(1, hot, k_size, 6, (k_size + 1) // 2, 20)[3]))
    # k_size 9 fits the key; at 31 the windows of sizes 11..31 come back as spill words, more than the default spill_cap of 65 536:
    # model_count ran a second time with a longer list
    assert spilled == [0, 64 * sum(257 - ks for ks in range(11, 32, 2))] and spilled[1] > (1 << 16)
    print('model_routes closed_forms qscore spill words at k_size 9, 31:', spilled)


def _by_key(res):
    keys, counts, first, spill = res
    order = np.argsort(keys, kind='stable')
    return keys[order].tolist(), counts[order].tolist(), first[order].tolist(), sorted(spill.tolist())


def _window_bases(job, a, start, k, gap, over_ref):
    """Read bases of the window of alignment a that starts at column `start` and holds k reference bases (over_ref) or k read
    bases, on the restatement's gapped strings; None when the alignment ends first."""
    read_seq, read_qual, ref_seq, parts = job.slices[a]
    read_g, qual_g, ref_g = restatement().gapped(read_seq, read_qual, ref_seq, parts, gap)
    counted = ref_g if over_ref else read_g
    end, have = start, 0
    while have < k:
        if end >= len(counted):
            return None
        have += counted[end] != gap
        end += 1
    return read_g[start:end].replace(gap, ''), qual_g[start:end].replace(gap, '')


def check_error_spill_route(engine, k):
    """`edges` holds insertions of 21 - k and 22 - k bases between exact flanks: a read k-mer of 21 bases is the last a key holds
    (BRX_MB_MAX_READ_KMER), one of 22 the first that goes to the host.  From the engine's own answer: the spill list has windows of
    22 bases and none shorter, and the table has keys of 21."""
    job = product_job('edges')
    keys, counts, first, spill = engine.model_count(0, job, k, 0, 1, 18)
    words = spill.tolist()
    assert len(words) == len(set(words)) > 0
    lengths = collections.Counter(len(_window_bases(job, w >> 32, w & 0xFFFFFFFF, k, '-', True)[0]) for w in words)
    in_keys = collections.Counter()                  # read k-mer length -> windows counted in the table
    for length, n in zip(((keys >> np.uint64(2 * k)) & np.uint64(31)).tolist(), counts.tolist()):
        in_keys[length] += n
    print(f'model_routes error k={k}: spill words {len(words)}, read k-mer lengths spilled {sorted(lengths)[:3]}..{max(lengths)}, '
          f'windows of 21 bases in the table {in_keys[21]}, table entries {len(keys)}')
    # two strands, each alignment twice, at least one window over the whole insertion in each
    assert min(lengths) == 22 and lengths[22] >= 4
    assert max(in_keys) == 21 and in_keys[21] >= 4


def check_qscore_spill_route(engine):
    """A qscore key holds 6 ks - 4 op bits: 50 at ks = 9, 62 at ks = 11.  At --k_size 11 on `edges`: every window of size index 5 is
    in the spill list (as many as the restatement counts windows of 11 read bases), no key has that index, and a window of a
    smaller size is there only for its quality character (q < 0 or q > 127), never for its length."""
    job = product_job('edges')
    from badread_amd import model_builder as MB
    keys, counts, first, spill = MB._table(engine, 1, job, 11, 1, 6)
    words = spill.tolist()
    assert len(words) == len(set(words))
    by_size = collections.Counter((w >> 32) & 15 for w in words)
    want = want_qscore('edges', 11, 1)
    windows = collections.Counter()
    for cigar, (_, qs) in want.items():
        windows[len(cigar.replace('D', '')) // 2] += sum(qs.values())
    assert by_size[5] == windows[5] > 10000
    assert int(((keys >> np.uint64(7)) & np.uint64(15)).max()) == 4
    small = [w for w in words if (w >> 32) & 15 <= 4]
    for w in small:
        ks = 2 * ((w >> 32) & 15) + 1
        q = ord(_window_bases(job, w >> 36, w & 0xFFFFFFFF, ks, ' ', False)[1][ks // 2]) - 33
        assert q < 0 or q > 127, (w, q)
    out_of_range = sum(n for _, qs in want.values() for q, n in qs.items() if q < 0 or q > 127)
    assert len(small) + sum(1 for w in words if (w >> 32) & 15 == 5 and not 0 <= ord(
        _window_bases(job, w >> 36, w & 0xFFFFFFFF, 11, ' ', False)[1][5]) - 33 <= 127) == out_of_range > 100
    print(f'model_routes qscore k_size=11: spill words {len(words)} (size index 5: {by_size[5]}, smaller sizes, for their quality: {len(small)}), '
          f'table entries {len(keys)}')


def check_regrow(engine):
    """Spill list and table too small: model_count(spill_cap=4) runs again with a list that fits and answers as the default call does;
    a table of 2^6 slots is full (None); model_builder._table(first_bits=6) grows it by two bits until the count fits and answers as
    the default does."""
    from badread_amd import model_builder as MB
    job = product_job('edges')
    for kind, k, max_del, n_ksizes, bits in ((0, 7, 0, 1, 17), (1, 11, 1, 6, 19)):
        whole = engine.model_count(kind, job, k, max_del, n_ksizes, bits)
        small = engine.model_count(kind, job, k, max_del, n_ksizes, bits, spill_cap=4)
        assert len(whole[3]) > 4 and _by_key(small) == _by_key(whole), kind
        assert engine.model_count(kind, job, k, max_del, n_ksizes, 6) is None
        print(f'model_routes regrow kind={kind}: spill words {len(whole[3])} with spill_cap 4 and with the default; table entries {len(whole[0])}; '
              f'2^6 slots: None')

    class Recorded(object):
        """The engine with every model_count call noted: (table_bits, answered)."""
        def __init__(self):
            self.calls = []

        def model_count(self, kind, job_, k, max_del, n_ksizes, bits):
            res = engine.model_count(kind, job_, k, max_del, n_ksizes, bits)
            self.calls.append((bits, res is not None))
            return res

    tiny = product_job('mixed', n_align=6)
    for kind, k, max_del, n_ksizes in ((0, 7, 0, 1), (1, 9, 6, 5)):
        rec = Recorded()
        grown = MB._table(rec, kind, tiny, k, max_del, n_ksizes, first_bits=6)
        whole = MB._table(engine, kind, tiny, k, max_del, n_ksizes)
        bits = [b for b, _ in rec.calls]
        assert bits == list(range(6, bits[-1] + 1, 2)) and len(bits) >= 3 and [ok for _, ok in rec.calls] == [False] * (len(bits) - 1) + [True]
        assert (1 << (bits[-1] - 2)) < len(whole[0]) + 1 <= (1 << bits[-1])          # the first size that holds the keys
        assert _by_key(grown) == _by_key(whole)
        print(f'model_routes _table(first_bits=6) kind={kind}: tables of 2^{bits} slots, {len(whole[0])} entries')
    rec = Recorded()                                 # and through the merge: the grown table gives the restatement's
    assert got_error(rec, tiny, 7, first_bits=6) == want_error('mixed', 7, n_align=6) and len(rec.calls) >= 3


def check_edges_golden(engine, kind):
    """The reference's own text for the file form of `edges` (tools/make_golden.py make_model_builder_edges)."""
    with gzip.open(os.path.join(HERE, 'golden', 'model_builder_edges.json.gz'), 'rt') as f:
        golden = json.load(f)
    assert len(golden[kind]) == 3
    from badread_amd import model_builder as MB
    for entry in golden[kind]:
        ns = types.SimpleNamespace(reference=os.path.join(FOLDER_EDGES, 'ref.fasta'), reads=os.path.join(FOLDER_EDGES, 'reads.fastq'),
                                   alignment=os.path.join(FOLDER_EDGES, 'aln.paf'), **entry['args'])
        out = io.StringIO()
        (MB.make_error_model if kind == 'error' else MB.make_qscore_model)(ns, output=io.StringIO(), engine=engine, stdout=out)
        assert out.getvalue() == entry['text'], entry['args']


def test_restatement_reproduces_the_reference_text_of_the_edges_files():
    R = restatement()
    from badread_amd.alignment import load_alignments
    from badread_amd.misc import load_fasta, load_fastq, reverse_complement
    with gzip.open(os.path.join(HERE, 'golden', 'model_builder_edges.json.gz'), 'rt') as f:
        golden = json.load(f)
    refs = load_fasta(os.path.join(FOLDER_EDGES, 'ref.fasta'))[0]
    reads = load_fastq(os.path.join(FOLDER_EDGES, 'reads.fastq'), output=io.StringIO())
    al = load_alignments(os.path.join(FOLDER_EDGES, 'aln.paf'), output=io.StringIO())
    assert len(al) == len(J.edges(files=True)[2]) > 100                  # the loader keeps every alignment of the file form
    assert [(e['args']['k_size'], e['args']['max_alt']) for e in golden['error']] == [(2, 10 ** 6), (3, 10 ** 6), (8, 10 ** 6)]
    assert [(e['args']['k_size'], e['args']['max_del']) for e in golden['qscore']] == [(1, 1), (11, 1), (15, 15)]
    for entry in golden['error']:
        a = entry['args']
        assert R.error_model_text(refs, reads, al, a['k_size'], a['max_alt'], reverse_complement) == entry['text'], a
    for entry in golden['qscore']:
        a = entry['args']
        assert R.qscore_model_text(refs, reads, al, a['k_size'], a['max_del'], a['min_occur'], a['max_output'], reverse_complement) == entry['text'], a


def test_synthetic_jobs_hold_what_their_names_promise():
    """The generator itself: the starts on the block borders, the spans, strands, indel lengths and characters of `edges`."""
    refs, reads, al = J.job('edges')
    starts = np.cumsum([0] + [sum(n for n, _ in a.cigar_parts) for a in al])
    spans = collections.defaultdict(set)
    for a, c in zip(al, starts):
        if len(a.cigar_parts) == 1:
            spans[a.ref_end - a.ref_start].add((int(c) % 256, a.strand))
    for span in (1, 2, 3, 4, 5, 6, 7, 8, 9, 30, 255, 256, 257, 511, 512, 600):
        assert {(r, s) for r in (0, 1, 255) for s in '+-'} <= spans[span], span
    assert set(range(1, 34)) <= set(spans)
    ins = {n for a in al for n, t in a.cigar_parts if t == 'I'}
    dels = {n for a in al for n, t in a.cigar_parts if t == 'D'}
    assert {1, 2, 3, 40} | {21 - k for k in ERROR_KS} | {22 - k for k in ERROR_KS} <= ins
    assert {1, 16, 30} | {d + x for _, d in QSCORE_CASES for x in (-1, 0, 1) if d + x > 0} <= dels
    assert any(a.cigar_parts[:2] == [(1, 'M'), (3, 'I')] for a in al) and any(a.cigar_parts[-2:] == [(3, 'I'), (1, 'M')] for a in al)
    assert all(a.cigar_parts[0][1] == 'M' and a.cigar_parts[-1][1] == 'M' for kind in ('edges', 'mixed', 'hot', 'two_keys') for a in J.job(kind)[2])
    quals = set(''.join(q for _, q in reads.values()))
    assert set('!~\x7f\x05\xa0\xa1') <= quals and ' ' not in quals
    assert set('NRYKM') <= set(refs['ctg']) and 'N' in set(''.join(s for s, _ in reads.values()))
    cols = {kind: sum(n for a in J.job(kind)[2] for n, _ in a.cigar_parts) for kind in ('edges', 'mixed', 'hot', 'two_keys')}
    assert all(10000 < n < 110000 for n in cols.values()), cols
    assert len(J.job('mixed')[2]) == 400 and {a.strand for a in J.job('mixed')[2]} == {'+', '-'}


@pytest.mark.parametrize('k', ERROR_KS)
@pytest.mark.parametrize('name', PARITY_JOBS)
def test_interpreted_error_table_equals_the_restatement(name, k):
    check_error_parity(emu(), name, k)


@pytest.mark.parametrize('k_size,max_del', QSCORE_CASES)
@pytest.mark.parametrize('name', PARITY_JOBS)
def test_interpreted_qscore_table_equals_the_restatement(name, k_size, max_del):
    check_qscore_parity(emu(), name, k_size, max_del)


def test_interpreted_closed_forms_of_one_and_two_keys():
    check_closed_forms(emu())


@pytest.mark.parametrize('k', ERROR_KS)
def test_interpreted_error_spill_holds_22_bases_and_never_21(k):
    check_error_spill_route(emu(), k)


def test_interpreted_qscore_spill_holds_every_window_of_size_11():
    check_qscore_spill_route(emu())


def test_interpreted_spill_list_and_table_regrow():
    check_regrow(emu())


@pytest.mark.parametrize('kind', ['error', 'qscore'])
def test_interpreted_kernels_reproduce_the_reference_text_of_the_edges_files(kind):
    check_edges_golden(emu(), kind)


@pytest.mark.gpu
@pytest.mark.parametrize('k', ERROR_KS)
@pytest.mark.parametrize('name', PARITY_JOBS)
def test_hip_error_table_equals_the_restatement(name, k):
    check_error_parity(H.hip_engine(), name, k)


@pytest.mark.gpu
@pytest.mark.parametrize('k_size,max_del', QSCORE_CASES)
@pytest.mark.parametrize('name', PARITY_JOBS)
def test_hip_qscore_table_equals_the_restatement(name, k_size, max_del):
    check_qscore_parity(H.hip_engine(), name, k_size, max_del)


@pytest.mark.gpu
def test_hip_closed_forms_of_one_and_two_keys():
    check_closed_forms(H.hip_engine())


@pytest.mark.gpu
@pytest.mark.parametrize('k', ERROR_KS)
def test_hip_error_spill_holds_22_bases_and_never_21(k):
    check_error_spill_route(H.hip_engine(), k)


@pytest.mark.gpu
def test_hip_qscore_spill_holds_every_window_of_size_11():
    check_qscore_spill_route(H.hip_engine())


@pytest.mark.gpu
def test_hip_spill_list_and_table_regrow():
    check_regrow(H.hip_engine())


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['error', 'qscore'])
def test_hip_kernels_reproduce_the_reference_text_of_the_edges_files(kind):
    check_edges_golden(H.hip_engine(), kind)
