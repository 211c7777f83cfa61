"""
User-supplied model files (`--error_model FILE`, `--qscore_model FILE`) on the CPU: the synthetic models of tests/custom_models.py,
each built to select a branch that no packaged model selects.

  * tests/golden/sequence_fragment_custom_models.json.gz: the UNMODIFIED reference's sequence_fragment replayed with our draws
    under these files (the reference loads them itself).  The oracle consumes the flattened tables of ErrorModel.tables() /
    QScoreModel.tables(); so kernel-against-oracle parity cannot see a flatten bug, and this replay can.
  * the flattened tables restate the files, with reach assertions computed from the tables: a later edit of a model cannot empty
    a branch silently.
  * reach assertions on results: the final alignment of the oracle's reads holds the D-runs and the rows the models are for.
  * the product's HIP sources interpreted on the CPU (tests/emu_engine.py) against the oracle: every digest case of up to
    1200 bases, three mutate routes under two model pairs, and a qscore table without its 'X' row (BRX_RS_QMISS).

Measured: 55 s for the whole file (of which 10 s build the interpreted library when no earlier test of the run has).
"""
import gzip
import json
import os
import re

import numpy as np
import pytest

import custom_models as CM
import helpers as H
import pyoracle
from badread_amd.engine import RS_QMISS
from badread_amd.qscore_model import cigar_key
from test_emulated_device import MUTATE_ROUTES, STAT_FIELDS

HERE = os.path.dirname(os.path.abspath(__file__))
TXT = np.frombuffer(b'ACGTN', dtype=np.uint8)


def load_cases():
    with gzip.open(os.path.join(HERE, 'golden', 'sequence_fragment_custom_models.json.gz'), 'rt') as f:
        return json.load(f)['cases']


def configured(engine, em, qm):
    engine.set_error_model(CM.error_tables(em))
    engine.set_qscore_model(CM.qscore_tables(qm))
    return engine


class Recording(object):
    """An engine for helpers.check_digest_cases that keeps what it returned."""

    def __init__(self, engine, kept):
        self.engine, self.kept = engine, kept

    def sequence_fragments(self, seed, read, frags, targets):
        res, st = self.engine.sequence_fragments(seed, read, frags, targets)
        self.kept[(seed, read)] = (frags[0], res[0][0], res[0][1], st)
        return res, st


@pytest.fixture(scope='module')
def oracle_results():
    """Every digest case through the oracle, checked against its digest ONCE: (seed, read) -> fragment, read, qualities, stats."""
    kept, engines = {}, {}

    def engine_of(em, qm):
        if (em, qm) not in engines:
            engines[(em, qm)] = Recording(configured(H.oracle_engine(), em, qm), kept)
        return engines[(em, qm)]
    cases = load_cases()
    H.check_digest_cases(engine_of, cases)
    return cases, kept, engines


def final_ops(frag, seq):
    """The read (query) against its fragment (target): the alignment get_qscores makes, but for the two ends -- that one is made
    before the k bases of padding at either end are trimmed away."""
    return pyoracle.align(TXT[seq].tobytes(), TXT[frag].tobytes())[1]


# ------------------------------------------------------------------------------------------------ files and digests
def test_the_model_files_are_what_their_names_generate():
    for name in CM.NAMES:
        with open(CM.path_of(name), newline='') as f:
            assert f.read() == CM.text(name), name
        assert os.path.getsize(CM.path_of(name)) < 64 << 10, name
    assert sorted(os.listdir(CM.MODEL_DIR)) == sorted(CM.NAMES)


def test_the_oracle_reproduces_the_reference_under_every_model_file(oracle_results):
    """The digests (sequence, qualities, identity, loop and alignment counts) hold -- the fixture asserted that -- and the cases
    are the ones the models need: every pair, the edges of ALIGNMENT_SIZE, 1500-3000 bases, targets 0.6-0.99, fragments on which
    present rows, absent rows and k-mers outside ACGT all occur."""
    cases, kept, _ = oracle_results
    assert len(cases) >= 60 and len(kept) == len(cases)
    assert {(c['em'], c['qm']) for c in cases} == set(CM.PAIRS)
    assert {e for e, _ in CM.PAIRS} == set(CM.ERROR_MODELS) | {'nanopore2023'} and {q for _, q in CM.PAIRS} == set(CM.QSCORE_MODELS)
    assert {30, 999, 1000, 1001} <= {c['length'] for c in cases} and sum(1500 <= c['length'] <= 3000 for c in cases) >= 30
    assert all(0.6 <= c['target'] <= 0.99 for c in cases)
    assert sum(CM.is_low_identity_e9(c) for c in cases) >= 2
    for c in cases:
        if c['em'] in ('e5_blocks', 'e8_sparse', 'e9_sparse', 'e7_long') and c['length'] >= 999:
            frag = H.case_fragment(c)
            share = CM.present_share(CM.text(c['em']), frag)
            assert 0.3 < share < 0.95, (c['em'], c['length'], share)
            assert not c['with_n'] or (frag == 4).any()


# ------------------------------------------------------------------------------------------------ the flattened tables
def pool_lengths(t):
    desc = t['desc'][:t['n_alts']].astype(np.int64)
    return np.stack([t['pool'][desc + 2 + j] for j in range(t['k'])], axis=1)


@pytest.mark.parametrize('name', CM.ERROR_MODELS)
def test_error_tables_restate_the_file(name):
    """tests/test_golden_host.py::test_lookup_order_tables_restate_the_table on these files, with the long flag held to its
    definition in both directions (a length above 15, or k above 8); thresholds monotone within a row and padded by eight zeros;
    rows, alternatives, strings and probabilities as the file's lines state them."""
    t = CM.error_tables(name)
    k, n_rows, n_alts = t['k'], t['n_rows'], t['n_alts']
    lines = CM.text(name).splitlines()
    assert k == len(lines[0].split(',', 1)[0]) and n_rows == 4 ** k and n_alts == sum(line.count(';') for line in lines)
    rowx, altx, pool = t['rowx'], t['altx'], t['pool']
    assert len(rowx) >= 2 * (n_rows + 1) + 4 and len(altx) == 4 * n_alts
    assert (rowx[0:2 * n_rows:2] == t['self_thr']).all() and (rowx[1:2 * n_rows + 2:2] == t['row_off']).all()
    desc = t['desc'][:n_alts].astype(np.int64)
    assert (altx[0::4] == t['desc'][:n_alts]).all()
    diff = pool[desc].astype(np.uint32) | (pool[desc + 1].astype(np.uint32) << 8)
    assert ((altx[1::4] & 0xFFFF) == diff).all()
    long_ = (altx[1::4] >> 16) != 0
    lens = pool_lengths(t)
    assert (long_ == ((lens.max(axis=1) > 15) | (k > 8))).all()
    for j in range(min(k, 8)):
        assert (((altx[2::4] >> (4 * j)) & 15)[~long_] == lens[:, j][~long_]).all()
    assert not altx[2::4][long_].any()
    thr, off = t['thr'][:n_alts].astype(np.int64), t['row_off'].astype(np.int64)
    assert len(t['thr']) >= n_alts + 8 and not t['thr'][n_alts:].any()
    starts = set(off[1:-1].tolist())
    assert not [i + 1 for i in np.flatnonzero(np.diff(thr) < 0) if (i + 1) not in starts]
    for line in lines:                                                      # every line: its row, its strings, its thresholds
        entries = [e.split(',') for e in line.split(';') if e]
        kmer = entries[0][0]
        row = int(''.join(str('ACGT'.index(ch)) for ch in kmer), 4)
        a0, a1 = int(off[row]), int(off[row + 1])
        assert a1 - a0 == len(entries)
        probs = [float(p) for _, p in entries]
        total = max(sum(probs), 1.0)
        for a, (alt, _) in enumerate(entries):
            o = int(desc[a0 + a])
            n = int(lens[a0 + a].sum())
            got = ''.join('ACGT'[c] for c in pool[o + 2 + k:o + 2 + k + n])
            assert got == alt and (diff[a0 + a] == 0) == (alt == kmer), (kmer, alt, got)
            assert diff[a0 + a] & 1 == 0 and diff[a0 + a] >> (k - 1) == 0          # the first and the last base stay
            want = 0xFFFFFFFF if (a == len(entries) - 1 and sum(probs) >= 1.0) else sum(probs[:a + 1]) / total * 2.0 ** 32
            assert abs(int(thr[a0 + a]) - want) <= 2048, (kmer, a)                 # (summation order: a few ulps of 2^32)


def test_error_tables_reach_the_branches_they_are_for():
    t = {name: CM.error_tables(name) for name in CM.ERROR_MODELS}
    sizes = {name: np.diff(t[name]['row_off'].astype(np.int64)) for name in t}
    last = {name: t[name]['thr'][np.maximum(t[name]['row_off'][1:].astype(np.int64) - 1, 0)][sizes[name] > 0] for name in t}
    long_ = {name: (t[name]['altx'][1::4] >> 16) != 0 for name in t}
    lens = {name: pool_lengths(t[name]) for name in t}
    assert [t[n]['k'] for n in CM.ERROR_MODELS] == [3, 3, 5, 8, 9, 7]
    # e3_full: every row present; rows that sum to 1 and more (the last alternative wins) beside rows with a remainder
    assert (sizes['e3_full'] == 4).all() and 20 <= int((last['e3_full'] == 0xFFFFFFFF).sum()) <= 44
    assert (lens['e3_full'][:, 1] == 0).any() and (lens['e3_full'][:, 1] == 2).any()
    # e3_big: long by length at k = 3
    assert long_['e3_big'].sum() == 64 and lens['e3_big'].max() == 61
    # e5_blocks: the block edges of the threshold scan, with and without a remainder; a non-first alternative that changes nothing
    s5 = sizes['e5_blocks']
    assert set(CM.E5_ROW_SIZES) <= set(s5.tolist())
    for n in (8, 16):
        ends = last['e5_blocks'][s5[s5 > 0] == n]
        assert (ends == 0xFFFFFFFF).any() and (ends != 0xFFFFFFFF).any(), n
    t5 = t['e5_blocks']
    diff5 = t5['altx'][1::4] & 0xFFFF
    first = np.zeros(t5['n_alts'], dtype=bool)
    first[t5['row_off'][:-1][s5 > 0]] = True
    assert ((diff5 == 0) & ~first).sum() >= 5 and (diff5[first] == 0).all()
    assert not long_['e5_blocks'].any()
    # e8_sparse / e9_sparse: absent rows; k = 8 on the packed path with the largest 4-bit length on its last inner position
    for name, k in (('e8_sparse', 8), ('e9_sparse', 9)):
        assert 250 <= int((sizes[name] > 0).sum()) <= 350 and (sizes[name] == 0).sum() > 4 ** k - 400
    assert not long_['e8_sparse'].any() and lens['e8_sparse'][:, 6].max() == 15 and (lens['e8_sparse'][:, 1:7].sum(axis=1) == 0).any()
    assert long_['e9_sparse'].all() and lens['e9_sparse'].max() == 20 and (lens['e9_sparse'][:, 1:8].sum(axis=1) == 0).any()
    # e7_long: both sides of the 15 / 16 edge, and the 7-bit length
    l7 = lens['e7_long'].max(axis=1)
    assert long_['e7_long'].any() and (~long_['e7_long']).any()
    assert {15, 16, 127} <= set(l7.tolist()) and (long_['e7_long'] == (l7 > 15)).all()
    # every inner base of a k-mer deleted by some alternative, at every k
    for name in ('e5_blocks', 'e8_sparse', 'e9_sparse', 'e7_long'):
        assert (lens[name][:, 1:-1] == 0).any(axis=0).all(), name


def key_bits(t):
    return 2 * t['k'] + t['gap_bits'] * (t['k'] - 1)


@pytest.mark.parametrize('name', CM.QSCORE_MODELS)
def test_qscore_tables_restate_the_file(name):
    """Every row of the file that a window can ask for is found through the hash, with its scores in file order and thresholds
    that are the cumulative probabilities (a zero-probability entry repeats the threshold before it)."""
    m = CM.qscore_model(name)
    t = m.tables()
    lines = [line.split(';') for line in CM.text(name).splitlines()]
    assert list(m.scores) == [p[0] for p in lines]
    row_of = {int(k): int(r) for k, r in zip(t['hash_key'], t['hash_row']) if int(k) != 0xFFFFFFFFFFFFFFFF}
    assert len(row_of) == t['n_rows'] == len(lines) and t['k'] == max(len(p[0].replace('D', '')) for p in lines)
    thr = t['thr'].astype(np.int64)
    for cigar, _, dist in lines:
        row = row_of[cigar_key(cigar, t['gap_bits'])]
        assert t['cigars'][row] == cigar
        e0, e1 = int(t['row_off'][row]), int(t['row_off'][row + 1])
        pairs = [x.split(':') for x in dist.split(',')]
        assert t['score'][e0:e1].tolist() == [int(q) for q, _ in pairs]
        p = np.array([float(x) for _, x in pairs])
        assert np.abs(thr[e0:e1] / 2.0 ** 32 - np.cumsum(p) / p.sum()).max() < 2e-9
        assert (np.diff(thr[e0:e1]) >= 0).all() and ((np.diff(thr[e0:e1]) == 0) == (p[1:] == 0)).all()


def test_qscore_tables_reach_the_branches_they_are_for():
    t = {name: CM.qscore_tables(name) for name in CM.QSCORE_MODELS}
    assert [(t[n]['k'], t[n]['gap_bits']) for n in CM.QSCORE_MODELS] == [(1, 3), (3, 3), (9, 4), (11, 3), (9, 3), (9, 3), (9, 3)]
    assert key_bits(t['q11']) == 52 and key_bits(t['q9_gap4']) == 50
    assert t['q1']['n_rows'] == 3 and set(t['q1']['cigars']) == {'=', 'X', 'I'}
    runs = lambda name: {len(r) for c in t[name]['cigars'] for r in re.findall('D+', c)}
    assert {7, 10, 14} <= runs('q9_gap4') and max(runs('q9_gap4')) == 14 and max(runs('q11')) == 6
    assert {'=D=', '=DD=', 'XD='} <= set(t['q3_gaps']['cigars']) and {1, 2, 3} == runs('q3_gaps')
    size = lambda name, c: int(np.diff(t[name]['row_off'])[t[name]['cigars'].index(c)]) if c in t[name]['cigars'] else None
    hot = '=' * 9
    assert size('q9_nohot', hot) is None and size('q9_nohot', '=' * 7) is not None
    assert size('q9_bighot', hot) == 130 and 0 < size('q9_gap4', hot) <= 128 and 0 < size('q9_zeros', hot) <= 128
    assert 0 < size('q11', '=' * 11) <= 128 and 0 < size('q1', '=') <= 128
    tz = t['q9_zeros']
    e0 = tz['row_off'][:-1].astype(np.int64)
    e1 = tz['row_off'][1:].astype(np.int64)
    zero = np.isin(tz['score'], CM.ZERO_SCORES)
    thr = tz['thr'].astype(np.int64)
    assert zero[e1 - 1].all() and (zero[e0].sum() >= 10) and not zero[e0].all()              # the last entry of every row; some first ones
    prev = np.concatenate([[0], thr[:-1]])
    prev[e0] = 0
    assert ((thr == prev) == zero).all()                                                      # exactly the zero entries repeat a threshold
    assert not any(np.isin(t[n]['score'], CM.ZERO_SCORES).any() for n in CM.QSCORE_MODELS if n != 'q9_zeros')


# ------------------------------------------------------------------------------------------------ reach, from results
def test_results_hold_what_the_models_are_for(oracle_results):
    """The final alignment of each oracle read against its fragment (the oracle's own aligner), and the row the oracle's
    fallback used for every base (orc_qscore_rows_probe: -1 where it ended without one)."""
    cases, kept, engines = oracle_results
    seen = {'low': 0, 'gap4_rows': 0, 'gap4_saturated': 0, 'zeros': 0, 'i126': 0, 'i19': 0, 'nohot_full': 0, 'bighot': 0, 'k11': 0, 'k1': 0}
    for c in cases:
        frag, seq, qual, st = kept[(c['seed'], c['read'])]
        ops = final_ops(frag, seq)
        assert st['status'][0] == 0
        d = CM.d_runs(ops)
        ins = CM.d_runs(np.where(ops == 2, 3, 0))
        t = CM.qscore_tables(c['qm'])
        rows, used = engines[(c['em'], c['qm'])].engine.qscore_rows(ops)
        assert (rows >= 0).all()
        cig = [t['cigars'][r] for r in sorted(set(rows.tolist()))]
        if CM.is_low_identity_e9(c):
            assert d.max() >= 15, (c['qm'], c['seed'], int(d.max()))        # longer than the 4-bit field holds
            seen['low'] += 1
        if c['qm'] == 'q9_gap4' and c['em'] in ('e8_sparse', 'e9_sparse') and c['length'] >= 1500:
            # (the other error models delete at most three bases at once: no final alignment of theirs holds a run beyond 6)
            assert ((d >= 7) & (d <= 14)).any(), (c['em'], c['seed'])
            seen['gap4_rows'] += sum(any(7 <= len(r) <= 14 for r in re.findall('D+', x)) for x in cig)
            seen['gap4_saturated'] += int((d >= 15).any())
        if c['qm'] == 'q9_zeros':
            assert not np.isin(qual.astype(np.int64) - 33, CM.ZERO_SCORES).any(), (c['em'], c['seed'])
            seen['zeros'] += len(qual)
        if c['em'] == 'e7_long':
            seen['i126'] += int((ins >= 126).sum())
        if c['em'] == 'e9_sparse':
            seen['i19'] += int((ins >= 19).sum())
        if c['qm'] == 'q9_nohot':
            assert '=' * 9 not in cig
            seen['nohot_full'] += int((2 * used + 1 == 9).sum())
        if c['qm'] == 'q9_bighot':
            seen['bighot'] += int((rows == t['cigars'].index('=' * 9)).sum())
        if c['qm'] == 'q11':
            seen['k11'] += int((2 * used + 1 == 11).sum())
        if c['qm'] == 'q1':
            assert (used == 0).all()
            seen['k1'] += len(used)
    assert seen['low'] >= 2 and seen['gap4_rows'] >= 10 and seen['gap4_saturated'] >= 1, seen
    assert seen['zeros'] > 5000 and seen['i126'] >= 1 and seen['i19'] >= 1, seen
    assert min(seen['nohot_full'], seen['bighot'], seen['k11'], seen['k1']) > 1000, seen


# ------------------------------------------------------------------------------------------------ the interpreted kernels
@pytest.fixture(scope='module')
def emu():
    import emu_engine as EE
    pref, _ = H.small_reference()
    return H.configure(EE.EmuEngine(1 << 29), pref)


def test_interpreted_kernels_reproduce_the_short_digest_cases(emu):
    """Every digest case of up to 1200 bases (30, 999, 1000, 1001: one or more per model file) through the product's HIP sources
    on the CPU."""
    cases = [c for c in load_cases() if c['length'] <= 1200]
    assert {c['em'] for c in cases} >= set(CM.ERROR_MODELS) and {c['qm'] for c in cases} == set(CM.QSCORE_MODELS)
    H.check_digest_cases(lambda em, qm: configured(emu, em, qm), sorted(cases, key=lambda c: (c['em'], c['qm'])))


@pytest.mark.parametrize('em,qm,route', [(em, qm, route) for em, qm in (('e9_sparse', 'q9_gap4'), ('e7_long', 'q9_nohot'))
                                         for route in ('default', 'lanes', 'passes_tail')] + [('e5_blocks', 'q1', 'default'), ('e5_blocks', 'q1', 'lanes')])
def test_interpreted_mutate_routes_equal_the_oracle(em, qm, route, monkeypatch):
    """Eight fragments of about 600 bases in place (few reads: all head), one per lane in k_mut_lanes, and through the host-driven
    passes with a head chain and a tail: all statistics and all bytes of the oracle.  (e5_blocks on two routes besides: both
    proposal sites of the threshold scan on rows that end at and beside its block edges.)"""
    import emu_engine as EE
    for k, v in MUTATE_ROUTES[route].items():
        monkeypatch.setenv(k, str(v))
    pref, _ = H.small_reference()
    eng = configured(H.configure(EE.EmuEngine(1 << 29), pref), em, qm)
    orc = configured(H.configure(H.oracle_engine(), pref), em, qm)
    frags, targets = CM.batch(CM.PAIRS.index((em, 'q9_gap4')), 8, 500, 700)
    rh, sh = eng.sequence_fragments(31, 0, frags, targets)
    ro, so = orc.sequence_fragments(31, 0, frags, targets)
    for f in STAT_FIELDS:
        assert (sh[f] == so[f]).all(), f
    for a, b in zip(rh, ro):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (so['change_count'] > 0).all() and so['change_count'].sum() > 500


def qmiss_case():
    """q3_gaps without its 'X' row, under nanopore2023: 12 fragments of 20-400 bases.  Returns the tables, the input and the
    oracle's result, checked: QMISS is set on reads whose qualities hold the score 0 (q3_gaps has none of its own: a window that
    found no row), on at least three reads, and on no read without a single change -- the three shortest, whose targets ask for
    less than half an error, so that no column of their alignments, padding included, is an X."""
    t = CM.qscore_tables_without(CM.qscore_tables('q3_gaps'), 'X')
    assert not (CM.qscore_tables('q3_gaps')['score'] == 0).any()
    frags = [CM.fragment_codes(70000 + i, n) for i, n in enumerate((20, 25, 30, 40, 60, 90, 150, 200, 250, 300, 350, 400))]
    targets = [0.99, 0.99, 0.99, 0.97, 0.95, 0.9, 0.9, 0.85, 0.8, 0.9, 0.85, 0.8]
    pref, _ = H.small_reference()
    orc = H.configure(H.oracle_engine(), pref, 'nanopore2023')
    orc.set_qscore_model(t)
    res, st = orc.sequence_fragments(17, 0, frags, targets)
    miss = (st['status'] & RS_QMISS) != 0
    unchanged = st['change_count'] == 0
    assert unchanged[:3].all() and not miss[unchanged].any()
    for frag, (seq, qual), flag, same in zip(frags, res, miss, unchanged):
        assert flag or not (qual == 33).any()
        assert not same or (np.array_equal(seq, frag) and not (final_ops(frag, seq) == 1).any())
    assert miss.sum() >= 3 and sum(bool((q == 33).any()) for _, q in res) >= 3
    assert (st['status'] & ~np.uint32(RS_QMISS) == 0).all()
    return t, frags, targets, res, st


def test_a_fallback_that_ends_without_a_row_sets_qmiss(emu):
    """The host class refuses a model file without '=', 'X' or 'I'; the C-ABI takes the table.  Oracle (oracle/brx_oracle.c: score
    0 and BRX_RS_QMISS) and the interpreted k_fin_qscore agree on every field and byte."""
    t, frags, targets, ro, so = qmiss_case()
    emu.set_error_model(H.error_tables('nanopore2023'))
    emu.set_qscore_model(t)
    rh, sh = emu.sequence_fragments(17, 0, frags, targets)
    for f in STAT_FIELDS:
        assert (sh[f] == so[f]).all(), f
    for a, b in zip(rh, ro):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
