"""
The interpreted kernels (tests/emu_engine.py) on low-complexity sequence (tests/lowcomplexity.py): homopolymer mosaics, tandem
repeats, diverged arrays, a two-letter alphabet, splices with N runs.  tests/test_emulated_device.py feeds the kernels uniform
bases; here every alignment has co-optimal paths all along (the tie-break I, D, diagonal decides the path), the CIGAR windows
of k_fin_qscore have long I/D runs, and the canonical path of a final alignment leaves the windowed traceback store
(csrc/brx_align.h, brx_make_geom_span) on a few per cent of the reads -- under the DEFAULT window, where uniform input needs
millions of reads for one miss.  Same bar as everywhere: bit-identical to the oracle through the C-ABI.
"""
import numpy as np
import pytest

import helpers as H
import lowcomplexity as LC
import pyoracle
from badread_amd.engine import SimParams
from test_emulated_device import STAT_FIELDS, check_pairs, emu_engine


def band_words(q, t, k):
    """Words per lane of the band of a (q x t) pair under the edit bound k (brx_make_geom: 56 superblocks of 32 G rows)."""
    a = abs(q - t)
    k = max(k, a)
    bw = 2 * ((k - a) // 2) + a + 1
    g = 1
    while bw > 56 * 32 * g:
        g *= 2
    return g


def doubled_bound(q, t, d):
    """The bound of the round that succeeds without a hint: 64, 128, ... capped at the longer sequence."""
    k = min(max(q, t), 64)
    while k < d:
        k = min(2 * k, max(q, t))
    return k


def test_aligner_every_kind_in_three_band_classes_with_hints():
    """Every kind with one, two and four words per lane.  The class follows from the bound the caller proves: a 1500-base pair
    at 8 % edits under k = d, a 2200-base pair under k = 2000, a 4100-base pair under k = 4000 -- and the path is the oracle's
    whatever the bound."""
    eng = emu_engine()
    rng = np.random.default_rng(21)
    qs, ts, ks, classes = [], [], [], []
    for i, kind in enumerate(LC.KINDS):
        for n, k in ((1500, None), (2200, 2000), (4100, 4000)):
            q = LC.text(kind, 100 + i, n)
            t = H.mutate_seq(rng, q, 0.08)
            d = pyoracle.align(q.encode(), t.encode(), want_ops=False)[0]
            assert d <= (k or d)
            qs.append(q.encode()); ts.append(t.encode()); ks.append(k or d)
            classes.append((kind, band_words(len(q), len(t), k or d)))
    assert set(classes) == {(kind, g) for kind in LC.KINDS for g in (1, 2, 4)}
    check_pairs(eng, qs, ts, k_hint=ks)


def test_aligner_every_kind_without_a_hint_and_unequal_lengths():
    """Band doubling on every kind (one word per lane: 700 bases at 10 % edits), on pairs of unrelated texts of one kind whose
    distance takes the doubling to two and to four words per lane, and on very unequal lengths (the band is all offset)."""
    eng = emu_engine()
    rng = np.random.default_rng(22)
    qs, ts = [], []
    for i, kind in enumerate(LC.KINDS):
        q = LC.text(kind, 200 + i, 700)
        qs.append(q.encode()); ts.append(H.mutate_seq(rng, q, 0.10).encode())
    for kind, n in (('two_letter', 3300), ('homopolymer', 3300), ('two_letter', 6400), ('array', 6400)):
        qs.append(LC.text(kind, 300, n).encode()); ts.append(LC.text(kind, 301, n + 50).encode())
    words = []
    for q, t in zip(qs, ts):
        d = pyoracle.align(q, t, want_ops=False)[0]
        words.append(band_words(len(q), len(t), doubled_bound(len(q), len(t), d)))
    assert words.count(1) >= 12 and words.count(2) >= 2 and words.count(4) >= 2, words
    qs += [LC.text('tandem2', 310, 1000).encode(), LC.text('array171', 311, 300).encode(), LC.text('tandem1', 312, 40).encode()]
    ts += [LC.text('tandem2', 313, 2794).encode(), LC.text('array171', 311, 2100).encode(), LC.text('tandem1', 312, 900).encode()]
    check_pairs(eng, qs, ts)


MODEL_PAIRS = [('nanopore2023', 'nanopore2023'), ('pacbio2021', 'pacbio2021'), ('random', 'ideal')]


@pytest.mark.parametrize('em,qm', MODEL_PAIRS)
def test_sequence_fragments_on_low_complexity_fragments(em, qm):
    """Caller-supplied fragments, lengths 1 and 999 / 1000 / 1001 (the edges of ALIGNMENT_SIZE: aligned whole or by windows),
    40, 300 and 1.6-2.9 kb, through the mutate loop and the final stage: reads, qualities and statistics of the oracle.  Eight
    kinds per model pair, every kind under two of the three."""
    pref, _ = H.small_reference()
    eng, orc = H.configure(emu_engine(), pref, em, qm), H.configure(H.oracle_engine(), pref, em, qm)
    m = MODEL_PAIRS.index((em, qm))
    lengths = [1, 999, 1000, 1001, 1600, 2900, 40, 300]
    kinds = [LC.KINDS[(i + 4 * m) % len(LC.KINDS)] for i in range(8)]
    frags = [LC.codes(kind, 400 + i, lengths[(i + 3 * m) % 8], with_n=(i % 4 == 0)) for i, kind in enumerate(kinds)]
    targets = [(0.80, 0.97, 0.88, 0.93, 0.99)[(i + m) % 5] for i in range(8)]
    rh, sh = eng.sequence_fragments(31, 0, frags, targets)
    ro, so = orc.sequence_fragments(31, 0, frags, targets)
    for f in STAT_FIELDS:
        assert (sh[f] == so[f]).all(), (em, f)
    for i, (a, b) in enumerate(zip(rh, ro)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (em, kinds[i], len(frags[i]))


REPEAT_ROUTES = [
    {},                                                                                    # few reads: all head, in place
    {'BRX_HEAD_READS': 0, 'BRX_TAIL_READS': 0},                                            # every read in k_mut_lanes
    {'BRX_HEAD_READS': 5, 'BRX_TAIL_READS': 3},                                            # a head / tail split
    {'BRX_FIN_LANES': 0, 'BRX_QUAD_MIN_READS': 0},                                         # final alignments four per wave
    {'BRX_FIN_QUAD': 0, 'BRX_FIN_LANES': 0},                                               # ... all on whole waves
    {'BRX_HEAD_READS': 0, 'BRX_TAIL_READS': 0, 'BRX_MUTATE_PASSES': 1},                    # the bulk set through host-driven passes
    {'BRX_LANES_MIN_READS': 2048},                                                         # the shipped rule for small by-lane sets
]
REPEAT_PARAMS = dict(frag_mean=1100, frag_stdev=900)
REPEAT_SEED, REPEAT_READS = 1, 14                # (chosen so that one read leaves the default window: short reads rarely do)


@pytest.fixture(scope='module')
def repeat_rich_oracle():
    pref = LC.packed_reference('small')
    p = SimParams(**REPEAT_PARAMS)
    orc = H.configure(H.oracle_engine(), pref, 'nanopore2023', 'nanopore2023', p)
    out, st = orc.simulate_batch(REPEAT_SEED, 0, REPEAT_READS)
    return pref, p, out.copy(), st.copy()


@pytest.mark.parametrize('env', REPEAT_ROUTES, ids=lambda e: ','.join(f'{k[4:]}={v}' for k, v in e.items()) or 'default')
def test_pipeline_routes_on_the_repeat_rich_reference(env, repeat_rich_oracle, monkeypatch):
    """simulate_batch on the 50 kb repeat-rich reference (a splice of every kind, long period-2 stretches, a contig that ends
    inside a 171-mer array, a circular contig that is one array) against the oracle, on the routes of both stages.  The window
    of the traceback store is the DEFAULT one, and a final alignment leaves it all the same: the second phase -- the repeat
    with the full store -- runs without being forced."""
    pref, p, out_o, st_o = repeat_rich_oracle
    eng = H.configure(emu_engine(monkeypatch, **env), pref, 'nanopore2023', 'nanopore2023', p)
    out_h, st_h = eng.simulate_batch(REPEAT_SEED, 0, REPEAT_READS)
    for f in STAT_FIELDS:
        assert (st_h[f] == st_o[f]).all(), (env, f)
    assert H.first_diff(out_h, out_o) < 0, env
    assert eng.window_misses() >= 1, env
    if env.get('BRX_MUTATE_PASSES'):
        assert eng.mutate_passes() > 3
