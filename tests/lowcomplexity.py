"""
Low-complexity sequence for the parity tests: homopolymer mosaics, exact tandem repeats, diverged tandem arrays (satellites),
a two-letter alphabet, and splices of those with uniform stretches and short N runs.  Every other generator of the suite
(helpers.random_dna, helpers.recipe_fragment, tools/synth_refs.py) draws uniform bases; on sequence like this the aligners
are in another regime -- co-optimal paths everywhere (the canonical tie-break I, D, diagonal decides the whole path), long I/D
runs in the CIGAR windows, one k-mer row of the error model hit over and over, and a canonical path that leaves the straight
line by far more than a random walk does (the windowed traceback store, csrc/brx_align.h).

A plain helper module.  Every sequence is a pure function of (kind, seed, length) built from splitmix64 and integer
arithmetic only -- no library generator whose stream could change -- so a fixture keeps the recipe and not the text
(tests/golden/sequence_fragment_lowcomplexity.json.gz; tools/make_golden.py imports this module as it imports helpers).

    codes(kind, seed, length, with_n=False) -> uint8 codes 0-4 (A C G T N)        text(...) -> the same as a str
    repeat_rich_reference('small' | 'large') -> the arguments of PackedReference.from_seqs
"""
import collections

import numpy as np

# 'tandem' and 'array' take period / unit length and divergence from the seed; the numbered kinds pin them
KINDS = ('homopolymer', 'tandem', 'tandem1', 'tandem2', 'tandem3', 'tandem4', 'tandem5', 'tandem6', 'array', 'array171',
         'two_letter', 'mixed')
BASIC_KINDS = ('homopolymer', 'tandem', 'array', 'two_letter', 'mixed')
_M64 = (1 << 64) - 1


def _mix(x):
    """splitmix64's output function on an array of uint64."""
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


class _Stream(object):
    """Counter-based draws: word i of stream `key` is splitmix64(hash(key) + i)."""

    def __init__(self, *key):
        h = 0x243F6A8885A308D3
        for k in key:
            h = int(_mix(np.array([(h ^ (int(k) & _M64)) & _M64], dtype=np.uint64))[0])
        self.base, self.pos = h, 0

    def words(self, n):
        with np.errstate(over='ignore'):
            x = np.uint64(self.base) + np.arange(self.pos, self.pos + n, dtype=np.uint64)
        self.pos += n
        return _mix(x)

    def below(self, n):
        """One integer of [0, n) (n far below 2^32: the modulo bias does not matter for test input)."""
        return int(self.words(1)[0] >> np.uint64(32)) % n


def _distinct_walk(first, steps):
    """Codes 0-3 in which every element differs from the one before: first, first + s0, first + s0 + s1, ... with steps 1-3."""
    return ((first + np.concatenate([[0], np.cumsum(steps, dtype=np.int64)])) & 3).astype(np.uint8)


def _uniform(s, n):
    return (s.words(n) >> np.uint64(62)).astype(np.uint8)


def _homopolymer(s, n):
    """Runs with geometric lengths (a position starts a new run with probability 1 / mean, mean 8-60), each run a base other
    than the one before."""
    mean = 8 + s.below(53)
    w = s.words(n)
    starts = ((w >> np.uint64(32)) % np.uint64(mean)) == 0
    steps = np.where(starts, 1 + ((w >> np.uint64(8)) % np.uint64(3)).astype(np.int64), 0)
    return ((s.below(4) + np.cumsum(steps, dtype=np.int64)) & 3).astype(np.uint8)


def _unit(s, length):
    """A repeat unit without two equal neighbours, and whose last base differs from its first where the length allows: no period
    shorter than the unit for lengths 1-3, and no homopolymer at the joint."""
    if length == 1:
        return np.array([s.below(4)], dtype=np.uint8)
    while True:
        u = _distinct_walk(s.below(4), 1 + ((s.words(length - 1) >> np.uint64(40)) % np.uint64(3)).astype(np.int64))
        if u[-1] != u[0]:
            return u


def _tandem(s, n, period=None):
    period = period or 1 + s.below(6)
    u = _unit(s, period)
    phase = s.below(period)
    return np.resize(np.roll(u, -phase), n) if n else np.zeros(0, np.uint8)


def _array(s, n, unit_len=None):
    """Copies of one unit of 7-200 bases, every position of every copy changed with a probability of 0-3 % (per array: 0, 0.5, 1,
    2 or 3 %): half of the changes substitutions, a quarter deletions, a quarter duplications of the base."""
    unit_len = unit_len or 7 + s.below(194)
    permille = (0, 5, 10, 20, 30)[s.below(5)]
    u = _unit(s, unit_len)
    m = n + n // 16 + 8                                   # deletions shorten the text: draw some more, cut to n
    base = np.resize(np.roll(u, -s.below(unit_len)), m)
    w = s.words(m)
    hit = ((w >> np.uint64(32)) % np.uint64(1000)) < np.uint64(permille)
    how = ((w >> np.uint64(16)) & np.uint64(3)).astype(np.int64)
    step = 1 + ((w >> np.uint64(8)) % np.uint64(3)).astype(np.int64)
    base = np.where(hit & (how < 2), (base + step) & 3, base).astype(np.uint8)
    counts = np.ones(m, dtype=np.int64)
    counts[hit & (how == 2)] = 0
    counts[hit & (how == 3)] = 2
    return np.repeat(base, counts)[:n]


def _two_letter(s, n):
    a = s.below(4)
    b = (a + 1 + s.below(3)) & 3
    return np.where((s.words(n) >> np.uint64(63)) == 0, a, b).astype(np.uint8)


def _mixed(s, n, seg_max=None, n_odds=2):
    """Segments of every other kind and of uniform sequence, 60 bases up to seg_max (default: 3000, or a third of a short text);
    an array or a tandem segment of 200 bases or more carries one run of 2-40 N inside with a chance of 1 in n_odds."""
    seg_max = seg_max or max(61, min(3000, n // 3 + 61))
    parts, have = [], 0
    while have < n:
        length = min(n - have, 60 + s.below(seg_max - 60))
        which = s.below(6)
        seg = (_homopolymer, _tandem, _array, _two_letter, _uniform, _tandem)[which](s, length)
        if which == 5:
            seg = _tandem(s, length, 2)                   # period 2 has a share of its own: the paths that stray furthest
        if which in (1, 2, 5) and length >= 200 and s.below(n_odds) == 0:
            seg = seg.copy()
            run = 2 + s.below(39)
            at = s.below(length - run)
            seg[at:at + run] = 4
        parts.append(seg)
        have += length
    return np.concatenate(parts)[:n] if parts else np.zeros(0, np.uint8)


def codes(kind, seed, length, with_n=False):
    """Codes 0-4 of the sequence (kind, seed, length); with_n: one base in 256 of it replaced by N (the 'mixed' kind has N runs
    of its own)."""
    if kind not in KINDS:
        raise ValueError(f'unknown kind {kind!r}')
    s = _Stream(KINDS.index(kind), seed, length)
    n = int(length)
    if kind == 'homopolymer':
        out = _homopolymer(s, n)
    elif kind.startswith('tandem'):
        out = _tandem(s, n, int(kind[6:]) if kind[6:] else None)
    elif kind.startswith('array'):
        out = _array(s, n, int(kind[5:]) if kind[5:] else None)
    elif kind == 'two_letter':
        out = _two_letter(s, n)
    else:
        out = _mixed(s, n)
    out = np.array(out, dtype=np.uint8)
    assert len(out) == n
    if with_n:
        out[(_Stream(0x4E, seed, length).words(n) >> np.uint64(20)) & np.uint64(255) == 0] = 4
    return out


def text(kind, seed, length, with_n=False):
    return np.frombuffer(b'ACGTN', dtype=np.uint8)[codes(kind, seed, length, with_n)].tobytes().decode()


def kind_of(i):
    """Kind number i of a round over all kinds (test loops)."""
    return KINDS[i % len(KINDS)]


# ------------------------------------------------------------------------------------------------
REFERENCE_SIZES = {'small': 1, 'large': 64}
_refs = {}


def repeat_rich_reference(size='small'):
    """(seqs, depths, circular, hairpin_left, hairpin_right) for PackedReference.from_seqs: 'small' is about 50 kb (CPU tests),
    'large' 64 times that plus 500 short scaffolds (3.4 Mb: the GPU tests).

      chrom      circular   a splice of every kind (segments up to 8 kb; 64 kb in 'large') with uniform stretches and N runs
      dinuc      linear     long period-2 and period-1..6 stretches between short uniform ones: the fragments whose canonical
                            path leaves the windowed traceback store
      lin_sat    linear     uniform sequence that runs into a 171-mer array: the contig ENDS inside the array (clipped reads)
      sat_circle circular   nothing but one diverged 171-mer array, with depth
      scaf0000.. linear     'large' only: 500 scaffolds of 300-1000 bases, each one tandem repeat or one diverged array, at depth
                            1.4 -- unplaced satellite scaffolds.  A fragment drawn from one is clipped to it, so a tenth of a
                            batch's reads are short, with a final band narrow enough for one read per lane.  The share is
                            chosen for the shipped rules of the final stage at 16 384 reads: the bulk set then holds more than
                            2048 reads for the one-per-lane route AND more than 4096 mid-sized ones for four per wave
                            (BRX_LANES_MIN_READS, BRX_QUAD_MIN_READS); with no scaffolds the first route stays empty, with a
                            third of the reads from scaffolds the second

    'large' keeps N runs rare in chrom (1 in 6 eligible segments; 'small': 1 in 2): a read with an N is not aligned by lane or
    four per wave, and at one run per 6 kb hardly a 15 kb read would be without.
    """
    if size in _refs:
        return _refs[size]
    f = REFERENCE_SIZES[size]
    txt = np.frombuffer(b'ACGTN', dtype=np.uint8)
    s = _Stream(0x5EF, f)
    chrom = _mixed(s, 24000 * f, seg_max=8000 * (8 if f > 1 else 1), n_odds=6 if f > 1 else 2)
    parts = []
    for i in range(4 * (4 if f > 1 else 1)):
        n = 2500 * f // (4 if f > 1 else 1)
        parts.append(_tandem(s, n, 2 if i % 2 == 0 else None))
        parts.append(_uniform(s, 300))
    dinuc = np.concatenate(parts)
    lin_sat = np.concatenate([_uniform(s, 3000 * f), _array(_Stream(0x171, f, 1), 5000 * f, 171)])
    sat_circle = _array(_Stream(0x171, f, 2), 171 * 35 * f, 171)
    contigs = [('chrom', chrom), ('dinuc', dinuc), ('lin_sat', lin_sat), ('sat_circle', sat_circle)]
    depths = {'chrom': 1.0, 'dinuc': 1.5, 'lin_sat': 1.0, 'sat_circle': 3.0}
    circ = {'chrom': True, 'dinuc': False, 'lin_sat': False, 'sat_circle': True}
    if f > 1:
        sc = _Stream(0x5CAF, f)
        for i in range(500):
            n = 300 + sc.below(701)
            contigs.append((f'scaf{i:04d}', _tandem(sc, n) if i % 2 else _array(sc, n)))
            depths[contigs[-1][0]], circ[contigs[-1][0]] = 1.4, False
    seqs = collections.OrderedDict((name, txt[c].tobytes().decode()) for name, c in contigs)
    none = {name: False for name in seqs}
    _refs[size] = (seqs, depths, circ, dict(none), dict(none))
    return _refs[size]


def packed_reference(size='small'):
    from badread_amd.reference import PackedReference
    key = ('packed', size)
    if key not in _refs:
        _refs[key] = PackedReference.from_seqs(*repeat_rich_reference(size))
    return _refs[key]


# ------------------------------------------------------------------------------------------------
# simulate_batch cases on the large reference (tests/test_gpu_lowcomplexity.py; tests/oracle_slice_worker.py computes the
# oracle's side of 'lowcomplexity:<case>' in processes of its own): error model, qscore model, --identity mean,max,stdev
# (pacbio2021: the qscore-distributed --identity 30,3), other parameters
SIM_CASES = {
    'default': ('nanopore2023', 'nanopore2023', (95.0, 99.0, 2.5), {}),
    'hifi': ('pacbio2021', 'pacbio2021', (30.0, None, 3.0), {}),
    'rough': ('nanopore2023', 'nanopore2023', (85.0, 95.0, 5.0),
              dict(chimera_rate=0.25, glitch_rate=1000.0, glitch_size=100.0, glitch_skip=100.0)),
    'random_ideal': ('random', 'ideal', (95.0, 99.0, 2.5), {}),
    'nanopore2018': ('nanopore2018', 'nanopore2018', (95.0, 99.0, 2.5), {}),
}


def configure_case(engine, case, size='large'):
    """`engine` set up for a case of SIM_CASES on the repeat-rich reference: --length 15000,13000 and the case's parameters."""
    import io
    import helpers
    from badread_amd.engine import SimParams
    from badread_amd.identities import Identities
    em, qm, (mean, mx, sd), extra = SIM_CASES[case]
    mode, a, b, id_max = Identities(mean, sd, mx, io.StringIO()).device_mode()
    params = SimParams(frag_mean=15000.0, frag_stdev=13000.0, identity_mode=mode, id_a=a, id_b=b, id_max=id_max, **extra)
    return helpers.configure(engine, packed_reference(size), em, qm, params)
