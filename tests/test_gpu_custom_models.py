"""
GPU parity under user-supplied model files (tests/custom_models.py; the CPU side is tests/test_custom_models.py): everything
through the C-ABI, everything compared bit for bit -- the arithmetic is integer plus the shared FP64 spec, so there is no tolerance.

The models select what no packaged model selects: in dev_propose_row / brx_prop_word the long flag (by length and by k = 9), k = 3
and k = 8, absent rows, rows that sum to 1 and more, an alternative equal to its k-mer, the block edges of the threshold scan,
strings of 16-127 characters on one position; in k_fin_qscore gap_bits = 4, k = 1 / 3 / 11, no hot row, a hot row beyond
BRX_QS_HOT_MAX, equal thresholds, D-runs beyond the field, BRX_RS_QMISS; and the window overflow into k_mutate with inline
alignments, which the rest of the suite reaches on the interpreted kernels only.

Every batch test prints one line: the reads compared, the route counts (brx_last_read_cycles word 7) and the seconds.
"""
import gzip
import io
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import custom_models as CM
import helpers as H
from badread_amd.error_model import ErrorModel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NULL = io.StringIO()
ALL_FIELDS = ('status', 'frag_len', 'seq_len', 'n_cols', 'n_match', 'padded_len', 'loop_count', 'change_count', 'n_alignments',
              'rec_len', 'target_identity', 'qerr_sum')
ROUTES = {'default': {}, 'bulk': {'BRX_TAIL_READS': '0', 'BRX_HEAD_READS': '0'},
          'bulk_passes': {'BRX_TAIL_READS': '0', 'BRX_HEAD_READS': '0', 'BRX_MUTATE_PASSES': '1'}}
SEED = 23


def configured(engine, em, qm):
    pref, _ = H.small_reference()
    H.configure(engine, pref)
    engine.set_error_model(CM.error_tables(em))
    engine.set_qscore_model(CM.qscore_tables(qm) if isinstance(qm, str) else qm)
    return engine


def compare(tag, hip, frags, targets, oracle, first=0):
    """One sequence_fragments call on `hip` against the oracle's (results, statistics): ALL_FIELDS and every byte.  Returns the
    statistics and the route words."""
    ro, so = oracle
    t0 = time.perf_counter()
    rh, sh = hip.sequence_fragments(SEED, first, frags, targets)
    gpu_s = time.perf_counter() - t0
    route = hip.read_cycles(len(frags))[:, 7].astype(np.int64)
    words = route & 0xFFFF
    print(f'\ncustom_models {tag}: ' + json.dumps({
        'reads_compared': len(frags), 'bases': int(sh['seq_len'].sum()), 'window_misses': hip.window_misses(), 'mutate_passes': hip.mutate_passes(),
        'band_words': {str(g): int((words == g).sum()) for g in sorted(set(words.tolist()))},
        'four_per_wave': int(((route >> 16) & 1).sum()), 'one_per_lane': int(((route >> 17) & 1).sum()), 'gpu_seconds': round(gpu_s, 2)}))
    for f in ALL_FIELDS:
        bad = np.flatnonzero(sh[f] != so[f])
        assert len(bad) == 0, f'{tag}: {f} of read {int(bad[0])} (and {len(bad) - 1} more) differs: hip {sh[f][bad[:4]]} oracle {so[f][bad[:4]]}'
    for i, ((a, qa), (b, qb)) in enumerate(zip(rh, ro)):
        assert H.first_diff(a, b) < 0, f'{tag}: sequence of read {i} differs at {H.first_diff(a, b)}'
        assert H.first_diff(qa, qb) < 0, f'{tag}: qualities of read {i} differ at {H.first_diff(qa, qb)}'
    return sh, route


# ------------------------------------------------------------------------------------------------ digests and tables
def test_digest_cases_through_the_c_abi():
    """tests/golden/sequence_fragment_custom_models.json.gz -- the unmodified reference's sequence_fragment replayed with our draws
    under the model files -- through the HIP path: sequence, qualities, identity, loop and alignment counts of every case."""
    with gzip.open(os.path.join(HERE, 'golden', 'sequence_fragment_custom_models.json.gz'), 'rt') as f:
        cases = json.load(f)['cases']
    assert len(cases) >= 60
    hip = H.hip_engine()
    current = [None]

    def engine_of(em, qm):
        if current[0] != (em, qm):
            configured(hip, em, qm)
            current[0] = (em, qm)
        return hip
    t0 = time.perf_counter()
    H.check_digest_cases(engine_of, sorted(cases, key=lambda c: (c['em'], c['qm'])))
    print(f'\ncustom_models digests: {len(cases)} cases, {time.perf_counter() - t0:.2f} s')


@pytest.mark.parametrize('name', CM.ERROR_MODELS)
def test_loader_inner_alignments_on_the_device_equal_the_oracles(name):
    """SURVEY.md row a4 on synthetic alternatives: the loader aligns every alternative to its k-mer in one batch on the device;
    the flattened tables equal, array for array, the ones built with the oracle's aligner."""
    ours = ErrorModel(CM.path_of(name), NULL, use_cache=False).tables()
    want = CM.error_tables(name)
    assert set(ours) == set(want)
    for key in want:
        assert np.array_equal(ours[key], want[key]), (name, key)


# ------------------------------------------------------------------------------------------------ batches per pair
@pytest.fixture(scope='module')
def oracle_batch():
    """The input of a pair's batch and the oracle's result, computed ONCE: the three routes compare with the same bytes."""
    cache = {}

    def get(pair):
        if pair not in cache:
            frags, targets = CM.batch(CM.PAIRS.index(pair), 256, 600, 2500)
            cache[pair] = (frags, targets, configured(H.oracle_engine(), *pair).sequence_fragments(SEED, 0, frags, targets))
        return cache[pair]
    return get


@pytest.mark.parametrize('route', sorted(ROUTES))
@pytest.mark.parametrize('pair', CM.PAIRS, ids='+'.join)
def test_batches_of_256_fragments_equal_the_oracle(pair, route, oracle_batch, monkeypatch):
    """256 fragments of 600-2500 bases (0.4 Mbases), targets spread over 0.6-0.99, on a fresh engine under the default route,
    with every read in the bulk set (k_mut_fill and k_mut_lanes carry full waves), and with the bulk set on host-driven passes."""
    from badread_amd.engine import HipEngine
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    frags, targets, oracle = oracle_batch(pair)
    assert len(frags) == 256 and all(600 <= len(f) <= 2500 for f in frags) and min(targets) == 0.6 and max(targets) == 0.99
    eng = configured(HipEngine(0, scratch_bytes=2 << 30), *pair)
    try:
        sh, route_words = compare(f'{pair[0]}+{pair[1]} {route}', eng, frags, targets, oracle)
        if route == 'bulk_passes':
            assert eng.mutate_passes() > 3
        if route == 'bulk':
            assert eng.mutate_passes() <= 3                      # ONE launch of k_mut_lanes for the bulk set
    finally:
        eng.close()
    assert (sh['status'] == 0).all()
    # at least two routes of the final stage per pair (whole waves of one word per lane, and one read per lane for the narrow
    # bands of the fragments without N; the wide classes are test_window_overflow_goes_through_the_whole_read_kernel's)
    assert len(set((route_words & 0x3FFFF).tolist())) >= 2, 'one band-class route only'


def test_window_overflow_goes_through_the_whole_read_kernel():
    """tests/test_emulated_device.py::_window_overflow on the device: e3_big's 60-base insertions make the joined windows outgrow
    their pass slots, so the reads go to k_mutate with inline alignments, and reads of many times the fragment's length reach the
    widest band classes.  The two fragments of that test (560 and 300 bases at 0.05 and 0.3) and 62 more of 200-600 bases."""
    rng = np.random.default_rng(4)
    frags = [rng.integers(0, 4, n).astype(np.uint8) for n in (560, 300)]
    more, targets = CM.batch(99, 62, 200, 600)
    frags += more
    targets = [0.05, 0.3] + [round(0.3 + 0.6 * i / 61, 4) for i in range(62)]
    oracle = configured(H.oracle_engine(), 'e3_big', 'ideal').sequence_fragments(SEED, 0, frags, targets)
    sh, route = compare('e3_big+ideal overflow', configured(H.hip_engine(), 'e3_big', 'ideal'), frags, targets, oracle)
    assert int(sh['padded_len'][0]) > 8 * 560                       # the windows really overflowed
    assert int((route & 0xFFFF).max()) >= 8                         # 8 or 16 words per lane in the final alignment


def test_a_fallback_that_ends_without_a_row_sets_qmiss():
    """q3_gaps without its 'X' row (the table level: the host class refuses such a file): score 0 and BRX_RS_QMISS exactly where
    the oracle has them."""
    from test_custom_models import qmiss_case
    t, frags, targets, ro, so = qmiss_case()
    hip = configured(H.hip_engine(), 'nanopore2023', t)
    rh, sh = hip.sequence_fragments(17, 0, frags, targets)
    for f in ALL_FIELDS:
        assert (sh[f] == so[f]).all(), f
    for (a, qa), (b, qb) in zip(rh, ro):
        assert np.array_equal(a, b) and np.array_equal(qa, qb)


def test_cli_with_model_files_matches_the_oracle_driver(tmp_path, monkeypatch):
    """`badread simulate --error_model FILE --qscore_model FILE` end to end against the same driver on the oracle engine."""
    from badread_amd import simulate as S
    from test_host_simulate import Args, parse_fastq
    em, qm = (os.path.join('tests', 'golden', 'models', n) for n in ('e9_sparse', 'q9_gap4'))
    cmd = [sys.executable, '-m', 'badread_amd', 'simulate', '--reference', os.path.join('tests', 'golden', 'small_ref.fasta'),
           '--quantity', '5x', '--error_model', em, '--qscore_model', qm, '--seed', '7']
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, timeout=600, env=dict(os.environ, BADREAD_AMD_CACHE=str(tmp_path / 'cli')))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    recs = parse_fastq(r.stdout)
    assert sum(len(x[1]) for x in recs) >= 5 * 3621 and f'Loading error model from {em}' in r.stderr.decode()
    monkeypatch.setenv('BADREAD_AMD_CACHE', str(tmp_path / 'driver'))
    args = Args(quantity='5x', mean_frag_length=15000.0, frag_length_stdev=13000.0, mean_identity=95.0, max_identity=99.0,
                identity_stdev=2.5, error_model=os.path.join(REPO, em), qscore_model=os.path.join(REPO, qm), seed=7,
                junk_reads=1, random_reads=1, chimeras=1)
    sink = io.BytesIO()
    S.simulate(args, output=io.StringIO(), engine=H.oracle_engine(), stdout=sink, shard=S.Shard())
    assert sink.getvalue() == r.stdout
    print(f'\ncustom_models cli: {len(recs)} reads, {time.perf_counter() - t0:.2f} s')
