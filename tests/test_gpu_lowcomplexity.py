"""
GPU parity on low-complexity sequence (tests/lowcomplexity.py): homopolymer mosaics, tandem repeats of period 1-6, diverged
arrays (a 171-mer among them), a two-letter alphabet, splices with N runs -- everything through the C-ABI, everything compared
with the oracle bit for bit.  The rest of the GPU suite feeds the kernels uniform bases; here

  * every alignment has co-optimal paths all along, so the tie-break (I, then D, then diagonal) decides the whole path;
  * the CIGAR windows of k_fin_qscore hold long I/D runs;
  * the canonical path of a final alignment strays from the straight line far beyond 2 sqrt(ub) + 24 rows on period-2
    stretches: the second phase of the final stage (the repeat with the full traceback store) is a COMMON route under the
    default window, with hundreds of reads of one batch in it at once;
  * and all of that at a size where the bulk routes fill up -- 64 reads per wave in k_mut_lanes, k_fin_quad, k_fin_lanes.

Route assertions come from the kernels' own records (brx_last_read_cycles, brx_last_window_misses), so that a changed threshold
cannot empty a route silently.  Every simulate_batch test prints one line: reads compared, window misses, retries (recorded,
not asserted: an arena that is short is grown and the batch repeated, which is correct), route counts, seconds.
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

import helpers as H
import lowcomplexity as LC
import pyoracle
from badread_amd.error_model import ErrorModel
from badread_amd.qscore_model import QScoreModel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NULL = io.StringIO()
SEED = 42
ALL_FIELDS = ('status', 'frag_len', 'seq_len', 'n_cols', 'n_match', 'padded_len', 'loop_count', 'change_count', 'n_alignments',
              'rec_len', 'target_identity', 'qerr_sum')
SCRATCH = 30 << 30


# ------------------------------------------------------------------------------------------------ align_batch
def _check(queries, targets, k_hint=None):
    eng = H.hip_engine()
    ops, dist, ncols, nmatch = eng.align_batch(queries, targets, k_hint=k_hint)
    for i, (q, t) in enumerate(zip(queries, targets)):
        d, o = pyoracle.align(q, t)
        assert dist[i] == d, f'pair {i}: distance {dist[i]} != {d} (|q|={len(q)}, |t|={len(t)})'
        assert ncols[i] == len(o)
        assert nmatch[i] == int((o == 0).sum())
        fd = H.first_diff(ops[i], o)
        assert fd < 0, f'pair {i}: path differs at column {fd} (|q|={len(q)}, |t|={len(t)}, d={d})'


def test_small_pairs_of_every_kind():
    """Every kind at every size of test_gpu_align.py::test_random_pairs_small, five times over: 1080 pairs; one in five against
    another text of the same kind instead of a mutated copy."""
    rng = np.random.default_rng(15)
    sizes = [1, 2, 3, 5, 10, 31, 32, 33, 63, 64, 65, 100, 128, 129, 200, 500, 1000, 1500]
    qs, ts = [], []
    for it in range(5 * len(LC.KINDS) * len(sizes)):
        kind, n = LC.KINDS[it % len(LC.KINDS)], sizes[(it // len(LC.KINDS)) % len(sizes)]
        q = LC.text(kind, it, n)
        if it % 5 == 0:
            t = LC.text(kind, it + 1, int(rng.integers(1, 2 * n + 1)))
        else:
            t = H.mutate_seq(rng, q, float(rng.choice([0, 0.01, 0.05, 0.2, 0.5]))) or 'A'
        qs.append(q.encode())
        ts.append(t.encode())
    assert len(qs) >= 1000
    _check(qs, ts)


def test_mid_sizes_with_and_without_bound():
    rng = np.random.default_rng(16)
    qs, ts, ks = [], [], []
    for kind, n, rate in (('tandem2', 3000, 0.05), ('homopolymer', 5000, 0.1), ('array171', 15000, 0.05), ('tandem2', 15000, 0.15),
                          ('mixed', 30000, 0.03), ('two_letter', 4000, 0.4), ('tandem1', 8000, 0.1), ('tandem3', 12000, 0.08),
                          ('array', 20000, 0.12), ('tandem6', 6000, 0.2)):
        q = LC.text(kind, n, n)
        t = H.mutate_seq(rng, q, rate)
        qs.append(q.encode())
        ts.append(t.encode())
        ks.append(pyoracle.align(q.encode(), t.encode(), want_ops=False)[0] + 7)
    _check(qs, ts)
    _check(qs, ts, k_hint=ks)


def test_long_pairs_with_bounds():
    """60-200 kb at 3-25 % edits, period-2 repeats and 171-mer arrays among them: the pairs whose canonical path strays furthest
    from the straight line (a 15 kb period-2 pair at 12 % edits: 292 rows, where a uniform one stays within 33)."""
    rng = np.random.default_rng(17)
    qs, ts, ks = [], [], []
    for kind, n, rate in (('tandem2', 60000, 0.25), ('array171', 120000, 0.08), ('tandem2', 200000, 0.03), ('array171', 60000, 0.12),
                          ('mixed', 100000, 0.05), ('tandem2', 80000, 0.12)):
        q = LC.text(kind, n + 1, n)
        t = H.mutate_seq(rng, q, rate)
        qs.append(q.encode())
        ts.append(t.encode())
        ks.append(pyoracle.align(q.encode(), t.encode(), want_ops=False)[0] + 7)
    _check(qs, ts, k_hint=ks)


# ------------------------------------------------------------------------------------------------ sequence_fragments
def test_low_complexity_digest_cases_through_the_c_abi():
    """tests/golden/sequence_fragment_lowcomplexity.json.gz -- the unmodified reference's sequence_fragment replayed with our draws
    on low-complexity fragments -- through the HIP path: sequence, qualities, identity and loop count of every case."""
    with gzip.open(os.path.join(HERE, 'golden', 'sequence_fragment_lowcomplexity.json.gz'), 'rt') as f:
        g = json.load(f)
    assert len(g['cases']) >= 200
    hip = H.hip_engine()
    current = [None]

    def engine_of(em, qm):
        if current[0] != (em, qm):
            hip.set_error_model(ErrorModel(em, NULL).tables())
            hip.set_qscore_model(QScoreModel(qm, NULL).tables())
            current[0] = (em, qm)
        return hip
    H.check_digest_cases(engine_of, sorted(g['cases'], key=lambda c: (c['em'], c['qm'])))


# ------------------------------------------------------------------------------------------------ simulate_batch
@pytest.fixture(autouse=True)
def shipped_final_stage_rules(monkeypatch):
    """tests/conftest.py runs the suite with BRX_LANES_MIN_READS=0; full batches run the shipped default (tests/test_gpu_fullsize.py)."""
    monkeypatch.delenv('BRX_LANES_MIN_READS', raising=False)


def usable_cores():
    cores = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            cores = max(1, min(cores, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return max(1, min(cores, 16))


def oracle_slices(case, n, tmp):
    """Reads [0, n) of a case through the oracle: one process per usable core (at most 16) on disjoint slices, none of them with a
    device.  Returns the FASTQ bytes and the statistics."""
    cores = usable_cores()
    per = -(-n // cores)
    env = dict(os.environ, OMP_NUM_THREADS='1', OPENBLAS_NUM_THREADS='1', MKL_NUM_THREADS='1', HIP_VISIBLE_DEVICES='')
    procs = []
    for i in range(cores):
        first, count = i * per, max(0, min(per, n - i * per))
        if count == 0:
            continue
        path = str(tmp / f'slice{i}.npz')
        procs.append((path, subprocess.Popen([sys.executable, os.path.join(HERE, 'oracle_slice_worker.py'), f'lowcomplexity:{case}', '-',
                                              str(SEED), str(first), str(count), path], env=env,
                                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)))
    data, stats = [], []
    for path, pr in procs:
        _, err = pr.communicate(timeout=1500)
        assert pr.returncode == 0, err.decode()[-2000:]
        z = np.load(path)
        data.append(z['data'].tobytes())
        stats.append(z['stats'])
    return b''.join(data), np.concatenate(stats)


@pytest.fixture(scope='module')
def oracle_batch(tmp_path_factory):
    """The oracle's result of (case, n), computed ONCE per parameter set: the route variants of a case compare with the same bytes."""
    cache = {}

    def get(case, n):
        if (case, n) not in cache:
            t0 = time.perf_counter()
            cache[(case, n)] = oracle_slices(case, n, tmp_path_factory.mktemp(f'oracle_{case}')) + (time.perf_counter() - t0,)
        return cache[(case, n)]
    return get


def run_case(case, n, oracle_batch, label=None):
    """One batch of `case` on a fresh engine (it reads the environment when it is created) against the oracle: every read, the
    FASTQ bytes and ALL_FIELDS.  Returns what the kernels recorded about the routes."""
    from badread_amd.engine import HipEngine, RS_EMPTY
    raw_o, st_o, oracle_s = oracle_batch(case, n)
    eng = LC.configure_case(HipEngine(0, scratch_bytes=SCRATCH), case)
    t0 = time.perf_counter()
    out, st = eng.simulate_batch(SEED, 0, n)
    gpu_s = time.perf_counter() - t0
    out, st = out.copy(), st.copy()
    route = eng.read_cycles(n)[:, 7]
    rec = {'case': label or case, 'reads_compared': n, 'live_reads': int((st['rec_len'] > 0).sum()), 'window_misses': eng.window_misses(),
           'retries': int(getattr(eng, 'retries', 0)), 'mutate_passes': eng.mutate_passes(),
           'four_per_wave': int(((route >> 16) & 1).sum()), 'one_per_lane': int(((route >> 17) & 1).sum()),
           'band_words': {str(g): int(((route & 0xFFFF) == g).sum()) for g in sorted(set((route & 0xFFFF).tolist()))},
           'bases': int(st['seq_len'].sum()), 'gpu_seconds': round(gpu_s, 2), 'oracle_seconds': round(oracle_s, 1)}
    eng.close()
    print('\nlowcomplexity ' + json.dumps(rec))
    assert (st['status'] & ~np.uint32(RS_EMPTY) == 0).all()
    for f in ALL_FIELDS:
        bad = np.flatnonzero(st[f] != st_o[f])
        assert len(bad) == 0, f'{rec["case"]}: {f} of read {int(bad[0])} (and {len(bad) - 1} more) differs from the oracle'
    raw = out.tobytes()
    if raw != raw_o:
        for r in range(n):
            lo, ln = int(st['rec_off'][r]), int(st['rec_len'][r])
            assert raw[lo:lo + ln] == raw_o[lo:lo + ln], f'{rec["case"]}: the record of read {r} differs from the oracle'
        assert False, f'{rec["case"]}: FASTQ bytes differ from the oracle'
    rec['words'] = (route & 0xFFFF).astype(np.int64)
    return rec


N_DEFAULT = 16384


def test_default_parameters_full_batch_equals_the_oracle(oracle_batch):
    """16384 reads of the 3 Mb repeat-rich reference, nanopore2023, default parameters, shipped environment: every read and
    every statistic.  A batch like this sends well over 0.4 % of its reads through the second phase of the final stage under
    the DEFAULT window (the 64-read prefix of this batch on the interpreted kernels: see DESIGN.md), and fills both the
    four-per-wave and the one-per-lane route."""
    rec = run_case('default', N_DEFAULT, oracle_batch)
    assert rec['window_misses'] >= 0.004 * rec['live_reads'], rec['window_misses']
    assert rec['four_per_wave'] >= 1000 and rec['one_per_lane'] >= 1000, (rec['four_per_wave'], rec['one_per_lane'])


@pytest.mark.parametrize('env', [{'BRX_MUTATE_PASSES': '1'}, {'BRX_FIN_LANES': '0', 'BRX_QUAD_MIN_READS': '0'},
                                 {'BRX_FIN_QUAD': '0', 'BRX_FIN_LANES': '0'}, {'BRX_TB_WINDOW': '0'}],
                         ids=lambda e: ','.join(f'{k[4:]}={v}' for k, v in e.items()))
def test_default_parameters_full_batch_on_other_routes(env, oracle_batch, monkeypatch):
    """The same batch, the same oracle bytes: the bulk set through host-driven passes; every narrow band four per wave; every
    final alignment on a whole wave; the full traceback store (no read may miss then)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rec = run_case('default', N_DEFAULT, oracle_batch, label='default ' + ' '.join(f'{k}={v}' for k, v in env.items()))
    if 'BRX_MUTATE_PASSES' in env:
        assert rec['mutate_passes'] > 3
    if env.get('BRX_TB_WINDOW') == '0':
        assert rec['window_misses'] == 0
    else:
        assert rec['window_misses'] >= 0.004 * rec['live_reads']
    if env.get('BRX_FIN_LANES') == '0':
        assert rec['one_per_lane'] == 0
    if env.get('BRX_FIN_QUAD') == '0':
        assert rec['four_per_wave'] == 0


@pytest.mark.parametrize('case,n', [('hifi', 16384), ('rough', 4096), ('random_ideal', 4096), ('nanopore2018', 4096)])
def test_other_parameter_sets_equal_the_oracle(case, n, oracle_batch):
    """pacbio2021 with --identity 30,3 (nearly every read aligned by lane); --identity 85,95,5 --chimeras 25 --glitches 1000,100,100
    (wide bands); the random / ideal models (k = 1); nanopore2018.

    The pacbio2021 batch has 16384 reads, not 8192: under the shipped rules the 1024 longest reads of a batch are the head set
    (BRX_HEAD_READS), and a set of fewer than 2048 by-lane reads (BRX_LANES_MIN_READS) keeps them on whole waves -- the head set
    never goes by lane.  Of 8192 reads at most 87.5 % can, whatever the input (measured: 7079, which is 98.8 % of the bulk set);
    the bar of 90 % of the live reads needs a batch of more than 10240."""
    rec = run_case(case, n, oracle_batch)
    if case == 'hifi':
        assert rec['one_per_lane'] >= 0.9 * rec['live_reads'], (rec['one_per_lane'], rec['live_reads'])
    if case == 'rough':
        assert int((rec['words'] >= 8).sum()) >= 100, rec['band_words']
