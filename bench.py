#!/usr/bin/env python3
"""
bench.py -- simulated bases per second of the HIP hot path on N MI355X (one process per GPU).

    python bench.py --gpus N --steps K --warmup W [--workload human|hifi|kpn] [--dump-outputs DIR] [--full]

With N > 1 and no WORLD_SIZE in the environment the script re-executes itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`, one rank per GPU; a
WORLD_SIZE that differs from --gpus is an error (it never silently measures fewer GPUs than asked for).

Workloads (BASELINE.json configs; tools/synth_refs.py writes the references as FASTA and they
are loaded through the native packer brx_fasta_pack + its sidecar, like a user's genome):
  human  (default) configs[3], the configuration the metric is quoted on: synthetic GRCh38-like reference -- 24 LINEAR
         contigs with the GRCh38 primary chromosome lengths (3 088 269 832 bp = 772 MB packed, one replica per GPU),
         uniform ACGT, 10 kb of N at both ends of every contig, a 1 Mb N run inside chr1, chr9, chrX -- default
         `badread simulate` parameters (--length 15000,13000 --identity 95,99,2.5, nanopore2023 error + qscore models,
         default adapters, junk/random/chimera 1 %, glitches 10000,25,25), seed 42
  hifi   configs[4]: the same reference, --error_model pacbio2021 --qscore_model pacbio2021 --identity 30,3
  kpn    configs[1]: 5.5 Mb K. pneumoniae-like reference (3 circular contigs, numpy default_rng(1)), defaults (round 1's line)

A "step" is ONE pass of the whole hot path (plan -> fragments -> mutate -> align -> qscores -> FASTQ bytes) over
one batch of `--reads-per-step` read indices per GPU (default 393216 reads x 15 kb ~ 5.9 Gbases; the 30x job is 16 such
steps on one GPU).  The batch goes through the C-ABI as `--streams` device batches (brx_simulate_batch, 6 x 65536
reads by default: measured best on the MI355X among 4..8 batches of 49152..98304 reads -- round 3's slab traceback stores
made the bigger batch fit a SMALLER arena, 6 x 40 GB) that are in flight together, one context + HIP stream + host thread each; device batches of
consecutive steps follow each other without a barrier, exactly as the CLI driver runs them
(badread_amd.simulate.run_batches).  Inputs (packed reference, model tables) are resident in HBM before the timed
region; the FASTQ bytes stay in HBM (`--d2h` adds the PCIe-inclusive rate as `value_incl_d2h`).  Weak scaling: every
rank processes its own slices of the read-index space; no collective on the data path.

`--scaling strong` (round 6; never the driver's default line) measures the JOB the metric names instead: a fixed total -- the
`--quantity`x job of the workload (30x of 3.09 Gb = 92.6 Gbases = 95 device batches of 65536 reads) -- split over the N ranks by
device batch, with every rank's START-UP INSIDE THE CLOCK (the clock starts at the first line of this file: interpreter, torch,
reference, engines and arenas, model tables, priming).  The line then carries `fixed_cost_s` (start of the process to the first
batch, the slowest rank), `loop_s`, `value` = job bases / (fixed + loop), `value_loop`, and `projected_wall_s` for 1 / 2 / 4 / 8
ranks from the measured fixed cost and loop -- what a scaling box would see, since the fixed cost does not shrink with N.

A plain run sets up, warms up, times the K steps and prints the line: `value` (simulated bases/s, all ranks), `ms_per_step` (wall
time of one timed step), the stage times the library records anyway, the host's share.  `--dump-outputs DIR` then writes what the
last timed step computed (dump_outputs(): per-read statistics, a seeded sample of whole FASTQ records, per-batch byte sums) as
.npy files; the inputs are seeded, so two builds run with the same arguments compare output for output.

With `--full` the kernels are timed launch by launch (HIP events; extra synchronisation inside every batch) and the JSON line carries
  roofline       the kernel with the largest summed launch time in this very run (per-kernel HIP events around
                 every launch, on the stream the kernel is launched on: brx_last_kernel_stats), HBM bound, algorithmic
                 bytes = 2.26 B per simulated base x the bases that kernel handled / its launches
  roofline_alu   wave-level VALU instructions issued per second (from the committed SQ_INSTS_VALU count per base,
                 profiles/) against the chip's VALU issue rate -- the roofline that actually bounds this integer path
  cpu_baseline   the C oracle (a single-threaded port of the same algorithm) on every usable host core of this box,
                 on a bounded sample of the same workload; `reference` inside it is the UNMODIFIED Python reference +
                 edlib shim measured in the CPU container by tools/ref_cpu_baseline.py (profiles/cpu_reference_baseline.json)
"""
import time as _time
T_PROCESS = _time.perf_counter()       # --scaling strong: the clock of a rank starts here, before torch is imported
import argparse
import os as _os
_os.environ.setdefault('GPU_MAX_HW_QUEUES', '32')      # a hardware queue per stream of every in-flight batch (HIP's default of 4 serialises them)
import json
import os
import sys
import threading
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (REPO, os.path.join(REPO, 'tools')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ALGO_BYTES_PER_BASE = 2.26          # 0.25 B packed reference read + 2 B FASTQ written + header share
HBM_PEAK_GBS = 8000.0               # MI355X_MICROARCH.md: 8.0 TB/s spec
SCRATCH_GB_DEFAULT = 32.0           # scratch arena per in-flight device batch (tests/test_gpu_fullsize.py runs the shipped geometry with it); 40 until the mutate stage's buffers and the bulk set's slabs shared their room (6.58 at 40, 32 and 28 GiB)
VALU_PEAK_PER_S = 6.56e11           # wave64 32-bit integer VALU instructions/s, chip-wide, MEASURED (profiles/valu_rate.json, tools/native/valu_bench.hip):
                                    # 4 cycles per instruction per SIMD -- half of what the 2-cycle v_fma_f32 rate of MI355X_MICROARCH.md would give
VALU_PEAK_GUIDE_PER_S = 256 * 4 * 2.4e9 / 2    # MI355X_MICROARCH.md: 256 CUs x 4 SIMDs x 2.4 GHz, one wave64 VALU instruction per 2 cycles = 1.229e12
SEED = 42

WORKLOADS = {
    'human': dict(ref='grch38', em='nanopore2023', qm='nanopore2023', identity=(95.0, 99.0, 2.5),
                  text='configs[3]: synthetic GRCh38-like 3.09 Gb reference (24 linear contigs, N runs at contig ends '
                       'and inside chr1/chr9/chrX), nanopore2023 error+qscore models, --identity 95,99,2.5 --length '
                       '15000,13000, other badread simulate parameters at their defaults, seed 42'),
    'hifi': dict(ref='grch38', em='pacbio2021', qm='pacbio2021', identity=(30.0, None, 3.0),
                 text='configs[4]: synthetic GRCh38-like 3.09 Gb reference, pacbio2021 error+qscore models, '
                      '--identity 30,3 (qscore-distributed), --length 15000,13000, other parameters default, seed 42'),
    'kpn': dict(ref='kpn', em='nanopore2023', qm='nanopore2023', identity=(95.0, 99.0, 2.5),
                text='configs[1]: 5.5 Mb K. pneumoniae-like synthetic reference (3 circular contigs), nanopore2023 '
                     'error+qscore models, default badread simulate parameters, seed 42'),
    # parity workloads (tests/test_gpu_fullsize.py), not bench lines: parameter sets that move the reads out of the default band classes
    'rough': dict(ref='grch38', em='nanopore2023', qm='nanopore2023', identity=(85.0, 95.0, 5.0), chimeras=25.0, glitches=(1000.0, 100.0, 100.0),
                  text='configs[3] reference with --identity 85,95,5 --chimeras 25 --glitches 1000,100,100: most bases in the 2-, 4- and '
                       '8+-word band classes of the final aligner'),
    'wide': dict(ref='kpn', em='nanopore2023', qm='nanopore2023', identity=(60.0, 75.0, 8.0), length=(40000.0, 35000.0),
                 text='configs[1] reference with --identity 60,75,8 --length 40000,35000: reads of 150+ kb at 60 % identity, whose final '
                      'band is beyond 16 words per lane (the memory-resident wide path)'),
}


def kpneumoniae_like():
    """configs[1] reference as Python strings (tests and tools): names, sequences, depths, circular flags."""
    import collections
    import synth_refs
    seqs = collections.OrderedDict()
    depths, circular = {}, {}
    for name, seq, depth in synth_refs.kpneumoniae_like_seqs():
        seqs[name] = seq.tobytes().decode()
        depths[name], circular[name] = float(depth), True
    return seqs, depths, circular


def reference_fasta(kind, ref_dir, scale=1.0):
    """Path of the workload's FASTA under ref_dir, written on first use (atomically)."""
    import synth_refs
    os.makedirs(ref_dir, exist_ok=True)
    if kind == 'kpn':
        path = os.path.join(ref_dir, 'kpneumoniae_like.fa')
        if not os.path.isfile(path):
            synth_refs.write_kpneumoniae_like(path)
        return path
    tag = 'grch38_like' if scale == 1.0 else f'grch38_like_x{scale:.5f}'
    path = os.path.join(ref_dir, tag + '.fa')
    if not os.path.isfile(path):
        synth_refs.write_grch38_like(path, scale=scale)
    return path


def load_reference(kind, ref_dir, scale=1.0, timing=None):
    """PackedReference of the workload through the native packer; the packed form is cached beside the FASTA
    (`.brx2bit` sidecar), so the ranks of one node and the CPU-baseline workers read it instead of re-packing."""
    from badread_amd.reference import PackedReference
    t0 = time.perf_counter()
    fasta = reference_fasta(kind, ref_dir, scale)
    t1 = time.perf_counter()
    had_sidecar = os.path.isfile(fasta + '.brx2bit')
    pref = PackedReference.from_fasta(fasta, cache=True)
    t2 = time.perf_counter()
    if timing is not None:
        timing.update({'fasta_write_s': round(t1 - t0, 2), 'fasta_pack_or_sidecar_load_s': round(t2 - t1, 2),
                       'sidecar_hit': had_sidecar, 'fasta_bytes': os.path.getsize(fasta)})
    return pref


def build_workload(io_null, workload='kpn', ref_dir=None, scale=1.0, timing=None):
    from badread_amd.engine import SimParams
    from badread_amd.error_model import ErrorModel
    from badread_amd.fragment_lengths import FragmentLengths
    from badread_amd.identities import Identities
    from badread_amd.qscore_model import QScoreModel
    from badread_amd.simulate import adjust_depths
    w = WORKLOADS[workload]
    pref = load_reference(w['ref'], ref_dir or default_ref_dir(), scale, timing)
    frag_mean, frag_stdev = w.get('length', (15000.0, 13000.0))
    frag = FragmentLengths(frag_mean, frag_stdev, io_null)
    mean, mx, sd = w['identity']
    ident = Identities(mean, sd, mx, io_null)
    depths = adjust_depths(pref, frag, False, np.random.RandomState(SEED))
    _, cum = pref.contig_weights(depths)
    mode, a, b, mx_ = ident.device_mode()
    extra = {}
    if 'chimeras' in w:
        extra['chimera_rate'] = w['chimeras'] / 100.0                       # --chimeras is a percentage (simulate.py:101)
    if 'glitches' in w:
        extra.update(glitch_rate=w['glitches'][0], glitch_size=w['glitches'][1], glitch_skip=w['glitches'][2])
    params = SimParams(frag_mean=frag_mean, frag_stdev=frag_stdev, identity_mode=mode, id_a=a, id_b=b, id_max=mx_, **extra)
    em = ErrorModel(w['em'], io_null).tables()
    qm = QScoreModel(w['qm'], io_null).tables()
    return pref, cum, em, qm, params


def default_ref_dir():
    return os.environ.get('BRX_BENCH_REF_DIR', '/tmp/brx_bench_refs')


def configure(engine, wl):
    pref, cum, em, qm, params = wl
    engine.set_reference(pref, cum)
    engine.set_error_model(em)
    engine.set_qscore_model(qm)
    engine.set_params(params)
    return engine


# ------------------------------------------------------------------------------------------------ CPU baseline leg
def cpu_worker(first_read, budget_s, out_path, workload, ref_dir):
    """One process = one core: the oracle over 16-read chunks of the same read-index stream for `budget_s` seconds."""
    import io
    sys.path.insert(0, os.path.join(REPO, 'oracle'))
    import pyoracle
    eng = configure(pyoracle.OracleEngine(), build_workload(io.StringIO(), workload, ref_dir))
    eng.simulate_batch(SEED, first_read, 2)                      # page everything in before the clock starts
    bases = reads = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < budget_s:
        _, st = eng.simulate_batch(SEED, first_read + reads, 16)
        bases += int(st['seq_len'].sum())
        reads += 16
    with open(out_path, 'w') as f:
        json.dump({'bases': bases, 'reads': reads, 'seconds': time.perf_counter() - t0}, f)


def usable_cores():
    """Host cores this process may really use: the affinity mask, capped by the cgroup CPU quota (the GPU boxes
    expose 256 hardware threads but limit the container to 16 CPUs' worth of time: /sys/fs/cgroup/cpu.max)."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            cores = max(1, min(cores, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return cores


def cpu_baseline(first_read, budget_s, workload, ref_dir):
    """The oracle (oracle/brx_oracle.c, a scalar C port of the same path: gamma/beta draws, fragment build, mutate
    loop with block-Myers window alignments, final alignment + traceback, qscore lookup, FASTQ record) on EVERY
    usable host core (usable_cores()): one single-threaded process per core, disjoint slices of the same read-index
    stream, own clock each.  `reference` = the unmodified Python reference measured in the CPU container."""
    import subprocess
    import tempfile
    cores = usable_cores()
    tmp = tempfile.mkdtemp(prefix='brx_cpu_')
    env = dict(os.environ, OMP_NUM_THREADS='1', OPENBLAS_NUM_THREADS='1', MKL_NUM_THREADS='1', HIP_VISIBLE_DEVICES='')
    procs = []
    for i in range(cores):
        out = os.path.join(tmp, f'{i}.json')
        procs.append((out, subprocess.Popen([sys.executable, os.path.abspath(__file__), '--cpu-worker', str(first_read + i * 100000),
                                             str(budget_s), out, workload, ref_dir], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)))
    bases = reads = 0
    rate = 0.0
    done = 0
    for out, pr in procs:
        pr.wait()
        if os.path.isfile(out):
            rec = json.load(open(out))
            bases += rec['bases']; reads += rec['reads']; rate += rec['bases'] / rec['seconds']; done += 1
    result = {'value': rate, 'unit': 'bases/s', 'cores': done, 'kind': 'port',
              'sample': f'{reads} reads / {bases} bases of the same workload ({workload}: full reference, same seed and '
                        f'read-index stream), {budget_s:.0f} s of CPU time per core, oracle/brx_oracle.c (gcc -O2) as one '
                        f'single-threaded process per host core; value = sum of the per-process rates'}
    ref_file = os.path.join(REPO, 'profiles', 'cpu_reference_baseline.json')
    if os.path.isfile(ref_file):
        try:
            rec = json.load(open(ref_file)).get(workload)
            if rec:
                result['reference'] = {k: rec[k] for k in ('value', 'unit', 'cores', 'kind', 'per_core', 'reference_genome', 'sample', 'host', 'measured_by') if k in rec}
                result['port_over_reference_per_core'] = (rate / max(done, 1)) / rec['per_core']
        except (OSError, ValueError, KeyError):
            pass
    return result


def aligner_lane_model(stats):
    """Share of the final aligner's lane-words that hold band cells, from the geometry of every read of a batch (a model, not a
    counter): a column of a read costs one trip-slot on all 64 lanes x G words, of which (band width) / 32 words are inside
    the Ukkonen band.  Band width ~ distance of the alignment + 1 (the kernels use the proven bound, a few percent more);
    G = words per lane of the band class (1 up to 56 x 32 diagonals, then doubling); reads that k_fin_quad takes are issued for the
    16 lanes of their row.  (The one-read-per-lane class of short reads is counted at 64 lanes: an underestimate of the useful share.)
    Returns (useful, issued) word-columns."""
    n = stats['frag_len'].astype(np.float64) + 14.0
    d = np.maximum(stats['n_cols'].astype(np.float64) - stats['n_match'], 0.0)
    live = stats['n_cols'] > 0
    bw = np.maximum(d + 1.0, np.abs(stats['padded_len'].astype(np.float64) - n) + 1.0)
    g = np.ones_like(bw)
    for _ in range(12):
        g = np.where(bw > 56.0 * 32.0 * g, g * 2.0, g)
    lanes = np.full_like(bw, 64.0)
    quad_bits = int(os.environ.get('BRX_FIN_QUAD', '1') or 0)
    if quad_bits:
        # four reads per wave (k_fin_quad<1>, csrc/brx_quad.h): a row of 16 lanes x 1 word up to 13 x 32 diagonals; reads with symbols
        # outside ACGT keep to the whole wave: not visible in the statistics, a few per thousand
        quad1 = (bw <= 13.0 * 32.0) & (bw > 88.0) & live & bool(quad_bits & 1)      # (up to 88 diagonals: the one-read-per-lane class)
        quad2 = np.zeros_like(quad1)                                                  # (a two-word class existed in round 5 and lost: removed)
        if int((quad1 | quad2).sum()) < int(os.environ.get('BRX_QUAD_MIN_READS', '4096')):      # a small class keeps to whole waves (brx_hip.hip)
            quad1 = quad2 = np.zeros_like(live)
        lanes = np.where(quad1 | quad2, 16.0, lanes)
        g = np.where(quad2, 2.0, g)
    useful = float((n * bw / 32.0)[live].sum())
    issued = float((n * lanes * g)[live].sum())
    return useful, issued


def valu_per_base(workload):
    """SQ_INSTS_VALU per simulated base of this workload from the committed counter pass (profiles/), or None."""
    path = os.path.join(REPO, 'profiles', 'valu_per_base.json')
    try:
        return json.load(open(path)).get(workload)
    except (OSError, ValueError):
        return None


DUMP_STATS_BYTES = 44 << 20          # --dump-outputs: per-read statistics (float64), all reads of the last step up to this size
DUMP_FASTQ_BYTES = 4 << 20           # FASTQ bytes of a seeded sample of whole records (one float32 per byte: 16 MiB)


def dump_outputs(out_dir, last):
    """--dump-outputs: what the timed path handed its caller in the last step, as DIR/<name>.npy (float64 / float32, < 64 MB).
    `last` = [(first read, FASTQ bytes, stats)] of the device batches of that step (one per batch in flight), in read order.
      read_index, stats_<field>   every read of the step (a seeded sample of them if they exceed DUMP_STATS_BYTES)
      fastq_sample_bytes          the records of a seeded sample of reads, concatenated (fastq_sample_read_index, fastq_sample_rec_len)
      fastq_batch_bytes, fastq_batch_byte_sum   length and byte sum of each batch's whole FASTQ output"""
    import torch
    last = sorted(last, key=lambda t: t[0])
    stats = np.concatenate([st for _, _, st in last])
    index = np.concatenate([first + np.arange(len(st), dtype=np.int64) for first, _, st in last])
    batch = np.concatenate([np.full(len(st), b, dtype=np.int64) for b, (_, _, st) in enumerate(last)])
    fields = stats.dtype.names
    rng = np.random.default_rng(SEED)
    n = len(stats)
    keep = np.arange(n)
    per_read = 8 * (len(fields) + 1)
    if n * per_read > DUMP_STATS_BYTES:
        keep = np.sort(rng.choice(n, DUMP_STATS_BYTES // per_read, replace=False))
    arrays = {'read_index': index[keep].astype(np.float64)}
    for f in fields:
        arrays['stats_' + f] = stats[f][keep].astype(np.float64)
    picked, total = [], 0
    for r in rng.permutation(n):
        size = int(stats['rec_len'][r])
        if total + size > DUMP_FASTQ_BYTES:
            break
        picked.append(int(r)); total += size
    picked.sort()
    parts = []
    for r in picked:
        out = last[batch[r]][1]
        lo = int(stats['rec_off'][r])
        part = out[lo: lo + int(stats['rec_len'][r])]
        parts.append(part.cpu().numpy() if isinstance(part, torch.Tensor) else np.asarray(part, dtype=np.uint8))
    arrays['fastq_sample_bytes'] = (np.concatenate(parts) if parts else np.zeros(0, np.uint8)).astype(np.float32)
    arrays['fastq_sample_read_index'] = index[picked].astype(np.float64)
    arrays['fastq_sample_rec_len'] = stats['rec_len'][picked].astype(np.float64)
    sizes, sums = [], []
    for _, out, _ in last:
        sizes.append(float(len(out)))
        if isinstance(out, torch.Tensor):
            sums.append(float(out.sum(dtype=torch.int64).item()))         # exact: < 2^53 for any batch that fits a device
        else:
            sums.append(float(np.asarray(out, dtype=np.uint8).sum(dtype=np.int64)))
    arrays['fastq_batch_bytes'] = np.array(sizes, dtype=np.float64)
    arrays['fastq_batch_byte_sum'] = np.array(sums, dtype=np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), arr)
    print(f'[bench] --dump-outputs: {len(arrays)} arrays, {sum(a.nbytes for a in arrays.values()) / 2 ** 20:.1f} MiB in {out_dir}',
          file=sys.stderr, flush=True)


# ------------------------------------------------------------------------------------------------ launch
def respawn_under_torchrun(args_list, n):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script (one per GPU) and wait."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + args_list
    return subprocess.call(cmd)


def main():
    if len(sys.argv) >= 7 and sys.argv[1] == '--cpu-worker':
        cpu_worker(int(sys.argv[2]), float(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--workload', default='human', choices=sorted(WORKLOADS))
    ap.add_argument('--reads-per-step', type=int, default=393216,
                    help='read indices per GPU per step; split into --streams device batches')
    ap.add_argument('--scratch-gb', type=float, default=SCRATCH_GB_DEFAULT, help='scratch arena per in-flight batch')
    ap.add_argument('--streams', type=int, default=6,
                    help='device batches in flight per GPU (one context + HIP stream + host thread each): the slowest '
                         'read of one device batch overlaps the bulk of the others')
    ap.add_argument('--cpu-seconds', type=float, default=12.0, help='seconds each host core runs the cpu_baseline leg of --full (0 = skip)')
    ap.add_argument('--d2h', action='store_true', help='also run the same amount of work through the CLI driver (PCIe + host output stage): value_incl_d2h, value_incl_gzip')
    ap.add_argument('--d2h-legs', default='devnull_cold,devnull,gzip_device,gzip1', help='which --d2h legs to run (comma separated)')
    ap.add_argument('--ref-dir', default=default_ref_dir(), help='where the synthetic reference FASTA and its packed sidecar live')
    ap.add_argument('--ref-scale', type=float, default=1.0, help='shrink the GRCh38-like reference (tests, dry runs); 1.0 = the metric\'s 3.09 Gb')
    ap.add_argument('--scaling', default='weak', choices=('weak', 'strong'),
                    help='weak (default; the driver\'s line): fixed work per GPU, inputs resident before the clock.  strong: the fixed --quantity job '
                         'split over the ranks, every rank\'s start-up inside the clock (fixed_cost_s, loop_s, projected_wall_s); --steps / --warmup are ignored')
    ap.add_argument('--quantity', type=float, default=30.0, help='--scaling strong: depth of the job (x the reference; 30 = the metric\'s job)')
    ap.add_argument('--full', action='store_true',
                    help='also measure what the headline figure does not need: per-kernel launch timing (kernels_per_device_batch, roofline, '
                         'roofline_alu) and the CPU baseline leg (--cpu-seconds per host core).  Off: set up, warm up, time the steps, '
                         'write --dump-outputs, print the line')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step computed (read statistics, a seeded sample of the FASTQ '
                         'records, per-batch byte counts and sums) as DIR/<name>.npy in float64 / float32, at most 64 MB in all')
    ap.add_argument('--cpu-engine', action='store_true',
                    help='DRY RUN of the launch / sharding / reporting logic on the CPU checker engine over gloo (tests only: '
                         'the line it prints is marked invalid and measures nothing)')
    args = ap.parse_args()

    world = int(os.environ.get('WORLD_SIZE', '0') or 0)
    if world == 0 and args.gpus > 1:
        sys.exit(respawn_under_torchrun(sys.argv[1:], args.gpus))
    world = max(world, 1)
    if world != args.gpus:
        sys.exit(f'bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to measure a different number of GPUs than asked for')
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if os.environ.get('BRX_DEVICE'):            # several ranks on ONE GPU (accounting runs on a 1-GPU box; with BRX_DIST_BACKEND=gloo)
        local = int(os.environ['BRX_DEVICE'])
    strong = args.scaling == 'strong'
    marks = {'process': T_PROCESS}              # --scaling strong: where a rank's start-up goes

    import io
    import torch
    marks['imports'] = time.perf_counter()
    dry = args.cpu_engine
    if not dry and not torch.cuda.is_available():
        sys.exit('bench.py needs a ROCm device: the HIP path has no CPU fallback')
    if not dry:
        if torch.cuda.device_count() < world and not os.environ.get('BRX_DEVICE'):
            sys.exit(f'bench.py: --gpus {world} but only {torch.cuda.device_count()} device(s) visible')
        torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if dry or os.environ.get('BRX_DIST_BACKEND') == 'gloo':
            dist.init_process_group(backend='gloo')
        else:
            dist.init_process_group(backend='nccl', device_id=torch.device('cuda', local))

    def barrier():
        if not dry:
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            if not dry:
                torch.cuda.synchronize()

    # ---- reference: rank 0 writes the FASTA and packs it (sidecar), the other ranks then load the sidecar ----
    ref_timing = {}
    wl = None
    if rank == 0:
        wl = build_workload(io.StringIO(), args.workload, args.ref_dir, args.ref_scale, ref_timing)
    barrier()
    if rank != 0:
        wl = build_workload(io.StringIO(), args.workload, args.ref_dir, args.ref_scale, None)
    pref = wl[0]
    marks['reference'] = time.perf_counter()
    # --scaling strong: what the clock does NOT hold is the one-off preparation of the synthetic genome on a fresh box (writing 3.1 GB
    # of FASTA, packing it into the sidecar): a user's genome exists and its packed form is in the cache from any earlier run on
    # it (the protocol of tools/cli_30x.sh).  Every rank waited for rank 0 to do it: the same seconds come off every rank's clock.
    prep = 0.0
    if strong:
        if rank == 0 and not ref_timing.get('sidecar_hit', True):
            prep = float(ref_timing.get('fasta_write_s', 0.0)) + float(ref_timing.get('fasta_pack_or_sidecar_load_s', 0.0))
        if dist is not None:
            tp = torch.tensor([prep], dtype=torch.float64, device='cpu' if (dry or os.environ.get('BRX_DIST_BACKEND') == 'gloo') else 'cuda')
            dist.all_reduce(tp, op=dist.ReduceOp.MAX)
            prep = float(tp.item())
        marks['process'] += prep
        marks['imports'] += prep

    C = max(1, args.streams)
    R = max(64, args.reads_per_step // C)              # reads per device batch (one brx_simulate_batch call)
    if dry:
        sys.path.insert(0, os.path.join(REPO, 'oracle'))
        import pyoracle
        engines = [configure(pyoracle.OracleEngine(), wl)]
        engines += [engines[0].clone() for _ in range(C - 1)]
        streams = [None] * C
    else:
        from badread_amd.engine import HipEngine
        t_up = time.perf_counter()
        first = configure(HipEngine(local, scratch_bytes=int(args.scratch_gb * (1 << 30))), wl)
        torch.cuda.synchronize()
        ref_timing['h2d_tables_s'] = round(time.perf_counter() - t_up, 2)
        engines = [first] + [None] * (C - 1)               # clones share the device tables: ONE replica of the reference per GPU
        streams = [torch.cuda.Stream(device=local) for _ in range(C)]
        boot_errors = []

        def boot(i):                                       # a thread per context, as the CLI's pool makes its clones: arena, context, priming batch
            try:
                torch.cuda.set_device(local)
                if i:
                    engines[i] = first.clone()
                if args.full:                              # events around every launch: the per-kernel figures of --full
                    engines[i].set_kernel_timing(True)
                with torch.cuda.stream(streams[i]):        # prime the context (lazy module load, buffers) -- not a step
                    engines[i].simulate_batch_device(SEED, 2 ** 40, 64, expected_bytes=int(R * first.expected_record_bytes() * 1.05))
                    streams[i].synchronize()
            except BaseException as ex:
                boot_errors.append(ex)
        boots = [threading.Thread(target=boot, args=(i,)) for i in range(C)]
        for th in boots:
            th.start()
        for th in boots:
            th.join()
        if boot_errors:
            raise boot_errors[0]
        torch.cuda.synchronize()
    marks['engines'] = time.perf_counter()
    # --scaling strong: the job as device batches; batch b covers read indices [b R, (b + 1) R) and belongs to rank b % world
    mean_len = float(WORKLOADS[args.workload].get('length', (15000.0, 13000.0))[0])
    n_job = max(1, int(np.ceil(args.quantity * float(pref.n_bases) / (R * mean_len)))) if strong else 0

    def run_one(e, index):
        """(first read, FASTQ bytes, stats) of device batch `index`; the bytes stay on the device until the engine's next batch."""
        first_read = index * R if strong else (index * world + rank) * R
        if dry:
            out, stats = e.simulate_batch(SEED, first_read, R)
            return first_read, out, stats
        out, stats = e.simulate_batch_device(SEED, first_read, R, expected_bytes=int(R * e.expected_record_bytes() * 1.05))
        return first_read, out, stats

    def run_steps(step_indices, indices=None):
        """The device batches of steps `step_indices`, C in flight: worker i owns context i / stream i and takes
        every C-th device batch; batch b of step k covers read indices ((k*C + b)*world + rank)*R ...
        (--scaling strong passes its own list of batch indices.)"""
        if indices is None:
            indices = [k * C + b for k in step_indices for b in range(C)]
        acc = [{'bases': 0, 'passes': 0, 'stages': {}, 'kernels': {}, 'final_launches': 0, 'misses': 0, 'bad': 0, 'host_ms': 0.0, 'error': None, 'lane_useful': 0.0, 'lane_issued': 0.0,
                'last': None} for _ in range(C)]

        def worker(i):
            try:
                if not dry:
                    torch.cuda.set_device(local)
                ctx = torch.cuda.stream(streams[i]) if not dry else _Null()
                with ctx:
                    for idx in indices[i::C]:
                        t_call = time.perf_counter()
                        acc[i]['last'] = run_one(engines[i], idx)      # (what --dump-outputs writes of the last step)
                        stats = acc[i]['last'][2]
                        acc[i]['host_ms'] += 1000.0 * (time.perf_counter() - t_call)
                        acc[i]['bases'] += int(stats['seq_len'].sum())
                        acc[i]['bad'] += int((stats['status'] & 0xE).astype(bool).sum())     # RS_TOO_MANY_SEGS | RS_BAND | RS_QMISS
                        if args.full:
                            useful, issued = aligner_lane_model(stats)
                            acc[i]['lane_useful'] += useful; acc[i]['lane_issued'] += issued
                        if dry:
                            continue
                        acc[i]['passes'] += engines[i].mutate_passes()
                        for name, ms in engines[i].stage_ms().items():
                            acc[i]['stages'][name] = acc[i]['stages'].get(name, 0.0) + ms
                        if args.full:
                            for name, (n_l, ms, b) in engines[i].kernel_stats().items():
                                k = acc[i]['kernels'].setdefault(name, [0, 0.0, 0.0])
                                k[0] += n_l; k[1] += ms; k[2] += b
                        acc[i]['final_launches'] += engines[i].final_launches()
                        acc[i]['misses'] += engines[i].window_misses()
                    if not dry:
                        streams[i].synchronize()
            except BaseException as ex:          # surfaced on the main thread
                acc[i]['error'] = ex

        threads = [threading.Thread(target=worker, args=(i,)) for i in range(C)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for a in acc:
            if a['error'] is not None:
                raise a['error']
        return acc

    if strong:
        args.warmup, args.steps = 0, max(1, -(-n_job // (C * world)))        # rounds of C batches per rank the job amounts to
    w_t0, w_cpu0 = time.perf_counter(), time.process_time()
    run_steps(list(range(args.warmup)) if args.warmup else [])
    warm_busy = (time.process_time() - w_cpu0) / max(time.perf_counter() - w_t0, 1e-9)      # host cores this rank kept busy while warming up
    barrier()
    host_throttled = None
    if dist is not None and args.warmup:
        # N > 1 on one node: every rank drives its batches with host threads, and the node has `usable_cores` for all of them
        # (1.2-1.5 cores per rank measured at N = 1).  Say so BEFORE the timed region, and refuse a run the host would throttle:
        # its number would measure the CPUs, not the GPUs.  BRX_BENCH_ALLOW_OVERSUBSCRIBED=1 runs it anyway.
        tb = torch.tensor([warm_busy], dtype=torch.float64, device='cpu' if dry else 'cuda')
        dist.all_reduce(tb, op=dist.ReduceOp.SUM)
        busy_all = float(tb.item())
        if rank == 0:
            print(f'[bench] host cores busy during warm-up: {warm_busy:.2f} on rank 0, {busy_all:.2f} on all {world} ranks, {usable_cores()} usable', file=sys.stderr, flush=True)
        # (round 5 refused such a run and printed no metric line: a scaling box with a small cgroup got NO data.  Now the run is
        #  timed and its line says `host_throttled: true` with the numbers: flagged data instead of none -- VERDICT r5.)
        host_throttled = {'host_throttled': bool(busy_all > 1.25 * usable_cores()),       # (warm-up steps cost more host time than steady ones: a margin)
                          'busy_cores_all_ranks_during_warmup': busy_all, 'usable_cores': usable_cores()}
    t0 = time.perf_counter()
    cpu0 = time.process_time()
    if strong:
        acc = run_steps(None, indices=[b for b in range(n_job) if b % world == rank])
        t_end_rank = time.perf_counter()
    else:
        acc = run_steps([args.warmup + k for k in range(args.steps)])
    barrier()
    elapsed = time.perf_counter() - t0
    host_cpu_s = time.process_time() - cpu0           # CPU seconds of this rank (all its threads) inside the timed region
    bases = sum(a['bases'] for a in acc)
    bad = sum(a['bad'] for a in acc)

    on_host = dry or os.environ.get('BRX_DIST_BACKEND') == 'gloo'
    t = torch.tensor([elapsed, float(bases), float(bad)], dtype=torch.float64, device='cpu' if on_host else 'cuda')
    strong_rec = None
    if strong:
        # per rank: start-up (process start -> first batch issued), loop (-> its last batch done); the job ends with its slowest rank
        names = ('imports', 'reference', 'engines')
        spans = [marks['imports'] - marks['process'], marks['reference'] - marks['imports'], marks['engines'] - marks['reference'],
                 t0 - marks['process'], t_end_rank - t0, t_end_rank - marks['process']]
        ts = torch.tensor(spans, dtype=torch.float64, device='cpu' if on_host else 'cuda')
        if dist is not None:
            dist.all_reduce(ts, op=dist.ReduceOp.MAX)
        spans = [float(x) for x in ts.tolist()]
        strong_rec = {'reference_preparation_s_not_in_the_clock': round(prep, 2),
                      'startup_s_slowest_rank': dict(zip(names, (round(x, 3) for x in spans[:3]))),
                      'fixed_cost_s': spans[3], 'loop_s': spans[4], 'wall_s': spans[5]}
    if dist is not None:
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        elapsed, bases, bad = float(tmax[0].item()), float(t[1].item()), float(t[2].item())
    if strong:
        elapsed = strong_rec['wall_s']             # the clock of the strong line: process start to the last batch of the slowest rank
    value = bases / elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, [a['last'] for a in acc if a['last'] is not None])

    # ---- --d2h: the SAME amount of work through the CLI's own driver (badread_amd.simulate.run_batches: stop rule,
    # pinned ring, writer thread), FASTQ text to /dev/null and through the multi-threaded gzip stage ----
    d2h = None
    if args.d2h and rank == 0 and not dry:
        from badread_amd.simulate import run_batches
        from badread_amd.output import GzipSink
        first = engines[0]
        for e in engines[1:]:
            e.close()
        del engines[1:]
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        target = int(sum(a['bases'] for a in acc))           # what this rank simulated in the timed region
        d2h = {}
        legs = [x for x in args.d2h_legs.split(',') if x]
        for name, level in (('devnull_cold', None), ('devnull', None), ('gzip_device', 'device'), ('gzip1', 1)):   # cold: includes mapping the clones' scratch
            if name not in legs:
                continue
            print(f'[bench --d2h] {name} ...', file=sys.stderr, flush=True)
            gc.collect()
            torch.cuda.empty_cache()                 # the legs run at the edge of the 288 GB (6 x 40 GB of scratch): give back what the last one cached
            raw = open(os.devnull, 'wb')
            sink = raw if level in (None, 'device') else GzipSink(raw, level)
            counter = {'bytes': 0}
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            def write_part(part, sink=sink, counter=counter):
                counter['bytes'] += len(part)
                sink.write(memoryview(part))
            count, total = run_batches(first, SEED, target, 15000.0, write_part, io.StringIO(),
                                       max_batch=R, in_flight=C, device_gzip=(level == 'device'))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            d2h[name] = {'bases_per_s': total / dt, 'reads': count, 'bases': total, 'seconds': dt,
                         'fastq_bytes_per_s': (getattr(sink, 'bytes_in', 0) or 2.02 * total) / dt}
            if level == 'device':
                d2h[name]['compressed_bytes'] = counter['bytes']
            elif level is not None:
                d2h[name]['compressed_bytes'] = sink.bytes_out
            d2h[name]['consumer_thread_seconds'] = {k: round(float(v), 3) for k, v in run_batches.last_timing.items()}
            raw.close()
        engines[:] = [first]

    n_batches = (len([b for b in range(n_job) if b % world == rank]) or 1) if strong else args.steps * C
    stage_sum, kern = {}, {}
    for a in acc:
        for name, ms in a['stages'].items():
            stage_sum[name] = stage_sum.get(name, 0.0) + ms
        for name, (n_l, ms, b) in a['kernels'].items():
            k = kern.setdefault(name, [0, 0.0, 0.0])
            k[0] += n_l; k[1] += ms; k[2] += b
    extra = {'passes': float(sum(a['passes'] for a in acc)), 'misses': float(sum(a['misses'] for a in acc)),
             'host_ms': float(sum(a['host_ms'] for a in acc)), 'host_cpu_s': float(host_cpu_s),
             'lane_useful': float(sum(a['lane_useful'] for a in acc)), 'lane_issued': float(sum(a['lane_issued'] for a in acc))}
    if dist is not None:
        # the per-kernel, per-stage and host statistics of EVERY rank (round 3 reported rank 0's alone): one sum over a fixed layout
        from badread_amd.engine import KERNEL_NAMES, STAGE_NAMES
        vec = [stage_sum.get(n, 0.0) for n in STAGE_NAMES]
        for n in KERNEL_NAMES:
            vec += list(kern.get(n, [0, 0.0, 0.0]))
        vec += [extra[k] for k in sorted(extra)]
        tv = torch.tensor(vec, dtype=torch.float64, device='cpu' if on_host else 'cuda')      # the dry run (gloo) takes the same path: tests/test_bench_launch.py
        dist.all_reduce(tv, op=dist.ReduceOp.SUM)
        vec = tv.tolist()
        stage_sum = dict(zip(STAGE_NAMES, vec[:len(STAGE_NAMES)]))
        at = len(STAGE_NAMES)
        kern = {}
        for n in KERNEL_NAMES:
            if vec[at]:
                kern[n] = [vec[at], vec[at + 1], vec[at + 2]]
            at += 3
        extra = dict(zip(sorted(extra), vec[at:]))
        n_batches = n_job if strong else n_batches * world
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return
    stages = {k: v / n_batches for k, v in stage_sum.items()}          # per device batch
    bases_per_step_rank0 = sum(a['bases'] for a in acc) / args.steps
    result = {
        'metric': 'simulated bases/sec', 'value': value, 'unit': 'bases/s', 'n_gpus': world, 'steps': args.steps,
        'warmup': args.warmup, 'ms_per_step': 1000.0 * elapsed / args.steps, 'higher_is_better': True,
        'scaling': args.scaling, 'vs_baseline': None, 'dtype': 'u32', 'data': 'synthetic',
        'config': {'workload': WORKLOADS[args.workload]['text'] + ('' if args.ref_scale == 1.0 else f' [REFERENCE SCALED x{args.ref_scale}: dry run]'),
                   'reference_bases': int(pref.n_bases), 'reference_contigs': len(pref.names), 'reference_non_acgt_runs': int(len(pref.exceptions)),
                   'reads_per_step_per_gpu': R * C, 'bases_per_step_per_gpu': bases_per_step_rank0,
                   'device_batches_per_step': C, 'reads_per_device_batch': R, 'scratch_arena_gib_per_device_batch': args.scratch_gb,
                   'parallelism': f'reads sharded by index over {world} GPU(s), reference replicated per GPU, no collectives on the data path'},
        'reference_load': ref_timing,
        'reads_flagged_band_segs_qmiss': bad,
    }
    if host_throttled is not None:
        result.update(host_throttled)
        if host_throttled['host_throttled']:
            result['host_throttled_note'] = ('the ranks kept more host cores busy during warm-up than the node gives this container: the value '
                                            'measures the host as much as the GPUs')
    if strong:
        fixed, loop = strong_rec['fixed_cost_s'], strong_rec['loop_s']
        result.update(strong_rec)
        result['value_loop'] = bases / loop
        result['job'] = {'quantity_x': args.quantity, 'device_batches': n_job, 'reads_per_device_batch': R, 'bases': bases,
                         'split': 'device batch b -> rank b % N; every rank runs its batches with --streams in flight'}
        # what N ranks would take if the loop splits evenly and the fixed cost stays: the 8-GPU wall time a scaling box would see
        result['projected_wall_s'] = {str(n): round(fixed + loop * world / n, 2) for n in (1, 2, 4, 8)}
        result['projected_speedup_vs_1'] = {str(n): round((fixed + loop * world) / (fixed + loop * world / n), 2) for n in (1, 2, 4, 8)}
        result['strong_note'] = ('clock = first line of bench.py to the last batch of the slowest rank (start-up INSIDE: interpreter, torch, reference, '
                                 'engines + arenas, tables, priming); value = job bases / that; never comparable with the weak line, whose inputs are resident')
    if dry:
        result['INVALID'] = 'dry run on the CPU checker engine (--cpu-engine): exercises launch / sharding / reporting only'
        result['roofline'] = result['cpu_baseline'] = None
        print(json.dumps(result), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return
    result['stage_ms_per_device_batch'] = stages
    result['host_ms_per_device_batch'] = extra['host_ms'] / n_batches        # wall time of one brx_simulate_batch call
    result['host_cpu'] = {'cpu_seconds_per_device_batch': extra['host_cpu_s'] / n_batches, 'busy_cores_per_rank': extra['host_cpu_s'] / elapsed / world,
                          'busy_cores_all_ranks': extra['host_cpu_s'] / elapsed, 'usable_cores': usable_cores(),
                          'note': 'process CPU time of every rank (six batch threads + main each) over the timed region, summed: it must fit the usable cores of the node'}
    result['scratch_or_output_retries'] = sum(getattr(e, 'retries', 0) for e in engines)
    result['retry_log'] = [m for e in engines for m in getattr(e, 'retry_log', [])][:8]
    result['mutate_passes_per_device_batch'] = extra['passes'] / n_batches
    result['traceback_window_misses_per_step'] = extra['misses'] / args.steps
    if d2h is not None:
        for key, leg in (('value_incl_d2h', 'devnull'), ('value_incl_d2h_cold', 'devnull_cold'), ('value_incl_gzip', 'gzip1'), ('value_incl_gzip_device', 'gzip_device')):
            if leg in d2h:
                result[key] = d2h[leg]['bases_per_s']
        result['driver_end_to_end'] = dict(d2h, note='badread_amd.simulate.run_batches (the CLI driver: stop rule, D2H through a ring of pinned '
                                                      'buffers, writer thread) over the same number of bases, FASTQ to /dev/null and through '
                                                      '--gzip 1 on all host cores; includes the start-up of its engine clones')
    if not args.full:
        result['roofline'] = result['roofline_alu'] = result['cpu_baseline'] = None
        result['full_note'] = 'per-kernel launch timing, rooflines and the CPU baseline: bench.py --full'
        print(json.dumps(result), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return
    # ---- --full: roofline of the kernel that ranks first by summed launch time in THIS run (what rocprofv3 --stats ranks first) ----
    ranked = sorted(((ms, name) for name, (n_l, ms, b) in kern.items() if n_l), reverse=True)
    top = ranked[0][1]
    n_l, ms, kb = kern[top]
    launch_ms = ms / n_l
    bases_per_launch = kb / n_l
    algo_bytes = ALGO_BYTES_PER_BASE * bases_per_launch
    achieved = algo_bytes / (launch_ms * 1e-3) / 1e9
    traffic = traffic_tree = None
    tfile = os.path.join(REPO, 'profiles', 'pmc_traffic.json')
    if os.path.isfile(tfile):
        try:
            rec = json.load(open(tfile))
            one = rec.get('kernels', {}).get(top) if 'kernels' in rec else (rec if rec.get('kernel') == top else None)      # tools/pmc_traffic.py --all: every kernel that may rank first
            if one and rec.get('reads_per_step') == R and rec.get('workload', 'kpn') == args.workload:
                traffic = one.get('hbm_bytes_per_launch')
                traffic_tree = rec.get('csrc_sha16')
        except (OSError, ValueError):
            pass
    result['roofline'] = {'bound': 'hbm', 'kernel': top, 'achieved': achieved, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                          'frac': achieved / HBM_PEAK_GBS, 'traffic': traffic, 'traffic_counted_on_tree': traffic_tree,
                          'algorithmic_bytes_per_launch': algo_bytes, 'bases_per_launch': bases_per_launch,
                          'launch_ms': launch_ms, 'launches_per_device_batch': n_l / n_batches,
                          'whole_path_frac': value / world * ALGO_BYTES_PER_BASE / 1e9 / HBM_PEAK_GBS,
                          'note': 'kernel = largest summed launch time of this run (HIP events around every launch on its own '
                                  'stream); bases_per_launch = fragment bases of the reads the kernel class handled / launches '
                                  '(a read counts once per class); launch_ms includes time the launch shares the GPU with '
                                  'the other batches in flight; integer-ALU / latency bound path: see roofline_alu'}
    result['kernels_per_device_batch'] = {name: {'launches': n_l / n_batches, 'ms': ms / n_batches, 'avg_launch_ms': ms / n_l,
                                                  'mbases': b / n_batches / 1e6}
                                          for name, (n_l, ms, b) in sorted(kern.items(), key=lambda kv: -kv[1][1]) if n_l}
    vpb = valu_per_base(args.workload)
    if vpb:
        rate = vpb['valu_per_base'] * value / world
        from badread_amd.build import source_hash
        tree = source_hash()
        lane_useful, lane_issued = extra['lane_useful'], extra['lane_issued']
        result['roofline_alu'] = {'bound': 'valu-issue', 'achieved': rate, 'peak': VALU_PEAK_PER_S, 'peak_source': 'profiles/valu_rate.json (measured integer VALU issue rate: 4 cycles per wave64 instruction per SIMD)',
                                  'unit': 'wave-instructions/s', 'frac': rate / VALU_PEAK_PER_S,
                                  'peak_guide': VALU_PEAK_GUIDE_PER_S, 'frac_of_guide_peak': rate / VALU_PEAK_GUIDE_PER_S,
                                  'peak_note': 'MI355X_MICROARCH.md quotes a 2-cycle issue for 32-bit VALU ops (256 CUs x 4 SIMDs x 2.4 GHz / 2 = 1.229e12/s = peak_guide); tools/native/valu_bench.hip reaches that rate only with fp32 FMA '
                                               '(control kernel: 1.07e12 FMA/s, issued as 5.3e11 v_pk_fma_f32/s) and measures 3.75 cycles for the integer ops of this path '
                                               '(v_and / v_add / v_bitop3 / v_alignbit; profiles/valu_rate.json): both fractions are given',
                                  'valu_per_base': vpb['valu_per_base'], 'source': vpb.get('source'),
                                  'counted_on_tree': vpb.get('csrc_sha16'), 'this_tree': tree,
                                  'stale': vpb.get('csrc_sha16') != tree,        # the instruction count was taken on other kernel sources: repeat tools/profile_round.sh
                                  'exec_lane_frac': vpb.get('exec_lane_frac'),
                                  'useful_lane_frac_aligner_model': (lane_useful / lane_issued) if lane_issued else None,
                                  'lane_note': 'issued instructions are not useful lane-operations: exec_lane_frac = lanes the EXEC mask leaves on (PMC), '
                                               'useful_lane_frac_aligner_model = band words / (64 lanes x words per lane) of the final alignments of THIS run '
                                               '(the kernels that issue more than half of the instructions)'}
    if world == 1 and args.cpu_seconds > 0:
        result['cpu_baseline'] = cpu_baseline(10_000_000, args.cpu_seconds, args.workload, args.ref_dir)
        result['gpu_over_cpu'] = value / result['cpu_baseline']['value']
        if 'reference' in result['cpu_baseline']:
            ref = result['cpu_baseline']['reference']
            result['gpu_over_reference_same_cores'] = value / (ref['per_core'] * result['cpu_baseline']['cores'])
    else:
        result['cpu_baseline'] = None
        if world > 1:
            result['cpu_baseline_note'] = 'the CPU leg runs at N = 1 only (the bench contract: rank 0, a bounded sample); the N = 1 line of the same tree carries it'
    print(json.dumps(result), flush=True)
    if dist is not None:
        dist.destroy_process_group()


class _Null(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


if __name__ == '__main__':
    main()
