"""
Host side of `badread simulate` for the MI355X path.

The reference runs one read at a time in a Python loop (/root/reference/badread/simulate.py:63-86).
Here the loop body -- build_fragment (:91-115), Identities.get_identity, sequence_fragment
(:256-358) with get_qscores, and the FASTQ record (:73-82) -- is one C-ABI call per batch of
read indices (brx_simulate_batch, include/brx.h); this module keeps what stays on the host:

  * start-up in the reference's order: load reference, FragmentLengths, adjust_depths (:516-536),
    Identities, models, adapters (:412-430), target size (:124-145), the same banner text;
  * the stop rule: reads are keyed by index, the host prefix-sums the read lengths of each batch
    in index order and cuts after the first read that reaches the target (:63,84), so the output
    is independent of batch size and of the number of GPUs;
  * sharding: rank r of N takes the r-th slice of every super-batch (no collective on the data
    path; the per-read lengths and, for an ordered stdout, the record bytes are gathered);
  * `sequence_fragment(fragment, target_identity, error_model, qscore_model)`: the narrow Python
    boundary the reference's tests use (test/test_simulate.py:47,83), as a batch of one.

Randomness: every draw on the device is Philox4x32-10 keyed by (seed, read index, stream)
(include/brx_spec.h), so a seed fixes the output bytes, but not to the reference's MT19937 stream.
"""
import collections
import concurrent.futures
import contextlib
import gzip
import math
import os
import queue
import random
import sys
import threading
import time

import numpy as np

from . import settings
# BAM_SHARE, PAF_SHARE and SAM_SHARE are not used here: tests and tools read them as simulate.PAF_SHARE and the like
from .engine import BAM_SHARE, PAF_SHARE, SAM_SHARE, TRUTH_KINDS, TRUTH_SHARE, fmt_share, tag_share, RS_BAND, RS_NOFRAG, RS_QMISS, RS_TOO_MANY_SEGS, SimParams
from .error_model import ErrorModel
from .fragment_lengths import FragmentLengths
from .identities import Identities
from .misc import float_to_str, get_random_sequence, str_is_int
from .qscore_model import QScoreModel
from .reference import PackedReference
from .version import __version__

NOFRAG_MESSAGE = ('Error: failed to generate any sequence fragments - are your read lengths '
                  'incompatible with your reference contig lengths?')
ADJUST_SAMPLES = 100000
DEFAULT_MAX_BATCH = 65536
DEFAULT_IN_FLIGHT = 6          # super-batches in flight per GPU (--gpu-streams): what bench.py measures


# ---------------------------------------------------------------------------------------------
# start-up pieces (host only)
# ---------------------------------------------------------------------------------------------
def print_intro(output):
    print(f'\nBadread v{__version__}\nlong read simulation', file=output)


def load_reference(reference, output):
    """The reference's function (simulate.py:494-507), same return value: (seqs, depths, circular, hairpin_left,
    hairpin_right) as Python dicts, after printing the summary.  The driver itself uses load_packed_reference."""
    from .misc import load_fasta
    print(f'\nLoading reference from {reference}', file=output)
    seqs, depths, circular, hp_left, hp_right = load_fasta(reference)
    print(f'  {len(seqs):,} contig{"" if len(seqs) == 1 else "s"}:', file=output)
    for name, seq in seqs.items():
        print(f'    {name}: {len(seq):,} bp, {"circular" if circular[name] else "linear"}, {depths[name]:.2f}x depth', file=output)
    if len(seqs) > 1:
        print(f'  total size: {sum(len(v) for v in seqs.values()):,} bp', file=output)
    return seqs, depths, circular, hp_left, hp_right


def load_packed_reference(reference, output):
    """FASTA(.gz) -> PackedReference through the native packer (libbrx_host.so, csrc/brx_fasta.cpp), with the
    reference's summary lines (simulate.py:494-507)."""
    print(f'\nLoading reference from {reference}', file=output)
    pref = PackedReference.from_fasta(reference)
    print(f'  {len(pref.names):,} contig{"" if len(pref.names) == 1 else "s"}:', file=output)
    for name, length in zip(pref.names, pref.lengths):
        shape = 'circular' if pref.circular[name] else 'linear'
        print(f'    {name}: {length:,} bp, {shape}, {pref.depths[name]:.2f}x depth', file=output)
    if len(pref.names) > 1:
        print(f'  total size: {sum(pref.lengths):,} bp', file=output)
    return pref


def adjust_depths(pref, frag_lengths, small_plasmid_bias, rng):
    """
    Depth compensation for fragments that cannot come from a short contig (simulate.py:516-536):
    circular contigs (unless --small_plasmid_bias) are scaled by total / sum(L for L <= len),
    linear contigs by total / sum(min(len, L)), over 100,000 sampled fragment lengths.
    Returns the adjusted {name: depth}; exits like the reference when no length fits a circular contig.
    """
    lengths = np.sort(frag_lengths.sample_many(ADJUST_SAMPLES, rng))
    prefix = np.concatenate(([0], np.cumsum(lengths)))
    total = int(prefix[-1])
    depths = dict(pref.depths)
    for name, ref_len in zip(pref.names, pref.lengths):
        n_fit = int(np.searchsorted(lengths, ref_len, side='right'))     # lengths <= ref_len
        if pref.circular[name]:
            if small_plasmid_bias:
                continue
            passing = int(prefix[n_fit])
            if passing == 0:
                sys.exit('Error: fragment length distribution incompatible with reference lengths '
                         '- try running with --small_plasmid_bias to avoid this error')
        else:
            passing = int(prefix[n_fit]) + ref_len * (len(lengths) - n_fit)
        depths[name] *= total / passing
    return depths


def get_target_size(ref_size, quantity):
    """'250M' / '25x' / plain integer -> bases (simulate.py:124-145)."""
    text = str(quantity)
    if str_is_int(text):
        return int(text)
    scale = {'x': ref_size, 'g': 1000000000, 'm': 1000000, 'k': 1000}.get(text[-1:].lower())
    if scale is not None:
        try:
            return int(round(float(text[:-1]) * scale))
        except ValueError:
            pass
    sys.exit('Error: could not parse quantity\n'
             '--quantity must be either an absolute value (e.g. 250M) or a relative depth '
             '(e.g. 25x)')


def adapter_parameters(param_str):
    fields = param_str.split(',')
    try:
        if len(fields) == 2:
            return [float(f) / 100 for f in fields]
    except ValueError:
        pass
    sys.exit('Error: adapter parameters must be two comma-separated values between 0 and 1')


def build_random_adapters(args):
    """An integer adapter 'sequence' means a random adapter of that length (simulate.py:422-432)."""
    made = []
    for attr in ('start_adapter_seq', 'end_adapter_seq'):
        value = getattr(args, attr)
        if str_is_int(value):
            setattr(args, attr, get_random_sequence(int(value)))
            made.append(True)
        else:
            made.append(False)
    return tuple(made)


def _print_adapter(label, seq, rate, amount, was_random, output):
    if seq and rate > 0.0 and amount > 0.0:
        print(f'{label} adapter:', file=output)
        print(f'  seq: {seq}{" (randomly generated)" if was_random else ""}', file=output)
        print(f'  rate:   {rate * 100.0:.1f}%', file=output)
        print(f'  amount: {amount * 100.0:.1f}%', file=output)
    else:
        print(f'{label} adapter: none', file=output)


def print_adapter_summary(start_rate, start_amount, start_seq, end_rate, end_amount, end_seq,
                          random_start, random_end, output):
    print('', file=output)
    _print_adapter('Start', start_seq, start_rate, start_amount, random_start, output)
    print('', file=output)
    _print_adapter('End', end_seq, end_rate, end_amount, random_end, output)


def print_glitch_summary(glitch_rate, glitch_size, glitch_skip, output):
    print('', file=output)
    if glitch_rate == 0:
        print('Reads will have no glitches', file=output)
        return
    print('Read glitches:', file=output)
    for text, value in (('rate (mean distance between glitches)', glitch_rate),
                        ('size (mean length of random sequence)', glitch_size),
                        ('skip (mean sequence lost per glitch) ', glitch_skip)):
        print(f'  {text} = {float_to_str(value):>5}', file=output)


def print_other_problem_summary(args, output):
    print('\nOther problems:', file=output)
    print(f'  chimera join rate: {args.chimeras}%', file=output)
    print(f'  junk read rate:    {args.junk_reads}%', file=output)
    print(f'  random read rate:  {args.random_reads}%', file=output)


def print_progress(count, bp, target, output):
    percent = min(int(1000.0 * bp / target) / 10, 100.0) if target else 100.0
    print(f'\rSimulating: {count:,} read{" " if count == 1 else "s"}  {bp:,} bp  {percent:.1f}%',
          file=output, flush=True, end='')


def sim_params_from_args(args, frag_lengths, identities, start_rate, start_amount, end_rate, end_amount):
    mode, id_a, id_b, id_max = identities.device_mode()
    return SimParams(frag_mean=frag_lengths.mean, frag_stdev=frag_lengths.stdev,
                     identity_mode=mode, id_a=id_a, id_b=id_b, id_max=id_max,
                     start_rate=start_rate, start_amount=start_amount, end_rate=end_rate, end_amount=end_amount,
                     start_adapter=args.start_adapter_seq, end_adapter=args.end_adapter_seq,
                     junk_rate=args.junk_reads / 100, random_rate=args.random_reads / 100,
                     chimera_rate=args.chimeras / 100,
                     glitch_rate=args.glitch_rate, glitch_size=args.glitch_size, glitch_skip=args.glitch_skip)


# ---------------------------------------------------------------------------------------------
# sharding and the stop rule
# ---------------------------------------------------------------------------------------------
class Shard(object):
    """This process's place among the ranks of one node: rank r of world N (torch.distributed or single)."""

    def __init__(self, rank=0, world=1, dist=None, owns_group=False):
        self.rank, self.world, self.dist = rank, world, dist
        self.owns_group = owns_group          # from_env() created the process group: finish() takes it down again

    def finish(self):
        """Leave the job together.  Every rank leaves run_batches at the same batch (stop rule, bad read, failed sink alike);
        a rank that then tears its connections down while a peer is still flushing makes gloo abort the peer, so the ranks
        meet once more and the group this object created is destroyed in order."""
        if self.world > 1 and self.dist is not None and self.dist.is_initialized():
            self.gather_word(0)
            if self.owns_group:
                self.dist.destroy_process_group()
                self.owns_group = False

    def abandon(self):
        """Leave WITHOUT meeting the peers (this rank failed alone): close the connections so that a peer's next exchange fails
        at once instead of waiting for this rank until the backend's timeout."""
        if self.world > 1 and self.dist is not None and self.owns_group and self.dist.is_initialized():
            try:
                self.dist.destroy_process_group()
            except Exception:              # the group may be in the middle of the collective that failed
                pass
            self.owns_group = False

    @classmethod
    def from_env(cls):
        world = int(os.environ.get('WORLD_SIZE', '1'))
        if world <= 1:
            return cls()
        import torch.distributed as dist
        owns = not dist.is_initialized()
        if owns:
            import torch
            # BRX_DIST_BACKEND=gloo keeps the exchange on the host (CPU tensors) whatever the engine computes on: several ranks
            # can then share ONE GPU (BRX_DEVICE picks it), which is how the tests run the HIP engine under world > 1 on a 1-GPU box
            backend = os.environ.get('BRX_DIST_BACKEND') or ('nccl' if torch.cuda.is_available() else 'gloo')
            if torch.cuda.is_available():
                from .engine import rank_device_index
                torch.cuda.set_device(rank_device_index(torch.cuda.device_count()))
            dist.init_process_group(backend=backend)
        return cls(dist.get_rank(), dist.get_world_size(), dist, owns_group=owns)

    def slice_of(self, first, count):
        """Contiguous slice of the super-batch [first, first+count) owned by this rank."""
        per = -(-count // self.world)
        lo = min(self.rank * per, count)
        hi = min(lo + per, count)
        return first + lo, hi - lo

    def _device(self):
        import torch
        return torch.device('cuda', torch.cuda.current_device()) if self.dist.get_backend() == 'nccl' else torch.device('cpu')

    def gather_words(self, words, counts):
        """Every rank's uint32 array (rank i contributes counts[i] words, known to all ranks from the batch plan), in
        rank order, on every rank: the ONLY collective of the driver -- 4 bytes per read (its length and two status
        bits) plus one word per rank, which is what every rank needs to apply the stop rule identically."""
        if self.world == 1:
            return [words]
        import torch
        dev = self._device()
        width = max(max(counts), 1)
        mine = torch.zeros(width, dtype=torch.int32, device=dev)
        if len(words):
            mine[:len(words)] = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev)
        parts = [torch.zeros_like(mine) for _ in range(self.world)]
        self.dist.all_gather(parts, mine)
        return [p[:n].cpu().numpy().view(np.uint32) for p, n in zip(parts, counts)]

    def gather_word(self, v):
        """One uint32 of every rank, as a list of ints in rank order."""
        return [int(x[0]) for x in self.gather_words(np.array([v], dtype=np.uint32), [1] * self.world)]

    def gather_word64(self, v):
        """One uint64 of every rank, as two words each: a byte count that may pass 2^32 (a super-batch's SAM records)."""
        v = int(v)
        parts = self.gather_words(np.array([v & 0xFFFFFFFF, v >> 32], dtype=np.uint32), [2] * self.world)
        return [int(x[0]) | (int(x[1]) << 32) for x in parts]

    def collect_bytes(self, mine, sizes, staging):
        """Record bytes to rank 0, point to point: rank r > 0 sends its `sizes[r]` bytes (a device tensor over RCCL /
        xGMI in production, a CPU tensor over gloo in the tests) and rank 0 receives them in rank order into `staging`.
        No rank other than 0 ever holds another rank's records.  Yields (rank, uint8 tensor) on rank 0."""
        if self.world == 1 or self.rank == 0:
            if sizes[0]:
                yield 0, mine[:sizes[0]]
            for r in range(1, self.world):
                if sizes[r]:
                    buf = staging(sizes[r])
                    self.dist.recv(buf, src=r)
                    yield r, buf
        elif sizes[self.rank]:
            part = mine[:sizes[self.rank]].contiguous()
            if self.dist.get_backend() != 'nccl' and part.device.type != 'cpu':
                part = part.cpu()                # host exchange (gloo) of an engine that computes on the GPU
            self.dist.send(part, dst=0)


FLAG_NOFRAG, FLAG_BAD = 1 << 31, 1 << 30          # status bits packed beside the read length in the 4 B/read gather
BAD_STATUS = RS_TOO_MANY_SEGS | RS_BAND | RS_QMISS
_Pending = collections.namedtuple('_Pending', 'future base n_super first n_mine')      # an issued super-batch [base, base + n_super) and this rank's slice of it


def cut_point(seq_lens, running_total, target_size):
    """
    Index (within this batch) of the read at which the reference's loop stops, or None.  Empty
    reads (seq_len 0) are skipped and never stop the loop (simulate.py:70-71).
    """
    seq_lens = np.asarray(seq_lens, dtype=np.int64)
    reached = np.flatnonzero((running_total + np.cumsum(seq_lens) >= target_size) & (seq_lens > 0))
    return int(reached[0]) if len(reached) else None


def plan_batch(remaining_bases, mean_length, world, max_batch):
    """Reads in the next super-batch: a little over the expected need, rounded to 64 per rank."""
    expect = remaining_bases / max(mean_length, 1.0)
    want = int(expect * 1.05) + 8 * world
    per_rank = min(max(-(-want // world), 1), max_batch)
    per_rank = -(-per_rank // 64) * 64 if per_rank >= 64 else per_rank
    return per_rank * world


def exchange_words(stats):
    """A batch's 4 B/read for the exchange between ranks: length (0 for skipped reads) | NOFRAG << 31 | BAD << 30."""
    words = (stats['seq_len'].astype(np.uint32) * (stats['rec_len'] > 0)).astype(np.uint32)
    assert not len(words) or int(words.max()) < FLAG_BAD
    words |= np.where(stats['status'] & RS_NOFRAG, FLAG_NOFRAG, 0).astype(np.uint32)
    words |= np.where(stats['status'] & BAD_STATUS, FLAG_BAD, 0).astype(np.uint32)
    return words


def stop_decision(allw, base, total, target_size):
    """(last, fatal, bad_read) from every rank's words of the super-batch starting at read `base`, `total` bases consumed before it.  `last`: batch
    position of the last read kept: the one reaching the target, or the one before an earlier flagged read (NOFRAG: `fatal`, else `bad_read`), or the end."""
    lens = (allw & (FLAG_BAD - 1)).astype(np.int64)
    cut = cut_point(lens, total, target_size)
    wrong = np.flatnonzero(allw & (FLAG_NOFRAG | FLAG_BAD))
    if len(wrong) and (cut is None or wrong[0] < cut):
        stop_at = int(wrong[0])
        nofrag = bool(allw[stop_at] & FLAG_NOFRAG)
        return stop_at - 1, nofrag, None if nofrag else base + stop_at
    return (cut if cut is not None else len(allw) - 1), False, None


def kept_bytes(stats, first, base, last, n_mine):
    """(keep, my_bytes): how many of this rank's reads [first, first + n_mine) have a batch position <= last, and their FASTQ bytes."""
    keep = int(np.clip(last - (first - base) + 1, 0, n_mine))
    return keep, (int(stats['rec_off'][keep - 1] + stats['rec_len'][keep - 1]) if keep else 0)


class TruthSpec(collections.namedtuple('TruthSpec', 'kinds tags fmt')):
    """What truth output a job writes beside its FASTQ: `kinds`, the files (--truth-paf, --truth-sam, --truth-bam) as a subset of
    ('paf', 'sam', 'bam') in that order, which is the order their records are made and shipped in; `tags` (--truth-tags), TAG_MD | TAG_SA
    on the SAM and BAM records; `fmt` (--truth-eqx, --truth-cs), FMT_EQX | FMT_CS | FMT_CS_LONG on all three.  'depth' (--truth-depth), the
    last kind, is not a file of records: its batches are the records' end points, which its sink keeps until the job ends (_DepthFile);
    tags and formats take no part in it.  'bam_sorted' (--truth-bam-sorted) is a file of records, those of 'bam': its batches are the BAM
    records as they are, framed with their reads' lengths (sorted_frame), which its sink keeps until the job ends (_SortedBamFile).
    TruthSpec.NONE: none."""
    __slots__ = ()

    def __new__(cls, kinds=(), tags=0, fmt=0):
        asked = set(kinds)
        return super().__new__(cls, tuple(k for k in TRUTH_KINDS if k in asked), int(tags), int(fmt))

    @classmethod
    def from_args(cls, args):
        return cls([k for k in TRUTH_KINDS if getattr(args, 'truth_' + k, None)], getattr(args, 'truth_tags', None) or 0,
                   getattr(args, 'truth_fmt', None) or 0)

    def share(self):
        """Bytes of truth records per FASTQ byte that a batch's buffers are first sized for: every file's own share, what the tags add to
        the SAM and the BAM records, what the formats add to each file."""
        share = sum(TRUTH_SHARE[k] for k in self.kinds)
        records = [k for k in self.kinds if k != 'depth']          # the files of records: the events of 'depth' carry neither tags nor formats
        share += tag_share(self.tags) * sum(k != 'paf' for k in records)
        return share + sum(fmt_share(self.fmt, k) for k in records)


TruthSpec.NONE = TruthSpec()


def expected_out_bytes(engine, n_reads, mean_length, truth=None):
    """Bytes a batch of `n_reads` reads is expected to leave on the device, the truth records of `truth` (a TruthSpec) included -- the BAM
    records before they are compressed too: by the engine's estimate
    from its parameters, or at 2.1 B per base + 400 per read for an engine without one (None: its parameters are not set yet)."""
    per_read = engine.expected_record_bytes() if hasattr(engine, 'expected_record_bytes') else 2.1 * mean_length + 400.0
    out_bytes = int(n_reads * per_read)
    share = (truth or TruthSpec.NONE).share()
    return int(out_bytes * (1.0 + share)) if share else out_bytes


def driver_reserve_bytes():
    """Device memory left to the runtime's own allocations (engines_for_memory)."""
    return int(float(os.environ.get('BRX_DRIVER_RESERVE_GB', '24')) * (1 << 30))


def engines_for_memory(free, wanted, arena_bytes, arenas_held, out_bytes, reserve):
    """How many of `wanted` engines fit into `free` bytes of device memory, at least one: n - arenas_held more arenas, n output buffers and
    n + 2 copies of a batch's bytes waiting for the consumer, beside `reserve` for what the runtime allocates on its own -- the private segments
    of the planning kernels (1.6 KB per lane, per hardware queue: ~0.9 GB each over the ~20 queues of a six-engine job), the gzip stage, other
    ranks' records on rank 0.  A job that asks for more runs on fewer (six 65536-read engines with 40 GB arenas died with
    HSA_STATUS_ERROR_OUT_OF_RESOURCES at the edge of the 288 GB, where no allocation of ours failed)."""
    n = wanted
    while n > 1 and (n - arenas_held) * arena_bytes + (2 * n + 2) * out_bytes + reserve > free:
        n -= 1
    return n


def _on_gpu(engine):
    """The engine computes on a GPU (the tests' CPU checker engines have no `device`)."""
    return getattr(getattr(engine, 'device', None), 'type', '') == 'cuda'


class _HostRing(object):
    """Pinned host buffers for the FASTQ bytes on their way out: the device-to-host copy of
    a finished batch lands in page-locked memory (full PCIe rate, no staging copy by the runtime) and a writer thread
    hands it to the sink while the GPU works on the next batches.  A buffer returns to the ring when the writer is done
    with it; `depth` buffers bound the memory and apply back-pressure when the sink is slower than the GPU."""

    def __init__(self, torch, pinned, sink, defer_errors=False, depth=3):
        self.torch, self.pinned = torch, pinned
        # The buffers are allocated (and grown) on first use.  (Pinning them beside the first batch looked free and was not: 3 x 2.6 GB of
        # hipHostMalloc against the clone threads' 40 GB arenas made every clone take 1.1 s instead of 0.05, profiles/r05b_cli_30x.json.)
        self.free = queue.Queue()
        for _ in range(depth):
            self.free.put(None)
        self.todo = queue.Queue()
        self.error = None
        self.defer_errors = defer_errors            # multi-rank runs: a failed sink is reported through the per-batch exchange, so that every rank stops at the same batch
        self.sink = sink
        self.sink_seconds = self.alloc_seconds = 0.0
        self.copy_stream = None                     # device -> pinned copies of the batches' bytes (write)
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        while True:
            item = self.todo.get()
            if item is None:
                return
            buf, n, landed, _source = item
            try:
                if landed is not None:              # the copy into `buf` runs on the ring's own stream: sleep until it has landed
                    while not landed.query():       # (event.synchronize() spins a core on this stack)
                        time.sleep(0.0002)
                if self.error is None and n:
                    t0 = time.perf_counter()
                    self.sink(memoryview(buf.numpy())[:n])
                    self.sink_seconds += time.perf_counter() - t0
            except BaseException as ex:             # surfaced by the next stage() / write() of the producer, or by flush()
                self.error = ex
            self.free.put(buf)

    def stage(self, nbytes):
        """A host buffer of at least nbytes (blocks while all buffers are with the writer).  A sink that has failed
        (BrokenPipe behind `| head`, a full disk) stops the run here, at the next batch, not after the whole target."""
        if self.error is not None and not self.defer_errors:
            raise self.error
        buf = self.free.get()
        if buf is None or buf.numel() < nbytes:
            cap = max(int(nbytes * 1.25), 1 << 20)
            t0 = time.perf_counter()
            buf = self.torch.empty(cap, dtype=self.torch.uint8, pin_memory=self.pinned)
            self.alloc_seconds += time.perf_counter() - t0
        return buf

    def write(self, tensor):
        """Copy a uint8 tensor (device or host) into a ring buffer and queue it for the sink.  A device tensor is copied
        ASYNCHRONOUSLY on the ring's own stream: the consumer thread goes on to the next batch (stop rule, refill of the pipeline) while the
        bytes cross PCIe, and the writer thread waits for the copy, not the consumer (which spent 5.0 of configs[4]'s 9.1 s of read loop inside
        blocking copies, profiles/r04_cli_30x_hifi.json).  The source tensor travels with the queue entry: its memory is not reused before."""
        n = int(tensor.numel())
        buf = self.stage(n)
        landed = None
        if n and self.pinned and tensor.is_cuda and not os.environ.get('BRX_SYNC_COPY_OUT'):
            torch = self.torch
            if self.copy_stream is None:
                # (default priority: a high-priority stream, -1, made configs[4]'s read loop 9.8 s against 8.8 s, profiles/r05h;
                #  the copy itself runs at 57 GB/s on an idle GPU: tools/d2h_probe.py)
                self.copy_stream = torch.cuda.Stream(device=tensor.device)
            self.copy_stream.wait_stream(torch.cuda.current_stream(tensor.device))     # the tensor's producer has been waited for on the current stream
            with torch.cuda.stream(self.copy_stream):
                buf[:n].copy_(tensor, non_blocking=True)
                landed = torch.cuda.Event()
                landed.record(self.copy_stream)
        elif n:
            buf[:n].copy_(tensor, non_blocking=False)
        self.todo.put((buf, n, landed, tensor if landed is not None else None))

    def flush(self, reraise=True):
        self.todo.put(None)
        self.thread.join()
        if reraise and self.error is not None:
            raise self.error


class _ArenaPrefetch(object):
    """The job's scratch arenas, allocated by threads of their own from the moment the first engine exists -- beside the model tables, the genome's
    upload and the first batch -- instead of when the read loop asks for them.  On a freshly leased GPU a 40 GB arena is ~4 s of `hipMalloc` (the
    driver provisions and clears the memory: 21 s of thread time for the five clones of a 30x human job, profiles/r05_cli_30x.json); started 1.4 s
    before the loop, the engines are there 1.4 s earlier.  take() hands out the next arena (waiting for its thread) or None."""

    def __init__(self, torch, device, nbytes, count):
        self.nbytes, self.count = int(nbytes), int(count)
        self.slots = [None] * self.count
        self.errors = []
        self.lock = threading.Lock()
        self.next = 0
        self.seconds = 0.0

        def alloc(i):
            t0 = time.perf_counter()
            try:
                torch.cuda.set_device(device)
                self.slots[i] = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
            except BaseException as ex:                  # the taker allocates what it needs itself (and reports what fails then)
                self.errors.append(ex)
            with self.lock:
                self.seconds += time.perf_counter() - t0
        self.threads = [threading.Thread(target=alloc, args=(i,), daemon=True) for i in range(self.count)]
        for th in self.threads:
            th.start()

    def take(self):
        with self.lock:
            i = self.next
            if i >= self.count:
                return None
            self.next += 1
        self.threads[i].join()
        t, self.slots[i] = self.slots[i], None
        return t

    def release_rest(self):
        while self.take() is not None:
            pass

    @staticmethod
    def for_job(engine, target_size, mean_length, error_rate, in_flight, world, truth=None):
        """Arenas for the batches in flight of THIS job on THIS device, or None (not a GPU engine, a job of one small batch,
        BRX_ARENA_PREFETCH=0).  How many: what the job will use and the free memory holds (engines_for_memory, no arena mapped yet)."""
        # Measured (profiles/r05i_arena_prefetch.json, r05k_*; DESIGN.md has the figures): the read loop then runs undisturbed, 18.8-19.0 s for
        # the 30x human job (20.9-23.7 without).  Right behind another process that gave 40+ GB back the allocations are ~0.13 s per GB and the
        # command takes what it took without this; on an idle GPU they are nearly free.  Never slower, so on by default; BRX_ARENA_PREFETCH=0: off.
        if not _on_gpu(engine) or os.environ.get('BRX_ARENA_PREFETCH', '1') in ('', '0'):
            return None
        from .engine import arena_estimate
        first_batch = plan_batch(target_size, mean_length, world, DEFAULT_MAX_BATCH) // max(world, 1)
        if first_batch < 4096:
            return None                                  # a small job: one arena, sized by presize
        nbytes = engine.arena_bytes(first_batch, mean_length, error_rate) if hasattr(engine, 'arena_bytes') else arena_estimate(first_batch, mean_length, error_rate)
        out_bytes = expected_out_bytes(None, first_batch, mean_length, truth)        # the engine's parameters are not set yet
        batches = -(-int(target_size) // max(int(first_batch * mean_length * max(world, 1)), 1))
        free, _ = engine.torch.cuda.mem_get_info(engine.device)
        n = engines_for_memory(free, max(1, min(int(in_flight), batches)), nbytes, 0, out_bytes, driver_reserve_bytes())
        return _ArenaPrefetch(engine.torch, engine.device, nbytes, n)


class _Done(object):
    """A finished batch behind a future's interface: what a pool of one engine, which has no worker thread, hands back."""
    def __init__(self, v): self.v = v
    def result(self): return self.v


# What a worker hands back: the FASTQ bytes, the stats, (text bytes, gzip members) or None, and per truth file
# {kind: (records or their BGZF blocks, read offsets into the records, whether these are the blocks)} -- {} for a batch of no reads
_Batch = collections.namedtuple('_Batch', 'out stats packed truth')


class _BatchPool(object):
    """`in_flight` engines (the given one + clones sharing its device tables), each driven by its own host thread on its own HIP stream, so that
    several batches overlap on the GPU.

    Batches are CONSUMED in index order (the stop rule), but they do not FINISH in index order: read lengths differ, and so do batch times.  An engine
    released only when its batch is consumed idles behind the slowest of the batches before it (60-70 % of the rate bench.py measures on the same
    kernels: DESIGN.md, "Through the CLI driver"), so the worker thread itself takes a free engine when it starts a batch, copies the batch's FASTQ
    bytes device-to-device out of the engine's buffer when the batch is done (2 GB at HBM speed: ~1 ms) and gives the engine back at once; `depth` =
    in_flight + 2 batches may be outstanding, the surplus holding only their bytes."""

    def __init__(self, engine, in_flight, arenas=None, device_gzip=False, truth=None):
        self.arenas = arenas
        # the truth files: every batch's truth alignments, made by its worker beside its FASTQ.  The BAM records of a batch that the stop rule
        # cannot cut (submit(..., pack=True)) are also compressed whole into BGZF blocks by the worker, on its engine's stream; any other
        # batch's are compressed by the consumer, for the reads it keeps
        self.truth = truth or TruthSpec.NONE
        # --gzip-device: the worker of a batch that the stop rule cannot cut (submit(..., pack=True)) packs ITS batch on ITS engine's stream and hands
        # over the gzip members; the consumer packs only the job's last batches (every batch there: 10.4 s of configs[4]'s read loop against 6.0 s)
        self.device_gzip = bool(device_gzip)
        torch = getattr(engine, 'torch', None)           # absent on the tests' CPU checker engines
        self.on_gpu = torch is not None and _on_gpu(engine)
        n = in_flight if in_flight > 1 and hasattr(engine, 'clone') else 1
        self.engines = [engine] + [None] * (n - 1)
        self.streams = [torch.cuda.Stream(device=engine.device) if self.on_gpu else None for _ in range(n)]
        self.free = queue.Queue()
        self.free.put(0)                                 # engine 0 exists already: it takes the first batch
        self.create_seconds = 0.0
        self.create_errors = []                          # clones that could not be made: the job runs on fewer engines
        self.lock = threading.Lock()                     # the counters below are updated by several worker threads
        # Mapping a clone's 40 GB arena takes ~0.6-1.2 s per engine whoever does it and whenever (the driver clears the memory: 14-29 ms per
        # GB, also for ONE 200 GB allocation on an idle device), so the clones are made by their own threads while engine 0 already computes.
        # Clone i is started when the job submits its (i + 1)-th batch: a one-batch job (a bacterial genome at 100x) maps no clone at all.
        def make(i):                                     # a clone maps tens of GB of scratch: its own thread, beside the first batches
            t0 = time.perf_counter()
            try:
                if self.on_gpu:
                    torch.cuda.set_device(self.engines[0].device)
                spare = self.arenas.take() if self.arenas is not None else None       # allocated since the first engine exists, or None
                self.engines[i] = self.engines[0].clone(scratch_tensor=spare) if spare is not None else self.engines[0].clone()
                self.free.put(i)
            except BaseException as ex:                  # this slot never joins the queue; engine 0 and the other clones carry on
                with self.lock:
                    self.create_errors.append(ex)
            finally:
                with self.lock:
                    self.create_seconds += time.perf_counter() - t0
        self.makers = [threading.Thread(target=make, args=(i,), daemon=True) for i in range(1, len(self.engines))]
        self.started = 0                                 # makers started so far
        self.submitted = 0
        self.depth = len(self.engines) + (2 if len(self.engines) > 1 else 0)
        self.job_seconds = self.job_count = 0.0          # wall time of the device batches (bench.py --d2h reports the average)
        self.wait_engine_seconds = 0.0
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=len(self.engines)) if len(self.engines) > 1 else None

    def __len__(self):
        return self.depth

    @staticmethod
    def engines_that_fit(torch, engine, in_flight, out_bytes):
        """How many engines the device's FREE memory holds (engines_for_memory): every clone maps an arena as large as the first engine's."""
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(engine.device)
        scratch = engine.scratch_bytes() if hasattr(engine, 'scratch_bytes') else 0
        return engines_for_memory(free, in_flight, scratch, 1, int(out_bytes), driver_reserve_bytes())       # the first engine's arena is mapped already

    COPY_STEP = 1 << 28

    @classmethod
    def _copy_of(cls, torch, out):
        """The batch's bytes out of the engine's buffer, in a block whose CAPACITY is a multiple of 256 MB.  A plain clone() asks torch's caching
        allocator for the batch's exact size -- 2.05-2.10 GB, never the same twice -- and a cached block a few MB short serves nobody: it stays
        cached and a new one is mapped, until over the 94 batches of the 30x job the cache had crept through the driver's reserve and a queue's
        private segment failed with HSA_STATUS_ERROR_OUT_OF_RESOURCES.  In steps, every freed block fits the next batch."""
        n = int(out.numel())
        if n <= cls.COPY_STEP // 16:
            return out.clone()
        cap = -(-n // cls.COPY_STEP) * cls.COPY_STEP
        buf = torch.empty(cap, dtype=torch.uint8, device=out.device)
        buf[:n].copy_(out)
        return buf[:n]

    def submit(self, seed, first, n_mine, pack=False):
        self.submitted += 1
        while self.started < min(self.submitted - 1, len(self.makers)):      # the k-th batch in the pipeline is what clone k - 1 is for
            self.makers[self.started].start()
            self.started += 1
        if self.pool is None:
            return _Done(self._work(seed, first, n_mine, pack))
        return self.pool.submit(self._work, seed, first, n_mine, pack)

    def _work(self, seed, first, n_mine, pack):
        """One batch on the next free engine, on a worker thread: a _Batch."""
        import torch
        t_q = time.perf_counter()
        i = self.free.get()
        t_job = time.perf_counter()
        with self.lock:
            self.wait_engine_seconds += t_job - t_q
        try:
            stream, eng = self.streams[i], self.engines[i]
            if n_mine == 0:
                return _Batch(torch.zeros(0, dtype=torch.uint8), np.zeros(0, dtype=eng.stats_dtype), None, {})
            if not self.on_gpu:
                out, stats = eng.simulate_batch(seed, first, n_mine, allow_nofrag=True)
                return _Batch(torch.from_numpy(np.ascontiguousarray(out).copy()), stats.copy(), None, self._truth_of(eng, n_mine, pack))
            torch.cuda.set_device(eng.device)
            with torch.cuda.stream(stream):
                out, stats = eng.simulate_batch_device(seed, first, n_mine, allow_nofrag=True)
                # the truth alignments read what the batch left in the engine's arena: same job, same stream, before the engine is free
                truth = self._truth_of(eng, n_mine, pack)
                stats = stats.copy()
                packed = None
                if pack and self.device_gzip and len(stats) and hasattr(eng, 'gzip_device'):
                    from .output import fastq_blocks
                    live = np.flatnonzero(stats['rec_len'] > 0)
                    if len(live) and not (stats['status'] & (RS_NOFRAG | BAD_STATUS)).any():
                        nbytes = int(stats['rec_off'][live[-1]] + stats['rec_len'][live[-1]])
                        blocks = fastq_blocks(stats['rec_off'], stats['rec_len'], stats['seq_len'], nbytes)
                        packed = (nbytes, eng.gzip_device(out[:nbytes], blocks))      # a new tensor, made on this batch's stream
                out = self._copy_of(torch, out) if packed is None else None   # the engine's buffer is free again; the copy runs on this batch's stream ...
                stream.synchronize()                     # ... and is complete before the engine is handed to the next batch
                return _Batch(out, stats, packed, truth)
        finally:
            with self.lock:
                self.job_seconds += time.perf_counter() - t_job
                self.job_count += 1
            self.free.put(i)

    def _truth_of(self, eng, n_mine, pack):
        """{kind: (the batch's records of that kind, their read offsets, False)}; with `pack` BAM's are (the records' BGZF blocks, made at
        once on the same stream, the read offsets into the records, True).  'bam_sorted' takes the BAM records as they are: with 'bam' in
        the job too they are emitted once."""
        truth, kinds, raw_bam = {}, self.truth.kinds, None
        for kind in kinds:
            if kind == 'bam_sorted':
                data, off = raw_bam or eng.emit_truth_device('bam', n_mine, tags=self.truth.tags, fmt=self.truth.fmt)
                truth[kind] = (data, off, False)
                continue
            data, off = eng.emit_truth_device(kind, n_mine, tags=self.truth.tags, fmt=self.truth.fmt)
            if kind == 'bam' and 'bam_sorted' in kinds:
                raw_bam = (data, off)
            packed = kind == 'bam' and pack and int(data.numel()) > 0
            truth[kind] = (eng.bgzf_device(data) if packed else data, off, packed)
        return truth

    def close(self):
        for th in self.makers[:self.started]:            # clones no batch asked for were never started
            th.join()
        if self.pool is not None:
            self.pool.shutdown(wait=True)
        for eng in self.engines[1:]:
            if eng is not None:
                eng.close()


def run_batches(engine, seed, target_size, mean_length, write, output, shard=None, max_batch=None, in_flight=1, device_gzip=False,
                local_write=None, local_parts=None, expected_error=None, arenas=None, truth=None, truth_write=None):
    """
    The `while total_size < target_size` loop (simulate.py:63-86) over super-batches of read indices.
    `write(bytes_like)` receives the FASTQ bytes in read order on rank 0 only.  Returns (read count, total bases).

    Up to `in_flight` super-batches run at once (one engine clone, stream and host thread each).  They cover
    consecutive index ranges and are CONSUMED in index order, where the stop rule is applied, so the output does
    not depend on `in_flight` or on the batch sizes; batches issued beyond the stopping read are discarded.  The
    issue schedule depends only on consumed totals, so every rank of a multi-GPU run plans the same batches.

    Between ranks: one all_gather of 4 bytes per read (length + two status bits) and one word per rank (bytes kept)
    per super-batch, then the kept record bytes travel point to point to rank 0 only.  On every rank the bytes leave the
    GPU through a ring of pinned host buffers drained by a writer thread (_HostRing).

    device_gzip: every rank turns the bytes it keeps into gzip members ON ITS GPU (brx_gzip_device, blocks cut at the
    lines of the records: badread_amd.output.fastq_blocks) before they go anywhere; `write` then receives gzip data.

    local_write (--output-shards): EVERY rank hands the bytes it keeps to its own `local_write` through its own pinned ring
    (its own PCIe link, its own file) and nothing travels to rank 0; `local_parts(n)` receives the byte count of every
    super-batch, which is what puts the ranks' files back into read order (batch by batch, rank after rank).  The
    exchange of 4 bytes per read and the stop rule are the same: the same reads are kept.

    truth (a TruthSpec) / truth_write ({kind: callable}): every batch also yields its reads' truth alignments in every kind of the spec
    (engine.emit_truth_device), cut at the same read as the FASTQ.  `truth_write[kind]` receives them in read order through a ring of its
    own: on rank 0, over the same point-to-point exchange as the FASTQ, or with local_write on every rank, its own reads' records (those
    of its own FASTQ file, in that file's order).  The @ lines of a SAM file are the caller's (sam_header).  The BAM records are cut at
    the same read and then compressed on the GPU into BGZF blocks (engine.bgzf_device); only the blocks cross to the host and between
    ranks.  A batch the stop rule cannot cut is compressed whole by its worker.  Header and EOF block are the caller's.

    A sink that fails on one rank of a multi-rank run (a full disk, a closed pipe) is reported in the same exchange -- one
    word per rank -- so that every rank leaves the loop at the same batch instead of waiting in a collective.
    """
    run = _Run(engine, seed, target_size, mean_length, write, output, shard or Shard(), max_batch or DEFAULT_MAX_BATCH, in_flight,
               device_gzip, local_write, local_parts, expected_error, arenas, truth or TruthSpec.NONE, truth_write or {})
    run_batches.last_timing = run.timing
    run.size_pipeline()
    run.open_rings()
    try:
        while run.total < target_size:
            run.fill()
            if not run.consume(run.pending.popleft()):
                break
    finally:
        run.close(unwinding=sys.exc_info()[0] is not None)
    if run.shard.rank == 0:
        print('\n', file=output)
    run.raise_outcome()
    return run.count, run.total


class _Run(object):
    """One call of run_batches: its arguments, the pipeline and the consumed totals as attributes, its steps as methods.  Every collective
    (Shard.gather_words, collect_bytes) and every pool.submit comes at a point that depends only on consumed totals: the ranks stay in step."""

    def __init__(self, engine, seed, target_size, mean_length, write, output, shard, max_batch, in_flight, device_gzip,
                 local_write, local_parts, expected_error, arenas, truth, truth_write):
        import torch
        self.torch = torch
        self.engine, self.seed, self.target_size, self.write, self.output, self.shard = engine, seed, target_size, write, output, shard
        self.max_batch, self.in_flight, self.device_gzip, self.expected_error, self.arenas = max_batch, in_flight, device_gzip, expected_error, arenas
        self.local_write, self.local_parts, self.truth, self.truth_write = local_write, local_parts, truth, truth_write
        self.count = self.total = self.next_read = 0
        self.expected_mean = float(mean_length)
        self.pending = collections.deque()          # _Pending, in index order
        self.fatal, self.bad_read, self.sink_failed_on = False, None, None
        self.pool = self.ring = self.gz_engine = None
        self.truth_rings = {}                       # {kind: _HostRing} of the truth files this rank writes
        if shard.rank == 0:
            print_progress(0, 0, target_size, output)
        self.timing = collections.Counter()         # seconds of the consumer thread per activity (bench.py --d2h)
        self.t_job = time.perf_counter()

    def size_pipeline(self):
        """The first engine's arena (the clones copy its size) for the batches this job will issue; as many engines as fit on every rank."""
        engine, shard, arenas = self.engine, self.shard, self.arenas
        first_arena, out_bytes = None, 0
        if hasattr(engine, 'presize'):
            first_batch = plan_batch(self.target_size, self.expected_mean, shard.world, self.max_batch) // shard.world
            first_arena = arenas.take() if arenas is not None else None
            if first_arena is not None:              # allocated beside the start-up (_ArenaPrefetch)
                engine.adopt_scratch(first_arena)
            else:                                    # by the job's identity law, if given: arenas for Q30 reads are half those of 95 % reads
                engine.presize(first_batch, self.expected_mean, self.expected_error)
            out_bytes = expected_out_bytes(engine, first_batch, self.expected_mean, self.truth)
        asked = fit = max(1, int(self.in_flight))
        if first_arena is not None:
            fit = min(fit, arenas.count)             # decided when the arenas were requested, by the same rule, from the memory that was free then
        elif fit > 1 and hasattr(engine, 'scratch_bytes') and _on_gpu(engine):
            fit = _BatchPool.engines_that_fit(engine.torch, engine, fit, out_bytes)
        if shard.world > 1:                          # the issue schedule depends on the depth of the pipeline: the same on every rank
            fit = min(shard.gather_word(fit))
        if fit < asked and shard.rank == 0:
            print(f'  {fit} of the {asked} batches in flight asked for fit into the free device memory', file=self.output)
        self.pool = _BatchPool(engine, fit, arenas, device_gzip=self.device_gzip, truth=self.truth)
        self.timing['create_engines'] = time.perf_counter() - self.t_job

    def open_rings(self):
        """A ring for the FASTQ bytes (rank 0, or every rank with local_write), one of its own for the PAF text, for the SAM records and for the
        BAM blocks, the consumer's small engine for gzip members and BGZF blocks."""
        pinned, defer = self.pool.on_gpu, self.shard.world > 1
        if self.local_write is not None or self.shard.rank == 0:
            self.ring = _HostRing(self.torch, pinned, self.local_write if self.local_write is not None else self.write, defer)
        self.truth_rings = {kind: _HostRing(self.torch, pinned, self.truth_write[kind], defer)
                            for kind in self.truth.kinds if self.truth_write.get(kind) is not None}
        if self.device_gzip and not hasattr(self.engine, 'gzip_device'):
            sys.exit('Error: --gzip-device needs the GPU engine')
        if self.device_gzip or 'bam' in self.truth.kinds:
            self.gz_engine = self.engine.clone(1 << 20) if hasattr(self.engine, 'clone') else self.engine      # its own context: the others are busy

    def staging(self, nbytes):
        """Where rank 0 receives another rank's records (device memory under RCCL): a tensor of ITS OWN per receive.  The ring copies device tensors
        asynchronously and keeps them until the copy has landed; one reused buffer would be overwritten by the next rank's `recv` meanwhile."""
        return self.torch.empty(int(nbytes), dtype=self.torch.uint8, device=self.shard._device())

    def fill(self):
        """Keep the pipeline full: what is outstanding is assumed to deliver its expected number of bases.  Called at
        points that depend only on consumed totals, so every rank issues the same batches."""
        while len(self.pending) < len(self.pool):
            outstanding = sum(p.n_super for p in self.pending) * self.expected_mean
            remaining = self.target_size - self.total - outstanding
            if remaining <= 0 and self.pending:
                break
            n_super = plan_batch(max(remaining, 1), self.expected_mean, self.shard.world, self.max_batch)
            first, n_mine = self.shard.slice_of(self.next_read, n_super)
            # --gzip-device: a batch with at least three batches' worth of bases still to come behind it is kept whole
            # (--truth-bam: the same batches' BAM records are compressed whole by their workers)
            pack = (self.device_gzip or 'bam' in self.truth.kinds) and remaining > 4.0 * n_super * self.expected_mean
            self.pending.append(_Pending(self.pool.submit(self.seed, first, n_mine, pack=pack), self.next_read, n_super, first, n_mine))
            self.next_read += n_super

    def consume(self, batch):
        """The next super-batch in index order: wait, exchange, decide, pack, account, refill, ship.  False: the loop ends here."""
        timing, shard, t0 = self.timing, self.shard, time.perf_counter()
        out, stats, prepacked, truth = batch.future.result()
        timing['wait_for_batch'] += time.perf_counter() - t0
        timing['batches'] += 1
        allw = exchange_words(stats)
        if shard.world > 1:                         # every rank's words in read order, and one more of each rank: "my sink has failed" (the FASTQ's or a truth file's)
            per_rank = [Shard(r, shard.world).slice_of(batch.base, batch.n_super)[1] for r in range(shard.world)]
            failed_here = any(x is not None and x.error is not None for x in (self.ring, *self.truth_rings.values()))
            parts = shard.gather_words(np.append(allw, np.uint32(1 if failed_here else 0)), [c + 1 for c in per_rank])
            failed = [r for r, part in enumerate(parts) if part[-1]]
            if failed:                              # every rank leaves here, at the same batch
                self.sink_failed_on = failed[0]
                return False
            allw = np.concatenate([part[:-1] for part in parts])
        last, self.fatal, self.bad_read = stop_decision(allw, batch.base, self.total, self.target_size)
        keep, my_bytes = kept_bytes(stats, batch.first, batch.base, last, batch.n_mine)
        out, my_bytes = self.pack(out, stats, prepacked, keep, my_bytes)
        local = self.local_write is not None       # every rank: its own bytes through its own ring to its own file
        sizes = None if local else [my_bytes]
        if shard.world > 1 and not local:
            sizes = shard.gather_word(my_bytes)
            assert my_bytes < 2 ** 32
        used = (allw & (FLAG_BAD - 1)).astype(np.int64)[:last + 1]
        self.count += int((used > 0).sum())
        self.total += int(used.sum())
        stop = self.fatal or self.bad_read is not None
        if self.count and not stop:
            self.expected_mean = max(self.total / self.count, 1.0)
        if not stop and self.total < self.target_size:
            self.fill()                             # the freed engine starts its next batch while this one's bytes leave
        t0 = time.perf_counter()
        self.ship(self.ring, out, my_bytes, sizes)
        if local and self.local_parts is not None:
            self.local_parts(my_bytes)
        # The truth records of the same reads, the same way, file after file.  PAF's sizes travel as 32-bit words like the FASTQ's; a
        # super-batch's SAM records may pass 2^32 bytes on a rank, and BAM's leave as BGZF blocks: whole blocks of every rank, so rank 0
        # only concatenates
        for kind in self.truth.kinds:
            part = truth.get(kind)                  # None: no reads of this batch on this rank
            if kind == 'bam':
                data = self.pack_bam(part, keep)
                nbytes = int(data.numel()) if data is not None else 0
            elif kind == 'bam_sorted':
                data = sorted_frame(self.torch, part, keep)
                nbytes = int(data.numel()) if data is not None else 0
            else:
                data, nbytes = (part[0], int(part[1][keep])) if part is not None else (None, 0)
            kind_sizes = None
            if shard.world > 1 and not local:
                kind_sizes = shard.gather_word(nbytes) if kind == 'paf' else shard.gather_word64(nbytes)
                assert kind != 'paf' or nbytes < 2 ** 32
            self.ship(self.truth_rings.get(kind), data, nbytes, kind_sizes)
        timing['copy_out'] += time.perf_counter() - t0
        if shard.rank == 0:
            print_progress(self.count, self.total, self.target_size, self.output)
        return not stop

    def pack(self, out, stats, prepacked, keep, my_bytes):
        """(what leaves, its bytes) for this rank's first `keep` reads, `my_bytes` of text.  --gzip-device: a batch its worker packed
        whole leaves as it is; one the stop rule cut after all is unpacked and, like every batch not packed ahead, packed here."""
        if prepacked is not None and my_bytes == prepacked[0]:
            self.timing['batches_packed_by_their_worker'] += 1
            return prepacked[1], int(prepacked[1].numel())
        if prepacked is not None:      # reads far longer than the job expected: unpack on the host, once
            text = gzip.decompress(bytes(prepacked[1].cpu().numpy()))
            out = self.torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(prepacked[1].device)
        if self.device_gzip and self.gz_engine is not None and my_bytes:
            from .output import fastq_blocks
            t0 = time.perf_counter()
            blocks = fastq_blocks(stats['rec_off'][:keep], stats['rec_len'][:keep], stats['seq_len'][:keep], my_bytes)
            out = self.gz_engine.gzip_device(out[:my_bytes], blocks)       # a new tensor: the engine's buffer is free again
            my_bytes = int(out.numel())
            self.timing['device_gzip'] += time.perf_counter() - t0
        return out, my_bytes

    def pack_bam(self, bam, keep):
        """The BGZF blocks of the BAM records of this rank's first `keep` reads (None: no reads here).  A batch its worker compressed whole
        leaves as it is; one the stop rule cut after all is unpacked on the host, once (a BGZF stream is a gzip stream), and like every
        batch not compressed ahead its kept records are compressed here, on the consumer's small engine."""
        if bam is None:
            return None
        data, off, packed = bam
        raw = int(off[keep])
        if packed and raw == int(off[-1]):
            self.timing['bam_batches_packed_by_their_worker'] += 1
            return data
        if packed:
            records = gzip.decompress(bytes(data.cpu().numpy()))
            data = self.torch.from_numpy(np.frombuffer(records, dtype=np.uint8).copy()).to(data.device)
        t0 = time.perf_counter()
        blocks = self.gz_engine.bgzf_device(data[:raw])
        self.timing['device_bgzf'] += time.perf_counter() - t0
        return blocks

    def ship(self, ring, data, nbytes, sizes):
        """`nbytes` of `data` into this rank's own `ring` (sizes None), or every rank's `sizes` bytes point to point into rank 0's."""
        if sizes is None:
            if nbytes and ring is not None:
                ring.write(data[:nbytes])
        else:
            for _, part in self.shard.collect_bytes(data, sizes, self.staging):
                ring.write(part)                    # rank 0: through pinned memory to the writer thread

    def close(self, unwinding):
        """Wait for what is in flight, close the engines, drain the rings.  `unwinding`: an exception propagates, which a sink's must not mask."""
        torch, timing, pool, arenas = self.torch, self.timing, self.pool, self.arenas
        for p in self.pending:              # speculative batches past the stopping read
            with contextlib.suppress(Exception):
                p.future.result()
        if _on_gpu(self.engine):            # what the device looked like when the last batch was through (BRX_DRIVER_TIMING)
            with contextlib.suppress(Exception):
                free_b, _total_b = torch.cuda.mem_get_info(self.engine.device)
                timing['device_free_gb_at_end'] = free_b / float(1 << 30)
                timing['torch_reserved_gb_at_end'] = torch.cuda.memory_reserved(self.engine.device) / float(1 << 30)
                timing['torch_allocated_gb_at_end'] = torch.cuda.memory_allocated(self.engine.device) / float(1 << 30)
        t0 = time.perf_counter()
        pool.close()
        if arenas is not None:                  # arenas no clone asked for (a job that stopped early, ranks that agreed on fewer engines)
            arenas.release_rest()
            timing['arena_prefetch_thread_seconds'] = arenas.seconds
            if arenas.errors:                   # a prefetch that failed left its clone to allocate by itself: say so (it may be what ran out of memory later)
                timing['arena_prefetch_failures'] = len(arenas.errors)
                if self.shard.rank == 0:
                    print(f'  {len(arenas.errors)} of the {arenas.count} scratch arenas could not be allocated ahead '
                          f'({type(arenas.errors[0]).__name__}: {arenas.errors[0]})', file=self.output)
        if self.gz_engine is not None and self.gz_engine is not self.engine:
            self.gz_engine.close()
        timing['close_engines'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        quiet = unwinding or self.sink_failed_on is not None      # in a multi-rank run a sink's error is reported by raise_outcome
        if self.ring is not None:
            self.ring.flush(reraise=not quiet and not self.ring.defer_errors)
            timing['sink'] = self.ring.sink_seconds
            timing['ring_alloc'] = self.ring.alloc_seconds
        for ring in self.truth_rings.values():
            ring.flush(reraise=not quiet and not ring.defer_errors)
        timing['flush'] = time.perf_counter() - t0
        timing['retries'] = sum(getattr(e, 'retries', 0) for e in pool.engines if e is not None)
        timing['device_batch_seconds_avg'] = pool.job_seconds / max(pool.job_count, 1.0)
        timing['wait_for_engine'] = pool.wait_engine_seconds
        timing['engines'] = len(pool.engines)
        timing['run_batches_seconds'] = time.perf_counter() - self.t_job
        timing['create_clones_thread_seconds'] = pool.create_seconds
        if pool.create_errors and self.shard.rank == 0:
            print(f'\n  {len(pool.create_errors)} of the {len(pool.engines) - 1} extra batch engines could not be created '
                  f'({pool.create_errors[0]}): the job ran on fewer', file=self.output)

    def raise_outcome(self):
        """The ways out other than a count: this rank's own sink, another rank's sink, no fragment, a read beyond the GPU path's limits."""
        for ring in (self.ring, *self.truth_rings.values()):      # this rank's own sink, then its own PAF, SAM and BAM files
            if ring is not None and ring.error is not None and (self.sink_failed_on is not None or ring.defer_errors):
                raise ring.error
        if self.sink_failed_on is not None:
            sys.exit(f'Error: the output of rank {self.sink_failed_on} failed; every rank stopped at the same batch')
        if self.fatal:
            sys.exit(NOFRAG_MESSAGE)
        if self.bad_read is not None:
            sys.exit(f'Error: read {self.bad_read} exceeded an internal limit of the GPU path (status bits in its statistics); '
                     'no output was written for it or any later read')


SORTED_FRAME_MAGIC = 0x4458524244544f53      # the word a frame of --truth-bam-sorted begins with: the sink's check that it reads frames


def sorted_frame(torch, part, keep):
    """What a batch leaves for --truth-bam-sorted: the BAM records of this rank's first `keep` reads behind a frame of 64-bit words -- the
    magic, the reads, the records' bytes, then every read's bytes.  The sink finds the frames one behind the other in the bytes it was
    given, however the ring or the collection to rank 0 cut or joined them.  None: nothing to keep."""
    if part is None or keep == 0:
        return None
    data, off, _ = part
    raw = int(off[keep])
    words = np.concatenate(([SORTED_FRAME_MAGIC, keep, raw], np.diff(off[:keep + 1].astype(np.int64)))).astype('<u8')
    head = torch.from_numpy(words.view(np.uint8).copy()).to(data.device)
    return torch.cat([head, data[:raw]])


def expected_error_rate(identities):
    """Mean errors per base of the job's identity law (beta: 1 - mean; qscore-normal: E[10^(-q / 10)]): what the traceback stores of
    a batch grow with (engine.presize)."""
    if identities.type == 'beta':
        return min(max(1.0 - float(identities.mean), 0.0), 1.0)
    sigma = float(identities.stdev) * math.log(10.0) / 10.0
    return min(10.0 ** (-float(identities.mean) / 10.0) * math.exp(0.5 * sigma * sigma), 1.0)


class _PartsLog(object):
    """PREFIX.<rank>.parts (and .zparts): a line per batch once the batch's bytes have gone through the sink.  batch() is called by the
    consumer thread in batch order, wrote() by the ring's writer thread after every write of the sink; a batch's bytes are written
    by writes of its own (the ring is handed one batch at a time), so when the bytes written reach a batch's end the sink's output
    counter stands at the end of that batch's last gzip member."""

    def __init__(self, parts_file, zparts_file=None, sink_bytes_out=None):
        self.parts_file, self.zparts_file, self.sink_bytes_out = parts_file, zparts_file, sink_bytes_out
        self.lock = threading.Lock()
        self.ends = collections.deque()
        self.issued = self.written = self.z_before = 0

    def batch(self, n):
        with self.lock:
            self.parts_file.write(f'{n}\n')
            self.issued += int(n)
            self.ends.append(self.issued)
            self._settle()

    def wrote(self, n):
        with self.lock:
            self.written += int(n)
            self._settle()

    def _settle(self):
        while self.ends and self.written >= self.ends[0]:
            self.ends.popleft()
            if self.zparts_file is not None:
                z = int(self.sink_bytes_out())
                self.zparts_file.write(f'{z - self.z_before}\n')
                self.z_before = z


class _Outputs(object):
    """Where a rank's bytes go (open_outputs): `write` to rank 0's stdout (through --gzip's sink if asked for); with --output-shards
    `local_write` and `local_parts`, this rank's own file and parts log (None where not in use); `truth_write`, {kind: the write of this
    rank's --truth-<kind> file}; `depth`, this rank's --truth-depth file (a _DepthFile, to be finished when the job has ended);
    `sorted_bam`, this rank's --truth-bam-sorted pair of files (a _SortedBamFile, finished the same way)."""
    local_write = local_parts = depth = sorted_bam = None

    def __init__(self, sink):
        self.sink, self.files, self.bam_files, self.truth_write = sink, [], [], {}

    def write(self, part):
        if self.sink is not None:
            self.sink.write(memoryview(part))
        else:                                   # a text-only stdout (e.g. captured in tests)
            sys.stdout.write(bytes(part).decode('latin-1'))

    def flush(self):
        if self.sink is not None and hasattr(self.sink, 'flush'):
            self.sink.flush()

    def close(self):
        from .output import BGZF_EOF
        for f in self.bam_files:                # the block that tells a reader the file is whole
            with contextlib.suppress(OSError):
                f.write(BGZF_EOF)
        for f in self.files:
            f.close()


def open_outputs(args, shard, engine, stdout, pref=None):
    """The sinks of one job.  Exits where the options exclude each other or, agreed between the ranks, where a rank cannot open its files."""
    sink = stdout if stdout is not None else getattr(sys.stdout, 'buffer', None)
    gzip_level = getattr(args, 'gzip_level', None)
    device_gzip = bool(getattr(args, 'gzip_device', False))
    if device_gzip and gzip_level is not None:
        sys.exit('Error: --gzip and --gzip-device exclude each other')
    if gzip_level is not None and sink is not None and shard.rank == 0:
        from .output import GzipSink
        sink = GzipSink(sink, gzip_level)          # multi-threaded gzip members (libbrx_host.so)
    outs = _Outputs(sink)
    # --output-shards PREFIX: every rank writes PREFIX.<rank>.fastq[.gz] itself (and the bytes per batch to PREFIX.<rank>.parts), so that N ranks
    # leave through N PCIe links and N files instead of rank 0's one of each (simulate.py:77-82 is one print loop).  .parts counts what the rank handed
    # to its sink per batch: FASTQ text (also with --gzip, whose .zparts holds the same batches' compressed bytes), compressed bytes with --gzip-device.
    prefix = getattr(args, 'output_shards', None)
    if prefix:
        open_error = zparts_file = None
        try:                                # a rank that cannot open its files must not leave the others in their first exchange
            shard_file = open(f'{prefix}.{shard.rank}.fastq' + ('.gz' if device_gzip or gzip_level is not None else ''), 'wb')
            outs.files.append(shard_file)
            parts_file = open(f'{prefix}.{shard.rank}.parts', 'w')
            outs.files.append(parts_file)
            if gzip_level is not None:
                zparts_file = open(f'{prefix}.{shard.rank}.zparts', 'w')
                outs.files.append(zparts_file)
        except OSError as ex:
            open_error = ex
        failed = shard.gather_word(1 if open_error else 0)
        if any(failed):
            outs.close()
            shard.finish()
            sys.exit(f'Error: could not open the output shards of rank(s) {[r for r, x in enumerate(failed) if x]}'
                     + (f': {open_error}' if open_error else ''))
        shard_sink = shard_file
        if gzip_level is not None:
            from .output import GzipSink
            shard_sink = GzipSink(shard_file, gzip_level)
        log = _PartsLog(parts_file, zparts_file, (lambda: shard_sink.bytes_out) if zparts_file is not None else None)

        def local_write(part):
            shard_sink.write(memoryview(part))
            log.wrote(len(part))
        outs.local_write, outs.local_parts = local_write, log.batch
    # --truth-paf PATH: the truth alignments of the reads (brx_emit_paf), plain text; with --output-shards every rank writes PATH.<rank>, the
    # records of the reads of its own FASTQ file.  --truth-sam PATH: the same as SAM (brx_emit_sam), the same files; each begins with the
    # header, which depends on the reference alone.  --truth-bam PATH: the same header and records as BAM; the host writes the header's BGZF
    # blocks and, on closing, the EOF block
    from .output import bam_header, bgzf_host
    # kind; what every rank makes of the reference first (ValueError: an exit all ranks take alike); what the file begins with, made of that
    for kind, checked, header in (('paf', None, None), ('sam', None, sam_header), ('bam', bam_header, bgzf_host)):
        path = getattr(args, 'truth_' + kind, None)
        if not path:
            continue
        if not hasattr(engine, 'emit_truth_device'):
            shard.finish()
            sys.exit(f'Error: --truth-{kind} needs the GPU engine')
        first = pref
        if checked is not None:
            try:
                first = checked(pref)
            except ValueError as ex:           # every rank alike: it depends on the reference alone
                shard.finish()
                sys.exit(f'Error: --truth-{kind}: {ex}')
        if prefix or shard.rank == 0:
            f = open(f'{path}.{shard.rank}' if prefix else path, 'wb')
            outs.files.append(f)
            if kind == 'bam':
                outs.bam_files.append(f)
            if header is not None:
                f.write(header(first))
            outs.truth_write[kind] = f.write
    # --truth-depth PATH: the coverage of the reference by the same records as bedGraph text.  The file's sink keeps the batches' events
    # (16 bytes per record, the same ring and the same cut as the other truth files) and writes the file when the job has ended (_DepthFile);
    # with --output-shards every rank writes PATH.<rank>, the coverage by the reads of its own FASTQ file
    path = getattr(args, 'truth_depth', None)
    if path:
        if not hasattr(engine, 'depth_bedgraph'):
            shard.finish()
            sys.exit('Error: --truth-depth needs the GPU engine')
        problem = depth_limits(pref)
        if problem:                            # every rank alike: it depends on the reference alone
            shard.finish()
            sys.exit(f'Error: --truth-depth: {problem}')
        if prefix or shard.rank == 0:
            f = open(f'{path}.{shard.rank}' if prefix else path, 'wb')
            outs.files.append(f)
            zipped = gzip_level is not None or device_gzip
            if zipped:
                from .output import GzipSink
            outs.depth = _DepthFile(GzipSink(f, gzip_level if gzip_level is not None else 6) if zipped else f)
            outs.truth_write['depth'] = outs.depth.write
    # --truth-bam-sorted PATH: the records of --truth-bam in coordinate order and PATH.bai, their index.  The sink keeps the batches' raw
    # records (the same ring and the same cut as the other truth files) and writes both files when the job has ended (_SortedBamFile);
    # with --output-shards every rank writes PATH.<rank> and PATH.<rank>.bai, the records of the reads of its own FASTQ file
    path = getattr(args, 'truth_bam_sorted', None)
    if path:
        if not hasattr(engine, 'bam_sort'):
            shard.finish()
            sys.exit('Error: --truth-bam-sorted needs the GPU engine')
        try:                                   # every rank alike: it depends on the reference alone
            bam_header(pref, b'')
        except ValueError as ex:
            shard.finish()
            sys.exit(f'Error: --truth-bam-sorted: {ex}')
        long_ones = [str(n) for n, x in zip(pref.names, pref.lengths) if int(x) >= BAI_MAX_LENGTH]
        if long_ones:
            shard.finish()
            sys.exit(f'Error: --truth-bam-sorted: contig {long_ones[0]} is too long for a BAI index')
        if prefix or shard.rank == 0:
            outs.sorted_bam = _SortedBamFile(f'{path}.{shard.rank}' if prefix else path, pref)
            outs.truth_write['bam_sorted'] = outs.sorted_bam.write
    return outs


DEPTH_MAX_CONTIGS, DEPTH_MAX_LENGTH = 2 ** 24, 2 ** 39      # include/brx.h, BRX_DEPTH_EVENT: 24 bits of contig index, 39 of position


def depth_limits(pref):
    """Why --truth-depth cannot take this reference (None: it can): an event holds 24 bits of contig index and 39 of position."""
    if len(pref.names) >= DEPTH_MAX_CONTIGS:
        return f'{len(pref.names)} contigs, an event of brx_emit_depth holds fewer than 2^24'
    long_ones = [str(n) for n, x in zip(pref.names, pref.lengths) if int(x) >= DEPTH_MAX_LENGTH]
    if long_ones:
        return f'contig {long_ones[0]} has 2^39 or more bases, more than an event of brx_emit_depth holds'
    return None


class _DepthFile(object):
    """The sink of --truth-depth.  `write` (the ring's writer thread) keeps the events of every batch: those of the reads the FASTQ holds,
    cut where the FASTQ is cut, of every rank on rank 0 or with --output-shards this rank's own.  `finish`, called once when the job has
    ended normally, uploads them, has the engine -- still open, its batches done -- make the text (brx_depth_bedgraph) and writes it.
    Events and scratch must fit the device then; a job that does not reach `finish` writes nothing."""

    def __init__(self, sink):
        self.sink, self.parts = sink, []

    def write(self, part):
        self.parts.append(bytes(part))          # the ring's buffer is reused

    def finish(self, engine):
        torch = engine.torch
        events = np.frombuffer(b''.join(self.parts), dtype='<i8')
        self.parts = []
        need = events.nbytes + int(engine.lib.brx_depth_bedgraph_scratch(len(events)))
        try:
            if getattr(engine.device, 'type', 'cpu') == 'cuda':
                torch.cuda.empty_cache()        # the batches' buffers, back to the driver
                if need + 28 * len(events) > torch.cuda.mem_get_info(engine.device)[0]:
                    raise MemoryError
            text = engine.depth_bedgraph(torch.from_numpy(events.copy()).to(engine.device))
        except (MemoryError, getattr(torch, 'OutOfMemoryError', MemoryError)):
            sys.exit(f'Error: --truth-depth: {len(events) // 2} records need {need / 1e9:.1f} GB on the device')
        self.sink.write(memoryview(text.cpu().numpy()))


BAI_MAX_LENGTH = 2 ** 29                    # a BAI index has bins and windows for positions below 2^29
SORTED_SPAN = 8192 * 32768                  # --truth-bam-sorted: bytes of the sorted stream per call of brx_bgzf_device, whole blocks


class _SortedBamFile(object):
    """The sink of --truth-bam-sorted.  `write` (the ring's writer thread) keeps what every batch leaves (sorted_frame): the raw BAM records
    of the reads the FASTQ holds, in host memory, of every rank on rank 0 or with --output-shards this rank's own.  `finish`, called once
    when the job has ended normally, uploads them, has the engine -- still open, its batches done -- sort them (brx_bam_sort), compress
    the sorted stream in spans of whole 32 KB blocks (brx_bgzf_device_off: the blocks do not depend on the spans) and make the index
    (brx_bam_index), and writes PATH and PATH.bai.  The records twice, their table and the scratch must fit the device then; a job that
    does not reach `finish`, or fails in it, leaves neither file."""

    def __init__(self, path, pref):
        self.path, self.pref, self.parts = path, pref, []
        if not os.path.isdir(os.path.dirname(os.path.abspath(path))):      # now, not when the job has run: the other truth files' error
            raise FileNotFoundError(2, 'No such file or directory', path)

    def write(self, part):
        self.parts.append(np.frombuffer(bytearray(part), dtype=np.uint8))      # a copy: the ring's buffer is reused

    def frames(self):
        """(the bytes of every read, the pieces of records) of the frames kept, in the order they came.  The pieces are views of what
        `write` kept -- a frame may begin in one part and end in another --, so the records lie in host memory once."""
        parts, self.parts = self.parts, []
        where = [0, 0]                          # the part and the byte in it that come next

        def take(n):
            got = []
            while n:
                part = parts[where[0]]
                piece = part[where[1]:where[1] + n]
                got.append(piece)
                n -= len(piece)
                where[1] += len(piece)
                if where[1] == len(part):
                    where[:] = [where[0] + 1, 0]
            return got
        lens, pieces = [], []
        while where[0] < len(parts):
            if not len(parts[where[0]]):
                where[0] += 1
                continue
            magic, keep, raw = (int(x) for x in np.concatenate(take(24)).view('<u8'))
            assert magic == SORTED_FRAME_MAGIC, 'a frame of --truth-bam-sorted was expected here'
            lens.append(np.concatenate(take(8 * keep)).view('<u8'))
            pieces += take(raw)
        return (np.concatenate(lens) if lens else np.zeros(0, dtype=np.uint64)), pieces

    def finish(self, engine):
        from .output import BGZF_EOF, bam_header, bgzf_host
        torch = engine.torch
        lens, pieces = self.frames()
        seg_off = np.concatenate(([0], np.cumsum(lens, dtype=np.uint64))).astype(np.uint64)
        n_bytes, n_ref = int(seg_off[-1]), len(self.pref.names)
        need = 2 * n_bytes + int(engine.lib.brx_bam_sort_scratch(n_bytes, len(lens))) + 24 * (n_bytes // 4096 + len(lens) + 64)
        done = []
        try:
            try:
                if getattr(engine.device, 'type', 'cpu') == 'cuda':
                    torch.cuda.empty_cache()        # the batches' buffers, back to the driver
                    if need > torch.cuda.mem_get_info(engine.device)[0]:
                        raise MemoryError
                records = torch.empty(n_bytes, dtype=torch.uint8, device=engine.device)
                at = 0
                for piece in pieces:
                    records[at:at + len(piece)].copy_(torch.from_numpy(piece))
                    at += len(piece)
                ordered, table, n, unmapped = engine.bam_sort(records, seg_off, n_ref, max([int(x) for x in self.pref.lengths] + [1]))
                del records
            except (MemoryError, getattr(torch, 'OutOfMemoryError', MemoryError)):
                n = sum(_count_records(piece) for piece in pieces)
                sys.exit(f'Error: --truth-bam-sorted: {n} records ({n_bytes / 1e9:.1f} GB) need {need / 1e9:.1f} GB on the device')
            del pieces
            head = bgzf_host(bam_header(self.pref, text=sam_header(self.pref, 'SO:coordinate')))
            block_off, total = [], 0
            done.append(self.path)
            with open(self.path, 'wb') as f:
                f.write(head)
                for a in range(0, n_bytes, SORTED_SPAN):
                    blocks, off = engine.bgzf_device(ordered[a:a + SORTED_SPAN], offsets=True)
                    f.write(memoryview(blocks.cpu().numpy()))
                    block_off.append(off[:-1] + np.uint64(total))
                    total += int(off[-1])
                f.write(BGZF_EOF)
            block_off = np.concatenate(block_off + [np.array([total], dtype=np.uint64)])
            index = engine.bam_index(table, n_ref, n_bytes, block_off, len(head))
            done.append(self.path + '.bai')
            with open(self.path + '.bai', 'wb') as f:
                f.write(memoryview(index.cpu().numpy()))
        except BaseException:
            for name in done:                   # neither file, not a part of one
                with contextlib.suppress(OSError):
                    os.remove(name)
            raise


def _count_records(piece):
    """The BAM records of a piece of whole records, by their block_size chain (the error path of _SortedBamFile.finish only)."""
    n, at = 0, 0
    while at + 4 <= len(piece):
        at += 4 + int(piece[at:at + 4].view('<u4')[0])
        n += 1
    return n


def sam_header(pref, order='SO:unsorted\tGO:query'):
    """The @ lines of a --truth-sam file: the contigs in reference order under the names the records use.  No CL: field and nothing
    else of the run: the file does not depend on streams, batch sizes or ranks.  `order`: what @HD says of the records' order."""
    from .version import __version__
    lines = ['@HD\tVN:1.6\t' + order]
    lines += [f'@SQ\tSN:{name}\tLN:{int(length)}' for name, length in zip(pref.names, pref.lengths)]
    lines.append(f'@PG\tID:badread_amd\tPN:badread_amd\tVN:{__version__}')
    return ('\n'.join(lines) + '\n').encode()


# ---------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------
def simulate(args, output=sys.stderr, engine=None, stdout=None, shard=None):
    """Same contract as badread.simulate.simulate(args, output): FASTQ to stdout, the rest to `output`."""
    marks = [('enter_simulate', time.time())]           # wall-clock marks of the start-up (BRX_DRIVER_TIMING: tools/cli_30x.sh)

    def mark(name):
        marks.append((name, time.time()))
    shard = shard or Shard.from_env()
    quiet = _Null() if shard.rank != 0 else output
    print_intro(quiet)
    seed = args.seed if args.seed is not None else int.from_bytes(os.urandom(7), 'little')
    if shard.world > 1 and args.seed is None:
        seed = _broadcast_seed(shard, seed)
    random.seed(seed)
    host_rng = np.random.RandomState(seed % (2 ** 32))
    pref = load_packed_reference(args.reference, quiet)
    mark('reference_loaded')
    frag_lengths = FragmentLengths(args.mean_frag_length, args.frag_length_stdev, quiet)
    depths = adjust_depths(pref, frag_lengths, args.small_plasmid_bias, host_rng)
    identities = Identities(args.mean_identity, args.identity_stdev, args.max_identity, quiet)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    mark('engine_created')
    # the genome goes to the device BEFORE the arenas are asked for (round 6): the allocations of 200+ GB hold the runtime's lock the
    # upload would otherwise wait for -- 0.2 s of copy became 2-6 s behind them right after another process (profiles/r05i, r05k)
    _, cum_weight = pref.contig_weights(depths)
    engine.set_reference(pref, cum_weight)
    mark('reference_on_device')
    truth = TruthSpec.from_args(args)
    # the job's arenas from now on, beside everything below (models, tables, the first batch): _ArenaPrefetch
    arenas = _ArenaPrefetch.for_job(engine, get_target_size(pref.n_bases, args.quantity), float(args.mean_frag_length),
                                    expected_error_rate(identities), getattr(args, 'gpu_streams', None) or DEFAULT_IN_FLIGHT, shard.world,
                                    truth=truth)
    # a model file that is not in the cache is aligned (align_kmers, error_model.py:179-229) on THIS engine
    error_model = ErrorModel(args.error_model, quiet, aligner=lambda qs, ts: engine.align_batch(qs, ts)[0])
    qscore_model = QScoreModel(args.qscore_model, quiet)
    mark('models_loaded')
    print_glitch_summary(args.glitch_rate, args.glitch_size, args.glitch_skip, quiet)
    start_rate, start_amount = adapter_parameters(args.start_adapter)
    end_rate, end_amount = adapter_parameters(args.end_adapter)
    random_start, random_end = build_random_adapters(args)
    print_adapter_summary(start_rate, start_amount, args.start_adapter_seq, end_rate, end_amount,
                          args.end_adapter_seq, random_start, random_end, quiet)
    print_other_problem_summary(args, quiet)
    target_size = get_target_size(pref.n_bases, args.quantity)
    print(f'\nTarget read set size: {target_size:,} bp\n', file=quiet)

    engine.set_error_model(error_model.tables())
    engine.set_qscore_model(qscore_model.tables())
    engine.set_params(sim_params_from_args(args, frag_lengths, identities, start_rate, start_amount,
                                           end_rate, end_amount))
    mark('tables_on_device')
    outs = open_outputs(args, shard, engine, stdout, pref)
    try:
        try:
            result = run_batches(engine, seed, target_size, float(args.mean_frag_length), outs.write, quiet, shard,
                                 in_flight=getattr(args, 'gpu_streams', None) or DEFAULT_IN_FLIGHT, device_gzip=bool(getattr(args, 'gzip_device', False)),
                                 local_write=outs.local_write, local_parts=outs.local_parts, expected_error=expected_error_rate(identities),
                                 arenas=arenas, truth=truth, truth_write=outs.truth_write)
            if outs.depth is not None:      # the job has ended normally: the coverage of the events it kept, on the engine that is still open
                outs.depth.finish(engine)
            if outs.sorted_bam is not None:  # the same for the records --truth-bam-sorted kept
                t_sorted = time.perf_counter()
                outs.sorted_bam.finish(engine)
                run_batches.last_timing['truth_bam_sorted_finish'] = time.perf_counter() - t_sorted
        finally:
            outs.close()
    except (SystemExit, OSError):
        shard.finish()                      # exits every rank takes at the same batch: NOFRAG, a bad read, a failed sink
        raise
    except BaseException:
        # Not an exit the ranks take together (an engine error, a sink raising something else: ADVICE r4): the peers are in, or on
        # their way to, an exchange this rank will never join.  Leave without meeting them -- under torchrun the failing rank takes
        # the job down; a peer left alone fails in its exchange instead of waiting for the backend's timeout.
        shard.abandon()
        raise
    shard.finish()
    outs.flush()
    if os.environ.get('BRX_DRIVER_TIMING') and shard.rank == 0:      # seconds of the consumer thread per activity + rate, for tools/cli_30x.sh
        t = dict(run_batches.last_timing)
        t['bases'], t['reads'] = result[1], result[0]
        print('driver_timing ' + repr({k: round(float(v), 3) for k, v in t.items()}), file=sys.stderr)
        mark('done')
        t0 = float(os.environ.get('BRX_T0', marks[0][1]))      # epoch seconds at which the shell started the command, if it says so
        steps = {'interpreter_and_imports': marks[0][1] - t0}
        steps.update({name: at - before for (name, at), (_, before) in zip(marks[1:], marks[:-1])})
        print('startup_timing ' + repr({k: round(float(v), 3) for k, v in steps.items()}), file=sys.stderr)
    return result


class _Null(object):
    def write(self, *_):
        return 0

    def flush(self):
        pass


def _broadcast_seed(shard, seed):
    import torch
    t = torch.tensor([seed], dtype=torch.int64, device=shard._device())
    shard.dist.broadcast(t, src=0)
    return int(t.item())


# ---------------------------------------------------------------------------------------------
# sequence_fragment: the narrow Python boundary (simulate.py:256-358)
# ---------------------------------------------------------------------------------------------
_seq_engine_state = {}


def _fragment_alphabet(fragment):
    """ACGT -> 0..3, N -> 4, other symbols of this fragment -> 5.. (all treated as 'not in the model')."""
    sym = bytearray(b'ACGTN' + b'N' * 11)
    lut = np.full(256, 4, dtype=np.uint8)
    for code, ch in enumerate(b'ACGT'):
        lut[ch] = code
    raw = np.frombuffer(fragment.encode('latin-1'), dtype=np.uint8)
    nxt = 5
    for b in np.unique(raw):
        if chr(b) not in 'ACGTN':
            if nxt < 16:
                lut[b], sym[nxt] = nxt, b
                nxt += 1
    return lut[raw], np.frombuffer(bytes(sym), dtype=np.uint8)


def sequence_fragment(fragment, target_identity, error_model, qscore_model, engine=None, seed=None, read_index=0):
    """
    Drop-in for badread.simulate.sequence_fragment: returns (seq, quals, actual_identity,
    identity_by_qscores).  Runs brx_sequence_fragments on a batch of one; the random streams are
    keyed by `seed` (default: 64 bits from Python's `random`, so random.seed() still fixes the result).
    """
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    # (re)configure the engine unless it holds exactly these tables already: the engine remembers what it was last
    # given, so a simulate() or a direct set_* call in between is noticed
    held = getattr(engine, '_configured', {})
    if held.get('em') is not error_model.tables():
        engine.set_error_model(error_model.tables())
    if held.get('qm') is not qscore_model.tables():
        engine.set_qscore_model(qscore_model.tables())
    _seq_engine_state['keep'] = (error_model, qscore_model)
    if seed is None:
        seed = random.getrandbits(64)
    if len(fragment) == 0:
        return '', '', 0.0, 0.0
    codes, sym = _fragment_alphabet(fragment)
    res, stats = engine.sequence_fragments(seed, read_index, [codes], [float(target_identity)])
    seq_codes, quals = res[0]
    st = stats[0]
    seq = sym[seq_codes].tobytes().decode('latin-1')
    n_cols, padded_len = int(st['n_cols']), int(st['padded_len'])
    actual_identity = int(st['n_match']) / n_cols if n_cols else 0.0
    # identity_by_qscores averages over the PADDED read, like get_qscores (qscore_model.py:71-73)
    identity_by_qscores = 1.0 - float(st['qerr_sum']) / padded_len if padded_len else 0.0
    return seq, quals.tobytes().decode('latin-1'), actual_identity, identity_by_qscores


assert settings.ALIGNMENT_INTERVAL == 25 and settings.ALIGNMENT_SIZE == 1000     # hard-coded in csrc/brx_kernels.h
