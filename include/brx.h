/*
 * include/brx.h -- C-ABI of libbrx_hip.so, the MI355X-native replacement for Badread's per-read
 * hot path (badread/simulate.py:63-86 -> build_fragment :91, sequence_fragment :256,
 * qscore_model.get_qscores qscore_model.py:32, and the edlib.align calls they make).
 *
 * Badread has no plugin/FFI interface of its own (it is pure Python; its one native dependency is
 * the `edlib` wheel).  This header therefore declares the boundary a maintainer would bind with
 * ctypes from badread/simulate.py -- see INTEGRATION.md for the stub.  Rules:
 *   - plain C, plain pointers and sizes, no torch / HIP types in any signature;
 *   - every pointer named d_* is a DEVICE pointer owned by the caller (the Python host holds them
 *     as PyTorch-ROCm tensors); the library never frees caller memory and never allocates output;
 *   - scratch is one caller-provided device arena; if it is too small a call fails with
 *     BRX_E_SCRATCH and brx_scratch_needed() tells how much the same call wants;
 *   - no exceptions cross the ABI: int status + brx_last_error();
 *   - a context belongs to one device and one host thread; work is enqueued on the caller's
 *     HIP stream (pass torch.cuda.current_stream().cuda_stream, or NULL for the default stream).
 *
 * The same descriptor structs (with HOST pointers) parameterise the CPU oracle under oracle/,
 * which is test infrastructure only.
 */
#ifndef BRX_H
#define BRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status codes */
enum {
    BRX_OK = 0,
    BRX_E_ARG = -1,        /* bad argument                                                    */
    BRX_E_HIP = -2,        /* a HIP runtime call failed (message in brx_last_error)            */
    BRX_E_SCRATCH = -3,    /* scratch arena too small; see brx_scratch_needed()                */
    BRX_E_OUTPUT = -4,     /* output buffer too small; see brx_output_needed()                 */
    BRX_E_NOFRAG = -5,     /* a read failed 1000 times to draw a fragment (simulate.py:159-165) */
    BRX_E_STATE = -6,      /* reference / models / params not set                             */
    BRX_E_INTERNAL = -7    /* a kernel flagged an internal inconsistency                      */
};

/* per-read status bits written to brx_read_stats.status */
enum {
    BRX_RS_NOFRAG = 1u,       /* get_fragment gave up after 1000 tries                        */
    BRX_RS_TOO_MANY_SEGS = 2u,/* more than 4096 base segments in one read AND the batch's overflow lists used up (see brx_kernels.h) */
    BRX_RS_BAND = 4u,         /* alignment failed: score above its proven bound (bug) or a band of more than 7.3 M rows */
    BRX_RS_QMISS = 8u,        /* qscore fallback reached a 1-op cigar absent from the model   */
    BRX_RS_EMPTY = 16u        /* read trimmed to zero length: skipped, like simulate.py:70-71  */
};

/* base codes: 0..3 = A,C,G,T; 4 = N; 5..15 = other symbols of this reference (sym[] gives ASCII) */
#define BRX_CODE_N 4

/* ------------------------------------------------------------------ reference (misc.py:122-153) */
typedef struct {
    uint64_t base_off;     /* index of the contig's first base in the packed array             */
    uint32_t length;       /* bases                                                            */
    uint32_t flags;        /* bit0 circular, bit1 hairpin_left, bit2 hairpin_right             */
    uint32_t name_off;     /* into names[]                                                     */
    uint32_t name_len;
} brx_contig;

typedef struct {           /* run of non-ACGT bases: packed coordinates [start,end) hold `code` */
    uint64_t start, end;
    uint32_t code;
    uint32_t pad_;
} brx_exception;

typedef struct {
    const uint32_t *d_packed;        /* 2-bit bases, 16 per word, base g at bits 2*(g%16) of word g/16 */
    uint64_t n_bases;
    const brx_contig *d_contigs;     /* [n_contigs]                                              */
    uint32_t n_contigs;
    const brx_exception *d_exceptions; /* sorted by start, non-overlapping                        */
    uint32_t n_exceptions;
    const uint8_t *d_names;          /* concatenated contig names (ASCII)                        */
    uint32_t names_len;
    uint8_t sym[16];                 /* code -> ASCII                                            */
    uint8_t comp[16];                /* code -> complement code (misc.py:56-67)                  */
    const double *d_cum_weight;      /* [n_contigs] running sum of depth*length (simulate.py:118-121) */
    double total_weight;
} brx_reference;

/* ------------------------------------------------------------------ error model (error_model.py:86-229)
 * Flattened by the host from the `kmer,p;alt,p;...` file after align_kmers():
 *   row r = 2-bit value of the k-mer (first base most significant); alts of row r are
 *   [row_off[r], row_off[r+1]); an absent row (error_model.py:143) has an empty range.
 *   thr[a]   cumulative probability of alts row_off[r]..a as a 32-bit fixed-point threshold:
 *            alt a is chosen iff it is the first with draw < thr[a]; if none is and the row's last
 *            thr is 0xFFFFFFFF the last alt is chosen (rows with sum p >= 1), otherwise the
 *            remainder goes to add_one_random_change (error_model.py:151-158).
 *   desc[a]  offset o into pool: pool[o], pool[o+1] = bitmask of positions whose string differs
 *            from the k-mer base; pool[o+2 .. o+2+k) = per-position string lengths;
 *            then the alt's characters (base codes), in order.
 *   self_thr[r] = thr of alt 0 (the unchanged k-mer), 0 for an absent row: one compare rejects
 *            the ~93 % of draws that leave the k-mer unchanged (simulate.py:300).
 * pool[0..528) is a fixed preamble used for add_one_random_change results:
 *   pool[c] = c for c<16 (single chars), pool[16 + 2*(16x+y)] = x,y (all two-char strings).     */
#define BRX_POOL_PREAMBLE 528
typedef struct {
    int32_t k;                  /* k-mer size; 1 for the 'random' model                          */
    int32_t type;               /* 0 = 'random' (no table), 1 = table                            */
    uint32_t n_rows;            /* 4^k                                                           */
    uint32_t n_alts;
    uint32_t pool_len;
    uint32_t pad_;
    const uint32_t *d_row_off;  /* [n_rows+1]                                                    */
    const uint32_t *d_self_thr; /* [n_rows]                                                      */
    const uint32_t *d_thr;      /* [n_alts]                                                      */
    const uint32_t *d_desc;     /* [n_alts]                                                      */
    const uint8_t *d_pool;      /* [pool_len]                                                    */
    /* The same table laid out for ONE load per step of the lookup (round 4; required when type = 1).  The proposal rounds of
     * the mutate loop are chains of dependent L2 round trips: self_thr -> row_off -> five probes of a binary search -> desc ->
     * pool was ten deep; with these it is three (row entry -> a block of eight thresholds -> the alternative's descriptor).
     *   d_rowx[2 r], [2 r + 1] = self_thr[r], row_off[r] for r <= n_rows (self_thr[n_rows] = 0): a 16-byte load at row r
     *            also holds row_off[r + 1]; 16 bytes of padding behind the last pair.
     *   d_thr    must be readable 8 entries past n_alts (zeros): thresholds are scanned in blocks of eight.
     *   d_altx[4 a .. 4 a + 3] = desc[a]; diff | flags << 16; lengths of positions 0-7 in 4 bits each; 0.
     *            flags bit 0: a length above 15 or k > 8 -- the kernel then reads the lengths from the pool.
     * badread_amd.error_model.derive_lookup_tables builds both from the arrays above.                */
    const uint32_t *d_rowx;     /* [2 (n_rows + 1) + 4]                                          */
    const uint32_t *d_altx;     /* [4 n_alts]                                                    */
} brx_error_model;

/* ------------------------------------------------------------------ qscore model (qscore_model.py:178-287)
 * A cigar window of w non-D ops (w odd) is keyed as
 *   key = (w << 56) | sum_i op_i << (bits*i)   with op codes 0 '=',1 'X',2 'I' in 2 bits and the
 *   D-run length between op i and op i+1 in `gap_bits` bits placed after op i
 * (see brx_qs_key in badread_amd/csrc).  A run longer than the field holds is encoded as all-ones,
 * which no table row uses, so it misses and falls back exactly like the reference's string lookup
 * (qscore_model.py:278-286).  Open-addressing hash: slot = hash(key) & (hash_size-1), linear probe,
 * empty slot = key ~0.                                                                           */
typedef struct {
    int32_t k;                  /* kmer_size: largest non-D window length in the model (odd)      */
    int32_t gap_bits;           /* 3 or 4                                                        */
    uint32_t hash_size;         /* power of two                                                  */
    uint32_t n_rows;
    uint32_t n_entries;
    uint32_t pad_;
    const uint64_t *d_hash_key; /* [hash_size]                                                   */
    const uint32_t *d_hash_row; /* [hash_size]                                                   */
    const uint32_t *d_row_off;  /* [n_rows+1] into thr/score                                     */
    const uint32_t *d_thr;      /* [n_entries] cumulative 32-bit thresholds; first draw < thr wins, else last */
    const uint8_t *d_score;     /* [n_entries] phred score                                       */
} brx_qscore_model;

/* ------------------------------------------------------------------ simulation parameters
 * The derived fields argparse validation leaves on `args` (badread/__main__.py:239-313).         */
typedef struct {
    /* fragment lengths, fragment_lengths.py:47-64 */
    double frag_mean, frag_stdev, gamma_k, gamma_t;
    /* identities, identities.py:76-103.  mode 0: constant id_max; 1: id_max*beta(id_a,id_b);
       2: 1-10^(-normal(id_a,id_b)/10) */
    int32_t identity_mode;
    int32_t pad0_;
    double id_a, id_b, id_max;
    /* adapters, simulate.py:361-387: rates/amounts as fractions */
    double start_rate, start_amount, end_rate, end_amount;
    const uint8_t *d_start_adapter;   /* base codes */
    const uint8_t *d_end_adapter;
    uint32_t start_adapter_len, end_adapter_len;
    /* problems: fractions (simulate.py:101,172-173) */
    double junk_rate, random_rate, chimera_rate;
    /* glitches (simulate.py:459-482) */
    double glitch_rate, glitch_size, glitch_skip;
} brx_sim_params;

/* ------------------------------------------------------------------ per-read results */
typedef struct {
    uint32_t status;           /* BRX_RS_* bits                                                 */
    uint32_t frag_len;         /* error-free_length: len(fragment) before padding (simulate.py:74) */
    uint32_t seq_len;          /* length= : trimmed read length                                 */
    uint32_t n_cols;           /* columns of the final alignment (pads included)                */
    uint32_t n_match;          /* '=' columns: read_identity = n_match / n_cols (misc.py:228-240) */
    uint32_t padded_len;       /* bases of the read before trimming the pads (what get_qscores scored);
                                  edit distance = n_cols - n_match                                */
    uint32_t loop_count;       /* k-mer draws consumed by the mutate loop                       */
    uint32_t change_count;     /* positions changed                                             */
    uint32_t n_alignments;     /* in-loop identity alignments (simulate.py:325-346)             */
    uint32_t rec_len;          /* bytes of this read's FASTQ record (0 if skipped)              */
    uint64_t rec_off;          /* offset of the record in the output buffer                     */
    double target_identity;
    double qerr_sum;           /* sum over read bases of 10^(-q/10) (qscore_model.py:71-73)     */
} brx_read_stats;

typedef struct brx_ctx brx_ctx;

/* ------------------------------------------------------------------ entry points */
int brx_create(int device_id, brx_ctx **out);
void brx_destroy(brx_ctx *ctx);
const char *brx_last_error(const brx_ctx *ctx);   /* ctx == NULL: why the last brx_create failed */
const char *brx_version(void);

int brx_set_reference(brx_ctx *ctx, const brx_reference *ref);
int brx_set_error_model(brx_ctx *ctx, const brx_error_model *em);
int brx_set_qscore_model(brx_ctx *ctx, const brx_qscore_model *qm);
int brx_set_params(brx_ctx *ctx, const brx_sim_params *p);
int brx_set_scratch(brx_ctx *ctx, void *d_scratch, size_t bytes);
size_t brx_scratch_needed(const brx_ctx *ctx);
size_t brx_output_needed(const brx_ctx *ctx);

/* replaces the body of the `while total_size < target_size` loop (simulate.py:63-86) for reads
 * [first_read, first_read+n_reads): FASTQ records are written back-to-back in read order into
 * d_out; d_stats[i] describes read first_read+i.  *out_bytes receives the bytes written.
 * Synchronous with respect to the host on return (small size read-backs happen inside).         */
int brx_simulate_batch(brx_ctx *ctx, uint64_t seed, uint64_t first_read, uint32_t n_reads,
                       uint8_t *d_out, size_t out_cap, brx_read_stats *d_stats,
                       size_t *out_bytes, void *hip_stream);

/* replaces badread.simulate.sequence_fragment (simulate.py:256-358) for caller-supplied fragments:
 * fragment i is d_frags[frag_off[i] .. frag_off[i+1]) as base codes, with target identity
 * d_target[i]; read index first_read+i keys the random streams.  Output per fragment i:
 * sequence codes then phred+33 bytes, each seq_len long, at d_out + stats[i].rec_off.           */
int brx_sequence_fragments(brx_ctx *ctx, uint64_t seed, uint64_t first_read, uint32_t n_frags,
                           const uint8_t *d_frags, const uint64_t *d_frag_off,
                           const double *d_target, uint8_t *d_out, size_t out_cap,
                           brx_read_stats *d_stats, size_t *out_bytes, void *hip_stream);

/* replaces edlib.align(query, target, task='path') (simulate.py:330,340; qscore_model.py:37;
 * error_model.py:202) for a batch: pair i aligns query d_queries[q_off[i]..q_off[i+1]) against
 * target d_targets[t_off[i]..t_off[i+1]) (any byte alphabet; equality is byte equality).
 * k_hint[i] >= 0 is a proven upper bound on the distance (no band search), -1 = unknown (band
 * doubling from 64, like edlib).  Writes the edit distance to d_dist[i], the number of alignment
 * columns to d_ncols[i], the number of '=' columns to d_nmatch[i] and, if d_ops != NULL, the
 * per-column ops (0 '=',1 'X',2 'I',3 'D', forward order; 'I' = byte present in the query only)
 * at d_ops + ops_off[i] (capacity qlen+tlen).                                                    */
int brx_align_batch(brx_ctx *ctx, uint32_t n_pairs,
                    const uint8_t *d_queries, const uint64_t *d_q_off,
                    const uint8_t *d_targets, const uint64_t *d_t_off, const int32_t *d_k_hint,
                    int32_t *d_dist, uint32_t *d_ncols, uint32_t *d_nmatch,
                    uint8_t *d_ops, const uint64_t *d_ops_off, void *hip_stream);

/* Device time (ms) of each pipeline stage of the last brx_simulate_batch / brx_sequence_fragments
 * call, from HIP events recorded on the launch stream immediately before and after the stage's
 * kernels (host work between stages is not included):
 *   PLAN    k_plan_count, k_scan_plan, k_plan_fill (includes one small size read-back)
 *   BUILD   k_build (+ k_copy_frags), k_order
 *   MUTATE  k_mut_fill, k_mut_lanes, k_mutate_seg, k_mut_epilogue (+ k_mutate for overflow reads) -- or, under BRX_MUTATE_PASSES=1,
 *           all passes of {k_mut_apply, k_mut_post, k_pass_lists, k_win_lane, k_win_wave} including the host round trips between
 *           them; brx_last_mutate_passes() gives the count of launches / passes
 *   SCAN    k_scan_mut
 *   FINAL   the whole final stage: k_fin_join, then k_fin_align<...> for every band class (two streams) +
 *           k_fin_qscore, one set of launches per scratch chunk (and per phase: brx_last_window_misses)
 *   EMIT    k_recsize, k_scan_rec, k_emit, k_stats (includes one small size read-back)
 *   ALIGN1  average duration of ONE launch of k_fin_align<1,1,1> (the largest single kernel) over the chunks
 *   QSCORE  average duration of ONE launch of k_fin_qscore for the one- and two-word band classes over the chunks */
enum { BRX_STAGE_PLAN = 0, BRX_STAGE_BUILD = 1, BRX_STAGE_MUTATE = 2, BRX_STAGE_SCAN = 3,
       BRX_STAGE_FINAL = 4, BRX_STAGE_EMIT = 5, BRX_STAGE_ALIGN1 = 6, BRX_STAGE_QSCORE = 7, BRX_STAGE_COUNT = 8 };
int brx_last_stage_ms(const brx_ctx *ctx, float ms[BRX_STAGE_COUNT]);
/* Shader-clock cycles (s_memtime) each read of the last pipeline call spent in the two heavy
 * kernels, 8 x u64 per read, copied to HOST memory h_out (valid until the next call on ctx):
 *   [0] k_mutate_seg / k_mut_post total over all passes  [1] passes (alignments) of the read  [2] 1 if the final traceback left the stored window
 *   [3] k_fin_align total   [4] final alignment forward    [5] final traceback   [6] k_fin_qscore
 *   [7] words per lane (G) of the final alignment's band geometry in bits 0-15; bit 16: the read was aligned as one of four per
 *       wave (k_fin_quad), bit 17: one read per lane (k_fin_lanes) -- a read repeated in the second phase carries k_fin_align's word */
int brx_last_read_cycles(brx_ctx *ctx, uint64_t *h_out, uint32_t n_reads);
/* number of scratch chunks (sets of final-stage launches) and of mutate passes of the last call */
/* With BRX_PROFILE=1 in the environment at brx_create the mutate kernels time their phases (shader clock, per read,
 * summed over passes), 8 x u64 per read to HOST memory h_out:
 *   [0] proposals (draws, k-mer bytes, table lookups)  [1] applying survivors  [2] parking a window (join, copies)
 *   [3] in-place window alignment  [4] everything else  [5] / [6] forward / traceback share of [3]  [7] unused
 * Zeros without BRX_PROFILE (the default kernels do not contain the clock reads). */
int brx_last_phase_cycles(brx_ctx *ctx, uint64_t *h_out, uint32_t n_reads);
uint32_t brx_last_mutate_passes(const brx_ctx *ctx);
/* Per-kernel launch timing, opt-in (brx_set_kernel_timing(ctx, 1); bench.py and the profiling tools use it): every
 * launch of the kernels below is bracketed by two HIP events ON THE STREAM THE KERNEL IS LAUNCHED ON, and
 * brx_last_kernel_stats() returns, for the last brx_simulate_batch / brx_sequence_fragments call, the number of
 * launches of each kernel, the sum of their event durations and the bases of the reads each kernel handled
 * (fragment bases incl. pads: a read counts ONCE per kernel class however many passes it took part in).  The
 * average launch duration ms / launches is what a rocprofv3 kernel trace reports for the same kernel. */
enum { BRX_KERN_PLAN = 0,        /* k_plan_count + k_scan_plan + k_plan_fill                                   */
       BRX_KERN_BUILD = 1,       /* k_build                                                                    */
       BRX_KERN_MUTATE_SEG = 2,  /* k_mut_apply: the sequential half of the bulk passes, one read per lane (round 6)  */
       BRX_KERN_MUTATE_RUN = 3,  /* k_mutate_seg: reads run to completion with in-place window alignments        */
       BRX_KERN_WIN_LANE = 4,    /* k_win_lane: parked window alignments of a bulk pass, one window per lane    */
       BRX_KERN_WIN_WAVE = 5,    /* k_win_wave                                                                 */
       BRX_KERN_FIN_JOIN = 6,
       BRX_KERN_FIN_ALIGN1 = 7,  /* k_fin_align<1,1,1>                                                         */
       BRX_KERN_FIN_ALIGN2 = 8,  /* k_fin_align<2,2,2>                                                         */
       BRX_KERN_FIN_ALIGN4 = 9,  /* k_fin_align<4,4,4>                                                         */
       BRX_KERN_FIN_ALIGN16 = 10,/* k_fin_align<16,8,65535>: 8 or more band words per lane                  */
       BRX_KERN_FIN_QSCORE = 11,
       BRX_KERN_EMIT = 12,       /* k_recsize + k_scan_rec + k_emit + k_stats                                  */
       BRX_KERN_FIN_LANES = 13,  /* k_fin_lanes: final alignments with a band of up to four blocks, one read per lane */
       BRX_KERN_FIN_QUAD1 = 14,  /* k_fin_quad<1>: bands of up to 13 superblocks of one word, four reads per wave      */
       BRX_KERN_MUT_POST = 15,   /* k_mut_post + k_pass_lists + k_mut_epilogue: parking, proposals ahead, lists, epilogues of the bulk passes (round 6) */
       BRX_KERN_COUNT = 16 };
typedef struct {
    uint32_t launches;
    float ms;                  /* sum of the launches' event durations                                          */
    double bases;              /* fragment bases (RS.n) of the reads this kernel class handled in the call      */
} brx_kernel_stat;
int brx_set_kernel_timing(brx_ctx *ctx, int on);
int brx_last_kernel_stats(const brx_ctx *ctx, brx_kernel_stat out[BRX_KERN_COUNT]);
/* Traceback slabs (= persistent waves of the final align kernels, summed over band classes and the two sets) of the last
 * call: one per read of a class up to the class's wave limit; fewer when the scratch arena could not hold that many. */
uint32_t brx_last_final_launches(const brx_ctx *ctx);
/* Reads of the last call whose final traceback asked for a cell outside the windowed traceback store and were
 * aligned a second time with the full store (environment BRX_TB_WINDOW: window height in
 * sqrt(edit bound) units, default 2, 0 = always the full store).  Results do not depend on it. */
uint32_t brx_last_window_misses(const brx_ctx *ctx);

/* ------------------------------------------------------------------ model builders
 * The counting loops of make_error_model (error_model.py:31-83) and make_qscore_model (qscore_model.py:78-162) over a set
 * of read-to-reference alignments.  The host parses FASTA / FASTQ / PAF exactly as the reference does and ships, as device
 * arrays: the aligned slices of the reads and their qualities, the reference slices (reverse-complemented for '-' strand
 * alignments), and the CIGAR parts ('M' 0, 'I' 1, 'D' 2; reversed for '-' strand, alignment.py:61-64) with the prefix sums
 * of their column / read / reference offsets.  brx_model_count expands the CIGARs into the gapped column arrays
 * (alignment.py:101-132) and counts every sliding window into the caller's hash table (keys preset to ~0, counts to 0,
 * first to ~0):
 *   kind 0, error model:   key = ref k-mer (2k bits, first base most significant) | read k-mer length << 2k
 *                                | read k-mer (2 bits per base, first base least significant) << (2k + 5)
 *   kind 1, qscore model:  key = quality of the middle base (7 bits) | window size index (k_size - 1) / 2 << 7
 *                                | ops << 11, ops = 2 bits per read base (0 '=', 1 'X', 2 'I'), each but the first
 *                                preceded by 4 bits holding the (collapsed) length of the deletion run before it
 *   first[slot] = the earliest (alignment, [size index,] window start) that produced the key: Python dictionaries and its
 *   stable sort order equal counts by first insertion.
 * Windows a key cannot hold (error model: a read k-mer of more than 21 bases; qscore model: more than 52 key bits, a
 * window opening with deletion columns) are appended to `spill` for the host to count: kind 0 as (alignment << 32 | start column), kind 1 as
 * (alignment << 36 | window size index << 32 | start column).
 * Returns BRX_E_OUTPUT when the table is full.                                                                        */
typedef struct {
    uint32_t n_align, k, max_del, n_ksizes;
    uint64_t n_cols;
    const uint8_t *d_seq, *d_qual, *d_ref;
    const uint8_t *d_part_type;
    const uint32_t *d_part_len;
    const uint64_t *d_part_col, *d_part_read, *d_part_ref;
    const uint64_t *d_align_part_off, *d_align_col_off;
    uint8_t *d_rcol, *d_qcol, *d_fcol;
    uint64_t *d_keys; uint32_t *d_counts; uint64_t *d_first;
    uint64_t table_mask;
    uint32_t *d_flags;                 /* [4], preset to 0: [0] table full, [1] / [2] spilled windows of kind 0 / 1 */
    uint64_t *d_spill; uint32_t spill_cap;
} brx_model_job;
int brx_model_count(brx_ctx *ctx, int kind, const brx_model_job *job, void *hip_stream);

/* ------------------------------------------------------------------ window identities (README: Window identities (`plot`))
 * The numbers of `badread plot` (align_sequences' errors_per_read_pos, alignment.py:103-132, and get_window_means,
 * plot_window_identity.py:54-70) over a set of alignments, all of them integers; the host makes the reference's doubles from them.
 * Input: the arrays of brx_model_job that hold the slices and the CIGAR parts (device memory; the column offsets are not needed),
 * d_align_read_off (n_align + 1: where each alignment's read slice begins in d_seq / d_qual, the last entry = n_bases), `window`
 * (W >= 1) and d_align_win_off (n_align + 1: the prefix sums of n, the last entry = n_windows).  For alignment a with a read slice
 * of L bases:
 *   E[p]  errors of read base p: an M column counts 1 where read and reference bytes differ, an I column 1, a D part its length at
 *         the read base behind it (the first base behind the CIGAR for a trailing one); bases the CIGAR does not reach count 0
 *   n     max(L - W, 0) windows -- not L - W + 1: the reference leaves the last one out
 *   S[i]  E[i] + .. + E[i + W - 1], 0 <= i < n;   Q[i] the same sum over q = quality byte - 33 (signed), when want_qual
 * Output: d_stat[a] = n, the smallest and largest S, the smallest i with the largest S, the sum of the S, and the same of Q without
 * the argmax (0 without want_qual); min, max and argmax are 0 where n = 0.  d_err_sum / d_qual_sum (either may be NULL): S[i] and
 * Q[i] at d_align_win_off[a] + i.  The caller keeps every alignment below 2^31 columns (and 223 L below 2^31 with want_qual), so the
 * 32-bit sums are exact.  d_scratch: brx_window_scratch(n_bases, want_qual) bytes of device memory.  Zero alignments, zero windows
 * and a window longer than every read are valid calls.  No atomics and no waiting between workgroups: the results do not depend on
 * scheduling.  Synchronous on `hip_stream`.
 *   BRX_E_ARG                             window 0, a NULL array that is needed, n_bases of 2^39 or more
 *   BRX_E_SCRATCH + brx_scratch_needed()  scratch_bytes is too small; nothing written.                                            */
typedef struct {
    uint32_t n, err_min, err_max, err_argmax;
    uint64_t err_total;
    int32_t qual_min, qual_max;
    int64_t qual_total;
} brx_window_stat;
typedef struct {
    uint32_t n_align, window, want_qual, reserved;
    uint64_t n_bases, n_windows;
    const uint8_t *d_seq, *d_qual, *d_ref;
    const uint8_t *d_part_type;
    const uint32_t *d_part_len;
    const uint64_t *d_part_read, *d_part_ref;
    const uint64_t *d_align_part_off, *d_align_read_off, *d_align_win_off;
    brx_window_stat *d_stat;
    uint32_t *d_err_sum; int32_t *d_qual_sum;
    void *d_scratch; size_t scratch_bytes;
} brx_window_job;
size_t brx_window_scratch(uint64_t n_bases, int want_qual);
int brx_window_means(brx_ctx *ctx, const brx_window_job *job, void *hip_stream);
/* ms between HIP events of the last brx_window_means on ctx that ran under brx_set_kernel_timing: errors, the scans, statistics, values */
int brx_window_last(const brx_ctx *ctx, float ms[4]);

/* ------------------------------------------------------------------ the device loader (README: The device loader (`--gpu-loader`))
 * What load_alignments and model_builder.Job do per CIGAR part, on the device; the host keeps what is O(1) per line or alignment.
 *
 * brx_paf_scan: n_bytes of PAF text in device memory -> one brx_paf_line per line (a byte is a line start if it is byte 0 or follows '\n';
 * a last line without '\n' is a line, the empty piece behind a final '\n' is not).  max_lines: 0 = all; the lines beyond it are neither
 * parsed nor able to flag anything.  *n_lines = the lines written.  d_scratch: brx_paf_scan_scratch(n_bytes) bytes of device memory.
 * A record holds line_off / line_len (without the '\n'), the spans of field 0 (qname: line_off, qname_len) and field 5 (tname), the strand
 * byte, ints[] = the fields 2, 3, 7, 8, 9, 10, `as` = the value of the LAST field that begins AS:i:, cigar_off / cigar_len = the value of
 * the LAST field that begins cg:Z: (all fields count, the first twelve included; offsets from line_off), and of that CIGAR's M / I / D
 * parts (every other letter is a part that is dropped): n_parts, sum_m / sum_i / sum_d, max_indel (the longest I or D part, 0 if none),
 * first_d / last_d (the M + I bases in front of the first / last D part in file order, ~0 without one).
 * A line is regular when every byte is '\t' or in 0x21..0x7e and the first and last are not '\t'; it has at least 11 fields and a strand
 * of one byte; the six integers are [0-9]{1,18} and field 10 is not zero; a cg:Z: and an AS:i: field exist; every AS:i: value is
 * -?[0-9]{1,18}; the CIGAR of the last cg:Z: field is ([0-9]{1,9}[A-Za-z])+.  Any other line carries
 * BRX_PAF_IRREGULAR in flags and nothing else of its record but line_off and line_len is promised: the host parses it.
 *   BRX_E_OUTPUT + brx_output_needed()   line_cap is too small (needed: the number of records); nothing written
 *   BRX_E_ARG                            a NULL argument that is needed; a line of 2^32 bytes or more
 *   BRX_E_SCRATCH + brx_scratch_needed() scratch_bytes is too small
 * Zero bytes is a valid call (no line).  Synchronous on `hip_stream`; takes nothing from the simulate pipeline's state.               */
#define BRX_PAF_IRREGULAR 1u
typedef struct {
    uint64_t line_off;
    uint32_t line_len, flags;
    uint32_t qname_len, tname_off, tname_len, cigar_off, cigar_len, n_parts, max_indel, strand;
    uint64_t ints[6];
    int64_t as;
    uint64_t sum_m, sum_i, sum_d, first_d, last_d;
} brx_paf_line;
size_t brx_paf_scan_scratch(uint64_t n_bytes);
int brx_paf_scan(brx_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint64_t max_lines, brx_paf_line *d_lines, uint64_t line_cap,
                 uint64_t *n_lines, void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* brx_align_pack: the arrays brx_model_count and brx_window_means read, written from the CIGAR text of n_align chosen alignments, a wave
 * per alignment.  Per alignment (d_align): its CIGAR's span in d_text -- ([0-9]{1,10}[A-Za-z])+ with every length below 2^32, or empty --,
 * the n_parts and sums brx_paf_scan gave for it, `reversed` ('-' strand), and its reference slice's start and length in d_reftext (the
 * contigs' text back to back).  d_align_part_off / d_align_col_off / d_align_read_off / d_align_ref_off (n_align + 1 each): where the
 * alignment's parts, columns, read slice and reference slice begin; part_off and ref_off advance by n_parts and ref_len, read_off by the
 * clipped read slice's length, as in model_builder.Job.  Output: d_part_type (0 / 1 / 2), d_part_len, d_part_col / d_part_read /
 * d_part_ref (a part's first column / read base / reference base, from the alignment's bases) and d_ref (the slice, or for a reversed
 * alignment its reverse through d_complement, 256 bytes).  The part with file index i of a reversed alignment lands at n_parts - 1 - i
 * with the mirrored offsets.  An alignment without parts, or without reference bases, is valid; so are zero alignments.
 *   BRX_E_ARG   a NULL array that is needed; a descriptor that leaves the texts, disagrees with the offset arrays or with its CIGAR
 *               (d_flags[0] is then 1, that alignment's outputs are not complete and nothing is stored outside its own ranges)
 * No global scan, no atomics, no waiting between workgroups.  Synchronous on `hip_stream`.                                              */
typedef struct {
    uint64_t cigar_off;
    uint32_t cigar_len, n_parts;
    uint64_t sum_m, sum_i, sum_d;
    uint64_t ref_off, ref_len;
    uint32_t reversed, reserved;
} brx_pack_align;
typedef struct {
    uint32_t n_align, reserved;
    const uint8_t *d_text; uint64_t n_text;
    const uint8_t *d_reftext; uint64_t n_reftext;
    const uint8_t *d_complement;
    const brx_pack_align *d_align;
    const uint64_t *d_align_part_off, *d_align_col_off, *d_align_read_off, *d_align_ref_off;
    uint8_t *d_part_type; uint32_t *d_part_len;
    uint64_t *d_part_col, *d_part_read, *d_part_ref;
    uint8_t *d_ref;
    uint32_t *d_flags;                 /* [1], preset to 0: set where a descriptor is refused */
} brx_pack_job;
int brx_align_pack(brx_ctx *ctx, const brx_pack_job *job, void *hip_stream);
/* ms between HIP events of the last brx_paf_scan and brx_align_pack on ctx that ran under brx_set_kernel_timing */
int brx_loader_last(const brx_ctx *ctx, float ms[2]);

/* ------------------------------------------------------------- the device read loader (README: The device read loader (`--gpu-reads`))
 * What load_fastq does per byte and what model_builder.Job does per read base, on the device.
 *
 * brx_fastq_scan: n_bytes of FASTQ text in device memory -> one brx_fastq_rec per record, for files of the REGULAR LAYOUT.  The rule is
 * the reference's load_fastq: lines end at '\n' only; a line whose stripped form begins with '@' opens a record and the next three lines
 * belong to it whatever they hold; strip() and split() take the six ASCII blanks (space, \t, \n, \r, \x0b, \x0c), so a CRLF file is an
 * ordinary file.  The layout is regular when that rule provably finds its headers on the lines 0, 4, 8, ...: the number of lines is a
 * multiple of 4 (a last line without '\n' is a line, the empty piece behind a final '\n' is not), every line 4k, stripped, begins with
 * '@' and has a name behind it (stripped[1:].split() is not empty), and no byte is 0x80 or more.  Any other file sets a bit in *layout,
 * *n_recs is 0, what d_recs holds is not promised, and the call still returns BRX_OK: the host loads such a file.
 *   BRX_FQ_LINES    the line count is not a multiple of 4 (nothing else of the file is looked at, the other bits stay 0)
 *   BRX_FQ_HEADER   some line 4k opens no record, or is a bare '@'
 *   BRX_FQ_HIGH     a byte of 0x80 or more
 * A record: head_off = the first byte of the header line; the name at head_off + name_off, name_len bytes; seq_off / seq_len and qual_off
 * / qual_len = the second and the fourth line without the blanks at both ends (absolute offsets; a line of blanks alone has length 0 and
 * its offset is where the line ends); flags = 0; reserved = 0.
 * d_scratch: brx_fastq_scan_scratch(n_bytes) bytes of device memory -- 8 bytes per 16 bytes of text for the scan and 8 bytes per line for
 * up to one line per 64 bytes of text.  A file with more lines than that needs more: BRX_E_SCRATCH names the size, as for any scratch
 * that is too small.
 *   BRX_E_ARG                            NULL n_recs, layout or d_text; 2^42 bytes or more; 2^31 records or more; a line of 2^32 bytes
 *   BRX_E_SCRATCH + brx_scratch_needed() scratch_bytes is too small
 *   BRX_E_OUTPUT + brx_output_needed()   rec_cap is below the number of records, or d_recs is NULL (needed: the records); nothing written
 * Zero bytes is a valid call (no record, layout 0).  Synchronous on `hip_stream`; takes nothing from the simulate pipeline's state.      */
#define BRX_FQ_LINES 1u
#define BRX_FQ_HEADER 2u
#define BRX_FQ_HIGH 4u
typedef struct {
    uint64_t head_off;
    uint32_t name_off, name_len;
    uint64_t seq_off, qual_off;
    uint32_t seq_len, qual_len;
    uint32_t flags, reserved;
} brx_fastq_rec;
size_t brx_fastq_scan_scratch(uint64_t n_bytes);
int brx_fastq_scan(brx_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, brx_fastq_rec *d_recs, uint64_t rec_cap, uint64_t *n_recs,
                   uint32_t *layout, void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* brx_reads_pack: seq and qual of model_builder.Job from the FASTQ text that lies on the device.  For alignment k with
 * len = d_align_read_off[k + 1] - d_align_read_off[k]:  d_seq[off[k] + i] = upper(d_text[d_seq_src[k] + i]) (only a-z change, as
 * bytes.upper()) and d_qual[off[k] + i] = d_text[d_qual_src[k] + i], i < len.  d_seq and d_qual hold off[n_align] bytes; every byte of
 * them is written once and none needs to be preset.  An alignment of no bases is valid; so are zero alignments.
 *   BRX_E_ARG   a NULL array that is needed; offsets that do not begin at 0 or do not ascend, a source range that leaves
 *               [0, n_text): d_flags[0] is then 1 and nothing was read or written, out of range or in it
 * No global atomics, no waiting between workgroups.  Synchronous on `hip_stream`.                                                       */
typedef struct {
    uint32_t n_align, reserved;
    const uint8_t *d_text; uint64_t n_text;
    const uint64_t *d_seq_src, *d_qual_src, *d_align_read_off;   /* n_align, n_align, n_align + 1 */
    uint8_t *d_seq, *d_qual;
    uint32_t *d_flags;                 /* [1], preset to 0: set where the job is refused */
} brx_reads_job;
int brx_reads_pack(brx_ctx *ctx, const brx_reads_job *job, void *hip_stream);
/* ms between HIP events of the last brx_fastq_scan and brx_reads_pack on ctx that ran under brx_set_kernel_timing */
int brx_reads_last(const brx_ctx *ctx, float ms[2]);

/* ---- output stage: the FASTQ bytes of a batch as gzip members, made on the device ----
 * Replaces the `| gzip` the reference's users put behind /root/reference/badread/simulate.py:73-82 (print of the
 * record text).  d_in: n_bytes of text in device memory.  d_block_off: n_blocks + 1 ascending byte offsets (device
 * memory; first 0, last n_bytes, no block longer than 128 MB) -- every block becomes one gzip member with its own
 * Huffman code -- or NULL (n_blocks 0): 64 KB blocks.  d_out: device buffer of at least brx_gzip_device_bound(n_bytes,
 * n_blocks) bytes (4-byte aligned); d_scratch: brx_gzip_device_scratch(n_bytes, n_blocks) bytes of device memory.
 * Writes the members back to back (dynamic Huffman coding of the bytes, no match search: gzip readers take them as one
 * stream); *out_bytes = their total size.  Synchronous on `hip_stream`.  BRX_E_OUTPUT / BRX_E_SCRATCH when a buffer is
 * too small. */
size_t brx_gzip_device_bound(size_t n_bytes, uint32_t n_blocks);
size_t brx_gzip_device_scratch(size_t n_bytes, uint32_t n_blocks);
int brx_gzip_device(brx_ctx *ctx, const void *d_in, size_t n_bytes, const uint64_t *d_block_off, uint32_t n_blocks, void *d_out,
                    size_t out_cap, void *d_scratch, size_t scratch_bytes, size_t *out_bytes, void *hip_stream);

/* ---- truth alignments: where every base of the simulated reads came from, as PAF text ----
 * Truth alignments (PAF text) of the reads of the LAST brx_simulate_batch on ctx; valid until the next pipeline call on ctx
 * (BRX_E_STATE otherwise, and after brx_sequence_fragments / brx_align_batch / brx_model_count).  Records back to back in
 * read order; d_read_off (device, n_reads + 1 u64, may be NULL) receives each read's start, the last entry = *out_bytes.
 * BRX_E_OUTPUT + brx_output_needed() when out_cap is too small (nothing written; the call may be repeated).  Synchronous.
 * A record is a maximal run of alignment columns whose fragment bases come from one contig and strand, consecutively, and
 * whose read bases are all in the FASTQ read, trimmed to its first and last =/X column (README: --truth-paf). */
int brx_emit_paf(brx_ctx *ctx, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream);

/* The same truth as SAM records (no header: the @HD/@SQ/@PG lines are the host's), under brx_emit_paf's contract: the reads
 * of the LAST brx_simulate_batch on ctx, BRX_E_STATE where there is none, BRX_E_OUTPUT + brx_output_needed(), d_read_off,
 * synchronous.  Both may be called for one batch, in either order.  One line per PAF record, in PAF order: FLAG 16 for '-',
 * 2048 on all but the primary (tp:A:P); POS = tstart + 1, MAPQ 60; CIGAR = the record's cg:Z: between clips (S on the
 * primary, H on the others); SEQ / QUAL = the whole read on the primary, the record's slice on the others, reverse-
 * complemented (brx_reference.comp on the codes) / reversed for '-'; NM:i: and AS:i:, and on the primary CO:Z: with the
 * FASTQ header line after the name.  A read with a FASTQ record and no PAF record gets one unmapped line (FLAG 4, with
 * CO:Z:), a read without a FASTQ record none (README: --truth-sam). */
int brx_emit_sam(brx_ctx *ctx, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream);

/* The same records as uncompressed BAM (SAM spec v1 section 4.2; no header, no BGZF), one per line of brx_emit_sam in the same
 * order, under the same contract: BRX_E_STATE, BRX_E_OUTPUT + brx_output_needed() with nothing written, d_read_off, synchronous;
 * callable before or after brx_emit_paf / brx_emit_sam, which stay byte-identical.  Little-endian, nothing aligned.  refID = the
 * contig's index, pos = POS - 1, l_read_name 37, mapq 60, bin = reg2bin(pos, pos + reflen), next_refID / next_pos -1, tlen 0; an
 * unmapped record has refID -1, pos -1, mapq 0, bin 4680, no CIGAR, flag 4.  SEQ in nibbles of '=ACMGRSVTWYHKDBN' (anything else
 * 15), QUAL = character - 33.  Tags NM, AS (smallest integer type: C S I, below zero c s i), CO:Z: on primary and unmapped
 * records.  A record with more than max_cigar_ops operations, clips included (0 = 65535; below 2 or above 65535: BRX_E_ARG),
 * holds `l_seq S, reflen N` as its CIGAR and the real operations in a last tag CG:B:I (README: --truth-bam). */
int brx_emit_bam(brx_ctx *ctx, uint32_t max_cigar_ops, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes,
                 void *hip_stream);

/* brx_emit_sam / brx_emit_bam with MD:Z: and / or SA:Z: behind AS (tags: BRX_TAG_MD | BRX_TAG_SA; 0 = exactly the functions above,
 * any other bit BRX_E_ARG), under the same contract; stateless, callable in any order with the other emitters, which stay byte-
 * identical.  Tag order NM AS [MD] [SA] [CO], then CG in a long-CIGAR BAM record; in BAM both are Z tags.  Unmapped lines get neither.
 *   MD  on every mapped line, samtools' rule: the '=' columns as numbers, a mismatch as the reference base, a run of deleted
 *       reference bases behind '^', a 0 between adjacent items and at an end that is a mismatch.  The reference base is the base of
 *       the fragment the read was aligned against (what NM counts by), through brx_reference.sym; on '-' lines complemented through
 *       brx_reference.comp, columns from the record's last to its first.  Clips take no part.
 *   SA  on every mapped line of a read with two or more: `RNAME,POS,strand,CIGAR,60,NM;` for each OTHER mapped line, the primary's
 *       first, the rest in line order.  CIGAR is the compact form `[left]S min(Q,T)M |Q-T|I-or-D [right]S` (Q = M + I, T = M + D
 *       lengths; clips always S).  Contig names are copied as they are (README: --truth-tags). */
enum { BRX_TAG_MD = 1u, BRX_TAG_SA = 2u };
int brx_emit_sam_tags(brx_ctx *ctx, uint32_t tags, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream);
int brx_emit_bam_tags(brx_ctx *ctx, uint32_t tags, uint32_t max_cigar_ops, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off,
                      size_t *out_bytes, void *hip_stream);

/* brx_emit_paf / brx_emit_sam_tags / brx_emit_bam_tags with minimap2's --eqx and --cs on every truth file (fmt: BRX_FMT_* bits; 0 =
 * exactly the functions above; an unknown bit, or BRX_FMT_CS_LONG without BRX_FMT_CS: BRX_E_ARG), under the same contract: BRX_E_STATE,
 * BRX_E_OUTPUT + brx_output_needed() with nothing written, stateless, callable in any order with the other emitters.  Records, their
 * order, the primaries and every field not named here are those of fmt 0.
 *   BRX_FMT_EQX      CIGAR runs are maximal runs of one op, = X I D (BAM: 7 8 1 2), in cg:Z:, the SAM CIGAR and the BAM operations; the
 *                    clips stay S / H.  n_cigar_op, and so max_cigar_ops and CG:B:I, count these runs.  SA:Z: keeps its compact CIGAR.
 *   BRX_FMT_CS       cs:Z: on every PAF record (last field) and every mapped SAM / BAM line (NM AS [MD] [cs] [SA] [CO], CG last): the
 *                    record's columns in reference-forward order (from its last column on '-'), a run of n '=' as `:n`, an X as `*rq`, a
 *                    run of I as `+q..`, a run of D as `-r..`; r = the fragment's base that MD:Z: writes, q = the read's base that SEQ
 *                    writes (both through brx_reference.sym, on '-' complemented through brx_reference.comp), in lower case (c | 0x20).
 *   BRX_FMT_CS_LONG  a run of '=' as `=` and its r bases as they are, instead of `:n` (README: --truth-cs, --truth-eqx). */
enum { BRX_FMT_EQX = 1u, BRX_FMT_CS = 2u, BRX_FMT_CS_LONG = 4u };
int brx_emit_paf_fmt(brx_ctx *ctx, uint32_t fmt, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream);
int brx_emit_sam_fmt(brx_ctx *ctx, uint32_t fmt, uint32_t tags, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes,
                     void *hip_stream);
int brx_emit_bam_fmt(brx_ctx *ctx, uint32_t fmt, uint32_t tags, uint32_t max_cigar_ops, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off,
                     size_t *out_bytes, void *hip_stream);

/* ---- the true coverage of the reference (README: --truth-depth) ----
 * brx_emit_depth: the end points of the truth records of the LAST brx_simulate_batch on ctx, a fourth truth kind under brx_emit_paf's
 * contract: BRX_E_STATE where there is no batch, BRX_E_OUTPUT + brx_output_needed() with nothing written, d_read_off in bytes,
 * synchronous, stateless, callable in any order with the other emitters, which stay byte-identical.  Its "records" are events: two
 * little-endian uint64 per PAF record, in PAF order, the start event and then the end event (d_out 8-byte aligned):
 *   event = contig index << 40 | position << 1 | is_start       start: position = tstart, is_start = 1; end: position = tend, is_start = 0
 * so a reference may have up to 2^24 - 1 contigs of fewer than 2^39 bases. */
#define BRX_DEPTH_EVENT(contig, position, is_start) (((uint64_t)(contig) << 40) | ((uint64_t)(position) << 1) | (uint64_t)(is_start))
int brx_emit_depth(brx_ctx *ctx, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream);

/* brx_depth_bedgraph: n_events events (device memory, any order, from any number of batches) against the reference of ctx
 * (brx_set_reference) -> the bedGraph text of the whole reference in d_out: `contig TAB start TAB end TAB depth LF`, 0-based half-open,
 * no header.  depth(contig, p) = the events' records with tstart <= p < tend.  Every contig is covered from 0 to its length, in
 * reference order, by maximal runs of equal depth, zero-depth runs included; a contig without a record is one line.  The bytes are the
 * same for every permutation of the events; n_events = 0 gives one zero line per contig.
 *   BRX_E_OUTPUT + brx_output_needed()   out_cap is too small; nothing written.
 *   BRX_E_ARG, nothing written           n_events is odd; an event names a contig outside the reference or a position beyond its contig's
 *                                        length; the running depth is negative somewhere or not zero at a contig's end; 2^24 or more
 *                                        contigs; 2^31 or more keys (n_events + 4 per contig).
 *   BRX_E_SCRATCH + brx_scratch_needed() d_scratch is too small: brx_depth_bedgraph_scratch(n_events) is enough for a reference of up to
 *                                        BRX_DEPTH_SCRATCH_CONTIGS contigs, each further contig takes four more events' worth.
 *   BRX_E_STATE                          no reference.
 * The events are sorted (LSD radix sort, 8 bits per pass, only the digits that the contig count and the longest contig let vary), summed
 * (+1 / -1 from the low bit) and written by workgroups of 256 threads over tiles of BRX_DEPTH_TILE keys.  Synchronous on `hip_stream`.
 * brx_depth_last: the sort passes of the last call on ctx and the host-side ms of its three stages (sort, depth, text). */
#define BRX_DEPTH_TILE 1024u
#define BRX_DEPTH_SCRATCH_CONTIGS 4096u
size_t brx_depth_bedgraph_scratch(uint64_t n_events);
int brx_depth_bedgraph(brx_ctx *ctx, const uint64_t *d_events, uint64_t n_events, uint8_t *d_out, size_t out_cap, size_t *out_bytes,
                       void *d_scratch, size_t scratch_bytes, void *hip_stream);
int brx_depth_last(const brx_ctx *ctx, uint32_t *sort_passes, float ms[3]);

/* n_bytes of device memory as BGZF blocks (SAM spec v1 section 4.1) back to back, one per BRX_BGZF_BLOCK input bytes, the last
 * one possibly shorter, none for no input: the members of brx_gzip_device (one dynamic Huffman code per block, no match search)
 * behind the 18-byte BGZF header (FEXTRA, 'B' 'C', BSIZE = the block's size - 1).  A block needs at most 61 607 bytes, so every
 * input fits the format's 64 KB without a stored block.  No EOF block: the caller ends its file with one.  Buffers as for
 * brx_gzip_device: d_out of brx_bgzf_device_bound(n_bytes) bytes (4-byte aligned; less is tried first by the Python wrapper,
 * BRX_E_OUTPUT + brx_output_needed() says what is missing), d_scratch of brx_bgzf_device_scratch(n_bytes).  Synchronous. */
#define BRX_BGZF_BLOCK 32768u
size_t brx_bgzf_device_bound(size_t n_bytes);
size_t brx_bgzf_device_scratch(size_t n_bytes);
int brx_bgzf_device(brx_ctx *ctx, const void *d_in, size_t n_bytes, void *d_out, size_t out_cap, void *d_scratch, size_t scratch_bytes,
                    size_t *out_bytes, void *hip_stream);
/* brx_bgzf_device with one more output: d_block_off (device memory, may be NULL: exactly the call above) receives n_blocks + 1 offsets,
 * n_blocks = ceil(n_bytes / BRX_BGZF_BLOCK): where each block begins in d_out, the last entry = *out_bytes.  The blocks' bytes are those
 * of brx_bgzf_device.  Nothing is written to it when the call answers BRX_E_OUTPUT or BRX_E_SCRATCH, and nothing for n_bytes = 0. */
int brx_bgzf_device_off(brx_ctx *ctx, const void *d_in, size_t n_bytes, void *d_out, size_t out_cap, void *d_scratch, size_t scratch_bytes,
                        size_t *out_bytes, uint64_t *d_block_off, void *hip_stream);

/* ---- the truth BAM in coordinate order and its index (README: --truth-bam-sorted) ----
 * brx_bam_sort: n_bytes of uncompressed BAM records back to back (device memory; what brx_emit_bam writes, of any number of batches)
 * and d_seg_off, n_seg + 1 ascending offsets (first 0, last n_bytes) that cut them into segments of whole records -- reads are the intended
 * segments, a segment may be empty -> the same records in d_sorted (n_bytes, device memory) ordered by ((uint32_t)refID, pos), so that
 * refID -1 comes last.  The sort is stable: equal keys keep the order of the input.  d_recs receives one brx_bam_rec per record in sorted
 * order: off = where the record begins in d_sorted, refID, pos and bin as the record holds them, end = pos + reflen, reflen = the sum of the
 * M, D, N, = and X lengths of the CIGAR field (of a long-CIGAR record: the N of its placeholder), 0 counting as 1; end = 0 on refID -1.
 * *n_records = the records, *n_unmapped = those of refID -1.  n_ref and max_pos say what the keys can hold: a record needs refID in
 * [-1, n_ref), pos in [0, max_pos) and, on refID -1, pos -1; only the digits that n_ref and max_pos let vary are sorted by.
 * Every record is walked by its block_size first, inside its segment: a chain that leaves its segment or does not end on the segment's
 * end, a block_size below 32 + l_read_name + 4 n_cigar_op, a refID or pos outside the ranges above are refused before any byte is moved.
 *   BRX_E_ARG                            a NULL argument that is needed; offsets that do not begin at 0, ascend and end at n_bytes; a record
 *                                        refused as above; 2^32 or more records; 2^43 or more bytes; max_pos above 2^31.  Nothing written.
 *   BRX_E_OUTPUT + brx_output_needed()   rec_cap is below the number of records (needed: the records); nothing written.
 *   BRX_E_SCRATCH + brx_scratch_needed() scratch_bytes is too small.  brx_bam_sort_scratch(n_bytes, n_seg) is enough for one record per
 *                                        4096 bytes and one per segment; input with more records needs more, and the call names the size.
 * Zero bytes is a valid call (no record).  LSD radix sort of (key, record number), 8 bits per pass, over tiles of BRX_DEPTH_TILE keys; the
 * gather is gridded over the output, every byte of d_sorted has one writer.  No global atomics, no waiting between workgroups.  Synchronous
 * on `hip_stream`; takes nothing from the simulate pipeline's state.
 * brx_bamsort_last: ms between HIP events of the last brx_bam_sort on ctx that ran under brx_set_kernel_timing (walk and table of records,
 * sort, length scan and record table, gather) and of the last brx_bam_index (check and chunks, chunk sort, linear index, text). */
typedef struct {
    uint64_t off;
    int32_t refID, pos;
    uint32_t end, bin;
} brx_bam_rec;
size_t brx_bam_sort_scratch(uint64_t n_bytes, uint64_t n_seg);
int brx_bam_sort(brx_ctx *ctx, const uint8_t *d_records, uint64_t n_bytes, const uint64_t *d_seg_off, uint64_t n_seg, uint32_t n_ref,
                 uint32_t max_pos, uint8_t *d_sorted, brx_bam_rec *d_recs, uint64_t rec_cap, uint64_t *n_records, uint64_t *n_unmapped,
                 void *d_scratch, size_t scratch_bytes, void *hip_stream);
int brx_bamsort_last(const brx_ctx *ctx, float ms[8]);

/* brx_bam_index: the BAI index (SAM spec v1 section 5.2, without the metadata pseudo-bin) of a sorted record stream of n_bytes that was
 * compressed into BGZF blocks of BRX_BGZF_BLOCK input bytes.  d_recs: the table brx_bam_sort wrote, n_records lines.  d_block_off:
 * n_blocks + 1 ascending compressed offsets of the blocks, n_blocks = ceil(n_bytes / BRX_BGZF_BLOCK), the last entry = where the file's
 * EOF block begins; `base` = the file offset of block 0 (the compressed header), added to each.  The byte at offset u of the stream has the
 * virtual offset (base + d_block_off[u / 32768]) << 16 | u % 32768.  d_out (4-byte aligned) receives, all little-endian:
 *   "BAI\1", int32 n_ref; per contig: int32 n_bin, the bins in ascending number {uint32 bin, int32 n_chunk, n_chunk x {uint64 beg, end}},
 *   int32 n_intv, n_intv x uint64 ioffset; uint64 n_no_coor = the records of refID -1.
 * A chunk is a maximal run of records consecutive in the file, of one contig and one bin: beg = the virtual offset of its first record, end
 * = that of the byte behind its last; a bin's chunks in file order, none merged.  n_intv = (the contig's largest end - 1 >> 14) + 1;
 * ioffset[w] = the virtual offset of the first record in file order with pos < (w + 1) << 14 and end > w << 14; a window no record
 * overlaps takes the value of the next window that has one; a contig without records has n_bin 0 and n_intv 0.
 *   BRX_E_ARG                            a NULL argument that is needed; the table is not sorted by ((uint32_t)refID, pos) or its offsets do
 *                                        not ascend inside [0, n_bytes); a refID outside [-1, n_ref); a mapped record with pos < 0, end <=
 *                                        pos or end > 2^29; n_blocks other than ceil(n_bytes / 32768); block offsets that descend or reach
 *                                        2^48 with base; 2^32 or more records.  Nothing written.
 *   BRX_E_OUTPUT + brx_output_needed()   out_cap is too small; nothing written.
 *   BRX_E_SCRATCH + brx_scratch_needed() scratch_bytes is below brx_bam_index_scratch(n_records, n_ref).
 * No records is a valid call.  No global atomics, no waiting between workgroups.  Synchronous on `hip_stream`. */
size_t brx_bam_index_scratch(uint64_t n_records, uint32_t n_ref);
int brx_bam_index(brx_ctx *ctx, const brx_bam_rec *d_recs, uint64_t n_records, uint32_t n_ref, uint64_t n_bytes, const uint64_t *d_block_off,
                  uint64_t n_blocks, uint64_t base, uint8_t *d_out, size_t out_cap, size_t *out_bytes, void *d_scratch, size_t scratch_bytes,
                  void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* BRX_H */
