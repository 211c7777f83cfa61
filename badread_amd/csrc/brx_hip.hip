/*
 * brx_hip.hip -- host side of libbrx_hip.so: the C-ABI declared in include/brx.h.
 *
 * Build (see badread_amd/build.py):
 *   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared brx_hip.hip -o libbrx_hip.so
 * -ffp-contract=off is part of the numerical spec (include/brx_spec.h): the device must round
 * every double operation exactly like the CPU oracle.
 *
 * All device memory comes from the caller: descriptors point at caller tensors, and every
 * temporary lives in the caller's scratch arena, carved by a bump allocator per call.
 */
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "brx_kernels.h"
#include "brx_finplan.h"

#define BRX_KEV_MAX 2048

struct brx_ctx {
    int device;
    int n_cu;
    int waves_per_cu;
    BrxDev dev;
    bool has_ref, has_em, has_qm, has_params;
    uint8_t *scratch;
    size_t scratch_bytes;
    size_t scratch_needed, output_needed;
    uint64_t win_bytes;
    uint64_t *h_totals;          /* pinned, 16 x u64 followed by 64 x u32 debug progress words and 16 x u32 of small read-backs */
    uint8_t *d_totals_alias;     /* the same block as the device sees it (hipHostMallocMapped) */
    uint8_t *h_stage, *d_stage;  /* pinned + mapped staging block of the batch: read states, orders, the final stage's tables.  Kernels copy
                                    to and from it (k_copy_words) -- a hipMemcpyAsync of a few bytes is a blit kernel of the runtime that
                                    waited 3.6 ms on average behind the resident waves of six batches, ~50 times per batch */
    size_t stage_bytes;
    uint32_t *h_prog, *d_prog;   /* host / device views of the progress words */
    hipEvent_t ev_b[BRX_STAGE_COUNT], ev_e[BRX_STAGE_COUNT];   /* begin / end of each stage on the launch stream */
    float stage_ms[BRX_STAGE_COUNT];
    uint32_t final_launches, mutate_passes;
    uint32_t lanes_cycles;
    int mutate_passes_route;     /* BRX_MUTATE_PASSES=1: the bulk set through host-driven passes {k_mut_apply, k_mut_post, k_pass_lists, k_win_lane, k_win_wave}
                                    and an in-place tail (rounds 2-6a) instead of one launch of k_mut_lanes */
    uint32_t tail_reads;         /* BRX_TAIL_READS: this few reads left in the mutate stage -> one in-place launch (0xFFFFFFFF = not set: n_reads / 8, at least 1024;
                                    measured on configs[3]: 1024 of 16384, 4096 of 49152) */
    int tb_hmul;                 /* BRX_TB_WINDOW: window of the final traceback store in sqrt(ub) units (2; 0 = full store; -1 = 8 rows, test) */
    uint32_t window_misses;      /* reads of the last batch whose final traceback left the stored window (phase 1) */
    uint32_t fin_head_reads;     /* BRX_FIN_HEAD_READS: the longest reads of a batch form the head set of the final stage (side streams) */
    uint32_t head_reads;         /* BRX_HEAD_READS: the longest reads of a batch run as their own chain on the side stream (0 = off) */
    int wide_stream;             /* BRX_WIDE_STREAM: the head set's widest band class aligns on a third stream */
    hipStream_t side2;
    hipEvent_t ev_fork2[2], ev_join2[2], ev_head_mut;
    hipEvent_t ev_fork3, ev_join3[2];   /* the bulk set's band classes on the head chain's streams */
    int fin_spread;                      /* BRX_FIN_SPREAD (default 1) */
    uint32_t quad_min_reads;             /* BRX_QUAD_MIN_READS (default 4096): a set with fewer four-per-wave reads aligns them on whole waves */
    int fin_lanes;                       /* BRX_FIN_LANES (default 1): narrow-band final alignments one read per lane (k_fin_lanes) */
    uint32_t lanes_min_reads;            /* BRX_LANES_MIN_READS (default 2048): a set with fewer by-lane reads aligns them on whole waves */
    int fin_quad;                        /* BRX_FIN_QUAD (default 1): final alignments of one-word bands four per wave (k_fin_quad<1>) */
    hipStream_t side;            /* second stream: the wide-band align kernels run beside the narrow one (one stream for all
                                    three wide classes: a stream per class measured 30 % slower, r01d) */
    hipEvent_t ev_fork, ev_join;
    hipEvent_t ev_wait;          /* the host thread polls this event with a short sleep in wait_stream (hipStreamSynchronize spins a core) */
    uint64_t *d_clk, *d_phase; uint32_t clk_reads;
    /* per-kernel launch timing (brx_set_kernel_timing / brx_last_kernel_stats): event pairs around every launch */
    int ktiming;
    hipEvent_t kev_b[BRX_KEV_MAX], kev_e[BRX_KEV_MAX];
    uint8_t kev_kind[BRX_KEV_MAX];
    int kev_n, kev_dropped;
    brx_kernel_stat kstat[BRX_KERN_COUNT];
    int profile;                 /* BRX_PROFILE=1: the mutate kernels time their phases (brx_last_phase_cycles) */
    /* brx_emit_paf / brx_emit_sam: what the last brx_simulate_batch left in the arena (valid until the next call that reuses the arena) */
    bool paf_valid;
    BrxDev paf_dev;
    const RS *paf_rs; const PSeg *paf_segs; uint32_t paf_reads;
    const PPiece *paf_pieces; const uint8_t *paf_seqbuf;      /* brx_emit_sam: what k_emit read the records from */
    const uint8_t *paf_frags;                                 /* MD:Z: -- the fragments (Fbuf: bottom of the arena, kept until the next batch) */
    uint8_t *h_sa, *d_sa; size_t sa_bytes;         /* pinned (mapped): SA:Z: -- one SaRec per record of the reads with two or more */
    uint8_t *h_paf, *d_paf; size_t paf_bytes;      /* pinned (mapped): per-read PAF bytes, primary records and offsets */
    uint32_t depth_passes; float depth_ms[3];      /* the last brx_depth_bedgraph: its sort passes; ms of its sort, depth and text stages */
    float window_ms[4];                            /* the last brx_window_means under brx_set_kernel_timing: errors, scans, statistics, values */
    float loader_ms[2];                            /* the last brx_paf_scan and brx_align_pack under brx_set_kernel_timing */
    float reads_ms[2];                             /* the last brx_fastq_scan and brx_reads_pack under brx_set_kernel_timing */
    float bamsort_ms[8];                           /* the last brx_bam_sort (four stages) and brx_bam_index (four) under brx_set_kernel_timing */
    char err[512];
};

static int fail(brx_ctx *c, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(c, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return fail((c), BRX_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

static int env_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
static bool brx_debug() { static int v = -1; if (v < 0) { const char *e = getenv("BRX_DEBUG"); v = (e && *e && *e != '0') ? 1 : 0; } return v == 1; }
#define DBG(...) do { if (brx_debug()) { fprintf(stderr, "[brx] " __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)

/* Bump allocator over the context's scratch arena.  take() grows from the bottom; take_top() carves from the high end what only the
 * mutate stage of the chain on the caller's stream needs -- the move-code stores of k_mut_lanes (6.6 MB per wave), the survivor rings,
 * the per-wave window scratch: 11.9 GB of a 65 536-read batch of configs[3] -- and release_top() hands that region back when that chain
 * is done, so that the bulk set's traceback slabs (13 GB, allocated after it) lie over it: the arena holds the larger of the two, not
 * their sum (40 -> 30 GB per batch in flight; VERDICT r5 #5 asked for <= 30). */
struct Arena {
    uint8_t *base; size_t cap; size_t used; size_t top;
    void *take(size_t bytes) {
        size_t at = (used + 255) & ~(size_t)255;
        used = at + bytes;
        return used + top <= cap ? base + at : nullptr;
    }
    void *take_top(size_t bytes) {
        if (bytes + top + 256 > cap) { top = cap + 1; return nullptr; }          /* ok() says no */
        const size_t end = (cap - top - bytes) & ~(size_t)255;
        top = cap - end;
        return used + top <= cap ? base + end : nullptr;
    }
    void release_top() { top = 0; }
    size_t room() const { return cap - (top < cap ? top : cap); }            /* what take() may grow to right now */
    bool ok() const { return used + top <= cap; }
};

extern "C" const char *brx_version(void) { return "brx-hip 0.1 (gfx950)"; }

static char g_create_err[512] = "";

/* every stream, event and pinned buffer the context owns (the context is calloc'ed: unset handles are null) */
static void release(brx_ctx *c) {
    if (!c) return;
    for (int i = 0; i < BRX_STAGE_COUNT; ++i) {
        if (c->ev_b[i]) (void)hipEventDestroy(c->ev_b[i]);
        if (c->ev_e[i]) (void)hipEventDestroy(c->ev_e[i]);
    }
    for (int i = 0; i < BRX_KEV_MAX; ++i) {
        if (c->kev_b[i]) (void)hipEventDestroy(c->kev_b[i]);
        if (c->kev_e[i]) (void)hipEventDestroy(c->kev_e[i]);
    }
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->side2) (void)hipStreamDestroy(c->side2);
    for (int i = 0; i < 2; ++i) { if (c->ev_fork2[i]) (void)hipEventDestroy(c->ev_fork2[i]); if (c->ev_join2[i]) (void)hipEventDestroy(c->ev_join2[i]); }
    if (c->ev_head_mut) (void)hipEventDestroy(c->ev_head_mut);
    if (c->ev_fork3) (void)hipEventDestroy(c->ev_fork3);
    for (int i = 0; i < 2; ++i) if (c->ev_join3[i]) (void)hipEventDestroy(c->ev_join3[i]);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_wait) (void)hipEventDestroy(c->ev_wait);
    if (c->h_totals) (void)hipHostFree(c->h_totals);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_paf) (void)hipHostFree(c->h_paf);
    if (c->h_sa) (void)hipHostFree(c->h_sa);
    free(c);
}

static int create_fail(brx_ctx *c, const char *what, hipError_t e) {
    snprintf(g_create_err, sizeof(g_create_err), "brx_create: %s failed: %s (%d)", what, hipGetErrorString(e), (int)e);
    release(c);
    return BRX_E_HIP;
}

extern "C" int brx_create(int device_id, brx_ctx **out) {
    if (!out) return BRX_E_ARG;
    g_create_err[0] = 0;
    brx_ctx *c = (brx_ctx *)calloc(1, sizeof(brx_ctx));
    if (!c) return BRX_E_ARG;
    c->device = device_id;
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return create_fail(c, "hipSetDevice", e);
    int n_cu = 0;
    if ((e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device_id)) != hipSuccess)
        return create_fail(c, "hipDeviceGetAttribute(MultiprocessorCount)", e);
    c->n_cu = n_cu > 0 ? n_cu : 256;
    c->waves_per_cu = std::max(env_int("BRX_WAVES_PER_CU", 16), 1);
    c->win_bytes = (uint64_t)env_int("BRX_WIN_KB", 512) << 10;      /* 512 KB: a 1000 x 1900 window with the whole matrix in the band (reads inside N runs: every draw changes a base) */
    if ((e = hipHostMalloc((void **)&c->h_totals, 16 * sizeof(uint64_t) + 80 * sizeof(uint32_t), hipHostMallocMapped)) != hipSuccess)
        return create_fail(c, "hipHostMalloc", e);
    c->h_prog = (uint32_t *)(c->h_totals + 16);
    memset(c->h_prog, 0, 80 * sizeof(uint32_t));
    void *dp = nullptr;
    if ((e = hipHostGetDevicePointer(&dp, c->h_totals, 0)) != hipSuccess) return create_fail(c, "hipHostGetDevicePointer", e);
    c->d_totals_alias = (uint8_t *)dp;
    c->d_prog = (uint32_t *)(c->d_totals_alias + 16 * sizeof(uint64_t));
    for (int i = 0; i < BRX_STAGE_COUNT; ++i) {
        if ((e = hipEventCreate(&c->ev_b[i])) != hipSuccess) return create_fail(c, "hipEventCreate", e);
        if ((e = hipEventCreate(&c->ev_e[i])) != hipSuccess) return create_fail(c, "hipEventCreate", e);
    }
    if ((e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking)) != hipSuccess) return create_fail(c, "hipStreamCreate", e);
    if ((e = hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking)) != hipSuccess) return create_fail(c, "hipStreamCreate", e);
    for (int i = 0; i < 2; ++i)
        if ((e = hipEventCreateWithFlags(&c->ev_fork2[i], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&c->ev_join2[i], hipEventDisableTiming)) != hipSuccess) return create_fail(c, "hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&c->ev_head_mut, hipEventDisableTiming)) != hipSuccess) return create_fail(c, "hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&c->ev_fork3, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_join3[0], hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_join3[1], hipEventDisableTiming)) != hipSuccess) return create_fail(c, "hipEventCreate", e);
    c->fin_spread = env_int("BRX_FIN_SPREAD", 1);
    c->quad_min_reads = (uint32_t)env_int("BRX_QUAD_MIN_READS", 4096);
    c->fin_lanes = env_int("BRX_FIN_LANES", 1);
    c->lanes_min_reads = (uint32_t)env_int("BRX_LANES_MIN_READS", 2048);
    /* the one-word class.  Measured on configs[3] (profiles/r05a): 5.30 Gbases/s with it against 5.22 without.  (A two-word class --
       14-26 superblocks of 32 rows as 7-13 of 64 -- cost 20.6 instructions per read column where the whole-wave kernel costs 25, on
       half the waves: 4.62-4.67 with both; round 6 removed its instantiation.  brx_quad.h keeps the words per lane a template
       parameter.) */
    c->fin_quad = env_int("BRX_FIN_QUAD", 1) & 1;
    c->head_reads = (uint32_t)env_int("BRX_HEAD_READS", 1024);      /* (512 until the lane kernel: 6.33-6.43 against 6.47-6.55 Gbases/s at 1024, three A/B pairs; 768: 6.44, 1536: 6.46 -- profiles/r06aa) */
    c->fin_head_reads = (uint32_t)env_int("BRX_FIN_HEAD_READS", 2048);
    c->wide_stream = env_int("BRX_WIDE_STREAM", 1);
    /* a context owns exactly three streams besides the caller's: every stream of a context takes a hardware queue, and two idle
       extra streams per context (6 contexts) cost 24 % of the rate (round 2, A/B on one box: 2.97 -> 2.27 Gbases/s) */
    if ((e = hipEventCreateWithFlags(&c->ev_wait, hipEventDisableTiming | hipEventBlockingSync)) != hipSuccess) return create_fail(c, "hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)) != hipSuccess) return create_fail(c, "hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming)) != hipSuccess) return create_fail(c, "hipEventCreate", e);
    c->profile = env_int("BRX_PROFILE", 0) ? 1 : 0;
    c->tb_hmul = env_int("BRX_TB_WINDOW", 2);
    c->mutate_passes_route = env_int("BRX_MUTATE_PASSES", 0) != 0;
    c->lanes_cycles = (uint32_t)env_int("BRX_LANES_CYCLES", 96);       /* alignment cycles a read spends in k_mut_lanes before the in-place kernel takes it over (0: all).
                                                                                                          Measured, configs[3], six batches in flight (profiles/r06s, r06w): 32: 5.26, 48: 5.74, 64: 6.18-6.24, 96: 6.27-6.40, 128: 6.23, all: 5.51 Gbases/s */
    c->tail_reads = (uint32_t)env_int("BRX_TAIL_READS", -1);   /* unset: an eighth of the batch, at least 1024 */
    c->err[0] = 0;
    *out = c;
    return BRX_OK;
}

extern "C" void brx_destroy(brx_ctx *c) { release(c); }

extern "C" const char *brx_last_error(const brx_ctx *c) { return c ? c->err : g_create_err; }

extern "C" int brx_set_reference(brx_ctx *c, const brx_reference *r) {
    if (!c || !r) return BRX_E_ARG;
    if (r->n_contigs == 0 || !r->d_packed || !r->d_contigs) return fail(c, BRX_E_ARG, "reference has no contigs");
    c->dev.ref = *r; c->has_ref = true; c->paf_valid = false; return BRX_OK;
}
extern "C" int brx_set_error_model(brx_ctx *c, const brx_error_model *m) {
    if (!c || !m) return BRX_E_ARG;
    if (m->k < 1 || m->k > 16) return fail(c, BRX_E_ARG, "error model k-mer size %d out of range", m->k);
    if (m->type != 0 && (!m->d_rowx || !m->d_altx))
        return fail(c, BRX_E_ARG, "error model without its lookup-order tables (d_rowx, d_altx: include/brx.h)");
    c->dev.em = *m; c->has_em = true; c->paf_valid = false; return BRX_OK;
}
extern "C" int brx_set_qscore_model(brx_ctx *c, const brx_qscore_model *m) {
    if (!c || !m) return BRX_E_ARG;
    if (m->k < 1 || (m->k & 1) == 0 || 2 * m->k + m->gap_bits * (m->k - 1) > 56 || (m->hash_size & (m->hash_size - 1)))
        return fail(c, BRX_E_ARG, "unsupported qscore model geometry");
    c->dev.qm = *m; c->has_qm = true; c->paf_valid = false; return BRX_OK;
}
extern "C" int brx_set_params(brx_ctx *c, const brx_sim_params *p) {
    if (!c || !p) return BRX_E_ARG;
    c->dev.p = *p; c->has_params = true; c->paf_valid = false; return BRX_OK;
}
extern "C" int brx_set_scratch(brx_ctx *c, void *d_scratch, size_t bytes) {
    if (!c) return BRX_E_ARG;
    c->scratch = (uint8_t *)d_scratch; c->scratch_bytes = bytes; c->paf_valid = false; return BRX_OK;
}
extern "C" size_t brx_scratch_needed(const brx_ctx *c) { return c ? c->scratch_needed : 0; }
extern "C" size_t brx_output_needed(const brx_ctx *c) { return c ? c->output_needed : 0; }
extern "C" int brx_last_stage_ms(const brx_ctx *c, float ms[BRX_STAGE_COUNT]) {
    if (!c || !ms) return BRX_E_ARG;
    for (int i = 0; i < BRX_STAGE_COUNT; ++i) ms[i] = c->stage_ms[i];
    return BRX_OK;
}

/* wait for the stream; with BRX_DEBUG set, poll instead and on a stall print the kernel's progress
 * words and leave the process (a hung kernel must not take the GPU box down with it) */
static int wait_stream(brx_ctx *c, hipStream_t st, const char *what) {
    if (!brx_debug()) {
        /* A batch waits ~25 times for its stream, and a rank keeps six batches in flight on six host threads: hipStreamSynchronize
           spins, i.e. six busy cores per GPU -- 48 on an 8-GPU node whose container has 16.  The thread polls an event every 40 us
           instead (tens of microseconds later per wait, against ~1.7 s per batch). */
        HIPCHK(c, hipEventRecord(c->ev_wait, st));
        for (;;) {                                   /* hipEventSynchronize spins even on a blocking-sync event (measured: 6.1 busy cores per rank) */
            const hipError_t q = hipEventQuery(c->ev_wait);
            if (q == hipSuccess) return BRX_OK;
            if (q != hipErrorNotReady) return fail(c, BRX_E_HIP, "%s: %s", what, hipGetErrorString(q));
            usleep(40);
        }
    }
    int limit_ms = env_int("BRX_WATCHDOG_S", 15) * 1000;
    for (int ms = 0;; ms += 20) {
        hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return BRX_OK;
        if (e != hipErrorNotReady) return fail(c, BRX_E_HIP, "%s: %s", what, hipGetErrorString(e));
        if (ms >= limit_ms) {
            fprintf(stderr, "[brx] WATCHDOG: %s stalled; progress words:", what);
            for (int i = 0; i < 64; ++i) fprintf(stderr, "%s%u", (i % 8) ? " " : " | ", c->h_prog[i]);
            fprintf(stderr, "\n"); fflush(stderr);
            _exit(99);
        }
        usleep(20000);
    }
}

extern "C" int brx_last_read_cycles(brx_ctx *c, uint64_t *h_out, uint32_t n_reads) {
    if (!c || !h_out) return BRX_E_ARG;
    if (!c->d_clk || n_reads > c->clk_reads) return fail(c, BRX_E_STATE, "no per-read cycle counters for %u reads", n_reads);
    HIPCHK(c, hipMemcpy(h_out, c->d_clk, (size_t)n_reads * 64, hipMemcpyDeviceToHost));
    return BRX_OK;
}

extern "C" int brx_last_phase_cycles(brx_ctx *c, uint64_t *h_out, uint32_t n_reads) {
    if (!c || !h_out) return BRX_E_ARG;
    if (!c->d_phase || n_reads > c->clk_reads) return fail(c, BRX_E_STATE, "no phase counters for %u reads", n_reads);
    HIPCHK(c, hipMemcpy(h_out, c->d_phase, (size_t)n_reads * 64, hipMemcpyDeviceToHost));
    return BRX_OK;
}

extern "C" int brx_set_kernel_timing(brx_ctx *c, int on) {
    if (!c) return BRX_E_ARG;
    if (on && !c->kev_b[0]) {
        HIPCHK(c, hipSetDevice(c->device));
        for (int i = 0; i < BRX_KEV_MAX; ++i) {
            HIPCHK(c, hipEventCreate(&c->kev_b[i]));
            HIPCHK(c, hipEventCreate(&c->kev_e[i]));
        }
    }
    c->ktiming = on ? 1 : 0;
    return BRX_OK;
}
extern "C" int brx_last_kernel_stats(const brx_ctx *c, brx_kernel_stat out[BRX_KERN_COUNT]) {
    if (!c || !out) return BRX_E_ARG;
    for (int i = 0; i < BRX_KERN_COUNT; ++i) out[i] = c->kstat[i];
    return BRX_OK;
}
/* bracket one launch (or a short group of launches) on `stream` with an event pair of kernel class `kind` */
struct KTimer {
    brx_ctx *c; hipStream_t st; int slot;
    KTimer(brx_ctx *c_, int kind, hipStream_t st_) : c(c_), st(st_), slot(-1) {
        if (!c->ktiming) return;
        if (c->kev_n >= BRX_KEV_MAX) { c->kev_dropped += 1; return; }
        slot = c->kev_n++;
        c->kev_kind[slot] = (uint8_t)kind;
        (void)hipEventRecord(c->kev_b[slot], st);
    }
    ~KTimer() { if (slot >= 0) (void)hipEventRecord(c->kev_e[slot], st); }
};
#define BRX_PASTE_(a, b) a##b
#define BRX_PASTE(a, b) BRX_PASTE_(a, b)
#define KTIMED(kind, stream) KTimer BRX_PASTE(ktimer_, __LINE__)(c, (kind), (stream))

extern "C" uint32_t brx_last_mutate_passes(const brx_ctx *c) { return c ? c->mutate_passes : 0; }
extern "C" uint32_t brx_last_final_launches(const brx_ctx *c) { return c ? c->final_launches : 0; }
extern "C" uint32_t brx_last_window_misses(const brx_ctx *c) { return c ? c->window_misses : 0; }

/* Small transfers between the arena and the context's pinned blocks, as a kernel on the stream: one wave for a few words, a few
   dozen for the read states.  (The runtime's copy is a blit kernel with its own launch geometry; VERDICT r4: 1495 dispatches,
   10.8 % of the summed kernel time of the bench, 3.65 ms each in the six-batch mix against 15 us alone.) */
#define BRX_COPY_KERNEL_MAX ((size_t)1 << 20)       /* larger transfers go through hipMemcpyAsync (pinned on the host side: a DMA) */
__global__ void __launch_bounds__(64) k_copy_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 64 + threadIdx.x; i < n; i += (size_t)gridDim.x * 64) dst[i] = src[i];
}
static uint8_t *pinned_alias(brx_ctx *c, const void *h) {        /* device view of an address inside h_totals or h_stage, nullptr otherwise */
    const uint8_t *p = (const uint8_t *)h;
    const uint8_t *t = (const uint8_t *)c->h_totals;
    if (p >= t && p < t + 16 * sizeof(uint64_t) + 80 * sizeof(uint32_t)) return c->d_totals_alias + (p - t);
    if (c->h_stage && p >= c->h_stage && p < c->h_stage + c->stage_bytes) return c->d_stage + (p - c->h_stage);
    return nullptr;
}
/* device -> pinned host (bytes a multiple of 4); the host reads the block after waiting for the stream */
static int to_host(brx_ctx *c, hipStream_t st, void *h_dst, const void *d_src, size_t bytes) {
    /* the read states of a batch (10 MB, three times per batch) stay with the runtime's copy engine: as a kernel over PCIe they cost
       configs[4], whose batches take 0.4 s, 1.5 % (profiles/r05g); the kernels are for the few-word read-backs that sat behind blits */
    uint8_t *alias = (bytes > BRX_COPY_KERNEL_MAX) ? nullptr : pinned_alias(c, h_dst);
    if (!alias || (bytes & 3)) { HIPCHK(c, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st)); return BRX_OK; }
    const size_t n = bytes / 4;
    hipLaunchKernelGGL(k_copy_words, dim3((unsigned)std::min<size_t>((n + 255) / 256, 128)), dim3(64), 0, st, (uint32_t *)alias, (const uint32_t *)d_src, n);
    return BRX_OK;
}
/* pinned host -> device; the host block must not change until the stream has been waited for */
static int to_device(brx_ctx *c, hipStream_t st, void *d_dst, const void *h_src, size_t bytes) {
    uint8_t *alias = (bytes > BRX_COPY_KERNEL_MAX) ? nullptr : pinned_alias(c, h_src);
    if (!alias || (bytes & 3)) { HIPCHK(c, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, st)); return BRX_OK; }
    const size_t n = bytes / 4;
    hipLaunchKernelGGL(k_copy_words, dim3((unsigned)std::min<size_t>((n + 255) / 256, 128)), dim3(64), 0, st, (uint32_t *)d_dst, (const uint32_t *)alias, n);
    return BRX_OK;
}
/* (*h, *d) becomes a fresh pinned block of `want` bytes and its device view; what it held is gone.  The callers decide when to grow and
   by how much; nothing of the context may be in flight. */
static int pinned_regrow(brx_ctx *c, uint8_t **h, uint8_t **d, size_t *have, size_t want) {
    if (*h) { (void)hipHostFree(*h); *h = nullptr; *d = nullptr; *have = 0; }
    HIPCHK(c, hipHostMalloc((void **)h, want, hipHostMallocMapped));
    void *dp = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dp, *h, 0));
    *d = (uint8_t *)dp; *have = want;
    return BRX_OK;
}
/* the staging block holds at least `bytes` (grown between batches only), in whole megabytes */
static int stage_reserve(brx_ctx *c, size_t bytes) {
    if (c->stage_bytes >= bytes) return BRX_OK;
    return pinned_regrow(c, &c->h_stage, &c->d_stage, &c->stage_bytes, (bytes + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1));
}

static int read_totals(brx_ctx *c, hipStream_t st, const uint64_t *d_totals, int n) {
    { int rc_ = to_host(c, st, c->h_totals, d_totals, (size_t)n * sizeof(uint64_t)); if (rc_) return rc_; }
    return wait_stream(c, st, "pipeline stage");
}

static int scratch_short(brx_ctx *c, size_t needed) {
    c->scratch_needed = needed;
    return fail(c, BRX_E_SCRATCH, "scratch arena too small: need about %zu bytes, have %zu", needed, c->scratch_bytes);
}

/* ---------------------------------------------------------------------------------------------
 * the shared pipeline: plan (or raw fragments) -> build -> mutate -> final -> records
 * ------------------------------------------------------------------------------------------- */

/* One set of reads of the final stage: a range of `order` with its streams and its region of the arena */
struct FinalSet {
    uint32_t b, e;                 /* range of `order` */
    hipStream_t st, wide;          /* its stream; the stream of the widest band class (may be the same) */
    int id;                        /* 0 head, 1 bulk: selects counter slots and events */
    bool launched, wide_forked;
    bool use_lanes, use_quad;      /* its reads flagged for k_fin_lanes / k_fin_quad take those kernels (decided once, in start_final) */
    size_t tb_at, tb_cap;          /* the slabs of the phase last launched, in the arena (phase 1 takes phase 0's again when that is the larger room) */
    uint64_t bases[FC_COUNT];      /* kernel statistics: bases by the kernel that aligns them (the giants count as FC_WIDE) */
};

/* Queue heads of the final stage: FQ_WORDS words of `counters` per (set, phase).  A class's align kernel pops its list with a
   64-bit counter (two words: list position, waves started), its k_fin_qscore with one word; FC_WIDE and FC_GIANT are scored
   together, over the set's range of `order`. */
enum {
    FQ_ALIGN_W1 = 0, FQ_ALIGN_W2 = 2, FQ_ALIGN_W4 = 4, FQ_ALIGN_WIDE = 6, FQ_SCORE_W1 = 8, FQ_SCORE_WIDE = 9, FQ_SCORE_W2 = 10, FQ_SCORE_W4 = 11,
    FQ_ALIGN_LANES = 12, FQ_SCORE_LANES = 14, FQ_ALIGN_QUAD = 16, FQ_SCORE_QUAD = 20, FQ_ALIGN_GIANT = 22, FQ_WORDS = 32
};
static constexpr uint32_t fq_align[FC_COUNT] = {FQ_ALIGN_W1, FQ_ALIGN_W2, FQ_ALIGN_W4, FQ_ALIGN_WIDE, FQ_ALIGN_LANES, FQ_ALIGN_QUAD, FQ_ALIGN_GIANT};
static constexpr uint32_t fq_score[FC_COUNT] = {FQ_SCORE_W1, FQ_SCORE_W2, FQ_SCORE_W4, FQ_SCORE_WIDE, FQ_SCORE_LANES, FQ_SCORE_QUAD, FQ_SCORE_WIDE};
static_assert(FQ_ALIGN_GIANT + 2 <= FQ_WORDS, "the last queue head of a (set, phase) lies inside its FQ_WORDS words");
static constexpr int fin_kern[FC_COUNT] = {BRX_KERN_FIN_ALIGN1, BRX_KERN_FIN_ALIGN2, BRX_KERN_FIN_ALIGN4, BRX_KERN_FIN_ALIGN16, BRX_KERN_FIN_LANES, BRX_KERN_FIN_QUAD1, BRX_KERN_FIN_ALIGN16};    /* kernel statistics */

/* One call of brx_simulate_batch / brx_sequence_fragments: the arena, what is carved from it, the two sets, and the steps in
   the order run() takes them. */
struct Batch {
    brx_ctx *c; uint64_t seed, first_read; uint32_t n_reads; bool raw;
    const uint8_t *d_frags; const uint64_t *d_frag_off; const double *d_target;
    uint8_t *d_out; size_t out_cap; brx_read_stats *d_stats; size_t *out_bytes; hipStream_t st;
    BrxDev dev; Arena A;
    uint32_t nb64, side_waves, lane_waves, tail_eff;
    bool all_head;                 /* the whole batch in one run-to-completion launch: no k_mut_lanes, no passes, none of their buffers */
    /* pinned staging (offsets into c->h_stage): read states, order, and the final stage's tables (read lists, slab tables) of one set at a time */
    size_t stg_rs, stg_order, stg_lists, stg_slabs, stg_aux;
    RS *h_rs; uint32_t *h_order; MutAux *h_aux;
    /* carved from the arena */
    RS *rs; uint64_t *totals; uint32_t *order, *counters; uint64_t *fin_slabs; uint32_t *fin_lists; uint64_t *clk, *phase_clk;
    PSeg *segs; PPiece *pieces; uint8_t *Fbuf; uint32_t *repl, *F2buf, *Cbuf;
    uint8_t *win, *win_head, *winbuf; MS *msv; uint32_t *mctr, *active_a, *active_b, *req_easy, *lane_cls, *req_hard, *req_legacy, *req_legacy_head;
    MutAux *aux_dev; uint2 *lane_tb; PQ *pq; uint4 *sv_a; uint32_t *sv_z;
    /* the two chains */
    uint32_t n_mh, n_mb, n_head, n_bulk; hipStream_t s_head;
    FinalSet sets[2];
    bool legacy_handled;           /* the whole-read fallback already ran for every read (no separate mutate head chain) */
    uint64_t tail_bases, rec_bytes;     /* kernel statistics: bases of the bulk reads that finished in the in-place tail; bytes of the records */

    int fetch_rs(hipStream_t s_) { return to_host(c, s_, h_rs, rs, (size_t)n_reads * sizeof(RS)); }
    uint32_t *h_ctr() const { return reinterpret_cast<uint32_t *>(c->h_totals + 8); }          /* pinned */
    /* counters: [0],[3] join queues of head / bulk; [1] flags; [2],[4] window misses of head / bulk; [5] overflow lists of the plan;
       [16 + FQ_WORDS x (set x 2 + phase)] final-stage queue heads */
    uint32_t *miss_counter(const FinalSet &S) const { return counters + (S.id ? 4 : 2); }
    uint32_t *set_lists(const FinalSet &S) const { return fin_lists + S.b; }                   /* the set's share of the final stage's device tables */
    uint64_t *set_slabs(const FinalSet &S) const { return fin_slabs + S.b + 8 * (size_t)S.id; }
    uint32_t set_waves(const FinalSet &S) const { return (uint32_t)std::min<uint64_t>(S.e - S.b, (uint64_t)c->n_cu * (uint64_t)c->waves_per_cu); }
    uint32_t *fin_queue(const FinalSet &S, int phase) const { return counters + 16 + FQ_WORDS * ((size_t)S.id * 2 + (size_t)phase); }
    int read_pass_counts(uint32_t *ctr) { const int rc_ = to_host(c, st, h_ctr(), ctr, MC_WORDS * sizeof(uint32_t)); return rc_ ? rc_ : wait_stream(c, st, "mutate pass"); }     /* blocking: a pass's counter block in h_ctr() */

    /* the steps, in the order run() takes them */
    int run(); int layout_and_plan(); int build(); int prepare_chains();
    void launch_run(hipStream_t s, uint32_t count, const uint32_t *act_in, const uint32_t *n_in, uint32_t *ctr, const MutAux *aux);
    int head_chain(); int bulk_chain_lanes(); int bulk_chain_passes(); int single_chain_legacy();
    int start_final(FinalSet &S); int launch_final_phase(FinalSet &S, int phase);
    void align_class(const FinalSet &S, const FinPlan &P, int phase, int k, hipStream_t s, bool score); void score_wide(const FinalSet &S, int phase, hipStream_t s);
    int finish_final(FinalSet &S); int records(); int kernel_statistics();
};

/* arena layout up to the mutate stage, and the plan stage */
int Batch::layout_and_plan() {
    dev = c->dev;
    dev.seed = seed; dev.first_read = first_read; dev.n_reads = n_reads; dev.raw_mode = raw ? 1u : 0u;
    dev.tb_hmul = c->tb_hmul;
    A.base = c->scratch; A.cap = c->scratch_bytes; A.used = 0; A.top = 0;
    nb64 = (n_reads + 63) / 64;
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    stg_rs = 0; stg_order = stg_rs + pad((size_t)n_reads * sizeof(RS)); stg_lists = stg_order + pad((size_t)n_reads * 4);
    stg_slabs = stg_lists + pad((size_t)n_reads * 4); stg_aux = stg_slabs + pad(((size_t)n_reads + 64) * 8);
    { int rcs_ = stage_reserve(c, stg_aux + 4096); if (rcs_) return rcs_; }
    h_order = reinterpret_cast<uint32_t *>(c->h_stage + stg_order);      /* pinned: filled by k_copy_words */
    h_rs = reinterpret_cast<RS *>(c->h_stage + stg_rs);
    h_aux = reinterpret_cast<MutAux *>(c->h_stage + stg_aux);            /* pinned; its copy is waited for with the mutate counters */
    rs = (RS *)A.take((size_t)n_reads * sizeof(RS));
    totals = (uint64_t *)A.take(16 * sizeof(uint64_t));
    order = (uint32_t *)A.take((size_t)n_reads * 4);
    counters = (uint32_t *)A.take(4096 * 4);
    fin_slabs = (uint64_t *)A.take(((size_t)n_reads + 32) * 8);             /* slab offset tables of the sets' align kernels (n_reads + 16 words) */
    fin_lists = (uint32_t *)A.take(((size_t)n_reads + 32) * 4);             /* class-pure read lists of the final align kernels */
    clk = (uint64_t *)A.take((size_t)n_reads * 64);       /* per-read cycle counters, brx_last_read_cycles() */
    phase_clk = (uint64_t *)A.take((size_t)n_reads * 64);     /* mutate phase cycles (BRX_PROFILE=1), brx_last_phase_cycles() */
    PSeg *plan_ovf = (PSeg *)A.take((size_t)BRX_OVF_LISTS * BRX_OVF_SEGS * sizeof(PSeg));
    if (!A.ok()) return scratch_short(c, A.used + (size_t)n_reads * 200000);
    dev.plan_ovf = plan_ovf; dev.plan_ovf_ctr = counters + 5;
    HIPCHK(c, hipMemsetAsync(counters, 0, 4096 * 4, st));
    HIPCHK(c, hipMemsetAsync(totals, 0, 16 * 8, st));
    HIPCHK(c, hipMemsetAsync(clk, 0, (size_t)n_reads * 64, st));
    HIPCHK(c, hipMemsetAsync(phase_clk, 0, (size_t)n_reads * 64, st));
    c->d_clk = clk; c->d_phase = phase_clk; c->clk_reads = n_reads;
    c->kev_n = 0; c->kev_dropped = 0;
    memset(c->kstat, 0, sizeof(c->kstat));

    /* ---- stage: plan ---- */
    HIPCHK(c, hipEventRecord(c->ev_b[BRX_STAGE_PLAN], st));
    {
        KTIMED(BRX_KERN_PLAN, st);
        if (raw) hipLaunchKernelGGL(k_init_raw, dim3(nb64), dim3(64), 0, st, dev, rs, d_frag_off, d_target);
        else hipLaunchKernelGGL(k_plan_count, dim3(nb64), dim3(64), 0, st, dev, rs);
        hipLaunchKernelGGL(k_scan_plan, dim3(1), dim3(64), 0, st, n_reads, rs, totals);
    }
    uint32_t *h_small = c->h_prog + 64;                 /* 16 pinned words for one-word read-backs */
    { int rc_ = to_host(c, st, h_small, counters + 5, 4); if (rc_) return rc_; }
    { int rc_ = read_totals(c, st, totals, 3); if (rc_) return rc_; }
    const uint32_t h_ovf = h_small[0];
    if (h_ovf > BRX_OVF_LISTS)       /* the sizing pass ran out of overflow lists: the fill pass could overflow OTHER reads */
        return fail(c, BRX_E_INTERNAL, "%u reads of one batch have more than %d base segments (chimera joins): only %d overflow lists",
                    h_ovf, BRX_MAX_BASE_SEGS, BRX_OVF_LISTS);
    HIPCHK(c, hipMemsetAsync(counters + 5, 0, 4, st));          /* the fill pass takes the same lists again */
    const uint64_t tot_segs = c->h_totals[0], tot_pieces = c->h_totals[1], f_bytes = c->h_totals[2];
    segs = (PSeg *)A.take((size_t)(tot_segs + 1) * sizeof(PSeg));
    pieces = (PPiece *)A.take((size_t)(tot_pieces + 1) * sizeof(PPiece));
    Fbuf = (uint8_t *)A.take((size_t)f_bytes + 64);
    repl = (uint32_t *)A.take(((size_t)f_bytes + 64) * 4);
    F2buf = (uint32_t *)A.take(((size_t)f_bytes / 16 + 16) * 4);       /* the fragments as 2-bit codes: word F_off / 16 (k_build) */
    Cbuf = (uint32_t *)A.take(((size_t)f_bytes / 16 + 16) * 4);        /* a bit per base: replaced (same index) */
    side_waves = std::min<uint32_t>(n_reads, 4096u);                    /* wave-level window aligner / legacy */
    tail_eff = c->tail_reads != 0xFFFFFFFFu ? c->tail_reads : std::max<uint32_t>(1024u, n_reads / 8u);
    all_head = n_reads <= tail_eff;
    lane_waves = all_head ? 0u : std::min<uint32_t>((n_reads + 63) / 64, c->mutate_passes_route ? 512u : (uint32_t)BRX_LANES_MAX_WAVES);   /* lane-level window aligner: one 6.4 MB store of move codes per wave */
    win = (uint8_t *)A.take_top((size_t)(side_waves + 1) * c->win_bytes);      /* one slot per wave (mutate chain on the caller's stream only: top region) */
    msv = (MS *)A.take((size_t)n_reads * sizeof(MS));
    mctr = (uint32_t *)A.take(8 * MC_WORDS * sizeof(uint32_t));   /* pass counters 0/1, 2 first bulk input, 3 bulk legacy, 4 head input, 5 head legacy, 6 head pass */
    active_a = (uint32_t *)A.take((size_t)n_reads * 4);
    active_b = (uint32_t *)A.take((size_t)n_reads * 4);
    req_easy = (uint32_t *)A.take((size_t)n_reads * 4 * BRX_LANE_CLASSES);    /* lane passes: one list per band-width class */
    lane_cls = (uint32_t *)A.take(2 * MC_WORDS * BRX_CLS_STRIDE * sizeof(uint32_t));             /* their counts, a block per pass parity */
    aux_dev = (MutAux *)A.take(2 * sizeof(MutAux));                               /* [0] bulk chain, [1] head chain: what k_mutate_seg reads where it uses it */
    req_hard = (uint32_t *)A.take((size_t)n_reads * 4);
    req_legacy = (uint32_t *)A.take((size_t)n_reads * 4);
    req_legacy_head = (uint32_t *)A.take((size_t)n_reads * 4);
    winbuf = (uint8_t *)A.take((size_t)n_reads * BRX_WIN_STRIDE + 64);
    lane_tb = (uint2 *)A.take_top((size_t)lane_waves * BRX_LANE_TB_UNITS * sizeof(uint2));
    /* the bulk passes' survivor rings (brx_passes.h): 20 bytes per entry, BRX_SV_CAP entries per read */
    pq = (PQ *)A.take((size_t)n_reads * sizeof(PQ));
    /* k_mut_lanes: ring of read r at F_off / 8 + 128 r, n / 8 + 128 entries (brx_ring_base); the passes: BRX_SV_CAP entries per read */
    const size_t sv_entries = all_head ? 256 : c->mutate_passes_route ? (size_t)n_reads * BRX_SV_CAP : ((size_t)f_bytes >> BRX_RING_SHIFT) + (size_t)BRX_RING_MIN * (size_t)n_reads + 256;
    sv_a = (uint4 *)A.take_top(sv_entries * sizeof(uint4));
    sv_z = (uint32_t *)A.take_top(sv_entries * sizeof(uint32_t));
    if (!A.ok()) return scratch_short(c, A.used + (A.top <= A.cap ? A.top : (size_t)lane_waves * BRX_LANE_TB_UNITS * sizeof(uint2) + (size_t)(side_waves + 1) * c->win_bytes + sv_entries * 20) + (size_t)f_bytes * 6 + ((size_t)1 << 28));
    if (!raw) { KTIMED(BRX_KERN_PLAN, st); hipLaunchKernelGGL(k_plan_fill, dim3(nb64), dim3(64), 0, st, dev, rs, segs, pieces); }
    HIPCHK(c, hipEventRecord(c->ev_e[BRX_STAGE_PLAN], st));
    return BRX_OK;
}

/* ---- stage: build ---- */
int Batch::build() {
    HIPCHK(c, hipEventRecord(c->ev_b[BRX_STAGE_BUILD], st));
    if (raw) hipLaunchKernelGGL(k_copy_frags, dim3(n_reads), dim3(64), 0, st, dev, rs, d_frags, d_frag_off, Fbuf);
    { KTIMED(BRX_KERN_BUILD, st); hipLaunchKernelGGL(k_build, dim3(n_reads), dim3(64), 0, st, dev, rs, segs, Fbuf, repl, F2buf, Cbuf); }
    hipLaunchKernelGGL(k_order, dim3(1), dim3(64), 0, st, n_reads, rs, order);
    HIPCHK(c, hipEventRecord(c->ev_e[BRX_STAGE_BUILD], st));
    return BRX_OK;
}

/* ---- stages: mutate + final, as TWO CHAINS per batch ------------------------------------------------------
 * `order` lists the reads by expected changes, most first (and, inside a bucket of equal work, by error rate).  The first
 * n_head of them (the HEAD set: BRX_HEAD_READS, default 1024) are the batch's critical path: a 150 kb read is ~300 dependent
 * {mutate segment, window alignment} cycles and then a final alignment with 8-16 band words per lane.  They run on the
 * side stream from the start: one launch of k_mutate_seg takes each of them to completion with in-place window
 * alignments, and their final alignment + qscores follow on that stream as soon as they are done.  The BULK set
 * (everything else) runs beside them on the caller's stream: k_mut_fill, ONE launch of k_mut_lanes (a wave keeps 64 reads
 * through their first BRX_LANES_CYCLES alignment cycles), k_mutate_seg for what is left, k_mut_epilogue -- or, under
 * BRX_MUTATE_PASSES=1, host-driven passes with an in-place tail -- then its own final stage.  The chains share nothing but
 * read-only inputs and the arena's bump allocator (host side), and join before the records are written.  A batch that is
 * small (n_reads <= BRX_TAIL_READS) is all head.  (Round 1 ran the sets one after the other:
 * bulk passes, THEN the in-place tail, THEN all final kernels -- 930 ms per batch with 8 batches in flight, of
 * which 230 ms tail and 270 ms wide-band alignments during which the batch used a few dozen waves.)
 *
 * prepare_chains: the split into sets, the chains' cold arguments and first counters */
int Batch::prepare_chains() {
    c->final_launches = 0; c->window_misses = 0;
    /* n_mh: reads the mutate HEAD chain takes (BRX_HEAD_READS, default 1024; 0 = every read goes through the passes);
       n_head: the head set of the FINAL stage (the mutate head set when that chain is on, because its final stage starts
       when its own reads are mutated; else BRX_FIN_HEAD_READS).  Measured on configs[3], 8 batches in flight
       (profiles/README.md r02g/r02h): head 1024 + tail 1024 2.08 Gbases/s, head 2048 + tail 2048 2.01, no head chain and a
       64-read tail (218 passes, the small ones with the packed window aligner) 1.63, 512-read tail 1.82 -- a pass costs
       1.5-2.6 ms beside the other batches' kernels whatever it aligns, an in-place cycle 0.3-0.6 ms. */
    n_mh = all_head ? n_reads : std::min<uint32_t>(c->head_reads, n_reads);
    n_mb = n_reads - n_mh;
    n_head = n_mh ? n_mh : (n_reads <= 2 * c->fin_head_reads ? 0u : c->fin_head_reads);
    n_bulk = n_reads - n_head;
    if (n_mh && n_mb) {
        win_head = (uint8_t *)A.take((size_t)(std::min(n_mh, side_waves) + 1) * c->win_bytes);
        if (!A.ok()) return scratch_short(c, A.used + A.top + ((size_t)1 << 28));
    } else win_head = win;
    s_head = n_bulk ? c->side : st;            /* an all-head batch stays on the caller's stream */
    h_aux[0] = MutAux{req_easy, req_hard, req_legacy, mctr + 3 * MC_WORDS, winbuf, clk, win, (uint64_t)c->win_bytes, counters + 1, phase_clk};
    h_aux[1] = MutAux{req_easy, req_hard, req_legacy_head, mctr + 5 * MC_WORDS, winbuf, clk, win_head, (uint64_t)c->win_bytes, counters + 1, phase_clk};
    { int rc_ = to_device(c, st, aux_dev, h_aux, 2 * sizeof(MutAux)); if (rc_) return rc_; }
    /* (Round 4 also ran THREE sets -- the reads with the fewest expected changes as an EARLY set whose final stage started
       during the passes on the head chain's idle stream, every early read counting itself when its loop was done.  It overlapped
       as designed -- final stage behind the mutate stage 250 -> 205 ms -- and the passes it ran beside slowed down by as much:
       5.16-5.18 against 5.22-5.26 Gbases/s without it, six batches in flight; removed.  profiles/r04i, r04j.) */
    sets[0] = FinalSet{0, n_head, s_head, (c->wide_stream && n_bulk) ? c->side2 : s_head, 0, false, false, false, false, 0, 0, {}};
    sets[1] = FinalSet{n_head, n_reads, st, st, 1, false, false, false, false, 0, 0, {}};
    legacy_handled = false; tail_bases = 0;

    { int rc_ = to_host(c, st, h_order, order, (size_t)n_reads * 4); if (rc_) return rc_; }
    HIPCHK(c, hipMemsetAsync(msv, 0, (size_t)n_reads * sizeof(MS), st));
    HIPCHK(c, hipMemsetAsync(pq, 0, (size_t)n_reads * sizeof(PQ), st));
    HIPCHK(c, hipMemsetAsync(mctr, 0, 8 * MC_WORDS * sizeof(uint32_t), st));
    HIPCHK(c, hipMemsetAsync(lane_cls, 0, 2 * MC_WORDS * BRX_CLS_STRIDE * sizeof(uint32_t), st));
    memset(h_ctr(), 0, 2 * MC_WORDS * sizeof(uint32_t));
    h_ctr()[MC_OUT] = n_mb;                      /* block 2: "previous pass" of the first bulk pass */
    h_ctr()[MC_WORDS + MC_OUT] = n_mh;           /* block 4 (copied below): the head launch's input count */
    { int rc_ = to_device(c, st, mctr + 2 * MC_WORDS, h_ctr(), MC_WORDS * sizeof(uint32_t)); if (rc_) return rc_; }
    { int rc_ = to_device(c, st, mctr + 4 * MC_WORDS, h_ctr() + MC_WORDS, MC_WORDS * sizeof(uint32_t)); if (rc_) return rc_; }
    return wait_stream(c, st, "mutate counters");
}

/* reads taken to completion in ONE launch (the head set from the start; the last BRX_TAIL_READS of the bulk set):
   k_mutate_seg, every read aligning its own windows with a whole wave.  (Rounds 2 and 3 measured three ways of
   taking these windows to a cheaper aligner -- workgroups of 8 reads with packed alignments, 8-wave pass kernels, a
   persistent launch with device queues -- and every one lost to this chain on the batch's critical path: DESIGN.md section 7.) */
void Batch::launch_run(hipStream_t s, uint32_t count, const uint32_t *act_in, const uint32_t *n_in, uint32_t *ctr, const MutAux *aux) {
    KTIMED(BRX_KERN_MUTATE_RUN, s);
#define BRX_LAUNCH_RUN(PROF)                                                                                                        \
    hipLaunchKernelGGL((k_mutate_seg<PROF, BRX_SEG_WPS>), dim3(std::min(count, side_waves)), dim3(64), 0, s, dev, rs, msv, act_in, n_in,   \
                       ctr, aux, Fbuf, repl, F2buf, Cbuf)
    if (c->profile) BRX_LAUNCH_RUN(true); else BRX_LAUNCH_RUN(false);
#undef BRX_LAUNCH_RUN
}

/* ---- head chain: mutate to completion ---- */
int Batch::head_chain() {
    if (n_mb) {
        HIPCHK(c, hipEventRecord(c->ev_fork, st));
        HIPCHK(c, hipStreamWaitEvent(s_head, c->ev_fork, 0));
    }
    launch_run(s_head, n_mh, order, mctr + 4 * MC_WORDS + MC_OUT, mctr + 6 * MC_WORDS, aux_dev + 1);
    if (n_mb) HIPCHK(c, hipEventRecord(c->ev_head_mut, s_head));
    c->mutate_passes = 1;
    return BRX_OK;
}

/* ---- bulk chain, round 6b: ONE launch -- a wave keeps 64 reads (neighbours in the order by expected changes) from the first
   iteration to the last (k_mut_lanes); their survivors are proposed ahead, all of them, by k_mut_fill; the epilogues follow ---- */
int Batch::bulk_chain_lanes() {
    const uint32_t post_waves = std::min<uint64_t>(n_mb, (uint64_t)c->n_cu * 32u);
    const uint32_t groups = (n_mb + 63u) / 64u;
    { KTIMED(BRX_KERN_MUT_POST, st); hipLaunchKernelGGL((k_mut_fill<BRX_POST_U>), dim3(post_waves), dim3(64), 0, st, dev, rs, pq, order + n_mh, n_mb, Fbuf, F2buf, Cbuf, sv_a, sv_z); }
    uint32_t *left_ctr = mctr + MC_OUT;                 /* block 0: [MC_QUEUE] the tail's queue, [MC_OUT] reads the lane kernel leaves */
    {   KTIMED(BRX_KERN_MUTATE_SEG, st);
#define BRX_LAUNCH_LANES(PROF)                                                                                                                                  \
        hipLaunchKernelGGL((k_mut_lanes<BRX_POST_U, PROF>), dim3(std::min(groups, lane_waves)), dim3(64), 0, st, dev, rs, msv, pq, order + n_mh, n_mb, h_aux[0], \
                           Fbuf, repl, F2buf, Cbuf, sv_a, sv_z, lane_tb, c->lanes_cycles ? c->lanes_cycles : 0xFFFFFFFFu, active_a, left_ctr)
        if (c->profile) BRX_LAUNCH_LANES(true); else BRX_LAUNCH_LANES(false);
#undef BRX_LAUNCH_LANES
    }
    if (c->lanes_cycles) {                             /* what is left of the reads with the most cycles: in place, one wave per read */
        launch_run(st, std::min<uint32_t>(n_mb, 8192u), active_a, left_ctr, mctr, aux_dev);
        c->mutate_passes += 1;
    }
    { KTIMED(BRX_KERN_MUT_POST, st); hipLaunchKernelGGL(k_mut_epilogue, dim3(post_waves), dim3(64), 0, st, dev, rs, msv, order + n_mh, n_mb, h_aux[0], Fbuf, repl); }
    c->mutate_passes += 1;
    return BRX_OK;
}

/* ---- bulk chain under BRX_MUTATE_PASSES=1: host-driven passes, then an in-place tail ---- */
int Batch::bulk_chain_passes() {
    const uint32_t post_waves = std::min<uint64_t>(n_mb, (uint64_t)c->n_cu * 32u);      /* k_mut_post: eight waves per SIMD, grid-stride over the pass's reads */
    const uint32_t *n_in = mctr + 2 * MC_WORDS + MC_OUT;
    const uint32_t *act_in = order + n_mh;
    uint32_t n_up = n_mb, pass = 0;
    const uint32_t tail_reads = tail_eff;   /* this few reads left: run them to completion in place (no host round trips) */
    for (; n_up > 0 && pass < (1u << 20); ++pass) {
        uint32_t *ctr = mctr + (pass & 1u) * MC_WORDS;
        uint32_t *act_out = (pass & 1u) ? active_b : active_a;
        /* ctr (this pass's counter block) was zeroed by the previous pass's k_win_wave -- by the memset before the loop for
           passes 0 and 1 -- instead of a fill kernel per pass on the batch's critical path */
        if (n_up <= tail_reads) {
            if (c->ktiming) {
                std::vector<uint32_t> h_act(n_up);
                HIPCHK(c, hipMemcpyAsync(h_act.data(), act_in, (size_t)n_up * 4, hipMemcpyDeviceToHost, st));
                { int rc_ = fetch_rs(st); if (rc_) return rc_; }
                HIPCHK(c, hipStreamSynchronize(st));
                for (uint32_t x : h_act) if (x < n_reads) tail_bases += h_rs[x].n;
            }
            launch_run(st, n_up, act_in, n_in, ctr, aux_dev);
            { int rc_ = read_pass_counts(ctr); if (rc_) return rc_; }
            n_up = h_ctr()[MC_OUT];                   /* 0 unless a window overflowed its slot (then: legacy list) */
            ++pass;
            break;
        }
        /* round 6 (brx_passes.h): the survivors of a read are applied by ONE LANE from the read's ring (k_mut_apply), a
           wave per read parks the window and proposes ahead (k_mut_post), the lists are appended by wave (k_pass_lists) */
        if (pass == 0) {                       /* the first rings: every bulk read is "not started" */
            KTIMED(BRX_KERN_MUT_POST, st);
            hipLaunchKernelGGL((k_mut_post<BRX_POST_U>), dim3(std::min(post_waves, n_up)), dim3(64), 0, st, dev, rs, msv, pq, act_in, n_in,
                               h_aux[0], Fbuf, repl, F2buf, Cbuf, sv_a, sv_z);
        }
        { KTIMED(BRX_KERN_MUTATE_SEG, st); hipLaunchKernelGGL(k_mut_apply, dim3((n_up + 63u) / 64u), dim3(64), 0, st, dev, rs, msv, pq, act_in, n_in, sv_a, sv_z, repl, Cbuf); }
        {
            KTIMED(BRX_KERN_MUT_POST, st);
            hipLaunchKernelGGL((k_mut_post<BRX_POST_U>), dim3(std::min(post_waves, n_up)), dim3(64), 0, st, dev, rs, msv, pq, act_in, n_in,
                               h_aux[0], Fbuf, repl, F2buf, Cbuf, sv_a, sv_z);
            hipLaunchKernelGGL(k_pass_lists, dim3((n_up + 63u) / 64u), dim3(64), 0, st, msv, act_in, n_in, act_out, ctr,
                               lane_cls + (pass & 1u) * MC_WORDS * BRX_CLS_STRIDE, h_aux[0], n_reads);
        }
        {
            KTIMED(BRX_KERN_WIN_LANE, st);
            hipLaunchKernelGGL(k_win_lane, dim3(std::min(lane_waves, (n_up + 63) / 64 + BRX_LANE_CLASSES)), dim3(64), 0, st, msv, req_easy,
                               lane_cls + (pass & 1u) * MC_WORDS * BRX_CLS_STRIDE, n_reads, winbuf, lane_tb);
        }
        {   /* the windows the lane kernel does not take: one per wave; it also zeroes the counter block of the NEXT pass */
            KTIMED(BRX_KERN_WIN_WAVE, st);
            /* few windows take this kernel (symbols outside ACGT, very wide bands): 512 waves pull them from the queue; a grid of one
               wave per active read was 4096 waves that start only to find the queue empty, once per pass on the critical path */
            hipLaunchKernelGGL(k_win_wave, dim3(std::min(std::min(side_waves, 512u), n_up)), dim3(64), 0, st, msv, req_hard, ctr + MC_HARD,
                               ctr + 5, winbuf, win, (uint64_t)c->win_bytes, counters + 1, mctr + ((pass + 1) & 1u) * MC_WORDS,
                               lane_cls + ((pass + 1) & 1u) * MC_WORDS * BRX_CLS_STRIDE);
        }
        /* the active count only shrinks: look at it every 4th pass while it is large, every pass near the end */
        if (n_up <= 4 * std::min<uint32_t>(tail_reads, 48u) || n_up <= tail_reads + 64 || (pass & 3u) == 3u) {
            { int rc_ = read_pass_counts(ctr); if (rc_) return rc_; }
            n_up = h_ctr()[MC_OUT];
            /* the head set's final stage starts as soon as its reads are mutated */
            if (n_mh && !sets[0].launched && hipEventQuery(c->ev_head_mut) == hipSuccess) { int rc_ = start_final(sets[0]); if (rc_) return rc_; }
        }
        n_in = ctr + MC_OUT;
        act_in = act_out;
    }
    c->mutate_passes += pass;
    if (n_up > 0) return fail(c, BRX_E_INTERNAL, "mutate pipeline did not converge after %u passes", pass);
    /* the reads that finished inside the passes: their epilogues, once */
    { KTIMED(BRX_KERN_MUT_POST, st); hipLaunchKernelGGL(k_mut_epilogue, dim3(std::min(post_waves, n_mb)), dim3(64), 0, st, dev, rs, msv, order + n_mh, n_mb, h_aux[0], Fbuf, repl); }
    return BRX_OK;
}

/* one mutate chain for all reads (no head chain): the whole-read fallback (windows that did not fit a slot) runs here, for both
   final sets, and the head set's side stream waits for the whole mutate stage */
int Batch::single_chain_legacy() {
    uint32_t *legacy_ctr = mctr + 3 * MC_WORDS;
    { int rc_ = to_host(c, st, h_ctr(), legacy_ctr, 2 * sizeof(uint32_t)); if (rc_) return rc_; }
    { int rcw = wait_stream(c, st, "mutate stage"); if (rcw) return rcw; }
    if (h_ctr()[0] > 0)
        hipLaunchKernelGGL(k_mutate, dim3(std::min(side_waves, h_ctr()[0])), dim3(64), 0, st, dev, rs, req_legacy, legacy_ctr,
                           legacy_ctr + 1, Fbuf, repl, win, (uint64_t)c->win_bytes, counters + 1, clk);
    legacy_handled = true;
    if (n_head && n_bulk) {
        HIPCHK(c, hipEventRecord(c->ev_fork, st));
        HIPCHK(c, hipStreamWaitEvent(s_head, c->ev_fork, 0));
    }
    return BRX_OK;
}

/* a set whose mutate kernels are all enqueued on its stream: legacy fallback, sizes, join, phase 0 of the final stage */
int Batch::start_final(FinalSet &S) {
    const uint32_t ns = S.e - S.b;
    S.launched = true;
    if (ns == 0) return BRX_OK;
    uint32_t *legacy = mctr + (S.id ? 3 : 5) * MC_WORDS;                       /* [0] count, [1] queue */
    const int tot_dev = S.id ? 3 : 8, tot_host = S.id ? 3 : 6;                 /* two words of `totals` (k_scan_mut) and of the pinned h_totals per set */
    { int rc_ = to_host(c, S.st, h_ctr(), legacy, 2 * sizeof(uint32_t)); if (rc_) return rc_; }
    { int rc_ = to_host(c, S.st, h_ctr() + 2, counters + 1, 4); if (rc_) return rc_; }
    { int rcw = wait_stream(c, S.st, S.id ? "mutate stage (bulk)" : "mutate stage (head)"); if (rcw) return rcw; }
    if (h_ctr()[2] & 1u) {                              /* an in-loop alignment did not fit its window scratch */
        uint32_t w4[4] = {0, 0, 0, 0};
        (void)hipMemcpy(w4, counters + 9, sizeof(w4), hipMemcpyDeviceToHost);
        c->win_bytes *= 4;
        c->scratch_needed = c->scratch_bytes + (size_t)side_waves * c->win_bytes;
        return fail(c, BRX_E_SCRATCH, "window scratch too small (read %llu: window of %u x %u bases, edit bound %u): need about %zu bytes, have %zu",
                    (unsigned long long)(first_read + w4[0]), w4[1], w4[2], w4[3], c->scratch_needed, c->scratch_bytes);
    }
    /* reads whose window did not fit a slot: the whole-read kernel with the inline wave aligner */
    DBG("set %d: %u reads, %u to the whole-read kernel", S.id, ns, h_ctr()[0]);
    if (h_ctr()[0] > 0 && !legacy_handled)
        hipLaunchKernelGGL(k_mutate, dim3(std::min(S.id ? side_waves : std::min(std::max(n_mh, 1u), side_waves), h_ctr()[0])), dim3(64), 0, S.st, dev, rs,
                           S.id ? req_legacy : req_legacy_head, legacy, legacy + 1, Fbuf, repl, S.id ? win : win_head,
                           (uint64_t)c->win_bytes, counters + 1, clk);
    hipLaunchKernelGGL(k_scan_mut, dim3(1), dim3(64), 0, S.st, ns, rs, order + S.b, totals + tot_dev);
    { int rc_ = to_host(c, S.st, c->h_totals + tot_host, totals + tot_dev, 2 * sizeof(uint64_t)); if (rc_) return rc_; }
    { int rc_ = to_host(c, S.st, h_ctr() + 2, counters + 1, 4); if (rc_) return rc_; }
    { int rcw = wait_stream(c, S.st, "k_scan_mut"); if (rcw) return rcw; }
    if (h_ctr()[2] & 1u) {                              /* ... nor did an alignment of the whole-read kernel */
        c->win_bytes *= 4;
        return scratch_short(c, c->scratch_bytes + (size_t)side_waves * c->win_bytes);
    }
    /* every kernel of the mutate chain on the caller's stream has been waited for (a set on the side stream of a batch without a
       head chain waited for ev_fork, recorded behind them): its top region is free for what follows */
    if (S.st == st || !n_mh) A.release_top();
    const uint64_t seq_bytes = c->h_totals[tot_host], ops_bytes = c->h_totals[tot_host + 1];
    uint8_t *seqbuf = (uint8_t *)A.take((size_t)seq_bytes + 64);
    uint8_t *opsbuf = (uint8_t *)A.take((size_t)ops_bytes + 64);
    if (!A.ok()) return scratch_short(c, A.used + A.top + ((size_t)1 << 28));
    {   KTIMED(BRX_KERN_FIN_JOIN, S.st);
        hipLaunchKernelGGL(k_fin_join, dim3(std::min<uint64_t>(ns, (uint64_t)c->n_cu * 16u)), dim3(64), 0, S.st, dev, rs, order, S.b, S.e,
                           counters + (S.id ? 3 : 0), (uint64_t)(seqbuf - c->scratch), (uint64_t)(opsbuf - c->scratch), Fbuf, repl, pieces, c->scratch,
                           F2buf, c->fin_lanes, c->fin_quad);
    }
    { int rc_ = fetch_rs(S.st); if (rc_) return rc_; }
    { int rcw = wait_stream(c, S.st, "k_fin_join"); if (rcw) return rcw; }
    uint32_t n_quad = 0, n_lanes = 0;
    for (uint32_t i = S.b; i < S.e; ++i) if (const RS &r = h_rs[h_order[i]]; r.n) { n_quad += (r.klass & BRX_KL_QUAD) ? 1u : 0u; n_lanes += (r.klass & BRX_KL_LANES) ? 1u : 0u; }
    /* Four per wave pays when the class fills the chip: a group is as slow as its longest read plus four tracebacks, and a
       class of a few hundred groups is all tail.  configs[4] (1509 such reads beside 63 435 by lane) lost 4 % to it
       (17.2 against 17.9 Gbases/s, profiles/r05g); below BRX_QUAD_MIN_READS the set's reads keep to whole waves. */
    S.use_quad = n_quad >= c->quad_min_reads;
    /* The same for one read per lane: a wave is as slow as its longest read, computed by ONE lane.  configs[4]'s head set (the 1024
       reads with the most expected changes: its longest, 100-200 kb) holds a few hundred reads whose band fits the lane aligner --
       a handful of waves that run a 200 kb alignment lane-serially while the chip waits for the set (k_fin_lanes 197 -> 278 ms
       per batch, 18.7 -> 15.6 Gbases/s when the head grew from 512 reads, none of which qualified, to 1024).  Below
       BRX_LANES_MIN_READS a set's reads keep to whole waves (k_fin_align reads klass's band words: the flag is only a route). */
    S.use_lanes = n_lanes >= c->lanes_min_reads;
    return launch_final_phase(S, 0);
}

/* one phase of one set (phase 0: windowed store for every read; phase 1: full store for the misses): the room the set may take,
   its plan (brx_finplan.h), the plan's tables on the device, the kernels */
int Batch::launch_final_phase(FinalSet &S, int phase) {
    const uint32_t ns = S.e - S.b;
    size_t at = (A.used + 255) & ~(size_t)255;
    size_t left = A.room() > at ? A.room() - at : 0;              /* below the top region while the mutate chain on the caller's stream still runs */
    const size_t room_now = left;
    if (phase == 0) {
        /* The sets that are not started yet size themselves the same way from what is left.  What a set needs is not
           proportional to its bases -- the head set is 512 reads and the largest stores of the batch -- so the set being
           launched takes what it needs at full grids (the planner's loop) out of what is left after the reserve of the sets
           still to come, and never less than a quarter.
           (A first version shared by bases: the head set got 1.2 GB, its classes ran on 35 / 27 / 12 / 7 waves and the batch took
           three times as long -- profiles/r04f.) */
        uint64_t others = 0;
        for (const FinalSet &O : sets) {
            if (O.e <= O.b || O.launched || O.id == S.id) continue;
            for (uint32_t i = O.b; i < O.e; ++i) others += h_rs[h_order[i]].n;
        }
        /* (round 6: 18 bytes per base of the sets to come -- seq + ops 4, slabs 14 without col_of[] -- and those sets will find the top
           region released: the reserve is taken from what the arena holds THEN) */
        const size_t reserve = (size_t)others * 18u;
        const size_t later = c->scratch_bytes > at ? c->scratch_bytes - at : 0;
        left = std::max<size_t>(std::min<size_t>(left, later > reserve ? later - reserve : 0), left / 4);
    } else if (S.tb_cap > left) { at = S.tb_at; left = S.tb_cap; }      /* the set's own slab area is free again */
    const FinPlanCfg cfg{(uint32_t)c->n_cu, (uint32_t)c->waves_per_cu, c->tb_hmul, S.use_lanes, S.use_quad, BRX_GIANT_UNITS};
    const FinPlan P = brx_plan_final(h_rs, h_order, S.b, S.e, phase, cfg, left, room_now);
    DBG("final set %d phase %d: %u reads, classes %u/%u/%u/%u(+%u giant) + %u by lane + %u four per wave, slabs %u/%u/%u/%u(+%u) + %u + %u, need %.2f GB, left %.2f GB, arena used %.2f GB", S.id, phase, ns,
        P.cnt[FC_W1], P.cnt[FC_W2], P.cnt[FC_W4], P.cnt[FC_WIDE], P.cnt[FC_GIANT], P.cnt[FC_LANES], P.cnt[FC_QUAD],
        P.grid[FC_W1], P.grid[FC_W2], P.grid[FC_W4], P.grid[FC_WIDE], P.grid[FC_GIANT], P.grid[FC_LANES], P.grid[FC_QUAD],
        (double)P.need / 1e9, (double)(P.fits ? std::max<size_t>(left, (size_t)P.need) : left) / 1e9, (double)A.used / 1e9);
    if (!P.fits) return scratch_short(c, c->scratch_bytes + (size_t)(P.need - left) + ((size_t)1 << 28));
    if (at == ((A.used + 255) & ~(size_t)255)) (void)A.take((size_t)P.need);      /* (phase 1 in the set's own area takes nothing) */
    S.tb_at = at; S.tb_cap = (size_t)P.need;
    if (phase == 0) for (int k = 0; k < FC_COUNT; ++k) {
        c->final_launches += P.grid[k];     /* slabs = waves of the set's align kernels */
        for (uint32_t x = 0; x < P.cnt[k]; ++x) S.bases[k == FC_GIANT ? FC_WIDE : k] += h_rs[P.lists[P.list_at[k] + x]].n;
    }
    /* device tables, in the set's share [S.b, S.e) of the arena's arrays (set_lists / set_slabs): read lists (u32) and slab offsets (u64, in units) */
    if (P.slabs.size() > (size_t)ns + 8 || P.lists.size() > (size_t)ns) return fail(c, BRX_E_INTERNAL, "final stage: slab table larger than its staging area");
    /* through the pinned staging block (one set at a time: the wait below ends before the next set's tables are written) */
    if (!P.lists.empty()) {
        memcpy(c->h_stage + stg_lists, P.lists.data(), P.lists.size() * 4);
        int rc_ = to_device(c, S.st, set_lists(S), c->h_stage + stg_lists, P.lists.size() * 4); if (rc_) return rc_;
    }
    memcpy(c->h_stage + stg_slabs, P.slabs.data(), P.slabs.size() * 8);
    { int rc_ = to_device(c, S.st, set_slabs(S), c->h_stage + stg_slabs, P.slabs.size() * 8); if (rc_) return rc_; }
    { int rcw_ = wait_stream(c, S.st, "final stage tables"); if (rcw_) return rcw_; }

    /* The widest bands (8+ words per lane: a few dozen reads, each a chain of ~100 k column steps of ~2 us) go first, on
       the set's wide stream when it has one; then the other classes, each scored as soon as it is aligned. */
    const bool any_wide = P.cnt[FC_WIDE] || P.cnt[FC_GIANT];
    const bool fork = S.wide != S.st;
    if (fork) {
        HIPCHK(c, hipEventRecord(c->ev_fork2[S.id], S.st));
        HIPCHK(c, hipStreamWaitEvent(S.wide, c->ev_fork2[S.id], 0));
    }
    align_class(S, P, phase, FC_WIDE, S.wide, false);
    align_class(S, P, phase, FC_GIANT, S.wide, false);             /* ... and its giants behind them */
    if (fork) {
        /* ... and is scored there as well.  (Until round 5 the set's own stream waited for the wide stream at this point and
           scored the class itself: for the head set that stream is `side`, the wait was enqueued when the head's final stage
           was launched, and everything the BULK set later put on `side` -- its two-word class -- sat behind the head's
           widest alignments: 391 ms into a 454 ms batch alone on the chip, profiles/r05_batch_timeline.json.  The host waits
           for both streams in finish_final instead.) */
        if (any_wide) score_wide(S, phase, S.wide);
        HIPCHK(c, hipEventRecord(c->ev_join2[S.id], S.wide)); S.wide_forked = true;
    }
    /* The 4-, 2- and 1-word classes are independent (own lists, own slabs).  The bulk set spreads them over the head chain's two
       streams, which are idle by the time the bulk passes end (round 3 ran the three classes and their scoring one after the
       other on the set's stream: ~490 ms of the batch's critical path where the longest of them takes ~300). */
    const bool spread = c->fin_spread && S.id == 1 && sets[0].e > sets[0].b && c->side != S.st;
    hipStream_t cls_stream[3] = {S.st, spread ? c->side : S.st, spread ? c->side2 : S.st};
    if (spread) {
        HIPCHK(c, hipEventRecord(c->ev_fork3, S.st));
        HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork3, 0));
        HIPCHK(c, hipStreamWaitEvent(c->side2, c->ev_fork3, 0));
    }
    align_class(S, P, phase, FC_W4, cls_stream[2], true);
    /* (round 5: the by-lane and four-per-wave classes ran in front of the one-word class on the set's own stream -- 11 + 18 ms
       that the 85 ms of k_fin_align<1,1,1> waited for in a batch alone on the chip; behind the two- and four-word classes on
       the side streams they ended the batch instead -- the third stream is the head set's widest class's until 360 ms into a
       454 ms batch.  Both go IN FRONT of the two-word class: 35 + 44 ms beside the one-word class's 82.) */
    hipStream_t lanes_stream = (spread && P.cnt[FC_W1]) ? cls_stream[1] : cls_stream[0];
    align_class(S, P, phase, FC_LANES, lanes_stream, true);
    align_class(S, P, phase, FC_QUAD, lanes_stream, true);
    align_class(S, P, phase, FC_W2, cls_stream[1], true);
    align_class(S, P, phase, FC_W1, cls_stream[0], true);
    if (spread) {
        HIPCHK(c, hipEventRecord(c->ev_join3[0], c->side));
        HIPCHK(c, hipEventRecord(c->ev_join3[1], c->side2));
        HIPCHK(c, hipStreamWaitEvent(S.st, c->ev_join3[0], 0));
        HIPCHK(c, hipStreamWaitEvent(S.st, c->ev_join3[1], 0));
    }
    if (any_wide && !fork) score_wide(S, phase, S.st);
    return BRX_OK;
}

/* the align kernel of class k on stream s; score: ... and k_fin_qscore on its class-pure list as soon as it is aligned */
void Batch::align_class(const FinalSet &S, const FinPlan &P, int phase, int k, hipStream_t s, bool score) {
    if (!P.cnt[k]) return;
    const uint32_t *list = set_lists(S) + P.list_at[k];
    const uint64_t *slabs = set_slabs(S) + P.slab_at[k];
    uint32_t *cq = fin_queue(S, phase), *misses = miss_counter(S);
    unsigned long long *head = reinterpret_cast<unsigned long long *>(cq + fq_align[k]);
    uint8_t *slab_base = c->scratch + S.tb_at;
#define BRX_FIN_ALIGN(...) hipLaunchKernelGGL((k_fin_align<__VA_ARGS__>), dim3(P.grid[k]), dim3(64), 0, s, dev, rs, list, P.cnt[k], head, slabs, misses, phase, \
                                              Fbuf, c->scratch, c->scratch, slab_base, clk)
    {
        KTIMED(fin_kern[k], s);
        switch (k) {
        case FC_W1: BRX_FIN_ALIGN(1, 1, 1); break;
        case FC_W2: BRX_FIN_ALIGN(2, 2, 2); break;
        case FC_W4: BRX_FIN_ALIGN(4, 4, 4); break;
        case FC_WIDE: case FC_GIANT: BRX_FIN_ALIGN(16, 8, 0xFFFF); break;      /* the giants: same kernel, own queue, own few slabs */
        case FC_LANES:                               /* the narrow-band class, one read per lane: with pacbio2021 / --identity 30,3 nearly every read */
            hipLaunchKernelGGL(k_fin_lanes, dim3(P.grid[k]), dim3(64), 0, s, dev, rs, list, P.cnt[k], head, slabs, misses, Fbuf, c->scratch, c->scratch, slab_base, clk);
            break;
        case FC_QUAD:                                /* bands of up to 13 superblocks, four reads per wave */
            hipLaunchKernelGGL((k_fin_quad<1>), dim3(P.grid[k]), dim3(64), 0, s, dev, rs, list, P.cnt[k], head, slabs, misses, Fbuf, c->scratch, c->scratch, slab_base, clk);
            break;
        }
    }
#undef BRX_FIN_ALIGN
    if (!score) return;
    KTIMED(BRX_KERN_FIN_QSCORE, s);
    hipLaunchKernelGGL(k_fin_qscore, dim3(std::min<uint32_t>(P.cnt[k], set_waves(S))), dim3(64), 0, s, dev, rs, list, 0u, P.cnt[k], cq + fq_score[k],
                       phase, 0, 0xFFFF, c->scratch, c->scratch, clk);
}

/* the widest class and its giants are scored over the set's range of `order` (klass 5 and up) */
void Batch::score_wide(const FinalSet &S, int phase, hipStream_t s) {
    KTIMED(BRX_KERN_FIN_QSCORE, s);
    hipLaunchKernelGGL(k_fin_qscore, dim3(std::min<uint32_t>(set_waves(S), (uint32_t)c->n_cu * 8u)), dim3(64), 0, s, dev, rs, order, S.b, S.e,
                       fin_queue(S, phase) + fq_score[FC_WIDE], phase, 5, 0xFFFF, c->scratch, c->scratch, clk);
}

/* blocking: phase 0 of the set is done; repeat its window misses with the full store */
int Batch::finish_final(FinalSet &S) {
    if (S.e == S.b) return BRX_OK;
    if (S.wide != S.st) { int rcw = wait_stream(c, S.wide, "final stage, widest class"); if (rcw) return rcw; }      /* its misses are counted before the counter is read */
    { int rc_ = to_host(c, S.st, h_ctr(), miss_counter(S), 4); if (rc_) return rc_; }
    { int rcw = wait_stream(c, S.st, S.id ? "final stage (bulk)" : "final stage (head)"); if (rcw) return rcw; }
    const uint32_t misses = h_ctr()[0];
    c->window_misses += misses;
    if (!misses) return BRX_OK;
    { int rc_ = fetch_rs(S.st); if (rc_) return rc_; }
    { int rcw_ = wait_stream(c, S.st, "final stage, misses"); if (rcw_) return rcw_; }
    { int rcp = launch_final_phase(S, 1); if (rcp) return rcp; }
    if (S.wide != S.st) { int rcw = wait_stream(c, S.wide, "final stage, second phase, widest class"); if (rcw) return rcw; }
    return wait_stream(c, S.st, "final stage, second phase");
}

/* ---- stage: records ---- */
int Batch::records() {
    HIPCHK(c, hipEventRecord(c->ev_b[BRX_STAGE_EMIT], st));
    {
        KTIMED(BRX_KERN_EMIT, st);
        hipLaunchKernelGGL(k_recsize, dim3(nb64), dim3(64), 0, st, dev, rs, pieces);
        hipLaunchKernelGGL(k_scan_rec, dim3(1), dim3(64), 0, st, n_reads, rs, totals);
    }
    { int rc_ = read_totals(c, st, totals, 6); if (rc_) return rc_; }
    rec_bytes = c->h_totals[5];
    if (rec_bytes > out_cap) {
        c->output_needed = rec_bytes;
        return fail(c, BRX_E_OUTPUT, "output buffer too small: need %llu bytes", (unsigned long long)rec_bytes);
    }
    {
        KTIMED(BRX_KERN_EMIT, st);
        hipLaunchKernelGGL(k_emit, dim3(n_reads), dim3(64), 0, st, dev, rs, pieces, c->scratch, d_out);
        hipLaunchKernelGGL(k_stats, dim3(nb64), dim3(64), 0, st, dev, rs, d_stats);
    }
    HIPCHK(c, hipEventRecord(c->ev_e[BRX_STAGE_EMIT], st));
    { int rcw = wait_stream(c, st, "final stage / k_emit"); if (rcw) return rcw; }
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < BRX_STAGE_COUNT; ++i) {
        float ms = 0.f;
        if (i != BRX_STAGE_ALIGN1 && i != BRX_STAGE_QSCORE) (void)hipEventElapsedTime(&ms, c->ev_b[i], c->ev_e[i]);
        c->stage_ms[i] = ms;
    }
    return BRX_OK;
}

/* per-kernel launch statistics (brx_set_kernel_timing): every event pair recorded by KTIMED */
int Batch::kernel_statistics() {
    if (n_head && n_bulk) HIPCHK(c, hipStreamSynchronize(c->side));
    if (sets[0].wide_forked) HIPCHK(c, hipStreamSynchronize(c->side2));
    for (int i = 0; i < c->kev_n; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->kev_b[i], c->kev_e[i]) != hipSuccess) continue;
        c->kstat[c->kev_kind[i]].launches += 1;
        c->kstat[c->kev_kind[i]].ms += ms;
    }
    uint64_t all = 0, head_b = 0;
    for (uint32_t i = 0; i < n_reads; ++i) { all += h_rs[h_order[i]].n; if (i < n_head) head_b += h_rs[h_order[i]].n; }
    if (n_mb && !c->mutate_passes_route && c->lanes_cycles) {      /* the reads k_mut_lanes left to the in-place kernel (statistics only) */
        uint32_t left = 0;
        if (hipMemcpy(&left, mctr + MC_OUT, 4, hipMemcpyDeviceToHost) == hipSuccess && left <= n_reads && left) {
            std::vector<uint32_t> h_left(left);
            if (hipMemcpy(h_left.data(), active_a, (size_t)left * 4, hipMemcpyDeviceToHost) == hipSuccess)
                for (uint32_t x : h_left) if (x < n_reads) tail_bases += h_rs[x].n;
        }
    }
    c->kstat[BRX_KERN_PLAN].bases = c->kstat[BRX_KERN_BUILD].bases = c->kstat[BRX_KERN_FIN_JOIN].bases =
        c->kstat[BRX_KERN_FIN_QSCORE].bases = c->kstat[BRX_KERN_EMIT].bases = (double)all;
    c->kstat[BRX_KERN_MUTATE_RUN].bases = (double)(head_b + tail_bases);
    c->kstat[BRX_KERN_MUTATE_SEG].bases = c->kstat[BRX_KERN_MUT_POST].bases = c->kstat[BRX_KERN_WIN_LANE].bases = c->kstat[BRX_KERN_WIN_WAVE].bases = (double)(all - head_b);
    for (int k = 0; k < FC_GIANT; ++k) c->kstat[fin_kern[k]].bases = (double)(sets[0].bases[k] + sets[1].bases[k]);      /* (the giants are counted with FC_WIDE) */
    /* compatibility: the two per-launch stage entries of brx_last_stage_ms */
    if (c->kstat[BRX_KERN_FIN_ALIGN1].launches) c->stage_ms[BRX_STAGE_ALIGN1] = c->kstat[BRX_KERN_FIN_ALIGN1].ms / (float)c->kstat[BRX_KERN_FIN_ALIGN1].launches;
    if (c->kstat[BRX_KERN_FIN_QSCORE].launches) c->stage_ms[BRX_STAGE_QSCORE] = c->kstat[BRX_KERN_FIN_QSCORE].ms / (float)c->kstat[BRX_KERN_FIN_QSCORE].launches;
    return BRX_OK;
}

int Batch::run() {
    if (!c->has_em || !c->has_qm) return fail(c, BRX_E_STATE, "error/qscore model not set");
    if (!raw && (!c->has_ref || !c->has_params)) return fail(c, BRX_E_STATE, "reference or parameters not set");
    if (!c->scratch) return fail(c, BRX_E_STATE, "scratch arena not set");
    if (out_bytes) *out_bytes = 0;
    if (n_reads == 0) return BRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = layout_and_plan()) || (rc = build()) || (rc = prepare_chains())) return rc;
    HIPCHK(c, hipEventRecord(c->ev_b[BRX_STAGE_MUTATE], st));
    if (n_mh && (rc = head_chain())) return rc;
    if (n_mb && (rc = c->mutate_passes_route ? bulk_chain_passes() : bulk_chain_lanes())) return rc;
    if (!n_mh && (rc = single_chain_legacy())) return rc;
    HIPCHK(c, hipEventRecord(c->ev_e[BRX_STAGE_MUTATE], st));
    HIPCHK(c, hipEventRecord(c->ev_b[BRX_STAGE_SCAN], st));
    HIPCHK(c, hipEventRecord(c->ev_e[BRX_STAGE_SCAN], st));
    HIPCHK(c, hipEventRecord(c->ev_b[BRX_STAGE_FINAL], st));
    /* ---- final stages: whichever set is not started yet (head first: it is the longer chain), then wait for both ---- */
    if (!sets[0].launched && (rc = start_final(sets[0]))) return rc;
    if ((rc = start_final(sets[1])) || (rc = finish_final(sets[0])) || (rc = finish_final(sets[1]))) return rc;
    if (n_head && n_bulk) {                           /* join: the records need both sets */
        HIPCHK(c, hipEventRecord(c->ev_join, s_head));
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_join, 0));
    }
    HIPCHK(c, hipEventRecord(c->ev_e[BRX_STAGE_FINAL], st));
    if ((rc = records())) return rc;
    if (c->ktiming && (rc = kernel_statistics())) return rc;
    if (out_bytes) *out_bytes = (size_t)rec_bytes;
    if (!raw) { c->paf_dev = dev; c->paf_rs = rs; c->paf_segs = segs; c->paf_reads = n_reads; c->paf_pieces = pieces; c->paf_seqbuf = c->scratch; c->paf_frags = Fbuf; c->paf_valid = true; }
    /* a read that exhausted its 1000 tries is fatal in the reference (simulate.py:164) */
    if (!raw) {
        { int rc_ = fetch_rs(st); if (rc_) return rc_; }
        { int rcw_ = wait_stream(c, st, "read status"); if (rcw_) return rcw_; }
        for (uint32_t i = 0; i < n_reads; ++i) if (h_rs[i].status & BRX_RS_NOFRAG) {
            snprintf(c->err, sizeof(c->err), "read %llu failed to generate a sequence fragment", (unsigned long long)(first_read + i));
            return BRX_E_NOFRAG;
        }
    }
    return BRX_OK;
}

/* A batch runs on the caller's stream AND on the context's side streams.  Whatever the status, nothing of the batch is
   in flight when the call returns: an early BRX_E_SCRATCH / BRX_E_OUTPUT return (the caller then replaces the arena or the
   output buffer and repeats the batch) must not leave kernels of the abandoned attempt reading and writing the old arena. */
static int run_pipeline(brx_ctx *c, uint64_t seed, uint64_t first_read, uint32_t n_reads, bool raw,
                        const uint8_t *d_frags, const uint64_t *d_frag_off, const double *d_target,
                        uint8_t *d_out, size_t out_cap, brx_read_stats *d_stats, size_t *out_bytes, hipStream_t st) {
    if (c) c->paf_valid = false;
    Batch B{c, seed, first_read, n_reads, raw, d_frags, d_frag_off, d_target, d_out, out_cap, d_stats, out_bytes, st};      /* the rest: zero */
    const int rc = B.run();
    if (rc != BRX_OK && rc != BRX_E_ARG && rc != BRX_E_STATE) {
        (void)hipStreamSynchronize(st);
        if (c->side) (void)hipStreamSynchronize(c->side);
        if (c->side2) (void)hipStreamSynchronize(c->side2);
    }
    return rc;
}

extern "C" int brx_simulate_batch(brx_ctx *c, uint64_t seed, uint64_t first_read, uint32_t n_reads,
                                  uint8_t *d_out, size_t out_cap, brx_read_stats *d_stats,
                                  size_t *out_bytes, void *hip_stream) {
    if (!c || !d_out || !d_stats) return BRX_E_ARG;
    return run_pipeline(c, seed, first_read, n_reads, false, nullptr, nullptr, nullptr, d_out, out_cap, d_stats, out_bytes,
                        (hipStream_t)hip_stream);
}

extern "C" int brx_sequence_fragments(brx_ctx *c, uint64_t seed, uint64_t first_read, uint32_t n_frags,
                                      const uint8_t *d_frags, const uint64_t *d_frag_off, const double *d_target,
                                      uint8_t *d_out, size_t out_cap, brx_read_stats *d_stats, size_t *out_bytes,
                                      void *hip_stream) {
    if (!c || !d_out || !d_stats || !d_frags || !d_frag_off || !d_target) return BRX_E_ARG;
    return run_pipeline(c, seed, first_read, n_frags, true, d_frags, d_frag_off, d_target, d_out, out_cap, d_stats, out_bytes,
                        (hipStream_t)hip_stream);
}

extern "C" int brx_align_batch(brx_ctx *c, uint32_t n_pairs, const uint8_t *d_queries, const uint64_t *d_q_off,
                               const uint8_t *d_targets, const uint64_t *d_t_off, const int32_t *d_k_hint,
                               int32_t *d_dist, uint32_t *d_ncols, uint32_t *d_nmatch, uint8_t *d_ops,
                               const uint64_t *d_ops_off, void *hip_stream) {
    if (!c || !d_q_off || !d_t_off || !d_k_hint || !d_dist || !d_ncols || !d_nmatch) return BRX_E_ARG;
    c->paf_valid = false;
    if (!c->scratch) return fail(c, BRX_E_STATE, "scratch arena not set");
    if (n_pairs == 0) return BRX_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(c, hipSetDevice(c->device));
    DBG("align_batch: %u pairs", n_pairs);
    std::vector<uint64_t> qo(n_pairs + 1), to(n_pairs + 1);
    std::vector<int32_t> kh(n_pairs);
    HIPCHK(c, hipMemcpyAsync(qo.data(), d_q_off, (size_t)(n_pairs + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(to.data(), d_t_off, (size_t)(n_pairs + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(kh.data(), d_k_hint, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    DBG("align_batch: offsets copied");
    Arena A; A.base = c->scratch; A.cap = c->scratch_bytes; A.used = 0; A.top = 0;
    uint64_t *scr_off = (uint64_t *)A.take((size_t)n_pairs * 8);
    uint64_t *scr_bytes = (uint64_t *)A.take((size_t)n_pairs * 8);
    uint32_t *counters = (uint32_t *)A.take(4096 * 4);
    if (!A.ok()) return scratch_short(c, A.used + ((size_t)1 << 26));
    size_t at = (A.used + 255) & ~(size_t)255;
    size_t cap = c->scratch_bytes - at;
    std::vector<uint64_t> h_off(n_pairs), h_bytes(n_pairs);
    std::vector<std::pair<uint32_t, uint32_t>> chunks;
    uint32_t begin = 0; uint64_t used = 0, biggest = 0;
    for (uint32_t i = 0; i < n_pairs; ++i) {
        uint64_t Q = qo[i + 1] - qo[i], T = to[i + 1] - to[i];
        if (Q >= ((uint64_t)1 << 30) || T >= ((uint64_t)1 << 30)) return fail(c, BRX_E_ARG, "sequence %u too long", i);
        /* the band-doubling rounds of the kernel (k = 64, 128, ... capped at max(Q,T)) do not need
           monotonically more traceback store: size the pair for the largest of them */
        uint64_t units = 0;
        if (Q && T) {
            const int maxk = (int)std::max(Q, T);
            int k = kh[i] >= 0 ? kh[i] : std::min(maxk, 64);
            for (;;) {
                BrxGeom g = brx_make_geom((int)Q, (int)T, k);
                if (g.G) units = std::max(units, brx_align_units(g));
                if (kh[i] >= 0 || k >= maxk) break;
                k = k * 2 > maxk ? maxk : k * 2;
            }
        }
        uint64_t need = (((Q + 31) & ~15ull) + ((T + 31) & ~15ull) + (units + 8) * 8 + 255) & ~255ull;
        biggest = std::max(biggest, need);
        if (used + need > cap) { chunks.push_back({begin, i}); begin = i; used = 0; }
        h_off[i] = used; h_bytes[i] = need; used += need;
    }
    chunks.push_back({begin, n_pairs});
    if (biggest > cap) return scratch_short(c, at + (size_t)biggest);
    if (chunks.size() > 4000) return scratch_short(c, at + (size_t)biggest * 64);
    HIPCHK(c, hipMemcpyAsync(scr_off, h_off.data(), (size_t)n_pairs * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(scr_bytes, h_bytes.data(), (size_t)n_pairs * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(counters, 0, 4096 * 4, st));
    HIPCHK(c, hipEventRecord(c->ev_b[BRX_STAGE_FINAL], st));
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        uint32_t b = chunks[ci].first, e = chunks[ci].second;
        if (e == b) continue;
        uint32_t waves = std::min<uint64_t>(e - b, (uint64_t)c->n_cu * (uint64_t)c->waves_per_cu);
        DBG("align_batch: chunk %zu pairs [%u,%u) waves %u", ci, b, e, waves);
        hipLaunchKernelGGL(k_align_batch, dim3(waves), dim3(64), 0, st, n_pairs, b, e, counters + ci, d_queries, d_q_off,
                           d_targets, d_t_off, d_k_hint, d_dist, d_ncols, d_nmatch, d_ops, d_ops_off,
                           c->scratch + at, scr_off, scr_bytes, brx_debug() ? c->d_prog : (uint32_t *)nullptr);
    }
    HIPCHK(c, hipEventRecord(c->ev_e[BRX_STAGE_FINAL], st));
    DBG("align_batch: launched, waiting");
    { int rcw = wait_stream(c, st, "k_align_batch"); if (rcw) return rcw; }
    for (int i = 0; i < BRX_STAGE_COUNT; ++i) c->stage_ms[i] = 0.f;
    (void)hipEventElapsedTime(&c->stage_ms[BRX_STAGE_FINAL], c->ev_b[BRX_STAGE_FINAL], c->ev_e[BRX_STAGE_FINAL]);
    c->final_launches = (uint32_t)chunks.size();
    HIPCHK(c, hipGetLastError());
    DBG("align_batch: done");
    return BRX_OK;
}

/* the tool calls: model builders, gzip members, truth output, depth, window identities, the device loaders */
#include "brx_tools.h"
