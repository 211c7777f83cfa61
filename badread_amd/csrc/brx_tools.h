/*
 * brx_tools.h -- the tool calls of the C-ABI: everything of include/brx.h that is not the simulate pipeline or brx_align_batch.
 * Included once, last, by brx_hip.hip, whose context and helpers (brx_ctx, fail, HIPCHK, wait_stream, pinned_regrow) it uses.
 *   brx_model_count                              brx_model.h      the counting loops of the model builders
 *   brx_gzip_device, brx_bgzf_device(_off)       brx_gzip_dev.h   gzip members / BGZF blocks
 *   brx_emit_paf / _sam / _bam / _depth          brx_paf.h, brx_sam.h, brx_bam.h, brx_depth.h   truth output of the last batch
 *   brx_depth_bedgraph                           brx_depth.h      the job's coverage as text
 *   brx_window_means                             brx_window.h     the plot command's numbers
 *   brx_paf_scan, brx_align_pack                 brx_pafin.h      the device loader
 *   brx_fastq_scan, brx_reads_pack               brx_fastqin.h    the device read loader
 *   brx_bam_sort, brx_bam_index                  brx_bamsort.h    the truth BAM in coordinate order and its index
 * The kernel headers share brx_scan.h and nothing else.  The calls share three helpers, below: Carver (where a call keeps what in the
 * caller's scratch), Call (stream, timing marks, read-backs, waits, the two "too small" answers) and last_ms (the *_last getters).
 */
#ifndef BRX_TOOLS_H
#define BRX_TOOLS_H

#include "brx_paf.h"
#include "brx_sam.h"
#include "brx_bam.h"
#include "brx_depth.h"
#include "brx_window.h"
#include "brx_pafin.h"
#include "brx_fastqin.h"
#include "brx_bamsort.h"

/* Offsets into a scratch block that the caller allocated: every piece begins on a multiple of 256 bytes of the block's first such
   address, so bytes() asks for 256 more than the pieces take -- the caller's block may begin anywhere. */
struct Carver {
    size_t used = 0;
    size_t take(uint64_t bytes) { const size_t here = used; used += (size_t)((bytes + 255) & ~(uint64_t)255); return here; }
    size_t bytes() const { return used + 256; }
    template <class T> static T *at(void *block, size_t off) { return (T *)((((uintptr_t)block + 255) & ~(uintptr_t)255) + off); }
};

/* One tool call on the caller's stream.  Constructing it touches nothing; begin() selects the device, after the argument checks. */
struct Call {
    brx_ctx *c; hipStream_t st; bool timed;      /* timed: brx_set_kernel_timing is on and its event pool exists; mark(i) records event i of it */
    Call(brx_ctx *c_, void *hip_stream) : c(c_), st((hipStream_t)hip_stream), timed(c_->ktiming && c_->kev_b[0]) {}
    int begin() { HIPCHK(c, hipSetDevice(c->device)); return BRX_OK; }
    void mark(int i) { if (timed) (void)hipEventRecord(c->kev_b[i], st); }
    /* a few words to pageable host memory; they are there after the next wait() or sync() */
    int read_back(void *h_dst, const void *d_src, size_t bytes) { HIPCHK(c, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st)); return BRX_OK; }
    int wait(const char *what) { return wait_stream(c, st, what); }
    int sync(const char *what) { const int rc = wait_stream(c, st, what); if (rc) return rc; HIPCHK(c, hipGetLastError()); return BRX_OK; }
    int elapsed(float *dst, int i, int j) { if (timed) HIPCHK(c, hipEventElapsedTime(dst, c->kev_b[i], c->kev_b[j])); return BRX_OK; }
    /* BRX_E_SCRATCH; brx_scratch_needed() then says `need`.  detail: what the size is for, when a call sizes twice */
    int need_scratch(const char *name, size_t have, size_t need, const char *detail = "") {
        c->scratch_needed = need;
        return fail(c, BRX_E_SCRATCH, "%s: scratch too small%s (%zu < %zu)", name, detail, have, need);
    }
    /* BRX_E_OUTPUT; brx_output_needed() then says `need`, in the unit of the call's output capacity */
    int need_output(size_t need, const char *fmt, ...) {
        c->output_needed = need;
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof(c->err), fmt, ap);
        va_end(ap);
        return BRX_E_OUTPUT;
    }
};
#define BRX_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

/* the body of the *_last getters: the milliseconds that the last call of a family left in the context */
template <size_t N> static int last_ms(const brx_ctx *c, float (brx_ctx::*field)[N], float *ms) {
    if (!c || !ms) return BRX_E_ARG;
    memcpy(ms, c->*field, sizeof(float) * N);
    return BRX_OK;
}

/* ---- the counting loops of the model builders (brx_model.h).  The job struct of the ABI has the layout of BrxMbJob. ---- */
static_assert(sizeof(brx_model_job) == sizeof(BrxMbJob), "brx_model_job and BrxMbJob must have the same layout");
extern "C" int brx_model_count(brx_ctx *c, int kind, const brx_model_job *job, void *hip_stream) {
    if (!c || !job || (kind != 0 && kind != 1)) return BRX_E_ARG;
    c->paf_valid = false;
    if (job->n_align == 0 || job->n_cols == 0) return BRX_OK;
    if (kind == 0 && (job->k < 2 || 2 * job->k + 5 + 2 * BRX_MB_MAX_READ_KMER > 64)) return fail(c, BRX_E_ARG, "error model k-mer size %u not supported (2..8)", job->k);
    if (kind == 1 && (job->n_ksizes < 1 || job->n_ksizes > 16 || job->max_del > 15)) return fail(c, BRX_E_ARG, "qscore model: k_size up to 31, max_del up to 15");
    Call K(c, hip_stream);
    BRX_TRY(K.begin());
    BrxMbJob j;
    memcpy(&j, job, sizeof(j));
    const uint64_t nb = (job->n_cols + 255) / 256;
    hipLaunchKernelGGL(k_mb_expand, dim3((unsigned)nb), dim3(256), 0, K.st, j);
    if (kind == 0) hipLaunchKernelGGL(k_mb_error, dim3((unsigned)nb), dim3(256), 0, K.st, j);
    else hipLaunchKernelGGL(k_mb_qscore, dim3((unsigned)((job->n_cols * job->n_ksizes + 255) / 256)), dim3(256), 0, K.st, j);
    uint32_t flags[4] = {0, 0, 0, 0};
    BRX_TRY(K.read_back(flags, job->d_flags, sizeof(flags)));
    BRX_TRY(K.sync("model builder"));
    if (flags[0] & 1u) return fail(c, BRX_E_OUTPUT, "model builder: hash table full");
    return BRX_OK;
}

/* ---- gzip members on the device (brx_gzip_dev.h) ---- */
static BrxGzConst gz_const() {
    BrxGzConst K;
    K.x2n[0] = 0x40000000u;
    for (int i = 1; i < 32; ++i) K.x2n[i] = brx_gz_mulmod(K.x2n[i - 1], K.x2n[i - 1]);
    return K;
}
extern "C" size_t brx_gzip_device_bound(size_t n_bytes, uint32_t n_blocks) {
    if (!n_bytes) return 8;
    const size_t nb = n_blocks ? n_blocks : (n_bytes + BRX_GZ_BLOCK - 1) / BRX_GZ_BLOCK;
    return nb * (size_t)brx_gz_member_bound(0) + (15 * n_bytes + 7) / 8 + nb + 16;      /* sum over the blocks of brx_gz_member_bound(len) */
}
extern "C" size_t brx_gzip_device_scratch(size_t n_bytes, uint32_t n_blocks) {
    const size_t nb = n_blocks ? n_blocks : (n_bytes + BRX_GZ_BLOCK - 1) / BRX_GZ_BLOCK;
    return nb * (size_t)(4 * BRX_GZ_TAB + 4 * BRX_GZ_OFFS + 8) + (nb + 1) * 8 + 1024;
}
/* gzip members (brx_gzip_device) or BGZF blocks (brx_bgzf_device: fixed blocks of BRX_BGZF_BLOCK bytes) of d_in.  Its scratch is laid
   out by hand, not by Carver: brx_gzip_device_scratch above promises callers the byte count of exactly this packing. */
template <bool BGZF>
static int gz_members(brx_ctx *c, const void *d_in, size_t n_bytes, const uint64_t *d_block_off, uint32_t n_blocks, void *d_out, size_t out_cap,
                      void *d_scratch, size_t scratch_bytes, size_t *out_bytes, void *hip_stream, uint64_t *d_member_off = nullptr) {
    if (!c || !out_bytes || (n_bytes && (!d_in || !d_out || !d_scratch)) || (d_block_off && !n_blocks)) return BRX_E_ARG;
    *out_bytes = 0;
    if (!n_bytes) return BRX_OK;
    if ((uintptr_t)d_out & 3u) return fail(c, BRX_E_ARG, "brx_gzip_device: the output buffer must be 4-byte aligned");
    const uint32_t nb = d_block_off ? n_blocks : (uint32_t)((n_bytes + BrxGzFlavour<BGZF>::block - 1) / BrxGzFlavour<BGZF>::block);
    Call K(c, hip_stream);
    if (scratch_bytes < brx_gzip_device_scratch(n_bytes, nb)) return K.need_scratch("brx_gzip_device", scratch_bytes, brx_gzip_device_scratch(n_bytes, nb));
    BRX_TRY(K.begin());
    static const BrxGzConst G = gz_const();
    uint8_t *p = (uint8_t *)d_scratch;
    uint64_t *member_off = (uint64_t *)p; p += ((size_t)nb + 1) * 8;
    uint32_t *tabs = (uint32_t *)p; p += (size_t)nb * 4 * BRX_GZ_TAB;
    uint32_t *offs = (uint32_t *)p; p += (size_t)nb * 4 * BRX_GZ_OFFS;
    uint32_t *crcs = (uint32_t *)p; p += (size_t)nb * 4;
    uint32_t *sizes = (uint32_t *)p;
    const uint32_t grid = std::min<uint32_t>(nb, (uint32_t)c->n_cu * 8u);
    hipLaunchKernelGGL((k_gz_plan<BGZF>), dim3(grid), dim3(64), 0, K.st, (const uint8_t *)d_in, (uint64_t)n_bytes, d_block_off, nb, G, tabs, offs, crcs, sizes);
    hipLaunchKernelGGL(k_gz_scan, dim3(1), dim3(64), 0, K.st, nb, sizes, member_off);
    uint64_t total = 0;
    BRX_TRY(K.read_back(&total, member_off + nb, 8));
    BRX_TRY(K.wait("brx_gzip_device (plan)"));
    if (total + 8 > out_cap) return K.need_output((size_t)total + 8, "brx_gzip_device: output buffer too small: need %llu bytes", (unsigned long long)total + 8);
    HIPCHK(c, hipMemsetAsync(d_out, 0, (size_t)((total + 7) & ~(uint64_t)3), K.st));
    hipLaunchKernelGGL((k_gz_pack<BGZF>), dim3(grid), dim3(64), 0, K.st, (const uint8_t *)d_in, (uint64_t)n_bytes, d_block_off, nb, (uint8_t *)d_out, member_off, tabs, offs, crcs);
    /* brx_bgzf_device_off: where the members begin, as the scan left them at the head of the scratch */
    if (d_member_off) HIPCHK(c, hipMemcpyAsync(d_member_off, member_off, ((size_t)nb + 1) * 8, hipMemcpyDeviceToDevice, K.st));
    BRX_TRY(K.sync("brx_gzip_device (pack)"));
    *out_bytes = (size_t)total;
    return BRX_OK;
}
extern "C" int brx_gzip_device(brx_ctx *c, const void *d_in, size_t n_bytes, const uint64_t *d_block_off, uint32_t n_blocks, void *d_out, size_t out_cap,
                               void *d_scratch, size_t scratch_bytes, size_t *out_bytes, void *hip_stream) {
    return gz_members<false>(c, d_in, n_bytes, d_block_off, n_blocks, d_out, out_cap, d_scratch, scratch_bytes, out_bytes, hip_stream);
}
static uint32_t bgzf_blocks(size_t n_bytes) { return (uint32_t)((n_bytes + BRX_BGZF_BLOCK - 1) / BRX_BGZF_BLOCK); }
extern "C" size_t brx_bgzf_device_bound(size_t n_bytes) {
    const size_t nb = bgzf_blocks(n_bytes);
    return nb * (18 + (BRX_GZ_HDR_BITS + 15 + 7) / 8 + 8) + (15 * n_bytes + 7) / 8 + nb + 16;
}
extern "C" size_t brx_bgzf_device_scratch(size_t n_bytes) { return brx_gzip_device_scratch(n_bytes, bgzf_blocks(n_bytes)); }
extern "C" int brx_bgzf_device_off(brx_ctx *c, const void *d_in, size_t n_bytes, void *d_out, size_t out_cap, void *d_scratch, size_t scratch_bytes,
                                   size_t *out_bytes, uint64_t *d_block_off, void *hip_stream) {
    if (n_bytes > (size_t)BRX_BGZF_BLOCK * 0xFFFFFFFFull) return c ? fail(c, BRX_E_ARG, "brx_bgzf_device: input too long") : BRX_E_ARG;
    return gz_members<true>(c, d_in, n_bytes, nullptr, 0, d_out, out_cap, d_scratch, scratch_bytes, out_bytes, hip_stream, d_block_off);
}
extern "C" int brx_bgzf_device(brx_ctx *c, const void *d_in, size_t n_bytes, void *d_out, size_t out_cap, void *d_scratch, size_t scratch_bytes,
                               size_t *out_bytes, void *hip_stream) {
    return brx_bgzf_device_off(c, d_in, n_bytes, d_out, out_cap, d_scratch, scratch_bytes, out_bytes, nullptr, hip_stream);
}

/* ---- truth alignments of the last simulate batch: PAF text (brx_paf.h), SAM records (brx_sam.h), BAM records (brx_bam.h) or the
   records' end points (brx_depth.h) ---- */
enum { TRUTH_PAF = 0, TRUTH_SAM = 1, TRUTH_BAM = 2, TRUTH_DEPTH = 3 };
/* f(std::integral_constant<uint32_t, TAGS>, std::bool_constant<F>) for the tags and "some format bit" of a call: one instantiation of the SAM /
   BAM kernels per pair.  TAGS = 0 is the untagged code, nothing of the tags in its column loops; F = false the code of brx_emit_*_tags,
   nothing of the formats in it; with F the bits are a value of the grid's. */
template <class Fn> static void with_tags_fmt(uint32_t tags, bool fmtd, Fn f) {
    auto with_fmt = [&](auto T) { if (fmtd) f(T, std::true_type{}); else f(T, std::false_type{}); };
    switch (tags) {
        case 0: with_fmt(std::integral_constant<uint32_t, 0u>{}); break;
        case 1: with_fmt(std::integral_constant<uint32_t, 1u>{}); break;
        case 2: with_fmt(std::integral_constant<uint32_t, 2u>{}); break;
        default: with_fmt(std::integral_constant<uint32_t, 3u>{}); break;
    }
}
static int emit_truth(brx_ctx *c, int kind, uint32_t fmt, uint32_t tags, uint32_t max_ops, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream) {
    if (!c || !out_bytes) return BRX_E_ARG;
    *out_bytes = 0;
    if (tags & ~(uint32_t)(BRX_TAG_MD | BRX_TAG_SA)) return fail(c, BRX_E_ARG, "truth tags %#x: only BRX_TAG_MD | BRX_TAG_SA", tags);
    if ((fmt & ~(uint32_t)(BRX_FMT_EQX | BRX_FMT_CS | BRX_FMT_CS_LONG)) || (fmt & (BRX_FMT_CS | BRX_FMT_CS_LONG)) == BRX_FMT_CS_LONG)
        return fail(c, BRX_E_ARG, "truth format %#x: BRX_FMT_EQX | BRX_FMT_CS | BRX_FMT_CS_LONG, the last only with BRX_FMT_CS", fmt);
    if (!c->paf_valid) return fail(c, BRX_E_STATE, "no simulate batch on this context to emit truth alignments for");
    Call K(c, hip_stream);
    BRX_TRY(K.begin());
    hipStream_t st = K.st;
    const uint32_t n = c->paf_reads;
    /* the pinned block of the sizes: per read its bytes, its primary record, its offset; for SA:Z: its records and their scan.  Exactly as
       large as this batch needs (the block itself is aligned: the offsets are used as they are) */
    Carver V;
    const size_t len_at = V.take((size_t)n * 4), best_at = V.take((size_t)n * 4), off_at = V.take(((size_t)n + 1) * 8);
    const size_t nrec_at = V.take((size_t)n * 4), recoff_at = V.take(((size_t)n + 1) * 8);
    const size_t need = recoff_at + ((size_t)n + 1) * 8;
    if (c->paf_bytes < need) BRX_TRY(pinned_regrow(c, &c->h_paf, &c->d_paf, &c->paf_bytes, need));
    uint32_t *len = (uint32_t *)(c->d_paf + len_at), *best = (uint32_t *)(c->d_paf + best_at), *n_rec = (uint32_t *)(c->d_paf + nrec_at);
    uint64_t *off = (uint64_t *)(c->d_paf + off_at), *rec_off = (uint64_t *)(c->d_paf + recoff_at);
    const uint8_t *arena = (const uint8_t *)c->scratch;
    const bool sam = kind == TRUTH_SAM, bam = kind == TRUTH_BAM, depth = kind == TRUTH_DEPTH, sa = (tags & BRX_TAG_SA) != 0;
    if (depth && ((uintptr_t)d_out & 7u)) return fail(c, BRX_E_ARG, "brx_emit_depth: the output buffer must be 8-byte aligned");
    const uint64_t *c_off = off, *c_rec_off = rec_off;
    const uint32_t *c_best = best;
    auto size = [&](auto T, auto F) {
        constexpr uint32_t TG = decltype(T)::value; constexpr bool FM = decltype(F)::value;
        if (bam) hipLaunchKernelGGL((k_bam_size<TG, FM>), dim3(n), dim3(64), 0, st, c->paf_dev, c->paf_rs, c->paf_segs, arena, max_ops, len, best, n_rec, fmt);
        else if (sam) hipLaunchKernelGGL((k_sam_size<TG, FM>), dim3(n), dim3(64), 0, st, c->paf_dev, c->paf_rs, c->paf_segs, arena, len, best, n_rec, fmt);
        else hipLaunchKernelGGL((k_paf_size<FM>), dim3(n), dim3(64), 0, st, c->paf_dev, c->paf_rs, c->paf_segs, arena, fmt, len, best);
    };
    if (n && depth) hipLaunchKernelGGL(k_depth_size, dim3(n), dim3(64), 0, st, c->paf_dev, c->paf_rs, c->paf_segs, arena, len);
    else if (n) with_tags_fmt(tags, fmt != 0, size);
    hipLaunchKernelGGL(k_truth_scan, dim3(1), dim3(64), 0, st, n, (const uint32_t *)len, off);
    if (sa) hipLaunchKernelGGL(k_truth_scan, dim3(1), dim3(64), 0, st, n, (const uint32_t *)n_rec, rec_off);
    BRX_TRY(K.sync(depth ? "k_depth_size" : bam ? "k_bam_size" : sam ? "k_sam_size" : "k_paf_size"));
    const uint64_t total = ((const uint64_t *)(c->h_paf + off_at))[n];
    if (total > out_cap || (total && !d_out)) return K.need_output(total, "truth alignment buffer too small: need %llu bytes", (unsigned long long)total);
    const uint64_t sa_recs = sa ? ((const uint64_t *)(c->h_paf + recoff_at))[n] : 0;
    if (sa_recs * sizeof(SaRec) > c->sa_bytes)       /* a quarter and 1024 records more than asked: the next batch has about as many */
        BRX_TRY(pinned_regrow(c, &c->h_sa, &c->d_sa, &c->sa_bytes, (size_t)(sa_recs + sa_recs / 4 + 1024) * sizeof(SaRec)));
    SaRec *table = (SaRec *)c->d_sa;
    if (n && total && sa_recs) hipLaunchKernelGGL(k_sa_fill, dim3(n), dim3(64), 0, st, c->paf_dev, c->paf_rs, c->paf_segs, arena, (const uint64_t *)rec_off, table);
    const SaRec *c_table = table;
    auto write = [&](auto T, auto F) {
        constexpr uint32_t TG = decltype(T)::value; constexpr bool FM = decltype(F)::value;
        if (bam) hipLaunchKernelGGL((k_bam_write<TG, FM>), dim3(n), dim3(64), 0, st, c->paf_dev, c->paf_rs, c->paf_segs, c->paf_pieces, c->paf_seqbuf, max_ops,
                                    c_off, c_best, d_out, c->paf_frags, c_rec_off, c_table, fmt);
        else if (sam) hipLaunchKernelGGL((k_sam_write<TG, FM>), dim3(n), dim3(64), 0, st, c->paf_dev, c->paf_rs, c->paf_segs, c->paf_pieces, c->paf_seqbuf,
                                         c_off, c_best, d_out, c->paf_frags, c_rec_off, c_table, fmt);
        else hipLaunchKernelGGL((k_paf_write<FM>), dim3(n), dim3(64), 0, st, c->paf_dev, c->paf_rs, c->paf_segs, arena, c->paf_seqbuf, c->paf_frags, fmt,
                                c_off, c_best, d_out);
    };
    if (n && total && depth) hipLaunchKernelGGL(k_depth_write, dim3(n), dim3(64), 0, st, c->paf_dev, c->paf_rs, c->paf_segs, arena, c_off, d_out);
    else if (n && total) with_tags_fmt(tags, fmt != 0, write);
    if (d_read_off) HIPCHK(c, hipMemcpyAsync(d_read_off, c->h_paf + off_at, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    BRX_TRY(K.sync(depth ? "k_depth_write" : bam ? "k_bam_write" : sam ? "k_sam_write" : "k_paf_write"));
    *out_bytes = (size_t)total;
    return BRX_OK;
}
extern "C" int brx_emit_paf_fmt(brx_ctx *c, uint32_t fmt, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream) {
    return emit_truth(c, TRUTH_PAF, fmt, 0, 0, d_out, out_cap, d_read_off, out_bytes, hip_stream);
}
extern "C" int brx_emit_sam_fmt(brx_ctx *c, uint32_t fmt, uint32_t tags, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream) {
    return emit_truth(c, TRUTH_SAM, fmt, tags, 0, d_out, out_cap, d_read_off, out_bytes, hip_stream);
}
extern "C" int brx_emit_bam_fmt(brx_ctx *c, uint32_t fmt, uint32_t tags, uint32_t max_cigar_ops, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off,
                                size_t *out_bytes, void *hip_stream) {
    if (!c || !out_bytes) return BRX_E_ARG;
    if (max_cigar_ops == 0) max_cigar_ops = 65535;
    if (max_cigar_ops < 2 || max_cigar_ops > 65535) return fail(c, BRX_E_ARG, "brx_emit_bam: max_cigar_ops %u (2..65535, or 0 for 65535)", max_cigar_ops);
    return emit_truth(c, TRUTH_BAM, fmt, tags, max_cigar_ops, d_out, out_cap, d_read_off, out_bytes, hip_stream);
}
/* the functions without formats: fmt = 0 */
extern "C" int brx_emit_paf(brx_ctx *c, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream) {
    return brx_emit_paf_fmt(c, 0, d_out, out_cap, d_read_off, out_bytes, hip_stream);
}
extern "C" int brx_emit_sam_tags(brx_ctx *c, uint32_t tags, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream) {
    return brx_emit_sam_fmt(c, 0, tags, d_out, out_cap, d_read_off, out_bytes, hip_stream);
}
extern "C" int brx_emit_sam(brx_ctx *c, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream) {
    return brx_emit_sam_fmt(c, 0, 0, d_out, out_cap, d_read_off, out_bytes, hip_stream);
}
extern "C" int brx_emit_bam_tags(brx_ctx *c, uint32_t tags, uint32_t max_cigar_ops, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes,
                                 void *hip_stream) {
    return brx_emit_bam_fmt(c, 0, tags, max_cigar_ops, d_out, out_cap, d_read_off, out_bytes, hip_stream);
}
extern "C" int brx_emit_bam(brx_ctx *c, uint32_t max_cigar_ops, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream) {
    return brx_emit_bam_fmt(c, 0, 0, max_cigar_ops, d_out, out_cap, d_read_off, out_bytes, hip_stream);
}
extern "C" int brx_emit_depth(brx_ctx *c, uint8_t *d_out, size_t out_cap, uint64_t *d_read_off, size_t *out_bytes, void *hip_stream) {
    return emit_truth(c, TRUTH_DEPTH, 0, 0, 0, d_out, out_cap, d_read_off, out_bytes, hip_stream);
}

/* ---- the true coverage of the reference as text (brx_depth.h) ---- */
/* where brx_depth_bedgraph keeps what in its scratch, for N keys (the events and four per contig) */
struct DpPlan { uint64_t n; uint32_t n_tiles; size_t keys_a, keys_b, gk, gd, cd, table, incl, sums, flags, bytes; };
static DpPlan dp_plan(uint64_t n) {
    DpPlan p; p.n = n; p.n_tiles = (uint32_t)((n + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE);
    const uint64_t cells = 256ull * p.n_tiles, longest = std::max(n, cells);
    Carver V;
    p.keys_a = V.take(n * 8); p.keys_b = V.take(n * 8); p.gk = V.take(n * 8); p.gd = V.take(n * 4); p.cd = V.take(n * 4);
    p.table = V.take(cells * 4); p.incl = V.take(cells * 8);
    p.sums = V.take(((longest + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE + 1) * 8); p.flags = V.take(256);
    p.bytes = V.bytes();
    return p;
}
extern "C" size_t brx_depth_bedgraph_scratch(uint64_t n_events) { return dp_plan(n_events + 4ull * BRX_DEPTH_SCRATCH_CONTIGS).bytes; }
extern "C" int brx_depth_last(const brx_ctx *c, uint32_t *sort_passes, float ms[3]) {
    if (!c) return BRX_E_ARG;
    if (sort_passes) *sort_passes = c->depth_passes;
    return ms ? last_ms(c, &brx_ctx::depth_ms, ms) : BRX_OK;
}
static double dp_now_ms() { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }

extern "C" int brx_depth_bedgraph(brx_ctx *c, const uint64_t *d_events, uint64_t n_events, uint8_t *d_out, size_t out_cap, size_t *out_bytes,
                                  void *d_scratch, size_t scratch_bytes, void *hip_stream) {
    if (!c || !out_bytes || (n_events && !d_events) || !d_scratch) return BRX_E_ARG;
    *out_bytes = 0;
    if (!c->has_ref) return fail(c, BRX_E_STATE, "brx_depth_bedgraph: reference not set");
    const brx_reference &ref = c->dev.ref;
    if (n_events & 1u) return fail(c, BRX_E_ARG, "brx_depth_bedgraph: %llu events: every record has two", (unsigned long long)n_events);
    if (ref.n_contigs >= (1u << 24)) return fail(c, BRX_E_ARG, "brx_depth_bedgraph: %u contigs (an event holds fewer than 2^24)", ref.n_contigs);
    const uint64_t n = n_events + 4ull * ref.n_contigs;
    if (n >= (1ull << 31)) return fail(c, BRX_E_ARG, "brx_depth_bedgraph: %llu events and %u contigs: fewer than 2^31 keys in one call", (unsigned long long)n_events, ref.n_contigs);
    const DpPlan P = dp_plan(n);
    Call K(c, hip_stream);
    if (scratch_bytes < P.bytes) return K.need_scratch("brx_depth_bedgraph", scratch_bytes, P.bytes);
    BRX_TRY(K.begin());
    hipStream_t st = K.st;
    uint64_t *keys[2] = { Carver::at<uint64_t>(d_scratch, P.keys_a), Carver::at<uint64_t>(d_scratch, P.keys_b) };
    uint64_t *gk = Carver::at<uint64_t>(d_scratch, P.gk), *incl = Carver::at<uint64_t>(d_scratch, P.incl), *sums = Carver::at<uint64_t>(d_scratch, P.sums);
    uint32_t *gd = Carver::at<uint32_t>(d_scratch, P.gd), *cd = Carver::at<uint32_t>(d_scratch, P.cd);
    uint32_t *table = Carver::at<uint32_t>(d_scratch, P.table), *err = Carver::at<uint32_t>(d_scratch, P.flags);
    const brx_contig *ct = ref.d_contigs;
    const uint32_t nt = P.n_tiles;
    double t0 = dp_now_ms();
    /* the digits that can vary: the bytes of (the longest contig's length << 1 | 1) below bit 40, those of the last contig's index above */
    uint32_t longest = 0;
    {
        std::vector<brx_contig> h(ref.n_contigs);
        BRX_TRY(K.read_back(h.data(), ct, sizeof(brx_contig) * ref.n_contigs));
        BRX_TRY(K.wait("brx_depth_bedgraph (contigs)"));
        for (const brx_contig &x : h) longest = std::max(longest, x.length);
    }
    uint32_t shifts[8], n_pass = 0;
    for (uint32_t b = 0; b < 5; ++b) if (((((uint64_t)longest << 1) | 1u) >> (8 * b)) != 0) shifts[n_pass++] = 8 * b;
    for (uint32_t b = 0; b < 3; ++b) if (((uint64_t)(ref.n_contigs - 1) >> (8 * b)) != 0) shifts[n_pass++] = 40 + 8 * b;
    c->depth_passes = n_pass;
    HIPCHK(c, hipMemsetAsync(err, 0, 256, st));
    const DpSrcTable tab = { table };
    auto pass = [&](auto in, auto check, uint32_t shift, uint64_t *dst) {       /* the first pass reads the caller's events and checks them */
        using Keys = decltype(in);
        hipLaunchKernelGGL((k_dp_hist<Keys, decltype(check)::value>), dim3(nt), dim3(BRX_DP_THREADS), 0, st, in, n, shift, nt, table, n_events, ct, ref.n_contigs, err);
        dp_scan(st, tab, 256ull * nt, sums, incl);
        hipLaunchKernelGGL((k_dp_scatter<Keys>), dim3(nt), dim3(BRX_DP_THREADS), 0, st, in, n, shift, nt, (const uint32_t *)table, (const uint64_t *)incl, dst);
    };
    pass(DpKeysIn{ d_events, n_events, ct }, std::true_type{}, shifts[0], keys[0]);
    for (uint32_t p = 1; p < n_pass; ++p) pass(DpKeysBuf{ keys[(p - 1) & 1u] }, std::false_type{}, shifts[p], keys[p & 1u]);
    uint64_t *sorted = keys[(n_pass - 1) & 1u], *spare = keys[n_pass & 1u];
    uint32_t bad = 0;
    BRX_TRY(K.read_back(&bad, err, 4));
    BRX_TRY(K.sync("brx_depth_bedgraph (sort)"));
    if (bad) return fail(c, BRX_E_ARG, "brx_depth_bedgraph: an event names a contig outside the reference or a position beyond its contig");
    double t1 = dp_now_ms();
    c->depth_ms[0] = (float)(t1 - t0);
    /* depth: from here on the keys are known to name contigs of the reference */
    const DpSrcPack pack = { sorted, n };
    dp_scan(st, pack, n, sums, spare);
    hipLaunchKernelGGL(k_dp_groups, dim3((uint32_t)((n + BRX_DP_THREADS - 1) / BRX_DP_THREADS)), dim3(BRX_DP_THREADS), 0, st, (const uint64_t *)sorted, (const uint64_t *)spare, n, gk, gd, err);
    uint64_t last = 0;
    BRX_TRY(K.read_back(&last, spare + (n - 1), 8));
    BRX_TRY(K.read_back(&bad, err, 4));
    BRX_TRY(K.sync("brx_depth_bedgraph (depth)"));
    if (bad) return fail(c, BRX_E_ARG, "brx_depth_bedgraph: the events are not pairs of a start and a later end (depth below 0, or not 0 at a contig's end)");
    const uint64_t n_groups = last >> 32;
    const DpSrcChange change = { gk, gd, ct };
    dp_scan(st, change, n_groups, sums, spare);
    uint64_t *ck = sorted;                               /* the sorted keys have been read for the last time */
    hipLaunchKernelGGL(k_dp_points, dim3((uint32_t)((n_groups + BRX_DP_THREADS - 1) / BRX_DP_THREADS)), dim3(BRX_DP_THREADS), 0, st, change, (const uint64_t *)spare, n_groups, ck, cd);
    uint64_t n_points = 0;
    BRX_TRY(K.read_back(&n_points, spare + (n_groups - 1), 8));
    BRX_TRY(K.sync("brx_depth_bedgraph (change points)"));
    double t2 = dp_now_ms();
    c->depth_ms[1] = (float)(t2 - t1);
    /* text */
    const DpSrcLine line = { ck, cd, ct };
    dp_scan(st, line, n_points, sums, spare);
    uint64_t total = 0;
    BRX_TRY(K.read_back(&total, spare + (n_points - 1), 8));
    BRX_TRY(K.wait("brx_depth_bedgraph (line sizes)"));
    if (total > out_cap || (total && !d_out)) return K.need_output((size_t)total, "brx_depth_bedgraph: output buffer too small: need %llu bytes", (unsigned long long)total);
    hipLaunchKernelGGL(k_dp_lines, dim3((uint32_t)((n_points + BRX_DP_THREADS - 1) / BRX_DP_THREADS)), dim3(BRX_DP_THREADS), 0, st, line, (const uint64_t *)spare, n_points, ref.d_names, d_out);
    BRX_TRY(K.sync("brx_depth_bedgraph (text)"));
    c->depth_ms[2] = (float)(dp_now_ms() - t2);
    *out_bytes = (size_t)total;
    return BRX_OK;
}

/* ---- the truth BAM in coordinate order and its index (brx_bamsort.h) ---- */
static uint32_t bs_blocks(uint64_t n) { return (uint32_t)((n + BRX_BS_THREADS - 1) / BRX_BS_THREADS); }
/* the sort's own pieces for n keys, in every plan that sorts */
struct BsSortPlan { size_t keys[2], pay[2], table, incl; };
static BsSortPlan bs_sort_plan(Carver &V, uint64_t n) {
    const uint64_t cells = 256ull * ((n + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE);
    BsSortPlan p;
    p.keys[0] = V.take(n * 8); p.keys[1] = V.take(n * 8); p.pay[0] = V.take(n * 4); p.pay[1] = V.take(n * 4);
    p.table = V.take(cells * 4); p.incl = V.take(cells * 8);
    return p;
}
static BsSort bs_sort_at(void *d_scratch, const BsSortPlan &p, uint64_t *sums) {
    BsSort S;
    for (int x = 0; x < 2; ++x) { S.keys[x] = Carver::at<uint64_t>(d_scratch, p.keys[x]); S.pay[x] = Carver::at<uint32_t>(d_scratch, p.pay[x]); }
    S.table = Carver::at<uint32_t>(d_scratch, p.table); S.incl = Carver::at<uint64_t>(d_scratch, p.incl); S.sums = sums;
    return S;
}
/* the words for the tile sums of a scan over up to `longest` elements */
static uint64_t bs_sums_bytes(uint64_t longest) { return ((longest + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE + 1) * 8; }

/* where brx_bam_sort keeps what in its scratch, for n_rec records in n_seg segments.  Sized twice: before the walk for the records that
   brx_bam_sort_scratch assumes, after it for the count found. */
struct BsPlan { size_t cnt, seg_incl, src, len, incl_len, sums, flags, bytes; BsSortPlan sort; };
static BsPlan bs_plan(uint64_t n_rec, uint64_t n_seg) {
    BsPlan p;
    Carver V;
    p.cnt = V.take(n_seg * 4); p.seg_incl = V.take(n_seg * 8); p.flags = V.take(256);
    p.src = V.take(n_rec * 8); p.len = V.take(n_rec * 4); p.incl_len = V.take(n_rec * 8);
    p.sort = bs_sort_plan(V, n_rec);
    p.sums = V.take(bs_sums_bytes(std::max<uint64_t>(std::max<uint64_t>(n_rec, 256ull * ((n_rec + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE)), n_seg)));
    p.bytes = V.bytes();
    return p;
}
extern "C" size_t brx_bam_sort_scratch(uint64_t n_bytes, uint64_t n_seg) { return bs_plan(n_bytes / 4096 + n_seg + 64, n_seg).bytes; }
extern "C" int brx_bamsort_last(const brx_ctx *c, float ms[8]) { return last_ms(c, &brx_ctx::bamsort_ms, ms); }

extern "C" int brx_bam_sort(brx_ctx *c, const uint8_t *d_records, uint64_t n_bytes, const uint64_t *d_seg_off, uint64_t n_seg, uint32_t n_ref, uint32_t max_pos,
                            uint8_t *d_sorted, brx_bam_rec *d_recs, uint64_t rec_cap, uint64_t *n_records, uint64_t *n_unmapped, void *d_scratch,
                            size_t scratch_bytes, void *hip_stream) {
    if (!c) return BRX_E_ARG;
    if (!n_records || !n_unmapped) return fail(c, BRX_E_ARG, "brx_bam_sort: n_records or n_unmapped is NULL");
    *n_records = 0; *n_unmapped = 0;
    if (n_bytes == 0) return BRX_OK;
    if (!d_records || !d_seg_off || !d_sorted || n_seg == 0) return fail(c, BRX_E_ARG, "brx_bam_sort: the records, the segment offsets or d_sorted is NULL");
    if (n_bytes >= (1ull << 43) || n_seg >= (1ull << 32)) return fail(c, BRX_E_ARG, "brx_bam_sort: %llu bytes in %llu segments: fewer than 2^43 and 2^32 in one call", (unsigned long long)n_bytes, (unsigned long long)n_seg);
    if (max_pos > (1u << 31)) return fail(c, BRX_E_ARG, "brx_bam_sort: max_pos %u above 2^31", max_pos);
    BsPlan P = bs_plan(0, n_seg);
    Call K(c, hip_stream);
    const size_t least = brx_bam_sort_scratch(n_bytes, n_seg);
    if (!d_scratch || scratch_bytes < least) return K.need_scratch("brx_bam_sort", d_scratch ? scratch_bytes : (size_t)0, least);
    BRX_TRY(K.begin());
    hipStream_t st = K.st;
    /* cnt, seg_incl and flags lie in front of everything that is sized by the records: the same places in both plans */
    uint32_t *cnt = Carver::at<uint32_t>(d_scratch, P.cnt), *flags = Carver::at<uint32_t>(d_scratch, P.flags);
    uint64_t *seg_incl = Carver::at<uint64_t>(d_scratch, P.seg_incl);
    uint64_t *first_unmapped = (uint64_t *)(flags + 2);
    /* the tile sums of the first scan: behind the pieces of a plan without records, where the plan with them puts its record arrays */
    uint64_t *sums0 = Carver::at<uint64_t>(d_scratch, P.sums);
    const BsIn in = { d_records, n_bytes, d_seg_off, n_seg, n_ref, max_pos };
    K.mark(0);
    HIPCHK(c, hipMemsetAsync(flags, 0, 256, st));
    hipLaunchKernelGGL((k_bs_walk<false>), dim3(bs_blocks(n_seg)), dim3(BRX_BS_THREADS), 0, st, in, cnt, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr,
                       (uint32_t *)nullptr, flags);
    const DpSrcTable counts = { cnt };
    dp_scan(st, counts, n_seg, sums0, seg_incl);
    uint32_t bad = 0;
    uint64_t n = 0;
    BRX_TRY(K.read_back(&bad, flags, 4));
    BRX_TRY(K.read_back(&n, seg_incl + (n_seg - 1), 8));
    BRX_TRY(K.sync("brx_bam_sort (walk)"));
    if (bad) return fail(c, BRX_E_ARG, "brx_bam_sort: the segment offsets do not ascend from 0 to n_bytes, a record chain leaves its segment, or a record's "
                                       "block_size, refID or pos is out of range");
    if (n >= (1ull << 32)) return fail(c, BRX_E_ARG, "brx_bam_sort: %llu records: fewer than 2^32 in one call", (unsigned long long)n);
    if (n > rec_cap || !d_recs) return K.need_output((size_t)n, "brx_bam_sort: room for %llu records, %llu in the input", (unsigned long long)(d_recs ? rec_cap : 0), (unsigned long long)n);
    P = bs_plan(n, n_seg);
    if (scratch_bytes < P.bytes) {
        char detail[48];
        snprintf(detail, sizeof(detail), " for %llu records", (unsigned long long)n);
        return K.need_scratch("brx_bam_sort", scratch_bytes, P.bytes, detail);
    }
    uint64_t *src = Carver::at<uint64_t>(d_scratch, P.src), *incl_len = Carver::at<uint64_t>(d_scratch, P.incl_len), *sums = Carver::at<uint64_t>(d_scratch, P.sums);
    uint32_t *len = Carver::at<uint32_t>(d_scratch, P.len);
    const BsSort S = bs_sort_at(d_scratch, P.sort, sums);
    hipLaunchKernelGGL((k_bs_walk<true>), dim3(bs_blocks(n_seg)), dim3(BRX_BS_THREADS), 0, st, in, cnt, (const uint64_t *)seg_incl, src, S.keys[0], len, flags);
    K.mark(1);
    /* the digits that can vary: the bytes of max_pos - 1 in the low word, those of n_ref (the state of refID -1) in the high word */
    uint32_t shifts[8], n_pass = 0;
    for (uint32_t b = 0; b < 4; ++b) if (max_pos && ((max_pos - 1u) >> (8 * b)) != 0) shifts[n_pass++] = 8 * b;
    for (uint32_t b = 0; b < 4; ++b) if ((n_ref >> (8 * b)) != 0) shifts[n_pass++] = 32 + 8 * b;
    if (!n_pass) shifts[n_pass++] = 0;
    const uint32_t r = bs_sort(st, S, n, shifts, n_pass);
    const uint64_t *skey = S.keys[r];
    const uint32_t *spay = S.pay[r];
    uint64_t *ssrc = S.keys[r ^ 1u];                         /* the other side of the last pass has been read for the last time */
    K.mark(2);
    const BsSrcLen lens = { len, spay };
    dp_scan(st, lens, n, sums, incl_len);
    HIPCHK(c, hipMemcpyAsync(first_unmapped, &n, 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bs_table, dim3((uint32_t)((n + 3) / 4)), dim3(BRX_BS_THREADS), 0, st, d_records, (const uint64_t *)src, spay, (const uint32_t *)len,
                       (const uint64_t *)incl_len, skey, n, n_ref, d_recs, ssrc, first_unmapped);
    K.mark(3);
    const bool wide = ((uintptr_t)d_records & 3u) == 0, aligned = ((uintptr_t)d_sorted & 15u) == 0;
    hipLaunchKernelGGL(k_bs_gather, dim3((uint32_t)((n_bytes + BRX_BS_SPAN - 1) / BRX_BS_SPAN)), dim3(BRX_BS_THREADS), 0, st, d_records, n_bytes, (const uint64_t *)incl_len,
                       (const uint64_t *)ssrc, n, d_sorted, wide, aligned);
    K.mark(4);
    uint64_t first = 0;
    BRX_TRY(K.read_back(&first, first_unmapped, 8));
    BRX_TRY(K.sync("brx_bam_sort"));
    for (int i = 0; i < 4; ++i) BRX_TRY(K.elapsed(&c->bamsort_ms[i], i, i + 1));
    *n_records = n;
    *n_unmapped = n - first;
    return BRX_OK;
}

/* where brx_bam_index keeps what in its scratch, for n records (no more chunks than records) of n_ref contigs */
struct BiPlan { size_t starts, maxend, cbeg, cend, hincl, head, cf, rf, winc, cbase, sums, flags, bytes; BsSortPlan sort; };
static BiPlan bi_plan(uint64_t n, uint32_t n_ref) {
    BiPlan p;
    Carver V;
    p.starts = V.take(n * 8); p.maxend = V.take(n * 8); p.cbeg = V.take(n * 8); p.cend = V.take(n * 8); p.hincl = V.take(n * 8); p.head = V.take((n + 1) * 8);
    p.cf = V.take(((uint64_t)n_ref + 1) * 8); p.rf = V.take(((uint64_t)n_ref + 1) * 8); p.winc = V.take(((uint64_t)n_ref + 1) * 8); p.cbase = V.take(((uint64_t)n_ref + 1) * 8);
    p.sort = bs_sort_plan(V, n);
    p.sums = V.take(bs_sums_bytes(std::max<uint64_t>(std::max<uint64_t>(n, 256ull * ((n + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE)), n_ref)));
    p.flags = V.take(256);
    p.bytes = V.bytes();
    return p;
}
extern "C" size_t brx_bam_index_scratch(uint64_t n_records, uint32_t n_ref) { return bi_plan(n_records, n_ref).bytes; }

extern "C" int brx_bam_index(brx_ctx *c, const brx_bam_rec *d_recs, uint64_t n, uint32_t n_ref, uint64_t n_bytes, const uint64_t *d_block_off, uint64_t n_blocks,
                             uint64_t base, uint8_t *d_out, size_t out_cap, size_t *out_bytes, void *d_scratch, size_t scratch_bytes, void *hip_stream) {
    if (!c) return BRX_E_ARG;
    if (!out_bytes) return fail(c, BRX_E_ARG, "brx_bam_index: out_bytes is NULL");
    *out_bytes = 0;
    if (n && (!d_recs || !n_bytes)) return fail(c, BRX_E_ARG, "brx_bam_index: records without a table or without a stream");
    if (!d_block_off) return fail(c, BRX_E_ARG, "brx_bam_index: d_block_off is NULL");
    if (n >= (1ull << 32)) return fail(c, BRX_E_ARG, "brx_bam_index: %llu records: fewer than 2^32 in one call", (unsigned long long)n);
    if (n_ref > 0x7FFFFFFFu) return fail(c, BRX_E_ARG, "brx_bam_index: n_ref %u", n_ref);
    if (n_blocks != (n_bytes + BRX_BGZF_BLOCK - 1) / BRX_BGZF_BLOCK)
        return fail(c, BRX_E_ARG, "brx_bam_index: %llu blocks for %llu bytes, one per %u", (unsigned long long)n_blocks, (unsigned long long)n_bytes, BRX_BGZF_BLOCK);
    if (base >= (1ull << 48)) return fail(c, BRX_E_ARG, "brx_bam_index: base of 2^48 or more");
    if ((uintptr_t)d_out & 3u) return fail(c, BRX_E_ARG, "brx_bam_index: the output buffer must be 4-byte aligned");
    const BiPlan P = bi_plan(n, n_ref);
    Call K(c, hip_stream);
    if (!d_scratch || scratch_bytes < P.bytes) return K.need_scratch("brx_bam_index", d_scratch ? scratch_bytes : (size_t)0, P.bytes);
    BRX_TRY(K.begin());
    hipStream_t st = K.st;
    uint64_t *starts = Carver::at<uint64_t>(d_scratch, P.starts), *M = Carver::at<uint64_t>(d_scratch, P.maxend), *cbeg = Carver::at<uint64_t>(d_scratch, P.cbeg);
    uint64_t *cend = Carver::at<uint64_t>(d_scratch, P.cend), *hincl = Carver::at<uint64_t>(d_scratch, P.hincl), *head = Carver::at<uint64_t>(d_scratch, P.head);
    uint64_t *cf = Carver::at<uint64_t>(d_scratch, P.cf), *rf = Carver::at<uint64_t>(d_scratch, P.rf), *winc = Carver::at<uint64_t>(d_scratch, P.winc);
    uint64_t *cbase = Carver::at<uint64_t>(d_scratch, P.cbase), *sums = Carver::at<uint64_t>(d_scratch, P.sums);
    uint32_t *err = Carver::at<uint32_t>(d_scratch, P.flags);
    const BsSort S = bs_sort_at(d_scratch, P.sort, sums);
    const BiVoff voff = { d_block_off, base };
    K.mark(0);
    HIPCHK(c, hipMemsetAsync(err, 0, 256, st));
    hipLaunchKernelGGL(k_bi_check, dim3(bs_blocks(std::max<uint64_t>(n, n_blocks + 1))), dim3(BRX_BS_THREADS), 0, st, d_recs, n, n_ref, n_bytes, d_block_off, n_blocks + 1, base, err);
    uint32_t bad = 0;
    BRX_TRY(K.read_back(&bad, err, 4));
    BRX_TRY(K.sync("brx_bam_index (check)"));
    if (bad) return fail(c, BRX_E_ARG, "brx_bam_index: the table is not sorted, a refID, pos, end or offset is out of range, or the block offsets descend or reach 2^48");
    /* chunks: from here on every record names a contig of the index or none */
    uint64_t m = 0;
    if (n) {
        const BiSrcStart start = { d_recs };
        dp_scan(st, start, n, sums, starts);
        hipLaunchKernelGGL(k_bi_chunks, dim3(bs_blocks(n)), dim3(BRX_BS_THREADS), 0, st, start, (const uint64_t *)starts, n, n_bytes, voff, S.keys[0], cbeg, cend);
        BRX_TRY(K.read_back(&m, starts + (n - 1), 8));
        BRX_TRY(K.wait("brx_bam_index (chunks)"));
    }
    K.mark(1);
    const uint64_t *skey = nullptr;
    const uint32_t *spay = nullptr;
    if (m) {
        uint32_t shifts[6], n_pass = 0;
        shifts[n_pass++] = 0; shifts[n_pass++] = 8;          /* the bin, then the bytes of the last contig's index */
        for (uint32_t b = 0; b < 4; ++b) if (((n_ref - 1u) >> (8 * b)) != 0) shifts[n_pass++] = 32 + 8 * b;
        const uint32_t r = bs_sort(st, S, m, shifts, n_pass);
        skey = S.keys[r]; spay = S.pay[r];
        const BiSrcHead heads = { skey };
        dp_scan(st, heads, m, sums, hincl);
        hipLaunchKernelGGL(k_bi_heads, dim3(bs_blocks(m)), dim3(BRX_BS_THREADS), 0, st, heads, (const uint64_t *)hincl, m, head);
    }
    K.mark(2);
    hipLaunchKernelGGL(k_bi_contigs, dim3(bs_blocks((uint64_t)n_ref + 1)), dim3(BRX_BS_THREADS), 0, st, d_recs, n, skey, m, n_ref, cf, rf);
    const BiLayout L = { cf, hincl, winc };
    uint64_t n_win = 0, body = 0;
    if (n_ref) {
        if (n) { const BiSrcEnd ends = { d_recs }; bx_max_scan(st, ends, n, sums, M); }
        const BiSrcIntv intv = { rf, M };
        dp_scan(st, intv, n_ref, sums, winc);
        dp_scan(st, L, n_ref, sums, cbase);
        BRX_TRY(K.read_back(&n_win, winc + (n_ref - 1), 8));
        BRX_TRY(K.read_back(&body, cbase + (n_ref - 1), 8));
    }
    K.mark(3);
    BRX_TRY(K.wait("brx_bam_index (sizes)"));
    const uint64_t total = 8 + body + 8;
    if (total > out_cap || !d_out) return K.need_output((size_t)total, "brx_bam_index: output buffer too small: need %llu bytes", (unsigned long long)total);
    hipLaunchKernelGGL(k_bi_put_contigs, dim3(bs_blocks((uint64_t)n_ref + 1)), dim3(BRX_BS_THREADS), 0, st, L, (const uint64_t *)cbase, (const uint64_t *)rf, n, n_ref, total, d_out);
    if (n_win) hipLaunchKernelGGL(k_bi_put_windows, dim3(bs_blocks(n_win)), dim3(BRX_BS_THREADS), 0, st, L, (const uint64_t *)cbase, (const uint64_t *)rf, (const uint64_t *)M, d_recs,
                                  n_ref, n_win, voff, d_out);
    if (m) hipLaunchKernelGGL(k_bi_put_chunks, dim3(bs_blocks(m)), dim3(BRX_BS_THREADS), 0, st, L, (const uint64_t *)cbase, skey, spay, m, (const uint64_t *)head,
                              (const uint64_t *)cbeg, (const uint64_t *)cend, d_out);
    K.mark(4);
    BRX_TRY(K.sync("brx_bam_index"));
    for (int i = 0; i < 4; ++i) BRX_TRY(K.elapsed(&c->bamsort_ms[4 + i], i, i + 1));
    *out_bytes = (size_t)total;
    return BRX_OK;
}

/* ---- window identities (brx_window.h) ---- */
struct PwPlan { uint32_t n_tiles; size_t err, pe, pq, sums, bytes; };
static PwPlan pw_plan(uint64_t n_bases, int want_qual) {
    PwPlan p; p.n_tiles = (uint32_t)((n_bases + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE);
    Carver V;
    p.err = V.take(n_bases * 4); p.pe = V.take((n_bases + 1) * 8); p.pq = V.take(want_qual ? (n_bases + 1) * 8 : 0);
    p.sums = V.take(((uint64_t)p.n_tiles + 1) * 8);
    p.bytes = V.bytes();
    return p;
}
extern "C" size_t brx_window_scratch(uint64_t n_bases, int want_qual) { return pw_plan(n_bases, want_qual).bytes; }
extern "C" int brx_window_last(const brx_ctx *c, float ms[4]) { return last_ms(c, &brx_ctx::window_ms, ms); }
extern "C" int brx_window_means(brx_ctx *c, const brx_window_job *job, void *hip_stream) {
    if (!c || !job) return BRX_E_ARG;
    const brx_window_job j = *job;
    if (j.window == 0) return fail(c, BRX_E_ARG, "brx_window_means: window 0");
    if (j.n_align == 0) return BRX_OK;
    if (!j.d_align_read_off || !j.d_align_part_off || !j.d_align_win_off || !j.d_stat) return fail(c, BRX_E_ARG, "brx_window_means: an offset array or d_stat is NULL");
    if (j.n_bases && (!j.d_seq || !j.d_ref || !j.d_part_type || !j.d_part_len || !j.d_part_read || !j.d_part_ref || (j.want_qual && !j.d_qual)))
        return fail(c, BRX_E_ARG, "brx_window_means: a slice or part array is NULL");
    if (j.n_bases >= (1ull << 39)) return fail(c, BRX_E_ARG, "brx_window_means: %llu read bases: fewer than 2^39 in one call", (unsigned long long)j.n_bases);
    if (j.n_windows > j.n_bases) return fail(c, BRX_E_ARG, "brx_window_means: more windows than read bases");
    const PwPlan P = pw_plan(j.n_bases, (int)j.want_qual);
    Call K(c, hip_stream);
    if (!j.d_scratch || j.scratch_bytes < P.bytes) return K.need_scratch("brx_window_means", j.scratch_bytes, P.bytes);
    BRX_TRY(K.begin());
    hipStream_t st = K.st;
    uint32_t *err = Carver::at<uint32_t>(j.d_scratch, P.err);
    uint64_t *pe = Carver::at<uint64_t>(j.d_scratch, P.pe), *pq = j.want_qual ? Carver::at<uint64_t>(j.d_scratch, P.pq) : nullptr;
    uint64_t *sums = Carver::at<uint64_t>(j.d_scratch, P.sums);
    K.mark(0);                                               /* five marks: errors, scans, statistics, values */
    if (j.n_bases) {
        hipLaunchKernelGGL(k_pw_errors, dim3((uint32_t)((j.n_bases + BRX_PW_THREADS - 1) / BRX_PW_THREADS)), dim3(BRX_PW_THREADS), 0, st, j, err, pe, pq);
        K.mark(1);
        const DpSrcTable e = { err };
        dp_scan(st, e, j.n_bases, sums, pe + 1);
        if (pq) { const PwSrcQual q = { j.d_qual }; dp_scan(st, q, j.n_bases, sums, pq + 1); }
    } else K.mark(1);
    K.mark(2);
    hipLaunchKernelGGL(k_pw_stats, dim3(j.n_align), dim3(BRX_PW_THREADS), 0, st, j, (const uint64_t *)pe, (const uint64_t *)pq);
    K.mark(3);
    if (j.n_windows && (j.d_err_sum || j.d_qual_sum))
        hipLaunchKernelGGL(k_pw_values, dim3((uint32_t)((j.n_windows + BRX_PW_THREADS - 1) / BRX_PW_THREADS)), dim3(BRX_PW_THREADS), 0, st, j, (const uint64_t *)pe, (const uint64_t *)pq);
    K.mark(4);
    BRX_TRY(K.sync("brx_window_means"));
    for (int i = 0; i < 4; ++i) BRX_TRY(K.elapsed(&c->window_ms[i], i, i + 1));
    return BRX_OK;
}

/* ---- the device loader (brx_pafin.h) ---- */
struct PiPlan { uint32_t n_tiles; size_t incl, sums, flags, bytes; };
static PiPlan pi_plan(uint64_t n_bytes) {
    PiPlan p; p.n_tiles = (uint32_t)((n_bytes + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE);
    Carver V;
    p.incl = V.take(n_bytes * 8); p.sums = V.take(((uint64_t)p.n_tiles + 1) * 8); p.flags = V.take(256);
    p.bytes = V.bytes();
    return p;
}
extern "C" size_t brx_paf_scan_scratch(uint64_t n_bytes) { return pi_plan(n_bytes).bytes; }
extern "C" int brx_loader_last(const brx_ctx *c, float ms[2]) { return last_ms(c, &brx_ctx::loader_ms, ms); }
extern "C" int brx_paf_scan(brx_ctx *c, const uint8_t *d_text, uint64_t n_bytes, uint64_t max_lines, brx_paf_line *d_lines, uint64_t line_cap,
                            uint64_t *n_lines, void *d_scratch, size_t scratch_bytes, void *hip_stream) {
    if (!c) return BRX_E_ARG;
    if (!n_lines) return fail(c, BRX_E_ARG, "brx_paf_scan: n_lines is NULL");
    *n_lines = 0;
    if (n_bytes == 0) return BRX_OK;
    if (!d_text) return fail(c, BRX_E_ARG, "brx_paf_scan: d_text is NULL");
    if (n_bytes >= (1ull << 42)) return fail(c, BRX_E_ARG, "brx_paf_scan: %llu bytes: fewer than 2^42 in one call", (unsigned long long)n_bytes);
    const PiPlan P = pi_plan(n_bytes);
    Call K(c, hip_stream);
    if (!d_scratch || scratch_bytes < P.bytes) return K.need_scratch("brx_paf_scan", d_scratch ? scratch_bytes : (size_t)0, P.bytes);
    BRX_TRY(K.begin());
    hipStream_t st = K.st;
    uint64_t *incl = Carver::at<uint64_t>(d_scratch, P.incl), *sums = Carver::at<uint64_t>(d_scratch, P.sums);
    uint32_t *err = Carver::at<uint32_t>(d_scratch, P.flags);
    K.mark(0);
    HIPCHK(c, hipMemsetAsync(err, 0, 256, st));
    const PiSrcStart start = { d_text };
    dp_scan(st, start, n_bytes, sums, incl);
    uint64_t total = 0;
    BRX_TRY(K.read_back(&total, incl + (n_bytes - 1), 8));
    BRX_TRY(K.sync("brx_paf_scan (line starts)"));
    const uint64_t n = max_lines && max_lines < total ? max_lines : total;
    if (n >= (1ull << 31)) return fail(c, BRX_E_ARG, "brx_paf_scan: %llu lines: fewer than 2^31 in one call", (unsigned long long)n);
    if (n > line_cap || !d_lines)
        return K.need_output((size_t)n, "brx_paf_scan: room for %llu records, %llu lines", (unsigned long long)(d_lines ? line_cap : 0), (unsigned long long)n);
    hipLaunchKernelGGL(k_pi_starts, dim3((uint32_t)((n_bytes + BRX_PI_THREADS - 1) / BRX_PI_THREADS)), dim3(BRX_PI_THREADS), 0, st, start, n_bytes, (const uint64_t *)incl, n, d_lines);
    hipLaunchKernelGGL(k_pi_lines, dim3((uint32_t)n), dim3(64), 0, st, d_text, n_bytes, d_lines, err);
    uint32_t bad = 0;
    BRX_TRY(K.read_back(&bad, err, 4));
    K.mark(1);
    BRX_TRY(K.sync("brx_paf_scan"));
    BRX_TRY(K.elapsed(&c->loader_ms[0], 0, 1));
    if (bad) return fail(c, BRX_E_ARG, "brx_paf_scan: a line of 2^32 bytes or more");
    *n_lines = n;
    return BRX_OK;
}

extern "C" int brx_align_pack(brx_ctx *c, const brx_pack_job *job, void *hip_stream) {
    if (!c || !job) return BRX_E_ARG;
    const brx_pack_job j = *job;
    if (j.n_align == 0) return BRX_OK;
    if (!j.d_align || !j.d_align_part_off || !j.d_align_col_off || !j.d_align_read_off || !j.d_align_ref_off)
        return fail(c, BRX_E_ARG, "brx_align_pack: d_align or an offset array is NULL");
    if (!j.d_text || !j.d_reftext || !j.d_complement || !j.d_part_type || !j.d_part_len || !j.d_part_col || !j.d_part_read || !j.d_part_ref || !j.d_ref || !j.d_flags)
        return fail(c, BRX_E_ARG, "brx_align_pack: a text, the complement table, an output array or d_flags is NULL");
    Call K(c, hip_stream);
    BRX_TRY(K.begin());
    K.mark(0);
    hipLaunchKernelGGL(k_pi_pack, dim3(j.n_align), dim3(64), 0, K.st, j, j.d_flags);
    K.mark(1);
    uint32_t bad = 0;
    BRX_TRY(K.read_back(&bad, j.d_flags, 4));
    BRX_TRY(K.sync("brx_align_pack"));
    BRX_TRY(K.elapsed(&c->loader_ms[1], 0, 1));
    if (bad) return fail(c, BRX_E_ARG, "brx_align_pack: an alignment's descriptor does not fit its CIGAR, the texts or the offset arrays");
    return BRX_OK;
}

/* ---- the device read loader (brx_fastqin.h) ---- */
/* where brx_fastq_scan keeps what in its scratch: the scan's prefix per group of 16 bytes, the tile sums, the flags, the line starts.
   Sized twice: before the scan for the line count that brx_fastq_scan_scratch assumes, after it for the count found. */
struct FqPlan { uint64_t n_groups; uint32_t n_tiles; size_t incl, sums, flags, lines, bytes; };
static FqPlan fq_plan(uint64_t n_bytes, uint64_t n_lines) {
    FqPlan p; p.n_groups = (n_bytes + 15) / 16; p.n_tiles = (uint32_t)((p.n_groups + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE);
    Carver V;
    p.incl = V.take(p.n_groups * 8); p.sums = V.take(((uint64_t)p.n_tiles + 1) * 8); p.flags = V.take(256); p.lines = V.take((n_lines + 1) * 8);
    p.bytes = V.bytes();
    return p;
}
extern "C" size_t brx_fastq_scan_scratch(uint64_t n_bytes) { return fq_plan(n_bytes, n_bytes / 64 + 64).bytes; }
extern "C" int brx_reads_last(const brx_ctx *c, float ms[2]) { return last_ms(c, &brx_ctx::reads_ms, ms); }
extern "C" int brx_fastq_scan(brx_ctx *c, const uint8_t *d_text, uint64_t n_bytes, brx_fastq_rec *d_recs, uint64_t rec_cap, uint64_t *n_recs,
                              uint32_t *layout, void *d_scratch, size_t scratch_bytes, void *hip_stream) {
    if (!c) return BRX_E_ARG;
    if (!n_recs || !layout) return fail(c, BRX_E_ARG, "brx_fastq_scan: n_recs or layout is NULL");
    *n_recs = 0; *layout = 0;
    if (n_bytes == 0) return BRX_OK;
    if (!d_text) return fail(c, BRX_E_ARG, "brx_fastq_scan: d_text is NULL");
    if (n_bytes >= (1ull << 42)) return fail(c, BRX_E_ARG, "brx_fastq_scan: %llu bytes: fewer than 2^42 in one call", (unsigned long long)n_bytes);
    const size_t least = brx_fastq_scan_scratch(n_bytes);
    Call K(c, hip_stream);
    if (!d_scratch || scratch_bytes < least) return K.need_scratch("brx_fastq_scan", d_scratch ? scratch_bytes : (size_t)0, least);
    BRX_TRY(K.begin());
    hipStream_t st = K.st;
    FqPlan P = fq_plan(n_bytes, 0);
    uint64_t *incl = Carver::at<uint64_t>(d_scratch, P.incl), *sums = Carver::at<uint64_t>(d_scratch, P.sums);
    uint32_t *flags = Carver::at<uint32_t>(d_scratch, P.flags);
    K.mark(0);
    HIPCHK(c, hipMemsetAsync(flags, 0, 256, st));
    const FqSrcStarts16 src = { d_text, n_bytes };
    dp_scan(st, src, P.n_groups, sums, incl);
    uint64_t n_lines = 0;
    BRX_TRY(K.read_back(&n_lines, incl + (P.n_groups - 1), 8));
    BRX_TRY(K.sync("brx_fastq_scan (line starts)"));
    if (n_lines & 3u) { *layout = BRX_FQ_LINES; return BRX_OK; }
    const uint64_t n = n_lines / 4;
    if (n >= (1ull << 31)) return fail(c, BRX_E_ARG, "brx_fastq_scan: %llu records: fewer than 2^31 in one call", (unsigned long long)n);
    if (n > rec_cap || !d_recs)
        return K.need_output((size_t)n, "brx_fastq_scan: room for %llu records, %llu in the file", (unsigned long long)(d_recs ? rec_cap : 0), (unsigned long long)n);
    P = fq_plan(n_bytes, n_lines);
    if (scratch_bytes < P.bytes) {
        char detail[48];
        snprintf(detail, sizeof(detail), " for %llu lines", (unsigned long long)n_lines);
        return K.need_scratch("brx_fastq_scan", scratch_bytes, P.bytes, detail);
    }
    uint64_t *line_start = Carver::at<uint64_t>(d_scratch, P.lines);
    hipLaunchKernelGGL(k_fq_starts, dim3((uint32_t)((P.n_groups + BRX_FQ_THREADS - 1) / BRX_FQ_THREADS)), dim3(BRX_FQ_THREADS), 0, st, src, P.n_groups, (const uint64_t *)incl, line_start, flags);
    hipLaunchKernelGGL(k_fq_records, dim3((uint32_t)((n + BRX_FQ_THREADS - 1) / BRX_FQ_THREADS)), dim3(BRX_FQ_THREADS), 0, st, d_text, (const uint64_t *)line_start, n, d_recs, flags);
    uint32_t got[3] = { 0, 0, 0 };
    BRX_TRY(K.read_back(got, flags, sizeof(got)));
    K.mark(1);
    BRX_TRY(K.sync("brx_fastq_scan"));
    BRX_TRY(K.elapsed(&c->reads_ms[0], 0, 1));
    if (got[2]) return fail(c, BRX_E_ARG, "brx_fastq_scan: a line of 2^32 bytes or more");
    *layout = (got[0] ? BRX_FQ_HIGH : 0u) | (got[1] ? BRX_FQ_HEADER : 0u);
    if (*layout == 0) *n_recs = n;
    return BRX_OK;
}

extern "C" int brx_reads_pack(brx_ctx *c, const brx_reads_job *job, void *hip_stream) {
    if (!c || !job) return BRX_E_ARG;
    const brx_reads_job j = *job;
    if (j.n_align == 0) return BRX_OK;
    if (!j.d_seq_src || !j.d_qual_src || !j.d_align_read_off) return fail(c, BRX_E_ARG, "brx_reads_pack: a source or offset array is NULL");
    if (!j.d_text || !j.d_seq || !j.d_qual || !j.d_flags) return fail(c, BRX_E_ARG, "brx_reads_pack: the text, an output array or d_flags is NULL");
    Call K(c, hip_stream);
    BRX_TRY(K.begin());
    K.mark(0);
    hipLaunchKernelGGL(k_fq_check, dim3((j.n_align + BRX_FQ_THREADS - 1) / BRX_FQ_THREADS), dim3(BRX_FQ_THREADS), 0, K.st, j, j.d_flags);
    uint32_t bad = 0;
    uint64_t total = 0;
    BRX_TRY(K.read_back(&bad, j.d_flags, 4));
    BRX_TRY(K.read_back(&total, j.d_align_read_off + j.n_align, 8));
    BRX_TRY(K.sync("brx_reads_pack (check)"));
    if (bad) return fail(c, BRX_E_ARG, "brx_reads_pack: the offsets do not ascend from 0, or a source range leaves the text");
    const uint64_t n_tiles = (total + BRX_FQ_TILE - 1) / BRX_FQ_TILE;
    if (n_tiles >= (1ull << 31)) return fail(c, BRX_E_ARG, "brx_reads_pack: %llu read bases: fewer than 2^43 in one call", (unsigned long long)total);
    if (n_tiles) hipLaunchKernelGGL(k_fq_pack, dim3((uint32_t)n_tiles), dim3(BRX_FQ_THREADS), 0, K.st, j, total, ((uintptr_t)j.d_text & 3u) == 0);
    K.mark(1);
    BRX_TRY(K.sync("brx_reads_pack"));
    BRX_TRY(K.elapsed(&c->reads_ms[1], 0, 1));
    return BRX_OK;
}

#endif /* BRX_TOOLS_H */
