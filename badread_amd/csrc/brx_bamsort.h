/*
 * brx_bamsort.h -- the truth BAM in coordinate order with its BAI index (--truth-bam-sorted): the kernels of brx_bam_sort and
 * brx_bam_index (include/brx.h; the calls themselves are in brx_tools.h).  The scans are dp_scan of brx_scan.h, the histogram of the
 * radix sort is k_dp_hist of brx_depth.h as it is, the 16-byte loads and stores of the gather are those of brx_fastqin.h.
 *
 * brx_bam_sort, over uncompressed BAM records (brx_bam.h) back to back, cut into segments of whole records:
 *   1. k_bs_walk<false>, a thread per segment: the offsets ascend and end at n_bytes, then the segment's block_size chain.  Every load is
 *      tested against the segment's end first; a step advances by at least 36 bytes.  A record must hold its fixed fields, its name and
 *      its CIGAR words, name a contig of [-1, n_ref) and a position of [0, max_pos) (-1 on refID -1).  It leaves the records per segment.
 *   2. the scan of the counts; k_bs_walk<true> writes every record's source offset, key and length at its number.  key = refID << 32 |
 *      pos, and n_ref << 32 for refID -1: the order of ((uint32_t)refID, pos) with one state more than there are contigs.
 *   3. the sort of (key, record number): k_dp_hist, the scan of its table, k_bs_scatter -- k_dp_scatter with a 32-bit payload beside the
 *      key; the first pass makes the payload, the record's number.  Stable, so equal keys keep the order of the input.
 *   4. the scan of the lengths in sorted order (64 bits); k_bs_table, a wave per sorted record: reflen from the CIGAR words, 64 per step,
 *      and the record's line of the table; k_bs_gather, gridded over the OUTPUT as k_fq_pack is: a workgroup per BRX_BS_SPAN bytes, a
 *      thread per 16, its record by binary search in the scanned lengths (among the records of its span, which two threads find first
 *      for the workgroup), 16 bytes of one record as five dwords and a funnel shift.
 *      Every output byte has one writer.
 *
 * brx_bam_index, over the table of the sorted records and the compressed offsets of the BGZF blocks of their stream:
 *   1. k_bi_check: the table is sorted, its offsets ascend inside the stream, contigs, positions and ends are in range, the block
 *      offsets ascend below 2^48.
 *   2. chunks: a run of consecutive records of one contig and one bin.  The scan of the run starts numbers them; k_bi_chunks writes
 *      (refID << 32 | bin, beg, end) of each.  The same sort over that key groups a contig's bins in ascending order, a bin's chunks
 *      in file order; the scan of the group heads and k_bi_heads give every bin its number and its first chunk.
 *   3. linear index: M = the inclusive max-scan of (uint32_t)refID << 32 | end, monotone as refID ascends (bx_max_scan, the sibling of
 *      dp_scan with max for +).  The first record j of contig r with M[j] > (r, w << 14) is the first whose end lies behind the window's
 *      start.  If its pos lies before the window's end it is the window's record.  If not, no record overlaps the window, and the next
 *      window that has one is pos >> 14, whose first record is the same j: every window takes the offset of its j, and no fill is needed.
 *      A contig's last window always has a record, the one with the largest end.
 *   4. text: k_bi_contigs finds every contig's records and chunks by binary search, two scans over the contigs place the windows and the
 *      bytes, k_bi_put_contigs / k_bi_put_windows / k_bi_put_chunks write them.  Every field lies on a multiple of 4 bytes.
 * No global atomics; no workgroup waits for another.
 */
#ifndef BRX_BAMSORT_H
#define BRX_BAMSORT_H

#include "brx_scan.h"
#include "brx_depth.h"
#include "brx_fastqin.h"

#define BRX_BS_THREADS 256u
#define BRX_BS_SPAN (BRX_BS_THREADS * 16u)              /* output bytes of a workgroup of k_bs_gather */
#define BRX_BS_FIXED 36u                                /* block_size and the 32 bytes of fixed fields */
#define BRX_BS_REF_OPS 0x18Du                           /* the operations that take reference bases: M D N = X (0 2 3 7 8) */
#define BRX_BI_MAX_END (1u << 29)

static_assert(sizeof(brx_bam_rec) == 24, "brx_bam_rec is 24 bytes");

__device__ __forceinline__ uint32_t bs_le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t bs_le32(const uint8_t *p) { return bs_le16(p) | (bs_le16(p + 2) << 16); }

/* ---- brx_bam_sort: the chain walk ---------------------------------------------------------------------------------------------------- */
struct BsIn { const uint8_t *rec; uint64_t n_bytes; const uint64_t *seg_off; uint64_t n_seg; uint32_t n_ref, max_pos; };

/* WRITE = false: cnt[s] = the records of segment s, *err where the offsets or a record are refused (nothing of a record is loaded that the
   segment does not hold).  WRITE = true, after *err stayed 0 (incl: the scan of cnt): source offset, key and length of every record. */
template <bool WRITE>
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bs_walk(BsIn in, uint32_t *cnt, const uint64_t *incl, uint64_t *src, uint64_t *key, uint32_t *len, uint32_t *err) {
    const uint64_t s = (uint64_t)blockIdx.x * BRX_BS_THREADS + threadIdx.x;
    if (s >= in.n_seg) return;
    const uint64_t a = in.seg_off[s], b = in.seg_off[s + 1u];
    if (!WRITE && (b < a || b > in.n_bytes || (s == 0 && a != 0) || (s + 1u == in.n_seg && b != in.n_bytes))) { *err = 1u; cnt[s] = 0u; return; }
    uint64_t at = a, i = WRITE ? incl[s] - cnt[s] : 0u;
    uint32_t n = 0;
    bool bad = false;
    while (at < b) {
        if (b - at < BRX_BS_FIXED) { bad = true; break; }
        const uint8_t *p = in.rec + at;
        const uint64_t size = bs_le32(p);
        const uint32_t l_name = p[12], n_cigar = bs_le16(p + 16);
        if (size < 32u + l_name + 4u * n_cigar || size > b - at - 4u) { bad = true; break; }
        const int32_t ref_id = (int32_t)bs_le32(p + 4), pos = (int32_t)bs_le32(p + 8);
        if (ref_id < -1 || (ref_id >= 0 && (uint32_t)ref_id >= in.n_ref)) { bad = true; break; }
        if (ref_id < 0 ? pos != -1 : (pos < 0 || (uint32_t)pos >= in.max_pos)) { bad = true; break; }
        if (WRITE) {
            src[i] = at;
            key[i] = ref_id < 0 ? (uint64_t)in.n_ref << 32 : ((uint64_t)(uint32_t)ref_id << 32) | (uint32_t)pos;
            len[i] = (uint32_t)size + 4u;
            ++i;
        }
        if (++n == 0u) { bad = true; break; }
        at += size + 4u;
    }
    if (!WRITE) {
        if (bad) *err = 1u;
        cnt[s] = bad ? 0u : n;
    }
}

/* ---- the sort with a payload ---------------------------------------------------------------------------------------------------------- */
/* k_dp_scatter of brx_depth.h, its ranks and places unchanged, with a 32-bit payload that travels beside every key.  pin NULL (the first
   pass): the payload is the key's number. */
__global__ void __launch_bounds__(BRX_DP_THREADS) k_bs_scatter(const uint64_t *keys, const uint32_t *pin, uint64_t n, uint32_t shift, uint32_t n_tiles, const uint32_t *table,
                                                              const uint64_t *incl, uint64_t *out, uint32_t *pout) {
    __shared__ uint32_t wcnt[BRX_DP_THREADS / 64u][256];
    __shared__ uint64_t base[256];
    const uint32_t t = threadIdx.x, w = t >> 6;
    const uint64_t below = (1ull << lane_id()) - 1ull;
    { const uint64_t e = (uint64_t)t * n_tiles + blockIdx.x; base[t] = incl[e] - table[e]; }
    for (uint32_t x = 0; x < BRX_DP_ITEMS; ++x) {
#pragma unroll
        for (uint32_t ww = 0; ww < BRX_DP_THREADS / 64u; ++ww) wcnt[ww][t] = 0;
        __syncthreads();
        const uint64_t i = (uint64_t)blockIdx.x * BRX_DEPTH_TILE + x * BRX_DP_THREADS + t;
        const bool valid = i < n;
        const uint64_t k = valid ? keys[i] : 0ull;
        const uint32_t pl = !valid ? 0u : pin ? pin[i] : (uint32_t)i;
        const uint32_t dg = (uint32_t)(k >> shift) & 255u;
        uint64_t same = __ballot(valid);
#pragma unroll
        for (uint32_t bit = 0; bit < 8; ++bit) {
            const bool on = ((dg >> bit) & 1u) != 0;
            const uint64_t m = __ballot(on);
            same &= on ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & below);
        if (valid && rank == 0) wcnt[w][dg] = (uint32_t)__popcll(same);
        __syncthreads();
        uint32_t acc = 0;
#pragma unroll
        for (uint32_t ww = 0; ww < BRX_DP_THREADS / 64u; ++ww) { const uint32_t c = wcnt[ww][t]; wcnt[ww][t] = acc; acc += c; }
        __syncthreads();
        if (valid) { const uint64_t to = base[dg] + wcnt[w][dg] + rank; out[to] = k; pout[to] = pl; }
        __syncthreads();
        base[t] += acc;
    }
}

/* where the sort keeps what: the keys and payloads of both sides of a pass, the table of k_dp_hist, its scan, the tile sums */
struct BsSort { uint64_t *keys[2]; uint32_t *pay[2]; uint32_t *table; uint64_t *incl, *sums; };
/* n >= 1 keys in S.keys[0] by the digits at `shifts`, lowest first; the sorted keys and payloads are in S.keys[r], S.pay[r], r returned */
static uint32_t bs_sort(hipStream_t st, const BsSort &S, uint64_t n, const uint32_t *shifts, uint32_t n_pass) {
    const uint32_t nt = (uint32_t)((n + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE);
    const DpSrcTable tab = { S.table };
    for (uint32_t p = 0; p < n_pass; ++p) {
        const uint64_t *in = S.keys[p & 1u];
        hipLaunchKernelGGL((k_dp_hist<DpKeysBuf, false>), dim3(nt), dim3(BRX_DP_THREADS), 0, st, DpKeysBuf{ in }, n, shifts[p], nt, S.table, (uint64_t)0,
                           (const brx_contig *)nullptr, 0u, (uint32_t *)nullptr);
        dp_scan(st, tab, 256ull * nt, S.sums, S.incl);
        hipLaunchKernelGGL(k_bs_scatter, dim3(nt), dim3(BRX_DP_THREADS), 0, st, in, p ? (const uint32_t *)S.pay[p & 1u] : (const uint32_t *)nullptr, n, shifts[p], nt,
                           (const uint32_t *)S.table, (const uint64_t *)S.incl, S.keys[(p + 1u) & 1u], S.pay[(p + 1u) & 1u]);
    }
    return n_pass & 1u;
}

/* ---- brx_bam_sort: table and gather ---------------------------------------------------------------------------------------------------- */
/* the lengths in sorted order */
struct BsSrcLen { const uint32_t *len, *pay; __device__ uint64_t operator()(uint64_t j) const { return len[pay[j]]; } };

/* A wave per sorted record j (four to a workgroup): the record's line of the table, its source offset at ssrc[j]; the first record of
   refID -1, if there is one, leaves its number in *first_unmapped (preset to n). */
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bs_table(const uint8_t *rec, const uint64_t *src, const uint32_t *pay, const uint32_t *len, const uint64_t *incl_len,
                                                            const uint64_t *skey, uint64_t n, uint32_t n_ref, brx_bam_rec *out, uint64_t *ssrc, uint64_t *first_unmapped) {
    const uint64_t j = (uint64_t)blockIdx.x * (BRX_BS_THREADS / 64u) + (threadIdx.x >> 6);
    if (j >= n) return;
    const uint32_t i = pay[j], lane = (uint32_t)lane_id();
    const uint64_t at = src[i];
    const uint8_t *p = rec + at;
    const uint32_t l_name = p[12], n_cigar = bs_le16(p + 16);
    const uint8_t *cg = p + BRX_BS_FIXED + l_name;
    uint32_t sum = 0;
    for (uint32_t b = 0; b < n_cigar; b += 64u) {
        const uint32_t c = b + lane;
        if (c < n_cigar) {
            const uint32_t w = bs_le32(cg + 4ull * c);
            if ((BRX_BS_REF_OPS >> (w & 15u)) & 1u) sum += w >> 4;
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) {
        const int32_t ref_id = (int32_t)bs_le32(p + 4), pos = (int32_t)bs_le32(p + 8);
        brx_bam_rec r;
        r.off = incl_len[j] - len[i]; r.refID = ref_id; r.pos = pos;
        r.end = ref_id < 0 ? 0u : (uint32_t)pos + (sum ? sum : 1u);
        r.bin = bs_le16(p + 14);
        out[j] = r;
        ssrc[j] = at;
        if ((skey[j] >> 32) == n_ref && (j == 0 || (skey[j - 1u] >> 32) != n_ref)) *first_unmapped = j;
    }
}

/* A workgroup per BRX_BS_SPAN output bytes, a thread per 16 of them.  incl_len: the scan of the sorted lengths (incl_len[n - 1] = n_bytes),
   ssrc: where each sorted record lies in rec.  wide: rec begins on a dword. */
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bs_gather(const uint8_t *rec, uint64_t n_bytes, const uint64_t *incl_len, const uint64_t *ssrc, uint64_t n, uint8_t *out,
                                                             bool wide, bool aligned) {
    __shared__ uint64_t range[2];
    const uint64_t o0 = (uint64_t)blockIdx.x * BRX_BS_SPAN, o = o0 + (uint64_t)threadIdx.x * 16u;
    /* two threads find the records of the span's first and last byte among all records; the others then search between those two, which
       are the same or neighbours wherever records are longer than the span */
    if (threadIdx.x < 2u) {
        const uint64_t want = threadIdx.x == 0 ? o0 : (n_bytes - o0 > BRX_BS_SPAN ? o0 + BRX_BS_SPAN : n_bytes) - 1u;
        uint64_t lo = 0, hi = n - 1u;                    /* the first record that ends behind `want` */
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2u;
            if (incl_len[mid] > want) hi = mid; else lo = mid + 1u;
        }
        range[threadIdx.x] = lo;
    }
    __syncthreads();
    if (o >= n_bytes) return;
    uint64_t lo = range[0], hi = range[1];               /* the first record that ends behind o */
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (incl_len[mid] > o) hi = mid; else lo = mid + 1u;
    }
    uint64_t j = lo, end = incl_len[j];
    uint64_t sp = ssrc[j] - (j ? incl_len[j - 1u] : 0ull);       /* + output position = the byte of rec (mod 2^64) */
    const uint32_t cnt = n_bytes - o >= 16u ? 16u : (uint32_t)(n_bytes - o);
    uint32_t w[4] = { 0u, 0u, 0u, 0u };
    if (!(wide && cnt == 16u && o + 16u <= end && fq_load16(rec, n_bytes, sp + o, w))) {
#pragma unroll
        for (uint32_t x = 0; x < 16u; ++x) {
            if (x < cnt) {
                const uint64_t pos = o + x;
                if (pos >= end) {                        /* a border: no record is empty */
                    ++j;
                    sp = ssrc[j] - end;
                    end = incl_len[j];
                }
                w[x >> 2] |= (uint32_t)rec[sp + pos] << (8u * (x & 3u));
            }
        }
    }
    fq_store16(out + o, w, cnt, aligned);
}

/* ---- the tile max-scan: dp_scan with max for +, 0 the identity -------------------------------------------------------------------------- */
__device__ __forceinline__ uint64_t bx_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t wave_incl_max_u64(uint64_t v) {
    const int lane = lane_id();
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, dd, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), dd, 64);
        if (lane >= dd) v = bx_max(v, ((uint64_t)hi << 32) | lo);
    }
    return v;
}
/* the max of v over the threads BEFORE this one in the workgroup (max has no inverse, so the exclusive form is what the kernels carry);
   *total = the workgroup's max.  lds: a word per wave.  Every thread calls it. */
__device__ __forceinline__ uint64_t bx_block_excl(uint64_t v, uint64_t *lds, uint64_t *total) {
    const uint32_t w = threadIdx.x >> 6;
    const uint64_t inc = wave_incl_max_u64(v);
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)inc, 1, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), 1, 64);
    const uint64_t lanes_before = lane_id() ? (((uint64_t)hi << 32) | lo) : 0ull;
    __syncthreads();                                   /* the words of the call before have been read */
    if (lane_id() == 63) lds[w] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t x = 0; x < BRX_DP_THREADS / 64u; ++x) { const uint64_t s = lds[x]; if (x < w) base = bx_max(base, s); tot = bx_max(tot, s); }
    *total = tot;
    return bx_max(base, lanes_before);
}
template <class Src>
__global__ void __launch_bounds__(BRX_DP_THREADS) k_bx_reduce(Src src, uint64_t n, uint64_t *sums) {
    __shared__ uint64_t lds[BRX_DP_THREADS / 64u];
    const uint64_t i0 = (uint64_t)blockIdx.x * BRX_DEPTH_TILE + (uint64_t)threadIdx.x * BRX_DP_ITEMS;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t x = 0; x < BRX_DP_ITEMS; ++x) if (i0 + x < n) v = bx_max(v, src(i0 + x));
    uint64_t tot;
    bx_block_excl(v, lds, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}
/* the tile maxima to the maximum before each tile, in place; sums[n_tiles] = the maximum of all.  One workgroup. */
__global__ void __launch_bounds__(BRX_DP_THREADS) k_bx_scan_sums(uint64_t *sums, uint32_t n_tiles) {
    __shared__ uint64_t lds[BRX_DP_THREADS / 64u];
    uint64_t run = 0;
    for (uint32_t b = 0; b < n_tiles; b += BRX_DP_THREADS) {
        const uint32_t i = b + threadIdx.x;
        const uint64_t v = i < n_tiles ? sums[i] : 0u;
        uint64_t tot;
        const uint64_t before = bx_block_excl(v, lds, &tot);
        if (i < n_tiles) sums[i] = bx_max(run, before);
        run = bx_max(run, tot);
    }
    if (threadIdx.x == 0) sums[n_tiles] = run;
}
template <class Src>
__global__ void __launch_bounds__(BRX_DP_THREADS) k_bx_apply(Src src, uint64_t n, const uint64_t *sums, uint64_t *out) {
    __shared__ uint64_t lds[BRX_DP_THREADS / 64u];
    const uint64_t i0 = (uint64_t)blockIdx.x * BRX_DEPTH_TILE + (uint64_t)threadIdx.x * BRX_DP_ITEMS;
    uint64_t val[BRX_DP_ITEMS], v = 0;
#pragma unroll
    for (uint32_t x = 0; x < BRX_DP_ITEMS; ++x) { val[x] = i0 + x < n ? src(i0 + x) : 0u; v = bx_max(v, val[x]); }
    uint64_t tot;
    uint64_t run = bx_max(sums[blockIdx.x], bx_block_excl(v, lds, &tot));
#pragma unroll
    for (uint32_t x = 0; x < BRX_DP_ITEMS; ++x) { run = bx_max(run, val[x]); if (i0 + x < n) out[i0 + x] = run; }
}
/* out[i] = the maximum of src over [0, i]; sums as for dp_scan */
template <class Src> static void bx_max_scan(hipStream_t st, Src src, uint64_t n, uint64_t *sums, uint64_t *out) {
    const uint32_t nt = (uint32_t)((n + BRX_DEPTH_TILE - 1) / BRX_DEPTH_TILE);
    hipLaunchKernelGGL((k_bx_reduce<Src>), dim3(nt), dim3(BRX_DP_THREADS), 0, st, src, n, sums);
    hipLaunchKernelGGL(k_bx_scan_sums, dim3(1), dim3(BRX_DP_THREADS), 0, st, sums, nt);
    hipLaunchKernelGGL((k_bx_apply<Src>), dim3(nt), dim3(BRX_DP_THREADS), 0, st, src, n, (const uint64_t *)sums, out);
}

/* ---- brx_bam_index ------------------------------------------------------------------------------------------------------------------------ */
/* the virtual offset of byte u of the record stream */
struct BiVoff {
    const uint64_t *boff; uint64_t base;
    __device__ uint64_t operator()(uint64_t u) const { return ((base + boff[u >> 15]) << 16) | (u & (uint64_t)(BRX_BGZF_BLOCK - 1u)); }
};
__device__ __forceinline__ uint64_t bi_key(const brx_bam_rec &r) { return ((uint64_t)(uint32_t)r.refID << 32) | (uint32_t)r.pos; }

/* thread t: record t of the table and block offset t.  *err where the call is to be refused. */
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bi_check(const brx_bam_rec *recs, uint64_t n, uint32_t n_ref, uint64_t n_bytes, const uint64_t *boff, uint64_t n_off,
                                                            uint64_t base, uint32_t *err) {
    const uint64_t t = (uint64_t)blockIdx.x * BRX_BS_THREADS + threadIdx.x;
    bool bad = false;
    if (t < n) {
        const brx_bam_rec r = recs[t];
        if (r.refID < -1 || (r.refID >= 0 && (uint32_t)r.refID >= n_ref)) bad = true;
        if (r.refID >= 0 && (r.pos < 0 || r.end <= (uint32_t)r.pos || r.end > BRX_BI_MAX_END)) bad = true;
        if (r.off >= n_bytes) bad = true;
        if (t) {
            const brx_bam_rec q = recs[t - 1u];
            if (q.off >= r.off || bi_key(q) > bi_key(r)) bad = true;
        }
    }
    if (t < n_off) {
        const uint64_t b = boff[t];
        if (b >= (1ull << 48) || base + b >= (1ull << 48) || (t && boff[t - 1u] > b)) bad = true;
    }
    if (bad) *err = 1u;
}

/* 1 where a mapped record begins a run of one contig and one bin */
struct BiSrcStart {
    const brx_bam_rec *r;
    __device__ uint64_t operator()(uint64_t j) const {
        const brx_bam_rec a = r[j];
        if (a.refID < 0) return 0u;
        if (j == 0) return 1u;
        const brx_bam_rec b = r[j - 1u];
        return (b.refID != a.refID || b.bin != a.bin) ? 1u : 0u;
    }
};
/* incl: the scan of BiSrcStart.  The run's first record writes the chunk's key and beg, its last record the end. */
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bi_chunks(BiSrcStart start, const uint64_t *incl, uint64_t n, uint64_t n_bytes, BiVoff voff, uint64_t *ckey, uint64_t *cbeg, uint64_t *cend) {
    const uint64_t j = (uint64_t)blockIdx.x * BRX_BS_THREADS + threadIdx.x;
    if (j >= n) return;
    const brx_bam_rec a = start.r[j];
    if (a.refID < 0) return;
    const uint64_t c = incl[j] - 1u;
    if (start(j)) { ckey[c] = ((uint64_t)(uint32_t)a.refID << 32) | (a.bin & 0xFFFFu); cbeg[c] = voff(a.off); }
    if (j + 1u == n) { cend[c] = voff(n_bytes); return; }
    const brx_bam_rec b = start.r[j + 1u];
    if (b.refID != a.refID || b.bin != a.bin) cend[c] = voff(b.off);
}
/* the sorted chunk keys: 1 where a bin begins */
struct BiSrcHead { const uint64_t *k; __device__ uint64_t operator()(uint64_t s) const { return (s == 0 || k[s] != k[s - 1u]) ? 1u : 0u; } };
/* hincl: the scan of BiSrcHead.  head[b] = the first chunk of bin number b, head[the number of bins] = m */
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bi_heads(BiSrcHead h, const uint64_t *hincl, uint64_t m, uint64_t *head) {
    const uint64_t s = (uint64_t)blockIdx.x * BRX_BS_THREADS + threadIdx.x;
    if (s >= m) return;
    if (h(s)) head[hincl[s] - 1u] = s;
    if (s + 1u == m) head[hincl[s]] = m;
}
/* thread r <= n_ref: cf[r] = the first sorted chunk of a contig >= r, rf[r] = the first record of one (as unsigned: refID -1 lies behind all) */
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bi_contigs(const brx_bam_rec *recs, uint64_t n, const uint64_t *skey, uint64_t m, uint32_t n_ref, uint64_t *cf, uint64_t *rf) {
    const uint64_t r = (uint64_t)blockIdx.x * BRX_BS_THREADS + threadIdx.x;
    if (r > n_ref) return;
    uint64_t lo = 0, hi = m;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2u; if ((skey[mid] >> 32) >= r) hi = mid; else lo = mid + 1u; }
    cf[r] = lo;
    lo = 0; hi = n;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2u; if ((uint64_t)(uint32_t)recs[mid].refID >= r) hi = mid; else lo = mid + 1u; }
    rf[r] = lo;
}
struct BiSrcEnd { const brx_bam_rec *r; __device__ uint64_t operator()(uint64_t j) const { const brx_bam_rec a = r[j]; return ((uint64_t)(uint32_t)a.refID << 32) | a.end; } };
/* the windows of contig r: behind the largest end of its records */
struct BiSrcIntv {
    const uint64_t *rf, *M;
    __device__ uint64_t operator()(uint64_t r) const { return rf[r + 1u] > rf[r] ? ((((uint32_t)M[rf[r + 1u] - 1u]) - 1u) >> 14) + 1u : 0u; }
};
/* what the index holds of contig r.  hincl / cf: the bins and chunks; winc: the scan of BiSrcIntv */
struct BiLayout {
    const uint64_t *cf, *hincl, *winc;
    __device__ uint64_t heads_before(uint64_t s) const { return s ? hincl[s - 1u] : 0u; }
    __device__ uint64_t chunks(uint64_t r) const { return cf[r + 1u] - cf[r]; }
    __device__ uint64_t bins(uint64_t r) const { return heads_before(cf[r + 1u]) - heads_before(cf[r]); }
    __device__ uint64_t windows(uint64_t r) const { return winc[r] - (r ? winc[r - 1u] : 0u); }
    __device__ uint64_t operator()(uint64_t r) const { return 8u + 8u * bins(r) + 16u * chunks(r) + 8u * windows(r); }
};
__device__ __forceinline__ void bi_put32(uint8_t *out, uint64_t at, uint32_t v) { *(uint32_t *)(out + at) = v; }
__device__ __forceinline__ void bi_put64(uint8_t *out, uint64_t at, uint64_t v) { bi_put32(out, at, (uint32_t)v); bi_put32(out, at + 4u, (uint32_t)(v >> 32)); }

/* cbase: the scan of BiLayout, so contig r begins at 8 + cbase[r - 1].  Thread r < n_ref: n_bin and n_intv of contig r; thread n_ref:
   the magic, n_ref and, at the end, the records of refID -1. */
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bi_put_contigs(BiLayout L, const uint64_t *cbase, const uint64_t *rf, uint64_t n, uint32_t n_ref, uint64_t total, uint8_t *out) {
    const uint64_t r = (uint64_t)blockIdx.x * BRX_BS_THREADS + threadIdx.x;
    if (r > n_ref) return;
    if (r == n_ref) {
        bi_put32(out, 0, 0x01494142u);                  /* BAI\1 */
        bi_put32(out, 4, n_ref);
        bi_put64(out, total - 8u, n - rf[n_ref]);
        return;
    }
    const uint64_t at = 8u + (r ? cbase[r - 1u] : 0u);
    bi_put32(out, at, (uint32_t)L.bins(r));
    bi_put32(out, at + 4u + 8u * L.bins(r) + 16u * L.chunks(r), (uint32_t)L.windows(r));
}
/* a thread per window of the whole index (n_win = winc[n_ref - 1]) */
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bi_put_windows(BiLayout L, const uint64_t *cbase, const uint64_t *rf, const uint64_t *M, const brx_bam_rec *recs, uint32_t n_ref,
                                                                  uint64_t n_win, BiVoff voff, uint8_t *out) {
    const uint64_t g = (uint64_t)blockIdx.x * BRX_BS_THREADS + threadIdx.x;
    if (g >= n_win) return;
    uint64_t lo = 0, hi = n_ref - 1u;                   /* the first contig whose windows end behind g */
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2u; if (L.winc[mid] > g) hi = mid; else lo = mid + 1u; }
    const uint64_t r = lo, w = g - (r ? L.winc[r - 1u] : 0u);
    const uint64_t want = (r << 32) | (w << 14);
    lo = rf[r]; hi = rf[r + 1u] - 1u;                   /* the contig's last record ends behind every window's start */
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2u; if (M[mid] > want) hi = mid; else lo = mid + 1u; }
    const uint64_t at = 8u + (r ? cbase[r - 1u] : 0u) + 4u + 8u * L.bins(r) + 16u * L.chunks(r) + 4u + 8u * w;
    bi_put64(out, at, voff(recs[lo].off));
}
/* a thread per sorted chunk: its beg and end, and with the first of a bin the bin's number and chunk count */
__global__ void __launch_bounds__(BRX_BS_THREADS) k_bi_put_chunks(BiLayout L, const uint64_t *cbase, const uint64_t *skey, const uint32_t *spay, uint64_t m, const uint64_t *head,
                                                                 const uint64_t *cbeg, const uint64_t *cend, uint8_t *out) {
    const uint64_t s = (uint64_t)blockIdx.x * BRX_BS_THREADS + threadIdx.x;
    if (s >= m) return;
    const uint64_t k = skey[s], r = k >> 32, first = L.cf[r];
    const uint64_t at = 8u + (r ? cbase[r - 1u] : 0u) + 4u + 8u * (L.hincl[s] - L.heads_before(first)) + 16u * (s - first);
    const uint32_t c = spay[s];
    bi_put64(out, at, cbeg[c]);
    bi_put64(out, at + 8u, cend[c]);
    if (s == 0 || skey[s - 1u] != k) {
        bi_put32(out, at - 8u, (uint32_t)k);
        bi_put32(out, at - 4u, (uint32_t)(head[L.hincl[s]] - s));
    }
}

#endif /* BRX_BAMSORT_H */
