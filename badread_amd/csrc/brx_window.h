/*
 * brx_window.h -- the `plot` command's numbers (README: Window identities): the errors of every read base of a set of read-to-reference
 * alignments and, of every alignment, the sums of its windows of W read bases.  The prefix sums are the tile
 * scan of brx_scan.h.
 *   align_sequences    /root/reference/badread/alignment.py:103-132       (errors_per_read_pos)
 *   get_window_means   /root/reference/badread/plot_window_identity.py:54-70
 * The reference walks every alignment in Python, one base and then one window at a time.  Here the host ships what brx_model_count
 * takes (the read, quality and reference slices, the CIGAR parts with the prefix sums of their read / reference offsets) and, over the
 * N read bases of the whole job:
 *   1. k_pw_errors: a thread per read base p writes E[p].  It finds its alignment (align_read_off) and, by k_mb_expand's search over
 *      part_read, the last part that begins at or before p.  A D part takes no read base, so it shares its offset with the part behind
 *      it and the search passes over it; the thread of the FIRST base of a part walks back over the D parts in front of it and adds
 *      their lengths.  A base behind the CIGAR's last read base gets 0, or a trailing deletion's length if it is the first such base.
 *   2. the scan of brx_scan.h (k_dp_reduce, k_dp_scan_sums, k_dp_apply) over E, and over q = quality byte - 33 when asked, written
 *      behind a leading 0: P[p + 1] = E[0] + .. + E[p].  No segments: a window sum is P[g + i + W] - P[g + i] inside one alignment
 *      (g: its first base), and 32 bits of it are exact as no alignment has 2^31 columns (negative q: two's complement, as exact).
 *   3. k_pw_stats: a workgroup per alignment strides over its n = max(L - W, 0) windows: min, max, the first window of the max and
 *      the total, in registers, then across the wave (__shfl_xor), then across the waves through LDS.
 *   4. k_pw_values, when the caller wants the sums themselves: a thread per window.
 * Order between workgroups comes from kernel boundaries alone; no workgroup waits for another and global memory takes no atomics, so
 * the results do not depend on scheduling.  Memory-bound: 1. reads a base of read and reference and writes 4 bytes, 2. reads them
 * twice and writes 8, 3. reads 16 per window (the two ends, W apart, each from a stream of its own).
 */
#ifndef BRX_WINDOW_H
#define BRX_WINDOW_H

#include "brx_scan.h"

#define BRX_PW_THREADS 256u

static_assert(sizeof(brx_window_stat) == 40, "brx_window_stat is 40 bytes");

/* the last a with off[a] <= x (off[0] <= x); alignments without a base or a window share their offset with the next and are passed over */
__device__ __forceinline__ uint32_t pw_find(const uint64_t *off, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if (off[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

/* E[p] of every read base; the thread of base 0 also writes the leading 0 of the prefix arrays (pq: NULL without qualities) */
__global__ void __launch_bounds__(BRX_PW_THREADS) k_pw_errors(brx_window_job j, uint32_t *err, uint64_t *pe, uint64_t *pq) {
    const uint64_t p = (uint64_t)blockIdx.x * BRX_PW_THREADS + threadIdx.x;
    if (p >= j.n_bases) return;
    if (p == 0) { pe[0] = 0; if (pq) pq[0] = 0; }
    const uint32_t a = pw_find(j.d_align_read_off, j.n_align, p);
    const uint64_t first = j.d_align_part_off[a], end = j.d_align_part_off[a + 1];
    uint32_t e = 0;
    if (first < end) {
        uint64_t lo = first, hi = end;
        while (lo + 1 < hi) { const uint64_t mid = (lo + hi) >> 1; if (j.d_part_read[mid] <= p) lo = mid; else hi = mid; }
        const uint64_t o = p - j.d_part_read[lo];
        const uint32_t t = j.d_part_type[lo], len = j.d_part_len[lo];
        uint64_t k = lo + 1;                                   /* the walk back begins at the part itself when it holds no base p */
        if (t != 2u && o < len) {
            e = t == 1u ? 1u : (j.d_seq[p] != j.d_ref[j.d_part_ref[lo] + o] ? 1u : 0u);
            k = lo;
        }
        if (o == 0)                                            /* deletions (and empty parts) directly in front: they end at base p */
            while (k > first) {
                k -= 1;
                const uint32_t tk = j.d_part_type[k], lk = j.d_part_len[k];
                if (tk == 2u) e += lk; else if (lk != 0u) break;
            }
    }
    err[p] = e;
}

/* what the second scan runs over: q of every read base, sign-extended (sums modulo 2^64 are the signed sums) */
struct PwSrcQual { const uint8_t *q; __device__ uint64_t operator()(uint64_t i) const { return (uint64_t)(int64_t)((int32_t)q[i] - 33); } };

/* the better of two (sum, window) pairs for "the first window of the largest sum": larger sum, then smaller window */
__device__ __forceinline__ void pw_best(uint32_t &s, uint32_t &i, uint32_t s2, uint32_t i2) {
    if (s2 > s || (s2 == s && i2 < i)) { s = s2; i = i2; }
}
__device__ __forceinline__ uint64_t pw_shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

/* the partial result of a thread, a wave or the workgroup; a thread without a window holds the neutral element of every field */
struct PwAcc {
    uint32_t emin, emax, earg; int32_t qmin, qmax; uint64_t etot, qtot;
    __device__ void merge(const PwAcc &o) {
        emin = o.emin < emin ? o.emin : emin;
        pw_best(emax, earg, o.emax, o.earg);
        qmin = o.qmin < qmin ? o.qmin : qmin;
        qmax = o.qmax > qmax ? o.qmax : qmax;
        etot += o.etot; qtot += o.qtot;
    }
};

__global__ void __launch_bounds__(BRX_PW_THREADS) k_pw_stats(brx_window_job j, const uint64_t *pe, const uint64_t *pq) {
    __shared__ PwAcc lds[BRX_PW_THREADS / 64u];
    const uint32_t a = blockIdx.x;
    const uint64_t g = j.d_align_read_off[a], len = j.d_align_read_off[a + 1] - g;
    const uint32_t w = j.window, n = len > w ? (uint32_t)(len - w) : 0u;
    PwAcc r; r.emin = 0xFFFFFFFFu; r.emax = 0; r.earg = 0xFFFFFFFFu; r.qmin = 0x7FFFFFFF; r.qmax = -0x7FFFFFFF - 1; r.etot = 0; r.qtot = 0;
    for (uint32_t i = threadIdx.x; i < n; i += BRX_PW_THREADS) {
        PwAcc x;
        x.emin = x.emax = (uint32_t)(pe[g + i + w] - pe[g + i]); x.earg = i; x.etot = x.emin;
        x.qmin = x.qmax = pq ? (int32_t)(uint32_t)(pq[g + i + w] - pq[g + i]) : 0; x.qtot = (uint64_t)(int64_t)x.qmin;
        r.merge(x);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        PwAcc o;
        o.emin = (uint32_t)__shfl_xor((int)r.emin, m, 64); o.emax = (uint32_t)__shfl_xor((int)r.emax, m, 64);
        o.earg = (uint32_t)__shfl_xor((int)r.earg, m, 64);
        o.qmin = __shfl_xor(r.qmin, m, 64); o.qmax = __shfl_xor(r.qmax, m, 64);
        o.etot = pw_shfl_xor_u64(r.etot, m); o.qtot = pw_shfl_xor_u64(r.qtot, m);
        r.merge(o);
    }
    if (lane_id() == 0) lds[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (uint32_t x = 1; x < BRX_PW_THREADS / 64u; ++x) r.merge(lds[x]);
    brx_window_stat s;
    s.n = n; s.err_total = r.etot; s.qual_total = (int64_t)r.qtot;
    s.err_min = n ? r.emin : 0u; s.err_max = n ? r.emax : 0u; s.err_argmax = n ? r.earg : 0u;
    s.qual_min = n ? r.qmin : 0; s.qual_max = n ? r.qmax : 0;
    j.d_stat[a] = s;
}

/* the window sums themselves, alignment after alignment (d_align_win_off) */
__global__ void __launch_bounds__(BRX_PW_THREADS) k_pw_values(brx_window_job j, const uint64_t *pe, const uint64_t *pq) {
    const uint64_t x = (uint64_t)blockIdx.x * BRX_PW_THREADS + threadIdx.x;
    if (x >= j.n_windows) return;
    const uint32_t a = pw_find(j.d_align_win_off, j.n_align, x);
    const uint64_t g = j.d_align_read_off[a], len = j.d_align_read_off[a + 1] - g, i = x - j.d_align_win_off[a];
    if (len <= j.window || i >= len - j.window) return;       /* offsets that are not the prefix sums of the n: nothing is read */
    const uint64_t at = g + i;
    if (j.d_err_sum) j.d_err_sum[x] = (uint32_t)(pe[at + j.window] - pe[at]);
    if (j.d_qual_sum && pq) j.d_qual_sum[x] = (int32_t)(uint32_t)(pq[at + j.window] - pq[at]);
}

#endif /* BRX_WINDOW_H */
