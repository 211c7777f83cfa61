/*
 * brx_depth.h -- the true coverage of the reference (--truth-depth): the end points of a batch's truth records (brx_emit_depth) and, at
 * the end of the job, the bedGraph text of all of them (brx_depth_bedgraph).  A sink of the record walk of brx_paf.h.
 *
 * Per batch.  DepthSink is a fourth sink of the record walk of brx_paf.h (paf_read): of every record it keeps the contig, tstart and tend
 * and nothing else -- one sweep over the record's columns counts the target bases (= X D), which with the origin of the first column
 * gives both.  A record becomes two events (include/brx.h: BRX_DEPTH_EVENT), the start and then the end, 16 bytes.  One wave per read:
 * k_depth_size / k_truth_scan / k_depth_write, the pattern of k_paf_size / k_truth_scan / k_paf_write.
 *
 * At the end of the job (brx_depth_bedgraph), over N keys = the job's events and four of the library's own per contig: a start and an
 * end at position 0 and at the contig's length.  They add nothing to any depth and make every contig begin and end with a group of
 * keys, so that contigs without a record and uncovered contig ends need no code of their own.
 *   1. Sort (k_dp_hist, the scan, k_dp_scatter per pass): LSD radix sort, 8 bits per pass, workgroups of 256 threads over tiles of
 *      BRX_DEPTH_TILE keys.  k_dp_hist counts a tile's digits in LDS and writes table[digit][tile]; the inclusive scan of the table turns
 *      the counts into the places of every (digit, tile); k_dp_scatter ranks a tile's keys, 256 at a time in key order: a lane's rank among
 *      the equal digits of its wave from eight ballots, the waves' counts per digit through LDS and a prefix sum over them.  The first
 *      pass reads the caller's events (DpKeysIn, which also makes the library's own keys) and checks them: contig and position in range.
 *      Nothing but LDS is indexed by a digit, so a bad key cannot lead a store astray; the host reads the flag when the sort is through.
 *   2. Depth (the scan over DpSrcPack, k_dp_groups; the scan over DpSrcChange, k_dp_points).  One scan carries two sums: in the low word
 *      delta + 1 of every key (2 for a start, 0 for an end; < 2^32 as N < 2^31), in the high word the keys that end a group of equal
 *      (contig, position).  k_dp_groups compacts the group ends: (contig, position, depth after the group); depth below 0 or not 0 behind
 *      a contig's last group raises the flag.  A group is a change point when it lies at 0, at the contig's length, or the depth after it
 *      differs from the depth after the group before; k_dp_points compacts those.
 *   3. Text (the scan over DpSrcLine, k_dp_lines).  A change point below the contig's length owns the line up to the next change point
 *      -- which belongs to the same contig, as the contig's length is one -- sized with paf_digits, placed by the scan.
 * Every scan is dp_scan of brx_scan.h over one of the functors below.
 */
#ifndef BRX_DEPTH_H
#define BRX_DEPTH_H

#include "brx_scan.h"
#include "brx_paf.h"

#define BRX_DP_POS_MASK ((1ull << 39) - 1ull)

/* ---- per batch: the end points of the truth records ------------------------------------------------------------------------------ */
/* WRITE = false counts 16 bytes per record and reads nothing of it. */
template <bool WRITE> struct DepthSink {
    static constexpr bool write = WRITE, need_f0 = false, fmtd = false; uint8_t *out;
    __device__ void record(const BrxDev &d, PafRead &R, const PafRec &q) {
        if (WRITE) {
            uint32_t tspan = 0;
            for (uint32_t b = q.c0; b <= q.c1; b += 64) {
                const uint32_t c = b + (uint32_t)lane_id();
                tspan += (uint32_t)__popcll(__ballot(c <= q.c1 && R.ops[c] != 2u));
            }
            if (lane_id() == 0) {
                const uint32_t cs = (uint32_t)(q.key0 >> 32), contig = cs >> 1, p0 = (uint32_t)q.key0;
                const uint64_t ts = (cs & 1u) ? (uint64_t)d.ref.d_contigs[contig].length - (uint64_t)p0 - tspan : (uint64_t)p0;
                uint64_t *e = (uint64_t *)(out + R.at);
                e[0] = BRX_DEPTH_EVENT(contig, ts, 1);
                e[1] = BRX_DEPTH_EVENT(contig, ts + tspan, 0);
            }
        }
        R.n_rec += 1;
        R.at += 16u;
    }
};

__global__ void __launch_bounds__(64) k_depth_size(BrxDev d, const RS *rs, const PSeg *segs, const uint8_t *arena, uint32_t *len) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    PafRead R; R.at = 0; R.best = 0; R.top = 0; R.frag = nullptr;
    if (paf_has_records(s)) { DepthSink<false> k_; k_.out = nullptr; paf_read(k_, d, s, r, segs, arena, R); }
    if (lane_id() == 0) len[r] = (uint32_t)R.at;
}

__global__ void __launch_bounds__(64) k_depth_write(BrxDev d, const RS *rs, const PSeg *segs, const uint8_t *arena, const uint64_t *off, uint8_t *out) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    if (!paf_has_records(s)) return;
    PafRead R; R.at = off[r]; R.best = 0; R.top = 0; R.frag = nullptr;
    DepthSink<true> w; w.out = out;
    paf_read(w, d, s, r, segs, arena, R);
}

/* ---- what the scans run over ------------------------------------------------------------------------------------------------------ */
/* the sorted keys: low word delta + 1, high word "ends its group" */
struct DpSrcPack {
    const uint64_t *k; uint64_t n;
    __device__ uint64_t operator()(uint64_t i) const {
        const uint64_t a = k[i];
        const bool end = i + 1 == n || (k[i + 1] >> 1) != (a >> 1);
        return ((a & 1ull) << 1) | ((uint64_t)end << 32);
    }
};
/* the groups (gk: contig << 39 | position, gd: depth after): 1 for a change point.  A group not at 0 has its contig's group at 0 before it. */
struct DpSrcChange {
    const uint64_t *gk; const uint32_t *gd; const brx_contig *ct;
    __device__ uint64_t operator()(uint64_t g) const {
        const uint64_t a = gk[g], pos = a & BRX_DP_POS_MASK;
        return (pos == 0 || pos == ct[a >> 39].length || gd[g] != gd[g - 1]) ? 1u : 0u;
    }
};
/* the change points: the bytes of the line each owns, 0 for a contig's last */
struct DpSrcLine {
    const uint64_t *ck; const uint32_t *cd; const brx_contig *ct;
    __device__ uint64_t operator()(uint64_t k) const {
        const uint64_t a = ck[k], pos = a & BRX_DP_POS_MASK;
        const brx_contig c = ct[a >> 39];
        if (pos == c.length) return 0u;
        return (uint64_t)c.name_len + 4u + paf_digits((uint32_t)pos) + paf_digits((uint32_t)(ck[k + 1] & BRX_DP_POS_MASK)) + paf_digits(cd[k]);
    }
};

/* ---- the sort -------------------------------------------------------------------------------------------------------------------- */
/* the keys of the first pass: the caller's events, then four per contig: start and end at 0, start and end at the contig's length */
struct DpKeysIn {
    const uint64_t *ev; uint64_t n_ev; const brx_contig *ct;
    __device__ uint64_t operator()(uint64_t i) const {
        if (i < n_ev) return ev[i];
        const uint64_t j = i - n_ev, c = j >> 2;
        return BRX_DEPTH_EVENT(c, (j & 2u) ? (uint64_t)ct[c].length : 0ull, j & 1u);
    }
};
struct DpKeysBuf { const uint64_t *k; __device__ uint64_t operator()(uint64_t i) const { return k[i]; } };

/* table[digit][tile] = the tile's keys with that digit at `shift`.  CHECK (the first pass): an event whose contig is not one of the
   reference's, or whose position lies beyond its contig's length, sets *err. */
template <class Keys, bool CHECK>
__global__ void __launch_bounds__(BRX_DP_THREADS) k_dp_hist(Keys keys, uint64_t n, uint32_t shift, uint32_t n_tiles, uint32_t *table,
                                                           uint64_t n_ev, const brx_contig *ct, uint32_t n_contigs, uint32_t *err) {
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t x = 0; x < BRX_DP_ITEMS; ++x) {
        const uint64_t i = (uint64_t)blockIdx.x * BRX_DEPTH_TILE + x * BRX_DP_THREADS + threadIdx.x;
        if (i < n) {
            const uint64_t k = keys(i);
            if (CHECK && i < n_ev) {
                const uint64_t contig = k >> 40, pos = (k >> 1) & BRX_DP_POS_MASK;
                if (contig >= n_contigs) *err = 1u;
                else if (pos > ct[contig].length) *err = 1u;
            }
            atomicAdd(&hist[(uint32_t)(k >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    table[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = hist[threadIdx.x];
}

/* Every key of the tile to its place: incl = the inclusive scan of the table, so (digit, tile) begins at incl - table.  256 keys at a
   time, in key order: the lanes of a wave that hold the same digit (eight ballots), the lane's rank among them, the first of them
   leaves their number in wcnt[wave][digit]; thread d then turns wcnt[.][d] into what lies before each wave. */
template <class Keys>
__global__ void __launch_bounds__(BRX_DP_THREADS) k_dp_scatter(Keys keys, uint64_t n, uint32_t shift, uint32_t n_tiles, const uint32_t *table,
                                                              const uint64_t *incl, uint64_t *out) {
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
        const uint64_t k = valid ? keys(i) : 0ull;
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
        if (valid) out[base[dg] + wcnt[w][dg] + rank] = k;
        __syncthreads();
        base[t] += acc;
    }
}

/* ---- depth and text ---------------------------------------------------------------------------------------------------------------- */
/* the last key of every group of equal (contig, position): the group's key and the depth after it, at its number among the groups.  A depth
   below 0, or other than 0 behind the last group of a contig, sets *err. */
__global__ void __launch_bounds__(BRX_DP_THREADS) k_dp_groups(const uint64_t *keys, const uint64_t *pack, uint64_t n, uint64_t *gk, uint32_t *gd, uint32_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * BRX_DP_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = keys[i], nx = i + 1 < n ? keys[i + 1] : ~0ull;
    if ((nx >> 1) == (a >> 1)) return;
    const uint64_t p = pack[i], g = (p >> 32) - 1u;
    const int64_t depth = (int64_t)(p & 0xFFFFFFFFull) - (int64_t)(i + 1);
    if (depth < 0 || ((nx >> 40) != (a >> 40) && depth != 0)) *err = 1u;
    gk[g] = a >> 1;
    gd[g] = depth < 0 ? 0u : (uint32_t)depth;
}
/* the change points among the groups, at their number among the change points (incl: the scan of DpSrcChange) */
__global__ void __launch_bounds__(BRX_DP_THREADS) k_dp_points(DpSrcChange change, const uint64_t *incl, uint64_t n_groups, uint64_t *ck, uint32_t *cd) {
    const uint64_t g = (uint64_t)blockIdx.x * BRX_DP_THREADS + threadIdx.x;
    if (g >= n_groups || !change(g)) return;
    ck[incl[g] - 1u] = change.gk[g];
    cd[incl[g] - 1u] = change.gd[g];
}
/* the line of every change point that owns one (incl: the scan of DpSrcLine): contig, start, end, depth */
__global__ void __launch_bounds__(BRX_DP_THREADS) k_dp_lines(DpSrcLine line, const uint64_t *incl, uint64_t n_points, const uint8_t *names, uint8_t *out) {
    const uint64_t k = (uint64_t)blockIdx.x * BRX_DP_THREADS + threadIdx.x;
    if (k >= n_points) return;
    const uint64_t size = line(k);
    if (!size) return;
    const uint64_t a = line.ck[k];
    const brx_contig c = line.ct[a >> 39];
    ByteSink b; b.p = out + (incl[k] - size); b.n = 0;
    for (uint32_t x = 0; x < c.name_len; ++x) b.put(names[c.name_off + x]);
    b.put('\t'); put_dec(b, a & BRX_DP_POS_MASK);
    b.put('\t'); put_dec(b, line.ck[k + 1] & BRX_DP_POS_MASK);
    b.put('\t'); put_dec(b, line.cd[k]);
    b.put('\n');
}

#endif /* BRX_DEPTH_H */
