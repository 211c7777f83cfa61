/*
 * brx_fastqin.h -- the FASTQ that `error_model`, `qscore_model` and `plot` read, parsed on the device, and the read slices of a job packed
 * there (--gpu-reads; README: The device read loader).  The scan is that of brx_scan.h.
 *   load_fastq    /root/reference/badread/misc.py:97-119   (a stripped line that begins with '@' opens a record of four lines)
 *   Job.__init__  badread_amd/model_builder.py            (seq: the read slices upper-cased, qual: their qualities, back to back)
 * brx_fastq_scan: text -> one brx_fastq_rec per four lines, for the layout in which the reference's state machine finds its headers on the
 * lines 0, 4, 8, ...: the line count a multiple of 4, every line 4k a header with a name, no byte of 0x80 or more.  Anything else is
 * named in *layout and the host loads the file.
 *   1. the scan of brx_scan.h over FqSrcStarts16: an element is a group of 16 text bytes, its value the line starts among them (byte 0
 *      and every byte behind a '\n').  8 bytes of prefix per 16 bytes of text.  k_fq_starts, a thread per group, writes the offset of
 *      each of its line starts to line_start[] and n_bytes behind the last; a byte of 0x80 or more raises BRX_FQ_HIGH.
 *   2. k_fq_records, a thread per record: the four line starts and the next one, the header, sequence and quality lines stripped of the
 *      six ASCII blanks at both ends, the name behind the '@'.  It reads the lines' ends and the header, not the bases.
 * brx_reads_pack: k_fq_check, a thread per alignment, refuses what leaves the text or does not ascend before a byte is moved; k_fq_pack,
 * gridded over the OUTPUT: a thread owns 16 consecutive bytes of seq and of qual, finds its alignment by binary search in the offsets,
 * steps over the borders inside its 16 bytes, and stores each array with one 16-byte store.  16 bytes of one alignment come from five
 * aligned dwords and a funnel shift, whatever the source's alignment; bytes are loaded one by one only around a border and at the ends.
 * No global atomics; no workgroup waits for another.
 */
#ifndef BRX_FASTQIN_H
#define BRX_FASTQIN_H

#include "brx_scan.h"

#define BRX_FQ_THREADS 256u
#define BRX_FQ_TILE (BRX_FQ_THREADS * 16u)              /* output bytes of a workgroup of k_fq_pack */

static_assert(sizeof(brx_fastq_rec) == 48, "brx_fastq_rec is 48 bytes");

__device__ __forceinline__ bool fq_is_blank(uint32_t c) { return c == 32u || c - 9u < 5u; }      /* space \t \n \x0b \x0c \r */

/* for each of the four bytes of w: bit 7 of the byte where it equals c, no other bit */
__device__ __forceinline__ uint32_t fq_eq_bytes(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
/* bits 7, 15, 23, 31 of m as bits 0..3 */
__device__ __forceinline__ uint32_t fq_byte_bits(uint32_t m) { return (((m >> 7) & 0x01010101u) * 0x01020408u) >> 24; }

/* Group g of the text: bit i of the result is set where byte 16 g + i begins a line.  *high: a byte of the group is 0x80 or more.
   One 16-byte load where the group lies inside the text and the text is aligned, bytes otherwise. */
__device__ __forceinline__ uint32_t fq_starts16(const uint8_t *t, uint64_t n, uint64_t g, bool *high) {
    const uint64_t p0 = g * 16u;
    uint32_t w[4] = { 0u, 0u, 0u, 0u };
    if (p0 + 16u <= n && ((uintptr_t)t & 15u) == 0) {
        const uint4 v = *(const uint4 *)(t + p0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        for (uint32_t i = 0; i < 16u && p0 + i < n; ++i) w[i >> 2] |= (uint32_t)t[p0 + i] << (8u * (i & 3u));
    }
    uint32_t nl = 0;
#pragma unroll
    for (uint32_t x = 0; x < 4u; ++x) nl |= fq_byte_bits(fq_eq_bytes(w[x], (uint32_t)'\n')) << (4u * x);
    *high = ((w[0] | w[1] | w[2] | w[3]) & 0x80808080u) != 0u;
    const uint32_t first = (g == 0 || t[p0 - 1u] == (uint8_t)'\n') ? 1u : 0u;
    const uint32_t inside = n - p0 >= 16u ? 0xFFFFu : (1u << (uint32_t)(n - p0)) - 1u;       /* a '\n' as the last byte starts no line */
    return ((nl << 1) | first) & inside;
}

/* the number of line starts in a group of 16 bytes; n: the bytes of the text, the groups are (n + 15) / 16 */
struct FqSrcStarts16 {
    const uint8_t *t; uint64_t n;
    __device__ uint64_t operator()(uint64_t g) const { bool high; return (uint64_t)__popc(fq_starts16(t, n, g, &high)); }
};

/* incl = the scan of FqSrcStarts16.  line_start[L] = the first byte of line L, line_start[the number of lines] = n_bytes.  flags[0]: a
   byte of 0x80 or more. */
__global__ void __launch_bounds__(BRX_FQ_THREADS) k_fq_starts(FqSrcStarts16 src, uint64_t n_groups, const uint64_t *incl, uint64_t *line_start, uint32_t *flags) {
    const uint64_t g = (uint64_t)blockIdx.x * BRX_FQ_THREADS + threadIdx.x;
    if (g >= n_groups) return;
    bool high;
    uint32_t m = fq_starts16(src.t, src.n, g, &high);
    if (high) flags[0] = 1u;
    const uint64_t after = incl[g];
    uint64_t L = after - (uint64_t)__popc(m);
    while (m) {
        const uint32_t i = (uint32_t)__ffs((int)m) - 1u;
        line_start[L++] = g * 16u + i;
        m &= m - 1u;
    }
    if (g + 1u == n_groups) line_start[after] = src.n;
}

/* [*lo, *hi) without the blanks at both ends; an empty result has *lo == *hi == where the line ended */
__device__ __forceinline__ void fq_strip(const uint8_t *t, uint64_t *lo, uint64_t *hi) {
    uint64_t a = *lo, b = *hi;
    while (a < b && fq_is_blank(t[a])) ++a;
    while (b > a && fq_is_blank(t[b - 1u])) --b;
    *lo = a; *hi = b;
}

/* One thread per record.  flags[1]: a line 4k that opens no record, or a bare '@'; flags[2]: a line of 2^32 bytes or more. */
__global__ void __launch_bounds__(BRX_FQ_THREADS) k_fq_records(const uint8_t *t, const uint64_t *line_start, uint64_t n_recs, brx_fastq_rec *recs, uint32_t *flags) {
    const uint64_t k = (uint64_t)blockIdx.x * BRX_FQ_THREADS + threadIdx.x;
    if (k >= n_recs) return;
    uint64_t s[5];
#pragma unroll
    for (uint32_t x = 0; x < 5u; ++x) s[x] = line_start[4u * k + x];
    bool too_long = false;
#pragma unroll
    for (uint32_t x = 0; x < 4u; ++x) if (s[x + 1u] - s[x] >= (1ull << 32)) too_long = true;
    if (too_long) { flags[2] = 1u; return; }
    uint64_t h0 = s[0], h1 = s[1], q0 = s[1], q1 = s[2], u0 = s[3], u1 = s[4];
    fq_strip(t, &h0, &h1); fq_strip(t, &q0, &q1); fq_strip(t, &u0, &u1);
    uint64_t name = h0 + 1u, name_end;
    bool ok = h0 < h1 && t[h0] == (uint8_t)'@';
    if (ok) {
        while (name < h1 && fq_is_blank(t[name])) ++name;
        ok = name < h1;
    }
    if (!ok) { flags[1] = 1u; name = h1; }
    name_end = name;
    while (name_end < h1 && !fq_is_blank(t[name_end])) ++name_end;
    brx_fastq_rec r;
    r.head_off = s[0]; r.name_off = (uint32_t)(name - s[0]); r.name_len = (uint32_t)(name_end - name);
    r.seq_off = q0; r.qual_off = u0; r.seq_len = (uint32_t)(q1 - q0); r.qual_len = (uint32_t)(u1 - u0);
    r.flags = ok ? 0u : BRX_FQ_HEADER; r.reserved = 0u;
    recs[k] = r;
}

/* ---- brx_reads_pack ------------------------------------------------------------------------------------------------------------------- */
/* One thread per alignment: offsets that ascend from 0, source ranges inside the text.  *err otherwise; k_fq_pack runs only after it
   stayed 0, so it reads and writes inside the arrays without a test of its own. */
__global__ void __launch_bounds__(BRX_FQ_THREADS) k_fq_check(brx_reads_job j, uint32_t *err) {
    const uint32_t a = blockIdx.x * BRX_FQ_THREADS + threadIdx.x;
    if (a >= j.n_align) return;
    const uint64_t o0 = j.d_align_read_off[a], o1 = j.d_align_read_off[a + 1u];
    if (o1 < o0 || (a == 0 && o0 != 0)) { *err = 1u; return; }
    const uint64_t len = o1 - o0, ss = j.d_seq_src[a], qs = j.d_qual_src[a];
    if (ss > j.n_text || len > j.n_text - ss || qs > j.n_text || len > j.n_text - qs) *err = 1u;
}

__device__ __forceinline__ uint32_t fq_upper(uint32_t c) { return c - (uint32_t)'a' < 26u ? c - 32u : c; }
/* fq_upper of each of the four bytes of w */
__device__ __forceinline__ uint32_t fq_upper4(uint32_t w) {
    const uint32_t x = w & 0x7F7F7F7Fu;
    const uint32_t lower = (x + 0x1F1F1F1Fu) & ~(x + 0x05050505u) & ~w & 0x80808080u;      /* 'a' <= byte <= 'z' */
    return w ^ (lower >> 2);
}

/* w = the 16 bytes of the text from `at`, which may lie anywhere: five aligned dwords and a funnel shift.  False, and nothing loaded, where
   the fifth dword would leave the text. */
__device__ __forceinline__ bool fq_load16(const uint8_t *text, uint64_t n_text, uint64_t at, uint32_t w[4]) {
    const uint64_t al = at & ~3ull;
    if (al + 20u > n_text) return false;
    const uint32_t *p = (const uint32_t *)(text + al);
    const uint32_t sh = 8u * (uint32_t)(at & 3u);
    uint32_t d[5];
#pragma unroll
    for (uint32_t x = 0; x < 5u; ++x) d[x] = p[x];
#pragma unroll
    for (uint32_t x = 0; x < 4u; ++x) w[x] = __builtin_amdgcn_alignbit(d[x + 1u], d[x], sh);
    return true;
}

/* 16 bytes to p: one store where all 16 lie inside the array and p is aligned */
__device__ __forceinline__ void fq_store16(uint8_t *p, const uint32_t w[4], uint32_t n, bool aligned) {
    if (n == 16u && aligned) { *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]); return; }
    for (uint32_t i = 0; i < n; ++i) p[i] = (uint8_t)(w[i >> 2] >> (8u * (i & 3u)));
}

/* A workgroup per BRX_FQ_TILE output bytes, a thread per 16 of them.  total = d_align_read_off[n_align].  wide: the text begins on a
   dword, so that 16 bytes of one alignment are loaded as dwords (profiles/gpu_reads.md: byte loads ran at a sixth of the copy rate);
   bytes where a border lies inside the 16, at the end of the arrays and at the end of the text. */
__global__ void __launch_bounds__(BRX_FQ_THREADS) k_fq_pack(brx_reads_job j, uint64_t total, bool wide) {
    const uint64_t o = (uint64_t)blockIdx.x * BRX_FQ_TILE + (uint64_t)threadIdx.x * 16u;
    if (o >= total) return;
    const uint64_t *off = j.d_align_read_off;
    uint32_t lo = 0, hi = j.n_align;                     /* the last alignment that begins at or before o: off[lo] <= o < off[hi] */
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= o) lo = mid; else hi = mid;
    }
    uint32_t a = lo;
    uint64_t end = off[a + 1u];
    uint64_t sp = j.d_seq_src[a] - off[a], qp = j.d_qual_src[a] - off[a];       /* + output position = the byte of the text (mod 2^64) */
    const uint32_t n = total - o >= 16u ? 16u : (uint32_t)(total - o);
    const bool aligned = (((uintptr_t)j.d_seq | (uintptr_t)j.d_qual) & 15u) == 0;
    uint32_t ws[4] = { 0u, 0u, 0u, 0u }, wq[4] = { 0u, 0u, 0u, 0u };
    if (wide && n == 16u && o + 16u <= end && fq_load16(j.d_text, j.n_text, sp + o, ws) && fq_load16(j.d_text, j.n_text, qp + o, wq)) {
#pragma unroll
        for (uint32_t x = 0; x < 4u; ++x) ws[x] = fq_upper4(ws[x]);
    } else {
        ws[0] = ws[1] = ws[2] = ws[3] = 0u;              /* a first load may have gone through before the second refused */
#pragma unroll
        for (uint32_t i = 0; i < 16u; ++i) {
            if (i < n) {
                const uint64_t pos = o + i;
                while (pos >= end) {                     /* a border, or several with alignments of no bases between them */
                    ++a;
                    end = off[a + 1u];
                    sp = j.d_seq_src[a] - off[a]; qp = j.d_qual_src[a] - off[a];
                }
                ws[i >> 2] |= fq_upper(j.d_text[sp + pos]) << (8u * (i & 3u));
                wq[i >> 2] |= (uint32_t)j.d_text[qp + pos] << (8u * (i & 3u));
            }
        }
    }
    fq_store16(j.d_seq + o, ws, n, aligned);
    fq_store16(j.d_qual + o, wq, n, aligned);
}

#endif /* BRX_FASTQIN_H */
