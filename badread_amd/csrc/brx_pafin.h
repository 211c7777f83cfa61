/*
 * brx_pafin.h -- the PAF that `error_model`, `qscore_model` and `plot` read, parsed and packed on the device (--gpu-loader; README: The
 * device loader).  The scan is that of brx_scan.h.
 *   Alignment.__init__   /root/reference/badread/alignment.py:24-64   (the fields, cg:Z:, AS:i:, the CIGAR's parts)
 *   Job.__init__         badread_amd/model_builder.py                 (the part arrays and the reference slices)
 * brx_paf_scan: text -> one brx_paf_line per line.
 *   1. the scan of brx_scan.h over PiSrcStart (1 for byte 0 and for every byte behind a '\n'); k_pi_starts leaves every line's first byte
 *      in its record.  Nothing is written for the lines beyond max_lines.
 *   2. k_pi_lines, a wave per line.  First the fields, 64 bytes per step: the tabs and the line's end come from ballots, and the lane that
 *      holds the delimiter BEHIND a field owns the field -- it knows where the field began (the delimiter before it, in this step or carried)
 *      and reads the field's few bytes back from memory: an integer, the strand, the five bytes of cg:Z: / AS:i:.  Then the CIGAR of the last
 *      cg:Z: field, 64 bytes per step (pi_lex): a lane that holds a letter owns a part and reads its digits back from memory, as they may lie
 *      in the step before; the sums and "the read bases in front of a D" are wave prefix sums carried across the steps.
 *      A line that is not regular (include/brx.h) gets BRX_PAF_IRREGULAR and the host parses it; nothing else of its record is promised.
 * brx_align_pack: k_pi_pack, a wave per alignment, lexes the CIGAR again with the same pi_lex and writes every M / I / D part where
 * Job.__init__ puts it (mirrored for a '-' alignment), then copies the reference slice, through the complement table and backwards for '-'.
 * Every store goes to a place computed from the alignment's own bases: no global scan, no atomics, no workgroup waits for another.
 */
#ifndef BRX_PAFIN_H
#define BRX_PAFIN_H

#include "brx_scan.h"

#define BRX_PI_THREADS 256u

static_assert(sizeof(brx_paf_line) == 144, "brx_paf_line is 144 bytes");
static_assert(sizeof(brx_pack_align) == 64, "brx_pack_align is 64 bytes");

/* 1 where a line begins */
struct PiSrcStart {
    const uint8_t *t;
    __device__ uint64_t operator()(uint64_t i) const { return (i == 0 || t[i - 1] == (uint8_t)'\n') ? 1u : 0u; }
};

/* line k begins at byte i: incl = the scan of PiSrcStart */
__global__ void __launch_bounds__(BRX_PI_THREADS) k_pi_starts(PiSrcStart start, uint64_t n_bytes, const uint64_t *incl, uint64_t n_lines, brx_paf_line *lines) {
    const uint64_t i = (uint64_t)blockIdx.x * BRX_PI_THREADS + threadIdx.x;
    if (i >= n_bytes || !start(i)) return;
    const uint64_t k = incl[i] - 1u;
    if (k < n_lines) lines[k].line_off = i;
}

__device__ __forceinline__ int pi_last_bit(uint64_t m) {          /* m != 0 */
    const uint32_t hi = (uint32_t)(m >> 32);
    return hi ? 63 - __clz((int)hi) : 31 - __clz((int)(uint32_t)m);
}
__device__ __forceinline__ uint64_t pi_shfl_u64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ bool pi_is_digit(uint32_t c) { return c - (uint32_t)'0' < 10u; }
__device__ __forceinline__ bool pi_is_alpha(uint32_t c) { return (c | 32u) - (uint32_t)'a' < 26u; }

/* The CIGAR text[0, len) of one alignment, 64 bytes per step, by every lane of the wave.  sink.part(k, type, n, pm, pi, pd) is called by
   the lane of every M / I / D part: its index among them in file order, its type (0 / 1 / 2), its length and the M, I and D bases of the
   parts in front of it.  sink.step() is called by every lane after each step, for what a sink does across the lanes.  Returns false where
   the text is not ([0-9]{1,MAXDIG}[A-Za-z])+; *n_parts, sum[3]: the number of M / I / D parts and their bases. */
template <uint32_t MAXDIG, class Sink>
__device__ __forceinline__ bool pi_lex(const uint8_t *text, uint32_t len, Sink &sink, uint32_t *n_parts, uint64_t sum[3]) {
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    bool bad = len == 0;
    uint32_t parts = 0, digits_from = 0;                  /* digits_from: the byte behind the last letter so far */
    uint64_t sm = 0, si = 0, sd = 0;
    for (uint32_t b = 0; b < len; b += 64u) {
        const uint32_t p = b + (uint32_t)lane;
        const bool in = p < len;
        const uint32_t c = in ? text[p] : 0u;
        const bool letter = in && pi_is_alpha(c);
        if (in && !letter && !pi_is_digit(c)) bad = true;
        const uint64_t letters = __ballot(letter);
        uint32_t n = 0, type = 3u;
        if (letter) {
            const uint64_t before = letters & below;
            const uint32_t from = before ? b + (uint32_t)pi_last_bit(before) + 1u : digits_from;
            const uint32_t nd = p - from;
            if (nd < 1u || nd > MAXDIG) bad = true;
            else {
                uint64_t v = 0;
                for (uint32_t x = from; x < p; ++x) { const uint32_t dg = text[x]; if (!pi_is_digit(dg)) bad = true; v = v * 10u + (dg - (uint32_t)'0'); }
                if (v >> 32) bad = true;
                n = (uint32_t)v;
            }
            type = c == 'M' ? 0u : c == 'I' ? 1u : c == 'D' ? 2u : 3u;
        }
        if (letters) digits_from = b + (uint32_t)pi_last_bit(letters) + 1u;
        const bool counted = type != 3u;
        const uint64_t cm = __ballot(counted);
        if (cm) {                                          /* wave-uniform */
            const uint64_t vm = type == 0u ? n : 0u, vi = type == 1u ? n : 0u, vd = type == 2u ? n : 0u;
            const uint64_t im = wave_incl_scan_u64(vm), ii = wave_incl_scan_u64(vi), id = wave_incl_scan_u64(vd);
            if (counted) sink.part(parts + (uint32_t)__popcll(cm & below), type, n, sm + im - vm, si + ii - vi, sd + id - vd);
            sink.step();
            parts += (uint32_t)__popcll(cm);
            sm += pi_shfl_u64(im, 63); si += pi_shfl_u64(ii, 63); sd += pi_shfl_u64(id, 63);
        }
    }
    if (digits_from != len) bad = true;                    /* digits without a letter behind them */
    *n_parts = parts; sum[0] = sm; sum[1] = si; sum[2] = sd;
    return __ballot(bad) == 0ull;
}

/* what brx_paf_scan keeps of a CIGAR beside the sums */
struct PiScanSink {
    uint32_t max_indel; uint64_t read_at_d; bool is_d; uint64_t first_d, last_d;
    __device__ void part(uint32_t, uint32_t type, uint32_t n, uint64_t pm, uint64_t pi, uint64_t) {
        if (type != 0u && n > max_indel) max_indel = n;
        if (type == 2u) { is_d = true; read_at_d = pm + pi; }
    }
    __device__ void step() {
        const uint64_t dm = __ballot(is_d);
        if (dm) {
            const uint64_t lo = pi_shfl_u64(read_at_d, __ffsll((long long)dm) - 1), hi = pi_shfl_u64(read_at_d, pi_last_bit(dm));
            if (first_d == ~0ull) first_d = lo;
            last_d = hi;
        }
        is_d = false;
    }
};

/* the decimal text[from, from + n) with n in 1..18; *bad where a byte is no digit */
__device__ __forceinline__ uint64_t pi_decimal(const uint8_t *text, uint64_t from, uint32_t n, bool *bad) {
    uint64_t v = 0;
    for (uint32_t x = 0; x < n; ++x) { const uint32_t dg = text[from + x]; if (!pi_is_digit(dg)) *bad = true; v = v * 10u + (dg - (uint32_t)'0'); }
    return v;
}
__device__ __forceinline__ bool pi_tag(const uint8_t *f, char a, char b, char t) { return f[0] == (uint8_t)a && f[1] == (uint8_t)b && f[2] == ':' && f[3] == (uint8_t)t && f[4] == ':'; }

/* One wave per line.  *err: a line of 2^32 bytes or more. */
__global__ void __launch_bounds__(64) k_pi_lines(const uint8_t *text, uint64_t n_bytes, brx_paf_line *lines, uint32_t *err) {
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    brx_paf_line *rec = lines + blockIdx.x;
    const uint64_t line_off = rec->line_off;
    const uint8_t *line = text + line_off;
    const uint64_t room = n_bytes - line_off;               /* > 0: a line begins on a byte of the text */
    bool bad = false;
    /* wave-uniform: what the fields gave so far */
    uint32_t tabs = 0, field_from = 0, line_len = 0, last_byte = 0;
    uint32_t qname_len = 0, tname_off = 0, tname_len = 0, cg_off = 0, cg_len = 0, strand = 0;
    bool has_cg = false, has_as = false;
    uint64_t ints[6] = { 0, 0, 0, 0, 0, 0 };
    int64_t as = 0;
    for (uint64_t off = 0;; off += 64u) {
        if (off >= (1ull << 32) - 64u) { if (lane == 0) *err = 1u; bad = true; break; }
        const uint64_t p = off + (uint64_t)lane;
        const bool in = p < room;
        const uint32_t c = in ? line[p] : (uint32_t)'\n';
        const uint64_t ends = __ballot(c == (uint32_t)'\n');
        const int end_lane = ends ? __ffsll((long long)ends) - 1 : 64;
        const bool content = lane < end_lane;
        const bool tab = content && c == (uint32_t)'\t';
        if (content && !tab && (c < 0x21u || c > 0x7eu)) bad = true;
        if (off == 0 && lane == 0 && (!content || tab)) bad = true;                  /* an empty line, or one that begins with a tab */
        const uint64_t tabmask = __ballot(tab);
        const uint64_t delims = tabmask | (ends ? 1ull << end_lane : 0ull);
        if (delims) {                                        /* wave-uniform: a field ends in this step */
            const bool owner = ((delims >> lane) & 1ull) != 0;
            const uint64_t before = delims & below;
            const uint32_t f = tabs + (uint32_t)__popcll(tabmask & below);
            const uint32_t from = before ? (uint32_t)off + (uint32_t)pi_last_bit(before) + 1u : field_from;
            const uint32_t flen = (uint32_t)p - from;
            /* the six integers: field 2, 3, 7, 8, 9, 10 -> 0..5 */
            const int slot = f == 2u ? 0 : f == 3u ? 1 : f == 7u ? 2 : f == 8u ? 3 : f == 9u ? 4 : f == 10u ? 5 : -1;
            uint64_t value = 0;
            bool is_cg = false, is_as = false;
            if (owner) {
                if (slot >= 0) {
                    if (flen < 1u || flen > 18u) bad = true;
                    else value = pi_decimal(line, from, flen, &bad);
                    if (slot == 5 && value == 0) bad = true;
                }
                if (f == 4u) { if (flen != 1u) bad = true; else value = line[from]; }
                if (flen >= 5u) {
                    is_cg = pi_tag(line + from, 'c', 'g', 'Z');
                    is_as = pi_tag(line + from, 'A', 'S', 'i');
                    if (is_as) {
                        const bool neg = flen > 5u && line[from + 5u] == (uint8_t)'-';
                        const uint32_t nd = flen - 5u - (neg ? 1u : 0u);
                        if (nd < 1u || nd > 18u) bad = true;
                        else { const uint64_t v = pi_decimal(line, from + 5u + (neg ? 1u : 0u), nd, &bad); value = neg ? 0ull - v : v; }
                    }
                }
            }
            /* every lane learns what the owners found; of cg:Z: and AS:i: the last owner counts */
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const uint64_t m = __ballot(owner && slot == s);
                if (m) ints[s] = pi_shfl_u64(value, pi_last_bit(m));
            }
            uint64_t m = __ballot(owner && f == 0u);
            if (m) qname_len = (uint32_t)__shfl((int)flen, pi_last_bit(m), 64);
            m = __ballot(owner && f == 4u);
            if (m) strand = (uint32_t)__shfl((int)(uint32_t)value, pi_last_bit(m), 64);
            m = __ballot(owner && f == 5u);
            if (m) { const int src = pi_last_bit(m); tname_off = (uint32_t)__shfl((int)from, src, 64); tname_len = (uint32_t)__shfl((int)flen, src, 64); }
            m = __ballot(is_cg);
            if (m) { const int src = pi_last_bit(m); cg_off = (uint32_t)__shfl((int)from, src, 64) + 5u; cg_len = (uint32_t)__shfl((int)flen, src, 64) - 5u; has_cg = true; }
            m = __ballot(is_as);
            if (m) { as = (int64_t)pi_shfl_u64(value, pi_last_bit(m)); has_as = true; }
            tabs += (uint32_t)__popcll(tabmask);
            field_from = (uint32_t)off + (uint32_t)pi_last_bit(delims) + 1u;
        }
        if (end_lane > 0) last_byte = (uint32_t)__shfl((int)c, end_lane - 1, 64);
        if (ends) { line_len = (uint32_t)off + (uint32_t)end_lane; break; }
    }
    if (line_len == 0 || last_byte == (uint32_t)'\t' || tabs < 10u || !has_cg || !has_as) bad = true;
    bad = __ballot(bad) != 0ull;
    uint32_t n_parts = 0;
    uint64_t sum[3] = { 0, 0, 0 };
    PiScanSink sink; sink.max_indel = 0; sink.read_at_d = 0; sink.is_d = false; sink.first_d = sink.last_d = ~0ull;
    if (!bad) {
        if (!pi_lex<9u>(line + cg_off, cg_len, sink, &n_parts, sum)) bad = true;
#pragma unroll
        for (int x = 1; x < 64; x <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)sink.max_indel, x, 64); sink.max_indel = o > sink.max_indel ? o : sink.max_indel; }
    }
    if (lane != 0) return;
    rec->line_len = line_len; rec->flags = bad ? BRX_PAF_IRREGULAR : 0u;
    rec->qname_len = qname_len; rec->tname_off = tname_off; rec->tname_len = tname_len;
    rec->cigar_off = cg_off; rec->cigar_len = cg_len; rec->n_parts = n_parts; rec->max_indel = sink.max_indel; rec->strand = strand;
#pragma unroll
    for (int s = 0; s < 6; ++s) rec->ints[s] = ints[s];
    rec->as = as; rec->sum_m = sum[0]; rec->sum_i = sum[1]; rec->sum_d = sum[2];
    rec->first_d = sink.first_d; rec->last_d = sink.last_d;
}

/* ---- brx_align_pack --------------------------------------------------------------------------------------------------------------------- */
/* nothing is stored outside the alignment's own [part_off[a], part_off[a] + n_parts): a part beyond them is dropped and reported */
struct PiPackSink {
    brx_pack_job j; uint64_t part0, col0, read0, ref0, cols, used_read, used_ref; uint32_t n_parts; bool reversed, over;
    __device__ void part(uint32_t k, uint32_t type, uint32_t n, uint64_t pm, uint64_t pi, uint64_t pd) {
        if (k >= n_parts) { over = true; return; }
        uint64_t at = part0 + k, col = pm + pi + pd, rd = pm + pi, rf = pm + pd;
        if (reversed) {                                     /* the part's place and offsets in the list read backwards */
            at = part0 + (n_parts - 1u - k);
            col = cols - (col + n);
            rd = used_read - (rd + (type != 2u ? n : 0u));
            rf = used_ref - (rf + (type != 1u ? n : 0u));
        }
        j.d_part_type[at] = (uint8_t)type; j.d_part_len[at] = n;
        j.d_part_col[at] = col0 + col; j.d_part_read[at] = read0 + rd; j.d_part_ref[at] = ref0 + rf;
    }
    __device__ void step() {}
};

/* One wave per alignment.  *err: a descriptor that points outside the texts or does not fit the offset arrays, a CIGAR that is not regular
   or does not hold the parts and bases the descriptor names.  Such an alignment stores nothing outside its own ranges. */
__global__ void __launch_bounds__(64) k_pi_pack(brx_pack_job j, uint32_t *err) {
    const uint32_t a = blockIdx.x;
    const int lane = lane_id();
    const brx_pack_align A = j.d_align[a];
    PiPackSink sink;
    sink.j = j; sink.part0 = j.d_align_part_off[a]; sink.col0 = j.d_align_col_off[a]; sink.read0 = j.d_align_read_off[a]; sink.ref0 = j.d_align_ref_off[a];
    sink.n_parts = A.n_parts; sink.reversed = A.reversed != 0; sink.over = false;
    sink.cols = A.sum_m + A.sum_i + A.sum_d; sink.used_read = A.sum_m + A.sum_i; sink.used_ref = A.sum_m + A.sum_d;
    if (A.cigar_off > j.n_text || A.cigar_len > j.n_text - A.cigar_off || A.ref_off > j.n_reftext || A.ref_len > j.n_reftext - A.ref_off ||
        j.d_align_part_off[a + 1] - sink.part0 != A.n_parts || j.d_align_ref_off[a + 1] - sink.ref0 != A.ref_len) {
        if (lane == 0) *err = 1u;
        return;
    }
    uint32_t n_parts = 0;
    uint64_t sum[3] = { 0, 0, 0 };
    bool ok = A.cigar_len == 0 || pi_lex<10u>(j.d_text + A.cigar_off, A.cigar_len, sink, &n_parts, sum);
    if (n_parts != A.n_parts || sum[0] != A.sum_m || sum[1] != A.sum_i || sum[2] != A.sum_d) ok = false;
    if (__ballot(sink.over) != 0ull) ok = false;
    if (!ok && lane == 0) *err = 1u;
    /* the reference slice: 256 bytes per trip, every load and store of the wave 64 bytes in a row */
    const uint8_t *src = j.d_reftext + A.ref_off;
    uint8_t *dst = j.d_ref + sink.ref0;
    const uint64_t n = A.ref_len;
    for (uint64_t b = 0; b < n; b += 256u) {
        uint8_t v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint64_t p = b + 64u * u + (uint64_t)lane;
            v[u] = p < n ? (sink.reversed ? j.d_complement[src[n - 1u - p]] : src[p]) : (uint8_t)0;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint64_t p = b + 64u * u + (uint64_t)lane;
            if (p < n) dst[p] = v[u];
        }
    }
}

#endif /* BRX_PAFIN_H */
