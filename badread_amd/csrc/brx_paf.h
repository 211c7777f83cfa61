/*
 * brx_paf.h -- truth alignments of a simulate batch as PAF text (brx_emit_paf).  Included once by brx_hip.hip after
 * brx_kernels.h.
 *
 * A read's truth is the composition of two things the batch leaves in the arena: the provenance of every fragment base
 * (the PSeg list of k_plan_fill) and the final alignment of the errored read (query) against the padded fragment
 * (target), one op byte per column (0 '=' 1 'X' 2 'I' 3 'D', the last RS.n_cols bytes before ops_off + n + m).
 *
 * A record is a maximal run of columns whose target bases (=, X, D) all come from the reference, consecutively on one
 * contig and strand, and whose query bases (=, X, I) are all kept in the FASTQ read; it is trimmed to its first and last
 * =/X column.  Over the M columns (= and X) of good provenance this means: two consecutive ones belong to one record
 * unless a column between them (the later one included) does not continue the run -- a "break".
 *
 * One wave per read, 64 columns per step:
 *   paf_read   walks every column once: r / f from ballot prefix counts, origin from the segment list (a scalar cursor that
 *              only moves forward), break flags against the neighbour column; a record is closed when the next one starts
 *   paf_record sizes a record (a sweep over its columns: op counts and the text length of its CIGAR) and, for the writing
 *              sink, writes it (a second sweep: every lane that ends a CIGAR run places its text with a wave prefix sum;
 *              '-' records mirror the runs, the convention of minimap2 that alignment.py undoes)
 * The same code sizes and writes (PafSink<WRITE, F>): k_paf_size / k_truth_scan / k_paf_write, the pattern of
 * k_recsize / k_scan_rec / k_emit.  The walk hands every record to its sink (sink.record), so brx_sam.h walks the same records.
 * Every sweep over a record's columns begins with the same step (run_step): the lane's column, its op, whether it starts or ends
 * a CIGAR run, and where its run started.
 *
 * brx_emit_paf_fmt (BRX_FMT_*): with BRX_FMT_EQX a CIGAR run is a run of one op instead of one class (template parameter EQX of the
 * sweeps, paf_run), with BRX_FMT_CS a third sweep (cs_sweep) writes minimap2's cs:Z: behind AS:i:.  The sinks and kernels with F
 * (PafSink<*, true>, k_paf_size<true>, k_paf_write<true>) carry the bits as a value; those without hold nothing of them.
 * brx_sam.h and brx_bam.h use the same sweeps.
 */
#ifndef BRX_PAF_H
#define BRX_PAF_H

#define BRX_PAF_NOKEY (~0ull)          /* no origin: pads, adapters, junk, random sequence, glitch inserts */


__device__ __forceinline__ uint32_t paf_digits(uint32_t v) { uint32_t n = 1; while (v >= 10) { v /= 10; ++n; } return n; }
__device__ __forceinline__ int paf_top(uint64_t bits) { return 63 - __builtin_clzll(bits); }     /* bits != 0 */
__device__ __forceinline__ uint32_t paf_cls(uint32_t op) { return op <= 1 ? 0u : op; }              /* M (= or X), I, D */
/* what a CIGAR run is a run of: the class, or with BRX_FMT_EQX the op itself (= X I D) */
template <bool EQX> __device__ __forceinline__ uint32_t paf_run(uint32_t op) { return EQX ? op : paf_cls(op); }
template <bool EQX> __device__ __forceinline__ uint8_t paf_letter(uint32_t op) {
    return (uint8_t)(EQX ? (op == 0 ? '=' : op == 1 ? 'X' : op == 2 ? 'I' : 'D') : (op <= 1 ? 'M' : op == 2 ? 'I' : 'D'));
}

struct PafRec { uint32_t c0, c1, r0, f0; uint64_t key0; };      /* first / last M column, read index and origin of the first; f0: its index in the
                                                                    padded fragment, kept only for a sink that asks (S::need_f0: MD:Z:, brx_sam.h; cs:Z:) */
struct PafRead {                                                 /* what a record needs of its read (uniform over the wave) */
    const uint8_t *ops; uint64_t read; uint32_t seq_len, start_trim;
    const uint8_t *frag;             /* the padded fragment the read was aligned against (Fbuf + RS.F_off); set by the kernels that write MD:Z: or cs:Z: */
    uint32_t best;                   /* the primary record (writing sink: found by the sizing pass) */
    uint32_t n_rec, top, top_set; int64_t top_as; uint64_t at;      /* records so far, the first of the highest AS among them */
};
struct PafShape { uint32_t cnt[4], text, runs; };                /* a record's columns by op, the text length and the runs of its CIGAR */

/* The sinks of the walk (paf_read): what is done with every record it closes.  brx_sam.h and brx_bam.h add their own. */
template <class S> __device__ void paf_record(S &sink, const BrxDev &d, PafRead &R, const PafRec &q);
/* WRITE: sizes or writes.  F: with BRX_FMT_* bits (fmt, uniform over the grid) and the read's kept bases for cs:Z: (seq); without F
   the two stay unset and unread. */
template <bool WRITE, bool F> struct PafSink {
    static constexpr bool write = WRITE, need_f0 = F, fmtd = F; uint8_t *out; uint32_t fmt; const uint8_t *seq;
    __device__ void record(const BrxDev &d, PafRead &R, const PafRec &q) { paf_record(*this, d, R, q); }
};
/* a sink's BRX_FMT_* bits: the constant 0 for the sinks without (fmtd = false), whose code holds nothing of the formats */
template <class S> __device__ __forceinline__ uint32_t sink_fmt(const S &sink) { if constexpr (S::fmtd) return sink.fmt; else return 0u; }

/* The header fields of a record (qname .. cg:Z:) and its tail (\tNM:i:..\tAS:i:..\n). */
template <class B>
__device__ void paf_head(B &b, const BrxDev &d, const PafRead &R, const PafRec &q, uint32_t qlen_cols, uint32_t tspan, uint32_t n_eq,
                         uint32_t cols, bool primary) {
    const uint32_t cs = (uint32_t)(q.key0 >> 32), contig = cs >> 1, strand = cs & 1u, p0 = (uint32_t)q.key0;
    const brx_contig ct = d.ref.d_contigs[contig];
    put_uuid(b, d, R.read); b.put('\t');
    put_dec(b, R.seq_len); b.put('\t');
    put_dec(b, q.r0 - R.start_trim); b.put('\t'); put_dec(b, q.r0 - R.start_trim + qlen_cols); b.put('\t');
    b.put(strand ? '-' : '+'); b.put('\t');
    for (uint32_t x = 0; x < ct.name_len; ++x) b.put(d.ref.d_names[ct.name_off + x]);
    b.put('\t'); put_dec(b, ct.length); b.put('\t');
    const uint64_t ts = strand ? (uint64_t)ct.length - (uint64_t)p0 - tspan : (uint64_t)p0;
    put_dec(b, ts); b.put('\t'); put_dec(b, ts + tspan); b.put('\t');
    put_dec(b, n_eq); b.put('\t'); put_dec(b, cols); put_str(b, "\t60\ttp:A:"); b.put(primary ? 'P' : 'S'); put_str(b, "\tcg:Z:");
}
template <class B>
__device__ void paf_tags(B &b, uint32_t nm, int64_t as) {
    put_str(b, "\tNM:i:"); put_dec(b, nm); put_str(b, "\tAS:i:");
    if (as < 0) { b.put('-'); put_dec(b, (uint64_t)(-as)); } else put_dec(b, (uint64_t)as);
}
template <class B>
__device__ void paf_tail(B &b, uint32_t nm, int64_t as) { paf_tags(b, nm, as); b.put('\n'); }

/* What every sweep over the record [q.c0, q.c1] begins a 64-column step at b with: the lane's column c (in: inside the record), its op,
   whether it starts (rs) or ends (re) a run -- of one class, with EQX of one op; beyond the record's ends prev / next are 0xFF, which is
   no op and no class -- the ballot of the starts, the first column s0 of the lane's own run (run_start: the last start of the steps
   before) and what the next step takes for run_start.  Every lane calls it. */
struct RunStep { uint32_t c, op, s0, next_start; bool in, rs, re; uint64_t rmask; };
template <bool EQX>
__device__ __forceinline__ RunStep run_step(const PafRead &R, const PafRec &q, uint32_t b, uint32_t run_start) {
    const int lane = lane_id();
    RunStep t;
    t.c = b + lane;
    t.in = t.c <= q.c1;
    t.op = t.in ? R.ops[t.c] : 0u;
    const uint32_t prev = (t.in && t.c > q.c0) ? R.ops[t.c - 1] : 0xFFu;
    const uint32_t next = (t.in && t.c < q.c1) ? R.ops[t.c + 1] : 0xFFu;
    t.rs = t.in && paf_run<EQX>(prev) != paf_run<EQX>(t.op);
    t.re = t.in && paf_run<EQX>(next) != paf_run<EQX>(t.op);
    t.rmask = __ballot(t.rs);
    const uint64_t mine = t.rmask & ((2ull << lane) - 1ull);
    t.s0 = mine ? b + (uint32_t)paf_top(mine) : run_start;
    t.next_start = t.rmask ? b + (uint32_t)paf_top(t.rmask) : run_start;
    return t;
}
/* the n decimal digits of v at p[0, n) */
__device__ __forceinline__ void put_dec_at(uint8_t *p, uint32_t v, uint32_t n) { for (uint32_t x = n; x-- > 0;) { p[x] = (uint8_t)('0' + v % 10); v /= 10; } }

/* Sweep 1 over the record [q.c0, q.c1]: op counts, the CIGAR's text length and its number of runs.  A lane whose column ends a run (the next column
   is another class, or the record ends) owns that run's text: its decimal length and the letter.  Every lane calls it. */
template <bool EQX>
__device__ PafShape paf_shape(const PafRead &R, const PafRec &q) {
    PafShape sh; sh.cnt[0] = sh.cnt[1] = sh.cnt[2] = sh.cnt[3] = 0; sh.text = 0; sh.runs = 0;
    uint32_t run_start = q.c0;
    for (uint32_t b = q.c0; b <= q.c1; b += 64) {
        const RunStep t = run_step<EQX>(R, q, b, run_start);
        sh.text += wave_sum(t.re ? paf_digits(t.c - t.s0 + 1) + 1u : 0u);
        sh.runs += (uint32_t)__popcll(t.rmask);
        for (uint32_t o = 0; o < 4; ++o) sh.cnt[o] += (uint32_t)__popcll(__ballot(t.in && t.op == o));
        run_start = t.next_start;
    }
    return sh;
}

/* Sweep 2: every run's text at its place in cig[0, text); the prefix sum of the text lengths over the lanes gives it.  '-'
   records mirror the runs. */
template <bool EQX>
__device__ void paf_cigar(const PafRead &R, const PafRec &q, uint8_t *cig, uint32_t text, bool minus) {
    uint32_t done = 0, run_start = q.c0;
    for (uint32_t b = q.c0; b <= q.c1; b += 64) {
        const RunStep s = run_step<EQX>(R, q, b, run_start);
        const uint32_t len = s.c - s.s0 + 1u;
        const uint32_t t = s.re ? paf_digits(len) + 1u : 0u;
        const uint32_t incl = wave_incl_scan(t);
        if (s.re) {
            const uint32_t fwd = done + incl - t;
            uint8_t *p = cig + (minus ? text - fwd - t : fwd);
            put_dec_at(p, len, t - 1u);
            p[t - 1] = paf_letter<EQX>(s.op);
        }
        done += wave_bcast_u32(incl, 63);
        run_start = s.next_start;
    }
}

/* ---- cs:Z: (BRX_FMT_CS) ----------------------------------------------------------------------------------------------------- */
#define BRX_PAF_CS "\tcs:Z:"
#define BRX_PAF_CS_LEN ((uint32_t)sizeof(BRX_PAF_CS) - 1u)

/* The sweep over the record [q.c0, q.c1] for minimap2's cs.  Every column owns a piece of the value (possibly empty), the wave's prefix
   sum places it:
     =  short form: the LAST column of a run of n owns ":n" (n = its distance to the run's first column, found as paf_shape finds it: the
        ballot of the run starts, carried across steps); long form: every column owns its reference base, the run's first one '=' before it
     X  "*", the reference base, the read's base
     I  the read's base; the run's first column '+' before it          D  the reference base; the run's first column '-' before it
   Bases of X, I and D in lower case.  '-' records are mirrored piece by piece (a piece keeps its own order), the bases complemented, and
   the '=' '+' '-' in front of a run goes to the run's LAST column, as '^' does in md_sweep.  The reference base is the fragment's
   (R.frag at q.f0 + the target columns before the lane: MD's base), the read's base is seq[(q.r0 - start_trim) + the query columns before
   the lane] (what SEQ holds).  WRITE = false only sizes: no fragment or sequence byte is read; it returns the value's length, which the
   writing sweep is given.  Every lane calls it. */
template <bool WRITE>
__device__ uint32_t cs_sweep(const BrxDev &d, const PafRead &R, const PafRec &q, bool minus, bool lng, const uint8_t *seq, uint8_t *cs, uint32_t text) {
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t done = 0, run_start = q.c0, f_base = q.f0, r_base = q.r0 - R.start_trim;
    for (uint32_t b = q.c0; b <= q.c1; b += 64) {
        const RunStep s = run_step<true>(R, q, b, run_start);            /* cs runs are runs of one op, whatever the CIGAR's are */
        const bool in = s.in, re = s.re, lead = minus ? s.re : s.rs;
        const uint32_t op = s.op, n = s.c - s.s0 + 1u;
        uint32_t t = 0;
        if (in) t = op == 1u ? 3u : (op == 0u && !lng) ? (re ? 1u + paf_digits(n) : 0u) : 1u + (lead ? 1u : 0u);
        if (!WRITE) done += wave_sum(t);
        else {
            const uint64_t tm = __ballot(in && op != 2u), qm = __ballot(in && op != 3u);
            const uint32_t incl = wave_incl_scan(t);
            if (t) {
                uint8_t *p = cs + (minus ? text - (done + incl) : done + incl - t);
                uint8_t rb = 0, qb = 0;
                if (op != 2u) { const uint32_t code = R.frag[f_base + (uint32_t)__popcll(tm & below)] & 15u; rb = d.ref.sym[minus ? d.ref.comp[code] & 15u : code]; }
                if (op != 3u && op != 0u) { const uint32_t code = seq[r_base + (uint32_t)__popcll(qm & below)] & 15u; qb = d.ref.sym[minus ? d.ref.comp[code] & 15u : code]; }
                if (op == 1u) { p[0] = '*'; p[1] = (uint8_t)(rb | 0x20u); p[2] = (uint8_t)(qb | 0x20u); }
                else if (op == 0u && !lng) {
                    p[0] = ':';
                    put_dec_at(p + 1, n, t - 1u);
                } else {
                    if (lead) p[0] = (uint8_t)(op == 0u ? '=' : op == 2u ? '+' : '-');
                    p[t - 1u] = op == 0u ? rb : (uint8_t)((op == 2u ? qb : rb) | 0x20u);
                }
            }
            done += wave_bcast_u32(incl, 63);
            f_base += (uint32_t)__popcll(tm); r_base += (uint32_t)__popcll(qm);
        }
        run_start = s.next_start;
    }
    return WRITE ? text : done;
}

/* Counts the record in; true when it is the read's best so far: the first of the highest AS becomes the primary. */
__device__ __forceinline__ bool paf_rank(PafRead &R, int64_t as) {
    const bool top = !R.top_set || as > R.top_as;
    if (top) { R.top_as = as; R.top = R.n_rec; R.top_set = 1; }
    R.n_rec += 1;
    return top;
}

/* One record [q.c0, q.c1] of the read: sized, and written when S writes.  Every lane calls it (wave-uniform arguments). */
template <class S>
__device__ void paf_record(S &sink, const BrxDev &d, PafRead &R, const PafRec &q) {
    const uint32_t fmt = sink_fmt(sink);
    const bool eqx = (fmt & BRX_FMT_EQX) != 0, minus = ((q.key0 >> 32) & 1u) != 0;
    const PafShape sh = eqx ? paf_shape<true>(R, q) : paf_shape<false>(R, q);
    const uint32_t *cnt = sh.cnt, text = sh.text;
    const uint32_t cols = q.c1 - q.c0 + 1u;
    const uint32_t nm = cnt[1] + cnt[2] + cnt[3];
    const int64_t as = (int64_t)cnt[0] - (int64_t)nm;
    const uint32_t qcols = cnt[0] + cnt[1] + cnt[2], tspan = cnt[0] + cnt[1] + cnt[3];
    const bool primary = S::write && R.n_rec == R.best;
    paf_rank(R, as);
    CountSink hc; hc.n = 0;
    paf_head(hc, d, R, q, qcols, tspan, cnt[0], cols, primary);
    CountSink tc; tc.n = 0;
    paf_tags(tc, nm, as);
    uint32_t cs_text = 0, cs_len = 0;
    if constexpr (S::fmtd) if (fmt & BRX_FMT_CS) {
        cs_text = cs_sweep<false>(d, R, q, minus, (fmt & BRX_FMT_CS_LONG) != 0, nullptr, nullptr, 0u);
        cs_len = BRX_PAF_CS_LEN + cs_text;
    }
    if (S::write) {
        uint8_t *o = sink.out + R.at;
        if (lane_id() == 0) {
            ByteSink h; h.p = o; h.n = 0;
            paf_head(h, d, R, q, qcols, tspan, cnt[0], cols, primary);
            ByteSink tl; tl.p = o + hc.n + text; tl.n = 0;
            paf_tags(tl, nm, as);
            if (cs_len) { put_str(tl, BRX_PAF_CS); tl.n += cs_text; }                 /* the value is the wave's, below */
            tl.put('\n');
        }
        if (eqx) paf_cigar<true>(R, q, o + hc.n, text, minus); else paf_cigar<false>(R, q, o + hc.n, text, minus);
        if constexpr (S::fmtd) if (cs_len)
            cs_sweep<true>(d, R, q, minus, (fmt & BRX_FMT_CS_LONG) != 0, sink.seq, o + hc.n + text + tc.n + BRX_PAF_CS_LEN, cs_text);
    }
    R.at += hc.n + text + tc.n + cs_len + 1u;
}

/* Every record of read r, in column order (= increasing qstart); R.at advances by the read's PAF bytes, R.top = its primary. */
template <class S>
__device__ void paf_read(S &sink, const BrxDev &d, const RS &s, uint32_t r, const PSeg *segs, const uint8_t *arena, PafRead &R) {
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t n = s.n, m = s.m, ncols = s.n_cols, k = (uint32_t)d.em.k, flen = s.frag_len;
    const uint32_t lo = s.start_trim, hi = (s.end_trim == 0 || m < s.end_trim) ? 0u : m - s.end_trim;      /* kept: lo <= r < hi */
    R.ops = arena + s.ops_off + (uint64_t)n + (uint64_t)m - ncols;
    R.read = d.first_read + r; R.seq_len = s.seq_len; R.start_trim = lo;
    R.n_rec = 0; R.top = 0; R.top_set = 0; R.top_as = 0;
    const PSeg *sg = segs + s.seg_off;
    uint32_t r_base = 0, f_base = 0, cur = 0;
    uint64_t carry_key = BRX_PAF_NOKEY, last_m = 0;
    bool carry_good = false, pend = true, open = false;
    PafRec q; q.c0 = q.c1 = q.r0 = q.f0 = 0; q.key0 = 0;
    for (uint32_t b = 0; b < ncols; b += 64) {
        const uint32_t c = b + lane;
        const bool in = c < ncols;
        const uint32_t op = in ? R.ops[c] : 0u;
        const bool isq = in && op != 3u, ist = in && op != 2u;
        const uint64_t qm = __ballot(isq), tm = __ballot(ist);
        const uint32_t rr = r_base + (uint32_t)__popcll(qm & below), ff = f_base + (uint32_t)__popcll(tm & below);
        /* origin of the target base: the segment cursor moves forward while some lane lies beyond the current segment */
        const uint32_t fq = ff - k;
        bool need = ist && ff >= k && fq < flen;
        uint64_t key = BRX_PAF_NOKEY;
        while (__ballot(need) && cur < s.n_segs) {        /* the segments cover [0, frag_len): the bound only guards the load */
            const PSeg g = sg[cur];
            if (need && fq < g.dst + g.len) {
                if ((g.w0 & 3u) == SEG_REF)
                    key = ((uint64_t)((g.w0 >> 5) * 2u + ((g.w0 >> 2) & 7u)) << 32) | (uint64_t)(g.start + (fq - g.dst));
                need = false;
            }
            if (__ballot(need)) ++cur;
        }
        if (cur >= s.n_segs) cur = s.n_segs ? s.n_segs - 1u : 0u;
        const bool kept = rr >= lo && rr < hi;
        const bool good = in && (!ist || key != BRX_PAF_NOKEY) && (!isq || kept);
        /* the previous column's state and the previous target column's origin */
        const bool up_good = __shfl_up((int)good, 1, 64) != 0;
        const bool prev_good = lane == 0 ? carry_good : up_good;
        const uint64_t tb = tm & below;
        const uint64_t up_key = wave_bcast_u64(key, tb ? paf_top(tb) : lane);
        const uint64_t prev_key = tb ? up_key : carry_key;
        const bool link = good && prev_good && (!ist || (prev_key != BRX_PAF_NOKEY && prev_key + 1 == key));
        const bool gm = good && op <= 1u;
        const uint64_t mm = __ballot(gm), bm = __ballot(in && !link);
        /* an M column starts a record when a break lies after the previous M column, up to itself */
        const uint64_t pmb = mm & below, lbb = bm & (below | (1ull << lane));
        const int pm = pmb ? paf_top(pmb) : -1, lb = lbb ? paf_top(lbb) : -1;
        const bool start = gm && (lb > pm || (pm < 0 && lb < 0 && pend));
        uint64_t sm = __ballot(start);
        while (sm) {
            const int L = __builtin_ctzll(sm);
            sm &= sm - 1ull;
            const uint64_t before = mm & ((1ull << L) - 1ull);
            const uint32_t r0 = wave_bcast_u32(rr, L);
            const uint64_t k0 = wave_bcast_u64(key, L);
            const uint32_t f0 = S::need_f0 ? wave_bcast_u32(ff, L) : 0u;
            if (open) { q.c1 = before ? b + (uint32_t)paf_top(before) : (uint32_t)last_m; sink.record(d, R, q); }
            q.c0 = b + (uint32_t)L; q.r0 = r0; q.f0 = f0; q.key0 = k0; open = true;
        }
        if (mm) {
            const int hm = paf_top(mm);
            last_m = b + (uint32_t)hm;
            pend = (bm & ~((2ull << hm) - 1ull)) != 0;
        } else pend = pend || bm != 0;
        carry_good = wave_bcast_u32((uint32_t)good, 63) != 0;
        if (tm) carry_key = wave_bcast_u64(key, paf_top(tm));
        r_base += (uint32_t)__popcll(qm); f_base += (uint32_t)__popcll(tm);
    }
    if (open) { q.c1 = (uint32_t)last_m; sink.record(d, R, q); }
}

__device__ __forceinline__ bool paf_has_records(const RS &s) {
    return s.rec_len != 0 && s.n_cols != 0 && !(s.status & (BRX_RS_BAND | BRX_RS_NOFRAG | BRX_RS_EMPTY | BRX_RS_TOO_MANY_SEGS));
}

/* bytes and primary record of every read */
template <bool F>
__global__ void __launch_bounds__(64) k_paf_size(BrxDev d, const RS *rs, const PSeg *segs, const uint8_t *arena, uint32_t fmt, uint32_t *len, uint32_t *best) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    PafRead R; R.at = 0; R.best = 0; R.top = 0; R.frag = nullptr;
    if (paf_has_records(s)) { PafSink<false, F> k_; k_.out = nullptr; if constexpr (F) { k_.fmt = fmt; k_.seq = nullptr; } paf_read(k_, d, s, r, segs, arena, R); }
    if (lane_id() == 0) { len[r] = (uint32_t)R.at; best[r] = R.top; }
}

/* read offsets of every truth format, and the SA table's record offsets: off[r] (n_reads + 1 entries, the last = the total); the running
   sums are 64 bits throughout (a batch's SAM or BAM records may pass 2^32 bytes) */
__global__ void __launch_bounds__(64) k_truth_scan(uint32_t n_reads, const uint32_t *len, uint64_t *off) {
    const int lane = lane_id();
    uint64_t run = 0;
    for (uint32_t base = 0; base < n_reads; base += 64) {
        const uint32_t r = base + lane;
        const uint64_t l = r < n_reads ? len[r] : 0u;
        uint64_t inc = l;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)inc, dd, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(inc >> 32), dd, 64);
            if (lane >= dd) inc += ((uint64_t)hi << 32) | lo;
        }
        if (r < n_reads) off[r] = run + inc - l;
        run += wave_bcast_u64(inc, 63);
    }
    if (lane == 0) off[n_reads] = run;
}

/* with F the writing kernel is given the fragments (Fbuf) and the reads' sequences (seqbuf, where k_emit read them) for cs:Z: */
template <bool F>
__global__ void __launch_bounds__(64) k_paf_write(BrxDev d, const RS *rs, const PSeg *segs, const uint8_t *arena, const uint8_t *seqbuf, const uint8_t *Fbuf,
                                                   uint32_t fmt, const uint64_t *off, const uint32_t *best, uint8_t *out) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    if (!paf_has_records(s)) return;
    PafRead R; R.at = off[r]; R.best = best[r]; R.frag = F ? Fbuf + s.F_off : nullptr;
    PafSink<true, F> w; w.out = out;
    if constexpr (F) { w.fmt = fmt; w.seq = seqbuf + s.seq_off + s.start_trim; }           /* as k_emit reads them */
    paf_read(w, d, s, r, segs, arena, R);
}

#endif /* BRX_PAF_H */
