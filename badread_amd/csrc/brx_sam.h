/*
 * brx_sam.h -- truth alignments of a simulate batch as SAM records (brx_emit_sam).  Included once by brx_hip.hip after
 * brx_paf.h.
 *
 * The records and the primary are the PAF's: the walk (paf_read), the two sweeps over a record's columns (paf_shape,
 * paf_cigar) and the choice of the primary (paf_rank) are brx_paf.h's; only what is done with a record differs.  A SAM line is
 *
 *   name FLAG RNAME POS 60 [clip]CIGAR[clip] * 0 0 SEQ QUAL NM:i: AS:i: [CO:Z:comment]
 *
 * with the whole read, soft clips and the FASTQ header's comment on the primary, the record's slice and hard clips on the
 * others (2048); '-' lines carry the reverse complement (ref.comp on the codes) and the reversed qualities.  A read with a FASTQ
 * record and no PAF record gets one unmapped line (FLAG 4), a read without a FASTQ record nothing.
 *
 * The primary is known only when the sizing walk ends, and its line is longer than the same record's supplementary line.  So
 * k_sam_size sizes every record as supplementary and keeps, beside the running best AS, what that record would add as the
 * primary (SamSink.surplus); it reads no SEQ or QUAL byte.  k_sam_write knows the primary from the sizing pass.  One wave per
 * read; lane 0 writes the fixed fields, the wave places the CIGAR runs and copies SEQ and QUAL 64 bytes per step (contiguous
 * stores; on '-' lines the loads run backwards).
 *
 * brx_emit_sam_fmt adds =/X CIGAR runs and cs:Z: (BRX_FMT_*; template parameter F of the sinks and kernels: with F the bits are a value
 * uniform over the grid, without it the code holds nothing of them).  The runs are paf_shape's and paf_cigar's, cs is brx_paf.h's cs_sweep.
 *
 * brx_emit_sam_tags adds MD:Z: and SA:Z: behind AS:i: (template parameter TAGS of the sinks and kernels; TAGS = 0 is the code above).
 *   MD  a third sweep over the record's columns (md_sweep): every X column and every D column owns a piece of the text, the wave's
 *       prefix sum places it; the number in front of an item is the count of '=' columns since the item before it (ballot
 *       popcounts, carried across steps).  The reference base is the fragment's: Fbuf + RS.F_off is carved from the bottom of the
 *       arena before anything take_top() hands out and lies under nothing the final stage's slabs reuse, so the bytes the read was
 *       aligned against are still there when the truth is emitted -- the packed reference is not consulted.
 *   SA  needs every record of the read before its first line: the sizing pass leaves the records per read, k_sa_fill writes one
 *       SaRec per record of every read with two or more into the context's table, and a line's value is then written one lane per
 *       element (sa_write).
 */
#ifndef BRX_SAM_H
#define BRX_SAM_H

#include <type_traits>

#define BRX_SAM_UNMAPPED (~0u)         /* best[r] of a read whose one line is the unmapped one */
#define BRX_SAM_NAME 36u               /* characters of a read name (put_uuid) */
#define BRX_SAM_MATE "\t*\t0\t0\t"                       /* RNEXT PNEXT TLEN, between CIGAR and SEQ */
#define BRX_SAM_NOMAP "\t4\t*\t0\t0\t*\t*\t0\t0\t"      /* FLAG .. TLEN of an unmapped line */
#define BRX_SAM_CO "\tCO:Z:"
#define BRX_SAM_MD "\tMD:Z:"
#define BRX_SAM_SA "\tSA:Z:"
#define BRX_SAM_LEN(lit) ((uint32_t)sizeof(lit) - 1u)

/* the fields of a mapped line before its CIGAR, and the clips around it */
template <class B>
__device__ void sam_head(B &b, const BrxDev &d, const PafRead &R, const PafRec &q, uint32_t tspan, bool primary) {
    const uint32_t cs = (uint32_t)(q.key0 >> 32), contig = cs >> 1, strand = cs & 1u, p0 = (uint32_t)q.key0;
    const brx_contig ct = d.ref.d_contigs[contig];
    put_uuid(b, d, R.read); b.put('\t');
    put_dec(b, (strand ? 16u : 0u) | (primary ? 0u : 2048u)); b.put('\t');
    for (uint32_t x = 0; x < ct.name_len; ++x) b.put(d.ref.d_names[ct.name_off + x]);
    b.put('\t');
    const uint64_t ts = strand ? (uint64_t)ct.length - (uint64_t)p0 - tspan : (uint64_t)p0;
    put_dec(b, ts + 1); put_str(b, "\t60\t");
}
template <class B>
__device__ void sam_clip(B &b, uint32_t n, bool primary) { if (n) { put_dec(b, n); b.put(primary ? 'S' : 'H'); } }

/* what a line needs of its read beside PafRead */
struct SamRead { const RS *s; const PPiece *pieces; const uint8_t *seq, *qual; };

/* SEQ, a tab and QUAL of the read's bases [lo, hi) at o, reversed and complemented for a '-' line.  Every lane calls it. */
__device__ void sam_bases(const BrxDev &d, const SamRead &M, uint8_t *o, uint32_t lo, uint32_t hi, bool minus) {
    const int lane = lane_id();
    const uint32_t len = hi - lo;
    for (uint32_t x = lane; x < len; x += 64) {
        const uint32_t src = minus ? hi - 1u - x : lo + x;
        const uint32_t code = M.seq[src] & 15u;
        o[x] = d.ref.sym[minus ? d.ref.comp[code] & 15u : code];
        o[len + 1u + x] = M.qual[src];
    }
    if (lane == 0) o[len] = '\t';
}


/* ---- MD:Z: ---------------------------------------------------------------------------------------------------------------- */
struct MdShape { uint32_t text, tail; };       /* length of the value; its last number: the '=' columns behind the last item */

/* The sweep over the record [q.c0, q.c1] for MD.  An X column owns "<u><base>", the first column of a D run "<u>^<base>", every
   other D column "<base>"; u = the '=' columns since the last X or D column (I columns do nothing).  '-' records are mirrored piece
   by piece: "<base><u>", the '^' goes to the run's LAST column, and the value's last number comes first.  WRITE = false only sizes
   (no fragment byte is read) and returns the shape that the writing sweep is given.  Every lane calls it. */
template <bool WRITE>
__device__ MdShape md_sweep(const BrxDev &d, const PafRead &R, const PafRec &q, bool minus, uint8_t *md, MdShape sh) {
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t done = 0, carry = 0, f_base = q.f0;
    for (uint32_t b = q.c0; b <= q.c1; b += 64) {
        const uint32_t c = b + lane;
        const bool in = c <= q.c1;
        const uint32_t op = in ? R.ops[c] : 2u;
        const uint32_t prev = (in && c > q.c0) ? R.ops[c - 1] : 0xFFu;
        const uint32_t next = (in && c < q.c1) ? R.ops[c + 1] : 0xFFu;
        const bool isx = in && op == 1u, isd = in && op == 3u;
        const bool first = isd && prev != 3u, last = isd && next != 3u, owner = isx || first;
        const uint64_t eq = __ballot(in && op == 0u), brk = __ballot(isx || isd);
        const uint64_t pb = brk & below;
        const uint32_t u = pb ? (uint32_t)__popcll(eq & below & ~((2ull << paf_top(pb)) - 1ull)) : carry + (uint32_t)__popcll(eq & below);
        const uint32_t nd = owner ? paf_digits(u) : 0u;
        const uint32_t t = ((isx || isd) ? 1u : 0u) + nd + ((minus ? last : first) ? 1u : 0u);
        if (!WRITE) done += wave_sum(t);
        else {
            const uint64_t tm = __ballot(in && op != 2u);
            const uint32_t incl = wave_incl_scan(t);
            if (t) {
                const uint32_t fwd = done + incl - t;
                const uint32_t code = R.frag[f_base + (uint32_t)__popcll(tm & below)] & 15u;
                const uint8_t base = d.ref.sym[minus ? d.ref.comp[code] & 15u : code];
                uint8_t *p = md + (minus ? sh.text - fwd - t : fwd);
                uint8_t *num = minus ? p + (t - nd) : p;
                put_dec_at(num, u, nd);
                if (minus) { if (last) p[0] = '^'; p[last ? 1 : 0] = base; }
                else { if (first) p[nd] = '^'; p[t - 1] = base; }
            }
            done += wave_bcast_u32(incl, 63);
            f_base += (uint32_t)__popcll(tm);
        }
        if (brk) carry = (uint32_t)__popcll(eq & ~((2ull << paf_top(brk)) - 1ull)); else carry += (uint32_t)__popcll(eq);
    }
    if (!WRITE) { sh.tail = carry; sh.text = done + paf_digits(carry); }
    else if (lane == 0) {
        const uint32_t nd = paf_digits(sh.tail);
        put_dec_at(minus ? md : md + sh.text - nd, sh.tail, nd);
    }
    return sh;
}

/* ---- SA:Z: ---------------------------------------------------------------------------------------------------------------- */
struct SaRec { uint32_t cs, pos, left, right, q, t, nm, len; };     /* contig << 1 | strand, POS, the clips, M+I, M+D, NM; the length of its element */

/* RNAME,POS,strand,CIGAR,60,NM; -- the CIGAR in the compact form: the clips as S, one M, and the surplus of either side as one I or D */
template <class B>
__device__ void sa_element(B &b, const BrxDev &d, const SaRec &e) {
    const brx_contig ct = d.ref.d_contigs[e.cs >> 1];
    for (uint32_t x = 0; x < ct.name_len; ++x) b.put(d.ref.d_names[ct.name_off + x]);
    b.put(','); put_dec(b, e.pos); b.put(','); b.put((e.cs & 1u) ? '-' : '+'); b.put(',');
    if (e.left) { put_dec(b, e.left); b.put('S'); }
    put_dec(b, e.q < e.t ? e.q : e.t); b.put('M');
    if (e.q > e.t) { put_dec(b, e.q - e.t); b.put('I'); } else if (e.t > e.q) { put_dec(b, e.t - e.q); b.put('D'); }
    if (e.right) { put_dec(b, e.right); b.put('S'); }
    put_str(b, ",60,"); put_dec(b, e.nm); b.put(';');
}

/* what the other lines of the read say about the record q of shape sh */
__device__ SaRec sa_rec_of(const BrxDev &d, const PafRead &R, const PafRec &q, const PafShape &sh) {
    const uint32_t cs = (uint32_t)(q.key0 >> 32), p0 = (uint32_t)q.key0;
    const uint32_t qcols = sh.cnt[0] + sh.cnt[1] + sh.cnt[2], tspan = sh.cnt[0] + sh.cnt[1] + sh.cnt[3];
    const uint32_t qs = q.r0 - R.start_trim, qe = qs + qcols;
    SaRec e; e.cs = cs;
    e.pos = ((cs & 1u) ? d.ref.d_contigs[cs >> 1].length - p0 - tspan : p0) + 1u;
    e.left = (cs & 1u) ? R.seq_len - qe : qs; e.right = (cs & 1u) ? qs : R.seq_len - qe;
    e.q = qcols; e.t = tspan; e.nm = sh.cnt[1] + sh.cnt[2] + sh.cnt[3];
    CountSink k_; k_.n = 0; sa_element(k_, d, e);
    e.len = k_.n;
    return e;
}

/* the sink of k_sa_fill: record i of the read goes to tab[i] */
struct SaFill {
    static constexpr bool write = false, need_f0 = false, fmtd = false; SaRec *tab;
    __device__ void record(const BrxDev &d, PafRead &R, const PafRec &q) {
        const PafShape sh = paf_shape<false>(R, q);                       /* the compact CIGAR takes the op counts alone */
        const SaRec e = sa_rec_of(d, R, q, sh);
        if (lane_id() == 0) tab[R.n_rec] = e;
        R.n_rec += 1;
    }
};

/* The table of a read's n records (n >= 2, or 0: no SA), and the sum of their elements' lengths. */
struct SaRead { const SaRec *tab; uint32_t n, sum; };
__device__ SaRead sa_read_of(const SaRec *table, const uint64_t *rec_off, uint32_t r) {
    SaRead A; A.tab = table + rec_off[r]; A.n = (uint32_t)(rec_off[r + 1] - rec_off[r]); A.sum = 0;
    for (uint32_t base = 0; base < A.n; base += 64) {
        const uint32_t j = base + (uint32_t)lane_id();
        A.sum += wave_sum(j < A.n ? A.tab[j].len : 0u);
    }
    return A;
}

/* The SA value of line i at o: the primary's element first unless i is the primary, then the others in line order; one lane per
   element, placed by the prefix sum of the lengths.  Every lane calls it. */
__device__ void sa_write(const BrxDev &d, const SaRead &A, uint32_t i, uint32_t best, uint8_t *o) {
    const uint32_t lane = (uint32_t)lane_id();
    uint32_t done = i != best ? A.tab[best].len : 0u;
    for (uint32_t base = 0; base < A.n; base += 64) {
        const uint32_t j = base + lane;
        const bool have = j < A.n && j != i, lead = have && j == best;
        SaRec e{};
        if (have) e = A.tab[j];
        const uint32_t len = lead ? 0u : e.len;
        const uint32_t incl = wave_incl_scan(len);
        if (have) { ByteSink s_; s_.p = o + (lead ? 0u : done + incl - len); s_.n = 0; sa_element(s_, d, e); }
        done += wave_bcast_u32(incl, 63);
    }
}

template <class S> __device__ void sam_record(S &sink, const BrxDev &d, PafRead &R, const PafRec &q);
/* WRITE: sizes or writes.  TAGS: BRX_TAG_MD | BRX_TAG_SA.  F: the sink carries BRX_FMT_* bits (fmt, uniform over the grid); F = false is
   the code without them.  surplus (sizing only): what the best record so far adds as the primary.  A: the read's SA table (sizing: A.sum is
   the elements' lengths of the records so far). */
struct NoWord {};
template <bool WRITE> using SizingWord = std::conditional_t<WRITE, NoWord, uint32_t>;       /* a word that only a sizing sink holds */
template <bool WRITE, uint32_t TAGS, bool F> struct SamSink {
    static constexpr bool write = WRITE, fmtd = F, need_f0 = (TAGS & BRX_TAG_MD) != 0 || F; static constexpr uint32_t tags = TAGS;
    uint8_t *out; SamRead M; [[no_unique_address]] SizingWord<WRITE> surplus; uint32_t fmt; SaRead A;
    __device__ void record(const BrxDev &d, PafRead &R, const PafRec &q) { sam_record(*this, d, R, q); }
};
/* what k_sam_* and k_bam_* set of their sink before the walk */
template <class S> __device__ __forceinline__ void sink_init(S &k, uint8_t *out, const SamRead &M, uint32_t fmt) {
    k.out = out; k.M = M; if constexpr (!S::write) k.surplus = 0; k.fmt = S::fmtd ? fmt : 0u; k.A.tab = nullptr; k.A.n = 0; k.A.sum = 0;
}
/* the comment's length: the FASTQ header is '@', the name, a blank, the comment and a newline (RS.hdr_len, k_recsize) */
template <class S> __device__ __forceinline__ uint32_t sam_comment(const S &sink) { return sink.M.s->hdr_len - (BRX_SAM_NAME + 3u); }

/* What a SAM line and a BAM record of the record q share, before their layouts part: the shape of the CIGAR (with BRX_FMT_EQX the =/X one),
   NM and AS, the query and target columns, the strand, the clips, the record's place among the read's (line; primary; top: the best AS so
   far, which paf_rank counts in), and the sizes of the tag values -- MD's shape, the text of cs, and of SA the value's length (sa: the line
   has one; a sized line counts none, its element goes to sink.A.sum and the size kernel adds the read's at the end).  What a tag costs
   around its value is the caller's.  Every lane calls it (wave-uniform arguments). */
struct RecGeom {
    PafShape sh; MdShape md; int64_t as;
    uint32_t nm, qcols, tspan, L, qs, qe, left, right, line, cs_text, sa_text;
    bool eqx, cs_long, minus, primary, top, cs, sa;
};
template <class S>
__device__ __forceinline__ RecGeom rec_geom(S &sink, const BrxDev &d, PafRead &R, const PafRec &q) {
    const uint32_t fmt = sink_fmt(sink);
    RecGeom g;
    g.eqx = (fmt & BRX_FMT_EQX) != 0; g.cs_long = (fmt & BRX_FMT_CS_LONG) != 0;
    g.sh = g.eqx ? paf_shape<true>(R, q) : paf_shape<false>(R, q);
    g.nm = g.sh.cnt[1] + g.sh.cnt[2] + g.sh.cnt[3];
    g.as = (int64_t)g.sh.cnt[0] - (int64_t)g.nm;
    g.qcols = g.sh.cnt[0] + g.sh.cnt[1] + g.sh.cnt[2]; g.tspan = g.sh.cnt[0] + g.sh.cnt[1] + g.sh.cnt[3];
    g.minus = ((q.key0 >> 32) & 1u) != 0;
    g.L = R.seq_len; g.qs = q.r0 - R.start_trim; g.qe = g.qs + g.qcols;
    g.left = g.minus ? g.L - g.qe : g.qs; g.right = g.minus ? g.qs : g.L - g.qe;
    g.line = R.n_rec;
    g.primary = S::write && g.line == R.best;
    g.top = paf_rank(R, g.as);
    g.md.text = g.md.tail = 0; g.cs_text = g.sa_text = 0; g.cs = g.sa = false;
    if (S::tags & BRX_TAG_MD) g.md = md_sweep<false>(d, R, q, g.minus, nullptr, g.md);
    if (S::tags & BRX_TAG_SA) {
        if (!S::write) sink.A.sum += sa_rec_of(d, R, q, g.sh).len;
        else if (sink.A.n) { g.sa = true; g.sa_text = sink.A.sum - sink.A.tab[g.line].len; }
    }
    if constexpr (S::fmtd) if (fmt & BRX_FMT_CS) { g.cs = true; g.cs_text = cs_sweep<false>(d, R, q, g.minus, g.cs_long, nullptr, nullptr, 0u); }
    return g;
}

/* One record of the read as a SAM line: sized (as a supplementary line; the primary's surplus goes with the best AS), or
   written.  Every lane calls it (wave-uniform arguments). */
template <class S>
__device__ void sam_record(S &sink, const BrxDev &d, PafRead &R, const PafRec &q) {
    const RecGeom g = rec_geom(sink, d, R, q);
    const bool primary = g.primary, minus = g.minus;
    /* MD:Z:, cs:Z: and SA:Z: behind AS:i:, in this order */
    const uint32_t md_len = (S::tags & BRX_TAG_MD) ? BRX_SAM_LEN(BRX_SAM_MD) + g.md.text : 0u;
    const uint32_t cs_len = g.cs ? BRX_PAF_CS_LEN + g.cs_text : 0u, sa_len = g.sa ? BRX_SAM_LEN(BRX_SAM_SA) + g.sa_text : 0u;
    CountSink hc; hc.n = 0;
    sam_head(hc, d, R, q, g.tspan, primary);
    CountSink lc; lc.n = 0; sam_clip(lc, g.left, primary);
    CountSink rc; rc.n = 0; sam_clip(rc, g.right, primary);
    CountSink tc; tc.n = 0; paf_tags(tc, g.nm, g.as);
    const uint32_t comment = sam_comment(sink);
    const uint32_t bases = primary ? g.L : g.qcols;
    const uint32_t cig_at = hc.n + lc.n, seq_at = cig_at + g.sh.text + rc.n + BRX_SAM_LEN(BRX_SAM_MATE), tag_at = seq_at + 2u * bases + 1u;
    const uint32_t bytes = tag_at + tc.n + md_len + cs_len + sa_len + (primary ? BRX_SAM_LEN(BRX_SAM_CO) + comment : 0u) + 1u;
    if (S::write) {
        uint8_t *o = sink.out + R.at;
        if (lane_id() == 0) {
            ByteSink h; h.p = o; h.n = 0;
            sam_head(h, d, R, q, g.tspan, primary); sam_clip(h, g.left, primary);
            ByteSink m; m.p = o + cig_at + g.sh.text; m.n = 0;
            sam_clip(m, g.right, primary); put_str(m, BRX_SAM_MATE);
            ByteSink t; t.p = o + tag_at; t.n = 0;
            paf_tags(t, g.nm, g.as);
            if (md_len) { put_str(t, BRX_SAM_MD); t.n += g.md.text; }            /* the values are the wave's, below */
            if (cs_len) { put_str(t, BRX_PAF_CS); t.n += g.cs_text; }
            if (sa_len) { put_str(t, BRX_SAM_SA); t.n += g.sa_text; }
            if (primary) { put_str(t, BRX_SAM_CO); put_comment(t, d, *sink.M.s, sink.M.pieces); }
            t.put('\n');
        }
        if (md_len) md_sweep<true>(d, R, q, minus, o + tag_at + tc.n + BRX_SAM_LEN(BRX_SAM_MD), g.md);
        if constexpr (S::fmtd) if (cs_len)
            cs_sweep<true>(d, R, q, minus, g.cs_long, sink.M.seq, o + tag_at + tc.n + md_len + BRX_PAF_CS_LEN, g.cs_text);
        if (sa_len) sa_write(d, sink.A, g.line, R.best, o + tag_at + tc.n + md_len + cs_len + BRX_SAM_LEN(BRX_SAM_SA));
        if (g.eqx) paf_cigar<true>(R, q, o + cig_at, g.sh.text, minus); else paf_cigar<false>(R, q, o + cig_at, g.sh.text, minus);
        sam_bases(d, sink.M, o + seq_at, primary ? 0u : g.qs, primary ? g.L : g.qe, minus);
    }
    /* the same record as the primary: FLAG loses its 2048 (4 digits -> "0" or "16"), SEQ and QUAL are the whole read, CO:Z: */
    if constexpr (!S::write) if (g.top) sink.surplus = 2u * (g.L - g.qcols) + BRX_SAM_LEN(BRX_SAM_CO) + comment - (minus ? 2u : 3u);
    R.at += bytes;
}

/* bytes of the unmapped line of a read of L bases: name, FLAG .. TLEN, SEQ, a tab, QUAL, CO:Z: with the comment, newline */
__device__ __forceinline__ uint32_t sam_unmapped_bytes(uint32_t L, uint32_t comment) {
    return BRX_SAM_NAME + BRX_SAM_LEN(BRX_SAM_NOMAP) + 2u * L + 1u + BRX_SAM_LEN(BRX_SAM_CO) + comment + 1u;
}

__device__ __forceinline__ SamRead sam_of(const RS &s, const PPiece *pieces, const uint8_t *seqbuf) {
    SamRead M; M.s = &s; M.pieces = pieces;
    M.seq = seqbuf + s.seq_off + s.start_trim;                                              /* as k_emit reads them */
    M.qual = seqbuf + s.seq_off + (((uint64_t)s.m + 16 + 15) & ~15ull) + s.start_trim;
    return M;
}

/* The end of k_sam_size and k_bam_size: the bytes and the primary record (BRX_SAM_UNMAPPED: none) of read r.  A read without a record takes
   `unmapped` bytes; with SA every line of a read of two or more gets the tag (`sa_tag`: what it costs around its value) and the elements of
   the n - 1 others, and the read's records are counted into the table (n_rec: 0 below two). */
template <class S>
__device__ __forceinline__ void truth_size_store(const S &k, const PafRead &R, uint32_t r, uint32_t unmapped, uint32_t sa_tag, uint32_t *len, uint32_t *best,
                                                 uint32_t *n_rec) {
    uint32_t bytes = (uint32_t)R.at + k.surplus, top = R.top;
    if (R.n_rec == 0) { top = BRX_SAM_UNMAPPED; bytes = unmapped; }
    if (S::tags & BRX_TAG_SA) {
        const uint32_t n = R.n_rec >= 2 ? R.n_rec : 0u;
        bytes += n * sa_tag + (n ? n - 1u : 0u) * k.A.sum;
        if (lane_id() == 0) n_rec[r] = n;
    }
    if (lane_id() == 0) { len[r] = bytes; best[r] = top; }
}

/* bytes and primary record of every read, SA's record counts */
template <uint32_t TAGS, bool F>
__global__ void __launch_bounds__(64) k_sam_size(BrxDev d, const RS *rs, const PSeg *segs, const uint8_t *arena, uint32_t *len, uint32_t *best,
                                                  uint32_t *n_rec, uint32_t fmt) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    PafRead R; R.at = 0; R.best = 0; R.top = 0; R.n_rec = 0; R.frag = nullptr;
    SamSink<false, TAGS, F> k_; sink_init(k_, nullptr, sam_of(s, nullptr, arena), fmt);
    if (paf_has_records(s)) paf_read(k_, d, s, r, segs, arena, R);
    truth_size_store(k_, R, r, s.rec_len ? sam_unmapped_bytes(s.seq_len, sam_comment(k_)) : 0u, BRX_SAM_LEN(BRX_SAM_SA), len, best, n_rec);
}

/* the SA table: one SaRec per record of every read that the sizing pass counted in (rec_off: the scan of its n_rec) */
__global__ void __launch_bounds__(64) k_sa_fill(BrxDev d, const RS *rs, const PSeg *segs, const uint8_t *arena, const uint64_t *rec_off, SaRec *table) {
    const uint32_t r = blockIdx.x;
    if (rec_off[r + 1] == rec_off[r]) return;
    const RS s = rs[r];
    PafRead R; R.at = 0; R.best = 0; R.top = 0; R.n_rec = 0; R.frag = nullptr;
    SaFill f_; f_.tab = table + rec_off[r];
    paf_read(f_, d, s, r, segs, arena, R);
}

template <uint32_t TAGS, bool F>
__global__ void __launch_bounds__(64) k_sam_write(BrxDev d, const RS *rs, const PSeg *segs, const PPiece *pieces, const uint8_t *arena,
                                                   const uint64_t *off, const uint32_t *best, uint8_t *out, const uint8_t *Fbuf,
                                                   const uint64_t *rec_off, const SaRec *table, uint32_t fmt) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    if (s.rec_len == 0) return;
    SamSink<true, TAGS, F> w; sink_init(w, out, sam_of(s, pieces, arena), fmt);
    if (best[r] != BRX_SAM_UNMAPPED) {
        PafRead R; R.at = off[r]; R.best = best[r]; R.frag = nullptr;
        if (w.need_f0) R.frag = Fbuf + s.F_off;
        if (TAGS & BRX_TAG_SA) w.A = sa_read_of(table, rec_off, r);
        paf_read(w, d, s, r, segs, arena, R);
        return;
    }
    uint8_t *o = out + off[r];
    const uint32_t L = s.seq_len, seq_at = BRX_SAM_NAME + BRX_SAM_LEN(BRX_SAM_NOMAP);
    if (lane_id() == 0) {
        ByteSink h; h.p = o; h.n = 0;
        put_uuid(h, d, d.first_read + r); put_str(h, BRX_SAM_NOMAP);
        ByteSink t; t.p = o + seq_at + 2u * L + 1u; t.n = 0;
        put_str(t, BRX_SAM_CO); put_comment(t, d, s, pieces); t.put('\n');
    }
    sam_bases(d, w.M, o + seq_at, 0u, L, false);
}

#endif /* BRX_SAM_H */
