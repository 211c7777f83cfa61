/*
 * brx_bam.h -- truth alignments of a simulate batch as BAM records (brx_emit_bam; SAM spec v1 section 4.2).  Included once by
 * brx_hip.hip after brx_sam.h.
 *
 * One record per line of brx_emit_sam, in the same order, with the same fields: the walk, the two sweeps and the choice of the
 * primary are brx_paf.h's, the read's bases and the comment are found as brx_sam.h finds them.  All integers little-endian,
 * nothing aligned (the name is 37 bytes: the CIGAR words start at an odd offset), so every store is a byte store.
 *
 *   block_size refID pos l_read_name=37 mapq bin n_cigar_op flag l_seq next_refID=-1 next_pos=-1 tlen=0 name\0
 *   cigar (len << 4 | op, MIDNSH = 0..5; with BRX_FMT_EQX = 7 and X 8 for M)
 *    seq (two bases per byte, '=ACMGRSVTWYHKDBN')   qual (FASTQ character - 33)
 *   NM AS [MD:Z:text\0] [cs:Z:text\0] [SA:Z:text\0] [CO:Z:comment\0] [CG:B:I]     (integers in the smallest type, htslib's rule; MD and SA:
 *                                            brx_emit_bam_tags, the texts of brx_sam.h's md_sweep and sa_write)
 *
 * A record with more than max_ops CIGAR operations, clips included, takes the long form of section 4.2.2: the CIGAR field holds
 * l_seq S and reflen N, the real operations follow as the last tag CG:B:I; bin comes from the real reflen either way.
 *
 * As in brx_sam.h the primary is known only when the sizing walk ends: k_bam_size sizes every record as supplementary and keeps
 * what the best one adds as the primary (whole-read SEQ and QUAL, CO).  The operation count is the same for both (S and H clips),
 * so the choice of the long form does not depend on it.  k_bam_size reads no sequence byte.  k_bam_write: one wave per read; lane 0
 * writes the fixed fields, the clips and the tags, the wave places one CIGAR word per run, packs 128 bases into 64 bytes per
 * step and copies 64 qualities per step -- consecutive lanes store consecutive bytes; on '-' records the loads run backwards.
 */
#ifndef BRX_BAM_H
#define BRX_BAM_H

#define BRX_BAM_CIGAR_AT 73u           /* block_size + 32 bytes of fixed fields + the name and its NUL */
#define BRX_BAM_UNMAPPED_BIN 4680u     /* reg2bin(-1, 0) */
enum { BAM_OP_M = 0, BAM_OP_I = 1, BAM_OP_D = 2, BAM_OP_N = 3, BAM_OP_S = 4, BAM_OP_H = 5, BAM_OP_EQ = 7, BAM_OP_X = 8 };

template <class B> __device__ void put_le(B &b, uint64_t v, int bytes) { for (int i = 0; i < bytes; ++i) b.put((uint8_t)(v >> (8 * i))); }

/* an integer tag in the smallest type that holds it: C S I from 0 up, c s i below */
template <class B>
__device__ void bam_tag_int(B &b, char t0, char t1, int64_t v) {
    b.put((uint8_t)t0); b.put((uint8_t)t1);
    if (v >= 0) { const int n = v <= 255 ? 1 : v <= 65535 ? 2 : 4; b.put((uint8_t)(n == 1 ? 'C' : n == 2 ? 'S' : 'I')); put_le(b, (uint64_t)v, n); }
    else { const int n = v >= -128 ? 1 : v >= -32768 ? 2 : 4; b.put((uint8_t)(n == 1 ? 'c' : n == 2 ? 's' : 'i')); put_le(b, (uint64_t)v, n); }
}
template <class B> __device__ void bam_tags(B &b, uint32_t nm, int64_t as) { bam_tag_int(b, 'N', 'M', (int64_t)nm); bam_tag_int(b, 'A', 'S', as); }

/* the spec's reg2bin (section 5.3) of [beg, end), as the 16 bits the field holds */
__device__ __forceinline__ uint32_t bam_reg2bin(uint32_t beg, uint32_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (((1u << 15) - 1u) / 7u + (beg >> 14)) & 0xFFFFu;
    if (beg >> 17 == end >> 17) return ((1u << 12) - 1u) / 7u + (beg >> 17);
    if (beg >> 20 == end >> 20) return ((1u << 9) - 1u) / 7u + (beg >> 20);
    if (beg >> 23 == end >> 23) return ((1u << 6) - 1u) / 7u + (beg >> 23);
    if (beg >> 26 == end >> 26) return ((1u << 3) - 1u) / 7u + (beg >> 26);
    return 0u;
}

/* block_size .. tlen, the name and its NUL: BRX_BAM_CIGAR_AT bytes */
template <class B>
__device__ void bam_fixed(B &b, const BrxDev &d, uint64_t read, uint32_t block_size, uint32_t ref_id, uint32_t pos, uint32_t mapq, uint32_t bin,
                          uint32_t n_cigar, uint32_t flag, uint32_t l_seq) {
    put_le(b, block_size, 4); put_le(b, ref_id, 4); put_le(b, pos, 4);
    b.put((uint8_t)(BRX_SAM_NAME + 1u)); b.put((uint8_t)mapq); put_le(b, bin, 2); put_le(b, n_cigar, 2); put_le(b, flag, 2); put_le(b, l_seq, 4);
    put_le(b, 0xFFFFFFFFu, 4); put_le(b, 0xFFFFFFFFu, 4); put_le(b, 0u, 4);
    put_uuid(b, d, read); b.put(0);
}

/* code -> nibble of '=ACMGRSVTWYHKDBN' (case-insensitive, anything else 15), sixteen nibbles in a word: forward, and through comp[] */
struct BamNib { uint64_t fwd, rev; };
__device__ __forceinline__ uint32_t bam_nibble_of(uint8_t ch) {
    const char *set = "=ACMGRSVTWYHKDBN";
    if (ch >= 'a' && ch <= 'z') ch = (uint8_t)(ch - 'a' + 'A');
    for (uint32_t i = 0; i < 16; ++i) if ((uint8_t)set[i] == ch) return i;
    return 15u;
}
/* Every lane calls it: lane c < 16 looks up code c, the wave sums the disjoint nibbles. */
__device__ BamNib bam_nibbles(const BrxDev &d) {
    const uint32_t lane = (uint32_t)lane_id(), c = lane & 15u, sh = 4u * (c & 7u);
    const uint32_t f = bam_nibble_of(d.ref.sym[c]) << sh, r = bam_nibble_of(d.ref.sym[d.ref.comp[c] & 15u]) << sh;
    const bool lo = lane < 8, hi = lane >= 8 && lane < 16;
    BamNib T;
    T.fwd = (uint64_t)wave_sum(lo ? f : 0u) | ((uint64_t)wave_sum(hi ? f : 0u) << 32);
    T.rev = (uint64_t)wave_sum(lo ? r : 0u) | ((uint64_t)wave_sum(hi ? r : 0u) << 32);
    return T;
}

/* SEQ and QUAL of the read's bases [lo, hi), reversed and complemented for a '-' record.  Every lane calls it. */
__device__ void bam_bases(const BamNib &T, const SamRead &M, uint8_t *seq, uint8_t *qual, uint32_t lo, uint32_t hi, bool minus) {
    const uint32_t lane = (uint32_t)lane_id(), len = hi - lo, packed = (len + 1u) / 2u;
    const uint64_t tab = minus ? T.rev : T.fwd;
    for (uint32_t x = lane; x < packed; x += 64) {
        const uint32_t i0 = 2u * x, i1 = i0 + 1u;
        const uint32_t n0 = (uint32_t)(tab >> (4u * (M.seq[minus ? hi - 1u - i0 : lo + i0] & 15u))) & 15u;
        const uint32_t n1 = i1 < len ? (uint32_t)(tab >> (4u * (M.seq[minus ? hi - 1u - i1 : lo + i1] & 15u))) & 15u : 0u;
        seq[x] = (uint8_t)((n0 << 4) | n1);
    }
    for (uint32_t x = lane; x < len; x += 64) qual[x] = (uint8_t)(M.qual[minus ? hi - 1u - x : lo + x] - 33u);
}

/* Sweep 2 of a record, binary: the lane whose column ends run i stores that run's word at ops[i] ('-' records: at ops[runs - 1 - i]),
   byte by byte.  The runs are paf_cigar's. */
template <bool EQX>
__device__ void bam_cigar(const PafRead &R, const PafRec &q, uint8_t *ops, uint32_t runs, bool minus) {
    const uint64_t below = (1ull << lane_id()) - 1ull;
    uint32_t done = 0, run_start = q.c0;
    for (uint32_t b = q.c0; b <= q.c1; b += 64) {
        const RunStep s = run_step<EQX>(R, q, b, run_start);
        const uint64_t emask = __ballot(s.re);
        if (s.re) {
            const uint32_t i = done + (uint32_t)__popcll(emask & below), op = s.op;
            const uint32_t code = op == 2 ? (uint32_t)BAM_OP_I : op == 3 ? (uint32_t)BAM_OP_D : !EQX ? (uint32_t)BAM_OP_M : op == 0 ? (uint32_t)BAM_OP_EQ : (uint32_t)BAM_OP_X;
            const uint32_t word = ((s.c - s.s0 + 1u) << 4) | code;
            uint8_t *p = ops + 4ull * (minus ? runs - 1u - i : i);
            p[0] = (uint8_t)word; p[1] = (uint8_t)(word >> 8); p[2] = (uint8_t)(word >> 16); p[3] = (uint8_t)(word >> 24);
        }
        done += (uint32_t)__popcll(emask);
        run_start = s.next_start;
    }
}

template <class S> __device__ void bam_record(S &sink, const BrxDev &d, PafRead &R, const PafRec &q);
/* brx_sam.h's sink with the longest CIGAR a record may hold in its field (max_ops) and the nibble table of the bases (T: writing only).
   The writing sink must not grow: the compiler keeps it in LDS, where the 80 bytes per lane it has are all that fit (5120 bytes for a
   wave at eight waves per SIMD); a word more and it goes to scratch. */
template <bool WRITE, uint32_t TAGS, bool F> struct BamSink {
    static constexpr bool write = WRITE, fmtd = F, need_f0 = (TAGS & BRX_TAG_MD) != 0 || F; static constexpr uint32_t tags = TAGS;
    uint8_t *out; SamRead M; uint32_t max_ops; [[no_unique_address]] SizingWord<WRITE> surplus; uint32_t fmt; BamNib T; SaRead A;
    __device__ void record(const BrxDev &d, PafRead &R, const PafRec &q) { bam_record(*this, d, R, q); }
};
#define BRX_BAM_ZTAG 4u                /* a Z tag around its text: two letters, 'Z' and the NUL */

__device__ __forceinline__ uint32_t bam_bases_bytes(uint32_t l_seq) { return (l_seq + 1u) / 2u + l_seq; }       /* SEQ and QUAL */

/* One record of the read as a BAM record: sized (as a supplementary one; the primary's surplus goes with the best AS), or
   written.  Every lane calls it (wave-uniform arguments). */
template <class S>
__device__ void bam_record(S &sink, const BrxDev &d, PafRead &R, const PafRec &q) {
    const RecGeom g = rec_geom(sink, d, R, q);       /* with EQX the runs, and so the long form, are the =/X CIGAR's */
    const bool primary = g.primary, minus = g.minus;
    const uint32_t left = g.left, right = g.right, tspan = g.tspan;
    /* MD, cs and SA as Z tags, in this order */
    const uint32_t md_len = (S::tags & BRX_TAG_MD) ? BRX_BAM_ZTAG + g.md.text : 0u;
    const uint32_t cs_len = g.cs ? BRX_BAM_ZTAG + g.cs_text : 0u, sa_len = g.sa ? BRX_BAM_ZTAG + g.sa_text : 0u;
    const uint32_t n_ops = g.sh.runs + (left ? 1u : 0u) + (right ? 1u : 0u);
    const bool lng = n_ops > sink.max_ops;
    const uint32_t n_cigar = lng ? 2u : n_ops;
    const uint32_t comment = sam_comment(sink);
    const uint32_t bases = primary ? g.L : g.qcols;
    CountSink tc; tc.n = 0; bam_tags(tc, g.nm, g.as);
    const uint32_t seq_at = BRX_BAM_CIGAR_AT + 4u * n_cigar, qual_at = seq_at + (bases + 1u) / 2u, tag_at = qual_at + bases;
    const uint32_t cg_at = tag_at + tc.n + md_len + cs_len + sa_len + (primary ? 4u + comment : 0u);     /* CO Z comment NUL */
    const uint32_t bytes = cg_at + (lng ? 8u + 4u * n_ops : 0u);                                 /* CG B I count, the words */
    if (S::write) {
        uint8_t *o = sink.out + R.at;
        uint8_t *ops = o + (lng ? cg_at + 8u : BRX_BAM_CIGAR_AT);
        if (lane_id() == 0) {
            const uint32_t cs = (uint32_t)(q.key0 >> 32), contig = cs >> 1, p0 = (uint32_t)q.key0;
            const uint32_t ts = minus ? d.ref.d_contigs[contig].length - p0 - tspan : p0;
            const uint32_t clip = primary ? (uint32_t)BAM_OP_S : (uint32_t)BAM_OP_H;
            ByteSink h; h.p = o; h.n = 0;
            bam_fixed(h, d, R.read, bytes - 4u, contig, ts, 60u, bam_reg2bin(ts, ts + tspan), n_cigar, (minus ? 16u : 0u) | (primary ? 0u : 2048u), bases);
            if (lng) { put_le(h, (bases << 4) | BAM_OP_S, 4); put_le(h, (tspan << 4) | BAM_OP_N, 4); }
            if (left) { ByteSink c; c.p = ops; c.n = 0; put_le(c, (left << 4) | clip, 4); }
            if (right) { ByteSink c; c.p = ops + 4ull * (n_ops - 1u); c.n = 0; put_le(c, (right << 4) | clip, 4); }
            ByteSink t; t.p = o + tag_at; t.n = 0;
            bam_tags(t, g.nm, g.as);
            if (md_len) { t.put('M'); t.put('D'); t.put('Z'); t.n += g.md.text; t.put(0); }          /* the texts are the wave's, below */
            if (cs_len) { t.put('c'); t.put('s'); t.put('Z'); t.n += g.cs_text; t.put(0); }
            if (sa_len) { t.put('S'); t.put('A'); t.put('Z'); t.n += g.sa_text; t.put(0); }
            if (primary) { t.put('C'); t.put('O'); t.put('Z'); put_comment(t, d, *sink.M.s, sink.M.pieces); t.put(0); }
            if (lng) { t.put('C'); t.put('G'); t.put('B'); t.put('I'); put_le(t, n_ops, 4); }
        }
        if (md_len) md_sweep<true>(d, R, q, minus, o + tag_at + tc.n + 3u, g.md);
        if constexpr (S::fmtd) if (cs_len)
            cs_sweep<true>(d, R, q, minus, g.cs_long, sink.M.seq, o + tag_at + tc.n + md_len + 3u, g.cs_text);
        if (sa_len) sa_write(d, sink.A, g.line, R.best, o + tag_at + tc.n + md_len + cs_len + 3u);
        if (g.eqx) bam_cigar<true>(R, q, ops + (left ? 4u : 0u), g.sh.runs, minus); else bam_cigar<false>(R, q, ops + (left ? 4u : 0u), g.sh.runs, minus);
        bam_bases(sink.T, sink.M, o + seq_at, o + qual_at, primary ? 0u : g.qs, primary ? g.L : g.qe, minus);
    }
    /* the same record as the primary: SEQ and QUAL are the whole read, CO:Z:; the operations stay as many (S for H) */
    if constexpr (!S::write) if (g.top) sink.surplus = bam_bases_bytes(g.L) - bam_bases_bytes(g.qcols) + 4u + comment;
    R.at += bytes;
}

/* bytes of the unmapped record of a read of L bases: the fixed part, SEQ, QUAL, CO:Z: with the comment and its NUL */
__device__ __forceinline__ uint32_t bam_unmapped_bytes(uint32_t L, uint32_t comment) { return BRX_BAM_CIGAR_AT + bam_bases_bytes(L) + 4u + comment; }

/* bytes and primary record (BRX_SAM_UNMAPPED: none) of every read; with SA its records in the table too, as k_sam_size */
template <uint32_t TAGS, bool F>
__global__ void __launch_bounds__(64) k_bam_size(BrxDev d, const RS *rs, const PSeg *segs, const uint8_t *arena, uint32_t max_ops, uint32_t *len, uint32_t *best,
                                                  uint32_t *n_rec, uint32_t fmt) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    PafRead R; R.at = 0; R.best = 0; R.top = 0; R.n_rec = 0; R.frag = nullptr;
    BamSink<false, TAGS, F> k_; sink_init(k_, nullptr, sam_of(s, nullptr, arena), fmt); k_.max_ops = max_ops; k_.T.fwd = k_.T.rev = 0;
    if (paf_has_records(s)) paf_read(k_, d, s, r, segs, arena, R);
    truth_size_store(k_, R, r, s.rec_len ? bam_unmapped_bytes(s.seq_len, sam_comment(k_)) : 0u, BRX_BAM_ZTAG, len, best, n_rec);
}

template <uint32_t TAGS, bool F>
__global__ void __launch_bounds__(64) k_bam_write(BrxDev d, const RS *rs, const PSeg *segs, const PPiece *pieces, const uint8_t *arena, uint32_t max_ops,
                                                   const uint64_t *off, const uint32_t *best, uint8_t *out, const uint8_t *Fbuf,
                                                   const uint64_t *rec_off, const SaRec *table, uint32_t fmt) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    if (s.rec_len == 0) return;
    BamSink<true, TAGS, F> w; sink_init(w, out, sam_of(s, pieces, arena), fmt); w.max_ops = max_ops; w.T = bam_nibbles(d);
    if (best[r] != BRX_SAM_UNMAPPED) {
        PafRead R; R.at = off[r]; R.best = best[r]; R.frag = nullptr;
        if (w.need_f0) R.frag = Fbuf + s.F_off;
        if (TAGS & BRX_TAG_SA) w.A = sa_read_of(table, rec_off, r);
        paf_read(w, d, s, r, segs, arena, R);
        return;
    }
    uint8_t *o = out + off[r];
    const uint32_t L = s.seq_len, qual_at = BRX_BAM_CIGAR_AT + (L + 1u) / 2u;
    if (lane_id() == 0) {
        ByteSink h; h.p = o; h.n = 0;
        bam_fixed(h, d, d.first_read + r, bam_unmapped_bytes(L, sam_comment(w)) - 4u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, BRX_BAM_UNMAPPED_BIN, 0u, 4u, L);
        ByteSink t; t.p = o + qual_at + L; t.n = 0;
        t.put('C'); t.put('O'); t.put('Z'); put_comment(t, d, s, pieces); t.put(0);
    }
    bam_bases(w.T, w.M, o + BRX_BAM_CIGAR_AT, o + qual_at, 0u, L, false);
}

#endif /* BRX_BAM_H */
