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
 * primary (SamCount.surplus); it reads no SEQ or QUAL byte.  k_sam_write knows the primary from the sizing pass.  One wave per
 * read; lane 0 writes the fixed fields, the wave places the CIGAR runs and copies SEQ and QUAL 64 bytes per step (contiguous
 * stores; on '-' lines the loads run backwards).
 */
#ifndef BRX_SAM_H
#define BRX_SAM_H

#define BRX_SAM_UNMAPPED (~0u)         /* best[r] of a read whose one line is the unmapped one */
#define BRX_SAM_NAME 36u               /* characters of a read name (put_uuid) */
#define BRX_SAM_MATE "\t*\t0\t0\t"                       /* RNEXT PNEXT TLEN, between CIGAR and SEQ */
#define BRX_SAM_NOMAP "\t4\t*\t0\t0\t*\t*\t0\t0\t"      /* FLAG .. TLEN of an unmapped line */
#define BRX_SAM_CO "\tCO:Z:"
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

template <class S> __device__ void sam_record(S &sink, const BrxDev &d, PafRead &R, const PafRec &q);
struct SamCount {
    static constexpr bool write = false; uint8_t *out; SamRead M; uint32_t surplus;
    __device__ void record(const BrxDev &d, PafRead &R, const PafRec &q) { sam_record(*this, d, R, q); }
};
struct SamWrite {
    static constexpr bool write = true; uint8_t *out; SamRead M;
    __device__ void record(const BrxDev &d, PafRead &R, const PafRec &q) { sam_record(*this, d, R, q); }
};
/* the comment's length: the FASTQ header is '@', the name, a blank, the comment and a newline (RS.hdr_len, k_recsize) */
template <class S> __device__ __forceinline__ uint32_t sam_comment(const S &sink) { return sink.M.s->hdr_len - (BRX_SAM_NAME + 3u); }
__device__ __forceinline__ void sink_surplus(SamCount &k, uint32_t v) { k.surplus = v; }
__device__ __forceinline__ void sink_surplus(SamWrite &, uint32_t) {}


/* One record of the read as a SAM line: sized (as a supplementary line; the primary's surplus goes with the best AS), or
   written.  Every lane calls it (wave-uniform arguments). */
template <class S>
__device__ void sam_record(S &sink, const BrxDev &d, PafRead &R, const PafRec &q) {
    const PafShape sh = paf_shape(R, q);
    const uint32_t nm = sh.cnt[1] + sh.cnt[2] + sh.cnt[3];
    const int64_t as = (int64_t)sh.cnt[0] - (int64_t)nm;
    const uint32_t qcols = sh.cnt[0] + sh.cnt[1] + sh.cnt[2], tspan = sh.cnt[0] + sh.cnt[1] + sh.cnt[3];
    const bool minus = ((q.key0 >> 32) & 1u) != 0;
    const uint32_t L = R.seq_len, qs = q.r0 - R.start_trim, qe = qs + qcols;
    const uint32_t left = minus ? L - qe : qs, right = minus ? qs : L - qe;
    const bool primary = S::write && R.n_rec == R.best;
    const bool top = paf_rank(R, as);
    CountSink hc; hc.n = 0;
    sam_head(hc, d, R, q, tspan, primary);
    CountSink lc; lc.n = 0; sam_clip(lc, left, primary);
    CountSink rc; rc.n = 0; sam_clip(rc, right, primary);
    CountSink tc; tc.n = 0; paf_tags(tc, nm, as);
    const uint32_t comment = sam_comment(sink);
    const uint32_t bases = primary ? L : qcols;
    const uint32_t cig_at = hc.n + lc.n, seq_at = cig_at + sh.text + rc.n + BRX_SAM_LEN(BRX_SAM_MATE), tag_at = seq_at + 2u * bases + 1u;
    const uint32_t bytes = tag_at + tc.n + (primary ? BRX_SAM_LEN(BRX_SAM_CO) + comment : 0u) + 1u;
    if (S::write) {
        uint8_t *o = sink.out + R.at;
        if (lane_id() == 0) {
            ByteSink h; h.p = o; h.n = 0;
            sam_head(h, d, R, q, tspan, primary); sam_clip(h, left, primary);
            ByteSink m; m.p = o + cig_at + sh.text; m.n = 0;
            sam_clip(m, right, primary); put_str(m, BRX_SAM_MATE);
            ByteSink t; t.p = o + tag_at; t.n = 0;
            paf_tags(t, nm, as);
            if (primary) { put_str(t, BRX_SAM_CO); put_comment(t, d, *sink.M.s, sink.M.pieces); }
            t.put('\n');
        }
        paf_cigar(R, q, o + cig_at, sh.text, minus);
        sam_bases(d, sink.M, o + seq_at, primary ? 0u : qs, primary ? L : qe, minus);
    } else if (top) {
        /* the same record as the primary: FLAG loses its 2048 (4 digits -> "0" or "16"), SEQ and QUAL are the whole read, CO:Z: */
        sink_surplus(sink, 2u * (L - qcols) + BRX_SAM_LEN(BRX_SAM_CO) + comment - (minus ? 2u : 3u));
    }
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

/* bytes and primary record (BRX_SAM_UNMAPPED: none) of every read */
__global__ void __launch_bounds__(64) k_sam_size(BrxDev d, const RS *rs, const PSeg *segs, const uint8_t *arena, uint32_t *len, uint32_t *best) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    PafRead R; R.at = 0; R.best = 0; R.top = 0; R.n_rec = 0;
    SamCount k_; k_.out = nullptr; k_.surplus = 0; k_.M = sam_of(s, nullptr, arena);
    if (paf_has_records(s)) paf_read(k_, d, s, r, segs, arena, R);
    uint32_t bytes = (uint32_t)R.at + k_.surplus, top = R.top;
    if (R.n_rec == 0) { top = BRX_SAM_UNMAPPED; bytes = s.rec_len ? sam_unmapped_bytes(s.seq_len, sam_comment(k_)) : 0u; }
    if (lane_id() == 0) { len[r] = bytes; best[r] = top; }
}

/* read offsets: off[r] (n_reads + 1 entries, the last = total bytes); the running sums are 64 bits throughout */
__global__ void __launch_bounds__(64) k_sam_scan(uint32_t n_reads, const uint32_t *len, uint64_t *off) {
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

__global__ void __launch_bounds__(64) k_sam_write(BrxDev d, const RS *rs, const PSeg *segs, const PPiece *pieces, const uint8_t *arena,
                                                   const uint64_t *off, const uint32_t *best, uint8_t *out) {
    const uint32_t r = blockIdx.x;
    const RS s = rs[r];
    if (s.rec_len == 0) return;
    SamWrite w; w.out = out; w.M = sam_of(s, pieces, arena);
    if (best[r] != BRX_SAM_UNMAPPED) {
        PafRead R; R.at = off[r]; R.best = best[r];
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
