/*
 * brx_finplan.h -- the slab planner of the final stage: which align kernel takes which read of a set, how many waves each
 * kernel gets and where their traceback slabs lie.  Host arithmetic only: no HIP call, no context, no arena -- a pure
 * function of its arguments (tests/native/finplan_check.hip calls it on synthetic read states).  The driver
 * (brx_hip.hip, Batch::launch_final_phase) derives the room, uploads the tables and launches the kernels.
 *
 * Traceback stores are SLABS owned by the persistent waves of the align kernels, not regions owned by reads: a read's
 * store is dead as soon as its path (the ops) is written, and round 2's one-region-per-read layout held ~50 GB of them
 * per 49152-read batch.  A band class walks ITS reads (a class-pure list, longest first) with one 64-bit counter whose
 * low half is the list position and whose high half counts the waves that have started: a wave's FIRST pop adds to
 * both halves in one atomic, so its ticket t is never larger than the position i0 it popped, and everything it will
 * ever pop comes after i0.  Slab t is therefore sized max(units of list[t..]) -- the suffix maximum -- and the set
 * needs the sum of the first W suffix maxima (W = waves of the class) instead of the sum over all its reads
 * (measured model, configs[3]: 51.7 -> 19 GB per batch at 4096 / 1024 / 256 / 64 waves).  A set that does not fit
 * halves the waves of a class until it does; only when ONE wave per class does not fit is the arena short.
 * (Rounds 1-5 kept col_of[] -- 4 bytes per read base for k_fin_qscore -- per read in front of the slabs; round 6 scores by column.)
 */
#ifndef BRX_FINPLAN_H
#define BRX_FINPLAN_H

#include <algorithm>
#include <utility>
#include <vector>

#include "brx_kernels.h"

/* A wave's slab holds the largest store it can meet: wave w of a class the w-th largest.  The widest class of a batch at
   --identity 85,95,5 --chimeras 25 holds a few reads whose store is GBs (a 300 kb chimera at 75 %: the memory-resident path
   keeps every cell) beside thousands of 10 MB: with the giants at the head of the class's queue, W waves needed the W largest
   stores, the set's share held two or three of them, and 400 Mbases of a batch ran on two or three waves -- 46.6 s of a 48 s
   batch.  The giants are a class of their own (same kernel, own queue, own few slabs); the others keep their 256 waves. */
#ifndef BRX_GIANT_UNITS
#define BRX_GIANT_UNITS ((uint64_t)64 << 17)       /* 64 MB in 8-byte units, above any windowed store of configs[3] (58 MB: 150 kb at 87 %); a test build sets it low */
#endif

/* The classes of a set, in the order of its list and slab tables.  FC_LANES counts its slabs per GROUP of 64 reads, FC_QUAD
   per group of 4; FC_GIANT: the reads of FC_WIDE whose store is above the giant threshold. */
enum FinClass {
    FC_W1 = 0, FC_W2, FC_W4,       /* k_fin_align<1,1,1>, <2,2,2>, <4,4,4>: one, two, four band words per lane */
    FC_WIDE,                       /* k_fin_align<16,8,0xFFFF>: eight words and more */
    FC_LANES,                      /* k_fin_lanes: narrow band, one read per lane */
    FC_QUAD,                       /* k_fin_quad<1>: one-word bands of up to 13 superblocks, four reads per wave */
    FC_GIANT,
    FC_COUNT
};

struct FinPlanCfg {
    uint32_t n_cu, waves_per_cu;
    int tb_hmul;                   /* window of the phase-0 store (BrxDev.tb_hmul) */
    bool use_lanes, use_quad;      /* the set's reads flagged BRX_KL_LANES / BRX_KL_QUAD take those kernels (phase 0 only) */
    uint64_t giant_units;          /* BRX_GIANT_UNITS */
};

struct FinPlan {
    std::vector<uint32_t> lists;   /* the class lists, concatenated: class k at list_at[k], cnt[k] reads, largest store first */
    std::vector<uint64_t> slabs;   /* slab offsets in 8-byte units: class k at slab_at[k], grid[k] + 1 entries (the last: its end) */
    uint32_t list_at[FC_COUNT], slab_at[FC_COUNT], cnt[FC_COUNT], grid[FC_COUNT];
    uint64_t need;                 /* bytes of the slabs (and 4 KB of slack) */
    bool fits;                     /* false: not even at one wave per class */
};

/* The plan of one phase of one set (phase 0: windowed store for every read; phase 1: full store for the misses): rs / order are
   the host copies of the read states and the processing order, [b, e) the set's range of `order`.  left: bytes the set may take
   (its share); room_now: bytes the arena holds right now. */
inline FinPlan brx_plan_final(const RS *rs, const uint32_t *order, uint32_t b, uint32_t e, int phase, const FinPlanCfg &cfg, size_t left, size_t room_now) {
    typedef std::pair<uint64_t, uint32_t> Ent;        /* what the class's list is sorted by, the read */
    std::vector<Ent> ent[FC_COUNT];
    auto quad_geom = [&](const RS &r) { return brx_make_geom_quad((int)r.m, (int)r.n, (int)r.ub, (r.klass & BRX_KL_FULL) ? 0 : cfg.tb_hmul); };
    for (uint32_t i = b; i < e; ++i) {
        const RS &r = rs[order[i]];
        if (!r.n) continue;
        if (phase == 1 && !(r.klass & BRX_KL_RETRY)) continue;
        bool too_wide = false;
        const uint64_t u = (phase == 1 ? brx_final_units(r.m, r.n, r.ub, 0, &too_wide) : r.units) - (((uint64_t)r.m * 4 + 7) / 8 + 2);     /* the aligner's share: without the raw columns */
        const uint64_t store = (u + 31) & ~31ull;
        const uint32_t kl = r.klass & 0xFFFFu;
        /* by lane: no windowed store: a repeat means the lane aligner failed; k_fin_align takes the read then (the flag is cleared).
           Sorted by fragment length; units per group follow.  Four per wave: a miss is repeated by k_fin_align (k_fin_quad clears
           the flag); sorted by the read's own store. */
        if ((r.klass & BRX_KL_LANES) && phase == 0 && cfg.use_lanes) ent[FC_LANES].push_back({((uint64_t)r.n << 8) | (uint64_t)brx_finl_blocks(r.m, r.n, r.ub), order[i]});
        else if ((r.klass & BRX_KL_QUAD) && phase == 0 && cfg.use_quad) ent[FC_QUAD].push_back({brx_align_units(quad_geom(r)), order[i]});
        else ent[kl <= 1 ? FC_W1 : kl == 2 ? FC_W2 : kl == 4 ? FC_W4 : store > cfg.giant_units ? FC_GIANT : FC_WIDE].push_back({store, order[i]});
    }
    /* A class's list is walked by STORE SIZE, largest first (a store grows with length x band width, and so does the work: the
       order is also longest-processing-time first), so the suffix maximum at position t is the t-th largest store and W waves
       hold the W largest stores of the class. */
    for (std::vector<Ent> &v : ent) std::stable_sort(v.begin(), v.end(), [](const Ent &x, const Ent &y) { return x.first > y.first; });
    std::vector<uint64_t> units[FC_COUNT];            /* the store of each entry the class's waves pop: a read, or a group of reads */
    for (int k = 0; k < FC_COUNT; ++k) if (k != FC_LANES && k != FC_QUAD) for (const Ent &x : ent[k]) units[k].push_back(x.first);
    /* groups of 64 reads, longest fragment first: the longest fragment of the group (its first) x the widest band in it */
    for (size_t g = 0, n = ent[FC_LANES].size(); g * 64 < n; ++g) {
        uint32_t blocks = 0;
        for (size_t x = g * 64; x < std::min(n, g * 64 + 64); ++x) blocks = std::max<uint32_t>(blocks, (uint32_t)(ent[FC_LANES][x].first & 0xFFu));
        units[FC_LANES].push_back((brx_finl_units((uint32_t)(ent[FC_LANES][g * 64].first >> 8), blocks) + 31) & ~31ull);
    }
    /* groups of four reads: rows for the longest of them, slots for the widest window */
    for (size_t g = 0, n = ent[FC_QUAD].size(); g * 4 < n; ++g) {
        BrxGeom g4[4]; int n4 = 0;
        for (size_t x = g * 4; x < std::min(n, g * 4 + 4); ++x) g4[n4++] = quad_geom(rs[ent[FC_QUAD][x].second]);
        units[FC_QUAD].push_back((brx_quad_units(g4, n4) + 31) & ~31ull);
    }

    FinPlan P;
    /* waves per class: what the chip can hold of each kernel beside the other batches' work (96 / 129 / 155 / 256 VGPRs: 5 / 3 / 3 /
       1-2 waves per SIMD) -- more waves than that only add slabs */
    const uint32_t limit_div[FC_COUNT] = {2, 4, 8, 16, 4, 4, 1};       /* of waves_per_cu, per CU (the giants: not used, 16 waves in all) */
    uint32_t grid_full[FC_COUNT];
    std::vector<uint64_t> slab_sum[FC_COUNT];         /* slab_sum[k][w]: units of the class's first w slabs (sums of suffix maxima) */
    double work[FC_COUNT] = {};                       /* a class's work: the sum of its stores (length x band) */
    for (int k = 0; k < FC_COUNT; ++k) {
        const size_t n = units[k].size();
        const uint32_t limit = k == FC_GIANT ? 16u : cfg.n_cu * std::max(cfg.waves_per_cu / limit_div[k], 1u);
        std::vector<uint64_t> sufmax(n + 1, 0);
        for (size_t x = n; x-- > 0;) sufmax[x] = std::max(sufmax[x + 1], units[k][x]);
        slab_sum[k].assign(n + 1, 0);
        for (size_t w = 0; w < n; ++w) { slab_sum[k][w + 1] = slab_sum[k][w] + sufmax[w]; work[k] += (double)units[k][w]; }
        P.cnt[k] = (uint32_t)ent[k].size();
        P.grid[k] = grid_full[k] = (uint32_t)std::min<size_t>(n, limit);
    }
    auto need = [&]() { uint64_t t = 512; for (int k = 0; k < FC_COUNT; ++k) t += slab_sum[k][P.grid[k]]; return t * 8; };
    /* A set that does not fit halves the waves of the class where that frees the most room for the least time.  A class's time is its
       work over its waves, and halving the waves adds that much; what it frees is the slabs of the upper half of its queue
       positions.  (Until round 6 the FATTEST class was halved: on a batch of --identity 85,95,5 the four-word class -- 14 717
       reads -- went down to 32 slabs while 21 488 short reads kept 2048 that held 0.2 MB each.) */
    for (int guard = 0; need() > left && guard < 128; ++guard) {
        int pick = -1; double best = -1.0;
        for (int k = 0; k < FC_COUNT; ++k) {
            if (P.grid[k] <= 1) continue;
            const uint64_t freed = slab_sum[k][P.grid[k]] - slab_sum[k][(P.grid[k] + 1) / 2];
            const double score = (double)freed / (work[k] / (double)P.grid[k] + 1.0);
            if (score > best) { best = score; pick = k; }
        }
        if (pick < 0) break;
        P.grid[pick] = (P.grid[pick] + 1) / 2;
    }
    /* ... and halving is coarse: give back what fits, to the class whose waves carry the most work each */
    for (int guard = 0; guard < 64; ++guard) {
        int pick = -1; double best = -1.0;
        for (int k = 0; k < FC_COUNT; ++k) {
            if (P.grid[k] >= grid_full[k]) continue;
            const uint32_t was = P.grid[k];
            P.grid[k] = std::min<uint32_t>(grid_full[k], was * 2u);
            const bool fits = need() <= left;
            P.grid[k] = was;
            const double load = work[k] / (double)was;
            if (fits && load > best) { best = load; pick = k; }
        }
        if (pick < 0) break;
        P.grid[pick] = std::min<uint32_t>(grid_full[pick], P.grid[pick] * 2u);
    }
    P.need = need();
    /* one wave per class and still more than the set's share: the share is a courtesy to the sets to come (they halve their own
       grids), the room is what counts -- a head set of --identity 85,95,5 --chimeras 25 holds reads whose store alone is GBs (a
       300 kb chimera at 75 %: the memory-resident wide path keeps every cell) */
    P.fits = P.need <= left || P.need <= room_now;
    uint64_t run = 0;
    for (int k = 0; k < FC_COUNT; ++k) {
        P.list_at[k] = (uint32_t)P.lists.size(); P.slab_at[k] = (uint32_t)P.slabs.size();
        for (const Ent &x : ent[k]) P.lists.push_back(x.second);
        for (uint32_t w = 0; w <= P.grid[k]; ++w) P.slabs.push_back(run + slab_sum[k][w]);      /* the last: end of the class's last slab */
        run += slab_sum[k][P.grid[k]];
    }
    return P;
}

#endif
