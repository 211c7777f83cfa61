/*
 * Host-side check of the final stage's slab planner (badread_amd/csrc/brx_finplan.h: brx_plan_final is a pure host function):
 * compiled with hipcc, run on the CPU by tests/test_finplan_host.py.  Synthetic read states -- a few hundred sets of 1..300
 * reads from seeded lengths, edit bounds and flags, classified as k_fin_join classifies them -- are planned for phase 0 and
 * phase 1 with ample, tight and insufficient room, and every plan is verified:
 *   1. every read the phase aligns is in exactly one list, the list of its class, and nothing else is;
 *   2. a list is ordered by what its class is sorted by, largest first;
 *   3. slab w of a class holds the store of every entry (read, or group of 64 / 4 reads) at list position >= w -- a wave's
 *      ticket is never beyond the position it pops, so this keeps every traceback inside its slab;
 *   4. slab offsets ascend, classes do not overlap, all ends within the bytes reported; a plan that fits is within the room;
 *   5. 1 <= grid <= min(entries, limit) for a class with entries (with ample room: equal), 0 for one without;
 *   6. insufficient room: the plan says so and reports more than the room.
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../badread_amd/csrc/brx_finplan.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((rng_state >> 33) % n); }

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

/* the read state as k_fin_join leaves it */
static RS make_read(uint32_t m, uint32_t n, uint32_t ub, bool junk, bool acgt, bool fin_lanes, bool fin_quad, int hmul) {
    RS r = {};
    r.m = m; r.n = n; r.ub = ub;
    if (!n) return r;
    const BrxGeom g = brx_make_geom((int)m, (int)n, (int)ub);
    const bool lanes = fin_lanes && !junk && acgt && brx_finl_blocks(m, n, ub) > 0;
    const bool quad = fin_quad && !lanes && acgt && g.G == 1 && (brx_quad_words(m, n, ub) & 1) != 0;
    bool too_wide;
    r.klass = (g.G ? (uint32_t)g.G : 0xFFFFu) | (junk ? BRX_KL_FULL : 0u) | (lanes ? BRX_KL_LANES : 0u) | (quad ? BRX_KL_QUAD : 0u);
    r.units = brx_final_units(m, n, ub, junk ? 0 : hmul, &too_wide);
    return r;
}
static RS random_read(int hmul, bool fin_lanes, bool fin_quad) {
    static const uint32_t lens[] = {0, 1, 33, 300, 1000, 3000, 3000, 8000, 20000, 60000};
    static const uint32_t rates[] = {0, 1, 1, 4, 8, 15, 30, 60};
    const uint32_t len = lens[rnd(10)], n = len ? len + rnd(17) : 0;
    if (!n) return make_read(0, 0, 0, false, true, fin_lanes, fin_quad, hmul);
    const uint32_t m = std::max<uint32_t>(1u, (uint32_t)((double)n * (0.95 + 0.1 * (rnd(1000) / 1000.0))));
    const uint32_t ub = (m > n ? m - n : n - m) + (uint32_t)((uint64_t)n * rates[rnd(8)] / 100);
    return make_read(m, n, ub, rnd(16) == 0, rnd(8) != 0, fin_lanes, fin_quad, hmul);
}

static int class_of(const RS &r, int phase, const FinPlanCfg &cfg, uint64_t store) {
    const uint32_t kl = r.klass & 0xFFFFu;
    if (phase == 0 && (r.klass & BRX_KL_LANES) && cfg.use_lanes) return FC_LANES;
    if (phase == 0 && (r.klass & BRX_KL_QUAD) && cfg.use_quad) return FC_QUAD;
    return kl <= 1 ? FC_W1 : kl == 2 ? FC_W2 : kl == 4 ? FC_W4 : store > cfg.giant_units ? FC_GIANT : FC_WIDE;
}
/* the store k_fin_align needs for the read in this phase, as the slabs count it (32-unit steps) */
static uint64_t wave_store(const RS &r, int phase) {
    bool tw;
    const uint64_t all = phase == 1 ? brx_final_units(r.m, r.n, r.ub, 0, &tw) : r.units;
    return ((all - (((uint64_t)r.m * 4 + 7) / 8 + 2)) + 31) & ~31ull;
}
static BrxGeom quad_geom(const RS &r, const FinPlanCfg &cfg) { return brx_make_geom_quad((int)r.m, (int)r.n, (int)r.ub, (r.klass & BRX_KL_FULL) ? 0 : cfg.tb_hmul); }

static uint32_t seen_class[FC_COUNT], seen_group[2][3];      /* coverage: reads per class; by-lane groups of 1 / 64 / 65, quad groups of 1 / 4 / 5 reads */

static int check_plan(const std::vector<RS> &rs, const std::vector<uint32_t> &order, uint32_t b, uint32_t e, int phase, const FinPlanCfg &cfg,
                      const FinPlan &P, size_t left, size_t room_now, bool ample) {
    /* waves per class, restated: a half, a quarter, an eighth, a sixteenth of the chip's waves (at least one per CU); 16 for the giants */
    const uint32_t wpc = cfg.waves_per_cu;
    uint32_t limit[FC_COUNT];
    limit[FC_W1] = cfg.n_cu * std::max(wpc / 2u, 1u);
    limit[FC_W2] = limit[FC_LANES] = limit[FC_QUAD] = cfg.n_cu * std::max(wpc / 4u, 1u);
    limit[FC_W4] = cfg.n_cu * std::max(wpc / 8u, 1u);
    limit[FC_WIDE] = cfg.n_cu * std::max(wpc / 16u, 1u);
    limit[FC_GIANT] = 16u;
    std::vector<int> hits(rs.size(), 0);
    uint32_t lists_run = 0, slabs_run = 0;
    uint64_t prev_end = 0;
    for (int k = 0; k < FC_COUNT; ++k) {
        if (P.list_at[k] != lists_run || P.slab_at[k] != slabs_run) FAIL("class %d: tables not concatenated in class order", k);
        lists_run += P.cnt[k]; slabs_run += P.grid[k] + 1;
        if (lists_run > P.lists.size() || slabs_run > P.slabs.size()) FAIL("class %d: tables shorter than their index", k);
        const uint32_t *l = P.lists.data() + P.list_at[k];
        /* 1. membership, 2. order */
        std::vector<uint64_t> key(P.cnt[k]);
        for (uint32_t x = 0; x < P.cnt[k]; ++x) {
            if (l[x] >= rs.size()) FAIL("class %d: read index out of range", k);
            const RS &r = rs[l[x]];
            hits[l[x]] += 1;
            if (class_of(r, phase, cfg, wave_store(r, phase)) != k) FAIL("read %u in class %d, belongs to %d", l[x], k, class_of(r, phase, cfg, wave_store(r, phase)));
            key[x] = k == FC_LANES ? r.n : k == FC_QUAD ? brx_align_units(quad_geom(r, cfg)) : wave_store(r, phase);
            if (x && key[x] > key[x - 1]) FAIL("class %d: list not ordered, position %u", k, x);
        }
        seen_class[k] += P.cnt[k];
        /* the store of every entry the class's waves pop */
        const uint32_t per = k == FC_LANES ? 64u : k == FC_QUAD ? 4u : 1u;
        std::vector<uint64_t> store((P.cnt[k] + per - 1) / per);
        for (size_t g = 0; g < store.size(); ++g) {
            const uint32_t g0 = (uint32_t)g * per, g1 = std::min(P.cnt[k], g0 + per);
            if (k == FC_LANES) {
                uint32_t t_max = 0, blocks = 0;
                for (uint32_t x = g0; x < g1; ++x) { t_max = std::max(t_max, rs[l[x]].n); blocks = std::max<uint32_t>(blocks, (uint32_t)brx_finl_blocks(rs[l[x]].m, rs[l[x]].n, rs[l[x]].ub)); }
                store[g] = brx_finl_units(t_max, blocks);
            } else if (k == FC_QUAD) {
                BrxGeom g4[4];
                for (uint32_t x = g0; x < g1; ++x) g4[x - g0] = quad_geom(rs[l[x]], cfg);
                store[g] = brx_quad_units(g4, (int)(g1 - g0));
            } else store[g] = key[g];
        }
        if (per > 1) for (int x = 0; x < 3; ++x) seen_group[k == FC_QUAD][x] += P.cnt[k] == (x == 0 ? 1u : x == 1 ? per : per + 1u);
        /* 5. grid */
        const uint32_t full = (uint32_t)std::min<size_t>(store.size(), limit[k]);
        if (store.empty() ? P.grid[k] != 0 : (P.grid[k] < 1 || P.grid[k] > full)) FAIL("class %d: grid %u with %zu entries, limit %u", k, P.grid[k], store.size(), limit[k]);
        if (ample && P.grid[k] != full) FAIL("class %d: grid %u with ample room, expected %u", k, P.grid[k], full);
        /* 3. slab w >= every store at position >= w; 4. offsets */
        const uint64_t *s = P.slabs.data() + P.slab_at[k];
        if (s[0] < prev_end) FAIL("class %d: slabs overlap the class before", k);
        uint64_t sufmax = 0;
        for (size_t x = store.size(); x-- > P.grid[k];) sufmax = std::max(sufmax, store[x]);
        for (uint32_t w = P.grid[k]; w-- > 0;) {
            sufmax = std::max(sufmax, store[w]);
            if (s[w + 1] < s[w]) FAIL("class %d: slab offsets descend at %u", k, w);
            if (s[w + 1] - s[w] < sufmax) FAIL("class %d: slab %u holds %llu units, an entry behind it needs %llu", k, w, (unsigned long long)(s[w + 1] - s[w]), (unsigned long long)sufmax);
        }
        prev_end = s[P.grid[k]];
    }
    if (lists_run != P.lists.size() || slabs_run != P.slabs.size()) FAIL("tables longer than their index");
    if (P.lists.size() > (size_t)(e - b) || P.slabs.size() > (size_t)(e - b) + 8) FAIL("tables larger than the driver's staging area");
    for (uint32_t i = b; i < e; ++i) {
        const RS &r = rs[order[i]];
        const int want = (r.n && (phase == 0 || (r.klass & BRX_KL_RETRY))) ? 1 : 0;
        if (hits[order[i]] != want) FAIL("read %u listed %d times, expected %d (phase %d)", order[i], hits[order[i]], want, phase);
        hits[order[i]] = 0;
    }
    for (int h : hits) if (h) FAIL("a read outside the set is listed");
    if (prev_end * 8 > P.need) FAIL("slabs end at %llu bytes, need says %llu", (unsigned long long)prev_end * 8, (unsigned long long)P.need);
    if (P.fits && P.need > std::max(left, room_now)) FAIL("fits, but needs %llu of %zu", (unsigned long long)P.need, std::max(left, room_now));
    if (!P.fits && P.need <= std::max(left, room_now)) FAIL("does not fit, but needs %llu of %zu", (unsigned long long)P.need, std::max(left, room_now));
    return 0;
}

static int plans = 0;
/* phase 0 and phase 1 of one set (the whole of rs, in a shuffled order), each with ample, tight and insufficient room */
static int check_set(std::vector<RS> rs, FinPlanCfg cfg) {
    const uint32_t n = (uint32_t)rs.size();
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    for (uint32_t i = n; i > 1; --i) std::swap(order[i - 1], order[rnd(i)]);
    const uint32_t b = rnd(2) ? 0 : rnd(n), e = n;                 /* a head set starts at 0, a bulk set behind it */
    for (int phase = 0; phase < 2; ++phase) {
        if (phase == 1) for (RS &r : rs) if (r.n && rnd(3) == 0) r.klass = (r.klass | BRX_KL_RETRY) & ~(BRX_KL_LANES | BRX_KL_QUAD);      /* the kernels clear the route of a miss */
        const size_t ample = (size_t)1 << 46;
        const FinPlan full = brx_plan_final(rs.data(), order.data(), b, e, phase, cfg, ample, ample);
        if (!full.fits || check_plan(rs, order, b, e, phase, cfg, full, ample, ample, true)) FAIL("... ample room, phase %d, %u reads", phase, n);
        const FinPlan least = brx_plan_final(rs.data(), order.data(), b, e, phase, cfg, 0, 0);       /* one wave per class */
        if (least.fits || check_plan(rs, order, b, e, phase, cfg, least, 0, 0, false)) FAIL("... no room, phase %d, %u reads", phase, n);
        for (int k = 0; k < FC_COUNT; ++k) if (least.grid[k] > 1) FAIL("no room: class %d keeps %u waves", k, least.grid[k]);
        if (least.need > full.need) FAIL("one wave per class needs more than full grids");
        for (int t = 0; t < 4; ++t) {                              /* tight: between the two, the share (left) at or below the room */
            const size_t room = (size_t)least.need + (size_t)((full.need - least.need) * (uint64_t)rnd(1001) / 1000);
            const size_t left = t == 3 ? room / 2 : room;         /* t == 3: more than the share, within the room */
            const FinPlan P = brx_plan_final(rs.data(), order.data(), b, e, phase, cfg, left, room);
            if (!P.fits || P.need > room || check_plan(rs, order, b, e, phase, cfg, P, left, room, false)) FAIL("... tight room %zu of %llu..%llu, phase %d, %u reads", room, (unsigned long long)least.need, (unsigned long long)full.need, phase, n);
            ++plans;
        }
        const size_t shortr = (size_t)least.need - 8;              /* insufficient */
        const FinPlan S = brx_plan_final(rs.data(), order.data(), b, e, phase, cfg, shortr, shortr);
        if (S.fits || S.need <= shortr || check_plan(rs, order, b, e, phase, cfg, S, shortr, shortr, false)) FAIL("... insufficient room, phase %d, %u reads", phase, n);
        plans += 3;
    }
    return 0;
}

int main() {
    static const uint32_t chips[][2] = {{256, 16}, {4, 16}, {8, 4}, {1, 1}};       /* n_cu, waves per CU: limits above, among and below the entries */
    static const int hm[] = {2, 2, 2, 0, -1};
    for (int it = 0; it < 300; ++it) {
        const uint32_t *chip = chips[rnd(4)];
        FinPlanCfg cfg = {chip[0], chip[1], hm[rnd(5)], rnd(4) != 0, rnd(4) != 0, (uint64_t)BRX_GIANT_UNITS};
        const bool fin_lanes = rnd(8) != 0, fin_quad = rnd(8) != 0;
        std::vector<RS> rs(1 + rnd(300));
        for (RS &r : rs) r = random_read(cfg.tb_hmul, fin_lanes, fin_quad);
        if (check_set(rs, cfg)) return 1;
    }
    /* by-lane groups of 1, 64 and 65 reads, quad groups of 1, 4 and 5, beside a few reads of the other classes and a giant */
    static const uint32_t sizes[2][3] = {{1, 64, 65}, {1, 4, 5}};
    static const uint32_t wide_ub[3] = {2500, 5000, 9000};         /* two, four and eight band words per lane at 20 kb */
    for (int row = 0; row < 2; ++row) for (int x = 0; x < 3; ++x) {
        FinPlanCfg cfg = {4, 16, 2, true, true, (uint64_t)BRX_GIANT_UNITS};
        std::vector<RS> rs;
        for (uint32_t i = 0; i < sizes[row][x]; ++i) { const uint32_t n = 2000 + rnd(2000); rs.push_back(make_read(n + rnd(9), n, row ? 150 + rnd(200) : 8 + rnd(40), false, true, true, true, 2)); }
        for (int i = 0; i < 6; ++i) rs.push_back(make_read(20000 + rnd(50), 20000, wide_ub[i % 3], false, true, true, true, 2));
        rs.push_back(make_read(60100, 60000, 18000, false, true, true, true, 2));
        const FinPlan P = brx_plan_final(rs.data(), std::vector<uint32_t>(rs.size(), 0).data(), 0, 0, 0, cfg, 0, 0);
        if (!P.lists.empty() || P.slabs.size() != FC_COUNT) FAIL("an empty range is not an empty plan");
        if (check_set(rs, cfg)) return 1;
    }
    for (int k = 0; k < FC_COUNT; ++k) if (!seen_class[k]) FAIL("class %d never occurred", k);
    for (int row = 0; row < 2; ++row) for (int x = 0; x < 3; ++x) if (!seen_group[row][x]) FAIL("no %s class of %u reads", row ? "four-per-wave" : "by-lane", sizes[row][x]);
    printf("ok %d plans, reads per class %u/%u/%u/%u + %u by lane + %u four per wave + %u giant\n", plans, seen_class[FC_W1], seen_class[FC_W2], seen_class[FC_W4],
           seen_class[FC_WIDE], seen_class[FC_LANES], seen_class[FC_QUAD], seen_class[FC_GIANT]);
    return 0;
}
