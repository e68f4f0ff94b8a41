// Stand-alone check of the host planner of a pair-forward call (align3r_amd/csrc/dedup.h: plan_call and the CallLists it fills):
// the grouping of the slots, the frame cache's and the stored priors' tables, the head products' bits and every list the plan
// then reads, together, against a content model.  Every slot of a call is given an image id and a prior id; the model keeps what
// each entry of each store holds (an id, and per side the id whose r0 / c blocks lie there -- never cleared, so stale content
// stays), applies the stores the lists order, and then every slot must find its own content through the lists: the frame rows,
// the prior's src, src_ent of every block-0 entry, the head's src per side.  No index may leave its range and the counts must
// equal those recomputed naively.  Random sequences with B = 1 .. 4, all-equal and all-distinct batches, capacities from 1,
// flushes, each store absent in turn, decode calls, and the named cases below.  Built with -fsanitize=address,undefined by
// tests/test_call_plan_cpu.py; prints "ok".
#include "dedup.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <utility>
#include <vector>

using namespace a3r;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);        \
            return 1;                                                  \
        }                                                              \
    } while (0)

namespace {

struct Config { int E, D, F, l0, H, W; };

// the handle's tables, the "device" content of the three storages, and the naive model of the head products' bits
struct World {
    int cap;
    FrameCacheTable fc, pd;
    HeadBits bits;
    std::vector<int> fc_held, pd_held;         // the id entry e holds (stale after a flush: the table then says the entry is free)
    std::vector<int> hp_rows[2];               // the image id whose r0 / c lie in (entry, side)
    std::vector<char> naive[2];                // (entry, side) holds the product of the frame the entry holds
    explicit World(int cap_) : cap(cap_), fc_held(cap_, -1), pd_held(cap_, -1) {
        fc.reset(cap);
        pd.reset(cap);
        for (int s = 0; s < 2; s++) { hp_rows[s].assign(cap, -1); naive[s].assign(cap, 0); }
    }
    void flush() {                             // a3r_model_s::drop_stored
        fc.flush();
        pd.flush();
        bits.flush();
        for (int s = 0; s < 2; s++) std::fill(naive[s].begin(), naive[s].end(), 0);
    }
};

struct CallSpec {
    int B;
    std::vector<int> img, pdid;                // [2 B] ids
    bool encode = true, first_kind = true, dedup_head = true, dedup_decoder = true, gemm_fh2 = true, map_fh2 = true, attn_maps = true;
    bool with_fc = true, with_pd = true, with_hp = true;
};

struct Seen { long hits = 0, unstored = 0, evictions = 0, head_hits = 0, head_fresh = 0, entries = 0, both_sides = 0, plain = 0, no_fit = 0; };

int distinct(const std::vector<int>& v, int lo, int hi) { return (int)std::set<int>(v.begin() + lo, v.begin() + hi).size(); }
// the entry of the table that holds `id`, as the lookup kernel answers: valid entries only
int lookup(const FrameCacheTable& t, const std::vector<int>& held, int id) {
    for (int e = 0; e < t.cap; e++)
        if (t.stamp[e] && held[e] == id) return e;
    return -1;
}

// One call: plans it, applies its stores to the world, checks everything.  Returns 0, or the line of the failed check.
#define REQUIRE(c)                 \
    do {                           \
        if (!(c)) return __LINE__; \
    } while (0)
int run_call(World& w, const Config& g, const CallSpec& k, CallLists& L, Seen& seen, CallPlan* out = nullptr) {
    const int B = k.B, S = 2 * B, N = (g.H / 16) * (g.W / 16);
    std::vector<int32_t> rep(4 * B), hit_img(S, -1), hit_pd(S, -1);
    for (int i = 0; i < S; i++) {
        rep[i] = (int32_t)(std::find(k.img.begin(), k.img.end(), k.img[i]) - k.img.begin());
        rep[S + i] = (int32_t)(std::find(k.pdid.begin(), k.pdid.end(), k.pdid[i]) - k.pdid.begin());
        if (rep[i] == i) hit_img[i] = lookup(w.fc, w.fc_held, k.img[i]);
        if (rep[S + i] == i) hit_pd[i] = lookup(w.pd, w.pd_held, k.pdid[i]);
    }
    const bool cached = k.with_fc && k.encode && k.first_kind, stored_pd = cached && k.with_pd && k.gemm_fh2;
    const CallInputs in = {rep.data(), 0, cached ? hit_img.data() : nullptr, stored_pd ? hit_pd.data() : nullptr, B, g.H, g.W, g.E, g.D,
                           g.F, g.l0, k.encode, k.first_kind, k.dedup_head, k.dedup_decoder, k.gemm_fh2, k.map_fh2, k.attn_maps,
                           cached && k.with_hp};
    // what the tables hold before the call, for the naive counts
    const int fc_size = w.fc.size(), pd_size = w.pd.size();
    std::set<int> img_ids(k.img.begin(), k.img.end()), pd_ids(k.pdid.begin(), k.pdid.end());
    int fc_hits = 0, pd_hits = 0;
    for (int id : img_ids) fc_hits += lookup(w.fc, w.fc_held, id) >= 0;
    for (int id : pd_ids) pd_hits += lookup(w.pd, w.pd_held, id) >= 0;
    std::set<int> head_stored[2];              // the ids of a side whose products are stored before the call
    for (int s = 0; s < 2; s++)
        for (int b = 0; b < B; b++) {
            const int e = lookup(w.fc, w.fc_held, k.img[s * B + b]);
            if (e >= 0 && w.naive[s][e]) head_stored[s].insert(k.img[s * B + b]);
        }
    std::memset(&L, 0x7f, sizeof(L));          // (an index the planner did not write is far out of every range)
    const CallPlan p = plan_call(in, w.fc, w.pd, w.bits, L);
    if (out) *out = p;
    REQUIRE(!p.fell_back && !p.drop);
    // ---- the counts, recomputed naively
    const bool fit = (size_t)img_ids.size() * g.E <= 3 * (size_t)S * g.D;      // the distinct frames' rows fit where they wait
    const int n_img = k.encode && k.first_kind && fit ? (int)img_ids.size() : S, n_pd = (int)pd_ids.size();
    seen.no_fit += k.encode && k.first_kind && !fit;
    REQUIRE(p.n_img == n_img && p.n_pd == n_pd);
    const bool sides = k.first_kind && k.dedup_head && k.map_fh2;
    int n_side[2];
    for (int s = 0; s < 2; s++) {
        const int u = distinct(k.img, s * B, (s + 1) * B);
        n_side[s] = sides && head_merge_fits(g.E, g.F, g.l0, N, B, u) ? u : B;
        REQUIRE(p.side_unique[s] == (sides ? u : B) && p.n_side[s] == n_side[s]);
    }
    int n_ent = 0, ent_unique[2] = {B, B};
    if (k.dedup_decoder && k.gemm_fh2 && k.attn_maps && n_img < S && n_pd < S) {
        for (int s = 0; s < 2; s++) {
            std::set<std::pair<int, int>> e;
            for (int b = 0; b < B; b++) e.insert({k.img[s * B + b], k.pdid[s * B + b]});
            ent_unique[s] = (int)e.size();
        }
        const int um = std::max(ent_unique[0], ent_unique[1]);
        if (um < B && (B * N) % 256 == 0 && (um * N) % 256 == 0) n_ent = um;
    }
    REQUIRE(p.n_ent == n_ent && p.ent_unique[0] == ent_unique[0] && p.ent_unique[1] == ent_unique[1]);
    seen.entries += n_ent > 0;
    const bool fc = cached && fit;             // (all 2 B frames' rows do not fit either when the distinct ones' do not)
    REQUIRE(p.fc == fc && p.pd == stored_pd);
    if (fc) {
        const int misses = n_img - fc_hits, stored = std::min(misses, w.cap - fc_hits);
        REQUIRE(p.fc_n[0] == fc_hits && p.fc_n[1] == misses && p.fc_n[0] + p.fc_n[1] == n_img);
        REQUIRE(p.fc_fresh == misses && p.fc_store == stored && p.fc_n[2] == std::max(0, stored - (w.cap - fc_size)));
        seen.hits += fc_hits;
        seen.unstored += misses - stored;
        seen.evictions += p.fc_n[2];
    } else
        REQUIRE(p.fc_n[0] == 0 && p.fc_n[1] == 0 && p.fc_n[2] == 0 && p.fc_fresh == 0 && p.fc_store == 0);
    if (stored_pd) {
        const int misses = n_pd - pd_hits, stored = std::min(misses, w.cap - pd_hits);
        REQUIRE(p.pd_n[0] == pd_hits && p.pd_n[1] == misses && p.pd_n[0] + p.pd_n[1] == n_pd);
        REQUIRE(p.pd_fresh == misses && p.pd_store == stored && p.pd_n[2] == std::max(0, stored - (w.cap - pd_size)));
    } else
        REQUIRE(p.pd_n[0] == 0 && p.pd_n[1] == 0 && p.pd_n[2] == 0 && p.pd_fresh == 0 && p.pd_store == 0);
    for (int s = 0; s < 2; s++) {
        const bool hp = fc && k.with_hp && k.map_fh2 && k.gemm_fh2 && n_side[s] < B;
        REQUIRE(p.hp[s] == hp);
        REQUIRE(p.hp_hits(s) == (hp ? (int)head_stored[s].size() : 0) && p.hp_misses(s) == (hp ? n_side[s] - (int)head_stored[s].size() : 0));
        seen.head_hits += p.hp_hits(s);
        seen.head_fresh += p.hp_misses(s);
    }
    const bool use = fc || stored_pd || n_img < S || n_pd < S || n_side[0] < B || n_side[1] < B;
    REQUIRE(p.use == use);
    REQUIRE(p.side_merged[0] == (use && n_side[0] < B) && p.side_merged[1] == (use && n_side[1] < B));
    seen.plain += !use;
    if (!use) return 0;
    // ---- the stores the lists order
    const bool img_lists = n_img < S || fc;
    if (fc)
        for (int j = 0, q = 0; j < n_img; j++) {
            REQUIRE(L.uniq_img[j] >= 0 && L.uniq_img[j] < S && L.fc_ent[j] >= -1 && L.fc_ent[j] < w.cap);
            if (L.fc_miss[j] < 0) continue;
            REQUIRE(L.fc_miss[j] == q && L.fc_fresh[q] == L.uniq_img[j]);      // the fresh rows in list order
            q++;
            if (L.fc_ent[j] < 0) continue;
            w.fc_held[L.fc_ent[j]] = k.img[L.uniq_img[j]];
            w.naive[0][L.fc_ent[j]] = w.naive[1][L.fc_ent[j]] = 0;
        }
    if (stored_pd)
        for (int j = 0; j < n_pd; j++) {
            REQUIRE(L.uniq_pd[j] >= 0 && L.uniq_pd[j] < S && L.pd_ent[j] >= -1 && L.pd_ent[j] < w.cap);
            REQUIRE(L.pd_miss[j] >= -1 && L.pd_miss[j] < p.pd_fresh);
            if (L.pd_miss[j] >= 0) REQUIRE(L.pd_fresh[L.pd_miss[j]] == L.uniq_pd[j]);
            if (L.pd_miss[j] >= 0 && L.pd_ent[j] >= 0) w.pd_held[L.pd_ent[j]] = k.pdid[L.uniq_pd[j]];
        }
    for (int s = 0; s < 2; s++)
        for (int j = 0; p.hp[s] && j < n_side[s]; j++) {
            const int off = s * B, e = L.hp_ent[off + j], f = L.hp_miss[off + j];
            REQUIRE(e >= -1 && e < w.cap && f >= -1 && f < p.hp_fresh[s]);
            REQUIRE(L.uniq_side[off + j] >= off && L.uniq_side[off + j] < off + B);
            if (f >= 0) REQUIRE(L.hp_fresh[off + f] == L.uniq_side[off + j]);
            if (f >= 0 && e >= 0) {
                w.hp_rows[s][e] = k.img[L.uniq_side[off + j]];
                w.naive[s][e] = 1;
            }
        }
    for (int e = 0; e < w.cap; e++)
        for (int s = 0; s < 2; s++) REQUIRE(w.bits.has(e, s) == (w.naive[s][e] != 0));
    // ---- every slot finds its own content
    for (int i = 0; i < S; i++) {
        if (img_lists) {                       // the frame rows: an entry, a fresh row, or the distinct image itself
            const int r = L.map_img[i];
            REQUIRE(r >= 0 && r < n_img && L.uniq_img[r] >= 0 && L.uniq_img[r] < S && k.img[L.uniq_img[r]] == k.img[i]);
            if (fc && L.fc_miss[r] < 0) REQUIRE(L.fc_ent[r] >= 0 && w.fc.stamp[L.fc_ent[r]] && w.fc_held[L.fc_ent[r]] == k.img[i]);
            if (fc && L.fc_miss[r] >= 0) REQUIRE(L.fc_miss[r] < p.fc_fresh && k.img[L.fc_fresh[L.fc_miss[r]]] == k.img[i]);
        }
        const int r = L.map_pd[i];
        REQUIRE(r >= 0 && r < n_pd && L.uniq_pd[r] >= 0 && L.uniq_pd[r] < S && k.pdid[L.uniq_pd[r]] == k.pdid[i]);
        if (stored_pd) {
            const int src = L.pd_src[i];
            if (src >= 0) REQUIRE(src < w.cap && w.pd.stamp[src] && w.pd_held[src] == k.pdid[i]);
            else REQUIRE(~src < p.pd_fresh && k.pdid[L.pd_fresh[~src]] == k.pdid[i]);
        }
    }
    for (int s = 0; s < 2; s++) {
        const int off = s * B;
        for (int b = 0; b < B && n_side[s] < B; b++) {
            const int r = L.map_side[off + b];
            REQUIRE(r >= 0 && r < n_side[s] && L.uniq_side[off + r] >= off && L.uniq_side[off + r] < off + B);
            REQUIRE(k.img[L.uniq_side[off + r]] == k.img[off + b]);
            if (!p.hp[s]) continue;
            const int src = L.hp_src[off + b];
            if (src >= 0) REQUIRE(src < w.cap && w.hp_rows[s][src] == k.img[off + b] && w.fc.stamp[src] && w.fc_held[src] == k.img[off + b]);
            else REQUIRE(~src < p.hp_fresh[s] && k.img[L.hp_fresh[off + ~src]] == k.img[off + b]);
        }
        // block 0 on entries: each slot's entry is its own (image, prior), and its keys are the other side's slot's entry
        for (int b = 0; b < B && n_ent > 0; b++) {
            const int r = L.map_eo[off + b], q = L.map_ekv[off + b];
            REQUIRE(r >= s * n_ent && r < (s + 1) * n_ent && q >= s * n_ent && q < (s + 1) * n_ent);
            REQUIRE(L.ent_img[r] >= 0 && L.ent_img[r] < n_img && L.ent_pd[r] >= 0 && L.ent_pd[r] < n_pd);
            REQUIRE(k.img[L.uniq_img[L.ent_img[r]]] == k.img[off + b] && k.pdid[L.uniq_pd[L.ent_pd[r]]] == k.pdid[off + b]);
            REQUIRE(q - s * n_ent == L.map_eo[(1 - s) * B + b] - (1 - s) * n_ent);
        }
    }
    for (int i = 0; i < 2 * n_ent; i++) {      // the z rows of a block-0 entry (padding rows repeat a real entry)
        REQUIRE(L.ent_pd[i] >= 0 && L.ent_pd[i] < n_pd);
        if (!stored_pd) continue;
        const int want = k.pdid[L.uniq_pd[L.ent_pd[i]]], src = L.pd_src_ent[i];
        if (src >= 0) REQUIRE(src < w.cap && w.pd.stamp[src] && w.pd_held[src] == want);
        else REQUIRE(~src < p.pd_fresh && k.pdid[L.pd_fresh[~src]] == want);
    }
    for (int s = 0; s < 2 && B > 1; s++)
        for (int b = 0; b < B; b++) seen.both_sides += std::count(k.img.begin() + (1 - s) * B, k.img.begin() + (2 - s) * B, k.img[s * B + b]) > 0;
    return 0;
}

CallSpec batch(int B, std::vector<int> img, std::vector<int> pdid) {
    CallSpec k;
    k.B = B;
    k.img = std::move(img);
    k.pdid = std::move(pdid);
    return k;
}

}  // namespace

#define RUN(...)                                                            \
    do {                                                                    \
        const int line__ = run_call(__VA_ARGS__);                           \
        if (line__) {                                                       \
            std::printf("FAILED run_call line %d (line %d)\n", line__, __LINE__); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main() {
    static_assert(DD_LISTS == 22 && sizeof(CallLists) == 22 * (DEDUP_MAX_SLOTS / 2) * 4, "the upload keeps its size");
    static_assert(offsetof(CallLists, map_side) == 5 * sizeof(CallLists::List) && offsetof(CallLists, fc_fresh) == 10 * sizeof(CallLists::List) &&
                      offsetof(CallLists, pd_src_ent) == 17 * sizeof(CallLists::List) && offsetof(CallLists, hp_src) == 21 * sizeof(CallLists::List),
                  "the lists keep their order in memory");
    const std::unique_ptr<CallLists> lists(new CallLists);
    CallLists& L = *lists;
    Seen seen;
    const Config small = {32, 32, 32, 32, 64, 96}, tiles = {32, 32, 32, 32, 256, 256}, wide = {128, 32, 32, 32, 64, 96};

    // ---- an entry whose head bits were set is evicted, and the entry is then reused for another frame: the stale r0 / c of the
    // first frame must not be named as a source
    {
        World w(1);
        CallPlan p;
        RUN(w, small, batch(2, {7, 7, 7, 7}, {1, 1, 1, 1}), L, seen, &p);       // frame 7 -> entry 0, both sides' products stored
        CHECK(p.fc && p.hp[0] && p.hp[1] && p.hp_store[0] == 1 && p.hp_store[1] == 1 && w.bits.count() == 2 && w.hp_rows[0][0] == 7);
        CallSpec k = batch(2, {8, 8, 8, 8}, {1, 1, 1, 1});
        k.with_hp = false;                                                       // frame 8 evicts it while no head storage is installed
        RUN(w, small, k, L, seen, &p);
        CHECK(p.fc_n[2] == 1 && w.fc_held[0] == 8 && w.bits.count() == 0 && w.hp_rows[0][0] == 7 && w.hp_rows[1][0] == 7);
        RUN(w, small, batch(2, {8, 8, 8, 8}, {1, 1, 1, 1}), L, seen, &p);       // a hit in the frame cache, but its products are frame 7's
        CHECK(p.fc_n[0] == 1 && p.hp_hits(0) == 0 && p.hp_hits(1) == 0 && L.hp_src[0] == ~0 && L.hp_src[2] == ~0 && w.hp_rows[0][0] == 8);
        RUN(w, small, batch(2, {8, 8, 8, 8}, {1, 1, 1, 1}), L, seen, &p);       // now they are frame 8's
        CHECK(p.hp_hits(0) == 1 && p.hp_hits(1) == 1 && L.hp_src[0] == 0 && L.hp_src[3] == 0 && p.fc_fresh == 0 && p.pd_fresh == 0);
        // the same with both storages installed throughout: the eviction and the refill in one call
        RUN(w, small, batch(2, {9, 9, 9, 9}, {2, 2, 2, 2}), L, seen, &p);
        CHECK(p.fc_n[2] == 1 && p.pd_n[2] == 1 && p.hp_hits(0) == 0 && L.hp_src[1] == ~0 && w.hp_rows[1][0] == 9 && w.bits.count() == 2);
    }
    // ---- capacity smaller than the number of misses: the first misses are stored, the others computed and not stored
    {
        World w(2);
        CallPlan p;
        RUN(w, small, batch(2, {1, 2, 3, 4}, {5, 6, 7, 8}), L, seen, &p);       // all distinct
        CHECK(p.fc_n[1] == 4 && p.fc_store == 2 && p.pd_store == 2 && L.fc_ent[0] == 0 && L.fc_ent[1] == 1 && L.fc_ent[2] == -1 && L.fc_ent[3] == -1);
        RUN(w, small, batch(2, {3, 3, 3, 1}, {7, 7, 5, 5}), L, seen, &p);       // frame 3 was not stored; frame 1 was; side 0 merges
        CHECK(p.fc_n[0] == 1 && p.fc_n[1] == 1 && p.fc_n[2] == 1 && p.hp[0] && !p.hp[1] && p.pd_n[0] == 1);
    }
    // ---- a malformed rep table, and a set mismatch flag: the fall-back is reported and the tables stay as they are
    {
        World w(3);
        RUN(w, small, batch(2, {1, 1, 2, 2}, {3, 3, 3, 4}), L, seen);
        const FrameCacheTable fc0 = w.fc, pd0 = w.pd;
        const HeadBits bits0 = w.bits;
        CHECK(bits0.count() > 0 && fc0.size() == 2);
        const int32_t hit[4] = {-1, -1, -1, -1};
        const int32_t bad[][8] = {{0, 0, 3, 2, 0, 0, 0, 3}, {0, 2, 2, 2, 0, 0, 0, 3}, {0, 0, 2, 2, 0, 2, 0, 3}, {0, 0, 2, -1, 0, 0, 0, 3},
                                  {0, 0, 2, 2, 0, 0, 1, 3}};
        for (int t = 0; t < 6; t++) {
            const int32_t good[8] = {0, 0, 2, 2, 0, 0, 0, 3};
            const CallInputs in = {t < 5 ? bad[t] : good, t < 5 ? 0 : 1, hit, hit, 2, 64, 96, 32, 32, 32, 32, true, true, true, true, true,
                                   true, true, true};
            const CallPlan p = plan_call(in, w.fc, w.pd, w.bits, L);
            CHECK(p.fell_back && !p.use && !p.drop && p.n_img == 4 && p.n_pd == 4 && p.side_unique[0] == 2 && p.side_unique[1] == 2);
            CHECK(!std::memcmp(&fc0, &w.fc, sizeof(fc0)) && !std::memcmp(&pd0, &w.pd, sizeof(pd0)) && !std::memcmp(&bits0, &w.bits, sizeof(bits0)));
        }
    }
    // ---- random sequences
    std::mt19937 rng(97531);
    for (int trial = 0; trial < 300; trial++) {
        const int cap = 1 + (int)(rng() % (trial % 5 == 0 ? 12 : 4));
        World w(cap);
        const Config& g = trial % 3 == 0 ? tiles : trial % 11 == 1 ? wide : small;
        const int universe = 1 + (int)(rng() % (cap + 4));
        // one store absent throughout, in turn: the frame cache (and with it the others), the priors, the head products
        const int absent = trial % 8 < 3 ? trial % 8 : -1;
        for (int call = 0; call < 40; call++) {
            if (rng() % 13 == 0) w.flush();    // a flush in mid-sequence
            CallSpec k;
            k.B = 1 + (int)(rng() % 4);
            const int S = 2 * k.B, kind = (int)(rng() % 6);
            k.img.resize(S);
            k.pdid.resize(S);
            for (int i = 0; i < S; i++) {
                k.img[i] = kind == 0 ? 0 : kind == 1 ? i : (int)(rng() % universe);       // all equal, all distinct, a mixture
                k.pdid[i] = kind == 0 ? 0 : kind == 1 ? i : (int)(rng() % universe);
            }
            k.with_fc = absent != 0 && rng() % 9 != 0;
            k.with_pd = absent != 1 && rng() % 9 != 0;
            k.with_hp = absent != 2 && rng() % 9 != 0;
            k.dedup_head = rng() % 7 != 0;
            k.dedup_decoder = rng() % 7 != 0;
            k.attn_maps = rng() % 11 != 0;
            k.gemm_fh2 = rng() % 11 != 0;
            k.map_fh2 = rng() % 11 != 0;
            if (rng() % 10 == 0) {             // a decode call: no store, the first kind looked at only for the heads
                k.encode = false;
                k.first_kind = rng() % 2 != 0;
            }
            RUN(w, g, k, L, seen);
        }
    }
    // every kind of case was met
    CHECK(seen.hits > 1000 && seen.unstored > 300 && seen.evictions > 300 && seen.head_hits > 300 && seen.head_fresh > 300);
    CHECK(seen.entries > 100 && seen.both_sides > 1000 && seen.plain > 30 && seen.no_fit > 20);
    std::printf("ok\n");
    return 0;
}
