// Stand-alone check of FrameCacheTable (align3r_amd/csrc/dedup.h) against a naive model: random sequences of calls whose distinct
// frames are partly stored (hits), partly new (misses), with fewer, as many and more misses than entries, flushes in between, and
// malformed hit lists.  Built with -fsanitize=address,undefined by tests/test_frame_cache_cpu.py; prints "ok".
#include "dedup.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace a3r;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);        \
            return 1;                                                  \
        }                                                              \
    } while (0)

// The naive model: frame[e] = the frame entry e holds (-1: free), order = the used entries from least to most recently used.
struct Naive {
    std::vector<int> frame, order;
    explicit Naive(int cap) : frame(cap, -1) {}
    void touch(int e) {
        order.erase(std::remove(order.begin(), order.end(), e), order.end());
        order.push_back(e);
    }
    // frames of one call (distinct) -> where each is read from / stored to, and the counts
    void call(const std::vector<int>& fr, std::vector<int>& ent, int* n) {
        const int cap = (int)frame.size();
        ent.assign(fr.size(), -1);
        n[0] = n[1] = n[2] = 0;
        std::vector<bool> used(cap, false);
        for (size_t k = 0; k < fr.size(); k++)
            for (int e = 0; e < cap; e++)
                if (frame[e] == fr[k]) { ent[k] = e; used[e] = true; }
        for (size_t k = 0; k < fr.size(); k++) {
            if (ent[k] >= 0) { n[0]++; continue; }
            n[1]++;
            int e = -1;
            for (int c = 0; c < cap && e < 0; c++)
                if (frame[c] < 0 && !used[c]) e = c;
            if (e < 0)
                for (int c : order)
                    if (!used[c]) { e = c; n[2]++; break; }
            if (e >= 0) { used[e] = true; frame[e] = fr[k]; }
            ent[k] = e;
        }
        for (size_t k = 0; k < fr.size(); k++)
            if (ent[k] >= 0) touch(ent[k]);
    }
};

int main() {
    std::mt19937 rng(12345);
    for (int trial = 0; trial < 300; trial++) {
        const int cap = 1 + (int)(rng() % (trial % 7 == 0 ? FC_MAX_ENTRIES : 6));
        FrameCacheTable t;
        t.reset(cap);
        Naive nv(cap);
        CHECK(t.size() == 0);
        const int universe = 1 + (int)(rng() % (2 * cap + 3));
        for (int call = 0; call < 60; call++) {
            if (rng() % 23 == 0) {
                t.flush();
                nv = Naive(cap);
                CHECK(t.size() == 0);
            }
            // distinct frames of the call, in random order; sometimes more of them than there are entries
            std::vector<int> fr(universe);
            for (int i = 0; i < universe; i++) fr[i] = i;
            std::shuffle(fr.begin(), fr.end(), rng);
            fr.resize(1 + rng() % universe);
            // what the device would answer: the entry holding the frame, or -1
            std::vector<int32_t> hit(fr.size()), ent(fr.size(), -7);
            for (size_t k = 0; k < fr.size(); k++) {
                hit[k] = -1;
                for (int e = 0; e < cap; e++)
                    if (nv.frame[e] == fr[k]) hit[k] = e;
            }
            const FrameCacheMask mk = t.mask();
            for (int e = 0; e < FC_MAX_ENTRIES; e++) CHECK((((mk.w[e / 32] >> (e % 32)) & 1u) != 0) == (e < cap && nv.frame[e] >= 0));
            std::vector<int> want;
            int n_want[3], n_got[3];
            nv.call(fr, want, n_want);
            CHECK(t.assign(hit.data(), (int)fr.size(), ent.data(), n_got) == 0);
            for (int i = 0; i < 3; i++) CHECK(n_got[i] == n_want[i]);
            CHECK(n_got[0] + n_got[1] == (int)fr.size());
            for (size_t k = 0; k < fr.size(); k++) {
                CHECK(ent[k] == want[k]);
                if (hit[k] >= 0) CHECK(ent[k] == hit[k]);                 // a hit is read where it was found
                for (size_t j = 0; j < k; j++) CHECK(ent[k] < 0 || ent[k] != ent[j]);      // no entry twice in one call
            }
            int stored = 0;
            for (int e = 0; e < cap; e++) stored += nv.frame[e] >= 0;
            CHECK(t.size() == stored);
        }
    }
    // malformed answers are refused and change nothing
    FrameCacheTable t;
    t.reset(3);
    int32_t ent[4];
    int n[3];
    const int32_t fill[2] = {-1, -1};
    CHECK(t.assign(fill, 2, ent, n) == 0 && ent[0] == 0 && ent[1] == 1 && n[0] == 0 && n[1] == 2 && n[2] == 0);
    const FrameCacheTable before = t;
    const int32_t twice[2] = {0, 0}, free_entry[1] = {2}, outside[1] = {3}, below[1] = {-2};
    CHECK(t.assign(twice, 2, ent, n) == -1);
    CHECK(t.assign(free_entry, 1, ent, n) == -1);
    CHECK(t.assign(outside, 1, ent, n) == -1);
    CHECK(t.assign(below, 1, ent, n) == -1);
    CHECK(t.assign(nullptr, 1, ent, n) == -1);
    CHECK(t.clock == before.clock && t.size() == before.size() && t.stamp[0] == before.stamp[0] && t.stamp[1] == before.stamp[1]);
    // capacity 0 stores nothing; capacities are clamped
    t.reset(0);
    CHECK(t.assign(fill, 2, ent, n) == 0 && ent[0] == -1 && ent[1] == -1 && n[1] == 2 && n[2] == 0);
    t.reset(FC_MAX_ENTRIES + 5);
    CHECK(t.cap == FC_MAX_ENTRIES);
    // the layout: fields inside the storage, in order, and no entry in storage that is too small
    const long wi = 3 * 64 * 96, wf = 24 * 64;
    const size_t one = frame_cache_entry_bytes(wi, wf);
    std::vector<char> store(3 * one + 5);
    CHECK(frame_cache_layout(store.data(), one - 1, wi, wf).cap == 0);
    CHECK(frame_cache_layout(nullptr, 3 * one, wi, wf).cap == 0);
    const FrameCacheLayout l = frame_cache_layout(store.data(), store.size(), wi, wf);
    CHECK(l.cap == 3 && l.keys == store.data() && l.keys < l.stats && l.stats < l.flags && l.flags < l.img && l.img < l.feat);
    CHECK(l.feat + (size_t)l.cap * wf * 4 <= store.data() + store.size());
    CHECK((l.stats - l.keys) % 16 == 0 && (l.img - l.keys) % 16 == 0 && (l.feat - l.keys) % 16 == 0);
    std::printf("ok\n");
    return 0;
}
