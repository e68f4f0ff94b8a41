// Stand-alone check of the host side of the head products kept across calls (align3r_amd/csrc/dedup.h): the (entry, side) bits
// (HeadBits) and head_lists, on top of the frame cache's FrameCacheTable, against a naive model.  Random sequences of calls whose
// frames are partly stored, partly new, with fewer, as many and more misses than entries, sides that take part or not, and flushes
// in between; after every call each slot of a side must find its own frame's blocks through the signed source list -- in the
// entry the table names, which must still hold that frame, or among the fresh blocks -- a stored frame must be exactly one the
// naive model has stored for that side, and an entry the frame cache refilled must have lost both of its bits.  Built with
// -fsanitize=address,undefined by tests/test_head_products_cpu.py; prints "ok".
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

int main() {
    std::mt19937 rng(8642);
    long n_hits = 0, n_fresh_all = 0, n_unstored = 0, n_evicted_bits = 0;
    for (int trial = 0; trial < 400; trial++) {
        const int cap = 1 + (int)(rng() % (trial % 7 == 0 ? 40 : 5));
        FrameCacheTable t;
        t.reset(cap);
        HeadBits bits;
        std::vector<int> held(cap, -1);                              // the frame entry e holds (the frame cache's image)
        // the "device" storage: the frame whose r0 / c blocks lie in (entry, side), never cleared -- stale content stays there
        std::vector<int> rows[2] = {std::vector<int>(cap, -1), std::vector<int>(cap, -1)};
        // the naive model: (entry, side) holds the product of the frame the entry holds
        std::vector<char> naive[2] = {std::vector<char>(cap, 0), std::vector<char>(cap, 0)};
        const int universe = 1 + (int)(rng() % (2 * cap + 3));
        for (int call = 0; call < 60; call++) {
            if (rng() % 23 == 0) {
                t.flush();
                bits.flush();
                std::fill(held.begin(), held.end(), -1);
                for (int s = 0; s < 2; s++) std::fill(naive[s].begin(), naive[s].end(), 0);
            }
            // the call's distinct images, in list order
            std::vector<int> fr(universe);
            for (int i = 0; i < universe; i++) fr[i] = i;
            std::shuffle(fr.begin(), fr.end(), rng);
            fr.resize(1 + rng() % universe);
            const int n_img = (int)fr.size();
            std::vector<int32_t> hit(n_img), ent(n_img, -7), miss(n_img);
            for (int k = 0; k < n_img; k++) {
                hit[k] = -1;
                for (int e = 0; e < cap; e++)
                    if (held[e] == fr[k]) hit[k] = e;
            }
            int n[3];
            CHECK(t.assign(hit.data(), n_img, ent.data(), n) == 0);
            // what find_distinct does with the answer: the misses in list order, and a refilled entry loses its bits
            int n_miss = 0;
            for (int k = 0; k < n_img; k++) {
                if (hit[k] >= 0) { miss[k] = -1; continue; }
                miss[k] = n_miss++;
                if (ent[k] >= 0) {
                    n_evicted_bits += bits.has(ent[k], 0) + bits.has(ent[k], 1);
                    bits.clear(ent[k]);
                    held[ent[k]] = fr[k];
                    naive[0][ent[k]] = naive[1][ent[k]] = 0;
                }
            }
            for (int e = 0; e < cap; e++)
                for (int s = 0; s < 2; s++) CHECK(bits.has(e, s) == (naive[s][e] != 0));
            // each side: some of the call's images, each at least once, first appearances ascending (dedup_group_side); a side may
            // not take part (it does not merge), and then nothing of it is read or written
            for (int s = 0; s < 2; s++) {
                if (rng() % 4 == 0) continue;
                std::vector<int32_t> row;                            // the side's distinct frames as rows of the image list
                for (int k = 0; k < n_img; k++)
                    if (rng() % 3) row.push_back(k);
                if (row.empty()) row.push_back((int32_t)(rng() % n_img));
                std::shuffle(row.begin(), row.end(), rng);
                const int U = (int)row.size();
                std::vector<int32_t> map, uniq(U);
                for (int k = 0; k < U; k++) {
                    uniq[k] = 1000 * s + (int32_t)map.size();        // the slot (any number: the list is only handed on)
                    map.push_back(k);
                    if (k > 0 && rng() % 2) map.push_back((int32_t)(rng() % (k + 1)));
                }
                const int B = (int)map.size();
                std::vector<int32_t> hent(U, -7), hmiss(U, -7), uniq_fresh(U, -7), src(B, 12345);
                int n_store = -1;
                const HeadBits before = bits;
                const int n_fresh = head_lists(bits, s, ent.data(), miss.data(), n_img, row.data(), uniq.data(), U, map.data(), B,
                                               hent.data(), hmiss.data(), uniq_fresh.data(), src.data(), &n_store);
                CHECK(n_fresh >= 0 && n_fresh <= U);
                int j = 0, stored = 0;
                std::vector<int> fresh;                              // the "device": fresh block j is the frame of slot uniq_fresh[j]
                for (int k = 0; k < U; k++) {
                    const int e = ent[row[k]];
                    const bool want_stored = hit[row[k]] >= 0 && naive[s][e];
                    CHECK(hent[k] == e);
                    if (want_stored) { CHECK(hmiss[k] == -1 && before.has(e, s)); n_hits++; continue; }
                    CHECK(hmiss[k] == j && uniq_fresh[j] == uniq[k]);
                    fresh.push_back(fr[row[k]]);
                    j++;
                    if (e >= 0) { stored++; CHECK(bits.has(e, s)); } else n_unstored++;
                }
                CHECK(j == n_fresh && stored == n_store);
                n_fresh_all += n_fresh;
                // the store pass, then the combine pass reads every slot
                for (int k = 0; k < U; k++)
                    if (hmiss[k] >= 0 && hent[k] >= 0) {
                        rows[s][hent[k]] = fresh[hmiss[k]];
                        naive[s][hent[k]] = 1;
                    }
                for (int b = 0; b < B; b++) {
                    const int want = fr[row[map[b]]];
                    if (src[b] >= 0) {
                        CHECK(src[b] < cap && rows[s][src[b]] == want && held[src[b]] == want);
                        CHECK(hmiss[map[b]] < 0);                    // a fresh frame is read from the arena, stored or not
                    } else
                        CHECK(~src[b] < n_fresh && fresh[~src[b]] == want);
                }
                // the other side's bits did not move
                for (int e = 0; e < cap; e++) CHECK(bits.has(e, 1 - s) == before.has(e, 1 - s));
            }
        }
    }
    CHECK(n_hits > 1000 && n_fresh_all > 1000 && n_unstored > 100 && n_evicted_bits > 100);      // every kind of case was met
    // malformed arguments are refused and change nothing
    {
        HeadBits bits;
        bits.set(1, 0);
        const int32_t ent[2] = {1, 0}, miss[2] = {-1, 0}, row[2] = {0, 1}, bad_row[2] = {0, 2}, uniq[2] = {0, 1}, map[3] = {0, 1, 0},
                      bad_map[3] = {0, 2, 0};
        int32_t hent[2], hmiss[2], uf[2], src[3];
        int ns;
        CHECK(head_lists(bits, 0, ent, miss, 2, bad_row, uniq, 2, map, 3, hent, hmiss, uf, src, &ns) == -1);
        CHECK(head_lists(bits, 0, ent, miss, 2, row, uniq, 2, bad_map, 3, hent, hmiss, uf, src, &ns) == -1);
        CHECK(head_lists(bits, 2, ent, miss, 2, row, uniq, 2, map, 3, hent, hmiss, uf, src, &ns) == -1);
        CHECK(head_lists(bits, 0, nullptr, miss, 2, row, uniq, 2, map, 3, hent, hmiss, uf, src, &ns) == -1);
        CHECK(bits.count() == 1 && bits.has(1, 0));
        CHECK(head_lists(bits, 0, ent, miss, 2, row, uniq, 2, map, 3, hent, hmiss, uf, src, &ns) == 1 && ns == 1);
        CHECK(src[0] == 1 && src[1] == ~0 && src[2] == 1 && hmiss[0] == -1 && hmiss[1] == 0 && uf[0] == 1 && bits.has(0, 0) && !bits.has(0, 1));
        // side 1 of the same entries: nothing stored yet
        CHECK(head_lists(bits, 1, ent, miss, 2, row, uniq, 2, map, 3, hent, hmiss, uf, src, &ns) == 2 && ns == 2 && bits.count() == 4);
        bits.clear(1);
        CHECK(!bits.has(1, 0) && !bits.has(1, 1) && bits.count() == 2);
        bits.flush();
        CHECK(bits.count() == 0);
    }
    // the storage's layout: sides and blocks of an entry, and a side's words
    {
        alignas(256) static char buf[3 * (2 * FC_STAT_WORDS * 4 + 4 * 64 * 4)];
        CHECK(head_products_entry_bytes(64) * 3 == sizeof(buf));
        const HeadStore st = head_store_layout(buf, 3, 64);
        CHECK(st.cap == 3 && st.stride() == 256 && st.rows == buf + 3 * 2 * FC_STAT_WORDS * 4);
        const float* rows = reinterpret_cast<const float*>(st.rows);
        CHECK(st.r0(0) == rows && st.c(0) == rows + 64 && st.r0(1) == rows + 128 && st.c(1) == rows + 192);
        CHECK(st.c(1) + 2 * st.stride() + 64 == reinterpret_cast<const float*>(buf + sizeof(buf)));      // the last block ends the storage
        CHECK(st.side_words(0) == reinterpret_cast<unsigned*>(buf) && st.side_words(1) == reinterpret_cast<unsigned*>(buf) + 3 * FC_STAT_WORDS);
        CHECK(head_store_layout(nullptr, 3, 64).cap == 0);
    }
    std::printf("ok\n");
    return 0;
}
