// Stand-alone check of the host side of the frame products kept across calls (align3r_amd/csrc/dedup.h): a FrameCacheTable of the
// depth priors, prior_lists and SiteMask, against a naive model.  Random sequences of calls whose distinct priors are partly
// stored, partly new, with fewer, as many and more misses than entries and flushes in between; after every call each row must
// find its own prior's rows through the source list -- in the entry the table names or among the fresh blocks -- and the
// statistics words of a masked site list must be the naive maximum.  Built with -fsanitize=address,undefined by
// tests/test_frame_products_cpu.py; prints "ok".
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

// what fc_stats_sites_kernel does with one word (dedup.hip), entry by entry
static unsigned merge_word(std::vector<unsigned>& entry_word, const std::vector<int32_t>& ent, const std::vector<int32_t>& miss, unsigned own) {
    unsigned w = own;
    for (size_t k = 0; k < ent.size(); k++) {
        if (ent[k] < 0) continue;
        if (miss[k] >= 0) entry_word[ent[k]] = own;
        else w = std::max(w, entry_word[ent[k]]);
    }
    return w;
}

int main() {
    std::mt19937 rng(4321);
    // ---- SiteMask: ranges with gaps, clipped at both ends
    for (int trial = 0; trial < 200; trial++) {
        SiteMask m;
        std::vector<bool> want(FC_STAT_WORDS, false);
        const int n = (int)(rng() % 9);
        for (int r = 0; r < n; r++) {
            const int lo = (int)(rng() % (FC_STAT_WORDS + 40)) - 20, hi = lo + (int)(rng() % 70) - 3;
            m.add(lo, hi);
            for (int i = std::max(lo, 0); i < hi && i < FC_STAT_WORDS; i++) want[i] = true;
        }
        for (int i = -3; i < FC_STAT_WORDS + 3; i++) CHECK(m.has(i) == (i >= 0 && i < FC_STAT_WORDS && want[i]));
    }
    // ---- table + lists: the stored content of entry e is the prior it holds (held[e], -1 free); stat[e][i] its words
    for (int trial = 0; trial < 300; trial++) {
        const int cap = 1 + (int)(rng() % (trial % 7 == 0 ? 40 : 5));
        FrameCacheTable t;
        t.reset(cap);
        std::vector<int> held(cap, -1);
        const int sites = 6;
        SiteMask mask;
        mask.add(1, 3);
        mask.add(4, 5);                                          // sites 1 2 4 of 0 .. 5
        std::vector<std::vector<unsigned>> stat(sites, std::vector<unsigned>(cap, 0));
        const int universe = 1 + (int)(rng() % (2 * cap + 3));
        for (int call = 0; call < 50; call++) {
            if (rng() % 19 == 0) {
                t.flush();
                std::fill(held.begin(), held.end(), -1);
            }
            std::vector<int> pr(universe);
            for (int i = 0; i < universe; i++) pr[i] = i;
            std::shuffle(pr.begin(), pr.end(), rng);
            pr.resize(1 + rng() % universe);
            const int U = (int)pr.size();
            // slots: every distinct prior at least once, in the order of first appearance, as dedup_group lists them
            std::vector<int32_t> row, uniq(U);
            for (int k = 0; k < U; k++) {
                uniq[k] = (int32_t)row.size();
                row.push_back(k);
                if (k > 0 && rng() % 2) row.push_back((int32_t)(rng() % (k + 1)));
            }
            std::vector<int32_t> hit(U), ent(U, -7), miss(U, -7), uniq_miss(U, -7), src(row.size(), 12345);
            for (int k = 0; k < U; k++) {
                hit[k] = -1;
                for (int e = 0; e < cap; e++)
                    if (held[e] == pr[k]) hit[k] = e;
            }
            int n[3], n_store = -1;
            CHECK(t.assign(hit.data(), U, ent.data(), n) == 0);
            const int n_miss = prior_lists(hit.data(), ent.data(), uniq.data(), U, miss.data(), uniq_miss.data(), row.data(), (int)row.size(),
                                           src.data(), &n_store);
            CHECK(n_miss == n[1]);
            // the misses keep their list order, and each names its first slot
            int j = 0, stored = 0;
            for (int k = 0; k < U; k++) {
                if (hit[k] >= 0) { CHECK(miss[k] == -1 && ent[k] == hit[k]); continue; }
                CHECK(miss[k] == j && uniq_miss[j] == uniq[k]);
                j++;
                stored += ent[k] >= 0;
            }
            CHECK(j == n_miss && stored == n_store && n_store <= cap);
            // the "device": fresh block j is the prior of slot uniq_miss[j]; the stored misses go to their entries
            std::vector<int> fresh(n_miss);
            for (int q = 0; q < n_miss; q++) fresh[q] = pr[row[uniq_miss[q]]];
            for (int k = 0; k < U; k++)
                if (miss[k] >= 0 && ent[k] >= 0) held[ent[k]] = fresh[miss[k]];
            for (size_t i = 0; i < row.size(); i++) {
                const int got = src[i] >= 0 ? (src[i] < cap ? held[src[i]] : -2) : (~src[i] < n_miss ? fresh[~src[i]] : -2);
                CHECK(got == pr[row[i]]);
                CHECK((src[i] >= 0) == (hit[row[i]] >= 0));           // a miss is read from its fresh rows, stored or not
            }
            // statistics: the words of the masked sites are kept with the filled entries and raised to those of the entries read;
            // the other sites keep their own
            for (int s = 0; s < sites; s++) {
                const unsigned own = n_miss ? (unsigned)(rng() % 1000) : 0u;
                std::vector<unsigned> before = stat[s];
                unsigned want = own;
                for (int k = 0; k < U; k++)
                    if (hit[k] >= 0) want = std::max(want, before[hit[k]]);
                const unsigned got = mask.has(s) ? merge_word(stat[s], ent, miss, own) : own;
                CHECK(got == (mask.has(s) ? want : own));
                for (int k = 0; k < U; k++)
                    if (miss[k] >= 0 && ent[k] >= 0 && mask.has(s)) CHECK(stat[s][ent[k]] == own);
            }
        }
    }
    // malformed arguments are refused
    {
        const int32_t hit[2] = {-1, 0}, ent[2] = {1, 0}, uniq[2] = {0, 1}, bad_row[1] = {2}, ok_row[3] = {0, 1, 0};
        int32_t miss[2], um[2], src[3];
        int ns;
        CHECK(prior_lists(hit, ent, uniq, 2, miss, um, bad_row, 1, src, &ns) == -1);
        CHECK(prior_lists(nullptr, ent, uniq, 2, miss, um, ok_row, 3, src, &ns) == -1);
        CHECK(prior_lists(hit, ent, uniq, 2, miss, um, ok_row, 3, src, &ns) == 1 && ns == 1);
        CHECK(src[0] == ~0 && src[1] == 0 && src[2] == ~0 && miss[0] == 0 && miss[1] == -1 && um[0] == 0);
    }
    std::printf("ok\n");
    return 0;
}
