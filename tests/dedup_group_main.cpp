// Stand-alone CPU program for tests/test_dedup_cpu.py: the host grouping of align3r_amd/csrc/dedup.h (representatives -> distinct
// list + slot map), built with -fsanitize=address,undefined.  Prints one line per failed check; exit status = number of failures.
#include "dedup.h"
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond, name)                                        \
    do {                                                         \
        if (!(cond)) {                                           \
            std::printf("FAILED %s: %s\n", name, #cond);         \
            failures++;                                          \
        }                                                        \
    } while (0)

// the representative table the device computes: the smallest slot with the same key
static std::vector<int32_t> reps_of(const std::vector<int>& keys) {
    std::vector<int32_t> rep(keys.size());
    for (size_t s = 0; s < keys.size(); s++) {
        size_t r = 0;
        while (keys[r] != keys[s]) r++;
        rep[s] = (int32_t)r;
    }
    return rep;
}

// groups `keys`, checks every property the plan relies on, returns U
static int group_and_check(const char* name, const std::vector<int>& keys, int want_u) {
    const int n = (int)keys.size();
    const std::vector<int32_t> rep = reps_of(keys);
    // exactly n entries each, so that the sanitizer sees a write past either list
    std::vector<int32_t> uniq(n, -7), map(n, -7);
    const int U = a3r::dedup_group(rep.data(), n, uniq.data(), map.data());
    CHECK(U == want_u, name);
    if (U < 1 || U > n) return U;
    std::vector<int> hit(U, 0);
    for (int s = 0; s < n; s++) {
        CHECK(map[s] >= 0 && map[s] < U, name);                       // a map into 0 .. U-1 ...
        if (map[s] < 0 || map[s] >= U) return U;
        hit[map[s]]++;
        const int r = uniq[map[s]];
        CHECK(keys[r] == keys[s], name);                              // ... that never merges unequal slots
        CHECK(r <= s, name);                                          // the representative is the smallest index of its group:
        for (int t = 0; t < r; t++) CHECK(keys[t] != keys[s], name);  // nothing before it has the key
    }
    for (int k = 0; k < U; k++) {
        CHECK(hit[k] >= 1, name);                                     // ... onto it (a surjection)
        CHECK(map[uniq[k]] == k, name);
        if (k) CHECK(uniq[k - 1] < uniq[k], name);                    // the distinct list ascends
    }
    for (int s = 0; s < n; s++)
        for (int t = 0; t < n; t++) CHECK((map[s] == map[t]) == (keys[s] == keys[t]), name);
    return U;
}

int main() {
    group_and_check("all equal", std::vector<int>(10, 4), 1);
    group_and_check("all distinct", {9, 8, 7, 6, 5, 4, 3, 2, 1, 0}, 10);
    group_and_check("interleaved", {0, 0, 1, 2, 1, 1, 2, 0, 0, 2}, 3);
    group_and_check("interleaved, long", {5, 3, 5, 3, 5, 3, 1, 1, 5, 3, 2, 1, 2, 5}, 4);
    group_and_check("one duplicate at the end", {0, 1, 2, 3, 4, 0}, 5);
    group_and_check("one slot", {3}, 1);
    group_and_check("two slots, equal", {3, 3}, 1);
    group_and_check("two slots, distinct", {3, 4}, 2);
    {   // tables that are not representative tables are refused, not used
        int32_t uniq[4], map[4];
        const int32_t forward[4] = {0, 2, 2, 3}, chain[4] = {0, 0, 1, 3}, negative[4] = {0, -1, 2, 3};
        CHECK(a3r::dedup_group(forward, 4, uniq, map) == -1, "rep > slot");
        CHECK(a3r::dedup_group(chain, 4, uniq, map) == -1, "rep of a non-representative");
        CHECK(a3r::dedup_group(negative, 4, uniq, map) == -1, "negative rep");
        CHECK(a3r::dedup_group(forward, 0, uniq, map) == -1, "no slots");
    }
    if (!failures) std::printf("ok\n");
    return failures;
}
