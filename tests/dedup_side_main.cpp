// Stand-alone CPU program for tests/test_dedup_side_cpu.py: the per-side host grouping of align3r_amd/csrc/dedup.h (the image kind's
// representatives -> each side's distinct list + slot map, which the DPT heads' level-0 branch runs on), built with
// -fsanitize=address,undefined.  Prints one line per failed check; exit status = number of failures.
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

// the representative table the device computes over the 2 B slots of the kind: the smallest slot with the same key
static std::vector<int32_t> reps_of(const std::vector<int>& keys) {
    std::vector<int32_t> rep(keys.size());
    for (size_t s = 0; s < keys.size(); s++) {
        size_t r = 0;
        while (keys[r] != keys[s]) r++;
        rep[s] = (int32_t)r;
    }
    return rep;
}

// keys: side 0's B slots then side 1's; checks every property the plan relies on for both sides
static void sides_and_check(const char* name, const std::vector<int>& keys, int want_u0, int want_u1) {
    const int B = (int)keys.size() / 2;
    const std::vector<int32_t> rep = reps_of(keys);
    const int want[2] = {want_u0, want_u1};
    for (int s = 0; s < 2; s++) {
        // exactly B entries each, so that the sanitizer sees a write past either list
        std::vector<int32_t> uniq(B, -7), map(B, -7);
        const int U = a3r::dedup_group_side(rep.data(), B, s, uniq.data(), map.data());
        CHECK(U == want[s], name);
        if (U < 1 || U > B) continue;
        std::vector<int> hit(U, 0);
        for (int k = 0; k < U; k++) {
            CHECK(uniq[k] >= s * B && uniq[k] < (s + 1) * B, name);       // a slot of the side itself, wherever the representative sits
            if (uniq[k] < s * B || uniq[k] >= (s + 1) * B) return;
            if (k) CHECK(uniq[k - 1] < uniq[k], name);                    // ascending
            CHECK(map[uniq[k] - s * B] == k, name);
            for (int t = s * B; t < uniq[k]; t++) CHECK(keys[t] != keys[uniq[k]], name);      // the first slot of the side with that content
        }
        for (int b = 0; b < B; b++) {
            CHECK(map[b] >= 0 && map[b] < U, name);
            if (map[b] < 0 || map[b] >= U) return;
            hit[map[b]]++;
            CHECK(keys[uniq[map[b]]] == keys[s * B + b], name);           // never merges unequal slots
        }
        for (int k = 0; k < U; k++) CHECK(hit[k] >= 1, name);             // onto 0 .. U-1
        for (int a = 0; a < B; a++)
            for (int b = 0; b < B; b++) CHECK((map[a] == map[b]) == (keys[s * B + a] == keys[s * B + b]), name);
    }
}

int main() {
    sides_and_check("all equal", {4, 4, 4, 4, 4, 4, 4, 4}, 1, 1);
    sides_and_check("all distinct", {9, 8, 7, 6, 5, 4, 3, 2}, 4, 4);
    sides_and_check("side 0 constant", {1, 1, 1, 1, 2, 3, 4, 5}, 1, 4);
    sides_and_check("side 1 constant", {2, 3, 4, 5, 1, 1, 1, 1}, 4, 1);
    sides_and_check("B = 1, equal", {3, 3}, 1, 1);
    sides_and_check("B = 1, distinct", {3, 4}, 1, 1);
    // every representative of side 1 sits on side 0
    sides_and_check("representatives on the other side", {0, 0, 1, 2, 1, 1, 2, 0, 0, 2}, 3, 3);
    sides_and_check("swapped sides", {0, 0, 1, 2, 1, 2, 0, 0}, 3, 3);
    sides_and_check("side 1 constant, held by side 0 too", {5, 6, 7, 6, 6, 6}, 3, 1);
    {   // tables that are not representative tables are refused, not used
        int32_t uniq[2], map[2];
        const int32_t forward[4] = {0, 2, 2, 3}, chain[4] = {0, 0, 1, 3}, negative[4] = {0, 1, -1, 3}, fine[4] = {0, 0, 0, 3};
        CHECK(a3r::dedup_group_side(forward, 2, 0, uniq, map) == -1, "rep > slot");
        CHECK(a3r::dedup_group_side(chain, 2, 1, uniq, map) == -1, "rep of a non-representative");
        CHECK(a3r::dedup_group_side(negative, 2, 1, uniq, map) == -1, "negative rep");
        CHECK(a3r::dedup_group_side(fine, 0, 0, uniq, map) == -1, "no slots");
        CHECK(a3r::dedup_group_side(fine, 2, 2, uniq, map) == -1, "no such side");
        CHECK(a3r::dedup_group_side(fine, 2, 0, uniq, map) == 1 && a3r::dedup_group_side(fine, 2, 1, uniq, map) == 2, "a good table");
    }
    if (!failures) std::printf("ok\n");
    return failures;
}
