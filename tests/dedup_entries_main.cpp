// Stand-alone CPU program for tests/test_dedup_entries_cpu.py: the entry grouping of align3r_amd/csrc/dedup.h (the two kinds' slot
// maps -> each side's distinct (image, depth prior) entries, padded to one count, which decoder block 0 runs its frame-only half on),
// built with -fsanitize=address,undefined.  Prints one line per failed check; exit status = number of failures.
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

// dedup_group's map of one kind from its keys: the row of each slot's content among the distinct ones, in order of first appearance
static std::vector<int32_t> map_of(const std::vector<int>& keys) {
    std::vector<int32_t> rep(keys.size()), uniq(keys.size()), map(keys.size());
    for (size_t s = 0; s < keys.size(); s++) {
        size_t r = 0;
        while (keys[r] != keys[s]) r++;
        rep[s] = (int32_t)r;
    }
    if (a3r::dedup_group(rep.data(), (int)keys.size(), uniq.data(), map.data()) < 1) failures++;
    return map;
}

// img, pd: the keys of side 0's B slots, then side 1's
static void entries_and_check(const char* name, const std::vector<int>& img, const std::vector<int>& pd, int want_u0, int want_u1) {
    const int B = (int)img.size() / 2;
    const std::vector<int32_t> mi = map_of(img), mp = map_of(pd);
    // exactly 2 B entries each, so that the sanitizer sees a write past either list
    std::vector<int32_t> ent(2 * B, -7), map_e(2 * B, -7);
    int U[2] = {-7, -7};
    const int Um = a3r::dedup_group_entries(mi.data(), mp.data(), B, ent.data(), map_e.data(), U);
    CHECK(U[0] == want_u0 && U[1] == want_u1, name);
    CHECK(Um == (want_u0 > want_u1 ? want_u0 : want_u1), name);
    if (Um < 1 || Um > B) return;
    auto same = [&](int a, int b) { return img[a] == img[b] && pd[a] == pd[b]; };       // the entry is the PAIR
    for (int s = 0; s < 2; s++) {
        if (U[s] < 1 || U[s] > Um) return;
        std::vector<int> hit(U[s], 0);
        for (int e = 0; e < Um; e++) {
            CHECK(ent[s * B + e] >= s * B && ent[s * B + e] < (s + 1) * B, name);       // a slot of the side itself
            if (ent[s * B + e] < s * B || ent[s * B + e] >= (s + 1) * B) return;
        }
        for (int e = 0; e < U[s]; e++) {
            if (e) CHECK(ent[s * B + e - 1] < ent[s * B + e], name);                    // ascending
            CHECK(map_e[ent[s * B + e]] == e, name);
            for (int t = s * B; t < ent[s * B + e]; t++) CHECK(!same(t, ent[s * B + e]), name);      // the first slot of the side holding it
        }
        for (int e = U[s]; e < Um; e++) CHECK(ent[s * B + e] == ent[s * B + U[s] - 1], name);       // padding repeats the last entry
        for (int b = 0; b < B; b++) {
            const int e = map_e[s * B + b];
            CHECK(e >= 0 && e < U[s], name);
            if (e < 0 || e >= U[s]) return;
            hit[e]++;
            CHECK(same(ent[s * B + e], s * B + b), name);                               // never merges unequal slots
        }
        for (int e = 0; e < U[s]; e++) CHECK(hit[e] >= 1, name);
        for (int a = 0; a < B; a++)
            for (int b = 0; b < B; b++) CHECK((map_e[s * B + a] == map_e[s * B + b]) == same(s * B + a, s * B + b), name);
    }
    for (int e = Um; e < B; e++) CHECK(ent[e] == -7 && ent[B + e] == -7, name);          // nothing written behind the padded lists
}

int main() {
    entries_and_check("all distinct", {0, 1, 2, 3, 4, 5}, {0, 1, 2, 3, 4, 5}, 3, 3);
    entries_and_check("all equal", {4, 4, 4, 4, 4, 4}, {9, 9, 9, 9, 9, 9}, 1, 1);
    entries_and_check("B = 1", {3, 3}, {1, 2}, 1, 1);
    // one image with two priors: two entries; one prior with two images: two entries
    entries_and_check("same image, two priors", {0, 0, 0, 1, 1, 1}, {0, 1, 0, 2, 2, 2}, 2, 1);
    entries_and_check("same prior, two images", {0, 1, 0, 2, 2, 2}, {5, 5, 5, 6, 6, 6}, 2, 1);
    entries_and_check("both kinds repeat, the pairs do not", {0, 0, 1, 1, 2, 2, 3, 3}, {0, 1, 0, 1, 2, 3, 2, 3}, 4, 4);
    // U_0 != U_1: the shorter list is padded
    entries_and_check("fan", {0, 0, 0, 1, 2, 3}, {0, 0, 0, 1, 2, 3}, 1, 3);
    entries_and_check("fan, sides swapped", {1, 2, 3, 3, 0, 0, 0, 0}, {1, 2, 3, 3, 0, 0, 0, 0}, 3, 1);
    // every image and prior of side 1 has its representative on side 0
    entries_and_check("representatives on the other side", {0, 0, 1, 2, 1, 1, 2, 0, 0, 2}, {0, 0, 1, 2, 1, 1, 2, 0, 0, 2}, 3, 3);
    entries_and_check("chain", {0, 1, 2, 1, 2, 3}, {0, 1, 2, 1, 2, 3}, 3, 3);
    {   // malformed tables are refused, not used
        int32_t ent[4], map_e[4];
        int U[2];
        const int32_t fine[4] = {0, 0, 1, 1}, negative[4] = {0, -1, 1, 1}, large[4] = {0, 4, 1, 1};
        CHECK(a3r::dedup_group_entries(fine, negative, 2, ent, map_e, U) == -1, "negative row");
        CHECK(a3r::dedup_group_entries(large, fine, 2, ent, map_e, U) == -1, "row past 2 B - 1");
        CHECK(a3r::dedup_group_entries(fine, fine, 0, ent, map_e, U) == -1, "no slots");
        CHECK(a3r::dedup_group_entries(nullptr, fine, 2, ent, map_e, U) == -1, "missing table");
        CHECK(a3r::dedup_group_entries(fine, fine, 2, ent, map_e, U) == 1 && U[0] == 1 && U[1] == 1, "a good table");
    }
    if (!failures) std::printf("ok\n");
    return failures;
}
