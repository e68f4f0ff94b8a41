// Stand-alone CPU program for tests/test_fh2_chooser_cpu.py: the tile table and the tile chooser of the fh2 GEMM
// (align3r_amd/csrc/fh2_chooser.h) on the two shape lists of tools/bench_fh2.py -- the launches of the bench's 42-pair step that run
// on distinct rows and those that run on every slot -- built with -fsanitize=address,undefined.  Checks the tile counts and waves of
// every tile shape, the bounds of a partial wave's cost, that the tile chosen for a shape is within 2 % of the fastest one in the
// committed measurements (the us columns are the table of profiles/fh2_tiles.json; 2 %: the same kernel on the same shape, timed twice
// in that table as the chooser's choice and as the forced tile, differs by up to 1.3 %), and that a forced tile out of range is
// refused.  Prints one line per failed check; exit status = failures.
#include "fh2_chooser.h"
#include <cstdio>

static int failures = 0;
#define CHECK(cond, name)                                        \
    do {                                                         \
        if (!(cond)) {                                           \
            std::printf("FAILED %s: %s\n", name, #cond);         \
            failures++;                                          \
        }                                                        \
    } while (0)

struct Shape {
    const char* name;
    int M, N, K, groups;
    long tiles[4];      // expected tile counts of tiles 0..3, worked out by hand: ceil(M / bm) ceil(N / bn) groups
    double us[3];       // measured us per launch of tiles 0, 1, 2
    int parent;         // what whole waves alone chose (the chooser before the fit)
};

// bm x bn: 256x128, 128x64, 128x128, 256x128.  12288 = 96 x 128 = 48 x 256; 11520 = 90 x 128 = 45 x 256; 32256 = 252 x 128 = 126 x 256
static const Shape kShapes[] = {
    {"enc qkv", 12288, 3072, 1024, 1, {1152, 4608, 2304, 1152}, {213.2, 227.6, 190.5}, 2},
    {"enc proj", 12288, 1024, 1024, 1, {384, 1536, 768, 384}, {85.0, 78.8, 68.7}, 1},
    {"enc fc1", 12288, 4096, 1024, 1, {1536, 6144, 3072, 1536}, {265.8, 299.8, 250.6}, 2},
    {"enc fc2", 12288, 1024, 4096, 1, {384, 1536, 768, 384}, {274.6, 287.4, 242.1}, 1},
    {"pc qkv", 12288, 2304, 768, 1, {864, 3456, 1728, 864}, {134.0, 135.6, 115.1}, 2},
    {"pc proj/zc", 12288, 768, 768, 1, {288, 1152, 576, 288}, {60.8, 49.4, 48.7}, 1},
    {"pc fc1", 12288, 3072, 768, 1, {1152, 4608, 2304, 1152}, {168.8, 177.2, 148.9}, 2},
    {"pc fc2", 12288, 768, 3072, 1, {288, 1152, 576, 288}, {204.8, 173.5, 168.3}, 1},
    {"dec_embed", 12288, 768, 1024, 1, {288, 1152, 576, 288}, {77.5, 63.7, 62.3}, 1},
    {"blk0 qkv", 11520, 2304, 768, 2, {1620, 6480, 3240, 1620}, {236.8, 251.6, 209.1}, 2},
    {"blk0 proj", 11520, 768, 768, 2, {540, 2160, 1080, 540}, {96.0, 87.7, 81.1}, 2},
    {"dec proj/q/cproj", 32256, 768, 768, 2, {1512, 6048, 3024, 1512}, {215.0, 260.6, 210.2}, 2},
    {"dec kv", 32256, 1536, 768, 2, {3024, 12096, 6048, 3024}, {422.8, 495.4, 403.1}, 2},
    {"dec qkv", 32256, 2304, 768, 2, {4536, 18144, 9072, 4536}, {621.9, 726.5, 589.7}, 2},
    {"dec fc1", 32256, 3072, 768, 2, {6048, 24192, 12096, 6048}, {830.5, 959.2, 789.4}, 2},
    {"dec fc2", 32256, 768, 3072, 2, {1512, 6048, 3024, 1512}, {739.5, 953.1, 740.2}, 2},
};

int main() {
    using namespace a3r;
    CHECK(kFh2NumTiles == 4 && fh2_slots(0) == 256 && fh2_slots(1) == 512 && fh2_slots(2) == 512 && fh2_slots(3) == 256, "slots");
    for (const Shape& s : kShapes) {
        for (int t = 0; t < kFh2NumTiles; t++) {
            CHECK(fh2_tile_count(t, s.M, s.N, s.groups) == s.tiles[t], s.name);
            // every tile of the launch sits in exactly one wave, and no wave but the last is partial
            const long n = fh2_tile_count(t, s.M, s.N, s.groups), w = fh2_waves(t, s.M, s.N, s.groups);
            CHECK(w * fh2_slots(t) >= n && (w - 1) * fh2_slots(t) < n, s.name);
            if (t == 3) continue;       // the lab tile has no rate
            // by whole waves a partial wave costs a full one; fitted, never more than that and never less than its share of one
            const double per_wave = (double)kFh2Tiles[t].bm * kFh2Tiles[t].bn * kFh2Tiles[t].occ / kFh2Tiles[t].eff;
            const double whole = fh2_tile_cost(t, s.M, s.N, s.groups, false), fitted = fh2_tile_cost(t, s.M, s.N, s.groups, true);
            CHECK(whole >= (double)w * per_wave * (1 - 1e-12) && whole <= (double)w * per_wave * (1 + 1e-12), s.name);
            CHECK(fitted <= whole && fitted >= (double)n / fh2_slots(t) * per_wave * (1 - 1e-12), s.name);
            if (kFh2Tiles[t].occ == 1) CHECK(fitted == whole, s.name);
        }
        const int t = choose_fh2_tile(s.M, s.N, s.groups, -1, true);
        CHECK(t >= 0 && t <= 2, s.name);
        if (t < 0 || t > 2) continue;
        double best = s.us[0];
        for (int i = 1; i < 3; i++)
            if (s.us[i] < best) best = s.us[i];
        if (!(s.us[t] <= 1.02 * best)) std::printf("%s: chose tile %d at %.1f us, the fastest measured takes %.1f us\n", s.name, t, s.us[t], best);
        CHECK(s.us[t] <= 1.02 * best, s.name);
        CHECK(choose_fh2_tile(s.M, s.N, s.groups, -1, false) == s.parent, s.name);      // the conv path's model is the earlier one
        for (int f = 0; f < kFh2NumTiles; f++) CHECK(choose_fh2_tile(s.M, s.N, s.groups, f, false) == f, s.name);      // a forced tile is taken
        CHECK(choose_fh2_tile(s.M, s.N, s.groups, 4, true) == t && choose_fh2_tile(s.M, s.N, s.groups, -3, true) == t &&
                  choose_fh2_tile(s.M, s.N, s.groups, 1 << 30, true) == t,
              "a forced tile out of range is refused");
    }
    // ragged shapes round up; one row is one tile
    CHECK(fh2_tile_count(1, 129, 65, 1) == 4 && fh2_tile_count(2, 129, 129, 3) == 12 && fh2_tile_count(0, 1, 1, 1) == 1, "ragged");
    if (!failures) std::printf("ok\n");
    return failures;
}
