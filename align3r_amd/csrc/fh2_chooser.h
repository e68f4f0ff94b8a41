// Tile table and tile chooser of the fh2 GEMM (gemm_fh2.hip), plain C++ so that tests/fh2_chooser_main.cpp can run it on the CPU.
// A launch of n tiles on S resident workgroup slots (256 CUs x occ) runs n / S full waves of workgroups and, when S does not divide
// n, a last partial one; a tile shape's cost is its waves times the output area a wave covers, divided by the shape's rate relative
// to the 128x128 tile.  The eff entries and the cost of a partial wave are fitted to the per-shape table of tools/bench_fh2.py --lists
// (profiles/fh2_tiles.json), not derived.
#pragma once

namespace a3r {

struct Fh2Tile { int bm, bn, occ; double eff; };
// 0: 256x128, 16 waves (4x4), 3 stages of 48 KB, one workgroup per CU.   1: 128x64, 8 waves (4x2), two workgroups per CU, for launches
// whose tile count quantises badly.   2: 128x128, 8 waves (2x4), 2 stages of 32 KB, TWO workgroups per CU -- one workgroup's epilogue
// (and its barrier waits) run under the other's matrix work: +4 % over tile 0 on the forward's shapes although it moves 1.33x the
// operand bytes per flop (same-call A/B, tools/bench_fh2.py).   3: 256x128 with 8 waves of 64x64 (a third fewer LDS fragment reads,
// 224 VGPRs): 17 % slower (two waves per SIMD hide neither the barrier nor the longer per-wave epilogue); kept for A3R_FH2_TILE=3.
constexpr int kFh2NumTiles = 4;
constexpr int kFh2CUs = 256;
static const Fh2Tile kFh2Tiles[kFh2NumTiles] = {{256, 128, 1, 0.96}, {128, 64, 2, 0.82}, {128, 128, 2, 1.0}, {256, 128, 1, 0.0}};
// A last wave that fills at most half of the slots of a shape with two workgroups per CU: a workgroup that has its CU to itself runs
// nearly twice as fast as one that shares it -- measured 0.54 of a full wave's time for the 128x128 tile after one full wave, 0.49 and
// 0.77 after four, so 1.5 waves of it beat 3 waves of the 128x64 tile by 12 - 16 %.  With one workgroup per CU (tiles 0 and 3) a
// partial wave takes as long as a full one.
constexpr double kFh2HalfWave = 0.55;

inline long fh2_tile_count(int t, int M, int N, int groups) {
    return (long)((M + kFh2Tiles[t].bm - 1) / kFh2Tiles[t].bm) * ((N + kFh2Tiles[t].bn - 1) / kFh2Tiles[t].bn) * groups;
}
inline long fh2_slots(int t) { return (long)kFh2CUs * kFh2Tiles[t].occ; }
inline long fh2_waves(int t, int M, int N, int groups) { return (fh2_tile_count(t, M, N, groups) + fh2_slots(t) - 1) / fh2_slots(t); }
// in output elements at the 128x128 tile's rate.  fitted: with the measured cost of a half-empty last wave; without, every started
// wave counts as a full one (the model the convolutions keep: their shapes are not in the table)
inline double fh2_tile_cost(int t, int M, int N, int groups, bool fitted) {
    const long n = fh2_tile_count(t, M, N, groups), slots = fh2_slots(t), rem = n % slots;
    double waves = (double)(n / slots);
    if (rem) waves += (fitted && kFh2Tiles[t].occ > 1 && 2 * rem <= slots) ? kFh2HalfWave : 1.0;
    return waves * kFh2Tiles[t].bm * kFh2Tiles[t].bn * kFh2Tiles[t].occ / kFh2Tiles[t].eff;
}

// forced: the developer override (A3R_FH2_TILE), taken when it names a tile, else ignored.  fitted: see fh2_tile_cost (the linear
// path).  Tile 3 is a lab tile and never chosen.  Ties go to the lower index.
inline int choose_fh2_tile(int M, int N, int groups, int forced, bool fitted) {
    if (forced >= 0 && forced < kFh2NumTiles) return forced;
    int best_t = 0;
    double best = 1e300;
    for (int t = 0; t < 3; t++) {
        const double cost = fh2_tile_cost(t, M, N, groups, fitted);
        if (cost < best * 0.999) { best = cost; best_t = t; }
    }
    return best_t;
}

}  // namespace a3r
