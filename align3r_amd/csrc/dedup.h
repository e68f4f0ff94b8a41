// Duplicate inputs of one pair-forward batch (dedup.hip finds them on the device, model.hip runs the frame-only parts of the plan on
// the distinct ones).  This header is plain C++ -- no HIP types -- so that the host grouping below can be tested by a stand-alone
// CPU program (tests/test_dedup_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>

namespace a3r {

// Host grouping.  rep[s] (s < n) is the representative of slot s: the smallest slot whose content equals slot s's, so rep[s] <= s
// and rep[rep[s]] == rep[s].  Writes the distinct slots in ascending order to uniq[0..U) and the row of each slot's representative
// in that list to map[0..n) (a surjection onto 0..U-1 with map[uniq[k]] == k), and returns U.  Returns -1 and writes nothing
// meaningful when rep is not such a table (the caller then runs the plan without merging anything).
inline int dedup_group(const int32_t* rep, int n, int32_t* uniq, int32_t* map) {
    if (!rep || !uniq || !map || n <= 0) return -1;
    int U = 0;
    for (int s = 0; s < n; s++) {
        const int32_t r = rep[s];
        if (r < 0 || r > s) return -1;
        if (r == s) {
            uniq[U] = s;
            map[s] = U++;
        } else {
            if (rep[r] != r) return -1;
            map[s] = map[r];
        }
    }
    return U;
}

// One side of the batch.  rep is the table above over the 2 B slots of the first kind (img1 then img2); side s holds the slots
// [s B, (s + 1) B).  Writes the side's distinct contents to uniq[0..U), each as the FIRST SLOT OF THAT SIDE holding it (so
// s B <= uniq[k] < (s + 1) B even when the representative sits on the other side; ascending), and for every slot b < B of the side
// its row in that list to map[0..B) (map[uniq[k] - s B] == k), and returns U.  The DPT heads run their frame-only branch on these
// (model.hip).  Returns -1 when rep is not a representative table.
inline int dedup_group_side(const int32_t* rep, int B, int s, int32_t* uniq, int32_t* map) {
    if (!rep || !uniq || !map || B <= 0 || s < 0 || s > 1) return -1;
    const int base = s * B;
    int U = 0;
    for (int b = 0; b < B; b++) {
        const int32_t r = rep[base + b];
        if (r < 0 || r > base + b || rep[r] != r) return -1;
        int k = 0;
        while (k < U && rep[uniq[k]] != r) k++;
        if (k == U) uniq[U++] = base + b;
        map[b] = k;
    }
    return U;
}

// Entries.  map_img / map_pd [2 B] are dedup_group's maps of the two kinds: the row of every slot's image / depth prior among the
// distinct ones.  What the decoder computes before its first cross-attention product depends on the slot's (image, prior) pair --
// its entry -- and on its side.  For side s (slots [s B, (s + 1) B)) writes the distinct entries to ent[s B + e], e < U[s], each as
// the FIRST SLOT OF THAT SIDE holding it (ascending; the representatives of its image and prior may sit on the other side), and the
// entry of slot b of the side to map_e[s B + b] (map_e[ent[s B + e]] == e).  Both lists are then padded to Um = max(U[0], U[1]) by
// repeating the side's last entry, so that grouped launches keep one row count and compute copies of real rows only.  Returns Um,
// or -1 when a row is outside 0 .. 2 B - 1 or an argument is missing.
inline int dedup_group_entries(const int32_t* map_img, const int32_t* map_pd, int B, int32_t* ent, int32_t* map_e, int* U) {
    if (!map_img || !map_pd || !ent || !map_e || !U || B <= 0) return -1;
    for (int i = 0; i < 2 * B; i++)
        if (map_img[i] < 0 || map_img[i] >= 2 * B || map_pd[i] < 0 || map_pd[i] >= 2 * B) return -1;
    for (int s = 0; s < 2; s++) {
        const int base = s * B;
        int u = 0;
        for (int b = 0; b < B; b++) {
            int e = 0;
            while (e < u && (map_img[ent[base + e]] != map_img[base + b] || map_pd[ent[base + e]] != map_pd[base + b])) e++;
            if (e == u) ent[base + u++] = base + b;
            map_e[base + b] = e;
        }
        U[s] = u;
    }
    const int Um = U[0] > U[1] ? U[0] : U[1];
    for (int s = 0; s < 2; s++)
        for (int e = U[s]; e < Um; e++) ent[s * B + e] = ent[s * B + U[s] - 1];
    return Um;
}

// ---- device side (dedup.hip).  An item of the first kind is one image [3, H, W] -- or, for the decode call, one frame's encoder
// features [N, E] --, one of the second kind a pred_depth map [H, W, 3]: words_a / words_pd 32-bit words each, multiples of 4.  Slot s < 4 B of a call is item s % B of group s / B, the groups being img1, img2, pd1, pd2; slots 0 .. 2 B - 1
// are the image kind, 2 B .. 4 B - 1 the depth-prior kind, and a representative is looked for inside a slot's own kind only.
constexpr int DEDUP_MAX_SLOTS = 2048;        // 4 B at most; larger batches run without merging
// device words: keys [DEDUP_MAX_SLOTS][2] of 64 bits, then rep [DEDUP_MAX_SLOTS] (index inside the kind) and the mismatch flag
constexpr size_t DEDUP_KEY_BYTES = (size_t)DEDUP_MAX_SLOTS * 16;
constexpr size_t DEDUP_REP_INTS = DEDUP_MAX_SLOTS + 1;
// slots [first, 4 B): first = 0 with items of the first kind, 2 B without (a decode call that does not look at its features).  const_key: every key is zero, so the
// grouping rests on the verification alone (a3r_model_set_dedup mode 2).  Enqueues: clear, key kernel, representative kernel,
// verify kernel; rep_flag[4 B] ends up nonzero when some slot differs from its representative in any bit.
int dedup_find(const float* img1, const float* img2, const float* pd1, const float* pd2, int B, long words_a, long words_pd, int first,
               bool const_key, void* keys, int32_t* rep_flag, void* stream);

// ---- the plan's ops on distinct items (elementwise.hip)
// a3r_patchify of the U items uniq[k] (device, indices inside the kind) of the 2 B items of img_a followed by img_b
int patchify_indexed(const float* img_a, const float* img_b, const int32_t* uniq, int U, int B, float* cols, int C, int H, int W, long sb,
                     long sc, long sy, long sx, void* stream);
// dst[(s * N + n) * C + c] = src[(map[s] * N + n) * C + c] for the slots s < S (map on the device); C a multiple of 4
int gather_rows(const float* src, float* dst, const int32_t* map, int S, int N, int C, void* stream);
// whether a3r_attention_fh2_mapped runs the kernel form that takes image maps (attention_fh2.hip; not under A3R_ATTN=v1)
bool attention_fh2_takes_maps();
// The second conv of refinenet1.resConfUnit1 on distinct frames (a3r.h: a3r_combine_resid_fh2 is the same with a C signature)
int combine_resid_fh2(const float* c, const float* r0, const float* p2, const int32_t* map, float* s, void* sr2, int S, long P, int C,
                      float scale, unsigned* absmax, void* stream);
// the same with p2 = the bilinear 2x (a3r_upsample2x, cropped to Hc x Wc) of x [S, H, W, C] made on the fly; P = Hc Wc
int upsample2x_combine_fh2(const float* x, const float* c, const float* r0, const int32_t* map, float* s, void* sr2, int S, int H, int W,
                           int C, int Hc, int Wc, float scale, unsigned* absmax, void* stream);

}  // namespace a3r
