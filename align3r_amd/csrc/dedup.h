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

// ---- frames kept across calls (a3r_model_set_frame_cache).  The device looks every distinct image of a call up among the stored
// ones (frame_cache_lookup below: the key proposes, a bitwise comparison decides); this table is the host's side of it: which
// entries hold a frame, and how recently each was used.  Plain C++ as well (tests/test_frame_cache_cpu.py).
constexpr int FC_MAX_ENTRIES = 256;          // entries at most (their validity travels to the lookup kernel as a bit mask)
struct FrameCacheMask { uint32_t w[FC_MAX_ENTRIES / 32]; };

struct FrameCacheTable {
    int cap = 0;
    uint64_t clock = 0;
    uint64_t stamp[FC_MAX_ENTRIES] = {};     // clock of the entry's last use; 0 = the entry is free
    void reset(int capacity) {
        cap = capacity < 0 ? 0 : capacity > FC_MAX_ENTRIES ? FC_MAX_ENTRIES : capacity;
        flush();
    }
    void flush() {
        clock = 0;
        for (uint64_t& s : stamp) s = 0;
    }
    int size() const {
        int n = 0;
        for (int e = 0; e < cap; e++) n += stamp[e] != 0;
        return n;
    }
    FrameCacheMask mask() const {
        FrameCacheMask k = {};
        for (int e = 0; e < cap; e++)
            if (stamp[e]) k.w[e / 32] |= 1u << (e % 32);
        return k;
    }
    // One call.  hit[k] (k < U) is the entry whose frame equals the call's k-th distinct image, or -1.  Writes to ent[k] the entry
    // image k is read from (a hit) or stored to (a miss), or -1 for a miss that is not stored: a miss takes the free entry of the
    // smallest index, then the least recently used entry, never one this call hit or filled, and when those run out the remaining
    // misses (in list order) are not stored.  n[0..2] = hits, misses, evictions.  Every entry the call touches becomes the most
    // recently used, in list order.  Returns 0, or -1 and changes nothing when hit is not such a list (an index out of range, a
    // free entry, or one entry named twice); the caller then runs without the cache.
    int assign(const int32_t* hit, int U, int32_t* ent, int* n) {
        if (!hit || !ent || !n || U < 0) return -1;
        bool used[FC_MAX_ENTRIES] = {};
        for (int k = 0; k < U; k++) {
            const int32_t e = hit[k];
            if (e < -1 || e >= cap) return -1;
            if (e >= 0) {
                if (!stamp[e] || used[e]) return -1;
                used[e] = true;
            }
        }
        n[0] = n[1] = n[2] = 0;
        for (int k = 0; k < U; k++) {
            int e = hit[k];
            if (e >= 0) n[0]++;
            else {
                n[1]++;
                for (int c = 0; c < cap && e < 0; c++)
                    if (!stamp[c] && !used[c]) e = c;
                if (e < 0) {
                    for (int c = 0; c < cap; c++)
                        if (!used[c] && (e < 0 || stamp[c] < stamp[e])) e = c;
                    if (e >= 0) n[2]++;
                }
                if (e >= 0) used[e] = true;
            }
            ent[k] = e;
        }
        for (int k = 0; k < U; k++)
            if (ent[k] >= 0) stamp[ent[k]] = ++clock;
        return 0;
    }
};

// The caller's storage as `cap` entries, one array per field: keys [cap][2] of 64 bits, the statistics words [cap][FC_STAT_WORDS]
// of the call that computed the entry, the lookup's mismatch flags [cap][2 B], the images [cap][words_img] and their enc_norm rows
// [cap][words_feat] (both multiples of 4 words).  cap = 0: the storage holds no entry of this size.
constexpr int FC_STAT_WORDS = 1024;
constexpr int FC_MAX_PAIRS = 512;            // larger calls run without the cache
struct FrameCacheLayout {
    int cap; long words_img, words_feat;
    char *keys, *stats, *flags, *img, *feat;
};
inline size_t frame_cache_entry_bytes(long words_img, long words_feat) {
    return 16 + (size_t)FC_STAT_WORDS * 4 + (size_t)4 * FC_MAX_PAIRS * 2 + ((size_t)words_img + (size_t)words_feat) * 4;
}
inline FrameCacheLayout frame_cache_layout(void* base, size_t bytes, long words_img, long words_feat) {
    const size_t n = bytes / frame_cache_entry_bytes(words_img, words_feat);
    const int cap = base ? (int)(n > (size_t)FC_MAX_ENTRIES ? (size_t)FC_MAX_ENTRIES : n) : 0;
    char* p = static_cast<char*>(base);
    FrameCacheLayout l = {cap, words_img, words_feat, p, nullptr, nullptr, nullptr, nullptr};
    l.stats = l.keys + (size_t)cap * 16;
    l.flags = l.stats + (size_t)cap * FC_STAT_WORDS * 4;
    l.img = l.flags + (size_t)cap * 4 * FC_MAX_PAIRS * 2;
    l.feat = l.img + (size_t)cap * words_img * 4;
    return l;
}
// device side (dedup.hip), queued after dedup_find on the same stream.  keys / rep: dedup_find's; for every slot s < 2 B that is
// its own representative, hit[s] = the valid entry (mask) whose key and whose every bit equal the slot's image, else -1; -1 for the
// other slots.  B <= FC_MAX_PAIRS.
int frame_cache_lookup(const float* img1, const float* img2, int B, const void* keys, const int32_t* rep, const FrameCacheLayout& l,
                       const FrameCacheMask& mask, int32_t* hit, void* stream);
// The call's U distinct images uniq[k] (device lists, as below): rows[k] = the stored rows of entry ent[k] where miss[k] < 0 (a
// hit), else fresh[miss[k]] -- the enc_norm rows of the miss[k]-th encoded image -- which, with image and key, also go to entry
// ent[k] when that is >= 0.
int frame_cache_exchange(const float* img1, const float* img2, int B, const void* keys, const FrameCacheLayout& l, const int32_t* uniq,
                         const int32_t* ent, const int32_t* miss, int U, const float* fresh, float* rows, void* stream);

// ---- frame products kept across calls (a3r_model_set_frame_products): what the plan makes from one depth prior alone -- the
// outputs z_0 .. z_n of the zero-convs -- in a second storage of the same layout (the `feat` of an entry: the levels' [N, D] rows
// one after the other), with a FrameCacheTable of its own and the lookup above on the pred_depth slots.
// The sites of the ops a call may skip, which do not form one range: a bit per statistics word.
struct SiteMask {
    uint32_t w[FC_STAT_WORDS / 32] = {};
    void add(int lo, int hi) {          // sites [lo, hi), clipped to the words there are
        for (int i = lo < 0 ? 0 : lo; i < hi && i < FC_STAT_WORDS; i++) w[i / 32] |= 1u << (i % 32);
    }
    bool has(int i) const { return i >= 0 && i < FC_STAT_WORDS && ((w[i / 32] >> (i % 32)) & 1u); }
};
// The lists of one call, after FrameCacheTable::assign.  hit[k] (k < U) is the lookup's answer for the call's k-th distinct prior
// (an entry, or -1).  Writes miss[k] = -1 for a hit, else the prior's row j among the n_miss priors the branch runs on, whose
// slots uniq[k] go to uniq_miss[j]; and for each of the n rows row[i] (a distinct prior each) where the gather-add pass finds its
// z: src[i] = the entry of a hit, or ~j (negative) for the j-th fresh row block.  *n_store = the misses that have an entry to go
// to (ent[k] >= 0).  Returns n_miss, or -1 for a row outside 0 .. U - 1 or a missing argument.
inline int prior_lists(const int32_t* hit, const int32_t* ent, const int32_t* uniq, int U, int32_t* miss, int32_t* uniq_miss,
                       const int32_t* row, int n, int32_t* src, int* n_store) {
    if (!hit || !ent || !uniq || !miss || !uniq_miss || !row || !src || !n_store || U <= 0 || n < 0) return -1;
    int n_miss = 0;
    *n_store = 0;
    for (int k = 0; k < U; k++) {
        if (hit[k] >= 0) { miss[k] = -1; continue; }
        uniq_miss[n_miss] = uniq[k];
        miss[k] = n_miss++;
        *n_store += ent[k] >= 0;
    }
    for (int i = 0; i < n; i++) {
        const int32_t k = row[i];
        if (k < 0 || k >= U) return -1;
        src[i] = miss[k] < 0 ? hit[k] : ~miss[k];
    }
    return n_miss;
}
// Device side.  For every distinct item k < U that was not found (miss[k] >= 0) and has an entry (ent[k] >= 0): with `fresh`, the
// part_words words of fresh row block miss[k] go to words [part_off, part_off + part_words) of the entry's `feat`; without, the
// item itself (slot uniq[k] of img1 / img2) and its key go to the entry.
int frame_cache_store(const float* img1, const float* img2, int B, const void* keys, const FrameCacheLayout& l, const int32_t* uniq,
                      const int32_t* ent, const int32_t* miss, int U, const float* fresh, long part_off, long part_words, void* stream);
// The statistics words `sites` of the call, for any of the stores: estats [cap][FC_STAT_WORDS] are the entries' words (a
// FrameCacheLayout's `stats`, or the head products' words of one side).  The call's words are stored with every entry it filled
// (miss[k] >= 0, ent[k] >= 0), then raised to the largest word of the entries it read (miss[k] < 0).
int stats_sites_words(unsigned* estats, int cap, const int32_t* ent, const int32_t* miss, int U, unsigned* stats, const SiteMask& sites,
                      void* stream);
// (the gather-add pass that reads src is a3r_gather_add_rows_src of a3r.h: a3r_gather_add_rows whose rows a come from two places)

// ---- head products kept across calls (a3r_model_set_head_products): what the DPT head of side s makes from one frame alone -- r0,
// the output of layer_rn[0], and c, the bias-only output of resConfUnit1's second conv, [16 N, F] fp32 each -- in a third storage
// indexed by the FRAME CACHE's entries: no lookup of its own, the image lookup already says which entry a distinct image is.  The
// host keeps one valid bit per (entry, side).
struct HeadBits {
    uint8_t b[FC_MAX_ENTRIES] = {};
    void flush() { for (uint8_t& x : b) x = 0; }                 // with every flush or reset of the frame cache's table
    void clear(int e) { if (e >= 0 && e < FC_MAX_ENTRIES) b[e] = 0; }      // the frame cache filled or replaced entry e
    bool has(int e, int s) const { return e >= 0 && e < FC_MAX_ENTRIES && ((b[e] >> s) & 1); }
    void set(int e, int s) { if (e >= 0 && e < FC_MAX_ENTRIES) b[e] |= (uint8_t)(1u << s); }
    int count() const { int n = 0; for (uint8_t x : b) n += (x & 1) + ((x >> 1) & 1); return n; }
};
// The storage as `cap` entries: the statistics words [2][cap][FC_STAT_WORDS] (side-major: one side's are an array [cap][FC_STAT_WORDS], as a frame
// cache's are), then the rows [cap][2 sides][r0, c][words] (words = 16 N F, a multiple of 64).
inline size_t head_products_entry_bytes(long words) { return (size_t)2 * FC_STAT_WORDS * 4 + (size_t)4 * words * 4; }
struct HeadStore {
    int cap; long words;
    char *stats, *rows;
    long stride() const { return 4 * words; }                  // floats from one entry's block to the next entry's
    const float* r0(int s) const { return reinterpret_cast<const float*>(rows) + (size_t)(2 * s) * words; }
    const float* c(int s) const { return reinterpret_cast<const float*>(rows) + (size_t)(2 * s + 1) * words; }
    unsigned* side_words(int s) const { return reinterpret_cast<unsigned*>(stats) + (size_t)s * cap * FC_STAT_WORDS; }      // [cap][FC_STAT_WORDS]
};
inline HeadStore head_store_layout(void* base, int cap, long words) {
    char* p = static_cast<char*>(base);
    return {base ? cap : 0, words, p, p + (size_t)cap * 2 * FC_STAT_WORDS * 4};
}
// The lists of one side of one call, after FrameCacheTable::assign and the clearing of the replaced entries' bits.  The side has U
// distinct frames; frame k is the call's distinct image row[k] (< n_img), whose entry in the frame cache is ent[row[k]] (-1: it
// has none) and which the lookup found there when miss[row[k]] < 0.  A frame is STORED when it was found and bit (entry, side) is
// set.  Writes for every frame k: hent[k] = its entry or -1, hmiss[k] = -1 when stored, else its row j among the n_fresh frames the
// branch runs on, whose slots uniq[k] go to uniq_fresh[j]; and for every slot b < B of the side (frame map[b]) the signed source
// of its c and r0: src[b] = the entry when stored, else ~j (the j-th fresh row block of the arena).  A fresh frame with an entry is
// stored there by the call (*n_store of them) and its bit is set; one without is computed, read from the arena and not stored.
// Returns n_fresh, or -1 and changes nothing for an index out of range or a missing argument.
inline int head_lists(HeadBits& bits, int s, const int32_t* ent, const int32_t* miss, int n_img, const int32_t* row, const int32_t* uniq,
                      int U, const int32_t* map, int B, int32_t* hent, int32_t* hmiss, int32_t* uniq_fresh, int32_t* src, int* n_store) {
    if (!ent || !miss || !row || !uniq || !map || !hent || !hmiss || !uniq_fresh || !src || !n_store || s < 0 || s > 1 || U <= 0 || B <= 0 ||
        n_img <= 0)
        return -1;
    for (int k = 0; k < U; k++)
        if (row[k] < 0 || row[k] >= n_img || ent[row[k]] < -1 || ent[row[k]] >= FC_MAX_ENTRIES) return -1;
    for (int b = 0; b < B; b++)
        if (map[b] < 0 || map[b] >= U) return -1;
    int n_fresh = 0;
    *n_store = 0;
    for (int k = 0; k < U; k++) {
        const int32_t e = ent[row[k]];
        hent[k] = e;
        if (miss[row[k]] < 0 && bits.has(e, s)) { hmiss[k] = -1; continue; }
        uniq_fresh[n_fresh] = uniq[k];
        hmiss[k] = n_fresh++;
        if (e >= 0) { bits.set(e, s); (*n_store)++; }
    }
    for (int b = 0; b < B; b++) src[b] = hmiss[map[b]] < 0 ? hent[map[b]] : ~hmiss[map[b]];
    return n_fresh;
}
// Device side: the r0 and c blocks (words floats each) of every fresh frame k < U that has an entry (hmiss[k] >= 0, hent[k] >= 0)
// go to side s of that entry.
int head_products_store(const HeadStore& st, int s, const int32_t* hent, const int32_t* hmiss, int U, const float* r0, const float* c,
                        void* stream);
// The combine passes of a side whose c and r0 come from two places (a3r.h: a3r_combine_resid_fh2_src,
// a3r_upsample2x_combine_fh2_src) read head_lists' src: src[b] >= 0 names an entry of the storage, whose blocks lie `stride`
// floats apart from store_c / store_r0 (HeadStore::c, r0, stride), src[b] < 0 the fresh block ~src[b] of c / r0.

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
// (the second conv of refinenet1.resConfUnit1 on distinct frames is a3r_combine_resid_fh2 of a3r.h, or a3r_upsample2x_combine_fh2
// with its residual, the bilinear 2x of x cropped to Hc x Wc, made on the fly)

// ---- the lists of one call.  Every list the host builds, in the order they lie in memory: one block of DD_HALF-word lists, which
// the host fills (pinned words) and one upload copies to the device; both blocks are viewed through this struct, so a member of
// the device view is the device address of that list.  The lists of the two sides (uniq_side, map_side, hp_*) share one member:
// side s's B words start at word s B.
constexpr int DD_HALF = DEDUP_MAX_SLOTS / 2;                       // slots of one kind at most
struct CallLists {
    using List = int32_t[DD_HALF];
    List uniq_img, map_img, uniq_pd, map_pd;         // dedup_group of the two kinds
    List uniq_side, map_side;                        // dedup_group_side, [2][B]
    List ent_img, ent_pd, map_eo, map_ekv;           // decoder block 0 on entries (dedup_group_entries; model.hip, Distinct)
    List fc_fresh, fc_ent, fc_miss;                  // the frame cache: the images to encode, FrameCacheTable::assign's entries
    List pd_fresh, pd_ent, pd_miss, pd_src, pd_src_ent;      // the stored priors (prior_lists); src_ent [2 n_ent]: src of the entries' priors
    List hp_ent, hp_miss, hp_fresh, hp_src;          // the head products (head_lists), [2][B]
};
constexpr int DD_LISTS = sizeof(CallLists) / sizeof(CallLists::List);
static_assert(sizeof(CallLists) == (size_t)DD_LISTS * DD_HALF * sizeof(int32_t), "CallLists is its lists and nothing else");

// Bytes of a head's level-0 buffers with n images of N tokens in them, as the arena rounds them: a0, l0, l03, r0, r0r3; the merged
// branch adds the compact enc_norm rows and the bias-only output c of resConfUnit1's second conv.  fh2 maps take 4 bytes per
// element.  E, F, l: enc_embed_dim, feature_dim, layer_dims[0].
inline size_t head_level0_bytes(int E, int F, int l, int N, int n, bool merged) {
    const size_t px = (size_t)n * N, f = F;
    const size_t fl[7] = {px * l, px * 16 * l, px * 16 * l, px * 16 * f, px * 16 * f, px * E, px * 16 * f};
    size_t b = 0;
    for (int i = 0; i < (merged ? 7 : 5); i++) b += (fl[i] * 4 + 255) / 256 * 256;
    return b;
}
// A side with U distinct frames merges when its level-0 buffers fit in what the plain plan reserves for them, so that the
// workspace requirement does not move: U (33 l + 48 F + E) <= B (33 l + 32 F) up to rounding, U <= 0.69 B for ViT-L heads
// (l = 96, F = 256, E = 1024).
inline bool head_merge_fits(int E, int F, int l, int N, int B, int U) {
    return U > 0 && U < B && head_level0_bytes(E, F, l, N, U, true) <= head_level0_bytes(E, F, l, N, B, false);
}

// What the planner is told about a call, in plain numbers.  rep [4 B]: dedup_find's representatives of the two kinds; flag: its
// mismatch word; hit_img / hit_pd [2 B]: frame_cache_lookup's answers for the image / pred_depth slots, null when that store was
// not looked up in this call (absent, or bypassed).
struct CallInputs {
    const int32_t* rep; int32_t flag; const int32_t *hit_img, *hit_pd;
    int B, H, W;
    int E, D, F, l0;                 // enc_embed_dim, dec_embed_dim, feature_dim, layer_dims[0]
    bool encode, first_kind;         // a forward from images (they are merged for the encoder too); the first kind was looked at
    bool dedup_head, dedup_decoder;  // a3r_model_set_dedup_head, a3r_model_set_dedup_decoder
    bool gemm_fh2, map_fh2;          // the GEMM inputs / the DPT maps are fh2
    bool attn_maps;                  // attention_fh2_takes_maps()
    bool heads;                      // a head-products storage with room for every entry of the frame cache is installed
};
// What the planner decided: the counts a3r_model_last_* report, and what the plan runs on.
struct CallPlan {
    bool use = false;                // the plan runs on the lists; else the plain plan
    bool fell_back = false;          // a slot differs from its representative, or a list is not what it must be
    bool drop = false;               // the tables no longer describe the storage: forget everything stored
    int n_img, n_pd;                 // distinct images / priors (2 B: that kind is not merged)
    int side_unique[2];              // distinct frames of each side, and whether its head merges on them (n_side < B)
    int n_side[2], side_merged[2] = {0, 0};
    int n_ent = 0, ent_unique[2];    // decoder block 0: entries per side, padded (0: per slot); each side's distinct entries
    // the stores this call uses, what it runs (fresh) and keeps (store) of each, and hits, misses, evictions
    bool fc = false, pd = false, hp[2] = {false, false};
    int fc_fresh = 0, fc_store = 0, pd_fresh = 0, pd_store = 0, hp_fresh[2] = {0, 0}, hp_store[2] = {0, 0};
    int fc_n[3] = {0, 0, 0}, pd_n[3] = {0, 0, 0};
    explicit CallPlan(int B = 0) : n_img(2 * B), n_pd(2 * B), side_unique{B, B}, n_side{B, B}, ent_unique{B, B} {}
    int hp_hits(int s) const { return hp[s] ? n_side[s] - hp_fresh[s] : 0; }
    int hp_misses(int s) const { return hp[s] ? hp_fresh[s] : 0; }
};

// The host's part of a call, between the one read-back and the one upload: groups the slots, asks the tables of the three stores
// for entries, and fills L.  The tables change as the call will change the storage; a call that falls back before it touches
// them leaves them as they were.
inline CallPlan plan_call(const CallInputs& in, FrameCacheTable& fc_table, FrameCacheTable& pd_table, HeadBits& hp_bits, CallLists& L) {
    const int B = in.B, S = 2 * B;
    const int32_t* rep = in.rep;
    CallPlan p(B);
    if (in.flag != 0) {
        p.fell_back = true;
        return p;
    }
    // the distinct frames' enc_norm rows must fit the buffers they wait in (run_plan)
    auto rows_fit = [&](int n) { return (size_t)n * in.E <= 3 * (size_t)S * in.D; };
    int n_img = S;
    if (in.encode && in.first_kind) {
        n_img = dedup_group(rep, S, L.uniq_img, L.map_img);
        if (n_img > 0 && !rows_fit(n_img)) n_img = S;
    }
    // the heads' level-0 branch: each side's own distinct frames
    if (in.first_kind && in.dedup_head && in.map_fh2)
        for (int s = 0; s < 2; s++) {
            const int u = dedup_group_side(rep, B, s, L.uniq_side + s * B, L.map_side + s * B);
            if (u <= 0) { n_img = 0; break; }
            p.side_unique[s] = u;
            if (head_merge_fits(in.E, in.F, in.l0, (in.H / 16) * (in.W / 16), B, u)) p.n_side[s] = u;
        }
    const int n_pd = dedup_group(rep + S, S, L.uniq_pd, L.map_pd);
    if (n_img <= 0 || n_pd <= 0) {       // not a representative table: cannot happen, and is not trusted if it does
        p = CallPlan(B);
        p.fell_back = true;
        return p;
    }
    p.n_img = n_img;
    p.n_pd = n_pd;
    // decoder block 0: each side's distinct (image, prior) entries, when both kinds merge (fh2 GEMM inputs, the attention form with maps)
    int n_ent = 0;
    if (in.dedup_decoder && in.gemm_fh2 && in.attn_maps && n_img < S && n_pd < S) {
        int32_t ent[DD_HALF], map_e[DD_HALF];
        const int um = dedup_group_entries(L.map_img, L.map_pd, B, ent, map_e, p.ent_unique);      // (-1: it wrote nothing)
        // The statistic of an fh2 GEMM output covers the whole last row tile: rows past M are copies of the last row, rotated at
        // their own RoPE positions.  The q / k / v projections keep the plain plan's statistics bit for bit only where neither
        // plan has such rows: both row counts whole multiples of the largest row tile (256).
        const long N = (long)(in.H / 16) * (in.W / 16);
        if (um > 0 && um < B && (B * N) % 256 == 0 && (um * N) % 256 == 0) {
            n_ent = um;
            for (int s = 0; s < 2; s++) {
                for (int e = 0; e < um; e++) {
                    L.ent_img[s * um + e] = L.map_img[ent[s * B + e]];
                    L.ent_pd[s * um + e] = L.map_pd[ent[s * B + e]];
                }
                for (int b = 0; b < B; b++) {
                    L.map_eo[s * B + b] = s * um + map_e[s * B + b];
                    L.map_ekv[s * B + b] = s * um + map_e[(1 - s) * B + b];
                }
            }
        }
    }
    p.n_ent = n_ent;
    // The frame cache: hits and misses among the distinct images, victims for the misses (FrameCacheTable::assign), the lists of
    // the exchange pass.  It needs the image stage on the distinct list, whose rows must fit where they wait (above).
    p.fc = in.hit_img && rows_fit(n_img);
    if (p.fc) {
        for (int k = 0; k < n_img; k++) L.fc_miss[k] = in.hit_img[L.uniq_img[k]];
        p.fc = fc_table.assign(L.fc_miss, n_img, L.fc_ent, p.fc_n) == 0;
    }
    if (p.fc)
        for (int k = 0; k < n_img; k++) {
            const bool hit = L.fc_miss[k] >= 0;
            if (!hit) {
                L.fc_fresh[p.fc_fresh] = L.uniq_img[k];
                p.fc_store += L.fc_ent[k] >= 0;
                hp_bits.clear(L.fc_ent[k]);      // the entry now holds another frame: what the heads made of the old one is stale
            }
            L.fc_miss[k] = hit ? -1 : p.fc_fresh++;
        }
    // The stored priors: hits, misses and victims among the distinct pred_depth maps, and the lists of the prior branch
    if (in.hit_pd) {
        int32_t hit[DD_HALF];
        for (int k = 0; k < n_pd; k++) hit[k] = in.hit_pd[L.uniq_pd[k]];
        p.pd = pd_table.assign(hit, n_pd, L.pd_ent, p.pd_n) == 0;
        if (p.pd) {
            p.pd_fresh = prior_lists(hit, L.pd_ent, L.uniq_pd, n_pd, L.pd_miss, L.pd_fresh, L.map_pd, S, L.pd_src, &p.pd_store);
            if (p.pd_fresh < 0) {               // (never: map_pd is dedup_group's)
                p.drop = p.fell_back = true;
                return p;
            }
            for (int i = 0; i < 2 * n_ent; i++) L.pd_src_ent[i] = L.pd_src[L.uniq_pd[L.ent_pd[i]]];      // ent_pd names distinct priors
        }
    }
    // The head products: which of a merging side's distinct frames are stored, and the lists of its level-0 branch.  They ride on
    // the frame cache (its entries, dropped and bypassed with it); a side that does not merge neither reads nor writes them.
    if (p.fc && in.heads && in.map_fh2 && in.gemm_fh2)
        for (int s = 0; s < 2; s++) {
            if (p.n_side[s] >= B) continue;
            const int off = s * B, U = p.n_side[s];
            int32_t row[DD_HALF];
            for (int k = 0; k < U; k++) row[k] = L.map_img[L.uniq_side[off + k]];
            p.hp_fresh[s] = head_lists(hp_bits, s, L.fc_ent, L.fc_miss, n_img, row, L.uniq_side + off, U, L.map_side + off, B, L.hp_ent + off,
                                       L.hp_miss + off, L.hp_fresh + off, L.hp_src + off, &p.hp_store[s]);
            if (p.hp_fresh[s] < 0) {            // (never: the lists are dedup_group's and assign's)
                p.drop = p.fell_back = true;
                return p;
            }
            p.hp[s] = true;
        }
    if (!p.fc && !p.pd && n_img == S && n_pd == S && p.n_side[0] == B && p.n_side[1] == B) return p;      // nothing to merge
    p.side_merged[0] = p.n_side[0] < B;
    p.side_merged[1] = p.n_side[1] < B;
    p.use = true;
    return p;
}

}  // namespace a3r
