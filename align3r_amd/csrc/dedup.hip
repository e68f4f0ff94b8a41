// Exact duplicate detection among the inputs of one pair-forward batch (dedup.h): a 128-bit content key per slot, the smallest slot
// with the same key as representative, and a bitwise comparison of every slot with its representative.  Everything works on the
// raw 32-bit patterns (-0.0 != +0.0, NaN payloads count); the key only proposes, the comparison decides.
#include "common.h"
#include "dedup.h"

namespace a3r {
namespace {

constexpr int UNITS_PER_BLOCK = 2048;      // 16-byte units per workgroup: 8 per thread, 32 KB

struct Items { const uint4* base[4]; long units[2]; };    // img1, img2, pd1, pd2; 16-byte units per item of either kind

__device__ __forceinline__ uint64_t mix64(uint64_t z) {      // the splitmix64 finaliser
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// key[slot] = sum over the slot's 16-byte units i of two mixes of (unit, i), modulo 2^64 each: the sum commutes, so waves add their
// parts in any order, and the position enters every term, so permuted content gives another key.
// grid: x over chunks of UNITS_PER_BLOCK units (of the longer kind), y over slots first .. 4 B - 1
__global__ __launch_bounds__(256) void dedup_key_kernel(Items it, int B, int first, unsigned long long* __restrict__ keys) {
    const int slot = first + blockIdx.y;
    const long units = it.units[slot >= 2 * B];
    const uint4* __restrict__ p = it.base[slot / B] + (long)(slot % B) * units;
    const long u0 = (long)blockIdx.x * UNITS_PER_BLOCK;
    uint64_t k0 = 0, k1 = 0;
#pragma unroll
    for (int j = 0; j < UNITS_PER_BLOCK / 256; j++) {
        const long u = u0 + j * 256 + threadIdx.x;
        if (u < units) {
            const uint4 w = p[u];
            const uint64_t a = (uint64_t)w.x | ((uint64_t)w.y << 32), b = (uint64_t)w.z | ((uint64_t)w.w << 32);
            const uint64_t pos = (2 * (uint64_t)u + 1) * 0x9e3779b97f4a7c15ull;
            const uint64_t x = mix64(a ^ pos), y = mix64(b + pos);
            k0 += x + (y << 1 | y >> 63);
            k1 += mix64(x + 3 * y);
        }
    }
    k0 = wave_sum_u64(k0);
    k1 = wave_sum_u64(k1);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(keys + 2 * slot, (unsigned long long)k0);
        atomicAdd(keys + 2 * slot + 1, (unsigned long long)k1);
    }
}

// rep[slot] = the smallest slot of the same kind with the same key, as an index inside the kind; one thread per slot
__global__ void dedup_rep_kernel(const unsigned long long* __restrict__ keys, int B, int first, int* __restrict__ rep) {
    const int slot = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= 4 * B) return;
    const int kind0 = slot < 2 * B ? 0 : 2 * B;
    const unsigned long long k0 = keys[2 * slot], k1 = keys[2 * slot + 1];
    int r = kind0;
    while (r < slot && (keys[2 * r] != k0 || keys[2 * r + 1] != k1)) r++;
    rep[slot] = r - kind0;
}

// raises *flag when a slot differs from its representative; same grid as the key kernel
__global__ __launch_bounds__(256) void dedup_verify_kernel(Items it, int B, int first, const int* __restrict__ rep,
                                                           int* __restrict__ flag) {
    const int slot = first + blockIdx.y;
    const long units = it.units[slot >= 2 * B];
    const int r = (slot < 2 * B ? 0 : 2 * B) + rep[slot];
    if (r == slot) return;
    const uint4* __restrict__ p = it.base[slot / B] + (long)(slot % B) * units;
    const uint4* __restrict__ q = it.base[r / B] + (long)(r % B) * units;
    const long u0 = (long)blockIdx.x * UNITS_PER_BLOCK;
    unsigned diff = 0;
#pragma unroll
    for (int j = 0; j < UNITS_PER_BLOCK / 256; j++) {
        const long u = u0 + j * 256 + threadIdx.x;
        if (u < units) {
            const uint4 a = p[u], b = q[u];
            diff |= (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w);
        }
    }
    if (diff) *flag = 1;
}

// ---- frames kept across calls (dedup.h, FrameCacheLayout)
struct Images { const uint4* base[2]; };      // img1, img2: slot s < 2 B is item s % B of base[s / B]

__device__ __forceinline__ bool fc_valid(const FrameCacheMask& m, int e) { return (m.w[e >> 5] >> (e & 31)) & 1u; }

// flag[e * 2 B + slot] becomes nonzero when the image of slot -- a representative -- differs from that of the valid entry e with
// the slot's key; grid: x over chunks of UNITS_PER_BLOCK units, y over the 2 B slots
__global__ __launch_bounds__(256) void fc_compare_kernel(Images im, int B, long units, const unsigned long long* __restrict__ keys,
                                                         const int* __restrict__ rep, const unsigned long long* __restrict__ ekeys,
                                                         const uint4* __restrict__ eimg, int cap, FrameCacheMask mask,
                                                         int* __restrict__ flag) {
    const int slot = blockIdx.y;
    if (rep[slot] != slot) return;
    const unsigned long long k0 = keys[2 * slot], k1 = keys[2 * slot + 1];
    const uint4* __restrict__ p = im.base[slot / B] + (long)(slot % B) * units;
    const long u0 = (long)blockIdx.x * UNITS_PER_BLOCK;
    for (int e = 0; e < cap; e++) {
        if (!fc_valid(mask, e) || ekeys[2 * e] != k0 || ekeys[2 * e + 1] != k1) continue;
        const uint4* __restrict__ q = eimg + (long)e * units;
        unsigned diff = 0;
#pragma unroll
        for (int j = 0; j < UNITS_PER_BLOCK / 256; j++) {
            const long u = u0 + j * 256 + threadIdx.x;
            if (u < units) {
                const uint4 a = p[u], b = q[u];
                diff |= (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w);
            }
        }
        if (diff) flag[(long)e * 2 * B + slot] = 1;
    }
}

// hit[slot] = the first valid entry with the slot's key and no mismatch flag, -1 without one or for a slot that is not its own
// representative; one thread per slot
__global__ void fc_pick_kernel(int B, const unsigned long long* __restrict__ keys, const int* __restrict__ rep,
                               const unsigned long long* __restrict__ ekeys, int cap, FrameCacheMask mask, const int* __restrict__ flag,
                               int* __restrict__ hit) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= 2 * B) return;
    int h = -1;
    if (rep[slot] == slot) {
        const unsigned long long k0 = keys[2 * slot], k1 = keys[2 * slot + 1];
        for (int e = 0; e < cap && h < 0; e++)
            if (fc_valid(mask, e) && ekeys[2 * e] == k0 && ekeys[2 * e + 1] == k1 && !flag[(long)e * 2 * B + slot]) h = e;
    }
    hit[slot] = h;
}

// grid: x over chunks of UNITS_PER_BLOCK units of the longer of image and rows, y over the U distinct images
__global__ __launch_bounds__(256) void fc_exchange_kernel(Images im, int B, long units_img, long units_feat,
                                                          const unsigned long long* __restrict__ keys, unsigned long long* __restrict__ ekeys,
                                                          uint4* __restrict__ eimg, uint4* __restrict__ efeat, const int* __restrict__ uniq,
                                                          const int* __restrict__ ent, const int* __restrict__ miss,
                                                          const uint4* __restrict__ fresh, uint4* __restrict__ rows) {
    const int k = blockIdx.y, e = ent[k], j = miss[k];
    const long u0 = (long)blockIdx.x * UNITS_PER_BLOCK;
    uint4* __restrict__ dst = rows + (long)k * units_feat;
    if (j < 0) {                                   // a hit: the stored rows
        if (e < 0) return;                         // (never: a hit names its entry)
        const uint4* __restrict__ src = efeat + (long)e * units_feat;
        for (int i = 0; i < UNITS_PER_BLOCK / 256; i++) {
            const long u = u0 + i * 256 + threadIdx.x;
            if (u < units_feat) dst[u] = src[u];
        }
        return;
    }
    const uint4* __restrict__ src = fresh + (long)j * units_feat;
    uint4* __restrict__ keep = e >= 0 ? efeat + (long)e * units_feat : nullptr;
    for (int i = 0; i < UNITS_PER_BLOCK / 256; i++) {
        const long u = u0 + i * 256 + threadIdx.x;
        if (u < units_feat) {
            const uint4 v = src[u];
            dst[u] = v;
            if (keep) keep[u] = v;
        }
    }
    if (e < 0) return;
    const int slot = uniq[k];
    const uint4* __restrict__ p = im.base[slot / B] + (long)(slot % B) * units_img;
    uint4* __restrict__ q = eimg + (long)e * units_img;
    for (int i = 0; i < UNITS_PER_BLOCK / 256; i++) {
        const long u = u0 + i * 256 + threadIdx.x;
        if (u < units_img) q[u] = p[u];
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) ekeys[2 * e + threadIdx.x] = keys[2 * slot + threadIdx.x];
}

// fc_exchange_kernel's stores alone, in parts: a missed item k with an entry e puts units_part units of fresh block miss[k] at
// unit `off` of the entry's rows, or without `fresh` its own bits and key; same grid
__global__ __launch_bounds__(256) void fc_store_kernel(Images im, int B, long units_img, long units_feat, long off, long units_part,
                                                       const unsigned long long* __restrict__ keys, unsigned long long* __restrict__ ekeys,
                                                       uint4* __restrict__ eimg, uint4* __restrict__ efeat, const int* __restrict__ uniq,
                                                       const int* __restrict__ ent, const int* __restrict__ miss,
                                                       const uint4* __restrict__ fresh) {
    const int k = blockIdx.y, e = ent[k], j = miss[k];
    if (j < 0 || e < 0) return;
    const long u0 = (long)blockIdx.x * UNITS_PER_BLOCK;
    if (fresh) {
        const uint4* __restrict__ src = fresh + (long)j * units_part;
        uint4* __restrict__ dst = efeat + (long)e * units_feat + off;
        for (int i = 0; i < UNITS_PER_BLOCK / 256; i++) {
            const long u = u0 + i * 256 + threadIdx.x;
            if (u < units_part) dst[u] = src[u];
        }
        return;
    }
    const int slot = uniq[k];
    const uint4* __restrict__ p = im.base[slot / B] + (long)(slot % B) * units_img;
    uint4* __restrict__ q = eimg + (long)e * units_img;
    for (int i = 0; i < UNITS_PER_BLOCK / 256; i++) {
        const long u = u0 + i * 256 + threadIdx.x;
        if (u < units_img) q[u] = p[u];
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) ekeys[2 * e + threadIdx.x] = keys[2 * slot + threadIdx.x];
}

// fc_store_kernel's sibling for the head products: a fresh frame k with an entry puts its r0 block (blockIdx.z = 0) or c block (1),
// `units` 16-byte units each, into its side of the entry; grid x over chunks, y over the side's frames
__global__ __launch_bounds__(256) void hp_store_kernel(const uint4* __restrict__ r0, const uint4* __restrict__ c, uint4* __restrict__ side,
                                                       long units, const int* __restrict__ hent, const int* __restrict__ hmiss) {
    const int k = blockIdx.y, e = hent[k], j = hmiss[k];
    if (j < 0 || e < 0) return;
    const uint4* __restrict__ src = (blockIdx.z ? c : r0) + (long)j * units;
    uint4* __restrict__ dst = side + ((long)e * 4 + blockIdx.z) * units;       // an entry: [2 sides][r0, c][units]
    const long u0 = (long)blockIdx.x * UNITS_PER_BLOCK;
    for (int i = 0; i < UNITS_PER_BLOCK / 256; i++) {
        const long u = u0 + i * 256 + threadIdx.x;
        if (u < units) dst[u] = src[u];
    }
}

// one thread per statistics word: those of `sites`
__global__ void fc_stats_sites_kernel(unsigned* __restrict__ estats, const int* __restrict__ ent, const int* __restrict__ miss, int U,
                                      unsigned* __restrict__ stats, SiteMask sites) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= FC_STAT_WORDS || !((sites.w[i >> 5] >> (i & 31)) & 1u)) return;
    const unsigned own = stats[i];
    unsigned w = own;
    for (int k = 0; k < U; k++) {
        const int e = ent[k];
        if (e < 0) continue;
        unsigned* s = estats + (long)e * FC_STAT_WORDS + i;
        if (miss[k] >= 0) *s = own;
        else w = *s > w ? *s : w;                  // words are bit patterns of non-negative floats: ordered as unsigned
    }
    stats[i] = w;
}

bool fc_layout_ok(const FrameCacheLayout& l) {
    return l.cap > 0 && l.cap <= FC_MAX_ENTRIES && l.keys && l.words_img > 0 && l.words_img % 4 == 0 && l.words_feat > 0 &&
           l.words_feat % 4 == 0 && (reinterpret_cast<uintptr_t>(l.keys) & 15) == 0;
}

}  // namespace

int frame_cache_lookup(const float* img1, const float* img2, int B, const void* keys, const int32_t* rep, const FrameCacheLayout& l,
                       const FrameCacheMask& mask, int32_t* hit, void* stream) {
    A3R_CHECK_ARG(B > 0 && B <= FC_MAX_PAIRS && fc_layout_ok(l), "frame_cache_lookup: bad shape (B=%d, %d entries)", B, l.cap);
    A3R_CHECK_ARG(img1 && img2 && keys && rep && hit && ((reinterpret_cast<uintptr_t>(img1) | reinterpret_cast<uintptr_t>(img2)) & 15) == 0,
                  "frame_cache_lookup: null or misaligned pointer");
    hipStream_t st = as_stream(stream);
    const Images im = {{reinterpret_cast<const uint4*>(img1), reinterpret_cast<const uint4*>(img2)}};
    const long units = l.words_img / 4;
    int* flag = reinterpret_cast<int*>(l.flags);
    const unsigned long long* ekeys = reinterpret_cast<const unsigned long long*>(l.keys);
    A3R_HIP(hipMemsetAsync(flag, 0, (size_t)l.cap * 2 * B * sizeof(int), st));
    ProfScope prof(PK_ELEMENTWISE, 2.0 * 16 * units * 2 * B, st);
    const dim3 grid((unsigned)((units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK), (unsigned)(2 * B));
    hipLaunchKernelGGL(fc_compare_kernel, grid, dim3(256), 0, st, im, B, units, static_cast<const unsigned long long*>(keys), rep, ekeys,
                       reinterpret_cast<const uint4*>(l.img), l.cap, mask, flag);
    hipLaunchKernelGGL(fc_pick_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, st, B, static_cast<const unsigned long long*>(keys), rep,
                       ekeys, l.cap, mask, flag, hit);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

int frame_cache_exchange(const float* img1, const float* img2, int B, const void* keys, const FrameCacheLayout& l, const int32_t* uniq,
                         const int32_t* ent, const int32_t* miss, int U, const float* fresh, float* rows, void* stream) {
    A3R_CHECK_ARG(B > 0 && B <= FC_MAX_PAIRS && U > 0 && U <= 2 * B && fc_layout_ok(l), "frame_cache_exchange: bad shape (B=%d, U=%d)", B, U);
    A3R_CHECK_ARG(img1 && img2 && keys && uniq && ent && miss && fresh && rows &&
                      ((reinterpret_cast<uintptr_t>(fresh) | reinterpret_cast<uintptr_t>(rows)) & 15) == 0,
                  "frame_cache_exchange: null or misaligned pointer");
    hipStream_t st = as_stream(stream);
    const Images im = {{reinterpret_cast<const uint4*>(img1), reinterpret_cast<const uint4*>(img2)}};
    const long ui = l.words_img / 4, uf = l.words_feat / 4, units = ui > uf ? ui : uf;
    ProfScope prof(PK_ELEMENTWISE, 16.0 * U * (3 * uf + 2 * ui), st);
    const dim3 grid((unsigned)((units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK), (unsigned)U);
    hipLaunchKernelGGL(fc_exchange_kernel, grid, dim3(256), 0, st, im, B, ui, uf, static_cast<const unsigned long long*>(keys),
                       reinterpret_cast<unsigned long long*>(l.keys), reinterpret_cast<uint4*>(l.img), reinterpret_cast<uint4*>(l.feat),
                       uniq, ent, miss, reinterpret_cast<const uint4*>(fresh), reinterpret_cast<uint4*>(rows));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

int frame_cache_store(const float* img1, const float* img2, int B, const void* keys, const FrameCacheLayout& l, const int32_t* uniq,
                      const int32_t* ent, const int32_t* miss, int U, const float* fresh, long part_off, long part_words, void* stream) {
    A3R_CHECK_ARG(B > 0 && B <= FC_MAX_PAIRS && U > 0 && U <= 2 * B && fc_layout_ok(l), "frame_cache_store: bad shape (B=%d, U=%d)", B, U);
    A3R_CHECK_ARG(uniq && ent && miss && (fresh || (img1 && img2 && keys)) && (reinterpret_cast<uintptr_t>(fresh) & 15) == 0,
                  "frame_cache_store: null or misaligned pointer");
    A3R_CHECK_ARG(!fresh || (part_off >= 0 && part_words > 0 && part_off % 4 == 0 && part_words % 4 == 0 && part_off + part_words <= l.words_feat),
                  "frame_cache_store: words %ld + %ld outside an entry's %ld", part_off, part_words, l.words_feat);
    hipStream_t st = as_stream(stream);
    const Images im = {{reinterpret_cast<const uint4*>(img1), reinterpret_cast<const uint4*>(img2)}};
    const long ui = l.words_img / 4, units = fresh ? part_words / 4 : ui;
    ProfScope prof(PK_ELEMENTWISE, 32.0 * U * units, st);
    const dim3 grid((unsigned)((units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK), (unsigned)U);
    hipLaunchKernelGGL(fc_store_kernel, grid, dim3(256), 0, st, im, B, ui, l.words_feat / 4, part_off / 4, part_words / 4,
                       static_cast<const unsigned long long*>(keys), reinterpret_cast<unsigned long long*>(l.keys),
                       reinterpret_cast<uint4*>(l.img), reinterpret_cast<uint4*>(l.feat), uniq, ent, miss, reinterpret_cast<const uint4*>(fresh));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

int head_products_store(const HeadStore& hs, int s, const int32_t* hent, const int32_t* hmiss, int U, const float* r0, const float* c,
                        void* stream) {
    A3R_CHECK_ARG(hs.cap > 0 && hs.cap <= FC_MAX_ENTRIES && hs.rows && hs.words > 0 && hs.words % 4 == 0 && (s == 0 || s == 1) && U > 0 &&
                      U <= FC_MAX_PAIRS, "head_products_store: bad shape (%d entries, side %d, U=%d)", hs.cap, s, U);
    A3R_CHECK_ARG(hent && hmiss && r0 && c && ((reinterpret_cast<uintptr_t>(r0) | reinterpret_cast<uintptr_t>(c) |
                                                 reinterpret_cast<uintptr_t>(hs.rows)) & 15) == 0,
                  "head_products_store: null or misaligned pointer");
    hipStream_t st = as_stream(stream);
    const long units = hs.words / 4;
    ProfScope prof(PK_ELEMENTWISE, 64.0 * U * units, st);
    const dim3 grid((unsigned)((units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK), (unsigned)U, 2);
    hipLaunchKernelGGL(hp_store_kernel, grid, dim3(256), 0, st, reinterpret_cast<const uint4*>(r0), reinterpret_cast<const uint4*>(c),
                       reinterpret_cast<uint4*>(hs.rows) + (long)(2 * s) * units, units, hent, hmiss);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

int stats_sites_words(unsigned* estats, int cap, const int32_t* ent, const int32_t* miss, int U, unsigned* stats, const SiteMask& sites,
                      void* stream) {
    A3R_CHECK_ARG(estats && cap > 0 && cap <= FC_MAX_ENTRIES && ent && miss && stats && U > 0, "stats_sites_words: bad argument");
    hipStream_t st = as_stream(stream);
    ProfScope prof(PK_ELEMENTWISE, 4.0 * FC_STAT_WORDS * (U + 2), st);
    hipLaunchKernelGGL(fc_stats_sites_kernel, dim3(FC_STAT_WORDS / 256), dim3(256), 0, st, estats, ent, miss, U, stats, sites);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

int dedup_find(const float* img1, const float* img2, const float* pd1, const float* pd2, int B, long words_a, long words_pd, int first,
               bool const_key, void* keys, int32_t* rep_flag, void* stream) {
    A3R_CHECK_ARG(B > 0 && 4 * B <= DEDUP_MAX_SLOTS && words_pd > 0 && words_pd % 4 == 0 && (first == 0 || first == 2 * B) &&
                      (first > 0 || (words_a > 0 && words_a % 4 == 0)),
                  "dedup_find: bad shape (B=%d, words=%ld / %ld, first=%d)", B, words_a, words_pd, first);
    A3R_CHECK_ARG(pd1 && pd2 && (first > 0 || (img1 && img2)) && keys && rep_flag, "dedup_find: null pointer");
    const Items it = {{reinterpret_cast<const uint4*>(img1), reinterpret_cast<const uint4*>(img2), reinterpret_cast<const uint4*>(pd1),
                       reinterpret_cast<const uint4*>(pd2)},
                      {first == 0 ? words_a / 4 : 0, words_pd / 4}};
    for (const uint4* p : it.base)
        A3R_CHECK_ARG((reinterpret_cast<uintptr_t>(p) & 15) == 0, "dedup_find: inputs must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    const long units = it.units[0] > it.units[1] ? it.units[0] : it.units[1];
    const int nslots = 4 * B - first;
    A3R_HIP(hipMemsetAsync(keys, 0, (size_t)4 * B * 16, st));
    A3R_HIP(hipMemsetAsync(rep_flag, 0, (size_t)(4 * B + 1) * sizeof(int32_t), st));
    ProfScope prof(PK_ELEMENTWISE, 3.0 * 16 * (it.units[0] * (2 * B - first) + it.units[1] * 2 * B), st);
    const dim3 grid((unsigned)((units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK), (unsigned)nslots);
    if (!const_key)
        hipLaunchKernelGGL(dedup_key_kernel, grid, dim3(256), 0, st, it, B, first, static_cast<unsigned long long*>(keys));
    hipLaunchKernelGGL(dedup_rep_kernel, dim3((nslots + 255) / 256), dim3(256), 0, st, static_cast<const unsigned long long*>(keys), B,
                       first, rep_flag);
    hipLaunchKernelGGL(dedup_verify_kernel, grid, dim3(256), 0, st, it, B, first, rep_flag, rep_flag + 4 * B);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

}  // namespace a3r

extern "C" int a3r_frame_cache_stats_sites(void* storage, size_t bytes, int64_t words_item, int64_t words_rows, const int32_t* ent,
                                           const int32_t* miss, int U, unsigned* stats, const uint32_t* site_mask, void* stream) {
    A3R_CHECK_ARG(storage && site_mask && words_item > 0 && words_rows > 0, "a3r_frame_cache_stats_sites: bad argument");
    a3r::SiteMask sites;
    for (int i = 0; i < a3r::FC_STAT_WORDS / 32; i++) sites.w[i] = site_mask[i];
    const a3r::FrameCacheLayout l = a3r::frame_cache_layout(storage, bytes, words_item, words_rows);
    A3R_CHECK_ARG(a3r::fc_layout_ok(l) && l.stats, "a3r_frame_cache_stats_sites: bad argument");
    return a3r::stats_sites_words(reinterpret_cast<unsigned*>(l.stats), l.cap, ent, miss, U, stats, sites, stream);
}
