// Voxel-grid downsampling of a point cloud for gfx950: the points grouped by the cell of a regular grid they fall into, one point
// out per cell, through an open-addressing hash table in global memory.  The definition (include/a3r.h has it in full), float64
// with every operation rounded on its own (this file is compiled with -ffp-contract=off):
//
//   r_a = (double)x_a / voxel,  q_a = floor(r_a);   in a voxel iff  -2^20 <= q_a < 2^20  for a = x, y, z  (false for NaN / inf)
//   key   = ((q_x + 2^20) << 42) | ((q_y + 2^20) << 21) | (q_z + 2^20)            63 bits: the all-ones word means "empty"
//   value = (w << 32) | i,  w = 0 without priorities, else the inverted order-preserving map of the fp32 bits (NaN: all ones)
//   a voxel's winner = the MINIMUM value of its points;  count = its points;  kept iff count >= min_count;  output in winner order
//
// The minimum and the sums are integer, so the result is a function of the inputs alone although the table is built with atomics:
// WHERE a key lands in the table depends on the arrival order, and nothing that is returned depends on where.
// Passes in stream order:
//   * fill:   keys and best values all ones, counts and sums zero, the error and dropped words zero.
//   * insert: a thread owns one point.  It hashes the key and probes linearly: the slot's key is read (an agent-scope load, served
//             by L2 where the atomics land); an empty slot is claimed by a 64-bit compare-and-swap; on its own key -- found or just
//             claimed -- the thread lowers the best value (an atomic minimum, skipped when a read shows it cannot lower the word:
//             best values only decrease, as the renderer's keys do), adds 1 to the count and, in mean mode, its fixed-point offsets
//             and colours to the slot's sums; otherwise it moves on.  No lock, no wait.  The slot is left in slot[i].  Neighbouring
//             lanes of a wave that share a key are folded into one lane first (voxel_insert_kernel: COMBINE).
//   * flag:   point i wins iff best[slot[i]] carries row i and count[slot[i]] >= min_count; the winners are compacted by the
//             count / scan / place scheme of compact.h over chunks of VX_CHUNK consecutive points, i.e. in ascending row.
#include "common.h"
#include "compact.h"
#include <cmath>

namespace a3r {

constexpr int VX_TPB = 256;
constexpr int VX_PPT = 4;                       // consecutive points per thread of the flag passes
constexpr int VX_CHUNK = VX_TPB * VX_PPT;
constexpr unsigned long long VX_EMPTY = ~0ull;
constexpr unsigned VX_NONE = 0xffffffffu;       // slot[i] of a point that is in no voxel
constexpr double VX_RANGE = 1048576.0;          // 2^20
constexpr double VX_FIX = 16777216.0;           // 2^24: the fixed-point step of the mean
constexpr long long VX_MAX_SLOTS = 1ll << 31;   // slot numbers are 32-bit words with VX_NONE set aside
#ifndef A3R_VOXEL_COMBINE
#define A3R_VOXEL_COMBINE 1
#endif
constexpr bool VX_COMBINE = A3R_VOXEL_COMBINE != 0;     // the insert pass folds runs of equal keys inside a wave (DESIGN 6.15 has the A/B)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct VoxelTable {
    unsigned long long* keys;       // [slots]
    unsigned long long* best;       // [slots]
    unsigned* count;                // [slots]
    unsigned long long* sums;       // [slots, 6] (mean mode: sum t_x, t_y, t_z, r, g, b) or null
    unsigned* slot;                 // [M]
    int* offsets;                   // [nchunks + 1]
    unsigned* head;                 // [0]: error word, [1]: dropped points
    unsigned long long mask;        // slots - 1
};

template <bool MEAN>
__global__ __launch_bounds__(VX_TPB) void voxel_fill_kernel(VoxelTable t) {
    const unsigned long long i = (unsigned long long)blockIdx.x * VX_TPB + threadIdx.x;
    if (i == 0) { t.head[0] = 0u; t.head[1] = 0u; }
    if (i > t.mask) return;
    t.keys[i] = VX_EMPTY;
    t.best[i] = VX_EMPTY;
    t.count[i] = 0u;
    if (MEAN) {                     // 48 bytes, 16-byte aligned
        ulonglong2* s = reinterpret_cast<ulonglong2*>(t.sums + i * 6);
        s[0] = s[1] = s[2] = make_ulonglong2(0ull, 0ull);
    }
}

// murmur3's 64-bit finaliser
__device__ __forceinline__ unsigned long long voxel_hash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// larger priority -> smaller word; NaN -> all ones (no other float maps there)
__device__ __forceinline__ unsigned voxel_priority_word(float p) {
    if (p != p) return 0xffffffffu;
    const unsigned b = __float_as_uint(p);
    return ~(b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u));
}

// One probe sequence: the slot that holds `key`, claimed if need be; VX_NONE after mask + 1 probes without a free slot.
__device__ __forceinline__ unsigned voxel_find_slot(const VoxelTable& t, unsigned long long key) {
    unsigned long long h = voxel_hash(key) & t.mask;
    for (unsigned long long n = 0; n <= t.mask; n++) {
        unsigned long long k = __hip_atomic_load(t.keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == VX_EMPTY) {
            const unsigned long long prev = atomicCAS(t.keys + h, VX_EMPTY, key);
            k = prev == VX_EMPTY ? key : prev;
        }
        if (k == key) return (unsigned)h;
        h = (h + 1) & t.mask;
    }
    return VX_NONE;
}

// COMBINE: neighbouring lanes of a wave that share a key -- a run: consecutive rows are consecutive pixels, which mostly fall
// into the same cell -- fold their value (minimum), count and sums (integer adds) into the run's first lane by a segmented
// suffix reduction, and that lane alone probes and issues the atomics.  Integer minima and sums: the table ends with the same
// words whatever is combined.
template <bool PRIO, bool MEAN, bool RGB, bool COMBINE>
__global__ __launch_bounds__(VX_TPB) void voxel_insert_kernel(const float* __restrict__ xyz, const float* __restrict__ priority,
                                                             const unsigned char* __restrict__ rgb, int M, double voxel, VoxelTable t) {
    const long long i = (long long)blockIdx.x * VX_TPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = i < M;
    bool in = false;
    unsigned long long key = 0ull, fix[3] = {0ull, 0ull, 0ull};
    if (live) {
        in = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double r = (double)xyz[(size_t)i * 3 + a] / voxel;
            const double q = floor(r);
            const bool ok = q >= -VX_RANGE && q < VX_RANGE;          // false for NaN and +-inf
            in = in && ok;
            key = (key << 21) | (ok ? (unsigned long long)(long long)(q + VX_RANGE) : 0ull);
            if (MEAN) fix[a] = ok ? (unsigned long long)floor((r - q) * VX_FIX) : 0ull;
        }
    }
    // no lane leaves before the end of the kernel: one add of the dropped points per wave, and the shuffles below see every lane
    const unsigned long long d = __ballot(live && !in);
    if (lane == 0 && d != 0ull) atomicAdd(t.head + 1, (unsigned)__popcll(d));
    unsigned long long value = VX_EMPTY;
    unsigned cnt = in ? 1u : 0u, col[3] = {0u, 0u, 0u};
    if (in) {
        value = ((unsigned long long)(PRIO ? voxel_priority_word(priority[i]) : 0u) << 32) | (unsigned)i;
        if (RGB) {
#pragma unroll
            for (int c = 0; c < 3; c++) col[c] = rgb[(size_t)i * 3 + c];
        }
    }
    bool head = in;
    unsigned long long below_or_self = 0ull;                        // COMBINE: the heads at or below this lane
    if (COMBINE) {
        const unsigned long long prev_key = __shfl_up(key, 1);
        const int prev_in = __shfl_up((int)in, 1);
        head = in && (lane == 0 || !prev_in || prev_key != key);
        below_or_self = __ballot(head) & (~0ull >> (63 - lane));
        // the run's number; a lane that is in no voxel gets a number of its own, so nothing folds into or across it
        const int run = in ? __popcll(below_or_self) : -1 - lane;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {                          // after the step a lane holds its run's lanes [lane, lane + 2 s)
            const int run_s = __shfl_down(run, s);                  // by every lane: a shuffle reads nothing from a lane that sits it out
            const bool take = lane + s < 64 && run_s == run;
            const unsigned long long v = __shfl_down(value, s);
            const unsigned n = __shfl_down(cnt, s);
            if (take) { value = v < value ? v : value; cnt += n; }
            if (MEAN) {
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const unsigned long long f = __shfl_down(fix[a], s);
                    if (take) fix[a] += f;
                }
                if (RGB) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const unsigned k = __shfl_down(col[c], s);
                        if (take) col[c] += k;
                    }
                }
            }
        }
    }
    unsigned slot = VX_NONE;
    if (head) {
        slot = voxel_find_slot(t, key);
        if (slot != VX_NONE) {
            // a stale value read here is an upper bound of the current one: a skipped minimum would not have changed the word
            if (__hip_atomic_load(t.best + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > value) atomicMin(t.best + slot, value);
            atomicAdd(t.count + slot, cnt);
            if (MEAN) {
                unsigned long long* sum = t.sums + (size_t)slot * 6;
#pragma unroll
                for (int a = 0; a < 3; a++) atomicAdd(sum + a, fix[a]);
                if (RGB) {
#pragma unroll
                    for (int c = 0; c < 3; c++) atomicAdd(sum + 3 + c, (unsigned long long)col[c]);
                }
            }
        } else {
            atomicOr(t.head, 1u);       // unreachable while slots > M (a free slot exists); a guard, not a path
        }
    }
    if (COMBINE) {                      // every lane of a run takes the slot of the run's first lane
        const int head_lane = in ? 63 - __clzll(below_or_self) : lane;
        const unsigned s = __shfl(slot, head_lane);
        if (in) slot = s;
    }
    if (live) t.slot[i] = slot;
}

struct VoxelOut {
    const float* xyz;               // inputs
    const unsigned char* rgb;
    double voxel;
    float* out_xyz;                 // [V, 3]
    unsigned char* out_rgb;         // [V, 3] or null
    int* out_index;                 // [V] or null
    int* out_count;                 // [V] or null
};

// grid (nchunks).  WRITE = false: offsets[chunk] = winners of the chunk.  WRITE = true: winner i goes to offsets[chunk] + its rank
// inside the chunk.
template <bool WRITE, bool MEAN>
__global__ __launch_bounds__(VX_TPB) void voxel_compact_kernel(VoxelTable t, int M, unsigned min_count, VoxelOut o) {
    __shared__ int wave_total[VX_TPB / 64];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * VX_CHUNK + tid * VX_PPT;
    unsigned s[VX_PPT], cnt[VX_PPT];
    if (p0 + VX_PPT <= M) {         // the slot array is 16-byte aligned and p0 a multiple of 4
        const u32x4 s4 = *reinterpret_cast<const u32x4*>(t.slot + p0);
        s[0] = s4.x; s[1] = s4.y; s[2] = s4.z; s[3] = s4.w;
    } else {
#pragma unroll
        for (int i = 0; i < VX_PPT; i++) s[i] = p0 + i < M ? t.slot[p0 + i] : VX_NONE;
    }
    bool keep[VX_PPT];
#pragma unroll
    for (int i = 0; i < VX_PPT; i++) {
        keep[i] = false; cnt[i] = 0u;
        if (s[i] != VX_NONE) {
            cnt[i] = t.count[s[i]];
            keep[i] = (unsigned)t.best[s[i]] == (unsigned)(p0 + i) && cnt[i] >= min_count;
        }
    }
    // the threads own consecutive point quads, so the order is (thread, i)
    int first, total;
    block_rank<VX_TPB, VX_PPT>(keep, wave_total, &first, &total);
    if (!WRITE) {
        if (tid == 0) t.offsets[blockIdx.x] = total;
        return;
    }
    // the count pass saw the same table, so these are its ranks; stay inside the chunk's range whatever the workspace holds
    const long long end = t.offsets[blockIdx.x + 1];
    long long l = (long long)t.offsets[blockIdx.x] + first;
#pragma unroll
    for (int i = 0; i < VX_PPT; i++) {
        if (!keep[i] || l >= end) continue;
        const size_t p = (size_t)(p0 + i);
        if (o.out_index) o.out_index[l] = (int)p;
        if (o.out_count) o.out_count[l] = (int)cnt[i];
        if (!MEAN) {
#pragma unroll
            for (int a = 0; a < 3; a++) o.out_xyz[l * 3 + a] = o.xyz[p * 3 + a];
            if (o.out_rgb) {
#pragma unroll
                for (int c = 0; c < 3; c++) o.out_rgb[l * 3 + c] = o.rgb[p * 3 + c];
            }
        } else {
            const unsigned long long key = t.keys[s[i]];
            const unsigned long long* sum = t.sums + (size_t)s[i] * 6;
            const double n = (double)cnt[i];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const double q = (double)((key >> (21 * (2 - a))) & 0x1fffffull) - VX_RANGE;
                o.out_xyz[l * 3 + a] = (float)((q + ((double)sum[a] + 0.5 * n) / (n * VX_FIX)) * o.voxel);
            }
            if (o.out_rgb) {
#pragma unroll
                for (int c = 0; c < 3; c++)
                    o.out_rgb[l * 3 + c] = (unsigned char)((2ull * sum[3 + c] + cnt[i]) / (2ull * cnt[i]));
            }
        }
        l++;
    }
}

static long long voxel_nchunks(long long M) { return (M + VX_CHUNK - 1) / VX_CHUNK; }

static long long voxel_default_slots(long long M) {
    long long s = 1;
    while (s < 2 * M && s < VX_MAX_SLOTS) s <<= 1;
    return s;
}

static bool voxel_sizes_ok(long long M, long long slots, int reduce) {
    return M >= 0 && M < (1ll << 31) && (reduce == A3R_VOXEL_BEST || reduce == A3R_VOXEL_MEAN) && slots > M && slots <= VX_MAX_SLOTS &&
           (slots & (slots - 1)) == 0;
}

// head | offsets [nchunks + 1] | slot [M] | keys [slots] | best [slots] | count [slots] | sums [slots, 6] (mean), each part rounded
// up to 256 bytes
static size_t voxel_head_bytes() { return 256; }
static size_t voxel_offsets_bytes(long long M) { return compact_offsets_bytes((size_t)voxel_nchunks(M)); }
static size_t voxel_slot_bytes(long long M) { return align_up((size_t)M * sizeof(unsigned), 256); }

}  // namespace a3r

// =============================================================================================== host
using namespace a3r;

extern "C" size_t a3r_voxel_workspace_bytes(long long M, long long slots, int reduce) {
    if (slots == 0 && M >= 0 && M < (1ll << 31)) slots = voxel_default_slots(M);
    if (!voxel_sizes_ok(M, slots, reduce)) return 0;
    const size_t S = (size_t)slots;
    return voxel_head_bytes() + voxel_offsets_bytes(M) + voxel_slot_bytes(M) + align_up(S * 8, 256) * 2 + align_up(S * 4, 256) +
           (reduce == A3R_VOXEL_MEAN ? align_up(S * 48, 256) : 0);
}

// fill, insert, flag, scan; V and the dropped count come back to the host (synchronises the stream).  mean_sums: the insert pass also
// accumulates the sums the placement pass of mean mode reads.
static int voxel_count(const char* who, const float* xyz, const float* priority, const unsigned char* rgb, long long M, double voxel,
                       int reduce, int min_count, long long slots, void* ws, size_t ws_bytes, bool mean_sums, hipStream_t st,
                       VoxelTable* t, long long* n_voxels, long long* dropped) {
    A3R_CHECK_ARG(M >= 0 && M < (1ll << 31), "%s: M = %lld: the point count is in [0, 2^31)", who, M);
    A3R_CHECK_ARG(reduce == A3R_VOXEL_BEST || reduce == A3R_VOXEL_MEAN, "%s: reduce = %d is neither A3R_VOXEL_BEST nor A3R_VOXEL_MEAN", who,
                  reduce);
    A3R_CHECK_ARG(std::isfinite(voxel) && voxel > 0, "%s: voxel = %g must be finite and positive", who, voxel);
    A3R_CHECK_ARG(min_count >= 1, "%s: min_count = %d must be at least 1", who, min_count);
    if (slots == 0) slots = voxel_default_slots(M);
    A3R_CHECK_ARG(slots > 0 && (slots & (slots - 1)) == 0, "%s: slots = %lld is not a power of two", who, slots);
    A3R_CHECK_ARG(slots > M, "%s: slots = %lld must exceed the %lld points (a free slot ends every probe)", who, slots, M);
    A3R_CHECK_ARG(slots <= VX_MAX_SLOTS, "%s: slots = %lld is above 2^31", who, slots);
    A3R_CHECK_ARG(xyz || M == 0, "%s: null xyz", who);
    const size_t need = a3r_voxel_workspace_bytes(M, slots, reduce);
    if (int rc = check_workspace(who, ws, ws_bytes, need)) return rc;
    *n_voxels = 0;
    *dropped = 0;
    if (M == 0) return A3R_OK;

    const size_t S = (size_t)slots;
    char* p = static_cast<char*>(ws);
    t->head = reinterpret_cast<unsigned*>(p);              p += voxel_head_bytes();
    t->offsets = reinterpret_cast<int*>(p);                p += voxel_offsets_bytes(M);
    t->slot = reinterpret_cast<unsigned*>(p);              p += voxel_slot_bytes(M);
    t->keys = reinterpret_cast<unsigned long long*>(p);    p += align_up(S * 8, 256);
    t->best = reinterpret_cast<unsigned long long*>(p);    p += align_up(S * 8, 256);
    t->count = reinterpret_cast<unsigned*>(p);             p += align_up(S * 4, 256);
    t->sums = mean_sums ? reinterpret_cast<unsigned long long*>(p) : nullptr;
    t->mask = (unsigned long long)slots - 1;

    const dim3 tpb(VX_TPB);
    const dim3 fill_grid((unsigned)((S + VX_TPB - 1) / VX_TPB)), point_grid((unsigned)((M + VX_TPB - 1) / VX_TPB));
    const int T = (int)voxel_nchunks(M);
    const bool colour = mean_sums && rgb;
    if (mean_sums) hipLaunchKernelGGL((voxel_fill_kernel<true>), fill_grid, tpb, 0, st, *t);
    else           hipLaunchKernelGGL((voxel_fill_kernel<false>), fill_grid, tpb, 0, st, *t);
#define A3R_VX_INSERT(PR, MN, CL) \
    hipLaunchKernelGGL((voxel_insert_kernel<PR, MN, CL, VX_COMBINE>), point_grid, tpb, 0, st, xyz, priority, rgb, (int)M, voxel, *t)
#define A3R_VX_INSERT_MODE(PR) \
    do { if (colour) A3R_VX_INSERT(PR, true, true); else if (mean_sums) A3R_VX_INSERT(PR, true, false); else A3R_VX_INSERT(PR, false, false); } while (0)
    if (priority) A3R_VX_INSERT_MODE(true); else A3R_VX_INSERT_MODE(false);
#undef A3R_VX_INSERT_MODE
#undef A3R_VX_INSERT
    hipLaunchKernelGGL((voxel_compact_kernel<false, false>), dim3(T), tpb, 0, st, *t, (int)M, (unsigned)min_count, VoxelOut{});
    compact_scan(t->offsets, T, st);
    A3R_LAUNCH_CHECK();
    unsigned head[2] = {0u, 0u};
    int total = 0;
    A3R_HIP(hipMemcpyAsync(head, t->head, sizeof(head), hipMemcpyDeviceToHost, st));
    A3R_HIP(compact_read_total(t->offsets, T, &total, st));
    A3R_HIP(hipStreamSynchronize(st));
    if (head[0] != 0u) {
        set_error("%s: a probe walked all %lld slots without finding a free one (the table was not the one this call filled)", who, slots);
        return A3R_ESTATE;
    }
    *n_voxels = total;
    *dropped = head[1];
    return A3R_OK;
}

extern "C" int a3r_voxel_count(const float* xyz, const float* priority, long long M, double voxel, int reduce, int min_count, long long slots,
                               void* ws, size_t ws_bytes, long long* n_voxels_host, long long* dropped_host, void* stream) {
    const char* who = "a3r_voxel_count";
    A3R_CHECK_ARG(n_voxels_host && dropped_host, "%s: null n_voxels_host / dropped_host", who);
    VoxelTable t;
    return voxel_count(who, xyz, priority, nullptr, M, voxel, reduce, min_count, slots, ws, ws_bytes, false, as_stream(stream), &t,
                       n_voxels_host, dropped_host);
}

extern "C" int a3r_voxel_export(const float* xyz, const float* priority, const unsigned char* rgb, long long M, double voxel, int reduce,
                                int min_count, long long slots, void* ws, size_t ws_bytes, long long capacity, float* out_xyz,
                                unsigned char* out_rgb, int* out_index, int* out_count, long long* n_voxels_host, long long* dropped_host,
                                void* stream) {
    const char* who = "a3r_voxel_export";
    A3R_CHECK_ARG(n_voxels_host && dropped_host, "%s: null n_voxels_host / dropped_host", who);
    A3R_CHECK_ARG(capacity >= 0, "%s: negative capacity", who);
    A3R_CHECK_ARG(out_xyz || capacity == 0, "%s: null out_xyz (only a capacity of 0 needs no buffer)", who);
    A3R_CHECK_ARG(!out_rgb || rgb || M == 0, "%s: out_rgb needs the rgb source buffer", who);
    hipStream_t st = as_stream(stream);
    VoxelTable t;
    const bool mean = reduce == A3R_VOXEL_MEAN;
    // the count is always taken afresh: the table and the offsets in the workspace then belong to exactly these inputs
    if (int rc = voxel_count(who, xyz, priority, out_rgb ? rgb : nullptr, M, voxel, reduce, min_count, slots, ws, ws_bytes, mean, st, &t,
                             n_voxels_host, dropped_host))
        return rc;
    const long long V = *n_voxels_host;
    A3R_CHECK_ARG(V <= capacity, "%s: capacity %lld is smaller than the %lld kept voxels (nothing was written)", who, capacity, V);
    if (V == 0) return A3R_OK;
    const VoxelOut o{xyz, out_rgb ? rgb : nullptr, voxel, out_xyz, out_rgb, out_index, out_count};
    const dim3 grid((unsigned)voxel_nchunks(M)), tpb(VX_TPB);
    if (mean) hipLaunchKernelGGL((voxel_compact_kernel<true, true>), grid, tpb, 0, st, t, (int)M, (unsigned)min_count, o);
    else      hipLaunchKernelGGL((voxel_compact_kernel<true, false>), grid, tpb, 0, st, t, (int)M, (unsigned)min_count, o);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
