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

}  // namespace

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
