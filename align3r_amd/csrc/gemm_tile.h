// Tile scaffold shared by the MFMA GEMM kernels of liba3r (gemm.hip, gemm_bf3.hip, gemm_fh2.hip): the launch arguments, the
// workgroup id -> (group, tile) maps, the counted vmcnt wait, the bf3 product ladder, and on the host the tile bookkeeping and the
// launch itself.  Included through gemm_common.h.  The kernels are sensitive to source motion (several sit at the register cap and
// carry scratch), so a device helper lives here only where the kernels that use it were compared instruction by instruction:
// gemm.hip and gemm_fh2.hip keep the remap written out, and the conv geometry stays written out in both LDS-DMA kernels.
#pragma once
#include "common.h"
#include "bf3.h"

namespace a3r {

struct GroupPtrs {
    const float* A;
    const float* Wt;        // [N, K]
    float* C;
    const float* bias;
    const float* resid;
    const float* resid2;
    // fh2 kernels: the power of two the out_fh2 / aux_fh2 output is stored with, and the word receiving max |out_scale * value| (or null)
    float out_scale;
    unsigned* out_absmax;
};

struct GemmArgs {
    GroupPtrs grp[4];
    int groups, tiles_per_group;
    int lda, ldc;
    int M, N, K;
    int tiles_m, tiles_n;
    a3r_epilogue epi;       // pointers inside are ignored (taken from grp[]) except the rope tables
    // implicit conv (AMODE 1): A = x [B, H, W, Cin]
    int cH, cW, cCin, cHo, cWo, cStride;
    int direct_epilogue;    // A/B switch (env A3R_BF3_DIRECT_EPI): keep the accumulator-layout epilogue instead of the LDS-staged one
};

// XCD-aware bijective remap of the workgroup id (blocks b and b+8 share an XCD: each XCD walks a contiguous run of tiles, its L2 is
// private), then the group split: -> the tile id within the group, grp = the group
__device__ __forceinline__ int tile_in_group(int tiles_per_group, int groups, int& grp) {
    const int nwg = tiles_per_group * groups;
    const int orig = blockIdx.x;
    const int xcd = orig & 7, q = nwg >> 3, r8 = nwg & 7;
    const int wgid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (orig >> 3);
    grp = wgid / tiles_per_group;
    return wgid - grp * tiles_per_group;
}
// row-major tile order
__device__ __forceinline__ void tile_row_major(int tile, int tiles_n, int& tile_m, int& tile_n) {
    tile_m = tile / tiles_n;
    tile_n = tile - tile_m * tiles_n;
}

// ---- s_waitcnt vmcnt takes an immediate: dispatch over the counts that occur (stages in flight x DMAs per stage per wave).  A count
// that is not listed falls to vmcnt(0) -- correct, but it drains the pipeline -- so every kernel asserts vmcnt_stages_listed for
// the counts it can request.
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
constexpr bool vmcnt_listed(int n) { return (n >= 0 && n <= 10) || n == 12; }
__device__ __forceinline__ void wait_vmcnt_dyn(int n) {
    switch (n) {
        case 0: wait_vmcnt<0>(); break;   case 1: wait_vmcnt<1>(); break;   case 2: wait_vmcnt<2>(); break;
        case 3: wait_vmcnt<3>(); break;   case 4: wait_vmcnt<4>(); break;   case 5: wait_vmcnt<5>(); break;
        case 6: wait_vmcnt<6>(); break;   case 7: wait_vmcnt<7>(); break;   case 8: wait_vmcnt<8>(); break;
        case 9: wait_vmcnt<9>(); break;   case 10: wait_vmcnt<10>(); break; case 12: wait_vmcnt<12>(); break;
        default: wait_vmcnt<0>(); break;                                    // always safe
    }
}
// s * lps is a listed count (listed: the predicate of the dispatch in use) for every s < stages (stages = the most stages a kernel
// leaves in flight, plus one)
constexpr bool vmcnt_stages_listed(bool (*listed)(int), int stages, int lps) {
    for (int s = 0; s < stages; s++)
        if (!listed(s * lps)) return false;
    return true;
}

// ---- one k-step of the bf3 product a0b0 + (a0b1 + a1b0) + (a0b2 + a1b1 + a2b0) on one 16x16 accumulator (v_mfma_f32_16x16x32_bf16),
// smallest terms first.  NP: 6 = all of it, 3 = without the last group, 1 = a0b0 alone.
template <int NP>
__device__ __forceinline__ void bf3_mma(f32x4& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
    if (NP == 6) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], acc, 0, 0, 0);
    }
    if (NP >= 3) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
}

// ---- host side
// tiles of bm x bn over the problem -> g.tiles_m / tiles_n / tiles_per_group; returns whether every tile is full
static inline bool set_tiles(GemmArgs& g, int bm, int bn) {
    g.tiles_m = (g.M + bm - 1) / bm;
    g.tiles_n = (g.N + bn - 1) / bn;
    g.tiles_per_group = g.tiles_m * g.tiles_n;
    return g.M % bm == 0 && g.N % bn == 0;
}

// one workgroup per tile and group; the dynamic-LDS attribute of KERN is set once per device
template <auto KERN, int THREADS, int LDS, class Args>
static int launch_tiles(const GemmArgs& g, const Args& args, hipStream_t st) {
    static_assert(LDS <= 160 * 1024, "LDS budget");
    static PerDeviceOnce attr_once;
    A3R_HIP(attr_once.ensure([&] { return hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, LDS); }));
    hipLaunchKernelGGL(KERN, dim3(g.tiles_per_group * g.groups), dim3(THREADS), LDS, st, args);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

}  // namespace a3r
