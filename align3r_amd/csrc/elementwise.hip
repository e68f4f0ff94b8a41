// HBM-bound kernels of the pair forward: LayerNorm, standalone RoPE-2D, patchify, bilinear x2,
// final 1x1 conv + postprocess, weight repacking.  All fp32, 16-byte vector accesses where the
// layout allows, one wave per row for the row reductions (64-wide DPP/shuffle sums).
#include "common.h"
#include "bf3.h"
#include "fh2.h"
#include "dedup.h"
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace a3r {

// ------------------------------------------------------------------------------------------- pieces the kernels below share
// The sum and the sum of squares of a float4, added left to right, and LayerNorm's affine step.  The products of sumsq4 are not
// fused into its sums and the affine step is an explicit fma (contraction is off here as in every kernel that calls these): the
// output forms of one operator must round identically (bf3 / fh2 output == split of the fp32 output, tested).
__device__ __forceinline__ float sum4(f32x4 v) { return v.x + v.y + v.z + v.w; }
__device__ __forceinline__ float sumsq4(f32x4 v) {
#pragma clang fp contract(off)
    return v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
}
__device__ __forceinline__ f32x4 ln_affine4(f32x4 v, float rstd, f32x4 wv, f32x4 bv) {
#pragma clang fp contract(off)
    const f32x4 t = v * rstd;
    return f32x4{__builtin_fmaf(t.x, wv.x, bv.x), __builtin_fmaf(t.y, wv.y, bv.y), __builtin_fmaf(t.z, wv.z, bv.z),
                 __builtin_fmaf(t.w, wv.w, bv.w)};
}
// The tail of an fh2 producer for one 8-k group: scale, range statistics, the two planes' 16-byte units.
__device__ __forceinline__ void fh2_emit8(char* row, int k0, f32x4 lo, f32x4 hi, float scale, float& amax) {
    lo = lo * scale;
    hi = hi * scale;
    amax = fh2_amax4(fh2_amax4(amax, lo), hi);
    fh2_store8(row, k0, lo, hi);
}
// The residual combine for one float4 (combine_resid_fh2_kernel below): v = c + (r0 + p2), the epilogue's order of additions, goes
// to *s; relu(v) * scale, which enters the range statistics, is returned for the caller's fh2_store8.
__device__ __forceinline__ f32x4 combine_emit(f32x4 c, f32x4 r0, f32x4 p2, f32x4* s, float scale, float& amax) {
    const f32x4 v = c + (r0 + p2);
    *s = v;
    const f32x4 o = f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)} * scale;
    amax = fh2_amax4(amax, o);
    return o;
}

// ------------------------------------------------------------------------------------------- LayerNorm
// nn.LayerNorm(D, eps) (croco.py:34; blocks.py:118-123,180-185): one wave per row, row kept in registers.
// BF3: write the normalised row in bf3 form (bf3.h) instead of fp32 -- the input format of gemm_bf3.hip.
template <int VPL, bool BF3>   // float4 per lane: D = 256 * VPL
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ b, float* __restrict__ y, int M,
                                                         int D, float eps, int pair) {
#pragma clang fp contract(off)      // the fp32 and the bf3 instantiation must round identically (bf3 output == split of the fp32 one)
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
    f32x4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        v[i] = xr[lane + 64 * i];
        s += sum4(v[i]);
    }
    const float mean = wave_sum(s) / (float)D;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        v[i] = v[i] - mean;
        ss += sumsq4(v[i]);
    }
    const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)D + eps);
    f32x4* yr = reinterpret_cast<f32x4*>(y + (size_t)row * D);
    const f32x4* wr = reinterpret_cast<const f32x4*>(w);
    const f32x4* br = reinterpret_cast<const f32x4*>(b);
    char* y3 = reinterpret_cast<char*>(y) + bf3_row_offset(row, D, pair);
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const f32x4 o = ln_affine4(v[i], rstd, wr[lane + 64 * i], br[lane + 64 * i]);
        if (BF3) bf3_store4(y3, (lane + 64 * i) * 4, o, pair);
        else yr[lane + 64 * i] = o;
    }
}

// Row-PAIR bf3 output (the layout every transformer GEMM input uses, bf3.h): ONE WAVE NORMALISES TWO ROWS (2j, 2j + 1) and
// stores their interleaved image -- 12 D contiguous bytes -- through LDS as whole 1 KB wave stores.  The one-row form above writes
// a row's planes as 8-byte pieces, 16 of every 48 bytes per instruction (a lane owns 4 consecutive k = half of each plane's
// 16-byte unit), and in the pair layout a single row is 192-byte runs at a 384-byte stride; here every store instruction covers
// eight whole cache lines, and the two rows' loads and reductions are in flight together.  Same arithmetic, same rounding.
template <int VPL>
__global__ __launch_bounds__(256) void layernorm_pair_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ b, char* __restrict__ y3, int M, int D, float eps) {
#pragma clang fp contract(off)
    // per wave two 3 KB images: the pair's 256 k of one step i (8 k-blocks x 384 B, contiguous in the pair layout), double-buffered
    __shared__ __attribute__((aligned(16))) char img_all[4][2][3072];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r0 = (blockIdx.x * 4 + wave) * 2;
    if (r0 >= M) return;                                                        // wave-uniform; M is even in this layout's callers
    const bool two = r0 + 1 < M;
    const f32x4* x0 = reinterpret_cast<const f32x4*>(x + (size_t)r0 * D);
    const f32x4* x1 = reinterpret_cast<const f32x4*>(x + (size_t)(two ? r0 + 1 : r0) * D);
    f32x4 v0[VPL], v1[VPL];
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        v0[i] = x0[lane + 64 * i];
        v1[i] = x1[lane + 64 * i];
    }
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        s0 += sum4(v0[i]);
        s1 += sum4(v1[i]);
    }
    const float mean0 = wave_sum(s0) / (float)D, mean1 = wave_sum(s1) / (float)D;
    float ss0 = 0.f, ss1 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        v0[i] = v0[i] - mean0;
        v1[i] = v1[i] - mean1;
        ss0 += sumsq4(v0[i]);
        ss1 += sumsq4(v1[i]);
    }
    const float rstd0 = 1.f / sqrtf(wave_sum(ss0) / (float)D + eps), rstd1 = 1.f / sqrtf(wave_sum(ss1) / (float)D + eps);
    const f32x4* wr = reinterpret_cast<const f32x4*>(w);
    const f32x4* br = reinterpret_cast<const f32x4*>(b);
    char* dst = y3 + (size_t)(r0 >> 1) * ((size_t)12 * D);
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        char* img = img_all[wave][i & 1];
        const f32x4 wv = wr[lane + 64 * i], bv = br[lane + 64 * i];
        bf3_store4(img, lane * 4, ln_affine4(v0[i], rstd0, wv, bv), 1);        // row parity 0: offset 0 of every 384-byte k block
        bf3_store4(img + 192, lane * 4, ln_affine4(v1[i], rstd1, wv, bv), 1);  // row parity 1: + 192
        __builtin_amdgcn_s_waitcnt(0xc07f);                                    // lgkmcnt(0): the image is wave-private
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const int un = u * 64 + lane;
            const u32x4 dv = *reinterpret_cast<const u32x4*>(img + un * 16);
            if (two || ((un * 16) % 384) < 192) *reinterpret_cast<u32x4*>(dst + (size_t)i * 3072 + (size_t)un * 16) = dv;
        }
    }
}

// fh2 output (fh2.h; scale 1): one wave per row, a lane owns 8 CONSECUTIVE k per step (two adjacent float4 loads), so it writes the
// two planes' 16-byte units of its group -- 32 contiguous bytes per lane, 2 KB contiguous per wave and step.
template <int VPL, bool STATS>   // 8-k groups per lane: D <= 512 VPL (D % 8 == 0); a lane whose group lies past the row contributes zeros and stores nothing
__global__ __launch_bounds__(256) void layernorm_fh2_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ b, char* __restrict__ y2, int M, int D, float eps,
                                                             float scale, unsigned* __restrict__ absmax) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int G = D >> 3;                                      // groups of 8 consecutive k in a row
    float amax = 0.f;
    // persistent rows loop (the grid is capped): the range statistics cost one atomic per workgroup, not one per row
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += gridDim.x * 4) {
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
    f32x4 v[VPL][2];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const bool in = lane + 64 * i < G;
        v[i][0] = in ? xr[2 * (lane + 64 * i)] : f32x4{0.f, 0.f, 0.f, 0.f};
        v[i][1] = in ? xr[2 * (lane + 64 * i) + 1] : f32x4{0.f, 0.f, 0.f, 0.f};
        s += sum4(v[i][0]) + sum4(v[i][1]);
    }
    const float mean = wave_sum(s) / (float)D;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        const bool in = lane + 64 * i < G;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            v[i][h] = v[i][h] - mean;
            if (in) ss += sumsq4(v[i][h]);
        }
    }
    const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)D + eps);
    const f32x4* wr = reinterpret_cast<const f32x4*>(w);
    const f32x4* br = reinterpret_cast<const f32x4*>(b);
    char* yr = y2 + (size_t)row * fh2_row_bytes(D);
#pragma unroll
    for (int i = 0; i < VPL; i++) {
        if (lane + 64 * i >= G) continue;
        f32x4 o[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int c = 2 * (lane + 64 * i) + h;
            o[h] = ln_affine4(v[i][h], rstd, wr[c], br[c]) * scale;
            if (STATS) amax = fh2_amax4(amax, o[h]);
        }
        fh2_store8(yr, (lane + 64 * i) * 8, o[0], o[1]);
    }
    }
    if (STATS) {
        __shared__ unsigned s_red[4];
        fh2_publish_block(absmax, amax, s_red);
    }
}
// generic fallback, one wave per row, three passes over an L1/L2-resident row.  FMT 0: fp32 (any D % 4 == 0), 1: bf3 (D % 8 == 0),
// 2: fh2 (D % 32 == 0: lanes stride over the row's 8-k groups).  The rows loop is the persistent one of layernorm_fh2_kernel; the
// fp32 and bf3 launches have a workgroup per four rows, so it runs once there.
template <int FMT>
__global__ __launch_bounds__(256) void layernorm_generic_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ b, void* __restrict__ y, int M, int D, float eps,
                                                                 int pair, float scale, unsigned* __restrict__ absmax) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    float amax = 0.f;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += gridDim.x * 4) {
        const float* xr = x + (size_t)row * D;
        float s = 0.f;
        for (int i = lane; i < D; i += 64) s += xr[i];
        const float mean = wave_sum(s) / (float)D;
        float ss = 0.f;
        for (int i = lane; i < D; i += 64) { const float c = xr[i] - mean; ss += c * c; }
        const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)D + eps);
        auto out = [&](int k) { return __builtin_fmaf((xr[k] - mean) * rstd, w[k], b[k]); };
        if (FMT == 2) {
            char* yr = static_cast<char*>(y) + (size_t)row * fh2_row_bytes(D);
            for (int k0 = lane * 8; k0 < D; k0 += 512) {
                f32x4 o[2];
#pragma unroll
                for (int j = 0; j < 8; j++) o[j >> 2][j & 3] = out(k0 + j) * scale;
                amax = fh2_amax4(fh2_amax4(amax, o[0]), o[1]);
                fh2_store8(yr, k0, o[0], o[1]);
            }
        } else if (FMT == 1) {
            char* y3 = static_cast<char*>(y) + bf3_row_offset(row, D, pair);
            for (int i = lane * 4; i < D; i += 256) {
                f32x4 o;
#pragma unroll
                for (int j = 0; j < 4; j++) o[j] = out(i + j);
                bf3_store4(y3, i, o, pair);
            }
        } else {
            float* yr = static_cast<float*>(y) + (size_t)row * D;
            for (int i = lane; i < D; i += 64) yr[i] = out(i);
        }
    }
    if (FMT == 2) {
        __shared__ unsigned s_red[4];
        fh2_publish_block(absmax, amax, s_red);
    }
}

// ------------------------------------------------------------------------------------------- RoPE-2D (standalone)
// curope.rope_2d semantics (curope.cpp:11-47, kernels.cu:17-82): tokens [B,N,H,D] in place.
__global__ void rope2d_kernel(float* tok, const int64_t* pos, int B, int N, int H, int D, float base, float fwd) {
    const int Q = D / 4;
    const long total = (long)B * N * H * 2 * Q;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int q = (int)(i % Q);
        long r = i / Q;
        const int xy = (int)(r % 2); r /= 2;
        const int hh = (int)(r % H); r /= H;      // r = b*N + n
        const float p = (float)pos[r * 2 + xy];
        const float ang = fwd * p / powf(base, (float)q / (float)Q);
        const float c = cosf(ang), s = sinf(ang);
        float* t = tok + (r * H + hh) * (long)D + xy * 2 * Q + q;
        const float u = t[0], v = t[Q];
        t[0] = u * c - v * s;
        t[Q] = v * c + u * s;
    }
}

// ------------------------------------------------------------------------------------------- patchify
// cols[(b*nh + ty)*nw + tx][c*256 + py*16 + px] = img(b, c, ty*16+py, tx*16+px)
__global__ void patchify_kernel(const float* __restrict__ img, float* __restrict__ cols, int B, int C, int H, int W,
                                long sb, long sc, long sy, long sx) {
    const int nh = H / 16, nw = W / 16, K = C * 256;
    const long total = (long)B * nh * nw * K;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const long t = i / K;
        const int tx = (int)(t % nw), ty = (int)((t / nw) % nh), b = (int)(t / ((long)nw * nh));
        const int c = k >> 8, py = (k >> 4) & 15, px = k & 15;
        cols[i] = img[b * sb + c * sc + (long)(ty * 16 + py) * sy + (long)(tx * 16 + px) * sx];
    }
}

// the same for the U distinct items of a batch (dedup.h): row block k is item uniq[k] of the 2 B items img_a[0..B), img_b[0..B)
__global__ void patchify_indexed_kernel(const float* __restrict__ img_a, const float* __restrict__ img_b, const int* __restrict__ uniq,
                                        float* __restrict__ cols, int U, int B, int C, int H, int W, long sb, long sc, long sy, long sx) {
    const int nh = H / 16, nw = W / 16, K = C * 256;
    const long total = (long)U * nh * nw * K;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const long t = i / K;
        const int tx = (int)(t % nw), ty = (int)((t / nw) % nh), u = (int)(t / ((long)nw * nh));
        const int c = k >> 8, py = (k >> 4) & 15, px = k & 15;
        const int s = uniq[u];
        const float* img = s < B ? img_a + s * sb : img_b + (s - B) * sb;
        cols[i] = img[c * sc + (long)(ty * 16 + py) * sy + (long)(tx * 16 + px) * sx];
    }
}

// rows of the distinct items back to every slot that holds one: dst row block s = src row block map[s], blocks of N rows of C4 float4
__global__ void gather_rows_kernel(const f32x4* __restrict__ src, f32x4* __restrict__ dst, const int* __restrict__ map, int S, long NC4) {
    const long total = (long)S * NC4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int s = (int)(i / NC4);
        dst[i] = src[(long)map[s] * NC4 + (i - s * NC4)];
    }
}

// the residual add of a linear that ran on distinct items only: dst row block s = a[map_a[s]] + b[map_b[s]], or with b null
// dst[s] + a[map_a[s]] in place (fp32 addition commutes: either order is the RESID epilogue's sum)
__global__ void gather_add_rows_kernel(const f32x4* __restrict__ a, const int* __restrict__ map_a, const f32x4* __restrict__ b,
                                       const int* __restrict__ map_b, f32x4* dst, int S, long NC4) {
    const long total = (long)S * NC4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int s = (int)(i / NC4);
        const long r = i - s * NC4;
        const f32x4 va = a[(long)map_a[s] * NC4 + r];
        const f32x4 vb = b ? b[(long)map_b[s] * NC4 + r] : dst[i];
        dst[i] = va + vb;
    }
}

// the same with the row blocks of a in two places (dedup.h, frame products): src[s] >= 0 names an entry of `store`, whose blocks lie
// stride4 float4 apart, src[s] < 0 the fresh block ~src[s]
__global__ void gather_add_rows_src_kernel(const f32x4* __restrict__ store, long stride4, const f32x4* __restrict__ fresh,
                                           const int* __restrict__ src, const f32x4* __restrict__ b, const int* __restrict__ map_b,
                                           f32x4* dst, int S, long NC4) {
    const long total = (long)S * NC4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int s = (int)(i / NC4);
        const long r = i - s * NC4;
        const int e = src[s];
        const f32x4 va = e >= 0 ? store[(long)e * stride4 + r] : fresh[(long)~e * NC4 + r];
        const f32x4 vb = b ? b[(long)map_b[s] * NC4 + r] : dst[i];
        dst[i] = va + vb;
    }
}

// ------------------------------------------------------------------------------------------- residual combine on distinct frames
// What the RESID2 epilogue of refinenet1.resConfUnit1's second conv produces, when that conv (and the skip it adds) ran on the U
// distinct frames of a side only (dedup.h): for slot b < S with k = map[b], per pixel row and channel
//     s[b] = c[k] + (r0[k] + p2[b])                (the epilogue's order: (acc + bias) + (resid + resid2), gemm_common.h)
//     sr2[b] = fh2 of relu(s[b]) * scale, max |stored| -> *absmax
// c, r0 [U, P, C], p2, s [S, P, C] fp32, sr2 [S P, C] fh2.  A thread makes 8 channels of one pixel row (two 16-byte loads per input,
// 32 contiguous bytes per output) and walks the rows with the grid's stride: the index divisions happen once per thread, and a
// workgroup publishes one statistics atomic.
//
// SRC (dedup.h, head products: c and r0 of a frame may lie in the caller's storage): map[b] is a signed source -- e >= 0 names the
// block of entry e, hs.stride floats apart from hs.c / hs.r0, e < 0 the fresh block ~e of c / r0.  Only the base pointers and the
// block index of the two loads differ, uniformly per slot; the arithmetic is the same code.
struct CombineSrc { const float *c, *r0; long stride; };
template <bool SRC>
__device__ __forceinline__ long combine_block(const CombineSrc& hs, int e, const float* __restrict__& c, const float* __restrict__& r0) {
    if (!SRC) return e;
    if (e < 0) return ~e;
    c = hs.c + (long)e * hs.stride;
    r0 = hs.r0 + (long)e * hs.stride;
    return 0;
}

template <bool SRC>
__global__ __launch_bounds__(256) void combine_resid_fh2_kernel(const float* __restrict__ c, const float* __restrict__ r0,
                                                                const float* __restrict__ p2, const int* __restrict__ map,
                                                                float* __restrict__ s, char* __restrict__ sr2, long rows, long P, int C8,
                                                                float scale, unsigned* __restrict__ absmax, CombineSrc hs) {
    const long stride = (long)gridDim.x * 256, i0 = (long)blockIdx.x * 256 + threadIdx.x;
    const long dr = stride / C8;
    const int dk = (int)(stride - dr * C8);
    long row = i0 / C8;
    int kg = (int)(i0 - row * C8);
    long b = row / P, pr = row - b * P;                        // slot, pixel row inside the slot
    float amax = 0.f;
    while (row < rows) {
        const float *__restrict__ cs = c, *__restrict__ rs = r0;
        const long blk = combine_block<SRC>(hs, map[b], cs, rs);
        const long src = ((blk * P + pr) * C8 + kg) * 2, dst = (row * C8 + kg) * 2;      // in float4
        f32x4 o[2];
#pragma unroll
        for (int h = 0; h < 2; h++)
            o[h] = combine_emit(reinterpret_cast<const f32x4*>(cs)[src + h], reinterpret_cast<const f32x4*>(rs)[src + h],
                                reinterpret_cast<const f32x4*>(p2)[dst + h], reinterpret_cast<f32x4*>(s) + dst + h, scale, amax);
        fh2_store8(sr2 + row * ((size_t)C8 * 32), kg * 8, o[0], o[1]);
        kg += dk; row += dr; pr += dr;
        if (kg >= C8) { kg -= C8; row++; pr++; }
        if (pr >= P) { const long q = pr / P; b += q; pr -= q * P; }
    }
    __shared__ unsigned s_red[4];
    fh2_publish_block(absmax, amax, s_red);                   // every thread arrives here
}

// ------------------------------------------------------------------------------------------- bilinear x2, align_corners=True
// Index arithmetic in fp32 exactly as ATen's upsample_bilinear2d (scale = (in-1)/(out-1); src = scale*dst).
// BF3: write the result in bf3 form (rows = output pixels, K = C) -- the input of the following 1x1 / 3x3 conv on the bf3 kernel.
// one fixed rounding order for the interpolation in every output format (products and fused multiply-adds spelled out: left to
// contraction the fp32 and the fh2 kernels would round differently and "fh2 output == split of the fp32 output" would not hold)
__device__ __forceinline__ f32x4 bilerp4(f32x4 v00, f32x4 v01, f32x4 v10, f32x4 v11, float lx0, float lx1, float ly0, float ly1) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float t0 = __fmaf_rn(v01[e], lx1, __fmul_rn(v00[e], lx0));
        const float t1 = __fmaf_rn(v11[e], lx1, __fmul_rn(v10[e], lx0));
        o[e] = __fmaf_rn(t1, ly1, __fmul_rn(t0, ly0));
    }
    return o;
}

// One axis of the map for output index o of 2 n: the two source indices and their weights.  Every operation is spelled out, the
// fused o * s - i0 of the second weight included, so that every kernel form below rounds the weights the same way.
struct UpAxis { int i0, i1; float l0, l1; };
__device__ __forceinline__ float up_scale(int n) { return (2 * n > 1) ? __fdiv_rn((float)(n - 1), (float)(2 * n - 1)) : 0.f; }
__device__ __forceinline__ UpAxis up_axis(float s, int o, int n) {
    const float fo = (float)o;
    int i0 = (int)__fmul_rn(s, fo);
    i0 = i0 < n - 1 ? i0 : n - 1;
    const int i1 = i0 < n - 1 ? i0 + 1 : i0;
    const float l1 = __fmaf_rn(s, fo, -(float)i0);
    return UpAxis{i0, i1, __fsub_rn(1.f, l1), l1};
}

// The output stage the two kernel forms below share.  o[] = the interpolated float4(s) of output pixel (oy, ox) of slot b, pixel
// number pix of the output, for the thread's channels, cq its first float4.  FMT 0: fp32, 1: bf3, 2: fh2, 3: fh2 combine -- combine_resid_fh2_kernel inside the
// producer of its per-slot residual: p2 = o, as FMT 0 computes it (bilerp4: the same rounding order), is neither written nor read
// back; c, r0 [U, Hc, Wc, C]; s [S, Hc, Wc, C]; y = sr2 its fh2 twin --, 4: the combine with signed sources (CombineSrc).
template <int FMT>
__device__ __forceinline__ void up2x_emit(const f32x4* o, float* __restrict__ y, const float* __restrict__ c, const float* __restrict__ r0,
                                          const int* __restrict__ map, float* __restrict__ s, const CombineSrc& hs, int b, int oy, int ox,
                                          long pix, int Hc, int Wc, int C4, int cq, float scale, float& amax) {
    if (FMT == 0) reinterpret_cast<f32x4*>(y)[pix * C4 + cq] = o[0];
    else if (FMT == 1) bf3_store4(reinterpret_cast<char*>(y) + pix * ((size_t)C4 * 24), cq * 4, o[0]);
    else {
        char* row = reinterpret_cast<char*>(y) + pix * ((size_t)C4 * 16);
        if (FMT == 2) fh2_emit8(row, cq * 4, o[0], o[1], scale, amax);
        else {
            const float *__restrict__ cs = c, *__restrict__ rs = r0;
            const long blk = combine_block<FMT == 4>(hs, map[b], cs, rs);
            const long src = ((blk * Hc + oy) * Wc + ox) * C4 + cq;
            f32x4 e[2];
#pragma unroll
            for (int q = 0; q < 2; q++)
                e[q] = combine_emit(reinterpret_cast<const f32x4*>(cs)[src + q], reinterpret_cast<const f32x4*>(rs)[src + q], o[q],
                                    reinterpret_cast<f32x4*>(s) + pix * C4 + cq + q, scale, amax);
            fh2_store8(row, cq * 4, e[0], e[1]);
        }
    }
}

// ---- first form (A3R_UP_FORM=v1): one output pixel per thread and step, four corners fetched per output.  The reference of the
// second form below.
// FMT as up2x_emit.  Grid: x over (output column, channel group) of one output row, y over (batch, output row):
// the row / batch decomposition is scalar work once per workgroup and a thread does ONE 32-bit division (the first version took
// three 64-bit divisions by runtime values per thread).  A thread produces 4 channels (fp32 / bf3) or 8 channels (fh2: the two
// planes' 16-byte units of one 8-k group = 32 contiguous bytes, and half the index arithmetic per element -- PMC showed the
// 4-channel fh2 form VALU-bound at 150 instructions per thread).
template <int FMT>
__global__ __launch_bounds__(256) void upsample2x_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ c,
                                                         const float* __restrict__ r0, const int* __restrict__ map, float* __restrict__ s,
                                                         int B, int H, int W, int C4, int Hc, int Wc, float scale,
                                                         unsigned* __restrict__ absmax, CombineSrc hs) {
    constexpr int Q = FMT >= 2 ? 2 : 1;                        // float4 per thread
    const float sh = up_scale(H), sw = up_scale(W);
    const f32x4* xv = reinterpret_cast<const f32x4*>(x);
    const unsigned CG = (unsigned)C4 / Q;                      // channel groups per pixel
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    const unsigned ox = idx / CG, cq = (idx - ox * CG) * Q;    // cq: first float4 of this thread
    const bool live = ox < (unsigned)Wc;                     // (no early return in the fh2 forms: the range statistics need every lane at the end)
    if (FMT < 2 && !live) return;
    const UpAxis ax = up_axis(sw, (int)ox, W);
    const int x0 = ax.i0, x1 = ax.i1;
    const float lx0 = ax.l0, lx1 = ax.l1;
    float amax = 0.f;
    for (int row = blockIdx.y; live && row < B * Hc; row += gridDim.y) {   // (batch, output row): uniform per workgroup
        const int b = row / Hc, oy = row - b * Hc;
        const UpAxis ay = up_axis(sh, oy, H);
        const int y0 = ay.i0, y1 = ay.i1;
        const float ly0 = ay.l0, ly1 = ay.l1;
        const long rb = (long)b * H;
        const f32x4* q0 = xv + (rb + y0) * W * C4 + cq;
        const f32x4* q1 = xv + (rb + y1) * W * C4 + cq;
        f32x4 o[Q];
#pragma unroll
        for (int q = 0; q < Q; q++)
            o[q] = bilerp4(q0[(long)x0 * C4 + q], q0[(long)x1 * C4 + q], q1[(long)x0 * C4 + q], q1[(long)x1 * C4 + q], lx0, lx1, ly0, ly1);
        up2x_emit<FMT>(o, y, c, r0, map, s, hs, b, oy, (int)ox, (long)row * Wc + ox, Hc, Wc, C4, (int)cq, scale, amax);
    }
    if (FMT >= 2) {
        __shared__ unsigned s_red[4];
        fh2_publish_block(absmax, amax, s_red);
    }
}

// ---- second form (default): a thread makes the 2 x 2 output pixels (2 kb - 1, 2 kb) x (2 jb - 1, 2 jb) of its channel group.  With
// align_corners=True these four share their source rows (kb - 1, kb) and columns (jb - 1, jb), so the four corners are fetched ONCE
// for four outputs: 2 sixteen-byte loads per 32-byte store where the first form issues 8, which is what bounds it (every input
// element requested 16 times: the texture-address path, not HBM).  Whether an output really has the corners of its block's first
// output is decided from ITS OWN up_axis, and one that has not (fp32 rounding of the source coordinate on a very large map)
// fetches its corners as the first form does: indices, weights and bilerp4 are the first form's for every output, bit for bit.
// The output beyond an edge of the window (-1, Hc, Wc) is skipped and lends its axis to its neighbour.
// FMT as up2x_emit, without the bf3 form: 0 makes 4 channels per thread, 2 to 4 make 8.
template <int FMT>
__global__ __launch_bounds__(256) void upsample2x_block_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ c,
                                                               const float* __restrict__ r0, const int* __restrict__ map,
                                                               float* __restrict__ s, int B, int H, int W, int C4, int Hc, int Wc,
                                                               float scale, unsigned* __restrict__ absmax, CombineSrc hs) {
    constexpr int Q = FMT == 0 ? 1 : 2;                        // float4 per thread
    const float sh = up_scale(H), sw = up_scale(W);
    const int NKB = Hc / 2 + 1, NJB = Wc / 2 + 1;              // blocks per map column / row
    const unsigned CG = (unsigned)C4 / Q;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    const unsigned jb = idx / CG;
    const int cq = (int)(idx - jb * CG) * Q;                   // first float4 of this thread
    const bool live = jb < (unsigned)NJB;                      // (no early return: the range statistics need every lane at the end)
    const int ox[2] = {2 * (int)jb - 1, 2 * (int)jb};
    const bool vx[2] = {ox[0] >= 0, ox[1] < Wc};
    const UpAxis ax[2] = {up_axis(sw, vx[0] ? ox[0] : ox[1], W), up_axis(sw, vx[1] ? ox[1] : ox[0], W)};
    const bool same_x = ax[1].i0 == ax[0].i0 && ax[1].i1 == ax[0].i1;
    float amax = 0.f;
    for (int rb = blockIdx.y; live && rb < B * NKB; rb += gridDim.y) {     // (batch, block row): uniform per workgroup
        const int b = rb / NKB, kb = rb - b * NKB;
        const int oy[2] = {2 * kb - 1, 2 * kb};
        const bool vy[2] = {oy[0] >= 0, oy[1] < Hc};
        const UpAxis ay[2] = {up_axis(sh, vy[0] ? oy[0] : oy[1], H), up_axis(sh, vy[1] ? oy[1] : oy[0], H)};
        const bool same = same_x && ay[1].i0 == ay[0].i0 && ay[1].i1 == ay[0].i1;
        const f32x4* img = reinterpret_cast<const f32x4*>(x) + (long)b * H * W * C4 + cq;
        auto corner = [&](int yi, int xi, int q) { return img[((long)yi * W + xi) * C4 + q]; };
        f32x4 v00[Q], v01[Q], v10[Q], v11[Q];                  // the corners of output (0, 0) of the block
#pragma unroll
        for (int q = 0; q < Q; q++) {
            v00[q] = corner(ay[0].i0, ax[0].i0, q);
            v01[q] = corner(ay[0].i0, ax[0].i1, q);
            v10[q] = corner(ay[0].i1, ax[0].i0, q);
            v11[q] = corner(ay[0].i1, ax[0].i1, q);
        }
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int t = 0; t < 2; t++) {
                if (!(vy[r] && vx[t])) continue;
                const UpAxis &Y = ay[r], &X = ax[t];
                f32x4 o[Q];
                if ((r == 0 && t == 0) || same) {
#pragma unroll
                    for (int q = 0; q < Q; q++) o[q] = bilerp4(v00[q], v01[q], v10[q], v11[q], X.l0, X.l1, Y.l0, Y.l1);
                } else {
#pragma unroll
                    for (int q = 0; q < Q; q++)
                        o[q] = bilerp4(corner(Y.i0, X.i0, q), corner(Y.i0, X.i1, q), corner(Y.i1, X.i0, q), corner(Y.i1, X.i1, q), X.l0, X.l1,
                                       Y.l0, Y.l1);
                }
                up2x_emit<FMT>(o, y, c, r0, map, s, hs, b, oy[r], ox[t], ((long)b * Hc + oy[r]) * Wc + ox[t], Hc, Wc, C4, cq, scale, amax);
            }
    }
    if (FMT != 0) {
        __shared__ unsigned s_red[4];
        fh2_publish_block(absmax, amax, s_red);
    }
}

// which form the fp32, fh2 and combine entry points launch: 2 (default) or 1 (A3R_UP_FORM=v1 / a3r_upsample2x_set_form)
static std::atomic<int> g_up_form{(getenv("A3R_UP_FORM") && !strcmp(getenv("A3R_UP_FORM"), "v1")) ? 1 : 2};

// ------------------------------------------------------------------------------------------- head final
// conv1x1 C -> 4 (+bias) then postprocess (postprocess.py:10-58). 32 lanes per pixel (C == 128: one float4 each).
__global__ __launch_bounds__(256) void head_final_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ pts,
                                                          float* __restrict__ conf, long P, int C) {
    const int lane = threadIdx.x & 63, sub = lane & 31;
    const long pix0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + (lane >> 5);
    const long stride = (long)gridDim.x * 8;
    const long iters = (P + stride - 1) / stride;      // uniform trip count: the shuffles need every lane
    const int nvec = C / 4;
    for (long it = 0; it < iters; it++) {
        const long pix = pix0 + it * stride;
        const bool ok = pix < P;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            const f32x4* xr = reinterpret_cast<const f32x4*>(x + pix * C);
            for (int j = sub; j < nvec; j += 32) {
                const f32x4 v = xr[j];
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    const f32x4 ww = reinterpret_cast<const f32x4*>(w + o * C)[j];
                    acc[o] += v.x * ww.x + v.y * ww.y + v.z * ww.z + v.w * ww.w;
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 4; o++) {
#pragma unroll
            for (int m = 16; m > 0; m >>= 1) acc[o] += __shfl_xor(acc[o], m);
            acc[o] += bias[o];
        }
        if (ok && sub == 0) {
            // reference order: xyz / d.clip(1e-8) * expm1(d)   (postprocess.py:37-46)
            const float d = sqrtf(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]);
            const float dd = fmaxf(d, 1e-8f), em = expm1f(d);
            pts[pix * 3 + 0] = acc[0] / dd * em;
            pts[pix * 3 + 1] = acc[1] / dd * em;
            pts[pix * 3 + 2] = acc[2] / dd * em;
            conf[pix] = 1.f + expf(acc[3]);
        }
    }
}

// C == 128 (the DPT head's last_dim): 8 lanes per pixel, a lane owns 16 consecutive channels = 64 contiguous bytes, so a wave reads
// 8 pixels = 4 KB contiguous per step (the 32-lanes-per-pixel form above has 1 KB per step in flight and re-loads its four weight
// vectors every pixel); the 4 x 16 weights of a lane stay in registers; three exchange steps finish the four dot products.
__global__ __launch_bounds__(256) void head_final128_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ pts,
                                                             float* __restrict__ conf, long P) {
    const int lane = threadIdx.x & 63, sub = lane & 7;
    f32x4 wr[4][4];
#pragma unroll
    for (int o = 0; o < 4; o++)
#pragma unroll
        for (int q = 0; q < 4; q++) wr[o][q] = reinterpret_cast<const f32x4*>(w + o * 128)[sub * 4 + q];
    const float b0 = bias[0], b1 = bias[1], b2 = bias[2], b3 = bias[3];
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    const long iters = (P + nwaves * 8 - 1) / (nwaves * 8);       // uniform trip count: the exchanges need every lane
    for (long it = 0; it < iters; it++) {
        const long pix = (it * nwaves + wave) * 8 + (lane >> 3);
        const bool ok = pix < P;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            const f32x4* xr = reinterpret_cast<const f32x4*>(x + pix * 128) + sub * 4;
            f32x4 v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = xr[q];
#pragma unroll
            for (int o = 0; o < 4; o++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[o] += v[q].x * wr[o][q].x + v[q].y * wr[o][q].y + v[q].z * wr[o][q].z + v[q].w * wr[o][q].w;
        }
#pragma unroll
        for (int o = 0; o < 4; o++) {
            acc[o] += __shfl_xor(acc[o], 1);
            acc[o] += __shfl_xor(acc[o], 2);
            acc[o] += __shfl_xor(acc[o], 4);
        }
        if (ok && sub == 0) {
            const float a0 = acc[0] + b0, a1 = acc[1] + b1, a2 = acc[2] + b2, a3 = acc[3] + b3;
            // reference order: xyz / d.clip(1e-8) * expm1(d)   (postprocess.py:37-46)
            const float d = sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
            const float dd = fmaxf(d, 1e-8f), em = expm1f(d);
            pts[pix * 3 + 0] = a0 / dd * em;
            pts[pix * 3 + 1] = a1 / dd * em;
            pts[pix * 3 + 2] = a2 / dd * em;
            conf[pix] = 1.f + expf(a3);
        }
    }
}

// ------------------------------------------------------------------------------------------- weight repacking
// [Cout, Cin, 3, 3] -> [Cout, 3, 3, Cin]
__global__ void pack_conv3x3_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin) {
    const long total = (long)Cout * Cin * 9;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Cin);
        const int tap = (int)((i / Cin) % 9);
        const int co = (int)(i / ((long)Cin * 9));
        wp[i] = w[((long)co * Cin + ci) * 9 + tap];
    }
}
// [Cin, Cout, s, s] -> [(dy*s+dx)*Cout + co][Cin]
__global__ void pack_convT_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int s) {
    const long total = (long)Cin * Cout * s * s;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Cin);
        const long n = i / Cin;
        const int co = (int)(n % Cout), tap = (int)(n / Cout);
        wp[i] = w[((long)ci * Cout + co) * (s * s) + tap];
    }
}

static inline int grid_for(long total, int block = 256) {
    long g = (total + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace a3r
using namespace a3r;

// the entry checks several producers share, with the texts their entries have always printed
static int check_scale(const char* who, float scale) {
    A3R_CHECK_ARG(scale > 0.f && std::isfinite(scale), "%s: scale must be positive and finite", who);
    return A3R_OK;
}
// c_multiple: 4 (fp32 output) or 8 (the packed forms, whose text names it)
static int check_up2x_shape(const char* who, int B, int H, int W, int C, int c_multiple, int Hc, int Wc) {
    A3R_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % c_multiple == 0,
                  c_multiple == 8 ? "%s: bad shape (C must be a multiple of 8)" : "%s: bad shape", who);
    A3R_CHECK_ARG(Hc > 0 && Hc <= 2 * H && Wc > 0 && Wc <= 2 * W, "%s: crop window larger than the 2x map", who);
    return A3R_OK;
}

template <bool BF3>
static int launch_layernorm(const float* x, const float* w, const float* b, float* y, int M, int D, float eps, void* stream, int pair = 0) {
    hipStream_t st = as_stream(stream);
    ProfScope prof(PK_LAYERNORM, (BF3 ? 10.0 : 8.0) * M * D, st);
    dim3 grid((M + 3) / 4), block(256);
    if (BF3 && pair && (D == 1024 || D == 768 || D == 256)) {
        const dim3 g2((M + 7) / 8);
        char* y3 = reinterpret_cast<char*>(y);
        if (D == 1024) hipLaunchKernelGGL(layernorm_pair_kernel<4>, g2, block, 0, st, x, w, b, y3, M, D, eps);
        else if (D == 768) hipLaunchKernelGGL(layernorm_pair_kernel<3>, g2, block, 0, st, x, w, b, y3, M, D, eps);
        else hipLaunchKernelGGL(layernorm_pair_kernel<1>, g2, block, 0, st, x, w, b, y3, M, D, eps);
        A3R_LAUNCH_CHECK();
        return A3R_OK;
    }
    if (D == 1024) hipLaunchKernelGGL((layernorm_kernel<4, BF3>), grid, block, 0, st, x, w, b, y, M, D, eps, pair);
    else if (D == 768) hipLaunchKernelGGL((layernorm_kernel<3, BF3>), grid, block, 0, st, x, w, b, y, M, D, eps, pair);
    else if (D == 256) hipLaunchKernelGGL((layernorm_kernel<1, BF3>), grid, block, 0, st, x, w, b, y, M, D, eps, pair);
    else hipLaunchKernelGGL(layernorm_generic_kernel<BF3 ? 1 : 0>, grid, block, 0, st, x, w, b, y, M, D, eps, pair, 1.f, nullptr);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_layernorm(const float* x, const float* w, const float* b, float* y, int M, int D, float eps,
                             void* stream) {
    A3R_CHECK_ARG(x && w && b && y, "a3r_layernorm: null pointer");
    A3R_CHECK_ARG(M > 0 && D > 0 && D % 4 == 0, "a3r_layernorm: bad shape M=%d D=%d", M, D);
    return launch_layernorm<false>(x, w, b, y, M, D, eps, stream);
}

template <int VPL>   // the register kernel for rows of up to 512 VPL, with or without the range statistics
static void launch_ln_fh2(bool stats, dim3 grid, hipStream_t st, const float* x, const float* w, const float* b, char* y, int M, int D,
                          float eps, float scale, unsigned* absmax) {
    if (stats) hipLaunchKernelGGL((layernorm_fh2_kernel<VPL, true>), grid, dim3(256), 0, st, x, w, b, y, M, D, eps, scale, absmax);
    else hipLaunchKernelGGL((layernorm_fh2_kernel<VPL, false>), grid, dim3(256), 0, st, x, w, b, y, M, D, eps, scale, absmax);
}

extern "C" int a3r_layernorm_fh2(const float* x, const float* w, const float* b, void* y2, int M, int D, float eps, float scale,
                                 unsigned* absmax, void* stream) {
    A3R_CHECK_ARG(x && w && b && y2, "a3r_layernorm_fh2: null pointer");
    if (int rc = check_scale("a3r_layernorm_fh2", scale)) return rc;
    A3R_CHECK_ARG(M > 0 && D > 0 && D % 32 == 0, "a3r_layernorm_fh2: bad shape M=%d D=%d (D must be a multiple of 32)", M, D);
    A3R_CHECK_ARG(aligned_to(y2, 16), "a3r_layernorm_fh2: y2 must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    ProfScope prof(PK_LAYERNORM, 8.0 * M * D, st);
    const int nblk = (M + 3) / 4;
    // with statistics: a persistent rows loop (16 workgroups per CU, one atomic each); without: one row per wave
    const dim3 grid(absmax && nblk > 4096 ? 4096 : nblk);
    char* y = static_cast<char*>(y2);
    // rows up to 1536 wide stay in registers (one, two or three 8-k groups per lane; D = 768 uses two with the upper lanes idle in
    // the second: 2.7 -> 4.5+ TB/s against the three-pass generic kernel it used before)
    const bool aligned = all_aligned16(x, w, b);
    if (aligned && D <= 512) launch_ln_fh2<1>(absmax, grid, st, x, w, b, y, M, D, eps, scale, absmax);
    else if (aligned && D <= 1024) launch_ln_fh2<2>(absmax, grid, st, x, w, b, y, M, D, eps, scale, absmax);
    else if (aligned && D <= 1536) launch_ln_fh2<3>(absmax, grid, st, x, w, b, y, M, D, eps, scale, absmax);
    else hipLaunchKernelGGL(layernorm_generic_kernel<2>, grid, dim3(256), 0, st, x, w, b, y2, M, D, eps, 0, scale, absmax);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_layernorm_bf3(const float* x, const float* w, const float* b, void* y3, int M, int D, float eps, int pair,
                                 void* stream) {
    A3R_CHECK_ARG(x && w && b && y3, "a3r_layernorm_bf3: null pointer");
    A3R_CHECK_ARG(M > 0 && D > 0 && D % 8 == 0, "a3r_layernorm_bf3: bad shape M=%d D=%d (D must be a multiple of 8)", M, D);
    A3R_CHECK_ARG(!pair || D % 32 == 0, "a3r_layernorm_bf3: the row-pair layout needs D (%d) to be a multiple of 32", D);
    A3R_CHECK_ARG(aligned_to(y3, 16), "a3r_layernorm_bf3: y3 must be 16-byte aligned");
    return launch_layernorm<true>(x, w, b, static_cast<float*>(y3), M, D, eps, stream, pair ? 1 : 0);
}

extern "C" int a3r_rope2d(float* tokens, const int64_t* positions, int B, int N, int H, int D, float base, float fwd,
                          void* stream) {
    // argument checks mirror curope.cpp:54-59 / kernels.cu:91-94
    A3R_CHECK_ARG(tokens && positions, "a3r_rope2d: null pointer");
    A3R_CHECK_ARG(B > 0 && N > 0 && H > 0, "a3r_rope2d: tokens must have 4 dimensions with positive sizes");
    A3R_CHECK_ARG(D > 0 && D % 4 == 0, "a3r_rope2d: token dim must be multiple of 4 (got %d)", D);
    const long total = (long)B * N * H * (D / 2);
    hipLaunchKernelGGL(rope2d_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), tokens, positions, B, N, H, D,
                       base, fwd);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_rope_table_host(float* cos_host, float* sin_host, int max_pos, float base) {
    A3R_CHECK_ARG(cos_host && sin_host && max_pos > 0, "a3r_rope_table_host: bad argument");
    // RoPE2D.get_cos_sin (pos_embed.py:118-128) with D = 32: inv_freq = 1/(base**(arange(0,32,2)/32)), fp32 steps
    for (int q = 0; q < 16; q++) {
        const float expo = (float)(2 * q) / 32.0f;
        const float inv_freq = 1.0f / powf(base, expo);
        for (int p = 0; p < max_pos; p++) {
            const float fr = (float)p * inv_freq;
            cos_host[p * 16 + q] = cosf(fr);
            sin_host[p * 16 + q] = sinf(fr);
        }
    }
    return A3R_OK;
}

extern "C" int a3r_patchify(const float* img, float* cols, int B, int C, int H, int W, long sb, long sc, long sy, long sx,
                            void* stream) {
    A3R_CHECK_ARG(img && cols, "a3r_patchify: null pointer");
    // patch_embed.py:22-23
    A3R_CHECK_ARG(H > 0 && H % 16 == 0, "Input image height (%d) is not a multiple of patch size (16).", H);
    A3R_CHECK_ARG(W > 0 && W % 16 == 0, "Input image width (%d) is not a multiple of patch size (16).", W);
    const long total = (long)B * (H / 16) * (W / 16) * C * 256;
    ProfScope prof(PK_ELEMENTWISE, 8.0 * total, as_stream(stream));
    hipLaunchKernelGGL(patchify_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), img, cols, B, C, H, W, sb, sc,
                       sy, sx);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

int a3r::patchify_indexed(const float* img_a, const float* img_b, const int32_t* uniq, int U, int B, float* cols, int C, int H, int W,
                          long sb, long sc, long sy, long sx, void* stream) {
    A3R_CHECK_ARG(img_a && img_b && uniq && cols, "patchify_indexed: null pointer");
    A3R_CHECK_ARG(H > 0 && H % 16 == 0 && W > 0 && W % 16 == 0 && B > 0 && U > 0 && U <= 2 * B, "patchify_indexed: bad shape");
    const long total = (long)U * (H / 16) * (W / 16) * C * 256;
    ProfScope prof(PK_ELEMENTWISE, 8.0 * total, as_stream(stream));
    hipLaunchKernelGGL(patchify_indexed_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), img_a, img_b, uniq, cols, U, B, C,
                       H, W, sb, sc, sy, sx);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

int a3r::gather_rows(const float* src, float* dst, const int32_t* map, int S, int N, int C, void* stream) {
    A3R_CHECK_ARG(src && dst && map, "gather_rows: null pointer");
    A3R_CHECK_ARG(S > 0 && N > 0 && C > 0 && C % 4 == 0, "gather_rows: bad shape");
    A3R_CHECK_ARG(all_aligned16(src, dst), "gather_rows: buffers must be 16-byte aligned");
    const long NC4 = (long)N * (C / 4), total = (long)S * NC4;
    ProfScope prof(PK_ELEMENTWISE, 32.0 * total, as_stream(stream));
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), reinterpret_cast<const f32x4*>(src),
                       reinterpret_cast<f32x4*>(dst), map, S, NC4);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_gather_add_rows(const float* a, const int32_t* map_a, const float* b, const int32_t* map_b, float* dst, int S, int N,
                                   int C, void* stream) {
    A3R_CHECK_ARG(a && map_a && dst && (!b || map_b), "a3r_gather_add_rows: null pointer");
    A3R_CHECK_ARG(S > 0 && N > 0 && C > 0 && C % 4 == 0, "a3r_gather_add_rows: bad shape");
    A3R_CHECK_ARG(all_aligned16(a, b, dst), "a3r_gather_add_rows: buffers must be 16-byte aligned");
    const long NC4 = (long)N * (C / 4), total = (long)S * NC4;
    ProfScope prof(PK_ELEMENTWISE, 48.0 * total, as_stream(stream));
    hipLaunchKernelGGL(gather_add_rows_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), reinterpret_cast<const f32x4*>(a),
                       map_a, reinterpret_cast<const f32x4*>(b), map_b, reinterpret_cast<f32x4*>(dst), S, NC4);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_gather_add_rows_src(const float* store, long stride, const float* fresh, const int32_t* src, const float* b,
                                       const int32_t* map_b, float* dst, int S, int N, int C, void* stream) {
    A3R_CHECK_ARG(store && fresh && src && dst && (!b || map_b), "a3r_gather_add_rows_src: null pointer");
    A3R_CHECK_ARG(S > 0 && N > 0 && C > 0 && C % 4 == 0 && stride >= (long)N * C && stride % 4 == 0, "a3r_gather_add_rows_src: bad shape");
    A3R_CHECK_ARG(all_aligned16(store, fresh, b, dst), "a3r_gather_add_rows_src: buffers must be 16-byte aligned");
    const long NC4 = (long)N * (C / 4), total = (long)S * NC4;
    ProfScope prof(PK_ELEMENTWISE, 48.0 * total, as_stream(stream));
    hipLaunchKernelGGL(gather_add_rows_src_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const f32x4*>(store), stride / 4, reinterpret_cast<const f32x4*>(fresh), src,
                       reinterpret_cast<const f32x4*>(b), map_b, reinterpret_cast<f32x4*>(dst), S, NC4);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

// one body for the two entry points: hs null = c / r0 hold the blocks map names; else map is the signed source list
static int combine_resid_launch(const char* who, const float* c, const float* r0, const CombineSrc* hs, const float* p2, const int32_t* map,
                                float* s, void* sr2, int S, long P, int C, float scale, unsigned* absmax, void* stream) {
    A3R_CHECK_ARG(p2 && map && s && sr2 && (hs ? (c && r0) || (hs->c && hs->r0) : c && r0), "%s: null pointer", who);
    A3R_CHECK_ARG(S > 0 && P > 0 && C > 0 && C % 8 == 0 && (long)S * P < (1L << 31), "%s: bad shape (C must be a multiple of 8)", who);
    A3R_CHECK_ARG(!hs || (hs->stride >= P * C && hs->stride % 4 == 0 && !hs->c == !hs->r0 && !c == !r0), "%s: bad storage stride or pointers", who);
    if (int rc = check_scale(who, scale)) return rc;
    A3R_CHECK_ARG(all_aligned16(c, r0, p2, s, sr2, hs ? hs->c : nullptr, hs ? hs->r0 : nullptr), "%s: buffers must be 16-byte aligned", who);
    const long rows = (long)S * P, total = rows * (C / 8);
    ProfScope prof(PK_ELEMENTWISE, 5.0 * 32 * total, as_stream(stream));
    const long blocks = (total + 255) / 256;
    // persistent grid (8 workgroups per CU), as the split pass
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));
    if (hs)
        hipLaunchKernelGGL(combine_resid_fh2_kernel<true>, grid, dim3(256), 0, as_stream(stream), c, r0, p2, map, s, static_cast<char*>(sr2),
                           rows, P, C / 8, scale, absmax, *hs);
    else
        hipLaunchKernelGGL(combine_resid_fh2_kernel<false>, grid, dim3(256), 0, as_stream(stream), c, r0, p2, map, s, static_cast<char*>(sr2),
                           rows, P, C / 8, scale, absmax, CombineSrc{});
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_combine_resid_fh2(const float* c, const float* r0, const float* p2, const int32_t* map, float* s, void* sr2, int S,
                                     long P, int C, float scale, unsigned* absmax, void* stream) {
    return combine_resid_launch("a3r_combine_resid_fh2", c, r0, nullptr, p2, map, s, sr2, S, P, C, scale, absmax, stream);
}

extern "C" int a3r_combine_resid_fh2_src(const float* c, const float* r0, const float* store_c, const float* store_r0, long stride,
                                         const int32_t* src, const float* p2, float* s, void* sr2, int S, long P, int C, float scale,
                                         unsigned* absmax, void* stream) {
    const CombineSrc hs = {store_c, store_r0, stride};
    return combine_resid_launch("a3r_combine_resid_fh2_src", c, r0, &hs, p2, src, s, sr2, S, P, C, scale, absmax, stream);
}

// The first form's grid.  groups: threads per output pixel.  rows: output rows a workgroup loops over.  The fh2 forms take ~8 and
// publish ONE statistics atomic per workgroup (a long per-thread loop of dependent row loads is latency-bound: 63 rows per
// workgroup cost +15 % on the full-resolution map; one row per workgroup is half a million atomics).
static inline dim3 upsample_grid(int B, int Hc, int Wc, int groups, unsigned rows = 1) {
    const long all = (long)B * Hc;
    const unsigned y = (unsigned)(all < 65535 ? all : 65535);
    return dim3((unsigned)(((long)Wc * groups + 255) / 256), (y + rows - 1) / rows);
}

// the second form's grid: x over (block column, channel group), y over (batch, block row); a workgroup of the fh2 forms loops over
// ~`rows` block rows and publishes one statistics atomic.  Measured on the headline's maps (tools/bench_up2x.py, one session, rows
// 1 / 2 / 3 / 4 / 8 / 16): fh2 [42, 192, 256, 128] 1644 / 1153 / 1179 / 1216 / 1291 / 1339 us, fh2 [42, 96, 128, 256] 829 / 616 / 634 / 639 /
// 662 / 685 us -- one block row per workgroup is 140 000 atomics on one word, many rows are a serial chain of load, compute, store
// per wave at 5 waves per SIMD; combine [42 <- 15, 48, 64, 256] 430 / 431 / 413 / 412 / 415 / 464 us.
static inline dim3 upsample_block_grid(int B, int Hc, int Wc, int groups, unsigned rows) {
    return upsample_grid(B, Hc / 2 + 1, Wc / 2 + 1, groups, rows);
}

extern "C" int a3r_upsample2x_set_form(int form) {
    A3R_CHECK_ARG(form == 1 || form == 2, "a3r_upsample2x_set_form: form must be 1 or 2");
    return g_up_form.exchange(form);
}

// one launch for the 2x entries: output format FMT (up2x_emit) in the form the process runs, each on its grid
template <int FMT>
static void launch_up2x(dim3 grid_v1, dim3 grid_v2, void* stream, const float* x, void* y, const float* c, const float* r0, const int32_t* map,
                        float* s, int B, int H, int W, int C, int Hc, int Wc, float scale, unsigned* absmax, const CombineSrc& hs) {
    if (g_up_form.load() == 1)
        hipLaunchKernelGGL(upsample2x_kernel<FMT>, grid_v1, dim3(256), 0, as_stream(stream), x, static_cast<float*>(y), c, r0, map, s, B, H, W,
                           C / 4, Hc, Wc, scale, absmax, hs);
    else
        hipLaunchKernelGGL(upsample2x_block_kernel<FMT>, grid_v2, dim3(256), 0, as_stream(stream), x, static_cast<float*>(y), c, r0, map, s, B,
                           H, W, C / 4, Hc, Wc, scale, absmax, hs);
}

extern "C" int a3r_upsample2x(const float* x, float* y, int B, int H, int W, int C, int Hc, int Wc, void* stream) {
    A3R_CHECK_ARG(x && y, "a3r_upsample2x: null pointer");
    if (int rc = check_up2x_shape("a3r_upsample2x", B, H, W, C, 4, Hc, Wc)) return rc;
    const long total = (long)B * Hc * Wc * (C / 4);
    ProfScope prof(PK_ELEMENTWISE, 16.0 * total + 4.0 * B * H * W * C, as_stream(stream));
    launch_up2x<0>(upsample_grid(B, Hc, Wc, C / 4), upsample_block_grid(B, Hc, Wc, C / 4, 1), stream, x, y, nullptr, nullptr, nullptr, nullptr,
                   B, H, W, C, Hc, Wc, 1.f, nullptr, CombineSrc{});
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_upsample2x_bf3(const float* x, void* y3, int B, int H, int W, int C, int Hc, int Wc, void* stream) {
    A3R_CHECK_ARG(x && y3, "a3r_upsample2x_bf3: null pointer");
    if (int rc = check_up2x_shape("a3r_upsample2x_bf3", B, H, W, C, 8, Hc, Wc)) return rc;
    const long total = (long)B * Hc * Wc * (C / 4);
    ProfScope prof(PK_ELEMENTWISE, 24.0 * total + 4.0 * B * H * W * C, as_stream(stream));
    hipLaunchKernelGGL(upsample2x_kernel<1>, upsample_grid(B, Hc, Wc, C / 4), dim3(256), 0, as_stream(stream), x, static_cast<float*>(y3),
                       nullptr, nullptr, nullptr, nullptr, B, H, W, C / 4, Hc, Wc, 1.f, nullptr, CombineSrc{});
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_upsample2x_fh2(const float* x, void* y2, int B, int H, int W, int C, int Hc, int Wc, float scale, unsigned* absmax,
                                  void* stream) {
    A3R_CHECK_ARG(x && y2, "a3r_upsample2x_fh2: null pointer");
    if (int rc = check_scale("a3r_upsample2x_fh2", scale)) return rc;
    if (int rc = check_up2x_shape("a3r_upsample2x_fh2", B, H, W, C, 8, Hc, Wc)) return rc;
    const long total = (long)B * Hc * Wc * (C / 4);
    ProfScope prof(PK_ELEMENTWISE, 16.0 * total + 4.0 * B * H * W * C, as_stream(stream));
    launch_up2x<2>(upsample_grid(B, Hc, Wc, C / 8, 8), upsample_block_grid(B, Hc, Wc, C / 8, 2), stream, x, y2, nullptr, nullptr, nullptr,
                   nullptr, B, H, W, C, Hc, Wc, scale, absmax, CombineSrc{});
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

// one body for the two entry points (combine_resid_launch)
static int upsample2x_combine_launch(const char* who, const float* x, const float* c, const float* r0, const CombineSrc* hs,
                                     const int32_t* map, float* s, void* sr2, int B, int H, int W, int C, int Hc, int Wc, float scale,
                                     unsigned* absmax, void* stream) {
    A3R_CHECK_ARG(x && map && s && sr2 && (hs ? (c && r0) || (hs->c && hs->r0) : c && r0), "%s: null pointer", who);
    if (int rc = check_scale(who, scale)) return rc;
    if (int rc = check_up2x_shape(who, B, H, W, C, 8, Hc, Wc)) return rc;
    A3R_CHECK_ARG(!hs || (hs->stride >= (long)Hc * Wc * C && hs->stride % 4 == 0 && !hs->c == !hs->r0 && !c == !r0),
                  "%s: bad storage stride or pointers", who);
    A3R_CHECK_ARG(all_aligned16(x, c, r0, s, sr2, hs ? hs->c : nullptr, hs ? hs->r0 : nullptr), "%s: buffers must be 16-byte aligned", who);
    const long total = (long)B * Hc * Wc * (C / 4);
    ProfScope prof(PK_ELEMENTWISE, 40.0 * total + 4.0 * B * H * W * C, as_stream(stream));
    const dim3 grid_v1 = upsample_grid(B, Hc, Wc, C / 8, 8), grid_v2 = upsample_block_grid(B, Hc, Wc, C / 8, 4);
    if (hs) launch_up2x<4>(grid_v1, grid_v2, stream, x, sr2, c, r0, map, s, B, H, W, C, Hc, Wc, scale, absmax, *hs);
    else launch_up2x<3>(grid_v1, grid_v2, stream, x, sr2, c, r0, map, s, B, H, W, C, Hc, Wc, scale, absmax, CombineSrc{});
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

// (the text of this entry's checks has never carried the a3r_ prefix)
extern "C" int a3r_upsample2x_combine_fh2(const float* x, const float* c, const float* r0, const int32_t* map, float* s, void* sr2, int S,
                                          int H, int W, int C, int Hc, int Wc, float scale, unsigned* absmax, void* stream) {
    return upsample2x_combine_launch("upsample2x_combine_fh2", x, c, r0, nullptr, map, s, sr2, S, H, W, C, Hc, Wc, scale, absmax, stream);
}

extern "C" int a3r_upsample2x_combine_fh2_src(const float* x, const float* c, const float* r0, const float* store_c, const float* store_r0,
                                              long stride, const int32_t* src, float* s, void* sr2, int S, int H, int W, int C, int Hc,
                                              int Wc, float scale, unsigned* absmax, void* stream) {
    const CombineSrc hs = {store_c, store_r0, stride};
    return upsample2x_combine_launch("a3r_upsample2x_combine_fh2_src", x, c, r0, &hs, src, s, sr2, S, H, W, C, Hc, Wc, scale, absmax, stream);
}

extern "C" int a3r_head_final(const float* x, const float* w, const float* b, float* pts3d, float* conf, long P, int C,
                              void* stream) {
    A3R_CHECK_ARG(x && w && b && pts3d && conf, "a3r_head_final: null pointer");
    A3R_CHECK_ARG(P > 0 && C > 0 && C % 4 == 0, "a3r_head_final: bad shape");
    long blocks = (P + 7) / 8;
    if (blocks > 16384) blocks = 16384;
    ProfScope prof(PK_ELEMENTWISE, 4.0 * P * (C + 4), as_stream(stream));
    if (C == 128 && all_aligned16(x, w)) {
        long nb = (P + 31) / 32;                                   // a block of four waves takes 32 pixels per step
        if (nb > 8192) nb = 8192;
        hipLaunchKernelGGL(head_final128_kernel, dim3((int)nb), dim3(256), 0, as_stream(stream), x, w, b, pts3d, conf, P);
    } else {
        hipLaunchKernelGGL(head_final_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), x, w, b, pts3d, conf, P, C);
    }
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_pack_conv3x3(const float* w, float* wp, int Cout, int Cin, void* stream) {
    A3R_CHECK_ARG(w && wp && Cout > 0 && Cin > 0, "a3r_pack_conv3x3: bad argument");
    hipLaunchKernelGGL(pack_conv3x3_kernel, dim3(grid_for((long)Cout * Cin * 9)), dim3(256), 0, as_stream(stream), w, wp, Cout, Cin);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_pack_convT(const float* w, float* wp, int Cin, int Cout, int s, void* stream) {
    A3R_CHECK_ARG(w && wp && Cout > 0 && Cin > 0 && s > 0, "a3r_pack_convT: bad argument");
    hipLaunchKernelGGL(pack_convT_kernel, dim3(grid_for((long)Cin * Cout * s * s)), dim3(256), 0, as_stream(stream), w, wp, Cin, Cout, s);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
