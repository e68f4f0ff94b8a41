// Input preprocessing of the pair forward for gfx950 (dust3r/utils/image_pose.py of the package: pixel_to_pointcloud, normalize_pointcloud,
// cv2_resize, crop_center, ImgNorm): the mono-depth prior [Hs, Ws] becomes the normalised, resized and cropped point map [Hc, Wc, 3], with
// the SAME NUMBERS as the host path.  The arithmetic contract, every operation rounded on its own, nothing fused:
//
//   un-project    x = f32(((px - Ws/2) * d) / f),  y = f32(((py - Hs/2) * d) / f),  z = d          float64, one rounding to float32
//   min / max     per channel over the float32 values; a NaN anywhere makes both NaN (np.min / np.max)
//   normalise     n = (v - min) / (max - min)                                                     float32, IEEE division
//   horizontal    t[y, j, c] = ((0 + n[y, ix[j,0], c] * wx[j,0]) + n[y, ix[j,1], c] * wx[j,1]) + ...  float64, kept as float64
//   vertical      out[i, j, c] = f32(((0 + t[iy[i,0], j, c] * wy[i,0]) + ...))                       float64, one rounding to float32
//
// ix / wx / iy / wy are the clipped source indices and weights of the host's resize (8-tap Lanczos-4 or 4-tap cubic), built on the host
// by the function the host path itself uses.  Only the crop window is computed: columns x0 .. x0 + Wc of the horizontal pass, rows
// y0 .. y0 + Hc of the vertical one, and of the source rows only those the window's vertical taps read.
//
// Streaming kernels, no atomics, fixed-order reductions (min / max are exact in any order, the NaN flag is an OR):
//   prep_minmax_kernel   grid (chunks): a workgroup owns PCHUNK = 1024 consecutive depth pixels, a thread 4 of them (one 16-byte load
//                        when Hs * Ws % 4 == 0); writes one (min, max) x 3 + NaN flags partial per chunk, nothing else
//   prep_fold_kernel     one workgroup folds the partials into (min, max - min) x 3
//   prep_hpass_kernel    grid (Wc / 256, rows / PROWS): a thread owns one output column, keeps its index and weight row in registers
//                        and walks PROWS source rows; from the depth map it un-projects and normalises each tap as it loads it (the
//                        full-resolution three-channel map never exists), from a [Hs, Ws, 3] source it loads the three channels
//   prep_vpass_kernel    grid (Wc * 3 / 1024, Hc): a workgroup owns one output row (its index and weight row are wave-uniform: scalar
//                        registers), a thread 4 consecutive floats of it (16-byte loads and stores when Wc * 3 % 4 == 0)
//   prep_image_kernel    uint8 [H, W, 3] -> img [3, H, W] = (u / 255 - 0.5) / 0.5 and mask [H, W] = ((c0/255 + c1/255) + c2/255) > 0.01
#include "common.h"

#include <cmath>

// Nothing in this file may be contracted into an FMA: the host rounds every product and every sum.  The pragma covers the operators
// written here; __dmul_rn / __dadd_rn of the HIP headers are plain operators compiled under the build's default mode, which is why
// the Makefile also gives this file -ffp-contract=off (without it the vertical pass is 32 v_fma_f64 and no v_add_f64).
#pragma clang fp contract(off)

namespace a3r {

constexpr int PPX = 4;                  // consecutive elements per thread (min / max, vertical pass, image)
constexpr int PTPB = 256;
constexpr int PCHUNK = PPX * PTPB;
constexpr int PROWS = 4;                // source rows per thread of the horizontal pass

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

static int prep_nchunks(long long P) { return (int)((P + PCHUNK - 1) / PCHUNK); }
static size_t prep_inter_bytes(int Hs, int Wc) { return align_up((size_t)Hs * Wc * 3 * sizeof(double), 256); }
static size_t prep_partial_bytes(int Hs, int Ws) { return align_up((size_t)prep_nchunks((long long)Hs * Ws) * 8 * sizeof(float), 256); }
static size_t prep_stats_bytes() { return 256; }

struct PrepView {
    int Hs, Ws, P, nch;
    int y0, x0, Hc, Wc;
    int ylo, yhi;                       // source rows the vertical taps of the window read: [ylo, yhi]
    double focal, cx, cy;               // cx = Ws / 2, cy = Hs / 2 (exact)
    const int* idx_x;                   // [Wr, taps]
    const double* w_x;
    const int* idx_y;                   // [Hr, taps]
    const double* w_y;
    double* inter;                      // [Hs, Wc, 3]
    float* partial;                     // [nch, 8]: min0, max0, min1, max1, min2, max2, NaN flags (bit c), 0
    float* stats;                       // [8]: min0, max0 - min0, min1, max1 - min1, min2, max2 - min2, 0, 0
};

// the three float32 coordinates of one depth pixel (pixel_to_pointcloud before the normalisation)
__device__ __forceinline__ void prep_unproject(float d, double fx, double fy, double focal, float& x, float& y) {
    const double dd = (double)d;
    x = __double2float_rn(__ddiv_rn(__dmul_rn(fx, dd), focal));
    y = __double2float_rn(__ddiv_rn(__dmul_rn(fy, dd), focal));
}

// grid (nch)
template <bool VEC>
__global__ __launch_bounds__(PTPB) void prep_minmax_kernel(PrepView v, const float* __restrict__ depth) {
    __shared__ float sh[PTPB / 64][6];
    __shared__ int sh_nan[PTPB / 64];
    const int tid = threadIdx.x, p0 = blockIdx.x * PCHUNK + tid * PPX;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int has_nan = 0;
    if (p0 < v.P) {
        float d[PPX];
        if (VEC) {                      // P % 4 == 0 and p0 % 4 == 0: the four pixels are inside P together
            const f32x4 q = *reinterpret_cast<const f32x4*>(depth + p0);
            d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
        } else {
#pragma unroll
            for (int i = 0; i < PPX; i++) d[i] = p0 + i < v.P ? depth[p0 + i] : 0.f;
        }
        int y = p0 / v.Ws, x = p0 - y * v.Ws;
#pragma unroll
        for (int i = 0; i < PPX; i++) {
            float c[3];
            prep_unproject(d[i], (double)x - v.cx, (double)y - v.cy, v.focal, c[0], c[1]);
            c[2] = d[i];
            if (p0 + i < v.P) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    has_nan |= (c[k] != c[k] ? 1 : 0) << k;
                    mn[k] = fminf(mn[k], c[k]);
                    mx[k] = fmaxf(mx[k], c[k]);
                }
            }
            if (++x == v.Ws) { x = 0; y++; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o));
        }
        has_nan |= __shfl_xor(has_nan, o);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) { sh[tid >> 6][2 * k] = mn[k]; sh[tid >> 6][2 * k + 1] = mx[k]; }
        sh_nan[tid >> 6] = has_nan;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < PTPB / 64; w++) {
#pragma unroll
            for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], sh[w][2 * k]); mx[k] = fmaxf(mx[k], sh[w][2 * k + 1]); }
            has_nan |= sh_nan[w];
        }
        f32x4* o = reinterpret_cast<f32x4*>(v.partial + (size_t)blockIdx.x * 8);
        o[0] = f32x4{mn[0], mx[0], mn[1], mx[1]};
        o[1] = f32x4{mn[2], mx[2], (float)has_nan, 0.f};
    }
}

// one workgroup
__global__ __launch_bounds__(PTPB) void prep_fold_kernel(PrepView v) {
    __shared__ float sh[PTPB / 64][6];
    __shared__ int sh_nan[PTPB / 64];
    const int tid = threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int has_nan = 0;
    for (int c = tid; c < v.nch; c += PTPB) {
        const f32x4* q = reinterpret_cast<const f32x4*>(v.partial + (size_t)c * 8);
        const f32x4 a = q[0], b = q[1];
        mn[0] = fminf(mn[0], a.x); mx[0] = fmaxf(mx[0], a.y);
        mn[1] = fminf(mn[1], a.z); mx[1] = fmaxf(mx[1], a.w);
        mn[2] = fminf(mn[2], b.x); mx[2] = fmaxf(mx[2], b.y);
        has_nan |= (int)b.z;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o));
        }
        has_nan |= __shfl_xor(has_nan, o);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) { sh[tid >> 6][2 * k] = mn[k]; sh[tid >> 6][2 * k + 1] = mx[k]; }
        sh_nan[tid >> 6] = has_nan;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < PTPB / 64; w++) {
#pragma unroll
            for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], sh[w][2 * k]); mx[k] = fmaxf(mx[k], sh[w][2 * k + 1]); }
            has_nan |= sh_nan[w];
        }
        const float nan = __builtin_nanf("");
        float s[8];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const bool bad = (has_nan >> k) & 1;
            s[2 * k] = bad ? nan : mn[k];
            s[2 * k + 1] = bad ? nan : __fsub_rn(mx[k], mn[k]);        // inf - inf = NaN, as numpy has it
        }
        f32x4* o = reinterpret_cast<f32x4*>(v.stats);
        o[0] = f32x4{s[0], s[1], s[2], s[3]};
        o[1] = f32x4{s[4], s[5], 0.f, 0.f};
    }
}

// grid (ceil(Wc / PTPB), ceil((yhi - ylo + 1) / PROWS)).  DEPTH: src is the depth map [Hs, Ws]; otherwise a float32 [Hs, Ws, 3] map.
template <int TAPS, bool DEPTH>
__global__ __launch_bounds__(PTPB) void prep_hpass_kernel(PrepView v, const float* __restrict__ src) {
    const int j = blockIdx.x * PTPB + threadIdx.x;
    if (j >= v.Wc) return;
    int ix[TAPS];
    double wx[TAPS], fx[TAPS];
    {
        const size_t row = (size_t)(v.x0 + j) * TAPS;           // 16-byte aligned rows: TAPS * 4 and TAPS * 8 bytes
#pragma unroll
        for (int k = 0; k < TAPS; k += 4) {
            const i32x4 q = *reinterpret_cast<const i32x4*>(v.idx_x + row + k);
            ix[k] = q.x; ix[k + 1] = q.y; ix[k + 2] = q.z; ix[k + 3] = q.w;
        }
#pragma unroll
        for (int k = 0; k < TAPS; k += 2) {
            const f64x2 q = *reinterpret_cast<const f64x2*>(v.w_x + row + k);
            wx[k] = q.x; wx[k + 1] = q.y;
        }
#pragma unroll
        for (int k = 0; k < TAPS; k++) fx[k] = (double)ix[k] - v.cx;
    }
    float mn[3] = {0.f, 0.f, 0.f}, den[3] = {1.f, 1.f, 1.f};
    if (DEPTH) {
#pragma unroll
        for (int c = 0; c < 3; c++) { mn[c] = v.stats[2 * c]; den[c] = v.stats[2 * c + 1]; }
    }
    const int ya = v.ylo + blockIdx.y * PROWS;
#pragma unroll
    for (int r = 0; r < PROWS; r++) {
        const int y = ya + r;
        if (y > v.yhi) break;
        const double fy = (double)y - v.cy;
        double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < TAPS; k++) {
            float c[3];
            if (DEPTH) {
                const float d = src[(size_t)y * v.Ws + ix[k]];
                prep_unproject(d, fx[k], fy, v.focal, c[0], c[1]);
                c[2] = d;
#pragma unroll
                for (int q = 0; q < 3; q++) c[q] = __fdiv_rn(__fsub_rn(c[q], mn[q]), den[q]);
            } else {
                const float* p = src + ((size_t)y * v.Ws + ix[k]) * 3;
                c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
            }
#pragma unroll
            for (int q = 0; q < 3; q++) acc[q] = __dadd_rn(acc[q], __dmul_rn((double)c[q], wx[k]));
        }
        double* o = v.inter + ((size_t)y * v.Wc + j) * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

// grid (ceil(Wc * 3 / PCHUNK), Hc)
template <int TAPS, bool VEC>
__global__ __launch_bounds__(PTPB) void prep_vpass_kernel(PrepView v, float* __restrict__ out) {
    const int i = blockIdx.y, rowlen = v.Wc * 3, e0 = (blockIdx.x * PTPB + threadIdx.x) * PPX;
    if (e0 >= rowlen) return;
    const int* __restrict__ iy = v.idx_y + (size_t)(v.y0 + i) * TAPS;           // wave-uniform: scalar loads
    const double* __restrict__ wy = v.w_y + (size_t)(v.y0 + i) * TAPS;
    double acc[PPX] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < TAPS; k++) {
        const double* __restrict__ p = v.inter + (size_t)iy[k] * rowlen + e0;
        const double w = wy[k];
        double t[PPX];
        if (VEC) {                      // rowlen % 4 == 0: the four values are inside the row together, 32-byte aligned
            const f64x2 a = *reinterpret_cast<const f64x2*>(p), b = *reinterpret_cast<const f64x2*>(p + 2);
            t[0] = a.x; t[1] = a.y; t[2] = b.x; t[3] = b.y;
        } else {
#pragma unroll
            for (int q = 0; q < PPX; q++) t[q] = e0 + q < rowlen ? p[q] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < PPX; q++) acc[q] = __dadd_rn(acc[q], __dmul_rn(t[q], w));
    }
    float* o = out + (size_t)i * rowlen + e0;
    if (VEC) {
        *reinterpret_cast<f32x4*>(o) = f32x4{__double2float_rn(acc[0]), __double2float_rn(acc[1]), __double2float_rn(acc[2]),
                                             __double2float_rn(acc[3])};
    } else {
#pragma unroll
        for (int q = 0; q < PPX; q++)
            if (e0 + q < rowlen) o[q] = __double2float_rn(acc[q]);
    }
}

// grid (ceil(P / PCHUNK))
template <bool VEC>
__global__ __launch_bounds__(PTPB) void prep_image_kernel(const unsigned char* __restrict__ u8, int P, float* __restrict__ img,
                                                          unsigned char* __restrict__ mask) {
    const int p0 = (blockIdx.x * PTPB + threadIdx.x) * PPX;
    if (p0 >= P) return;
    unsigned char b[PPX * 3];
    if (VEC) {                          // P % 4 == 0: twelve bytes, 4-byte aligned
        const unsigned* q = reinterpret_cast<const unsigned*>(u8 + (size_t)p0 * 3);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const unsigned w = q[k];
            b[4 * k] = w & 0xFF; b[4 * k + 1] = (w >> 8) & 0xFF; b[4 * k + 2] = (w >> 16) & 0xFF; b[4 * k + 3] = w >> 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PPX * 3; k++) b[k] = (size_t)p0 * 3 + k < (size_t)P * 3 ? u8[(size_t)p0 * 3 + k] : 0;
    }
    float o[3][PPX];
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < PPX; i++) {
        float t[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            t[c] = __fdiv_rn((float)b[i * 3 + c], 255.f);                       // ToTensor
            o[c][i] = __fdiv_rn(__fsub_rn(t[c], 0.5f), 0.5f);                   // Normalize(0.5, 0.5)
        }
        const float s = __fadd_rn(__fadd_rn(t[0], t[1]), t[2]);
        bits |= (s <= 0.01f ? 0u : 1u) << (8 * i);                              // ~(sum <= 0.01)
    }
    if (VEC) {
#pragma unroll
        for (int c = 0; c < 3; c++) *reinterpret_cast<f32x4*>(img + (size_t)c * P + p0) = f32x4{o[c][0], o[c][1], o[c][2], o[c][3]};
        *reinterpret_cast<unsigned*>(mask + p0) = bits;
    } else {
#pragma unroll
        for (int i = 0; i < PPX; i++)
            if (p0 + i < P) {
#pragma unroll
                for (int c = 0; c < 3; c++) img[(size_t)c * P + p0 + i] = o[c][i];
                mask[p0 + i] = (unsigned char)((bits >> (8 * i)) & 1u);
            }
    }
}

}  // namespace a3r

// =============================================================================================== host
using namespace a3r;

extern "C" size_t a3r_prep_workspace_bytes(int Hs, int Ws, int Wc) {
    if (Hs <= 0 || Ws <= 0 || Wc <= 0) return 0;
    return prep_inter_bytes(Hs, Wc) + prep_partial_bytes(Hs, Ws) + prep_stats_bytes();
}

// everything both resampling entries refuse; fills the view
static int prep_check(const char* who, const float* src, const a3r_prep_desc* d, void* ws, size_t ws_bytes, float* out, PrepView& v) {
    A3R_CHECK_ARG(d, "%s: null descriptor", who);
    A3R_CHECK_ARG(d->Hs > 0 && d->Ws > 0 && d->Hr > 0 && d->Wr > 0 && d->Hc > 0 && d->Wc > 0,
                  "%s: sizes must be positive (Hs=%d Ws=%d Hr=%d Wr=%d Hc=%d Wc=%d)", who, d->Hs, d->Ws, d->Hr, d->Wr, d->Hc, d->Wc);
    A3R_CHECK_ARG(d->taps == 4 || d->taps == 8, "%s: taps = %d, must be 4 (cubic) or 8 (Lanczos-4)", who, d->taps);
    A3R_CHECK_ARG((long long)d->Hs * d->Ws < (1ll << 30) && (long long)d->Hs * d->Wc < (1ll << 28) && d->Hs <= 65535 && d->Hc <= 65535 && d->Hr < (1 << 24) &&
                  d->Wr < (1 << 24), "%s: the map is too large (Hs=%d Ws=%d Hc=%d Wc=%d)", who, d->Hs, d->Ws, d->Hc, d->Wc);
    A3R_CHECK_ARG(d->y0 >= 0 && d->x0 >= 0 && d->y0 <= d->Hr - d->Hc && d->x0 <= d->Wr - d->Wc,
                  "%s: the crop window (y0=%d x0=%d Hc=%d Wc=%d) is outside the resized map %d x %d", who, d->y0, d->x0, d->Hc, d->Wc, d->Hr, d->Wr);
    A3R_CHECK_ARG(src && out, "%s: null source or output buffer", who);
    A3R_CHECK_ARG(d->idx_x && d->idx_x_host && d->w_x && d->idx_y && d->idx_y_host && d->w_y, "%s: null index or weight table", who);
    A3R_CHECK_ARG(aligned_to(d->idx_x, 16) && aligned_to(d->w_x, 16) && aligned_to(d->idx_y, 16) && aligned_to(d->w_y, 16),
                  "%s: the device tables must be 16-byte aligned", who);
    const size_t need = a3r_prep_workspace_bytes(d->Hs, d->Ws, d->Wc);
    if (int rc = check_workspace(who, ws, ws_bytes, need)) return rc;
    for (long long k = 0; k < (long long)d->Wr * d->taps; k++)
        A3R_CHECK_ARG(d->idx_x_host[k] >= 0 && d->idx_x_host[k] < d->Ws, "%s: idx_x[%lld, %lld] = %d is outside [0, %d)", who, k / d->taps,
                      k % d->taps, d->idx_x_host[k], d->Ws);
    for (long long k = 0; k < (long long)d->Hr * d->taps; k++)
        A3R_CHECK_ARG(d->idx_y_host[k] >= 0 && d->idx_y_host[k] < d->Hs, "%s: idx_y[%lld, %lld] = %d is outside [0, %d)", who, k / d->taps,
                      k % d->taps, d->idx_y_host[k], d->Hs);
    v.Hs = d->Hs; v.Ws = d->Ws; v.P = d->Hs * d->Ws; v.nch = prep_nchunks(v.P);
    v.y0 = d->y0; v.x0 = d->x0; v.Hc = d->Hc; v.Wc = d->Wc;
    v.ylo = d->Hs - 1; v.yhi = 0;
    for (long long k = (long long)d->y0 * d->taps; k < (long long)(d->y0 + d->Hc) * d->taps; k++) {
        v.ylo = d->idx_y_host[k] < v.ylo ? d->idx_y_host[k] : v.ylo;
        v.yhi = d->idx_y_host[k] > v.yhi ? d->idx_y_host[k] : v.yhi;
    }
    v.focal = 1.0; v.cx = d->Ws / 2.0; v.cy = d->Hs / 2.0;
    v.idx_x = d->idx_x; v.w_x = d->w_x; v.idx_y = d->idx_y; v.w_y = d->w_y;
    char* w = static_cast<char*>(ws);
    v.inter = reinterpret_cast<double*>(w);
    v.partial = reinterpret_cast<float*>(w + prep_inter_bytes(d->Hs, d->Wc));
    v.stats = reinterpret_cast<float*>(w + prep_inter_bytes(d->Hs, d->Wc) + prep_partial_bytes(d->Hs, d->Ws));
    return A3R_OK;
}

template <bool DEPTH>
static void prep_resample(const PrepView& v, int taps, const float* src, float* out, hipStream_t st) {
    const dim3 block(PTPB);
    const dim3 gh((v.Wc + PTPB - 1) / PTPB, (v.yhi - v.ylo + PROWS) / PROWS);
    if (taps == 8) hipLaunchKernelGGL((prep_hpass_kernel<8, DEPTH>), gh, block, 0, st, v, src);
    else           hipLaunchKernelGGL((prep_hpass_kernel<4, DEPTH>), gh, block, 0, st, v, src);
    const dim3 gv((v.Wc * 3 + PCHUNK - 1) / PCHUNK, v.Hc);
    const bool vec = (v.Wc * 3) % 4 == 0 && aligned_to(out, 16);
#define A3R_PREP_VPASS(T, V) hipLaunchKernelGGL((prep_vpass_kernel<T, V>), gv, block, 0, st, v, out)
    if (taps == 8) { if (vec) A3R_PREP_VPASS(8, true); else A3R_PREP_VPASS(8, false); }
    else           { if (vec) A3R_PREP_VPASS(4, true); else A3R_PREP_VPASS(4, false); }
#undef A3R_PREP_VPASS
}

// Enqueues four kernels on `stream`: no allocation, no synchronisation, nothing read back (graph-capturable).
extern "C" int a3r_prep_pointmap(const float* depth, double focal, const a3r_prep_desc* d, void* ws, size_t ws_bytes, float* out, void* stream) {
    const char* who = "a3r_prep_pointmap";
    PrepView v;
    const int rc = prep_check(who, depth, d, ws, ws_bytes, out, v);
    if (rc != A3R_OK) return rc;
    A3R_CHECK_ARG(std::isfinite(focal) && focal != 0.0, "%s: the focal must be finite and non-zero (%g)", who, focal);
    v.focal = focal;
    hipStream_t st = as_stream(stream);
    if (v.P % 4 == 0 && aligned_to(depth, 16)) hipLaunchKernelGGL((prep_minmax_kernel<true>), dim3(v.nch), dim3(PTPB), 0, st, v, depth);
    else                                      hipLaunchKernelGGL((prep_minmax_kernel<false>), dim3(v.nch), dim3(PTPB), 0, st, v, depth);
    hipLaunchKernelGGL(prep_fold_kernel, dim3(1), dim3(PTPB), 0, st, v);
    prep_resample<true>(v, d->taps, depth, out, st);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

// The same resampling of a float32 [Hs, Ws, 3] map (no un-projection, no normalisation): two kernels.
extern "C" int a3r_prep_resize3(const float* src, const a3r_prep_desc* d, void* ws, size_t ws_bytes, float* out, void* stream) {
    PrepView v;
    const int rc = prep_check("a3r_prep_resize3", src, d, ws, ws_bytes, out, v);
    if (rc != A3R_OK) return rc;
    prep_resample<false>(v, d->taps, src, out, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_prep_image(const unsigned char* u8, int H, int W, float* img, unsigned char* mask, void* stream) {
    const char* who = "a3r_prep_image";
    A3R_CHECK_ARG(H > 0 && W > 0, "%s: H and W must be positive (H=%d W=%d)", who, H, W);
    A3R_CHECK_ARG((long long)H * W < (1ll << 28), "%s: H * W = %lld is too large", who, (long long)H * W);
    A3R_CHECK_ARG(u8 && img && mask, "%s: null image, output or mask buffer", who);
    const int P = H * W;
    const dim3 grid((P + PCHUNK - 1) / PCHUNK), block(PTPB);
    hipStream_t st = as_stream(stream);
    if (P % 4 == 0 && aligned_to(u8, 4) && aligned_to(img, 16) && aligned_to(mask, 4))
        hipLaunchKernelGGL((prep_image_kernel<true>), grid, block, 0, st, u8, P, img, mask);
    else
        hipLaunchKernelGGL((prep_image_kernel<false>), grid, block, 0, st, u8, P, img, mask);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
