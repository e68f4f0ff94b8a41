// RAFT2 ("SEA-RAFT") optical flow -- the flow provider of cloud_opt_flow -- as a launch plan over liba3r.
//
// The reference computes the flow of every pair, both directions, inside the aligner's constructor
// (dust3r/cloud_opt_flow/optimizer.py:118-154) with third_party/RAFT (third_party/raft.py:39-73 builds RAFT2 from
// core/configs/congif_spring_M.json).  Mirrored here, all under /root/reference/third_party/RAFT/core:
//   RAFT2.forward / upsample_data                      raft.py:152-246
//   ResNetFPN (context and feature encoders)           extractor.py:262-350, layer.py:113-141 (BasicBlock)
//   CorrBlock2 (pyramid over down-sampled fmap2)       corr.py:10-60, utils/utils.py:76-91 (bilinear_sampler)
//   BasicUpdateBlock2 / BasicMotionEncoder2            update.py:99-174
//   ConvNextBlock / LayerNorm                          layer.py:35-104
// Every 3x3 convolution and every 1x1 / Linear runs on liba3r's matrix-core kernels, in one of two operand forms (plan.h, Form)
// chosen per handle by a3r_raft_set_arith; the all-pairs correlation is the same GEMM with the second feature map as the weight
// operand.  The default is FH2, two fp16 planes (gemm_fh2.hip: fp32-grade while every stored value stays inside fp16's range).  Its
// range control is one device word: every fh2 producer of a call reports max |stored value| into it, a3r_raft_range reads it back,
// and a caller that finds it at or above 2^15 repeats the call in the other form (RaftEngine does).  That form is BF3, three bf16
// planes (gemm_bf3.hip: fp32-accurate with fp32's range, twice the matrix passes).  Weights are packed in both forms at finalize.
// What has no GEMM shape is in this file: the 7x7 stems on 3 / 6 / 2 channels, the depthwise 7x7 of ConvNeXt, the strided gather of
// the 1x1 shortcuts, 2x2 averaging, the correlation lookup and the convex up-sampling.  BatchNorm (evaluation mode) is folded into
// the convolutions by the caller (align3r_amd/raft_weights.py fold_batchnorm), as are the ConvNeXt layer scale (into pwconv2) and
// the 0.25 of the up-sampling weights (raft.py:216).  Maps are channels-last fp32 [B, h, w, C]; all buffers live in the caller's
// workspace.  Below: the kernels and their launchers, the weights as the plan reads them (bound once, at finalize), the pack plan,
// the launch plan, and the operator entries a3r_flow_* that run one kernel each through the same launchers.
#include "plan.h"
#include <cstdlib>
#include <initializer_list>
#include <new>

namespace a3r {

// ------------------------------------------------------------------------------------------- kernels
// direct convolution, k x k, for a handful of input channels (3, 6 or 2): y [B, Ho, Wo, Cout] channels-last.
// Input element (b, c, y, x) of source s sits at xs[s] + b sb + c sc + y sy + x sx and enters as x * in_mul + in_add (the image
// normalisation 2 (x / 255) - 1 of raft.py:194-195); the two sources are concatenated along channels (raft.py:207).
struct DirectConvArgs {
    const float* x0; const float* x1; int c0, c1;
    long sb, sc, sy, sx;
    int B, H, W, k, stride, pad, Ho, Wo, Cout;
    float in_mul, in_add;
    const float* w;      // [(c0 + c1) k k][Cout]  (transposed at finalize)
    const float* bias;
    int relu;
    float* y;
};
// A thread owns PX = 4 consecutive output columns of one output channel; lanes run over the output channels, so the weight loads
// (w transposed to [Cin k k][Cout] at finalize) are coalesced and the input loads are wave-wide broadcasts.  (The first version -- one
// output per thread, weights [Cout][Cin][k][k] -- spent 38 % of the whole flow network in this kernel.)
constexpr int DC_PX = 4;
__global__ __launch_bounds__(256) void direct_conv_kernel(DirectConvArgs a) {
    const int WoG = (a.Wo + DC_PX - 1) / DC_PX;
    const long total = (long)a.B * a.Ho * WoG * a.Cout;
    const int Cin = a.c0 + a.c1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int co = (int)(i % a.Cout);
        long p = i / a.Cout;
        const int ox0 = (int)(p % WoG) * DC_PX; p /= WoG;
        const int oy = (int)(p % a.Ho);
        const int b = (int)(p / a.Ho);
        float acc[DC_PX];
        const float bias = a.bias ? a.bias[co] : 0.f;
#pragma unroll
        for (int q = 0; q < DC_PX; q++) acc[q] = bias;
        for (int c = 0; c < Cin; c++) {
            const float* src = (c < a.c0 ? a.x0 + (long)c * a.sc : a.x1 + (long)(c - a.c0) * a.sc) + (long)b * a.sb;
            for (int ky = 0; ky < a.k; ky++) {
                const int iy = oy * a.stride - a.pad + ky;
                if (iy < 0 || iy >= a.H) continue;
                const float* row = src + (long)iy * a.sy;
                for (int kx = 0; kx < a.k; kx++) {
                    const float wv = a.w[(size_t)((c * a.k + ky) * a.k + kx) * a.Cout + co];
#pragma unroll
                    for (int q = 0; q < DC_PX; q++) {
                        const int ix = (ox0 + q) * a.stride - a.pad + kx;
                        if (ix >= 0 && ix < a.W) acc[q] = __fmaf_rn(row[(long)ix * a.sx] * a.in_mul + a.in_add, wv, acc[q]);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < DC_PX; q++)
            if (ox0 + q < a.Wo) a.y[(((long)b * a.Ho + oy) * a.Wo + ox0 + q) * a.Cout + co] = a.relu ? fmaxf(acc[q], 0.f) : acc[q];
    }
}

// The same convolution with the filter size, stride and pixels per thread fixed at compile time (the 7x7 stems, stride 2, and the
// update block's convf1, stride 1): per (channel, filter row) a thread loads the (PX - 1) S + K input columns its PX outputs share
// ONCE (normalised on the way in, zeros outside the image -- fma(0, w, acc) = acc, so the sums are bitwise those of the generic
// kernel, which skips the taps) and then runs K x PX fused multiply-adds from registers; the generic form issued one bounds-checked
// load per multiply-add.  Lanes are consecutive output channels: the input loads are broadcasts, the weight loads coalesced.
template <int K, int S, int PX>
__global__ __launch_bounds__(256) void direct_conv_fixed_kernel(DirectConvArgs a) {
    constexpr int NI = (PX - 1) * S + K;
    const int WoG = (a.Wo + PX - 1) / PX;
    const long total = (long)a.B * a.Ho * WoG * a.Cout;
    const int Cin = a.c0 + a.c1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int co = (int)(i % a.Cout);
        long p = i / a.Cout;
        const int ox0 = (int)(p % WoG) * PX; p /= WoG;
        const int oy = (int)(p % a.Ho);
        const int b = (int)(p / a.Ho);
        float acc[PX];
        const float bias = a.bias ? a.bias[co] : 0.f;
#pragma unroll
        for (int q = 0; q < PX; q++) acc[q] = bias;
        const int ix0 = ox0 * S - a.pad;
        for (int c = 0; c < Cin; c++) {
            const float* src = (c < a.c0 ? a.x0 + (long)c * a.sc : a.x1 + (long)(c - a.c0) * a.sc) + (long)b * a.sb;
#pragma unroll 1
            for (int ky = 0; ky < K; ky++) {
                const int iy = oy * S - a.pad + ky;
                if (iy < 0 || iy >= a.H) continue;
                const float* row = src + (long)iy * a.sy;
                float in[NI];
#pragma unroll
                for (int t = 0; t < NI; t++) {
                    const int ix = ix0 + t;
                    in[t] = (ix >= 0 && ix < a.W) ? row[(long)ix * a.sx] * a.in_mul + a.in_add : 0.f;
                }
                const float* wr = a.w + (size_t)((c * K + ky) * K) * a.Cout + co;
#pragma unroll
                for (int kx = 0; kx < K; kx++) {
                    const float wv = wr[(size_t)kx * a.Cout];
#pragma unroll
                    for (int q = 0; q < PX; q++) acc[q] = __fmaf_rn(in[q * S + kx], wv, acc[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < PX; q++)
            if (ox0 + q < a.Wo) a.y[(((long)b * a.Ho + oy) * a.Wo + ox0 + q) * a.Cout + co] = a.relu ? fmaxf(acc[q], 0.f) : acc[q];
    }
}

// depthwise 7x7, padding 3, channels-last x [B, h, w, C]; weights wt [49][C] (transposed at finalize), bias [C].  A thread owns 4
// consecutive output columns of one channel: 7 x 10 input loads for 4 outputs instead of 4 x 49.
__global__ __launch_bounds__(256) void dwconv7_kernel(const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                                                      float* __restrict__ y, int B, int h, int w, int C) {
    const int wG = (w + 3) / 4;
    const long total = (long)B * h * wG * C;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        long p = i / C;
        const int ox0 = (int)(p % wG) * 4; p /= wG;
        const int oy = (int)(p % h);
        const int b = (int)(p / h);
        float acc[4] = {bias[c], bias[c], bias[c], bias[c]};
        for (int ky = 0; ky < 7; ky++) {
            const int iy = oy - 3 + ky;
            if (iy < 0 || iy >= h) continue;
            const float* row = x + ((long)b * h + iy) * w * C + c;
            float v[10];
#pragma unroll
            for (int j = 0; j < 10; j++) {
                const int ix = ox0 - 3 + j;
                v[j] = (ix >= 0 && ix < w) ? row[(long)ix * C] : 0.f;
            }
#pragma unroll
            for (int kx = 0; kx < 7; kx++) {
                const float wv = wt[(ky * 7 + kx) * C + c];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int ix = ox0 + q - 3 + kx;
                    if (ix >= 0 && ix < w) acc[q] = __fmaf_rn(v[q + kx], wv, acc[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (ox0 + q < w) y[(((long)b * h + oy) * w + ox0 + q) * C + c] = acc[q];
    }
}

// y [B, ho, wo, C] = x [B, h, w, C] at (2 oy, 2 ox): the sampling of a 1x1 convolution with stride 2 (layer.py:125)
__global__ __launch_bounds__(256) void gather_s2_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int h, int w, int ho, int wo, int C4) {
    const long total = (long)B * ho * wo * C4;
    const f32x4* xv = reinterpret_cast<const f32x4*>(x);
    f32x4* yv = reinterpret_cast<f32x4*>(y);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4);
        long p = i / C4;
        const int ox = (int)(p % wo); p /= wo;
        const int oy = (int)(p % ho);
        const int b = (int)(p / ho);
        yv[i] = xv[(((long)b * h + 2 * oy) * w + 2 * ox) * C4 + c];
    }
}

// F.interpolate(scale_factor=0.5, mode='bilinear', align_corners=False) on channels-last maps (corr.py:22): the source position of
// output o is 2 o + 0.5, i.e. the plain mean of the 2x2 block (0.5 (0.5 a + 0.5 b) + 0.5 (0.5 c + 0.5 d) as ATen evaluates it)
__global__ __launch_bounds__(256) void halve_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int h, int w, int ho, int wo, int C) {
    const long total = (long)B * ho * wo * C;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        long p = i / C;
        const int ox = (int)(p % wo); p /= wo;
        const int oy = (int)(p % ho);
        const int b = (int)(p / ho);
        const float* r0 = x + (((long)b * h + 2 * oy) * w + 2 * ox) * C + c;
        const float* r1 = r0 + (long)w * C;
        const float t0 = 0.5f * r0[0] + 0.5f * r0[C], t1 = 0.5f * r1[0] + 0.5f * r1[C];
        y[i] = 0.5f * t0 + 0.5f * t1;
    }
}

__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, float s, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] *= s;
}

// max |x| of each of gridDim.y equally long images (out: one zeroed word per image; a non-negative float compares like its bit pattern)
__global__ __launch_bounds__(256) void image_absmax_kernel(const float* __restrict__ x, long n_per, unsigned* __restrict__ out) {
    const float* p = x + (size_t)blockIdx.y * n_per;
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_per; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(p[i]));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out + blockIdx.y, __float_as_uint(m));
}

// dst[r, c0 + c] = src[r, c] (c < Cs): channel concatenation of channels-last maps (torch.cat(dim=1) of the reference's NCHW tensors)
__global__ __launch_bounds__(256) void pack_cols_kernel(float* __restrict__ dst, int ldd, int c0, const float* __restrict__ src, int lds, int Cs, long rows) {
    const long total = rows * Cs;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / Cs;
        const int c = (int)(i - r * Cs);
        dst[r * ldd + c0 + c] = src[r * lds + c];
    }
}

// flow [rows, 2] += upd [rows, ldu][:, 0:2]      (raft.py:233)
__global__ __launch_bounds__(256) void flow_add_kernel(float* __restrict__ flow, const float* __restrict__ upd, int ldu, long rows) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < rows * 2; i += (long)gridDim.x * 256) flow[i] += upd[(i >> 1) * ldu + (i & 1)];
}

// Correlation lookup (corr.py:25-50): for query pixel q = (b, y, x) with target position (x + fx, y + fy), level l, window entry
// (a, c) in [0, 2r]^2: bilinear sample of corr_l[q] ([h_l, w_l]) at (cx / 2^l + (a - r), cy / 2^l + (c - r)) -- the reference stacks
// meshgrid(dy, dx), so the FIRST window index moves x -- with grid_sample's align_corners=True arithmetic (utils.py:79-84: the pixel
// coordinate goes through 2 v / (n - 1) - 1 and back) and zeros outside.  out [B h w, ldo]: channel l (2r+1)^2 + a (2r+1) + c; the
// columns from levels (2r+1)^2 up to ldo are zero-filled (K of the consumer GEMM is padded to a multiple of 32).
struct LookupArgs {
    const float* corr[4]; int hl[4], wl[4];
    const float* flow;        // [B h w, 2]
    float* out; int ldo;
    int B, h, w, r, levels;
};
__global__ __launch_bounds__(256) void corr_lookup_kernel(LookupArgs a) {
    const int win = 2 * a.r + 1, per = win * win, nch = a.levels * per;
    const long total = (long)a.B * a.h * a.w * a.ldo;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ch = (int)(i % a.ldo);
        const long q = i / a.ldo;
        if (ch >= nch) { a.out[i] = 0.f; continue; }
        const int l = ch / per, e = ch - l * per, wa = e / win, wc = e - wa * win;
        const int qx = (int)(q % a.w), qy = (int)((q / a.w) % a.h);
        const float cx = (float)qx + a.flow[q * 2], cy = (float)qy + a.flow[q * 2 + 1];          // coords_grid2 + flow (raft.py:227)
        const float div = (float)(1 << l);
        const float px = cx / div + (float)(wa - a.r), py = cy / div + (float)(wc - a.r);
        const int H = a.hl[l], W = a.wl[l];
        // bilinear_sampler: normalise, then grid_sample(align_corners=True) un-normalises
        const float gx = 2.f * px / (float)(W - 1) - 1.f, gy = 2.f * py / (float)(H - 1) - 1.f;
        const float ix = (gx + 1.f) * 0.5f * (float)(W - 1), iy = (gy + 1.f) * 0.5f * (float)(H - 1);
        const float fx0 = floorf(ix), fy0 = floorf(iy);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const float wx1 = ix - fx0, wy1 = iy - fy0, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
        const float* c = a.corr[l] + q * ((long)H * W);
        auto at = [&](int yy, int xx) { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? c[yy * W + xx] : 0.f; };
        a.out[i] = at(y0, x0) * (wx0 * wy0) + at(y0, x0 + 1) * (wx1 * wy0) + at(y0 + 1, x0) * (wx0 * wy1) + at(y0 + 1, x0 + 1) * (wx1 * wy1);
    }
}

// Convex up-sampling (raft.py:183-199): mask [B h w, 576] with channel k 64 + i 8 + j (k = ky 3 + kx over the 3x3 neighbourhood,
// (i, j) the position inside the 8x8 cell); softmax over k; out[b, c, 8 y + i, 8 x + j] = sum_k p_k 8 flow[b, y + ky - 1, x + kx - 1, c]
// (F.unfold pads with zeros).  out NCHW [B, 2, 8h, 8w].
__global__ __launch_bounds__(256) void convex_upsample_kernel(const float* __restrict__ flow, const float* __restrict__ mask, float* __restrict__ out,
                                                              int B, int h, int w) {
    const long total = (long)B * h * w * 64;
    for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int ij = (int)(t & 63), i = ij >> 3, j = ij & 7;
        const long q = t >> 6;
        const int x = (int)(q % w), y = (int)((q / w) % h), b = (int)(q / ((long)w * h));
        const float* m = mask + q * 576 + ij;
        float mv[9], mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < 9; k++) { mv[k] = m[k * 64]; mx = fmaxf(mx, mv[k]); }
        float den = 0.f;
#pragma unroll
        for (int k = 0; k < 9; k++) { mv[k] = expf(mv[k] - mx); den += mv[k]; }
        float o0 = 0.f, o1 = 0.f;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
            const float p = mv[k] / den;
            const float* f = flow + (((long)b * h + yy) * w + xx) * 2;
            o0 += p * (8.f * f[0]);
            o1 += p * (8.f * f[1]);
        }
        const long H8 = 8L * h, W8 = 8L * w;
        const long pix = ((long)(8 * y + i)) * W8 + (8 * x + j);
        out[((long)b * 2 + 0) * H8 * W8 + pix] = o0;
        out[((long)b * 2 + 1) * H8 * W8 + pix] = o1;
    }
}

// [N][K] -> [K][N]  (depthwise weights [C][49] -> [49][C]; direct-conv weights [Cout][Cin k k] -> [Cin k k][Cout])
__global__ void transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int N, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N * K) wt[(size_t)(i % K) * N + i / K] = w[i];
}

static inline unsigned grid1d(long n) {
    const long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

// ------------------------------------------------------------------------------------------- launchers
// One function per kernel: the plan below and the operator entries at the end of the file (a3r_flow_*, which the float64 pins of
// tests/test_gpu_flow_kernels_f64.py call) launch through these, so the grid a test runs is the grid of production.
// 7x7 convolutions of 2..6 input channels (stems, convf1): the fixed-size kernel where it applies, the generic one otherwise
// (force_generic: the entries' form 1; A3R_RAFT_DIRECT_CONV=generic does the same for a whole process)
static void launch_direct_conv(const DirectConvArgs& a, hipStream_t st, bool force_generic = false) {
    constexpr int PX = 8;
    const long work = (long)a.B * a.Ho * ((a.Wo + PX - 1) / PX) * a.Cout;
    static const bool env_generic = getenv("A3R_RAFT_DIRECT_CONV") && std::string(getenv("A3R_RAFT_DIRECT_CONV")) == "generic";     // A/B switch
    const bool generic = env_generic || force_generic;
    if (!generic && a.k == 7 && a.stride == 2) hipLaunchKernelGGL((direct_conv_fixed_kernel<7, 2, PX>), dim3(grid1d(work)), dim3(256), 0, st, a);
    else if (!generic && a.k == 7 && a.stride == 1) hipLaunchKernelGGL((direct_conv_fixed_kernel<7, 1, PX>), dim3(grid1d(work)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(direct_conv_kernel, dim3(grid1d((long)a.B * a.Ho * ((a.Wo + DC_PX - 1) / DC_PX) * a.Cout)), dim3(256), 0, st, a);
}
// a 7x7 convolution, padding 3, of B maps [H, W] given as strided planes (see DirectConvArgs) -> y [B, Ho, Wo, Cout]
struct Planes { const float *x0, *x1; int c0, c1; long sb, sc, sy, sx; float in_mul, in_add; };
static void launch_conv7(const Planes& src, const float* wt, const float* bias, int B, int H, int W, int stride, int Cout, int relu, float* y,
                         hipStream_t st, bool force_generic = false) {
    DirectConvArgs a = {};
    a.x0 = src.x0; a.x1 = src.x1; a.c0 = src.c0; a.c1 = src.c1;
    a.sb = src.sb; a.sc = src.sc; a.sy = src.sy; a.sx = src.sx;
    a.B = B; a.H = H; a.W = W; a.k = 7; a.stride = stride; a.pad = 3;
    a.Ho = (H - 1) / stride + 1; a.Wo = (W - 1) / stride + 1; a.Cout = Cout;
    a.in_mul = src.in_mul; a.in_add = src.in_add;
    a.w = wt; a.bias = bias; a.relu = relu; a.y = y;
    launch_direct_conv(a, st, force_generic);
}
// image planes [B, c, H, W] (one source, or two concatenated along channels); the channels-last 2-channel coarse flow [B, h, w, 2]
static Planes image_planes(const float* x0, const float* x1, int c, int H, int W, float in_mul, float in_add) {
    return {x0, x1, c, x1 ? c : 0, (long)c * H * W, (long)H * W, W, 1, in_mul, in_add};
}
static Planes flow_planes(const float* flow, int h, int w) { return {flow, nullptr, 2, 0, (long)h * w * 2, 1, (long)w * 2, 2, 1.f, 0.f}; }
static void launch_transpose(const float* w, float* wt, int N, int K, hipStream_t st) {
    hipLaunchKernelGGL(transpose_kernel, dim3((N * K + 255) / 256), dim3(256), 0, st, w, wt, N, K);
}
static void launch_dwconv7(const float* x, const float* wt, const float* bias, float* y, int B, int h, int w, int C, hipStream_t st) {
    hipLaunchKernelGGL(dwconv7_kernel, dim3(grid1d((long)B * h * ((w + 3) / 4) * C)), dim3(256), 0, st, x, wt, bias, y, B, h, w, C);
}
static void launch_gather_s2(const float* x, float* y, int B, int h, int w, int ho, int wo, int C, hipStream_t st) {
    hipLaunchKernelGGL(gather_s2_kernel, dim3(grid1d((long)B * ho * wo * C / 4)), dim3(256), 0, st, x, y, B, h, w, ho, wo, C / 4);
}
static void launch_halve(const float* x, float* y, int B, int h, int w, int ho, int wo, int C, hipStream_t st) {
    hipLaunchKernelGGL(halve_kernel, dim3(grid1d((long)B * ho * wo * C)), dim3(256), 0, st, x, y, B, h, w, ho, wo, C);
}
static void launch_scale(float* x, float s, long n, hipStream_t st) {
    hipLaunchKernelGGL(scale_kernel, dim3(grid1d(n)), dim3(256), 0, st, x, s, n);
}
static void launch_pack_cols(float* dst, int ldd, int c0, const float* src, int lds, int Cs, long rows, hipStream_t st) {
    hipLaunchKernelGGL(pack_cols_kernel, dim3(grid1d(rows * Cs)), dim3(256), 0, st, dst, ldd, c0, src, lds, Cs, rows);
}
static void launch_flow_add(float* flow, const float* upd, int ldu, long rows, hipStream_t st) {
    hipLaunchKernelGGL(flow_add_kernel, dim3(grid1d(rows * 2)), dim3(256), 0, st, flow, upd, ldu, rows);
}
// out [images] words, zeroed by the caller on the same stream
static void launch_image_absmax(const float* x, long n_per, int images, unsigned* out, hipStream_t st) {
    const long blocks = (n_per + 1023) / 1024;
    hipLaunchKernelGGL(image_absmax_kernel, dim3((unsigned)(blocks < 64 ? blocks : 64), images), dim3(256), 0, st, x, n_per, out);
}
static void launch_corr_lookup(const LookupArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(corr_lookup_kernel, dim3(grid1d((long)a.B * a.h * a.w * a.ldo)), dim3(256), 0, st, a);
}
static void launch_convex_upsample(const float* flow, const float* mask, float* out, int B, int h, int w, hipStream_t st) {
    hipLaunchKernelGGL(convex_upsample_kernel, dim3(grid1d((long)B * h * w * 64)), dim3(256), 0, st, flow, mask, out, B, h, w);
}

// ------------------------------------------------------------------------------------------- the weights, as the plan reads them
// Resolved once, by a3r_raft_finalize; the structs follow the network.  Shapes and block geometry are filled in by a3r_raft_create
// (the sizing pass needs them and runs on a handle without weights), pointers by finalize.
// a 3x3 convolution (K = 9 Cin) or a 1x1 / Linear as the matrix [N, K]: its twins in the packed buffer -- BOTH the bf3 image and the
// fh2 image, so that a3r_raft_set_arith can switch between them after finalize -- and its bias
struct RConvW { Twin w; const float* b = nullptr; int N = 0, K = 0; };
// a 7x7 direct or depthwise convolution: the weight, transposed into the packed buffer, and its bias
struct RDirectW { const float* wt = nullptr; const float* b = nullptr; };
struct RNormW { const float* w = nullptr; const float* b = nullptr; };
struct RBlockW { int cin = 0, dim = 0, stride = 1; bool project = false; RConvW conv1, conv2, down; };      // BasicBlock (`down`: if project)
struct REncoderW { RDirectW stem; std::vector<RBlockW> blocks; RConvW final_conv; };                         // ResNetFPN
struct RMotionW { RConvW convc1, convc2, convf2, conv; RDirectW convf1; };                                   // BasicMotionEncoder2
struct RRefineW { RDirectW dw; RNormW norm; RConvW pw1, pw2, fin; };                                         // ConvNextBlock
struct RHeadsW { RConvW flow0, flow2, up0, up2; };                                                           // flow_head, upsample_weight
struct RaftW { REncoderW cnet, fnet; RConvW init_conv; RHeadsW heads; RMotionW enc; std::vector<RRefineW> refine; };

// ------------------------------------------------------------------------------------------- weight plan
// One walk over the network names every weight the launch plan reads: `name`.weight and `name`.bias, what becomes of the weight in
// the packed buffer, and the field of RaftW that receives the result.
enum class Pack {
    CONV3,       // [N, K / 9, 3, 3] -> twins, through an fp32 [N, 3, 3, Cin] staging copy at `tmp`
    LINEAR,      // [N, K] or [N, K, 1, 1] -> twins
    DIRECT,      // 7x7 direct [N, K / 49, 7, 7] or depthwise [N, 1, 7, 7] (K = 49) -> fp32 [K][N]
    NORM,        // LayerNorm weight and bias [N]: nothing packed
};
struct RItem {
    std::string name; Pack kind; int N, K;
    RConvW* conv = nullptr; RDirectW* direct = nullptr; RNormW* norm = nullptr;
    size_t off = 0, tmp = 0, off2 = 0;      // packed image (bf3 twin or transposed fp32), conv staging, fh2 twin
};
struct PackPlan {
    std::vector<RItem> items;
    size_t total = 0;
    void add(RItem it) {
        it.off = total;
        const bool twin = it.kind == Pack::CONV3 || it.kind == Pack::LINEAR;
        if (twin) total = align_up(total + a3r_bf3_w_bytes(it.N, it.K), 256);
        else if (it.kind == Pack::DIRECT) total = align_up(total + (size_t)it.N * it.K * 4, 256);
        if (it.kind == Pack::CONV3) { it.tmp = total; total = align_up(total + (size_t)it.N * it.K * 4, 256); }
        if (twin) { it.conv->N = it.N; it.conv->K = it.K; }
        items.push_back(it);
    }
    void conv3(const std::string& n, int cout, int cin, RConvW* w) { RItem it{n, Pack::CONV3, cout, 9 * cin}; it.conv = w; add(it); }
    void linear(const std::string& n, int N, int K, RConvW* w) { RItem it{n, Pack::LINEAR, N, K}; it.conv = w; add(it); }
    void direct(const std::string& n, int cout, int cin, RDirectW* w) { RItem it{n, Pack::DIRECT, cout, 49 * cin}; it.direct = w; add(it); }
    void norm(const std::string& n, int N, RNormW* w) { RItem it{n, Pack::NORM, N, 0}; it.norm = w; add(it); }
};

// K of convc1: the correlation features levels (2 r + 1)^2, padded to the GEMM's K granularity (the lookup kernel writes the zeros)
static int corr_width(const a3r_raft_config& c) {
    const int win = 2 * c.radius + 1;
    return (c.corr_levels * win * win + 31) / 32 * 32;
}

static void encoder_items(PackPlan& pp, const std::string& p, const a3r_raft_config& c, int output_dim, REncoderW* e) {
    e->blocks.resize(c.n_blocks[0] + c.n_blocks[1] + c.n_blocks[2]);      // (the items point into it: sized once)
    RBlockW* b = e->blocks.data();
    int in_planes = c.initial_dim;
    for (int li = 0; li < 3; li++) {
        const int dim = c.block_dims[li];
        for (int bi = 0; bi < c.n_blocks[li]; bi++, b++) {
            const std::string q = p + ".layer" + std::to_string(li + 1) + "." + std::to_string(bi);
            b->cin = bi == 0 ? in_planes : dim;
            b->dim = dim;
            b->stride = bi == 0 && li > 0 ? 2 : 1;
            b->project = !(b->stride == 1 && b->cin == dim);               // layer.py:122-129
            pp.conv3(q + ".conv1", dim, b->cin, &b->conv1);
            pp.conv3(q + ".conv2", dim, dim, &b->conv2);
            if (b->project) pp.linear(q + ".downsample.0", dim, b->cin, &b->down);
        }
        in_planes = dim;
    }
    pp.linear(p + ".final_conv", output_dim, c.block_dims[2], &e->final_conv);
}

// The packed layout is the order of the lines here (observable: a3r_raft_packed_bytes, tests/golden/plan_sizes.json)
static void raft_pack_plan(const a3r_raft_config& c, PackPlan& pp, RaftW* w) {
    const int d = c.dim;
    const std::string e = "update_block.encoder.";
    pp.direct("cnet.conv1", c.initial_dim, 6, &w->cnet.stem);
    pp.direct("fnet.conv1", c.initial_dim, 3, &w->fnet.stem);
    pp.direct(e + "convf1", d, 2, &w->enc.convf1);
    encoder_items(pp, "cnet", c, 2 * d, &w->cnet);
    encoder_items(pp, "fnet", c, 2 * d, &w->fnet);
    pp.conv3("init_conv", 2 * d, 2 * d, &w->init_conv);
    pp.conv3("upsample_weight.0", 2 * d, d, &w->heads.up0);
    pp.linear("upsample_weight.2", 576, 2 * d, &w->heads.up2);
    pp.conv3("flow_head.0", 2 * d, d, &w->heads.flow0);
    pp.conv3("flow_head.2", 6, 2 * d, &w->heads.flow2);
    pp.linear(e + "convc1", 2 * d, corr_width(c), &w->enc.convc1);
    pp.conv3(e + "convc2", d + d / 2, 2 * d, &w->enc.convc2);
    pp.conv3(e + "convf2", d / 2, d, &w->enc.convf2);
    pp.conv3(e + "conv", d - 2, 2 * d, &w->enc.conv);
    w->refine.resize(c.num_blocks);
    for (int i = 0; i < c.num_blocks; i++) {
        const std::string q = "update_block.refine." + std::to_string(i) + ".";
        RRefineW& r = w->refine[i];
        pp.direct(q + "dwconv", 3 * d, 1, &r.dw);
        pp.norm(q + "norm", 3 * d, &r.norm);
        pp.linear(q + "pwconv1", 4 * d, 3 * d, &r.pw1);
        pp.linear(q + "pwconv2", 3 * d, 4 * d, &r.pw2);
        pp.linear(q + "final", d, 3 * d, &r.fin);
    }
    // second image of every conv / linear weight: fh2 form (4 bytes per element); then one line for the range statistic and the
    // absmax scratch word of the packing pass
    for (RItem& it : pp.items)
        if (it.conv) { it.off2 = pp.total; pp.total = align_up(pp.total + (size_t)it.N * it.K * 4, 256); }
    pp.total = align_up(pp.total + 256, 256);
}

}  // namespace a3r
using namespace a3r;

struct a3r_raft_s {
    a3r_raft_config cfg;
    WeightTable w;                                  // what a3r_raft_set_weight registered
    PackPlan pack;                                  // a3r_raft_create: the layout of the packed buffer ...
    RaftW bound;                                    // ... and the shapes of the bound weights; a3r_raft_finalize: their pointers
    bool finalized = false;
    bool use_fh2 = true;                            // a3r_raft_set_arith
    unsigned* stat = nullptr;                       // device word: max |value written in fh2 form| of the last forward (range check)
};

extern "C" int a3r_raft_create(const a3r_raft_config* cfg, a3r_raft_t* out) {
    A3R_CHECK_ARG(cfg && out, "a3r_raft_create: null argument");
    A3R_CHECK_ARG(cfg->initial_dim % 32 == 0 && cfg->dim % 64 == 0, "a3r_raft_create: initial_dim must be a multiple of 32 and dim of 64");
    for (int i = 0; i < 3; i++)
        A3R_CHECK_ARG(cfg->block_dims[i] % 32 == 0 && cfg->n_blocks[i] >= 1, "a3r_raft_create: block_dims must be multiples of 32");
    A3R_CHECK_ARG(cfg->corr_levels >= 1 && cfg->corr_levels <= 4 && cfg->radius >= 1 && cfg->radius <= 8 && cfg->num_blocks >= 1,
                  "a3r_raft_create: corr_levels in 1..4, radius in 1..8, num_blocks >= 1");
    a3r_raft_s* m = new (std::nothrow) a3r_raft_s();
    A3R_CHECK_ARG(m, "out of host memory");
    m->cfg = *cfg;
    raft_pack_plan(m->cfg, m->pack, &m->bound);
    *out = m;
    return A3R_OK;
}

extern "C" int a3r_raft_destroy(a3r_raft_t m) {
    delete m;
    return A3R_OK;
}

extern "C" int a3r_raft_set_weight(a3r_raft_t m, const char* name, const float* ptr, int ndim, const int64_t* shape) {
    A3R_CHECK_ARG(m, "a3r_raft_set_weight: bad argument");
    if (int rc = m->w.set("a3r_raft_set_weight", name, ptr, ndim, shape)) return rc;
    m->finalized = false;
    return A3R_OK;
}

extern "C" size_t a3r_raft_packed_bytes(a3r_raft_t m) {
    return m ? m->pack.total : 0;
}

extern "C" int a3r_raft_corr_width(a3r_raft_t m) {
    return m ? corr_width(m->cfg) : 0;
}

// One item of the pack plan: its weight into the packed buffer pk, weight and bias into the item's field of the bound weights.
// A name that was not registered is A3R_ESTATE, a shape that does not fit A3R_EINVAL, either with the name in a3r_last_error.
static int bind_item(a3r_raft_s* m, const RItem& it, char* pk, TwinTable<std::string>& twins, void* stream) {
    const char* who = "a3r_raft_finalize";
    const std::string wn = it.name + ".weight";
    const float *src, *bias;
    if (int rc = m->w.need(it.name + ".bias", {it.N}, who, &bias)) return rc;
    if (it.kind == Pack::NORM) {
        *it.norm = {nullptr, bias};
        return m->w.need(wn, {it.N}, who, &it.norm->w);
    }
    if (it.kind == Pack::DIRECT) {
        if (int rc = m->w.need(wn, {it.N, it.K / 49, 7, 7}, who, &src)) return rc;
        float* wt = reinterpret_cast<float*>(pk + it.off);
        launch_transpose(src, wt, it.N, it.K, as_stream(stream));
        A3R_LAUNCH_CHECK();
        *it.direct = {wt, bias};
        return A3R_OK;
    }
    if (it.kind == Pack::CONV3) {
        const int cin = it.K / 9;
        if (int rc = m->w.need(wn, {it.N, cin, 3, 3}, who, &src)) return rc;
        float* tmp = reinterpret_cast<float*>(pk + it.tmp);
        if (int rc = a3r_pack_conv3x3(src, tmp, it.N, cin, stream)) return rc;
        src = tmp;
    } else {
        // Linear weights are [N, K]; 1x1 convolutions [N, K, 1, 1]
        const WeightTable::Ref* wi = m->w.find(wn);
        if (!wi) { set_error("%s: missing weight '%s'", who, wn.c_str()); return A3R_ESTATE; }
        const std::vector<int64_t>& sh = wi->shape;
        const bool ok = (sh.size() == 2 || (sh.size() == 4 && sh[2] == 1 && sh[3] == 1)) && sh[0] == it.N && sh[1] == it.K;
        A3R_CHECK_ARG(ok, "%s: weight '%s' must be [%d, %d] (or [%d, %d, 1, 1])", who, wn.c_str(), it.N, it.K, it.N, it.K);
        src = wi->p;
    }
    float* scratch = reinterpret_cast<float*>(pk + m->pack.total - 128);     // the absmax word of the fh2 packing
    if (int rc = twins.pack(wn, Form::BF3, src, pk + it.off, it.N, it.K, nullptr, who, wn.c_str(), stream)) return rc;
    if (int rc = twins.pack(wn, Form::FH2, src, pk + it.off2, it.N, it.K, scratch, who, wn.c_str(), stream)) return rc;
    it.conv->w = twins.t[wn];
    it.conv->b = bias;
    return A3R_OK;
}

extern "C" int a3r_raft_finalize(a3r_raft_t m, void* packed, size_t packed_bytes, void* stream) {
    A3R_CHECK_ARG(m && packed, "a3r_raft_finalize: null argument");
    const size_t total = m->pack.total;
    A3R_CHECK_ARG(packed_bytes >= total, "a3r_raft_finalize: packed buffer too small (%zu < %zu)", packed_bytes, total);
    A3R_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & 255) == 0, "a3r_raft_finalize: packed buffer must be 256-byte aligned");
    char* pk = static_cast<char*>(packed);
    m->finalized = false;
    m->stat = reinterpret_cast<unsigned*>(pk + total - 256);
    TwinTable<std::string> twins;
    for (const RItem& it : m->pack.items)
        if (int rc = bind_item(m, it, pk, twins, stream)) return rc;
    m->finalized = true;
    return A3R_OK;
}

// ------------------------------------------------------------------------------------------- launch plan
namespace {
struct RPlan {
    a3r_raft_s* m;
    Arena ar;
    void* stream;
    int rc = A3R_OK;
    static constexpr const char* WHO = "a3r_raft_forward";
    bool skip() { return ar.skip(rc, WHO); }
    OpEpi epi(int kind, const float* resid = nullptr) {      // (the bias is the bound weight's: target)
        OpEpi e = {};
        e.epi = kind; e.resid = resid;
        return e;
    }
    // Operands ("xo" maps and matrices, out_op / aux_op epilogues) are in form f: FH2 (3 fp16 passes, 4 operand bytes) unless
    // a3r_raft_set_arith chose BF3 (6 bf16 passes, 6 bytes).  Every operand buffer is sized for BF3, the larger, so that the workspace
    // layout does not depend on the arithmetic.  Range policy: fh2 operands carry scale 1 (but the correlation's, below), and every
    // fh2 producer reports max |stored value| into the one word m->stat, which the caller checks against fp16's range after the forward.
    Form f = Form::FH2;
    float* alloc_op(size_t rows, int K) { return ar.alloc(form_floats(Form::BF3, rows, K)); }
    a3r_epilogue target(const OpEpi& e0, const float* bias) {
        a3r_epilogue e = retarget(e0, f, [&](a3r_epilogue& r) { r.out_absmax = (r.out_fh2 || r.aux_fh2) ? m->stat : nullptr; });
        e.bias = bias;
        return e;
    }
    // 3x3 convolution c on the operand-form map xo [B, H, W, c.K / 9] -> y [B, Ho, Wo, c.N]
    void conv3(const float* xo, const RConvW& c, float* y, int B, int H, int W, int stride, const OpEpi& e0) {
        if (skip()) return;
        rc = op_conv3x3(f, xo, nullptr, &c.w, y, B, H, W, c.K / 9, c.N, stride, target(e0, c.b), stream);
    }
    // 1x1 convolution / Linear c on the operand-form rows xo [M, c.K] -> y [M, c.N]
    void linear(const float* xo, const RConvW& c, float* y, long M, const OpEpi& e0) {
        if (skip()) return;
        rc = op_linear(f, xo, 0, nullptr, &c.w, y, c.N, (int)M, c.N, c.K, target(e0, c.b), stream);
    }
    void split(const float* x, int ldx, float* yo, long M, int K) {
        if (skip()) return;
        rc = op_split(f, x, ldx, yo, M, K, false, 1.f, m->stat, stream);
    }
    // LayerNorm (eps 1e-6) of the fp32 rows x [M, C] into operand form
    void layernorm(const float* x, const RNormW& n, float* yo, long M, int C) {
        if (skip()) return;
        rc = f == Form::FH2 ? a3r_layernorm_fh2(x, n.w, n.b, yo, (int)M, C, 1e-6f, 1.f, m->stat, stream)
                            : a3r_layernorm_bf3(x, n.w, n.b, yo, (int)M, C, 1e-6f, 0, stream);
    }
    template <class F> void launch(F&& f) {
        if (skip()) return;
        f(as_stream(stream));
        if (hipGetLastError() != hipSuccess) { set_error("a3r_raft_forward: kernel launch failed"); rc = A3R_EHIP; }
    }
    void pack_cols(float* dst, int ldd, int c0, const float* src, int lds, int Cs, long rows) {
        launch([&](hipStream_t st) { launch_pack_cols(dst, ldd, c0, src, lds, Cs, rows, st); });
    }
    // n floats device to device: the given feature maps, the correlation's copy of fmap1, and the taps (dst null: not asked for)
    void copy(float* dst, const float* src, size_t n) {
        if (skip() || !dst) return;
        if (hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, as_stream(stream)) != hipSuccess) { set_error("a3r_raft_forward: device copy failed"); rc = A3R_EHIP; }
    }
    // a 7x7 direct convolution (padding 3, ReLU) of B maps [H, W] -> y [B, Ho, Wo, Cout]; src: where input element (b, c, y, x) sits
    void conv7(const RDirectW& w, const Planes& src, int B, int H, int W, int stride, int Cout, float* y) {
        launch([&](hipStream_t st) { launch_conv7(src, w.wt, w.b, B, H, W, stride, Cout, /*relu=*/1, y, st); });
    }
};

// ResNetFPN.forward (extractor.py:338-350) after the stem: s = relu(bn1(conv1(x))) [nimg, H2, W2, C0] fp32 is given.  Writes
// final_conv's output to out (fp32 [nimg, h, w, out_dim]) or, when out3 is given, in operand form to out3.
void resnet(RPlan& P, const REncoderW& enc, float* s, int nimg, int H2, int W2, float* out, float* out3) {
    Arena& ar = P.ar;
    int h = H2, w = W2;
    const int C0 = P.m->cfg.initial_dim;
    const float* x = s;                                  // fp32 block input
    float* x3 = P.alloc_op((size_t)nimg * h * w, C0);
    P.split(x, C0, x3, (long)nimg * h * w, C0);
    for (const RBlockW& b : enc.blocks) {
        const int cin = b.cin, dim = b.dim;
        const int ho = (h - 1) / b.stride + 1, wo = (w - 1) / b.stride + 1;
        const size_t px = (size_t)nimg * ho * wo;
        // y = relu(bn1(conv1(x)))                                                        layer.py:134
        float* y3 = P.alloc_op(px, dim);
        OpEpi e1 = P.epi(A3R_EPI_RELU);
        e1.out_op = 1;
        P.conv3(x3, b.conv1, y3, nimg, h, w, b.stride, e1);
        // shortcut: x, or bn3(conv1x1 stride s (x))                                      layer.py:122-129,137-138
        const float* sc = x;
        if (b.project) {
            const float* g3 = x3;
            if (b.stride == 2) {
                float* gx = ar.alloc(px * cin);
                P.launch([&](hipStream_t st) { launch_gather_s2(x, gx, nimg, h, w, ho, wo, cin, st); });
                float* gx3 = P.alloc_op(px, cin);
                P.split(gx, cin, gx3, (long)px, cin);
                g3 = gx3;
            }
            float* scb = ar.alloc(px * dim);
            P.linear(g3, b.down, scb, (long)px, P.epi(A3R_EPI_NONE));
            sc = scb;
        }
        // y = relu(bn2(conv2(y))); out = relu(shortcut + y)                              layer.py:135-141: ONE launch
        float* o = ar.alloc(px * dim);
        float* o3 = P.alloc_op(px, dim);
        OpEpi e2 = P.epi(A3R_EPI_RESID, sc);
        e2.relu_acc = 1; e2.relu_out = 1; e2.aux_op = o3;
        P.conv3(y3, b.conv2, o, nimg, ho, wo, 1, e2);
        x = o; x3 = o3; h = ho; w = wo;
    }
    OpEpi ef = P.epi(A3R_EPI_NONE);
    if (out3) ef.out_op = 1;
    P.linear(x3, enc.final_conv, out3 ? out3 : out, (long)nimg * h * w, ef);
}

// ---- one call of the plan.  phase 0: RAFT2.forward(test_mode=True) (raft.py:185-246) for B pairs, img1 / img2 [B, 3, H, W] with
// values in [0, 255] -> flow_out [B, 2, H, W] (the last prediction; the reference up-samples every iteration's flow and returns the
// list, its caller keeps `[1]`); with fmap1_in / fmap2_in the feature network is skipped and those per-frame features are used.
// phase 1: the feature network alone on the B frames img1 -> fmap_out [B, h, w, 2 dim] (a3r_raft_encode).
// taps: optional intermediate copies for the parity tests (any pointer may be null).  dry: the sizing pass (every pointer null).
struct RaftCall {
    int phase = 0, B = 0, H = 0, W = 0, iters = 0;
    bool dry = false;
    const float *img1 = nullptr, *img2 = nullptr, *fmap1_in = nullptr, *fmap2_in = nullptr;
    float *fmap_out = nullptr, *flow_out = nullptr;
    a3r_raft_taps taps = {};
    void *ws = nullptr, *stream = nullptr;
    size_t ws_bytes = 0;
};

// its shapes: hidden width d and feature width D, the eighth-resolution map h x w (hw pixels, Bhw in the batch), the stems' half
// resolution, the correlation window and feature count (cc, padded: ccp), and the pyramid's levels
struct RaftDims {
    const a3r_raft_config& c;
    int B, H, W, d, D, h, w, H2, W2;
    long hw, Bhw;
    int win, cc, ccp, hl[4], wl[4];
    RaftDims(const a3r_raft_config& c_, const RaftCall& k)
        : c(c_), B(k.B), H(k.H), W(k.W), d(c.dim), D(2 * c.dim), h(k.H / 8), w(k.W / 8), H2((k.H - 1) / 2 + 1), W2((k.W - 1) / 2 + 1),
          hw((long)h * w), Bhw(B * hw), win(2 * c.radius + 1), cc(c.corr_levels * win * win), ccp(corr_width(c)) {
        for (int l = 0, a = h, b = w; l < 4; l++, a /= 2, b /= 2) { hl[l] = a; wl[l] = b; }      // corr.py:22
    }
    size_t stem_floats() const { return (size_t)B * H2 * W2 * c.initial_dim; }      // one stem's output
};

// the buffers that outlive a stage (allocated below the arena mark the stages release to)
struct RState {
    float* cn;           // init_conv output: [net | context]
    float* fm3;          // fnet(image1), fnet(image2) in operand form (rows: all of image1, then image2)
    float* fm;           // the same in fp32 (the pyramid's 2x2 means, the taps)
    float* corr[4];      // the correlation pyramid
    float* net;          // hidden state
    float* X;            // [net | context | motion features]: the ConvNeXt blocks' input (update.py:170-173)
    float* flow8;        // coarse flow
    float* fu;           // flow_head output: flow update (2) + info (4)
    float* wgt;          // .25 * upsample_weight(net)
};
// the scratch of the heads and of one iteration, allocated once above the mark (names ending in 3: operand form)
struct RIter { float *n3, *t3, *lk, *lk3, *c13, *cf, *tmp, *f1, *f13, *cf3, *dw, *ln3, *hid3, *S, *S3; };

// a 7x7 stem on image planes [B, 3, H, W] in [0, 255], normalised to 2 x / 255 - 1 on the way in (raft.py:194-195); x1: a second
// image, concatenated along channels (raft.py:207)
void stem(RPlan& P, const RDirectW& w, const float* x0, const float* x1, const RaftDims& g, float* y) {
    P.conv7(w, image_planes(x0, x1, 3, g.H, g.W, 2.f / 255.f, -1.f), g.B, g.H, g.W, 2, g.c.initial_dim, y);
}

// context network on cat(image1, image2) and init_conv (raft.py:207-209); net, context = split(cnet) (raft.py:210)
void context_stage(RPlan& P, const RaftCall& k, const RaftDims& g, const RState& v) {
    const RaftW& wt = P.m->bound;
    {
        ArenaScope scope(P.ar);
        float* s = P.ar.alloc(g.stem_floats());
        stem(P, wt.cnet.stem, k.img1, k.img2, g, s);
        float* c3 = P.alloc_op(g.Bhw, g.D);
        resnet(P, wt.cnet, s, g.B, g.H2, g.W2, nullptr, c3);
        P.conv3(c3, wt.init_conv, v.cn, g.B, g.h, g.w, 1, P.epi(A3R_EPI_NONE));
    }
    P.copy(k.taps.cnet, v.cn, (size_t)g.Bhw * g.D);
    P.pack_cols(v.net, g.d, 0, v.cn, g.D, g.d, g.Bhw);
    P.pack_cols(v.X, 3 * g.d, g.d, v.cn + g.d, g.D, g.d, g.Bhw);
}

// feature network (raft.py:222-223; its rows do not depend on what else is in the batch) on both images -> out [2 B, h, w, D], or
// the per-frame features a3r_raft_encode computed once, copied there.  Phase 1: on the B frames img1 -> out [B, h, w, D]
void feature_stage(RPlan& P, const RaftCall& k, const RaftDims& g, float* out) {
    ArenaScope scope(P.ar);
    if (k.fmap1_in && k.fmap2_in) {
        const size_t n = (size_t)g.Bhw * g.D;
        P.copy(out, k.fmap1_in, n);
        P.copy(out + n, k.fmap2_in, n);
        return;
    }
    const REncoderW& fnet = P.m->bound.fnet;
    const int sides = k.phase == 1 ? 1 : 2;
    float* s = P.ar.alloc(sides * g.stem_floats());
    stem(P, fnet.stem, k.img1, nullptr, g, s);
    if (sides == 2) stem(P, fnet.stem, k.img2, nullptr, g, s + g.stem_floats());
    if (k.phase == 1 && k.dry) P.ar.alloc(g.Bhw * g.D);      // (a3r_raft_encode's sizing has always counted the output map)
    resnet(P, fnet, s, sides * g.B, g.H2, g.W2, out, nullptr);
}

// fh2 operands of the correlation: feature maps have no fixed magnitude (a checkpoint's final_conv decides it), and two fp16 planes
// at scale 1 are fp32-grade only while max|x| is in [2^-2, 2^15] (fh2.h).  So every image's map is stored with its own power of two,
// the one a weight matrix would get (max|s x| in [2^12, 2^13)), from that image's max|fmap| -- read back here: the ONE wait on the
// stream of an fh2 call (bf3 calls have none).  Per image, not per batch: a pair's flow must not depend on what else is in the batch.
// s1 / s2 [B]: the scales of fmap1 / sqrt(D) and of fmap2, 1 on entry; amx: 2 B device words.
void corr_scales(RPlan& P, const RaftDims& g, const float* fm, float* amx, std::vector<float>& s1, std::vector<float>& s2) {
    if (P.f != Form::FH2 || P.skip()) return;
    const int B = g.B;
    std::vector<float> mx(2 * B, 0.f);
    hipStream_t st = as_stream(P.stream);
    const long n_per = g.hw * g.D;
    bool ok = hipMemsetAsync(amx, 0, (size_t)2 * B * 4, st) == hipSuccess;
    if (ok) {
        launch_image_absmax(fm, n_per, 2 * B, reinterpret_cast<unsigned*>(amx), st);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(mx.data(), amx, (size_t)2 * B * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (!ok) { set_error("a3r_raft_forward: reading the feature maps' range failed"); P.rc = A3R_EHIP; }
    for (int b = 0; b < B && ok; b++) {                     // (zero / non-finite maximum: scale 1; the split then reports it)
        s1[b] = a3r_fh2_weight_scale(mx[b] / sqrtf((float)g.D));
        s2[b] = a3r_fh2_weight_scale(mx[B + b]);
    }
}

// the correlation pyramid (corr.py:11-23): corr_l[b] = fmap1[b] @ fmap2_l[b]^T / sqrt(dim) (corr.py:53-60).  fmap1 is scaled once;
// fmap2_l, 2 x 2 means of level l - 1, enters as the GEMM's weight operand
void corr_stage(RPlan& P, const RaftCall& k, const RaftDims& g, const RState& v) {
    Arena& ar = P.ar;
    const int B = g.B, D = g.D;
    const long hw = g.hw, Bhw = g.Bhw;
    const bool fh2 = P.f == Form::FH2;
    unsigned* stat = P.m->stat;
    {
        ArenaScope scope(ar);
        float* f1s = ar.alloc(Bhw * D);
        P.copy(f1s, v.fm, (size_t)Bhw * D);
        P.launch([&](hipStream_t st) { launch_scale(f1s, 1.f / sqrtf((float)D), Bhw * D, st); });
        std::vector<float> s1(B, 1.f), s2(B, 1.f);
        float* amx = ar.alloc(2 * B);
        corr_scales(P, g, v.fm, amx, s1, s2);
        if (fh2) {
            for (int b = 0; b < B && !P.skip(); b++)
                P.rc = op_split(P.f, f1s + (size_t)b * hw * D, D, v.fm3 + form_floats(P.f, (size_t)b * hw, D), hw, D, false, s1[b], stat, P.stream);
        } else {
            P.split(f1s, D, v.fm3, Bhw, D);
        }
        float* f2 = v.fm + (size_t)Bhw * D;                         // level 0 of fmap2
        float* f2n = ar.alloc((size_t)B * (g.h / 2) * (g.w / 2) * D);
        float* f2m = ar.alloc((size_t)B * (g.h / 4 > 0 ? g.h / 4 : 1) * (g.w / 4 > 0 ? g.w / 4 : 1) * D);
        float* w3 = ar.alloc((size_t)a3r_bf3_w_bytes(hw, D) / 4 + 64);
        for (int l = 0; l < g.c.corr_levels; l++) {
            const long n2 = (long)g.hl[l] * g.wl[l];
            for (int b = 0; b < B; b++) {
                if (P.skip()) break;
                // fmap2_l[b] in the weight layout of the form, with image b's scale under fh2
                // (the coarser levels are 2 x 2 means of level 0: their maximum is not above its, one s2 serves all levels)
                a3r_epilogue e = {};
                if (fh2) e.x_scale = s1[b];
                const Twin tw = {w3, w3, s2[b]};
                P.rc = op_split(P.f, f2 + (size_t)b * n2 * D, D, w3, n2, D, /*row_pair=*/true, s2[b], stat, P.stream);
                if (!P.rc) P.rc = op_linear(P.f, v.fm3 + form_floats(P.f, (size_t)b * hw, D), 0, nullptr, &tw, v.corr[l] + (size_t)b * hw * n2, (int)n2, (int)hw, (int)n2, D, e, P.stream);
            }
            if (l + 1 < g.c.corr_levels) {                           // fmap2 <- interpolate(fmap2, 0.5) (corr.py:22)
                float* dst = (f2 == f2n) ? f2m : f2n;
                const int ha = g.hl[l], wa = g.wl[l], hb = g.hl[l + 1], wb = g.wl[l + 1];
                const float* src = f2;
                P.launch([&](hipStream_t st) { launch_halve(src, dst, B, ha, wa, hb, wb, D, st); });
                f2 = dst;
            }
        }
    }
    for (int l = 0; l < g.c.corr_levels; l++) P.copy(k.taps.corr_pyr[l], v.corr[l], (size_t)Bhw * g.hl[l] * g.wl[l]);
}

// heads on the hidden state (raft.py:213-216, 230-231): fu = flow_head(net), wgt = .25 * upsample_weight(net)
void heads(RPlan& P, const RaftDims& g, const RState& v, const RIter& t) {
    const RHeadsW& hd = P.m->bound.heads;
    P.split(v.net, g.d, t.n3, g.Bhw, g.d);
    OpEpi er = P.epi(A3R_EPI_RELU);
    er.out_op = 1;
    P.conv3(t.n3, hd.flow0, t.t3, g.B, g.h, g.w, 1, er);
    P.conv3(t.t3, hd.flow2, v.fu, g.B, g.h, g.w, 1, P.epi(A3R_EPI_NONE));
    P.conv3(t.n3, hd.up0, t.t3, g.B, g.h, g.w, 1, er);
    P.linear(t.t3, hd.up2, v.wgt, g.Bhw, P.epi(A3R_EPI_NONE));
}

// corr = corr_fn(coords_grid + flow_8x) (raft.py:227-228) -> lk [Bhw, ccp]
void lookup(RPlan& P, const RaftDims& g, const RState& v, const RIter& t) {
    LookupArgs a = {};
    for (int l = 0; l < g.c.corr_levels; l++) { a.corr[l] = v.corr[l]; a.hl[l] = g.hl[l]; a.wl[l] = g.wl[l]; }
    a.flow = v.flow8; a.out = t.lk; a.ldo = g.ccp; a.B = g.B; a.h = g.h; a.w = g.w; a.r = g.c.radius; a.levels = g.c.corr_levels;
    P.launch([&](hipStream_t st) { launch_corr_lookup(a, st); });
}

// BasicMotionEncoder2 (update.py:99-117): lk, flow8 -> the motion features, columns 2 d .. 3 d of X
void motion_encoder(RPlan& P, const RaftDims& g, const RState& v, const RIter& t) {
    const RMotionW& me = P.m->bound.enc;
    const int B = g.B, h = g.h, w = g.w, d = g.d;
    const long Bhw = g.Bhw;
    P.split(t.lk, g.ccp, t.lk3, Bhw, g.ccp);
    OpEpi er = P.epi(A3R_EPI_RELU);
    er.out_op = 1;
    P.linear(t.lk3, me.convc1, t.c13, Bhw, er);                                         // cor = relu(convc1(corr))
    P.conv3(t.c13, me.convc2, t.tmp, B, h, w, 1, P.epi(A3R_EPI_RELU));                   // cor = relu(convc2(cor))
    P.pack_cols(t.cf, 2 * d, 0, t.tmp, d + d / 2, d + d / 2, Bhw);
    // flo = relu(convf1(flow)): 7x7 on the 2 channels of the channels-last coarse flow
    P.conv7(me.convf1, flow_planes(v.flow8, h, w), B, h, w, 1, d, t.f1);
    P.split(t.f1, d, t.f13, Bhw, d);
    P.conv3(t.f13, me.convf2, t.tmp, B, h, w, 1, P.epi(A3R_EPI_RELU));                   // flo = relu(convf2(flo))
    P.pack_cols(t.cf, 2 * d, d + d / 2, t.tmp, d / 2, d / 2, Bhw);                       // cat([cor, flo]) (update.py:113)
    P.split(t.cf, 2 * d, t.cf3, Bhw, 2 * d);
    P.conv3(t.cf3, me.conv, t.tmp, B, h, w, 1, P.epi(A3R_EPI_RELU));                     // out = relu(conv(cat))
    P.pack_cols(v.X, 3 * d, 2 * d, t.tmp, d - 2, d - 2, Bhw);                            // motion = cat([out, flow])
    P.pack_cols(v.X, 3 * d, 3 * d - 2, v.flow8, 2, 2, Bhw);
}

// refine: net = ConvNextBlock_i(cat([net, inp])) for every block (update.py:170-173, layer.py:35-70)
void refine(RPlan& P, const RaftDims& g, const RState& v, const RIter& t) {
    const int B = g.B, h = g.h, w = g.w, d = g.d;
    const long Bhw = g.Bhw;
    for (const RRefineW& r : P.m->bound.refine) {
        P.pack_cols(v.X, 3 * d, 0, v.net, d, d, Bhw);
        P.launch([&](hipStream_t st) { launch_dwconv7(v.X, r.dw.wt, r.dw.b, t.dw, B, h, w, 3 * d, st); });
        P.layernorm(t.dw, r.norm, t.ln3, Bhw, 3 * d);
        OpEpi eg = P.epi(A3R_EPI_GELU);
        eg.out_op = 1;
        P.linear(t.ln3, r.pw1, t.hid3, Bhw, eg);
        OpEpi es = P.epi(A3R_EPI_RESID, v.X);                                            // input + gamma * pwconv2(...) (gamma folded)
        es.aux_op = t.S3;
        P.linear(t.hid3, r.pw2, t.S, Bhw, es);
        P.linear(t.S3, r.fin, v.net, Bhw, P.epi(A3R_EPI_NONE));
    }
}

// The plan of one call: the persistent buffers, then the stages.  What the sizing pass, the goldens (tests/golden/plan_sizes.json)
// and a bitwise comparison with an earlier build all rest on, and what an edit here must therefore keep:
//   * the order and the sizes of the allocations are the order of the lines here and inside each stage (workspace layout is
//     observable), and a stage's scratch is released to the same arena mark when the stage ends;
//   * the order of the launches, and the buffer each launch reads and writes;
//   * every operand buffer is sized for BF3, the larger form, so that the layout does not depend on the arithmetic;
//   * one range word, m->stat, receives every fh2 producer's maximum, and is cleared once, before the first launch;
//   * an fh2 call waits on the stream exactly once (corr_scales), a bf3 call never;
//   * no name is looked up: every weight was bound by a3r_raft_finalize (RaftW).
int raft_plan(a3r_raft_s* m, const RaftCall& k, size_t* peak = nullptr) {
    const RaftDims g(m->cfg, k);
    RPlan P;
    P.m = m; P.stream = k.stream; P.f = m->use_fh2 ? Form::FH2 : Form::BF3;
    P.ar = {static_cast<char*>(k.ws), 0, k.ws_bytes, k.dry, 0};
    Arena& ar = P.ar;
    if (!k.dry && P.f == Form::FH2 && m->stat && hipMemsetAsync(m->stat, 0, 4, as_stream(k.stream)) != hipSuccess) {
        set_error("a3r_raft_forward: clearing the range statistic failed");
        return A3R_EHIP;
    }
    if (k.phase == 1) {
        feature_stage(P, k, g, k.fmap_out);
        if (peak) *peak = ar.peak;
        return P.rc;
    }
    const int d = g.d;
    const long Bhw = g.Bhw;
    // ---------------- persistent buffers
    RState v = {};
    v.cn = ar.alloc(Bhw * 2 * d);
    v.fm3 = P.alloc_op(2 * Bhw, 2 * d);
    v.fm = ar.alloc(2 * Bhw * 2 * d);
    for (int l = 0; l < g.c.corr_levels; l++) v.corr[l] = ar.alloc((size_t)Bhw * g.hl[l] * g.wl[l]);
    v.net = ar.alloc(Bhw * d);
    v.X = ar.alloc(Bhw * 3 * d);
    v.flow8 = ar.alloc(Bhw * 2);
    v.fu = ar.alloc(Bhw * 6);
    v.wgt = ar.alloc(Bhw * 576);
    // ---------------- context, features (raft.py:222-223), correlation pyramid: each in its own scope above this mark
    context_stage(P, k, g, v);
    feature_stage(P, k, g, v.fm);
    P.copy(k.taps.fmap, v.fm, (size_t)2 * Bhw * 2 * d);
    corr_stage(P, k, g, v);
    // ---------------- scratch of the heads and the iterations
    RIter t = {};
    t.n3 = P.alloc_op(Bhw, d);
    t.t3 = P.alloc_op(Bhw, 2 * d);
    t.lk = ar.alloc(Bhw * g.ccp);
    t.lk3 = P.alloc_op(Bhw, g.ccp);
    t.c13 = P.alloc_op(Bhw, 2 * d);
    t.cf = ar.alloc(Bhw * 2 * d);
    t.tmp = ar.alloc(Bhw * 2 * d);
    t.f1 = ar.alloc(Bhw * d);
    t.f13 = P.alloc_op(Bhw, d);
    t.cf3 = P.alloc_op(Bhw, 2 * d);
    t.dw = ar.alloc(Bhw * 3 * d);
    t.ln3 = P.alloc_op(Bhw, 3 * d);
    t.hid3 = P.alloc_op(Bhw, 4 * d);
    t.S = ar.alloc(Bhw * 3 * d);
    t.S3 = P.alloc_op(Bhw, 3 * d);
    // ---------------- the first prediction, from the context network alone (raft.py:213-217)
    heads(P, g, v, t);
    P.copy(k.taps.flow_update0, v.fu, (size_t)Bhw * 6);
    P.copy(k.taps.weight0, v.wgt, (size_t)Bhw * 576);
    P.pack_cols(v.flow8, 2, 0, v.fu, 6, 2, Bhw);                     // flow_8x = flow_update[:, :2]
    // ---------------- iterations (raft.py:225-238)
    for (int it = 0; it < k.iters; it++) {
        lookup(P, g, v, t);
        if (it == 0) P.copy(k.taps.lookup0, t.lk, (size_t)Bhw * g.ccp);
        motion_encoder(P, g, v, t);
        if (it == 0 && k.taps.motion0) P.pack_cols(k.taps.motion0, d, 0, v.X + 2 * d, 3 * d, d, Bhw);      // (tap: the motion features alone)
        refine(P, g, v, t);
        heads(P, g, v, t);
        P.launch([&](hipStream_t st) { launch_flow_add(v.flow8, v.fu, 6, Bhw, st); });
        if (it < 4) {
            P.copy(k.taps.net[it], v.net, (size_t)Bhw * d);
            P.copy(k.taps.flow8[it], v.flow8, (size_t)Bhw * 2);
        }
    }
    // flow_up = upsample_data(flow_8x, info_8x, weight_update)[0] (raft.py:183-199, 236)
    P.launch([&](hipStream_t st) { launch_convex_upsample(v.flow8, v.wgt, k.flow_out, g.B, g.h, g.w, st); });
    if (peak) *peak = ar.peak;
    return P.rc;
}
}  // namespace

// the sizing pass: the workspace a call of this phase and shape needs (no allocation depends on the number of iterations)
static size_t raft_size(a3r_raft_t m, int phase, int B, int H, int W) {
    RaftCall k;
    k.phase = phase; k.B = B; k.H = H; k.W = W; k.dry = true;
    size_t peak = 0;
    raft_plan(m, k, &peak);
    return peak;
}

// what the three forward entry points share: their checks, then the launch pass of call k.  pointers: the entry's own are all given
static int raft_run(a3r_raft_t m, const RaftCall& k, bool pointers, const char* who) {
    const int B = k.B, H = k.H, W = k.W;
    A3R_CHECK_ARG(m, "%s: null handle", who);
    A3R_CHECK_ARG(B > 0 && k.iters >= 0, "%s: batch must be positive, iters non-negative", who);
    // InputPadder (utils.py:11-28) pads to multiples of 8; the pyramid halves the 1/8 map corr_levels times (corr.py:22)
    A3R_CHECK_ARG(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0, "%s: image size %dx%d must be a multiple of 8 (pad first, as InputPadder does)", who, H, W);
    A3R_CHECK_ARG(((H / 8) >> (m->cfg.corr_levels - 1)) >= 2 && ((W / 8) >> (m->cfg.corr_levels - 1)) >= 2,
                  "%s: image %dx%d too small for a %d-level correlation pyramid", who, H, W, m->cfg.corr_levels);
    if (!m->finalized) { set_error("%s: a3r_raft_finalize has not been called", who); return A3R_ESTATE; }
    A3R_CHECK_ARG(pointers && k.ws, "%s: null pointer", who);
    A3R_CHECK_ARG((reinterpret_cast<uintptr_t>(k.ws) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    const size_t need_bytes = raft_size(m, k.phase, B, H, W);
    A3R_CHECK_ARG(k.ws_bytes >= need_bytes, "%s: workspace too small (%zu < %zu)", who, k.ws_bytes, need_bytes);
    return raft_plan(m, k);
}

extern "C" size_t a3r_raft_workspace_bytes(a3r_raft_t m, int B, int H, int W) {
    if (!m || B <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8) return 0;
    return raft_size(m, 0, B, H, W);
}

extern "C" int a3r_raft_set_arith(a3r_raft_t m, int fh2) {
    A3R_CHECK_ARG(m, "a3r_raft_set_arith: null handle");
    const int prev = m->use_fh2 ? 1 : 0;
    m->use_fh2 = fh2 != 0;
    return prev;
}

extern "C" int a3r_raft_range(a3r_raft_t m, float* max_abs_host, void* stream) {
    A3R_CHECK_ARG(m && max_abs_host, "a3r_raft_range: null argument");
    if (!m->finalized || !m->stat) { set_error("a3r_raft_range: a3r_raft_finalize has not been called"); return A3R_ESTATE; }
    A3R_HIP(hipMemcpyAsync(max_abs_host, m->stat, 4, hipMemcpyDeviceToHost, as_stream(stream)));
    A3R_HIP(hipStreamSynchronize(as_stream(stream)));
    return A3R_OK;
}

extern "C" int a3r_raft_encode(a3r_raft_t m, const float* image, int B, int H, int W, float* fmap, void* workspace, size_t workspace_bytes,
                               void* stream) {
    RaftCall k;
    k.phase = 1; k.B = B; k.H = H; k.W = W;
    k.img1 = image; k.fmap_out = fmap;
    k.ws = workspace; k.ws_bytes = workspace_bytes; k.stream = stream;
    return raft_run(m, k, image && fmap, "a3r_raft_encode");
}

extern "C" int a3r_raft_forward_features(a3r_raft_t m, const float* image1, const float* image2, const float* fmap1, const float* fmap2, int B,
                                         int H, int W, int iters, float* flow, void* workspace, size_t workspace_bytes, void* stream) {
    RaftCall k;
    k.B = B; k.H = H; k.W = W; k.iters = iters;
    k.img1 = image1; k.img2 = image2; k.fmap1_in = fmap1; k.fmap2_in = fmap2; k.flow_out = flow;
    k.ws = workspace; k.ws_bytes = workspace_bytes; k.stream = stream;
    return raft_run(m, k, image1 && image2 && fmap1 && fmap2 && flow, "a3r_raft_forward_features");
}

extern "C" int a3r_raft_forward(a3r_raft_t m, const float* image1, const float* image2, int B, int H, int W, int iters, float* flow,
                                void* workspace, size_t workspace_bytes, const a3r_raft_taps* taps, void* stream) {
    RaftCall k;
    k.B = B; k.H = H; k.W = W; k.iters = iters;
    k.img1 = image1; k.img2 = image2; k.flow_out = flow;
    if (taps) k.taps = *taps;
    k.ws = workspace; k.ws_bytes = workspace_bytes; k.stream = stream;
    return raft_run(m, k, image1 && image2 && flow, "a3r_raft_forward");
}

// ------------------------------------------------------------------------------------------- operator entries
// The kernels of this file one by one, through the launchers the plan uses (a3r.h has the contracts).  Sizes are bounded so that every
// int the kernels compute stays an int; buffers are the caller's.
#define A3R_FLOW_DIMS(who, ...) A3R_CHECK_ARG(flow_dims_ok({__VA_ARGS__}), who ": dimensions must be positive and their product below 2^31")
static bool flow_dims_ok(std::initializer_list<long> dims) {
    long n = 1;
    for (long d : dims) {
        if (d <= 0 || d > 0x7fffffffL) return false;
        n *= d;
        if (n > 0x7fffffffL) return false;
    }
    return true;
}

extern "C" int a3r_flow_conv7_planes(const float* x0, const float* x1, int c, const float* w, const float* bias, float* wt, float* y, int B,
                                     int H, int W, int Cout, float in_mul, float in_add, int relu, int form, void* stream) {
    A3R_CHECK_ARG(x0 && w && wt && y, "a3r_flow_conv7_planes: null pointer");
    A3R_CHECK_ARG(c >= 1 && c <= 3, "a3r_flow_conv7_planes: 1..3 channels per source (got %d)", c);
    A3R_CHECK_ARG(form == 0 || form == 1, "a3r_flow_conv7_planes: form must be 0 (as the plan chooses) or 1 (generic kernel)");
    A3R_FLOW_DIMS("a3r_flow_conv7_planes", B, c, H, W);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, Cin = x1 ? 2 * c : c;
    A3R_FLOW_DIMS("a3r_flow_conv7_planes", B, Ho, Wo, Cout);
    A3R_FLOW_DIMS("a3r_flow_conv7_planes", Cout, Cin * 49);
    launch_transpose(w, wt, Cout, Cin * 49, as_stream(stream));
    launch_conv7(image_planes(x0, x1, c, H, W, in_mul, in_add), wt, bias, B, H, W, 2, Cout, relu != 0, y, as_stream(stream), form == 1);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_conv7_flow(const float* flow, const float* w, const float* bias, float* wt, float* y, int B, int h, int wd, int Cout,
                                   int relu, int form, void* stream) {
    A3R_CHECK_ARG(flow && w && wt && y, "a3r_flow_conv7_flow: null pointer");
    A3R_CHECK_ARG(form == 0 || form == 1, "a3r_flow_conv7_flow: form must be 0 (as the plan chooses) or 1 (generic kernel)");
    A3R_FLOW_DIMS("a3r_flow_conv7_flow", B, h, wd, Cout);
    A3R_FLOW_DIMS("a3r_flow_conv7_flow", Cout, 2 * 49);
    launch_transpose(w, wt, Cout, 2 * 49, as_stream(stream));
    launch_conv7(flow_planes(flow, h, wd), wt, bias, B, h, wd, 1, Cout, relu != 0, y, as_stream(stream), form == 1);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_dwconv7(const float* x, const float* w, const float* bias, float* wt, float* y, int B, int h, int wd, int C, void* stream) {
    A3R_CHECK_ARG(x && w && bias && wt && y, "a3r_flow_dwconv7: null pointer");
    A3R_FLOW_DIMS("a3r_flow_dwconv7", B, h, wd, C);
    launch_transpose(w, wt, C, 49, as_stream(stream));
    launch_dwconv7(x, wt, bias, y, B, h, wd, C, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_gather_s2(const float* x, float* y, int B, int h, int wd, int C, void* stream) {
    A3R_CHECK_ARG(x && y, "a3r_flow_gather_s2: null pointer");
    A3R_CHECK_ARG(C % 4 == 0, "a3r_flow_gather_s2: C must be a multiple of 4 (got %d)", C);
    A3R_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0, "a3r_flow_gather_s2: x and y must be 16-byte aligned");
    A3R_FLOW_DIMS("a3r_flow_gather_s2", B, h, wd, C);
    launch_gather_s2(x, y, B, h, wd, (h - 1) / 2 + 1, (wd - 1) / 2 + 1, C, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_halve(const float* x, float* y, int B, int h, int wd, int C, void* stream) {
    A3R_CHECK_ARG(x && y, "a3r_flow_halve: null pointer");
    A3R_CHECK_ARG(h >= 2 && wd >= 2, "a3r_flow_halve: map %dx%d smaller than one 2x2 block", h, wd);
    A3R_FLOW_DIMS("a3r_flow_halve", B, h, wd, C);
    launch_halve(x, y, B, h, wd, h / 2, wd / 2, C, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_corr_lookup(const float* const* corr, const int* hl, const int* wl, const float* flow, float* out, int ldo, int B, int h,
                                    int wd, int r, int levels, void* stream) {
    A3R_CHECK_ARG(corr && hl && wl && flow && out, "a3r_flow_corr_lookup: null pointer");
    A3R_CHECK_ARG(levels >= 1 && levels <= 4 && r >= 1 && r <= 8, "a3r_flow_corr_lookup: levels in 1..4, r in 1..8");
    A3R_CHECK_ARG(ldo >= levels * (2 * r + 1) * (2 * r + 1), "a3r_flow_corr_lookup: ldo %d below the %d channels", ldo, levels * (2 * r + 1) * (2 * r + 1));
    A3R_FLOW_DIMS("a3r_flow_corr_lookup", B, h, wd);
    A3R_CHECK_ARG((long)B * h * wd * ldo < (1L << 40), "a3r_flow_corr_lookup: output too large");
    LookupArgs a = {};
    for (int l = 0; l < levels; l++) {
        A3R_CHECK_ARG(corr[l], "a3r_flow_corr_lookup: null level %d", l);
        A3R_CHECK_ARG(hl[l] >= 2 && wl[l] >= 2, "a3r_flow_corr_lookup: level %d is %dx%d, smaller than 2x2 (2 v / (n - 1) - 1 needs n >= 2)", l, hl[l], wl[l]);
        A3R_FLOW_DIMS("a3r_flow_corr_lookup", hl[l], wl[l]);
        a.corr[l] = corr[l]; a.hl[l] = hl[l]; a.wl[l] = wl[l];
    }
    a.flow = flow; a.out = out; a.ldo = ldo; a.B = B; a.h = h; a.w = wd; a.r = r; a.levels = levels;
    launch_corr_lookup(a, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_convex_upsample(const float* flow, const float* mask, float* out, int B, int h, int wd, void* stream) {
    A3R_CHECK_ARG(flow && mask && out, "a3r_flow_convex_upsample: null pointer");
    A3R_FLOW_DIMS("a3r_flow_convex_upsample", B, h, wd, 64);
    launch_convex_upsample(flow, mask, out, B, h, wd, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_scale(float* x, float s, long n, void* stream) {
    A3R_CHECK_ARG(x && n > 0, "a3r_flow_scale: null pointer or empty array");
    launch_scale(x, s, n, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_pack_cols(float* dst, int ldd, int c0, const float* src, int lds, int Cs, long rows, void* stream) {
    A3R_CHECK_ARG(dst && src, "a3r_flow_pack_cols: null pointer");
    A3R_CHECK_ARG(rows > 0 && Cs > 0 && c0 >= 0 && lds >= Cs && ldd >= c0 + Cs, "a3r_flow_pack_cols: columns %d..%d of %d from %d of %d do not fit", c0,
                  c0 + Cs, ldd, Cs, lds);
    launch_pack_cols(dst, ldd, c0, src, lds, Cs, rows, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_add(float* flow, const float* upd, int ldu, long rows, void* stream) {
    A3R_CHECK_ARG(flow && upd && rows > 0 && ldu >= 2, "a3r_flow_add: null pointer, no rows or ldu below 2");
    launch_flow_add(flow, upd, ldu, rows, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_flow_image_absmax(const float* x, long n_per, int images, unsigned* out, void* stream) {
    A3R_CHECK_ARG(x && out, "a3r_flow_image_absmax: null pointer");
    A3R_CHECK_ARG(n_per > 0 && images > 0 && images <= 65535, "a3r_flow_image_absmax: n_per positive, 1..65535 images");
    A3R_HIP(hipMemsetAsync(out, 0, (size_t)images * 4, as_stream(stream)));
    launch_image_absmax(x, n_per, images, out, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
