/*
 * a3r.h -- C ABI of liba3r.so, the MI355X (gfx950) pair-forward + global-alignment engine.
 *
 * The reference (OliEfr/Align3R) has no plugin/operator registry: its only native boundary is the
 * pybind function curope.rope_2d (croco/models/curope/curope.cpp:49-69); everything else on the hot
 * path is reached through Python.  This header therefore declares
 *   (1) a3r_rope2d            -- same semantics as curope.rope_2d,
 *   (2) the operators a reference nn.Module on the path maps to (Linear, LayerNorm, Attention,
 *       Conv2d/ConvTranspose2d/Interpolate of the DPT head, postprocess), each citing the reference
 *       lines it replaces, so that the Python mirror modules stay thin,
 *   (3) a3r_model_*           -- the whole AsymmetricCroCo3DStereo.forward (dust3r/model.py:241-257),
 *   (4) a3r_align_*           -- the PointCloudOptimizer inner loop (dust3r/cloud_opt/optimizer.py:223-241
 *                                + base_opt.py:424-464: loss, gradients, Adam).
 *
 * Conventions
 *   - plain C types only; every pointer is a CALLER-OWNED DEVICE buffer (e.g. torch tensor data_ptr())
 *     unless the name ends in _host; the library never allocates or frees device memory;
 *   - float = IEEE fp32; activations are channels-last: tokens [B, N, C], maps [B, H, W, C];
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued
 *     asynchronously, nothing synchronises;
 *   - return value 0 = ok; otherwise a negative A3R_E* code and a3r_last_error() holds a message
 *     (the Python wrapper raises RuntimeError, mirroring TORCH_CHECK in curope.cpp:54-59);
 *   - handles are not thread-safe; use one handle per host thread / GPU.
 */
#ifndef A3R_H
#define A3R_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A3R_OK 0
#define A3R_EINVAL (-1)   /* bad argument / shape */
#define A3R_EHIP (-2)     /* a HIP runtime call failed */
#define A3R_ESTATE (-3)   /* handle not in the required state (e.g. weights missing) */

const char* a3r_last_error(void);
int a3r_version(void);
/* number of HIP devices visible; does not initialise a context */
int a3r_device_count(void);

/* Per-kernel timing with HIP events recorded on the launch stream around every kernel launch of the
 * library (used by bench.py for the roofline numbers).  a3r_prof_enable(1) clears and starts recording,
 * a3r_prof_enable(0) stops.  a3r_prof_get synchronises the recorded events and returns, for kernel class
 * `kernel` (0 <= kernel < a3r_prof_kernel_count()), the number of launches, their summed duration and
 * the summed algorithmic work (FLOP for the MFMA kernels, bytes for the HBM-bound ones). */
int a3r_prof_enable(int on);
int a3r_prof_kernel_count(void);
int a3r_prof_get(int kernel, const char** name, long* launches, double* total_ms, double* total_work);
/* Summed ALGORITHMIC bytes of the MFMA-bound kernel classes (every operand read once, every result written once; 0 for classes
 * whose `work` already is a byte count): lets bench.py print algorithmic bytes per launch next to the PMC traffic. */
int a3r_prof_get_bytes(int kernel, double* total_bytes);

/* ------------------------------------------------------------------------------------------------
 * (1) 2-D rotary embedding, in place.  Replaces curope.rope_2d(tokens, positions, base, fwd)
 *     croco/models/curope/curope.cpp:49-69 / kernels.cu:17-108.
 *     tokens [B, N, H, D] fp32 (D % 4 == 0), positions [B, N, 2] int64 (y, x);
 *     first D/2 dims rotate with y, last D/2 with x, pairs (d, d + D/4), angle = fwd*pos*base^(-d/(D/4)).
 */
int a3r_rope2d(float* tokens, const int64_t* positions, int B, int N, int H, int D, float base, float fwd,
               void* stream);

/* ------------------------------------------------------------------------------------------------
 * (2) operators
 */

/* nn.LayerNorm over the last dim, eps as given (croco.py:34 uses 1e-6). x,y [M, D]; y may alias x. */
int a3r_layernorm(const float* x, const float* w, const float* b, float* y, int M, int D, float eps, void* stream);

/* Epilogues of a3r_linear / a3r_conv3x3 */
enum {
    A3R_EPI_NONE = 0,     /* y = acc (+bias) */
    A3R_EPI_GELU = 1,     /* y = gelu_erf(acc + bias)                      Mlp.fc1+act  blocks.py:73-75 */
    A3R_EPI_RESID = 2,    /* y = resid + acc + bias  (resid may alias y)  residual adds blocks.py:128-129 */
    A3R_EPI_RELU = 3,     /* y = relu(acc + bias) */
    A3R_EPI_ROPE = 4,     /* y = rope2d(acc + bias) on the first rope_cols columns (heads of 64), rest plain:
                             fuses RoPE2D (pos_embed.py:141-157) into the q/k projections blocks.py:96-103,155-162 */
    A3R_EPI_RESID2 = 5,   /* y = resid + resid2 + acc + bias              RCU skip + fusion add dpt_block.py:142,198 */
    A3R_EPI_PIXSHUF = 6,  /* ConvTranspose2d(kernel=stride=s) scatter: row = input pixel, col = (dy,dx,co) */
    A3R_EPI_HEAD = 7      /* fh2 kernels, N == 128 only: the tail of the DPT head fused into its last 3x3 conv -- t = relu(acc + bias)
                             [M, 128] never reaches memory; f = t @ head_w^T + head_b (Conv2d 1x1 128 -> 4, dpt_block.py:328) and the
                             postprocess (heads/postprocess.py:10-58: pts3d = xyz / max(|xyz|, 1e-8) * expm1(|xyz|), conf = 1 + exp(f3))
                             are done in the epilogue: y = pts3d [M, 3], head_conf = conf [M] */
};

typedef struct {
    int epi;              /* A3R_EPI_* */
    const float* bias;    /* [N] or NULL */
    const float* resid;   /* [M, ldc] for RESID/RESID2 */
    const float* resid2;  /* [M, ldc] for RESID2 */
    int relu_a;           /* a3r_conv3x3 only: relu on the input while staging it (RCU pre-activation dpt_block.py:131,136) */
    /* ROPE */
    int rope_cols;        /* leading output columns to rotate (multiple of 64) */
    int tokens_per_image; /* N tokens; row r has token index r % N */
    int grid_w;           /* tokens per image row: pos = (tok / grid_w, tok % grid_w)  (PositionGetter blocks.py:195-207) */
    const float* rope_cos;/* [max_pos, 16] cos table (a3r_rope_table) */
    const float* rope_sin;
    /* PIXSHUF */
    int ps_s, ps_h, ps_w, ps_cout;  /* stride s, input map h x w, output channels */
    /* a3r_linear_bf3 only: write y in bf3 form ([M][N/8][3][8] bf16, N % 8 == 0, ldc = N) instead of fp32, for outputs that
     * only feed the next bf3 kernel (Mlp: fc1 + GELU -> fc2, blocks.py:73-77; qkv + RoPE -> attention).  NONE / GELU / RELU / ROPE. */
    int out_bf3;
    /* bf3 kernels only: ALSO write the result (after bias / activation / residuals; through a ReLU if aux_relu) in bf3 form
     * [M][N/8][3][8] to aux_bf3 -- the pre-activated input of the next 3x3 conv of a ResidualConvUnit, whose fp32 value is
     * still needed for the skip connection (dpt_block.py:131-141). */
    void* aux_bf3;
    int aux_relu;
    /* a3r_linear_bf3 only -- operand layouts rather than epilogue options, kept here so the entry points stay as they are:
     * x_pair: x3 is stored in the ROW-PAIR form (the layout a3r_split_bf3_w documents; produced by a3r_split_bf3_w,
     * a3r_layernorm_bf3(pair = 1), a3r_attention_bf3(out_pair = 1) or an out_bf3 + out_pair epilogue).  out_pair: with out_bf3, write
     * y in that form (N % 32 == 0) -- for outputs only ever read as the x3 of another a3r_linear_bf3 (fc1 + GELU -> fc2).
     * A matrix with an odd number of rows occupies (rows + 1) * K * 6 bytes in this form (a3r_bf3_w_bytes). */
    int x_pair;
    int out_pair;
    /* a3r_linear_fh2 only: write y in fh2 form ([M][N/8][2][8] fp16, N % 32 == 0, ldc = N) instead of fp32, for outputs that only
     * feed the next a3r_linear_fh2 (Mlp: fc1 + GELU -> fc2, blocks.py:73-77).  NONE / GELU / RELU. */
    int out_fh2;
    /* fh2 kernels only: ALSO write the result (after bias / activation / residuals; through a ReLU if aux_relu) in fh2 form
     * [M][N/8][2][8] to aux_fh2 -- as aux_bf3, for the DPT convolutions on the fh2 kernel (y, resid, resid2 16-byte aligned). */
    void* aux_fh2;
    /* fh2 kernels only -- range control of the fh2 operands (see a3r_model_range_check).  All three may stay zero.
     * x_scale: the power of two the x2 operand was stored with (0 = 1); out_scale: the power of two to store the out_fh2 / aux_fh2
     * output with (0 = 1: the planes hold out_scale * value); out_absmax: device word that receives max |out_scale * value| over
     * that output by an atomic max on the bit pattern (NULL: no statistics; the caller zeroes it beforehand).  The grouped entry
     * point takes them per group (a3r_group_ptrs_fh2) and ignores these. */
    float x_scale, out_scale;
    unsigned* out_absmax;
    /* A3R_EPI_HEAD */
    const float* head_w;  /* [4, 128] */
    const float* head_b;  /* [4] */
    float* head_conf;     /* [M] */
    /* RESID / RESID2 only (fp32 y, LDS-staged or direct epilogue of the 16x16 kernels): y = relu(resid (+ resid2) + acc + bias) -- the
     * tail of a ResNet BasicBlock, `return self.relu(x + y)` (third_party/RAFT/core/layer.py:141); an aux_bf3 / aux_fh2 twin then holds the
     * same relu-ed value */
    int relu_out;
    /* RESID / RESID2 only: the branch is clamped BEFORE the addition, y = resid + relu(acc + bias) (then relu_out) -- BasicBlock's
     * `y = relu(bn2(conv2(y))); return relu(x + y)` (layer.py:135-141).  Either flag with any other epilogue is refused (A3R_EINVAL). */
    int relu_acc;
} a3r_epilogue;

/* nn.Linear: y[M, N] = x[M, K] @ w[N, K]^T (+ epilogue).  lda/ldc = row strides in floats
 * (K % 32 == 0, lda % 4 == 0).  fp32 MFMA (v_mfma_f32_32x32x2_f32), exact fp32 products. */
int a3r_linear(const float* x, int lda, const float* w, float* y, int ldc, int M, int N, int K,
               const a3r_epilogue* epi, void* stream);

/* Up to 4 same-shape nn.Linear problems in ONE launch (e.g. the two decoders' projections, model.py:218-220):
 * per-problem operands, shared M/N/K, leading dimensions and epilogue kind (epi->bias/resid/resid2 are ignored,
 * the per-group pointers are used instead). */
typedef struct {
    const float* x;
    const float* w;
    float* y;
    const float* bias;
    const float* resid;
    const float* resid2;
} a3r_group_ptrs;
int a3r_linear_grouped(const a3r_group_ptrs* groups, int n_groups, int lda, int ldc, int M, int N, int K,
                       const a3r_epilogue* epi, void* stream);

/* ---- the same nn.Linear on the bf16 matrix cores, fp32-accurate ("bf3" operands)
 * An fp32 matrix X [R, K] (K % 8 == 0) in bf3 form is three bf16 planes with X = X0 + X1 + X2 exactly, laid out
 * [R][K/8][3][8] bf16 (6 K bytes per row, a3r_bf3_bytes).  a3r_linear_bf3 evaluates the six bf16 x bf16 plane
 * products whose magnitude reaches fp32 precision (each exact in the fp32 accumulator; the dropped terms are
 * <= 2^-23 |x w| per product), so y matches a3r_linear to fp32 rounding while running on the 16x faster bf16 MFMA
 * pipes.  Replaces the same call sites as a3r_linear (blocks.py:58-169); epilogues as above. K % 32 == 0. */
size_t a3r_bf3_bytes(long rows, int K);
/* Process-wide arithmetic mode of the bf3 kernels (a3r_linear_bf3 / a3r_conv3x3_bf3 / a3r_attention_bf3): the plane products
 * evaluated per multiply.  6 (default): all products down to 2^-16, fp32-accurate.  3: a0 b0 + a0 b1 + a1 b0, operands
 * effectively 16 bits (error ~2^-17 per product).  1: a0 b0 only = plain bf16 operands, fp32 accumulation -- BASELINE config 5's
 * "bf16-MFMA mode", a reduced-precision mode that is never the default.  Returns the previous value; other values are ignored. */
int a3r_bf3_set_products(int products);
/* Process-wide arithmetic mode of the fh2 kernels (a3r_linear_fh2 / a3r_conv3x3_fh2 / a3r_attention_fh2): matrix passes per product.
 * 3 (default): h0 g0 + h0 g1 + h1 g0, fp32-grade.  1: h0 g0 only = plain fp16 operands (11 significant bits, kept inside fp16's range by
 * the same per-site scales), fp32 accumulation -- the 16-bit operand mode (A3R_GEMM=f16; BASELINE config 5's reduced-precision role with
 * three more mantissa bits than bf16), never the default.  Returns the previous value; other values are ignored. */
int a3r_fh2_set_passes(int passes);
/* fp32 x [M, ldx] (first K columns) -> bf3 y [M][K/8][3][8] */
int a3r_split_bf3(const float* x, int ldx, void* y, long M, int K, void* stream);
/* WEIGHT operands (w3 of a3r_linear_bf3, wp3 of a3r_conv3x3_bf3) use the row-pair form of the layout,
 * [ceil(N/2)][K/32][2 rows][4][3][8] bf16 (K % 32 == 0): rows 2j, 2j+1 interleaved per 32-deep k block, so the 32 k of a row
 * pair that one GEMM stage fetches are 384 contiguous bytes = three whole cache lines (the plain form drags 2 lines per row for
 * 1.5 lines of payload).  byte offset of (n, k) = (n/2) 12K + (k/32) 384 + (n%2) 192 + ((k/8)%4) 48 + plane 16 + (k%8) 2. */
size_t a3r_bf3_w_bytes(long rows, int K);
int a3r_split_bf3_w(const float* w, int ldw, void* y, long N, int K, void* stream);
/* nn.LayerNorm (as a3r_layernorm) writing its output directly in bf3 form (D % 8 == 0): the producer of every
 * transformer GEMM input (blocks.py:127-130,186-190), fused so the fp32 normalised rows never reach HBM.
 * pair != 0: y3 in the row-pair form (D % 32 == 0), for rows that only feed a3r_linear_bf3 (x_pair). */
int a3r_layernorm_bf3(const float* x, const float* w, const float* b, void* y3, int M, int D, float eps, int pair, void* stream);
/* x3: bf3 [M, K] (a3r_split_bf3 / a3r_layernorm_bf3 / a bf3 epilogue output); w3: [N, K] in the weight layout (a3r_split_bf3_w) */
int a3r_linear_bf3(const void* x3, const void* w3, float* y, int ldc, int M, int N, int K, const a3r_epilogue* epi,
                   void* stream);
typedef struct {
    const void* x3;       /* bf3 [M, K] */
    const void* w3;       /* bf3 [N, K], row-pair weight layout (a3r_split_bf3_w) */
    float* y;
    const float* bias;
    const float* resid;
    const float* resid2;
} a3r_group_ptrs_bf3;
int a3r_linear_bf3_grouped(const a3r_group_ptrs_bf3* groups, int n_groups, int ldc, int M, int N, int K,
                           const a3r_epilogue* epi, void* stream);

/* ---- the same nn.Linear on the fp16 matrix cores, fp32-GEMM-accurate ("fh2" operands)
 * An fp32 matrix X [R, K] (K % 32 == 0) in fh2 form is two fp16 planes, s X ~ X0 + X1 (X0 = rn_f16(s X), X1 = rn_f16(s X - X0)), laid
 * out [R][K/8][2][8] fp16 (4 K bytes per row, a3r_fh2_bytes), with s a power of two: 1 for activations, a3r_fh2_weight_scale(max|w|)
 * for weights.  a3r_linear_fh2 evaluates x0 w0 + x0 w1 + x1 w0 -- three fp16 MFMA passes, every product exact in the fp32
 * accumulator -- so the operands carry 22 of fp32's 24 significant bits; against float64 the result is as accurate as a3r_linear's
 * (the fp32 accumulation error dominates: tests/test_gpu_fh2.py) at half the matrix passes of a3r_linear_bf3.
 * Same call sites as a3r_linear (blocks.py:58-169); epilogues as above (no PIXSHUF), out_bf3 for the projections that feed the
 * attention kernel, out_fh2 (NONE / GELU / RELU / ROPE) for fc1 + GELU -> fc2 and for the q / k / v of a3r_attention_fh2. */
size_t a3r_fh2_bytes(long rows, int K);
/* fp32 x [M, ldx] (first K columns) * scale -> fh2 y (K % 8 == 0); absmax (device, may be NULL): atomic max of |scale * x| */
int a3r_split_fh2(const float* x, int ldx, void* y, long M, int K, float scale, unsigned* absmax, void* stream);
/* max |x| over n floats -> *out_dev (device float; the call zeroes it first) and the weight scale derived from it (host helper) */
int a3r_absmax(const float* x, long n, float* out_dev, void* stream);
float a3r_fh2_weight_scale(float absmax);
/* nn.LayerNorm (as a3r_layernorm) writing scale * y in fh2 form (D % 32 == 0; scale a power of two, absmax as a3r_split_fh2) */
int a3r_layernorm_fh2(const float* x, const float* w, const float* b, void* y2, int M, int D, float eps, float scale,
                      unsigned* absmax, void* stream);
typedef struct {
    const void* x2;       /* fh2 [M, K], stored with x_scale */
    const void* w2;       /* fh2 [N, K], stored with w_scale */
    float* y;
    const float* bias;
    const float* resid;
    const float* resid2;
    float w_scale;
    float x_scale;        /* 0 = 1 */
    float out_scale;      /* out_fh2 / aux_fh2 output: 0 = 1 */
    unsigned* out_absmax; /* or NULL */
} a3r_group_ptrs_fh2;
int a3r_linear_fh2_grouped(const a3r_group_ptrs_fh2* groups, int n_groups, int ldc, int M, int N, int K, const a3r_epilogue* epi,
                           void* stream);
int a3r_linear_fh2(const void* x2, const void* w2, float w_scale, float* y, int ldc, int M, int N, int K, const a3r_epilogue* epi,
                   void* stream);

/* nn.Conv2d(k=3, padding=1, stride in {1,2}) as an implicit GEMM on the bf3 kernel: x3 = bf3 form of the channels-last map
 * [B, H, W, Cin] (i.e. of the [B H W, Cin] matrix), wp3 = bf3 form of the packed weights [Cout, 9 Cin] (a3r_pack_conv3x3
 * then a3r_split_bf3_w); y [B, Ho, Wo, Cout] fp32 (or bf3 with out_bf3).  Same call sites as a3r_conv3x3 (dpt_block.py). */
int a3r_conv3x3_bf3(const void* x3, const void* wp3, float* y, int B, int H, int W, int Cin, int Cout, int stride,
                    const a3r_epilogue* epi, void* stream);

/* The same on the fh2 kernel: x2 = fh2 form of the channels-last map (scale 1), wp2 = fh2 form of the packed weights [Cout, 9 Cin]
 * (a3r_pack_conv3x3 then a3r_split_fh2 with the power-of-two w_scale of a3r_fh2_weight_scale); Cin % 32 == 0.  y fp32
 * (optionally also aux_fh2) or fh2 (out_fh2, Cout % 32 == 0).  Same call sites as a3r_conv3x3 (dpt_block.py:120-142, 186-218, 323-330). */
int a3r_conv3x3_fh2(const void* x2, const void* wp2, float w_scale, float* y, int B, int H, int W, int Cin, int Cout, int stride,
                    const a3r_epilogue* epi, void* stream);

/* nn.Conv2d(k=3, padding=1, stride in {1,2}) on channels-last x [B, H, W, Cin] with PACKED weights
 * wp [Cout, 3, 3, Cin] (a3r_pack_conv3x3 from the checkpoint layout [Cout, Cin, 3, 3]); Cin % 32 == 0.
 * y [B, Ho, Wo, Cout].  Implicit GEMM on the same MFMA core.  (dpt_block.py:33-68,93-111,323-329,402-405) */
int a3r_conv3x3(const float* x, const float* wp, float* y, int B, int H, int W, int Cin, int Cout, int stride,
                const a3r_epilogue* epi, void* stream);
int a3r_pack_conv3x3(const float* w, float* wp, int Cout, int Cin, void* stream);
/* ConvTranspose2d weight [Cin, Cout, s, s] -> [(dy*s+dx)*Cout + co, Cin] for a3r_linear + A3R_EPI_PIXSHUF */
int a3r_pack_convT(const float* w, float* wp, int Cin, int Cout, int s, void* stream);

/* softmax(q k^T / sqrt(64)) v per head, head_dim 64 (Attention/CrossAttention blocks.py:105-109,164-168).
 * q [B, Nq, ldq], k/v [B, Nk, ldk/ldv] with head h at column h*64; o [B, Nq, ldo].  q,k already rotated. */
int a3r_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                  int B, int H, int Nq, int Nk, void* stream);
/* The same attention on the bf16 matrix cores with fp32 accuracy: q3 / k3 / v3 / o3 are bf3 matrices (pointers to the first
 * column's 48-byte group, leading dimensions in fp32 columns, multiples of 8); six exact bf16 MFMA passes per product,
 * fp32 softmax, P split exactly into three planes in registers.  Consumes the RoPE + out_bf3 output of a3r_linear_bf3 and
 * produces the bf3 input of the output projection (out_pair != 0: in the row-pair form, ldo % 32 == 0, o3 = the matrix origin;
 * q3 / k3 / v3 are always plain rows). */
int a3r_attention_bf3(const void* q3, int ldq, const void* k3, int ldk, const void* v3, int ldv, void* o3, int ldo,
                      int B, int H, int Nq, int Nk, int out_pair, void* stream);
/* the same, writing o in fh2 form (scale 1, plain rows, ldo % 8 == 0): the input of an a3r_linear_fh2 output projection */
int a3r_attention_bf3_fh2out(const void* q3, int ldq, const void* k3, int ldk, const void* v3, int ldv, void* o2, int ldo,
                             int B, int H, int Nq, int Nk, void* stream);

/* The same attention on the fp16 matrix cores from fh2 operands (q2 / k2 / v2 / o2: fh2 matrices, pointers to the first column's
 * 32-byte group, leading dimensions in fp32 columns, multiples of 8): three exact fp16 MFMA passes per product, fp32 softmax,
 * P split into two fp16 planes of 1024 p in registers.  Consumes the RoPE + out_fh2 output of a3r_linear_fh2 and produces the fh2
 * input of the output projection.  range (or NULL = all ones, no statistics): the powers of two q2 / k2 / v2 were stored with (divided
 * out exactly: q_scale k_scale in the exp2 argument, v_scale with the softmax normaliser), the one to store o2 with, and the
 * device word receiving max |out_scale * o| (see a3r_epilogue.out_absmax); zeros mean 1 / none. */
typedef struct {
    float q_scale, k_scale, v_scale, out_scale;
    unsigned* out_absmax;
} a3r_fh2_attn_range;
int a3r_attention_fh2(const void* q2, int ldq, const void* k2, int ldk, const void* v2, int ldv, void* o2, int ldo,
                      int B, int H, int Nq, int Nk, const a3r_fh2_attn_range* range, void* stream);
/* The same with image maps (device, B words each, or NULL = the identity): batch b takes the q rows of image q_map[b] of q2 and the
 * k / v rows of image kv_map[b] of k2 / v2, and writes the o rows of image b -- a3r_attention_fh2 on explicitly gathered operands,
 * bit for bit, without the gather.  With both maps NULL it is a3r_attention_fh2.  Kernel form 2 only (an error with form 1). */
int a3r_attention_fh2_mapped(const void* q2, int ldq, const void* k2, int ldk, const void* v2, int ldv, void* o2, int ldo,
                             int B, int H, int Nq, int Nk, const a3r_fh2_attn_range* range, const int32_t* q_map,
                             const int32_t* kv_map, void* stream);
/* Kernel form behind a3r_attention_fh2: 2 (default: K and V tiles by LDS-DMA, transposed LDS reads) or 1 (round 2: V staged through
 * registers); the results are bitwise equal (tests/test_gpu_fh2.py).  Returns the previous form, or a negative error code.
 * Process-wide; environment A3R_ATTN=v1 selects form 1 at start-up.  A development switch, not part of the reference's interface. */
int a3r_attention_fh2_set_form(int form);

/* cos/sin tables [max_pos, 16] for head_dim 64 computed like RoPE2D.get_cos_sin (pos_embed.py:118-128);
 * HOST buffers. */
int a3r_rope_table_host(float* cos_host, float* sin_host, int max_pos, float base);

/* PatchEmbedDust3R conv k=s=16 as im2col: cols[B*N, C*256] with k = c*256 + py*16 + px
 * (patch_embed.py:19-29).  img element (b,c,y,x) at b*sb + c*sc + y*sy + x*sx (floats). */
int a3r_patchify(const float* img, float* cols, int B, int C, int H, int W, long sb, long sc, long sy, long sx,
                 void* stream);

/* F.interpolate(scale_factor=2, bilinear, align_corners=True) on [B, H, W, C], writing only the
 * top-left Hc x Wc window of the 2H x 2W result (crop of dpt_head.py:57 folded in). C % 4 == 0. */
/* Raw weighted second moments of B point-set pairs for the similarity registrations of the aligner's initialisation
 * (cloud_opt/init_im_poses.py:415-418, roma.rigid_points_registration): problem b uses x + x_off[b], y + y_off[b] ([P,3] each) and
 * w + w_off[b] ([P]) (element offsets, device int64).  partial [B][a3r_umeyama_chunks(P)][17] doubles:
 * sum w | sum w x (3) | sum w y (3) | sum w |x|^2 | sum w y_r x_c (9, r major); the caller adds the chunks. */
int a3r_umeyama_chunks(int P);
int a3r_umeyama_moments(const float* x, const float* y, const float* w, const long* x_off, const long* y_off, const long* w_off,
                        int B, int P, double* partial, void* stream);

/* Closed-form weighted similarity registration of B problems from the raw moments of a3r_umeyama_moments (partial [B][nch][17]):
 * out [B][13] = (s, R row-major [9], T [3]) minimising sum w |s R x + T - y|^2 -- 3x3 SVD by Jacobi on the device, one thread per
 * problem (replaces roma.rigid_points_registration, init_im_poses.py:415-418). */
int a3r_umeyama_solve(const double* partial, int nch, int B, float* out, void* stream);
/* Batched camera pose from a world-space point map with known intrinsics (stands in for fast_pnp, init_im_poses.py:442-482; parity
 * unpinned: cv2.solvePnPRansac is stochastic and absent).  desc: B device records of a3r_pnp_desc_bytes() bytes
 * {const float* pts [H,W,3]; const uint8* mask [H,W]; int H, W, step, n; float focal, ppx, ppy, pad} -- the problem uses the n =
 * ceil(H W / step) pixels p * step that the mask keeps.  Closed-form start + `iterations` robust Gauss-Newton steps on the reprojection error
 * (Cauchy weights annealed to 5 px), float64, no host synchronisation.  c2w [B][16] camera-to-world;
 * info [B][4] = (valid, inliers < 5 px in front of the camera, sum of min(e^2, 25 px^2) over the points in front, focal).  work: a3r_pnp_work_bytes(B, n_max). */
size_t a3r_pnp_desc_bytes(void);
int a3r_pnp_chunks(int n_max);
size_t a3r_pnp_work_bytes(int B, int n_max);
int a3r_pnp_solve(const void* desc, int B, int n_max, int iterations, void* work, float* c2w, float* info, void* stream);

/* ---- per-pixel passes of the aligner's construction and of the MST initialisation (csrc/init_maps.hip), so that neither moves
 * the confidences through the host nor depends on which torch kernels happen to be loaded already.
 * a3r_conf_prepare: w_* [E, P] = trf(conf_* [E, P]) with mode 0 log | 1 sqrt | 2 x - 1 | 3 identity (commons.py:42-55; w_i = w_j =
 *   NULL skips it) and edge_mean [2 E] (or NULL): mean(conf_i[e]) at 2 e, mean(conf_j[e]) at 2 e + 1 (commons.py:20-25), float64
 *   sums in a fixed order.  16-byte aligned maps, P % 4 == 0.
 * a3r_im_conf_max: out [N, P] = per-image confidence = max over the edges an image appears in, from 0 (base_opt.py:169-175);
 *   ei / ej: DEVICE int32 [E].
 * a3r_weiszfeld_focal: focal [B] of B point maps [B, H, W, 3], principal point at the centre, `iterations` re-weighting steps
 *   (post_process.py:36-60, 'weiszfeld', 10 iterations in the reference), clipped at 0.
 * a3r_sim3_apply: y [P, 3] = post * (k R x + T) with (s, R row-major, T) = sol[0..12] in DEVICE memory (a row of a3r_umeyama_solve's
 *   output), k = s if with_scale else 1: geotrf(sRT_to_4x4(...), pts) without a host round trip (init_im_poses.py:226-233).
 * a3r_depth_init: depth [N, P] = log of the camera-space depth of scale * pts [N, P, 3] under the world-to-camera matrices w2c
 *   [N, 3, 4] (DEVICE), with log(z <= 0 | nan) -> 0 and log(inf) -> FLT_MAX, i.e. _set_depthmap's .log().nan_to_num(neginf=0)
 *   (init_im_poses.py:116-126).
 * a3r_mask_gt: out [n] (uint8) = x > thr. */
int a3r_conf_prepare(const float* conf_i, const float* conf_j, int E, long P, int mode, float* w_i, float* w_j, float* edge_mean,
                     void* stream);
int a3r_im_conf_max(const float* conf_i, const float* conf_j, const int* ei, const int* ej, int E, int N, long P, float* out,
                    void* stream);
int a3r_weiszfeld_focal(const float* pts3d, int B, int H, int W, int iterations, float* focal, void* stream);
int a3r_sim3_apply(const float* x, const float* sol, int with_scale, float post, float* y, long P, void* stream);
int a3r_depth_init(const float* pts, const float* w2c, float scale, int N, long P, float* depth, void* stream);
int a3r_mask_gt(const float* x, float thr, unsigned char* out, long n, void* stream);

int a3r_upsample2x(const float* x, float* y, int B, int H, int W, int C, int Hc, int Wc, void* stream);
/* the same, written in bf3 form ([B Hc Wc][C/8][3][8] bf16, C % 8 == 0): input of the next conv on the bf3 kernel */
int a3r_upsample2x_bf3(const float* x, void* y3, int B, int H, int W, int C, int Hc, int Wc, void* stream);
/* the same, written in fh2 form ([B Hc Wc][C/8][2][8] fp16 planes of scale * y, C % 8 == 0): input of the next conv on the fh2
 * kernel; scale a power of two, absmax (device, may be NULL) receives max |scale * y| as in a3r_split_fh2 */
int a3r_upsample2x_fh2(const float* x, void* y2, int B, int H, int W, int C, int Hc, int Wc, float scale, unsigned* absmax,
                       void* stream);
/* The residual epilogue of a conv that ran on distinct frames only: c, r0 [U, P, C] fp32 (bias-only conv output and its skip
 * input), p2, s [S, P, C] fp32, map [S] (device) the row of each slot in 0..U-1.  s[b] = c[map[b]] + (r0[map[b]] + p2[b]) -- the
 * RESID2 epilogue's order of additions -- and sr2 [S P, C] = relu(s) * scale in fh2 form, absmax as a3r_split_fh2.  C % 8 == 0,
 * S P < 2^31, 16-byte aligned buffers. */
int a3r_combine_resid_fh2(const float* c, const float* r0, const float* p2, const int32_t* map, float* s, void* sr2, int S, long P,
                          int C, float scale, unsigned* absmax, void* stream);
/* the same with p2 = a3r_upsample2x(x [S, H, W, C], window Hc x Wc) made inside the kernel and never written; P = Hc Wc */
int a3r_upsample2x_combine_fh2(const float* x, const float* c, const float* r0, const int32_t* map, float* s, void* sr2, int S, int H,
                               int W, int C, int Hc, int Wc, float scale, unsigned* absmax, void* stream);
/* The two combine passes with c and r0 in two places (stored head products, a3r_model_set_head_products): src [S] (device) is a
 * signed source per slot -- src[b] >= 0: the blocks at store_c / store_r0 + src[b] * stride floats; src[b] < 0: the blocks ~src[b]
 * of c / r0 [., P, C].  stride >= P C, stride % 4 == 0.  The pair (c, r0) or the pair (store_c, store_r0) may be NULL when src
 * never names it.  Arithmetic, rounding order and statistics are those of the calls above: only where the two loads go differs. */
int a3r_combine_resid_fh2_src(const float* c, const float* r0, const float* store_c, const float* store_r0, long stride,
                              const int32_t* src, const float* p2, float* s, void* sr2, int S, long P, int C, float scale,
                              unsigned* absmax, void* stream);
int a3r_upsample2x_combine_fh2_src(const float* x, const float* c, const float* r0, const float* store_c, const float* store_r0,
                                   long stride, const int32_t* src, float* s, void* sr2, int S, int H, int W, int C, int Hc, int Wc,
                                   float scale, unsigned* absmax, void* stream);
/* The residual add of a linear layer that ran on distinct rows only (the decoder's level 0 and zero-convs, a3r_model_set_dedup_decoder):
 * blocks of N rows of C floats, dst [S] = a[map_a[s]] + b[map_b[s]], or with b NULL dst[s] += a[map_a[s]] in place.  fp32; maps on
 * the device; C % 4 == 0, 16-byte aligned buffers. */
int a3r_gather_add_rows(const float* a, const int32_t* map_a, const float* b, const int32_t* map_b, float* dst, int S, int N, int C,
                        void* stream);
/* The same with the row blocks of a in two places (stored frame products, a3r_model_set_frame_products): src[s] >= 0 is the block
 * at store + src[s] * stride floats, src[s] < 0 the block ~src[s] of fresh [., N, C]; stride >= N C, stride % 4 == 0. */
int a3r_gather_add_rows_src(const float* store, long stride, const float* fresh, const int32_t* src, const float* b, const int32_t* map_b,
                            float* dst, int S, int N, int C, void* stream);
/* (tests) the statistics pass of the storages kept across calls on the words named by site_mask (host, 32 words, bit i = word i):
 * `storage` is laid out as by a3r_model_set_frame_cache for items of words_item and rows of words_rows words; stats[i] is stored
 * with every entry ent[k] >= 0 that the call filled (miss[k] >= 0), then raised to the largest word of the entries it read. */
int a3r_frame_cache_stats_sites(void* storage, size_t bytes, int64_t words_item, int64_t words_rows, const int32_t* ent,
                                const int32_t* miss, int U, unsigned* stats, const uint32_t* site_mask, void* stream);
/* Kernel form behind a3r_upsample2x, a3r_upsample2x_fh2 and a3r_upsample2x_combine_fh2: 2 (default: a thread makes 2 x 2 output
 * pixels from corners fetched once) or 1 (four corners fetched per output pixel); the results are bitwise equal
 * (tests/test_gpu_up2x_forms.py).  Returns the previous form, or a negative error code.  Process-wide; environment A3R_UP_FORM=v1
 * selects form 1 at start-up.  A development switch, not part of the reference's interface. */
int a3r_upsample2x_set_form(int form);

/* last 1x1 conv (128 -> 4) + postprocess (dpt_block.py:329, postprocess.py:10-58):
 * x [P, C] -> pts3d [P, 3] = xyz/max(|xyz|,1e-8)*expm1(|xyz|), conf [P] = 1 + exp(c). */
int a3r_head_final(const float* x, const float* w, const float* b, float* pts3d, float* conf, long P, int C,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * (3) whole-model forward: AsymmetricCroCo3DStereo (dust3r/model.py:65-257)
 */
typedef struct {
    int enc_embed_dim, enc_depth, enc_num_heads;
    int dec_embed_dim, dec_depth, dec_num_heads;
    int mlp_ratio, patch_size;
    float rope_base;
    int feature_dim, last_dim;
    int layer_dims[4];
} a3r_model_config;

typedef struct a3r_model_s* a3r_model_t;

int a3r_model_create(const a3r_model_config* cfg, a3r_model_t* out);
int a3r_model_destroy(a3r_model_t m);
/* Register one checkpoint tensor by its state-dict name (reference layout, device pointer, fp32).
 * The pointer must stay valid for the lifetime of the handle. */
int a3r_model_set_weight(a3r_model_t m, const char* name, const float* ptr, int ndim, const int64_t* shape);
/* Bytes of device memory the caller must provide for repacked conv / fused-projection weights. */
size_t a3r_model_packed_bytes(a3r_model_t m);
/* Checks that every parameter is present, repacks into `packed` (caller-owned, >= packed_bytes). */
int a3r_model_finalize(a3r_model_t m, void* packed, size_t packed_bytes, void* stream);
/* Workspace bytes for a batch of B pairs of H x W images. */
size_t a3r_model_workspace_bytes(a3r_model_t m, int B, int H, int W);
/* One forward over B pairs.  img1/img2 [B,3,H,W]; pd1/pd2 = view['pred_depth'] [B,H,W,3];
 * outputs pts1 [B,H,W,3], conf1 [B,H,W], pts2 (= pts3d_in_other_view), conf2. */
int a3r_model_forward(a3r_model_t m, const float* img1, const float* img2, const float* pd1, const float* pd2,
                      int B, int H, int W, float* pts1, float* conf1, float* pts2, float* conf2,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Encoder feature caching (an algorithmic saving the reference does not have: it re-encodes each frame once per
 * pair, dust3r/inference.py:66 + model.py:165-174, although the encoder output depends on the frame only).
 * a3r_model_encode: B frames img [B,3,H,W] -> enc_norm'd tokens feat_out [B, (H/16)*(W/16), enc_embed_dim].
 * a3r_model_decode: the rest of forward() for B pairs from cached features feat1/feat2 [B, N, enc_embed_dim]
 * (workspace >= a3r_model_workspace_bytes).  encode + decode is bit-identical to a3r_model_forward. */
size_t a3r_model_encode_workspace_bytes(a3r_model_t m, int B, int H, int W);
int a3r_model_encode(a3r_model_t m, const float* img, int B, int H, int W, float* feat_out, void* workspace,
                     size_t workspace_bytes, void* stream);
int a3r_model_decode(a3r_model_t m, const float* feat1, const float* feat2, const float* pd1, const float* pd2, int B,
                     int H, int W, float* pts1, float* conf1, float* pts2, float* conf2, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Duplicate inputs inside one call.  A batch cut from a clip repeats its frames (42 pairs of a 16-frame window graph hold 84 image
 * slots and 16 distinct images), and the encoder and the depth-prior token branch depend on one frame alone.  a3r_model_forward and
 * a3r_model_decode therefore find the slots whose images / pred_depth maps are equal bit for bit (the two kinds independently: a
 * 128-bit content key per slot proposes, a bitwise comparison on the device decides), run those parts once per distinct frame and
 * copy the rows to every slot.  Outputs are bitwise those of the plain plan, the fh2 sites and their scales are the same, and the
 * workspace requirement does not change.  Cost: one small read-back and ONE stream synchronise at the start of the call, and about
 * 100 KB of device and pinned host memory owned by the handle.  A comparison that fails (a key collision) makes the call run the
 * plain plan.  With a tap level set, or with more than 512 pairs in a call, the plain plan runs.
 * mode: 0 = off, 1 = on (the default; the environment variable A3R_DEDUP = 0 / 1 / 2 sets the default of new handles), 2 = on with
 * a constant key, so that the comparison alone decides (debugging).
 * a3r_model_last_dedup: what the last forward / decode did -- distinct images and pred_depth maps among its 2 B slots each (2 B
 * where nothing was merged; decode has no images), and whether a failed comparison sent it to the plain plan. */
int a3r_model_set_dedup(a3r_model_t m, int mode);
int a3r_model_last_dedup(a3r_model_t m, int* n_img_unique, int* n_pd_unique, int* fell_back);
/* The DPT heads' level-0 branch.  Each head reads the enc_norm rows of its side; the adapter, the 4x transposed conv, layer_rn[0] and
 * the two 3x3 convs of refinenet1.resConfUnit1 depend on that frame alone (the pair enters as a residual).  With the fh2 maps (the
 * default arithmetic) a forward or decode call runs them once per DISTINCT frame of the side -- decode finds equal feature rows as
 * forward finds equal images, in the same read-back -- and a combine pass (a3r_combine_resid_fh2, by default folded into the 2x
 * up-sample that produces the residual) adds the pair's residual per slot in the conv epilogue's own order of additions: outputs,
 * fh2 sites, scales and statistics are bitwise the plain plan's, and the workspace requirement does not change.  A side merges when it has fewer distinct frames than slots and its level-0 buffers still
 * fit what the plain plan reserves for them (about 0.69 B distinct frames at most for ViT-L); the two sides decide separately.
 * Dedup mode 0, a failed comparison, a tap level and the bf3 / f32 maps run the plain head.
 * on: 1 (the default; environment variable A3R_DEDUP_HEAD = 0 / 1 for new handles) or 0.
 * a3r_model_last_dedup_sides: distinct frames of side 1 / side 2 of the last forward / decode call (B where they were not looked
 * for), and whether that side's head ran merged. */
int a3r_model_set_dedup_head(a3r_model_t m, int on);
int a3r_model_last_dedup_sides(a3r_model_t m, int* u1, int* u2, int* merged1, int* merged2);
/* The decoder's frame-only work (fh2 GEMM inputs only).  decoder_embed reads one frame's enc_norm
 * rows and the zero-convs read one depth prior's tokens: with merged inputs (a3r_model_set_dedup) they run on the distinct rows
 * with the bias-only epilogue, and a3r_gather_add_rows adds their rows to every slot -- level 0 needs both kinds merged in a
 * forward call, the zero-convs the depth priors (forward and decode).  Block 0 of the two decoders reads one side's level-0 rows
 * alone up to its cross-attention product (norm1, qkv, self-attention, proj, norm2, projq, norm_y, projk/v): in a forward call
 * with both kinds merged it runs that half on each side's distinct (image, prior) entries, Um = max(U_1, U_2) per side (the
 * shorter list padded with copies of its last entry), and the cross-attention reads them through image maps
 * (a3r_attention_fh2_mapped).  It does so when Um < B and B N and Um N are multiples of 256 (N tokens per frame: every batch at
 * 512x384) -- the statistic of a q / k / v projection covers the whole last row tile, and only without a partial one is it the
 * plain plan's bit for bit -- and not with attention kernel form 1.  Outputs, fh2 sites, scales
 * and statistics are bitwise the plain plan's and the workspace requirement does not change.
 * on: 1 (the default; environment variable A3R_DEDUP_DEC = 0 / 1 for new handles) or 0. */
int a3r_model_set_dedup_decoder(a3r_model_t m, int on);
/* a3r_model_last_dedup_entries: distinct (image, depth prior) entries of side 1 / side 2 of the last forward call (B where they
 * were not looked for), and whether decoder block 0 ran its frame-only half on them. */
int a3r_model_last_dedup_entries(a3r_model_t m, int* u1, int* u2, int* merged);
/* Frames kept ACROSS calls.  Consecutive calls on one clip repeat their frames (a window graph cut into calls of 16 or more pairs),
 * and a frame's enc_norm rows depend on that frame alone.  With storage installed, a3r_model_forward looks every distinct image of
 * the call up among the frames the handle has stored -- on the device, in the same read-back and behind the same single
 * synchronise as the duplicate search: the 128-bit key proposes, a comparison of every bit with the stored copy of the image
 * decides, so a frame is only ever taken for itself -- encodes the images it did not find, and copies the rows of the others from
 * the storage.  Outputs are bitwise those of a handle without storage; sites, scales and the workspace requirement do not change.
 * The encoder sites' statistics words are those of the frames encoded in this call, raised to the words stored with the entries it
 * read (the words of the call that encoded them): the first call's words exactly when a batch repeats, an upper bound otherwise.
 * Storage: `frames` entries of a3r_model_frame_cache_bytes(m, H, W, frames) bytes together (0 for a bad argument; at most 256
 * entries), each the image, its rows, the key and 8 KB of words; buf is device memory, 256-byte aligned, and stays the caller's.
 * buf == NULL or bytes == 0 removes it.  Storage too small for one entry of the smallest image is refused; a forward at a resolution
 * of which the storage holds no entry fails with A3R_EINVAL before it writes anything.  The least recently used entry makes room,
 * never one the same call reads; a call with more new frames than entries stores the first ones.
 * The entries are dropped by a3r_model_set_weight, a3r_model_finalize, a3r_model_reset_ranges, a3r_model_range_check when it
 * adjusts a site or finds a non-finite word, a change of the dedup mode, a call at another resolution and a failed call (the
 * arithmetic mode is fixed when the handle is created).  A call runs as if there were no storage, and leaves it alone, with dedup mode 0, a tap level,
 * more than 512 pairs, a failed comparison among the call's own slots, or encoder widths whose rows do not fit the buffers they wait
 * in (enc_embed_dim > 3 dec_embed_dim).  a3r_model_decode and a3r_model_encode do not use it.
 * a3r_model_last_frame_cache: distinct images of the last forward found / not found in the storage, and entries it replaced (all 0
 * when the call did not use the storage). */
size_t a3r_model_frame_cache_bytes(a3r_model_t m, int H, int W, int frames);
int a3r_model_set_frame_cache(a3r_model_t m, void* buf, size_t bytes);
int a3r_model_last_frame_cache(a3r_model_t m, int* hits, int* misses, int* evictions);
/* Frame products kept across calls: a second, optional storage beside the frame cache for what the plan makes from one pred_depth
 * map alone -- patch_embed_point_cloud, the dec_blocks_pc blocks and the zero-convs.  Per entry it holds the map (3 H W floats), the
 * zero-conv outputs z_0 .. z_n ((dec_depth / 2 - 1) N dec_embed_dim floats), the key and 8 KB of words: about 14 MB at 512 x 384.
 * With it, a3r_model_forward looks every distinct pred_depth map of the call up as it does the images (key, then every bit; same
 * read-back, same synchronise), runs the branch on the maps it did not find, stores their z rows, and the decoder's gather-add
 * passes read every slot's z rows where they lie.  A call that finds all of its maps launches nothing of the branch.  Outputs are
 * bitwise those of a handle without storage; sites, scales and the workspace requirement do not change; the branch's statistics
 * words follow the frame cache's rule.
 * The storage is used only while a frame cache is installed and it has room for as many entries as that has at the call's
 * resolution (a3r_model_frame_products_bytes(m, H, W, frames) with the same `frames`); a smaller one is ignored.  It has a table
 * and a least-recently-used order of its own, is dropped and bypassed exactly where the frame cache is, and is not used outside
 * the default fh2 arithmetic.  a3r_model_set_dedup_decoder does not concern it: stored maps take the zero-convs' gather-add form
 * in either setting, so that both settings read the same stored words.  buf: device memory, 256-byte aligned, the caller's; NULL
 * or bytes == 0 removes it.
 * a3r_model_last_frame_products: distinct pred_depth maps of the last forward found / not found, and entries replaced (all 0 when
 * the call did not use the storage). */
size_t a3r_model_frame_products_bytes(a3r_model_t m, int H, int W, int frames);
int a3r_model_set_frame_products(a3r_model_t m, void* buf, size_t bytes);
int a3r_model_last_frame_products(a3r_model_t m, int* hits, int* misses, int* evictions);
/* Head products kept across calls: a third, optional storage, indexed by the FRAME CACHE's entries, for what the DPT head of a
 * side makes from one frame alone -- the level-0 branch of a3r_model_set_dedup_head: adapter, 4x transposed conv, layer_rn[0] and
 * the two convs of refinenet1.resConfUnit1.  Per entry and side it holds r0 (the output of layer_rn[0]) and c (the bias-only output
 * of the second conv), [16 N, feature_dim] fp32 each, and 4 KB of words: 50.3 MB per entry at 512 x 384 with ViT-L heads.  It has no
 * lookup of its own -- the image lookup already says which entry a distinct image is -- and the handle keeps one valid bit per
 * (entry, side), cleared when the frame cache fills or replaces the entry.  A side whose head merges (the admission rule of
 * a3r_model_set_dedup_head, unchanged, as is a3r_model_last_dedup_sides) runs the branch on those of its distinct frames whose bit
 * is not set, stores their r0 and c where the frame has an entry, and the combine pass reads every slot's c and r0 where they lie:
 * nothing stored is copied.  A side whose every frame is stored launches nothing of the branch.  A side that does not merge neither
 * reads nor writes the storage.  Outputs are bitwise those of a handle without it; sites, scales and the workspace requirement do
 * not change; the branch's statistics words follow the frame cache's rule, with words of their own per (entry, side).
 * The storage is used only while a frame cache is installed and it has room for as many entries as that has at the call's
 * resolution (a3r_model_head_products_bytes(m, H, W, frames) with the same `frames`); a smaller one is ignored and never written.
 * It is dropped and bypassed exactly where the frame cache is, not used outside the default fh2 arithmetic, and not used by
 * a3r_model_decode.  buf: device memory, 256-byte aligned, the caller's; NULL or bytes == 0 removes it.
 * a3r_model_last_head_products: per side s, hits[s] / misses[s] = distinct frames of the side's head in the last forward that were
 * stored / were computed (both 0 for a side that did not use the storage). */
size_t a3r_model_head_products_bytes(a3r_model_t m, int H, int W, int frames);
int a3r_model_set_head_products(a3r_model_t m, void* buf, size_t bytes);
int a3r_model_last_head_products(a3r_model_t m, int hits[2], int misses[2]);
/* Debug taps for the parity tests: intermediate tensors inside the workspace after a forward; returns device pointer + element
 * count.  name: "feat" (enc_norm output, model.py:163), "hook_a" / "hook_b" (the decoder levels the DPT head reads,
 * dpt_head.py:101), "dec_last" (dec_norm output, model.py:231-232); after a3r_model_set_tap_level(m, L > 0) also "level" (the two
 * decoders' outputs of block L incl. the zero-conv add, model.py:218-228) and "pc0" (patch_embed_point_cloud output,
 * model.py:244-248) -- two more [2 B N, dec_embed_dim] buffers in the workspace (a3r_model_workspace_bytes accounts for them). */
int a3r_model_set_tap_level(a3r_model_t m, int level);
int a3r_model_tap(a3r_model_t m, const char* name, const float** ptr, size_t* count);

/* Range control of the default (fh2) arithmetic.  The reference computes in fp32 (croco.py:13 even allows TF32) and has no
 * activation range limit; two fp16 planes do: a tensor is fp32-grade only while its largest |scale * x| lies in [2^-2, 2^15]
 * (csrc/fh2.h).  Every site of the launch plan that writes an fh2 tensor therefore carries its own power-of-two scale (initially 1)
 * and records max |scale * x| during a3r_model_forward / _encode / _decode.  a3r_model_range_check waits for `stream`, reads the
 * statistics of the LAST such call, and gives every site whose maximum left the band (or was not finite) a new scale that puts it at
 * [2^11, 2^12).  *n_adjusted = number of sites changed; *n_nonfinite = sites whose maximum was Inf / NaN (their own scale cannot be
 * derived until the upstream overflow is gone).  When either is non-zero the outputs of that call are NOT fp32-grade (an overflow
 * makes them Inf / NaN) and the call must be repeated -- the scales persist in the handle, so a checkpoint with large activations
 * pays this once.  With both zero the outputs are final.  Modes other than fh2 (A3R_GEMM=f32|bf3|...) have fp32 range: always 0.
 * a3r_model_reset_ranges puts every scale back to 1. */
int a3r_model_range_check(a3r_model_t m, void* stream, int* n_adjusted, int* n_nonfinite);
int a3r_model_reset_ranges(a3r_model_t m);
/* (diagnostic) max |scale * x| every site of the LAST forward / encode / decode call recorded, in plan order (waits for `stream`);
 * 0 = all-zero tensor or a site that did not run. */
int a3r_model_range_stats(a3r_model_t m, void* stream, float* stored_absmax, int capacity, int* n_sites);
/* (diagnostic) the current scales of plan `phase` (0 = forward, 1 = encode, 2 = decode), in plan order: *n_sites = their number,
 * the first min(capacity, *n_sites) are copied to scales (host). */
int a3r_model_range_scales(a3r_model_t m, int phase, float* scales, int capacity, int* n_sites);

/* ------------------------------------------------------------------------------------------------
 * (3b) RAFT2 ("SEA-RAFT") optical flow: the flow provider of cloud_opt_flow (dust3r/cloud_opt_flow/optimizer.py:118-154 ->
 *      third_party/raft.py:39-73 -> third_party/RAFT/core/raft.py:152-246), csrc/raft.hip.
 *      Weights: the reference's state_dict names with evaluation-mode BatchNorm folded into the convolution in front of it, the
 *      ConvNeXt layer scale `gamma` folded into pwconv2, the factor 0.25 of raft.py:216 folded into upsample_weight.2, and
 *      update_block.encoder.convc1's input channels zero-padded to a3r_raft_corr_width (a multiple of 32; align3r_amd/raft.py
 *      engine_weights does all four).  Every weight the network reads is bound by a3r_raft_finalize: an incomplete set is reported
 *      there (A3R_ESTATE, A3R_EINVAL for a wrong shape, the weight's name in a3r_last_error), never by a forward.
 */
typedef struct {
    int initial_dim;       /* 64 */
    int block_dims[3];     /* 64, 128, 256 */
    int n_blocks[3];       /* 3, 4, 6 ('resnet34', extractor.py:286) */
    int dim;               /* 128: hidden = context = dim, feature maps 2 dim */
    int radius;            /* 4 */
    int corr_levels;       /* 4 (raft.py:159) */
    int num_blocks;        /* 2 ConvNeXt refinement blocks */
} a3r_raft_config;
typedef struct a3r_raft_s* a3r_raft_t;
/* optional copies of intermediates for the parity tests (device pointers or NULL), channels-last, h = H / 8, w = W / 8 */
typedef struct {
    float* cnet;           /* [B, h, w, 2 dim]  init_conv(cnet(cat(image1, image2)))           raft.py:207-209 */
    float* fmap;           /* [2 B, h, w, 2 dim] fnet(image1) then fnet(image2)                  raft.py:222-223 */
    float* corr_pyr[4];    /* [B h w, h_l, w_l]  the correlation pyramid                         corr.py:17-23 */
    float* flow_update0;   /* [B, h, w, 6]       flow_head(net) before the first iteration       raft.py:213 */
    float* weight0;        /* [B, h, w, 576]     .25 * upsample_weight(net), same point          raft.py:214 */
    float* lookup0;        /* [B, h, w, ceil32(levels (2r+1)^2)] the first correlation lookup    raft.py:228 */
    float* motion0;        /* [B, h, w, dim]     BasicMotionEncoder2's output, first iteration   update.py:108-117 */
    float* net[4];         /* [B, h, w, dim]     hidden state after iterations 0..3 */
    float* flow8[4];       /* [B, h, w, 2]       coarse flow after iterations 0..3 */
} a3r_raft_taps;
int a3r_raft_create(const a3r_raft_config* cfg, a3r_raft_t* out);
int a3r_raft_destroy(a3r_raft_t m);
int a3r_raft_set_weight(a3r_raft_t m, const char* name, const float* ptr, int ndim, const int64_t* shape);
size_t a3r_raft_packed_bytes(a3r_raft_t m);
/* input channels of update_block.encoder.convc1 as the library takes it: corr_levels (2 radius + 1)^2 rounded up to a multiple of 32 */
int a3r_raft_corr_width(a3r_raft_t m);
int a3r_raft_finalize(a3r_raft_t m, void* packed, size_t packed_bytes, void* stream);
size_t a3r_raft_workspace_bytes(a3r_raft_t m, int B, int H, int W);
/* flow [B, 2, H, W] = RAFT2(image1, image2, iters, test_mode=True)[1]: image* [B, 3, H, W] with values in [0, 255] (the reference
 * feeds img * 255, optimizer.py:141-146); H, W multiples of 8 (the reference pads to that with InputPadder) and at least
 * 16 << (corr_levels - 1) (its pyramid needs it, corr.py:22). */
int a3r_raft_forward(a3r_raft_t m, const float* image1, const float* image2, int B, int H, int W, int iters, float* flow,
                     void* workspace, size_t workspace_bytes, const a3r_raft_taps* taps, void* stream);
/* Arithmetic of the flow network's convolutions / linear layers / correlation: 1 (default) = the two-plane fp16 form (fh2 kernels: three
 * fp16 MFMA passes, operands stored with scale 1), 0 = the three-plane bf16 form (six passes, fp32 range).  The fh2 form is fp32-grade
 * while every stored activation stays inside fp16's range; every fh2 producer of a call reports max |stored value| into one device
 * word that a3r_raft_range reads back (it waits for the stream): a caller that finds it at or above 2^15 (or NaN) repeats the call
 * after a3r_raft_set_arith(m, 0) -- align3r_amd.raft.RaftEngine does.  set_arith returns the previous setting.
 * The one activation without a fixed magnitude, the feature map (the correlation's operands fmap1 / sqrt(dim) and fmap2), is stored per
 * image with the power of two that puts that image's max |x| into [2^12, 2^13): the forward reads the per-image maxima back (one wait
 * on the stream), so small or large feature maps cost neither accuracy nor a repeat (absolute error <= 2^-37 max|x| per operand). */
int a3r_raft_set_arith(a3r_raft_t m, int fh2);
int a3r_raft_range(a3r_raft_t m, float* max_abs_host, void* stream);
/* The feature network alone: fmap [B, H/8, W/8, 2 dim] = fnet(2 image / 255 - 1) for B frames (raft.py:222-223).  A frame's features do
 * not depend on the pair it appears in: the reference's cloud_opt_flow re-encodes every frame for every edge and direction
 * (optimizer.py:141-146); computing them once per frame and passing them to a3r_raft_forward_features gives the same flow with a
 * third fewer FLOPs.  workspace: a3r_raft_workspace_bytes(m, B, H, W) is sufficient. */
int a3r_raft_encode(a3r_raft_t m, const float* image, int B, int H, int W, float* fmap, void* workspace, size_t workspace_bytes, void* stream);
/* a3r_raft_forward with the two feature maps given (fmap1 / fmap2 [B, H/8, W/8, 2 dim] from a3r_raft_encode of image1 / image2). */
int a3r_raft_forward_features(a3r_raft_t m, const float* image1, const float* image2, const float* fmap1, const float* fmap2, int B, int H,
                              int W, int iters, float* flow, void* workspace, size_t workspace_bytes, void* stream);

/* (3c) The flow network's kernels that have no GEMM shape, one by one (csrc/raft.hip): each entry goes through the launcher the plan
 *      of a3r_raft_forward uses, so its grid is production's.  Maps are channels-last fp32 unless said otherwise; every buffer is the
 *      caller's; nothing waits for the stream.  Dimensions must be positive with a product below 2^31. */
/* 7x7 convolution, padding 3, stride 2, of image planes: x0 (and x1 unless NULL, concatenated along channels, raft.py:207), each
 * [B, c, H, W] with c in 1..3, every element entering as x * in_mul + in_add (raft.py:194-195) -> y [B, Ho, Wo, Cout], Ho = (H - 1) / 2
 * + 1.  w: [Cout, Cin, 7, 7] as PyTorch stores it (Cin = c or 2 c); wt: Cout Cin 49 floats of workspace that receive its transpose
 * (as a3r_raft_finalize makes it); bias [Cout] or NULL; relu: clamp at zero.  form: 0 = the kernel the plan chooses, 1 = the generic
 * kernel (what A3R_RAFT_DIRECT_CONV=generic selects for a whole process); the two agree bit for bit. */
int a3r_flow_conv7_planes(const float* x0, const float* x1, int c, const float* w, const float* bias, float* wt, float* y, int B, int H,
                          int W, int Cout, float in_mul, float in_add, int relu, int form, void* stream);
/* the same, stride 1, on the channels-last 2-channel coarse flow [B, h, w, 2] (update.py:105) -> y [B, h, w, Cout]; w [Cout, 2, 7, 7] */
int a3r_flow_conv7_flow(const float* flow, const float* w, const float* bias, float* wt, float* y, int B, int h, int w_, int Cout, int relu,
                        int form, void* stream);
/* depthwise 7x7, padding 3 (layer.py:52): x, y [B, h, w, C]; w [C, 49] ([C, 1, 7, 7]); wt: 49 C floats of workspace; bias [C] */
int a3r_flow_dwconv7(const float* x, const float* w, const float* bias, float* wt, float* y, int B, int h, int w_, int C, void* stream);
/* y [B, (h - 1) / 2 + 1, (w - 1) / 2 + 1, C] = x [B, h, w, C] at even rows and columns (layer.py:125); C % 4 == 0, 16-byte aligned */
int a3r_flow_gather_s2(const float* x, float* y, int B, int h, int w_, int C, void* stream);
/* y [B, h / 2, w / 2, C] = F.interpolate(x, scale_factor=0.5, mode='bilinear') (corr.py:22): 2x2 means; h, w >= 2 */
int a3r_flow_halve(const float* x, float* y, int B, int h, int w_, int C, void* stream);
/* Correlation lookup (corr.py:25-50, utils.py:76-91): corr[l] [B h w, hl[l], wl[l]] for l < levels (host arrays of `levels` entries;
 * 1..4 levels, each at least 2x2), flow [B, h, w, 2], r in 1..8 -> out [B h w, ldo]: channel l (2r+1)^2 + a (2r+1) + c is level l
 * sampled at ((x + fx) / 2^l + a - r, (y + fy) / 2^l + c - r), zeros outside; columns from levels (2r+1)^2 to ldo are set to zero. */
int a3r_flow_corr_lookup(const float* const* corr, const int* hl, const int* wl, const float* flow, float* out, int ldo, int B, int h, int w_,
                         int r, int levels, void* stream);
/* Convex up-sampling (raft.py:183-199): flow [B, h, w, 2], mask [B, h, w, 576] -> out [B, 2, 8 h, 8 w] (planes) */
int a3r_flow_convex_upsample(const float* flow, const float* mask, float* out, int B, int h, int w_, void* stream);
/* the movers: x[i] *= s (i < n); dst[r, c0 + c] = src[r, c] (c < Cs, r < rows; rows of ldd / lds floats); flow [rows, 2] += upd [rows, ldu]
 * [:, 0:2]; out[i] = bits of max |x| over image i of `images` (<= 65535) images of n_per floats (out is cleared first) */
int a3r_flow_scale(float* x, float s, long n, void* stream);
int a3r_flow_pack_cols(float* dst, int ldd, int c0, const float* src, int lds, int Cs, long rows, void* stream);
int a3r_flow_add(float* flow, const float* upd, int ldu, long rows, void* stream);
int a3r_flow_image_absmax(const float* x, long n_per, int images, unsigned* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (4) global alignment inner loop: PointCloudOptimizer (cloud_opt/optimizer.py, base_opt.py)
 */
typedef struct {
    int E, N, P;                 /* edges, images, max pixels per image */
    int use_mono;                /* depth = mono*exp(scalemap)+shift (optimizer.py:181-185) else exp(log-depth) */
    int norm_pw_scale;           /* base_opt.py:212-218 */
    int dist_l2;                 /* 0 = l1_dist, 1 = l2_dist (commons.py:102-107) */
    int train_poses, train_focals, train_pp;
    float base_scale, pw_break, focal_break;
    double total_area_i, total_area_j;     /* optimizer.py:70-71 */
    /* graph (HOST arrays, copied at create) */
    const int32_t* ei_host;      /* [E] */
    const int32_t* ej_host;      /* [E] */
    const int32_t* imw_host;     /* [N] image widths  */
    const int32_t* imarea_host;  /* [N] h*w; pixels >= imarea are padding (grid 0, weight 0) */
    /* stacked observations (device), optimizer.py:60-67 */
    const float* pred_i;         /* [E, P, 3] */
    const float* pred_j;         /* [E, P, 3] */
    const float* w_i;            /* [E, P] conf_trf(conf) */
    const float* w_j;            /* [E, P] */
    const float* mono;           /* [N, P] or NULL */
    const float* pp0;            /* [N, 2] = (w/2, h/2) */
    /* parameters (device, updated in place) */
    float* pw_poses;             /* [E, 8] quat xyzw, signed_log1p(T), log scale */
    float* pw_adaptors;          /* [E, 2] (frozen: allow_pw_adaptors=False) */
    float* depth;                /* [N, P] log-depth, or scalemap when use_mono */
    float* shifts;               /* [N] (use_mono) */
    float* im_poses;             /* [N, 7] */
    float* im_focals;            /* [N] focal_break*log(f) */
    float* im_pp;                /* [N, 2] */
    /* Adam state (device, zero-initialised by the caller): [m | v] for each parameter, same shapes */
    float* adam_pw_poses;        /* [2, E, 8] */
    float* adam_depth;           /* [2, N, P] */
    float* adam_small;           /* [2, N, 16]: per image (im_poses 7, im_focals 1, im_pp 2, shift 1, pad) */
    /* scratch + outputs (device) */
    void* workspace;             /* >= a3r_align_workspace_bytes(E, N, P) */
    size_t workspace_bytes;
    float* loss_history;         /* [loss_capacity]; entry t = loss of iteration t (before its update) */
    int loss_capacity;
    /* allow_pw_adaptors=True (base_opt.py:117-118,177-182): pw_adaptors [E,2] = (xy, z) log-scale adaptation of each pairwise
     * prediction become trainable: gradient + Adam like every other small parameter.  adam_pw_adaptors [2, E, 2] (zero-initialised)
     * is required when train_adaptors != 0 and ignored otherwise. */
    int train_adaptors;
    float* adam_pw_adaptors;
    /* Storage of the observations.  obs_format = 0 (a zeroed tail: every caller that predates these fields): fp32 in pred_i / pred_j /
     * w_i / w_j, the four pointers below null.  obs_format = 1: packed fp16, half the bytes -- per edge side and pixel one 8-byte record
     * {half(x 2^k), half(y 2^k), half(z 2^k), half(w)} in obs_i / obs_j [E, P] (16-byte aligned) and one exponent k per edge side in
     * obs_exp_i / obs_exp_j [E] int32, as a3r_align_pack_obs writes them; pred_i / pred_j / w_i / w_j must be null and P % 4 == 0.
     * The handle then computes exactly what an fp32 handle computes on the decoded observations float(h) 2^-k, float(h_w): parameters,
     * moments and all arithmetic stay fp32.  Everything else (flow variant, depth prior, train masks, shards) is unchanged. */
    int obs_format;
    const void* obs_i;           /* [E, P] records (device) */
    const void* obs_j;
    const int32_t* obs_exp_i;    /* [E] (device) */
    const int32_t* obs_exp_j;
} a3r_align_desc;

typedef struct a3r_align_s* a3r_align_t;

/* Packs `rows` edge sides of fp32 observations (pred [rows, P, 3], w [rows, P], device) into the obs_format = 1 form: obs [rows, P]
 * 8-byte records, exps [rows] int32.  Per row: m = max |v| over the FINITE components of pred; k = 0 if m == 0 or nothing is finite,
 * else clamp(14 - ilogb(m), -100, 100), which puts the largest finite magnitude into [2^14, 2^15); every value is scaled by 2^k
 * (exact) and rounded to fp16 to nearest-even, the weight is rounded unscaled; non-finite values convert by the IEEE rule.  Decoded,
 * |pred' - pred| <= max(2^-11 |pred|, 2^-25 2^-k).  Deterministic.  Any row range of larger buffers can be passed (offset all four
 * pointers), so a caller can stream chunks through one staging buffer and never hold the whole fp32 stack on the device.
 * obs must be 8-byte aligned; 16-byte loads and stores are used when P % 4 == 0 and pred, w and obs are 16-byte aligned. */
int a3r_align_pack_obs(const float* pred, const float* w, int rows, long P, void* obs, int32_t* exps, void* stream);

size_t a3r_align_workspace_bytes(int E, int N, int P);
int a3r_align_create(const a3r_align_desc* desc, a3r_align_t* out, void* stream);
int a3r_align_destroy(a3r_align_t a);
/* Per-image train masks (ModularPointCloudOptimizer: preset_pose / preset_focal / preset_principal_point on a SUBSET of the images,
 * dust3r/cloud_opt/modular_optimizer.py:73-110).  Each argument is a HOST array of N bytes (non-zero = this image's group is trained,
 * zero = frozen) or NULL (no per-image freeze: the handle-wide train_* switch alone decides, as on a handle that never calls this).
 * A group is updated only where both the switch and the mask allow it.  A frozen entry gets no Adam step and its moments are not
 * touched; a frozen depth map (no counterpart in the reference) is neither read for its moments nor written.  a3r_align_grad*
 * return exact zeros in the rows of frozen groups.  Every call replaces all four masks.  A focal mask is refused with shared_focal,
 * every mask on an edge-shard handle.  Synchronises the stream. */
int a3r_align_set_train_masks(a3r_align_t a, const uint8_t* pose_host, const uint8_t* focal_host, const uint8_t* pp_host,
                              const uint8_t* depth_host, void* stream);
/* One global_alignment_iter (base_opt.py:450-464): loss + gradients + Adam(betas .9,.9, eps 1e-8) with
 * learning rate lr.  Fully asynchronous; the loss lands in loss_history[step]. */
int a3r_align_step(a3r_align_t a, float lr, void* stream);
/* n iterations in one call: lrs_host[k] is the learning rate of iteration k (host array; the caller evaluates its schedule),
 * epochs first_epoch .. first_epoch + n - 1.  Same results as n a3r_align_step_epoch calls, without a host round trip each. */
int a3r_align_run(a3r_align_t a, const float* lrs_host, int n, int first_epoch, void* stream);
/* Loss only (net() without backward), written to *loss_dev (device float). */
int a3r_align_loss(a3r_align_t a, float* loss_dev, void* stream);
/* Gradients of the current state without updating (for the parity tests):
 * g_pw_poses [E,8], g_depth [N,P], g_small [N,16] (layout of adam_small), loss_dev [1]. */
int a3r_align_grad(a3r_align_t a, float* g_pw_poses, float* g_depth, float* g_small, float* loss_dev, void* stream);
/* the same with the gradient of pw_adaptors [E,2] as well (g_pw_adaptors may be NULL); epoch as a3r_align_grad_epoch */
int a3r_align_grad_full(a3r_align_t a, int epoch, float* g_pw_poses, float* g_pw_adaptors, float* g_depth, float* g_small,
                        float* loss_dev, void* stream);
/* cloud_opt_flow variant (dust3r/cloud_opt_flow/optimizer.py:36-116,500-572): shared focal, temporal smoothing of
 * consecutive image poses (relative_pose_loss), ego-flow smooth-L1 term against precomputed optical flow (the RAFT
 * fields and the dynamic masks are INPUTS).  Call once after a3r_align_create (not with use_mono).  With shared_focal
 * im_focals has one element and the Adam moments of the focal live in slot [0][7] of adam_small. */
typedef struct {
    int shared_focal;
    float temporal_smoothing_weight;   /* 0 disables */
    float translation_weight;
    float flow_loss_weight;            /* 0 disables the ego-flow term */
    float flow_loss_thre;              /* > 0: the term is dropped in an iteration whose flow loss exceeds it (optimizer.py:538) */
    float pxl_thre;                    /* per-element threshold of smooth_L1_loss_fn (optimizer.py:18-24) */
    int flow_start_iter;               /* first epoch e with e >= num_total_iter * flow_loss_start_epoch */
    int H, W;                          /* image shape, H*W == P */
    const float* flow_ij;              /* [E, 2, H*W] flow of image ei towards ej (x then y planes), device */
    const float* flow_ji;              /* [E, 2, H*W] */
    const uint8_t* dynamic_mask;       /* [N, H*W], 1 = dynamic pixel (excluded), device */
    void* workspace;                   /* >= a3r_align_flow_workspace_bytes(E, N, P), device */
    size_t workspace_bytes;
} a3r_align_flow_desc;
size_t a3r_align_flow_workspace_bytes(int E, int N, int P);
int a3r_align_set_flow(a3r_align_t a, const a3r_align_flow_desc* f, void* stream);
/* Depth prior of the flow variant: depth_regularize_weight * depth_regularization_si_weighted(depthmaps, init_depthmaps,
 * dynamic_masks) (dust3r/utils/goem_opt.py:15-36 as called at dust3r/cloud_opt_flow/optimizer.py:546-555): a scale-invariant
 * squared log-depth distance to the depth maps captured by _set_init_depthmap (optimizer.py:452-454), pixels of the dynamic
 * mask weighted 2, others 1, averaged over images.  init_log_depth: [N, P] log-depth parameters at capture time, device;
 * dynamic_mask: [N, P] (1 = dynamic) or NULL; both stay owned by the caller and must outlive the handle.  weight == 0 turns
 * the term off (other arguments ignored).  Loss, gradient export and step all include the term afterwards. */
size_t a3r_align_depth_prior_workspace_bytes(int N, int P);
int a3r_align_set_depth_prior(a3r_align_t a, float weight, const float* init_log_depth, const uint8_t* dynamic_mask,
                              void* workspace, size_t workspace_bytes, void* stream);
/* a3r_align_step with an explicit epoch (net(epoch=cur_iter), cloud_opt_flow/base_opt.py:571); a3r_align_step uses
 * the handle's own iteration count. */
int a3r_align_step_epoch(a3r_align_t a, float lr, int epoch, void* stream);
int a3r_align_grad_epoch(a3r_align_t a, int epoch, float* g_pw_poses, float* g_depth, float* g_small, float* loss_dev,
                         void* stream);
/* HOST out[5] = {c_ij, c_ji, last flow loss, dropped in the last evaluation, dropped ever (flow_loss_flag)}; synchronises. */
int a3r_align_flow_state(a3r_align_t a, float* state_host5);
int a3r_align_steps_done(a3r_align_t a);
/* Tell the handle that the caller rewrote parameter buffers (preset_pose, init, load_state_dict ...). */
int a3r_align_invalidate(a3r_align_t a);
/* per-edge [E,3,4] = [s*R*diag(a) | s*T] and per-image [N,3,4] = [R | t] (get_pw_poses/get_im_poses rows 0-2) */
int a3r_align_pose_matrices(a3r_align_t a, float* edge_M, float* img_R, void* stream);

/* Edge-sharded form of the same loop ("option B"): a shard handle owns the observation rows [e0, e1) of a graph
 * with desc->E edges and a full replica of every parameter and Adam moment.  One iteration is
 *     a3r_align_shard_partial   (every shard: loss + gradient sums of its own edges -> one flat fp32 reduce buffer)
 *     sum of the buffers        (one all-reduce(SUM) between ranks, or a3r_align_shard_sum inside one process)
 *     a3r_align_shard_apply     (every shard: chain rules, scale-normalisation coupling and Adam from the REDUCED buffer)
 * Everything in the reduce buffer is additive over edges; every non-linear step runs after the reduction, so the replicas stay
 * identical.  Layout (floats): [N*P rounded up to 4] d loss / d depth parameter, [N][16] per-image sums, [E][16] per-edge sums
 * (12 gradient sums, the loss of the edge, 3 zeros; rows outside [e0, e1) are zero).
 * desc is read as by a3r_align_create, except: pred_i / pred_j / w_i / w_j (with obs_format = 1: obs_i / obs_j / obs_exp_i /
 * obs_exp_j) hold the shard's rows only ([e1 - e0, P, 3] / [e1 - e0, P], row 0 = edge e0); ei_host / ej_host, total_area_i / j and
 * the parameter buffers describe the WHOLE graph; workspace holds
 * a3r_align_shard_workspace_bytes(E, e1 - e0, N, P).  a3r_align_step / _loss / _grad*, a3r_align_set_flow and
 * a3r_align_set_depth_prior refuse a shard handle; destroy, steps_done, invalidate and pose_matrices work on it. */
size_t a3r_align_shard_workspace_bytes(int E, int E_shard, int N, int P);
size_t a3r_align_shard_reduce_floats(int E, int N, int P);
int a3r_align_shard_create(const a3r_align_desc* desc, int e0, int e1, a3r_align_t* out, void* stream);
/* reduce_buf: device, 16-byte aligned, n_floats == a3r_align_shard_reduce_floats(E, N, P); every float is written. */
int a3r_align_shard_partial(a3r_align_t a, float* reduce_buf, size_t n_floats, void* stream);
/* One update from the reduced buffer with learning rate lr; the loss lands in loss_history like a3r_align_step's. */
int a3r_align_shard_apply(a3r_align_t a, const float* reduced, size_t n_floats, float lr, void* stream);
/* Gradients of the small parameters and the loss from the reduced buffer, without updating (layouts of a3r_align_grad_full;
 * g_pw_adaptors may be NULL); the gradient of the depth parameters is the first N*P floats of the reduced buffer itself. */
int a3r_align_shard_grad(a3r_align_t a, const float* reduced, size_t n_floats, float* g_pw_poses, float* g_pw_adaptors,
                         float* g_small, float* loss_dev, void* stream);
/* dst = ((src[0] + src[1]) + src[2]) + ... over K device buffers of n_floats floats (srcs_host: HOST array of K device pointers),
 * always in this order: bitwise reproducible.  dst may be src[0]. */
int a3r_align_shard_sum(float* dst, const float* const* srcs_host, int K, size_t n_floats, void* stream);
/* n iterations of K shard handles of ONE graph living in one process on one device (learning rates as a3r_align_run): per
 * iteration K partials into bufs_host[k], their fixed-order sum into bufs_host[0], K applies. */
int a3r_align_shard_run_local(const a3r_align_t* handles_host, int K, float* const* bufs_host, size_t n_floats,
                              const float* lrs_host, int n, void* stream);

/* Scene out: the aligned scene of a handle as world points (what tool/demo.py's get_3D_model_from_scene assembles from get_pts3d()
 * and get_masks()).  For image n and pixel p < h_n * w_n (x = p % w_n, y = p / w_n):
 *     world = R_n * (d (x - ppx) / f, d (y - ppy) / f, d) + t_n,  d = exp(log_depth) | mono * exp(scalemap) + shift
 * from the handle's CURRENT parameters, decoded as for a3r_align_pose_matrices (shared_focal: the focal of image 0 for all).
 * Fused and edge-shard handles are both accepted (a shard holds a full replica of everything read here).
 *
 * a3r_align_scene_points: dense out_xyz [N,P,3]; the padding pixels p >= h_n * w_n of a mixed-shape scene are written as zeros.
 *
 * Compacted form.  A pixel is kept iff p < h_n * w_n, conf[n,p] > thr (strict), dyn == NULL or dyn[n,p] == 0, and its three world
 * coordinates are finite.  Kept pixels come out image-major, row-major; the result is a deterministic function of the inputs (two
 * passes: per-chunk counts, an exclusive scan, then placement -- no atomics).  All buffers are device memory unless named *_host;
 * workspace: a3r_align_scene_workspace_bytes(N, P) bytes, 4-byte aligned.  Both entry points synchronise the stream (the kept
 * count returns to the host).  N * P must be below 2^31.
 *   a3r_align_scene_count : *total_host = kept pixels of the scene; counts_dev [N] (or NULL) = kept pixels per image.
 *   a3r_align_scene_export: counts afresh, then writes out_xyz [M,3] fp32 and, where non-NULL, out_rgb [M,3] (gathered from
 *     rgb [N,P,3] uint8) and out_index [M] (n * P + p).  *n_written_host = M.  capacity (in points, of every output given) < M is
 *     A3R_EINVAL BEFORE any output element is written, with *n_written_host = the needed count; elements at and beyond M are never
 *     written; M = 0 is a success. */
size_t a3r_align_scene_workspace_bytes(int N, int P);
int a3r_align_scene_points(a3r_align_t a, float* out_xyz, void* stream);
int a3r_align_scene_count(a3r_align_t a, const float* conf, float thr, const uint8_t* dyn, void* workspace, size_t workspace_bytes,
                          int* counts_dev, long long* total_host, void* stream);
int a3r_align_scene_export(a3r_align_t a, const float* conf, float thr, const uint8_t* dyn, const uint8_t* rgb, void* workspace,
                           size_t workspace_bytes, long long capacity, float* out_xyz, uint8_t* out_rgb, int* out_index,
                           long long* n_written_host, void* stream);

/* Scene out as a triangle mesh (pts3d_to_trimesh / cat_meshes of dust3r/viz.py, the default form of get_3D_model_from_scene), with
 * the inputs and the kept rule of a3r_align_scene_export.
 *   Vertices: the kept pixels, image-major and row-major -- bitwise the out_xyz / out_rgb of a3r_align_scene_export on the same
 *     inputs.  A vertex's id is its rank in that order; kept pixels that end up in no triangle stay in the list.
 *   Quads: for image n of shape (h, w) every (y, x), 0 <= y < h - 1, 0 <= x < w - 1, row-major, with the corners tl = (y, x),
 *     tr = (y, x + 1), bl = (y + 1, x), br = (y + 1, x + 1) (each image's own w; no quad wraps from the end of a row to the next).
 *     Triangle A = (tl, tr, bl) exists iff those three pixels are kept, its colour is rgb[tl];
 *     triangle B = (tr, bl, br) exists iff those three pixels are kept, its colour is rgb[br].
 *   Face order: images in order; inside an image with double_sided = 0 all existing A (quad order), then all existing B; with
 *     double_sided = 1 the reference's [A, A', B, B'], A' = (bl, tr, tl) and B' = (br, bl, tr) being the same triangles wound
 *     backwards, each block in quad order, with the colours of A and B.
 *   out_faces [F,3] int32 vertex ids, out_face_rgb [F,3] uint8.  cat_meshes([pts3d_to_trimesh(img_n, pts_n, kept_n)]) indexes the
 *     dense grids (image offsets = cumulative h * w); this mesh is that one with every index replaced by the pixel's rank among the
 *     kept pixels.
 * Passes, no atomics (the output is a function of the inputs alone): per-chunk vertex counts + a rank map (rank inside the chunk,
 * -1 = dropped), scan, per-chunk face counts from the rank map alone, scan, vertex placement, face placement.
 * workspace: a3r_align_scene_mesh_workspace_bytes(N, P) bytes, 16-byte aligned (vertex offsets, face offsets, rank map [N,P] int32).
 * Both entry points synchronise the stream (the counts return to the host).  N * P and the face bound 2 * N * P (double_sided:
 * 4 * N * P) must be below 2^31.
 *   a3r_align_scene_mesh_count : *n_vertices_host = V, *n_faces_host = F.
 *   a3r_align_scene_mesh_export: counts afresh, then writes out_xyz [V,3], out_faces [F,3] and, where non-NULL, out_vertex_rgb [V,3]
 *     and out_face_rgb [F,3] (both need rgb).  A3R_EINVAL BEFORE any output element is written: a null handle, conf or workspace, a
 *     workspace that is too small or misaligned, a colour output without rgb, vertex_capacity < V or face_capacity < F (the needed
 *     counts are still returned), totals that do not fit.  Elements at and beyond V / F are never written; V = 0 and F = 0 are
 *     successes. */
size_t a3r_align_scene_mesh_workspace_bytes(int N, int P);
int a3r_align_scene_mesh_count(a3r_align_t a, const float* conf, float thr, const uint8_t* dyn, void* workspace, size_t workspace_bytes,
                               int double_sided, long long* n_vertices_host, long long* n_faces_host, void* stream);
int a3r_align_scene_mesh_export(a3r_align_t a, const float* conf, float thr, const uint8_t* dyn, const uint8_t* rgb, void* workspace,
                                size_t workspace_bytes, int double_sided, long long vertex_capacity, long long face_capacity,
                                float* out_xyz, uint8_t* out_vertex_rgb, int* out_faces, uint8_t* out_face_rgb,
                                long long* n_vertices_host, long long* n_faces_host, void* stream);

/* clean_pointcloud (cloud_opt/base_opt.py:468-503) on the handle's CURRENT state: conf [N,P] fp32 (device) is updated in place, as if
 * the images were processed in order i = 0 .. N-1 and, for every pixel p < h_i * w_i of image i, the other views j in increasing order:
 *     (cx, cy, z) = R_j^T (world(i,p) - t_j);  u = rint(f_j cx / z + ppx_j), v = rint(f_j cy / z + ppy_j)   (half to even)
 *     visible  iff z > 0, 0 <= u < w_j, 0 <= v < h_j, everything finite (a non-finite value is "not visible", never an index)
 *     bad      iff visible, z < (1 - tol) * depth_j[v,u] and conf[i,p] < conf[j, v * w_j + u]                (both strict)
 *     bad  =>  conf[i,p] = min(conf[i,p], bad_conf)
 * The rows j < i are read as FINISHED, the rows j > i as given.  Padding entries p >= h_i * w_i and NaN confidences are never
 * written; padding pixels of image j are never visible.  One small preparation kernel and N kernels in stream order (image i writes
 * row i only and reads the other rows), no atomics: the result is a function of the inputs alone.  Nothing is allocated,
 * synchronised or read back, so the call can be captured into a graph.  workspace: a3r_align_scene_clean_workspace_bytes(N, P)
 * bytes, 16-byte aligned (a world-to-camera table and the dense depth maps).  A3R_EINVAL before conf is touched: null conf, a
 * workspace that is too small or misaligned, tol outside [0, 1) or NaN, bad_conf NaN. */
size_t a3r_align_scene_clean_workspace_bytes(int N, int P);
int a3r_align_scene_clean(a3r_align_t a, float* conf, float tol, float bad_conf, void* workspace, size_t workspace_bytes, void* stream);

/* Self-computed motion masks of the flow aligner (dust3r/cloud_opt_flow/optimizer.py:201-235): everything after the pair geometry of
 * get_motion_mask_from_pairs.  M symmetric pairs give 2M DIRECTED entries; entry k compares the ego flow its pair geometry implies
 * with one optical-flow field and votes for one image.  Per entry and pixel (x, y), fp32, in this order of operations:
 *     D = r . pt + t;  disp = 1 / (D + 1e-6);  tgt = Hm (x, y, 1) + disp * Kt;  tgt /= tgt_z + 1e-6;
 *     err = | tgt_xy - (x, y) - flow(x, y) |
 * per entry nerr = (err - min) / (max - min) over the whole map; per image the mean of its entries' nerr in list order;
 * masks = mean > motion_mask_thre.  IEEE as torch evaluates it: a NaN anywhere in an entry's map, or a constant map (0 / 0), makes
 * that entry's contribution NaN at every pixel, and every image it votes for gets an all-false mask and a NaN mean.
 * Three kernels in stream order, no atomics, fixed-order reductions: the result is a function of the inputs alone.  Nothing is
 * allocated, synchronised or read back, so the call can be captured into a graph. */
typedef struct {
    int depth_row;       /* row of the stacked pointmaps that supplies the depth: [0, E) = pred_i, [E, 2E) = pred_j[row - E] */
    int flow_row;        /* [0, E) = flow_ij, [E, 2E) = flow_ji[row - E] */
    int image;           /* the image this entry votes for (must agree with the lists below) */
    int pad;
    float depth_rt[4];   /* (r, t): D = r . pt + t; (0,0,1,0) = z of the pointmap, or the third row of inv(rel_pose) */
    float Hm[9];         /* K_tgt R_rel K_src^-1, row-major */
    float Kt[3];         /* K_tgt t_rel */
} a3r_motion_entry;
typedef struct {
    int M, N, E;                        /* symmetric pairs, images, rows of the stacked buffers */
    int H, W;                           /* one image shape, P = H * W */
    float motion_mask_thre;
    const float* pred_i;                /* [E, P, 3] device */
    const float* pred_j;                /* [E, P, 3] device */
    const float* flow_ij;               /* [E, 2, H, W] device */
    const float* flow_ji;               /* [E, 2, H, W] device */
    const a3r_motion_entry* entries;    /* [2M] device */
    const a3r_motion_entry* entries_host; /* the same table in host memory: validated before anything is launched */
    const int* list_start;              /* [N + 1] device: image n owns list_entry[list_start[n] .. list_start[n + 1]) */
    const int* list_start_host;
    const int* list_entry;              /* [list_start[N]] device: entry indices, per image in the order their errors are averaged */
    const int* list_entry_host;
} a3r_motion_desc;
/* workspace: a3r_motion_workspace_bytes(M, N, P) bytes, 16-byte aligned (the error maps [2M, P], per-chunk and per-entry min / max).
 * masks [N, P] bytes 0 / 1; mean_err [N, P] fp32 or NULL.  A3R_EINVAL before anything is written: a null pointer, a workspace that
 * is too small or misaligned, M, N, E, H or W <= 0, an image with an empty list, a table or list index out of range, NaN thre. */
size_t a3r_motion_workspace_bytes(int M, int N, int P);
int a3r_motion_masks(const a3r_motion_desc* d, void* ws, size_t ws_bytes, unsigned char* masks, float* mean_err, void* stream);

/* Input preprocessing (dust3r/utils/image_pose.py: pixel_to_pointcloud, normalize_pointcloud, cv2_resize, crop_center, ImgNorm): the
 * mono-depth prior becomes the point map the network reads, with the same numbers as the host path.  Per depth pixel, float64 with
 * every operation rounded on its own:  x = f32(((px - Ws/2) * d) / f),  y = f32(((py - Hs/2) * d) / f),  z = d;  per channel
 * n = (v - min) / (max - min) in float32 over the whole map (a NaN anywhere makes the channel's min and max NaN, a constant channel
 * gives 0 / 0);  then the separable resample  acc = acc + v_k * w_k, k = 0 .. taps - 1, in float64 from acc = 0: horizontally into a
 * float64 intermediate, vertically with one final rounding to float32.  The tables are the host's: per output column (row) `taps`
 * clipped source indices and float64 weights, taps = 8 (Lanczos-4) or 4 (cubic).  Only the crop window (y0, x0, Hc, Wc) of the
 * resized Hr x Wr map is computed.  No atomics, fixed-order reductions: the result is a function of the inputs alone.  Nothing is
 * allocated, synchronised or read back, so the calls can be captured into a graph. */
typedef struct {
    int Hs, Ws;                 /* source rows and columns */
    int Hr, Wr;                 /* the resized map: rows of the y tables and of the x tables */
    int taps;                   /* 8 or 4 */
    int y0, x0, Hc, Wc;         /* the window of the resized map that is written: out [Hc, Wc, 3] */
    const int* idx_x;           /* [Wr, taps] device, 16-byte aligned: source columns in [0, Ws) */
    const int* idx_x_host;      /* the same table in host memory: validated before anything is launched */
    const double* w_x;          /* [Wr, taps] device, 16-byte aligned */
    const int* idx_y;           /* [Hr, taps] device, 16-byte aligned: source rows in [0, Hs) */
    const int* idx_y_host;
    const double* w_y;          /* [Hr, taps] device, 16-byte aligned */
} a3r_prep_desc;
/* workspace: a3r_prep_workspace_bytes(Hs, Ws, Wc) bytes, 16-byte aligned (the float64 intermediate [Hs, Wc, 3], the per-chunk and the
 * final min / max); 0 for an empty size.  a3r_prep_pointmap: depth [Hs, Ws] float32 -> out [Hc, Wc, 3] float32 (four kernels).
 * a3r_prep_resize3: the resample alone on a float32 [Hs, Ws, 3] map (two kernels).  A3R_EINVAL before anything is launched: a null
 * pointer, a workspace that is too small or misaligned, a non-positive size, taps other than 4 or 8, a crop window outside the resized
 * map, a focal that is zero or not finite, an index-table entry outside its range, misaligned device tables.
 * a3r_prep_image: u8 [H, W, 3] -> img [3, H, W] = (u / 255 - 0.5) / 0.5 and mask [H, W] bytes 0 / 1 = ((c0/255 + c1/255) + c2/255) > 0.01,
 * written as !(sum <= 0.01) (one kernel). */
size_t a3r_prep_workspace_bytes(int Hs, int Ws, int Wc);
int a3r_prep_pointmap(const float* depth, double focal, const a3r_prep_desc* d, void* ws, size_t ws_bytes, float* out, void* stream);
int a3r_prep_resize3(const float* src, const a3r_prep_desc* d, void* ws, size_t ws_bytes, float* out, void* stream);
int a3r_prep_image(const unsigned char* u8, int H, int W, float* img, unsigned char* mask, void* stream);

/* Video-depth evaluation (tool/depth_metrics.py; the reference's tool/depth_test.py:689-835) on the device: ONE scale and shift for
 * the whole clip, a clip to [1e-5, depth_max], AbsRel / SqRel / RMSE / logRMSE / delta.  pred, gt: float32 device buffers of n =
 * T * H * W elements; a pixel is valid iff 1e-3 < gt < depth_max (both strict, so a NaN gt is invalid); every sum is float64 over
 * the float32 inputs.  Streaming reductions with per-workgroup partials folded in a fixed order by one workgroup: no floating-point
 * atomics, the same call twice gives the same bits.  16-byte loads when pred and gt are both 16-byte aligned, scalar loads otherwise.
 * Both calls only enqueue on `stream`: nothing is allocated, synchronised or read back.
 * a3r_depth_align writes st_dev = (scale, shift) and info_dev [A3R_DEPTH_INFO_DOUBLES]:
 *   [0] n_valid   [1] sum |s p + t - g| at (scale, shift)   [2] passes over the data of the solve   [3] enlargements of the LAD start region
 *   [4] [5] the two middle order statistics of the valid pred (equal for an odd count)   [6] [7] those of the valid gt   [8] median pred
 *   [9] median gt   [10] [11] the LAD normalisation (s0, T): the search runs on (s / s0, t / T)
 * With fewer than 2 valid pixels scale = shift = NaN and info[0] says why.  Modes: LAD (least absolute deviations scale + shift, central-cut
 * ellipsoid method driven by a one-wave kernel), LSTSQ (least squares scale + shift, centred sums), SCALE (mean ratio + 10 IRLS passes,
 * shift 0; the passes amplify rounding about 1e12 times, so this rule adds the valid pixels in order with numpy's summation tree and
 * returns the host's bits; it uses the 8 n bytes of the workspace that hold the compacted maps), MEDIAN (ratio of the medians, shift 0; np.median semantics).
 * a3r_depth_metrics reads (scale, shift) from st_dev and writes out_dev [A3R_DEPTH_METRIC_DOUBLES]: abs_rel, sq_rel, rmse, log_rmse,
 * d1, d2, d3, n_valid (the means are NaN when n_valid = 0).
 * A3R_EINVAL before anything is launched: a null pointer, n <= 0, a depth_max that is not above 1e-3, an unknown mode, a workspace that
 * is too small or not 16-byte aligned. */
#define A3R_DEPTH_ALIGN_LAD 0
#define A3R_DEPTH_ALIGN_LSTSQ 1
#define A3R_DEPTH_ALIGN_SCALE 2
#define A3R_DEPTH_ALIGN_MEDIAN 3
#define A3R_DEPTH_INFO_DOUBLES 16
#define A3R_DEPTH_METRIC_DOUBLES 8
size_t a3r_depth_eval_workspace_bytes(long n);
int a3r_depth_align(const float* pred, const float* gt, long n, double depth_max, int mode, void* workspace, size_t workspace_bytes,
                    double* st_dev, double* info_dev, void* stream);
int a3r_depth_metrics(const float* pred, const float* gt, long n, double depth_max, const double* st_dev, void* workspace,
                      size_t workspace_bytes, double* out_dev, void* stream);

/* Point correspondences (csrc/match.hip): exact 3-D nearest neighbours by brute force and the reciprocity test of
 * find_reciprocal_matches (dust3r/utils/geometry.py:351-367, two KD-trees on the host there).  Points are fp32 [n,3], device memory.
 * For a query q and a data point k, in float64 with every operation rounded on its own (no fused multiply-add):
 *     dx = (double)q.x - (double)data[k].x  (dy, dz likewise);   d2 = (dx * dx + dy * dy) + dz * dz
 *     nn(q) = the SMALLEST k with d2(q, k) = min over { k : d2(q, k) < +inf },   -1 if that set is empty
 * -- what numpy gives with dx*dx + dy*dy + dz*dz on float64 copies and np.argmin's first-minimum rule.  The search starts from
 * (+inf, -1) and compares with a strict <, so a NaN or infinite coordinate, in the query or in the data, never wins and never becomes
 * an index, and an empty data set gives -1 everywhere.
 * Passes, no atomics and no data-dependent control flow (the output is a function of the inputs alone): the data set is cut into
 * `chunks` contiguous index ranges [n_data c / chunks, n_data (c + 1) / chunks) on a second grid axis, each (query, range) leaves one
 * partial (d2, index), and a fold walks a query's partials in ascending range order with the same strict <; the result therefore does
 * not depend on `chunks`.  chunks = 0 lets the library choose (a3r_nn_chunks says what it chose: enough workgroups to fill the device,
 * never more ranges than LDS tiles of data, at most 64); chunks >= 1 forces that many ranges (at most 65535; ranges are empty when
 * chunks > n_data).  It is the tuning knob of the search.
 * workspace: a3r_nn_workspace_bytes(n_query, n_data, chunks) bytes, 16-byte aligned: partial d2 [chunks, n_query] float64, then partial
 * index [chunks, n_query] int32, each rounded up to 256 bytes; 0 bytes (workspace may be NULL) when either size is 0.
 *   a3r_nn_search: out_index [n_query] int32; out_dist2 [n_query] float64 or NULL = the minimum, +inf where the index is -1.  It only
 *     enqueues on `stream`: nothing is allocated, synchronised or read back.
 * Reciprocal matches of (p1 [n1,3], p2 [n2,3]), the reference's contract:
 *     nn2_in_p1[k2] = nn of p2[k2] in p1;   nn1_in_p2[k1] = nn of p1[k1] in p2
 *     reciprocal_in_p2[k2] = (nn2_in_p1[k2] >= 0 and nn1_in_p2[nn2_in_p1[k2]] == k2)
 * The match list is the pairs (nn2_in_p1[k2], k2) of the reciprocal k2 in ascending k2, M of them (flags and per-block counts by wave
 * ballots, an exclusive scan, placement by rank).
 * workspace: a3r_match_workspace_bytes(n1, n2, chunks) bytes, 16-byte aligned: the search partials of the larger direction,
 * nn1_in_p2 [n1] int32, the block offsets; 0 bytes when either size is 0.
 *   a3r_reciprocal_matches: writes nn2_in_p1 [n2], reciprocal_in_p2 [n2] (0 / 1) and, where non-NULL, nn1_in_p2 [n1] and
 *     out_pairs [M,2] int32 (k1, k2).  *n_matches_host = M.  It synchronises the stream once (the count returns to the host); the pairs
 *     are enqueued after that.  With out_pairs given, capacity (in pairs) < M is A3R_EINVAL BEFORE any pair is written, with
 *     *n_matches_host = the needed count and the three other outputs complete; elements at and beyond M are never written; without
 *     out_pairs the capacity is not looked at.  n1 = 0 or n2 = 0 is a success with zero matches (-1 and 0 everywhere).
 * A3R_EINVAL before anything is launched: a null pointer to a non-empty array, a negative size, a size at or above 2^31, chunks
 * outside [0, 65535], a workspace that is too small or misaligned, a negative capacity, a null n_matches_host. */
int a3r_nn_chunks(long long n_query, long long n_data, int chunks);           /* the range count a search uses; 0 for refused arguments */
size_t a3r_nn_workspace_bytes(long long n_query, long long n_data, int chunks);
int a3r_nn_search(const float* query, long long n_query, const float* data, long long n_data, int chunks, void* workspace,
                  size_t workspace_bytes, int* out_index, double* out_dist2, void* stream);
size_t a3r_match_workspace_bytes(long long n1, long long n2, int chunks);
int a3r_reciprocal_matches(const float* p1, long long n1, const float* p2, long long n2, int chunks, void* workspace,
                           size_t workspace_bytes, int* nn2_in_p1, int* nn1_in_p2, unsigned char* reciprocal_in_p2, long long capacity,
                           int* out_pairs, long long* n_matches_host, void* stream);

/* Rendering (csrc/render.hip): a point cloud drawn into the pictures of n_cams pinhole cameras as z-buffered square splats -- what
 * stands in for the reference's interactive scene.show() (dust3r/cloud_opt/base_opt.py) on a machine without a display, and the
 * primitive of occlusion-aware reprojection checks.  The reference has no renderer; this text is the specification.
 * A camera holds a world-to-camera transform [R|t] (w2c: 12 doubles, row-major 3x4) and fx, fy, cx, cy (doubles, no skew).  The other
 * inputs are the image size H x W, an integer radius in [0, 8] and near_z, finite and > 0.  For camera c and point m with fp32
 * coordinates (x, y, z), on float64 copies of the coordinates, every operation rounded on its own (no fused multiply-add):
 *     xc = (R00 * x + R01 * y) + R02 * z + t0          (yc from row 1, zc from row 2 likewise)
 *     u = fx * (xc / zc) + cx,   v = fy * (yc / zc) + cy,   zf = (float)zc
 *     drawn  iff  zc >= near_z, zf is finite, u and v are finite, |u| < 2^30 and |v| < 2^30
 *                 (a NaN or infinite coordinate and a point behind the camera never draw)
 *     col = (int)rint(u), row = (int)rint(v), half to even (as a3r_align_scene_clean rounds)
 *     footprint = every pixel (row + dy, col + dx) with |dx|, |dy| <= radius that lies inside the image
 *     every pixel of the footprint takes the 64-bit key  (bits(zf) << 32) | m
 * A pixel's result is the MINIMUM key over all points: the nearest point and, at equal zf, the lowest point index (zf > 0, so the
 * bits of zf order as zf does).  Outputs:
 *     depth [n_cams,H,W] fp32 = zf of the winner, 0 where nothing landed
 *     index [n_cams,H,W] int32 (or NULL) = the winner's m, -1 where nothing landed
 *     out_rgb [n_cams,H,W,3] uint8 (or NULL; needs rgb [M,3]) = rgb[m] of the winner, `background` where nothing landed
 * Contract: the minimum of integers does not depend on the order of its operands, so the pictures are bitwise reproducible from
 * call to call although the splat runs on atomics, and they are bitwise what numpy's np.minimum.at gives on uint64 keys formed
 * as above (tests/render_cases.py: render_ref).  Leaving out rgb / out_rgb or index changes nothing in the other outputs.
 * Three kernels in stream order: the key planes are filled with all ones, the splat (atomic minimum on unsigned 64-bit words in
 * global memory, one thread per point), the resolve of keys to depth / index / colour.  Nothing is allocated, synchronised or read
 * back, so the call can be captured into a graph.  workspace: a3r_render_workspace_bytes(n_cams, H, W) bytes, 16-byte aligned (the
 * key planes [n_cams,H,W] of 8 bytes; 0 for refused sizes).  cams_dev: the cameras in device memory; cams_host: the same table in
 * host memory, validated before anything is launched.  `stream` is a hipStream_t, passed as void* like everywhere in this header.
 * A3R_EINVAL before anything is launched, naming the argument: a null pointer to a non-empty array (xyz with M > 0, either camera
 * table, depth, the workspace, background with out_rgb), M < 0 or M >= 2^31, n_cams <= 0, a non-positive H or W,
 * n_cams * H * W >= 2^31, radius outside [0, 8], near_z not finite or <= 0, a non-finite camera entry, out_rgb without rgb (M > 0),
 * a workspace that is too small or misaligned.  M = 0 is a success with every pixel empty.
 * a3r_render_set_form: the splat's form, a developer's A/B switch that does not change the pictures (returns the previous value;
 * values outside [0, 7] only query).  Bit 0: a grid axis over the cameras instead of the camera loop inside the thread.  Bit 1:
 * every atomic is issued instead of first reading the pixel's key and skipping the atomic that cannot lower it.  Bit 2: the keys
 * of a footprint are read one pixel at a time instead of nine at a time (no effect with bit 1 or at radius 0).  Default 0. */
typedef struct { double w2c[12]; double fx, fy, cx, cy; } a3r_render_cam;
size_t a3r_render_workspace_bytes(int n_cams, int H, int W);
int a3r_render_points(const float* xyz, const unsigned char* rgb, long long M, const a3r_render_cam* cams_dev,
                      const a3r_render_cam* cams_host, int n_cams, int H, int W, int radius, double near_z,
                      const unsigned char background[3], void* ws, size_t ws_bytes, float* depth, unsigned char* out_rgb, int* index,
                      void* stream);
int a3r_render_set_form(int form);

/* Tracks and scene flow (csrc/track.hip): points followed through a clip by chaining the optical-flow fields of the scene's edges,
 * read off the aligned point maps at every frame they pass.  The reference has no such output (it computes the forward-backward
 * consistency of its flows, OccMask of dust3r/utils/goem_opt.py, stores it and never reads it); this text is the specification.
 * Inputs, all images of one shape H x W:
 *     xyz [N,H,W,3] fp32 world points, keep [N,H,W] uint8 (non-zero = the pixel counts)
 *     flow_a, flow_b [E,2,H,W] fp32: the flow of every edge in both directions (the scene's flow_ij / flow_ji); channel 0 = x, 1 = y
 *     steps [C,S,4] int32: C chains of S steps, each row (frame_from, frame_to, edge, reversed); the forward field of a step is
 *         reversed ? flow_b[edge] : flow_a[edge] and its backward field the other one
 *     seeds [M,2] fp32 (x, y) positions shared by all chains, or NULL = every pixel: M = H * W, x = m % W, y = m / W
 *     fb_thr: the forward-backward threshold in pixels (inf switches the check off)
 * All arithmetic is float64 on float64 copies of the fp32 inputs, every operation rounded on its own (no fused multiply-add).
 *     bilinear(F, x, y) for 0 <= x <= W - 1, 0 <= y <= H - 1:
 *         x0 = floor(x), x1 = min(x0 + 1, W - 1), ax = x - x0;   y0, y1, ay likewise
 *         top = F[y0,x0] + ax * (F[y0,x1] - F[y0,x0]),   bot likewise on row y1,   val = top + ay * (bot - top)
 *         (at integer coordinates and finite neighbours this is exactly F[y0,x0])
 * A track starts at (x, y) = its seed and is alive iff both coordinates are finite and inside [0, W-1] x [0, H-1].  It is recorded
 * at t = 0 in frame steps[c,0].frame_from (frame 0 when S = 0).  Then, for every step s:
 *     1. f = bilinear(fwd, x, y);  xn = x + f.x, yn = y + f.y.  The track ends unless xn, yn are finite and inside the image (the
 *        out-of-bounds rule of OccMask).
 *     2. b = bilinear(bwd, xn, yn);  dx = f.x + b.x, dy = f.y + b.y.  The track ends unless dx * dx + dy * dy < fb_thr * fb_thr (a
 *        NaN ends it).  This DIFFERS from OccMask on purpose: OccMask tests |dx + dy| < th, the absolute value of the SUM of the
 *        two components, which passes a pixel whose x and y errors cancel (dx = 10, dy = -10); the rule here is the Euclidean
 *        length of the disagreement.
 *     3. Otherwise (x, y) = (xn, yn) and the track is recorded at t = s + 1 in frame_to.
 * An ended track stays ended.  record(t, n) of a living track:
 *     col = rint(x), row = rint(y), half to even (as a3r_render_points rounds);  pix = row * W + col;  xy[t] = ((float)x, (float)y)
 *     state = 2 if keep[n,pix] is set and the three coordinates of xyz[n,pix] are finite, and then xyz[t] = xyz[n,pix];
 *     state = 1 otherwise (followed, not visible), xyz[t] = 0
 * and of an ended one: state 0, pix -1, xy and xyz zeros.  Outputs (planar: at every t the tracks are contiguous):
 *     out_xy [C,S+1,M,2] fp32, out_xyz [C,S+1,M,3] fp32, out_pix [C,S+1,M] int32, out_state [C,S+1,M] uint8
 * Scene flow is the case S = 1 with NULL seeds: xyz[1] - xyz[0] where state 2 holds at both ends.
 * Contract: the outputs are bitwise those of the numpy restatement (tests/track_cases.py: track_ref) and the same from call to
 * call.  One kernel, one thread per (chain, track) with the steps in a loop; no atomics, no LDS; nothing is allocated,
 * synchronised or read back, so the call can be captured into a graph.  steps_dev: the steps in device memory; steps_host: the
 * same table in host memory, validated before anything is launched.  `stream` is a hipStream_t, passed as void*.
 * A3R_EINVAL before anything is launched, naming the argument: a non-positive H or W, H * W >= 2^31, N <= 0, a negative E, C or S,
 * M < 0 or M >= 2^31, NULL seeds with M neither H * W nor 0, C * (S + 1) * M >= 2^31, fb_thr NaN or negative; then, unless M = 0 or C = 0
 * (a success that writes nothing): a null xyz, keep or output, and with S > 0 a null flow field or step table, a frame_from or
 * frame_to outside [0, N), an edge outside [0, E), reversed outside {0, 1}, a frame_from that is not the frame_to of the step
 * before it. */
int a3r_track_points(const float* xyz, const unsigned char* keep, int N, int H, int W, const float* flow_a, const float* flow_b, int E,
                     const int* steps_dev, const int* steps_host, int C, int S, const float* seeds, long long M, double fb_thr,
                     float* out_xy, float* out_xyz, int* out_pix, unsigned char* out_state, void* stream);

/* Voxel-grid downsampling (csrc/voxel.hip): the points of a cloud grouped by the cell of a regular grid they fall into, one point out
 * per cell, with the number of points that fell into it.  The reference has no such routine (its users run a voxel filter on the
 * host afterwards); this text is the specification.  Inputs: xyz [M,3] fp32, priority [M] fp32 or NULL, rgb [M,3] uint8 or NULL,
 * voxel (the cell's edge), reduce, min_count.  All arithmetic is float64 on float64 copies, every operation rounded on its own.
 *     r_a = x_a / voxel,  q_a = floor(r_a)  for a = x, y, z
 *     the point is IN A VOXEL iff its coordinates are finite and -2^20 <= q_a < 2^20 for all three (compared as doubles); every
 *         other point is dropped and counted in *dropped_host
 *     key = ((q_x + 2^20) << 42) | ((q_y + 2^20) << 21) | (q_z + 2^20)     (63 bits)
 *     value = (w << 32) | i  with i the point's row; w = 0 without priority, else with b = the fp32 bits of priority[i]:
 *         w = ~(b ^ (b >> 31 ? 0xffffffff : 0x80000000)), and w = 0xffffffff for a NaN: the larger priority has the smaller w
 *     the WINNER of a voxel is the minimum value over its points: the highest priority, the lowest row at an exact tie; a NaN
 *         priority wins only against NaNs.  count = the number of points with the voxel's key.
 *     kept voxels: count >= min_count, in ascending winner row (the output is a sub-sequence of the input)
 * Outputs, one row per kept voxel: out_index [V] int32 = the winner's row, out_count [V] int32 (either may be NULL), and
 *     reduce = A3R_VOXEL_BEST: out_xyz [V,3] and out_rgb [V,3] (or NULL) are the winner's rows, byte for byte
 *     reduce = A3R_VOXEL_MEAN: the unweighted mean over the voxel's points, order-independent by integer sums:
 *         t_a = (uint64)floor((r_a - q_a) * 2^24) per point,  S_a = the sum of t_a over the voxel (64-bit integers)
 *         out_xyz_a = (float)(((double)q_a + ((double)S_a + 0.5 * count) / ((double)count * 2^24)) * voxel)
 *         out_rgb_c = (2 * sum_c + count) / (2 * count) in integer arithmetic, sum_c = the sum of the channel over the voxel
 * Contract: minima and sums of integers do not depend on the order of their operands, so the outputs are bitwise reproducible from
 * call to call although the table is built with atomics, and bitwise the numpy restatement (tests/voxel_cases.py: voxel_ref).  Leaving
 * out priority, rgb / out_rgb, out_index or out_count changes nothing in the other outputs.
 * The table: open addressing with linear probing over `slots` entries (key, best value, count; six 64-bit sums more in mean mode).
 * slots is a power of two above M and at most 2^31; slots = 0 means the smallest power of two >= 2 M (at most 2^31).  Where a key
 * lands depends on the arrival order; nothing that is returned depends on it.  Passes in stream order: fill, insert (one thread per
 * point: an agent-scope read of the slot's key, a 64-bit compare-and-swap on an empty slot, then an atomic minimum and atomic adds on
 * the slot of its key, or the next slot; no locks, no waiting, at most `slots` probes; neighbouring lanes of a wave that share a key
 * fold their integer minimum and sums into one lane first, which changes no word of the table), flag + per-chunk counts, scan,
 * placement.
 * Two phases, as a3r_align_scene_count / _export:
 *   a3r_voxel_count  : *n_voxels_host = V, *dropped_host = the dropped points.
 *   a3r_voxel_export : counts afresh; capacity < V is refused with A3R_EINVAL, the message names V and NOTHING is written; otherwise
 *                      V rows are written.  *n_voxels_host = V and *dropped_host are set in both cases.
 * Both synchronise `stream` once (the counts return to the host).  workspace: a3r_voxel_workspace_bytes(M, slots, reduce) bytes,
 * 16-byte aligned: 256 + 4 (ceil(M / 1024) + 1) + 4 M + 20 slots bytes, 48 slots more for A3R_VOXEL_MEAN, each part rounded up to
 * 256 (0 for refused sizes).
 * A3R_EINVAL before anything is launched, naming the argument: M < 0 or M >= 2^31, an unknown reduce, voxel not finite or <= 0,
 * min_count < 1, slots not a power of two, slots <= M or above 2^31, a null xyz with M > 0, a null count pointer, a workspace that
 * is too small or misaligned, a negative capacity, a null out_xyz with capacity > 0, out_rgb without rgb.  A3R_ESTATE: a probe
 * found no free slot (impossible while slots > M; a guard).  M = 0 is a success with V = 0. */
#define A3R_VOXEL_BEST 0
#define A3R_VOXEL_MEAN 1
size_t a3r_voxel_workspace_bytes(long long M, long long slots, int reduce);
int a3r_voxel_count(const float* xyz, const float* priority, long long M, double voxel, int reduce, int min_count, long long slots,
                    void* workspace, size_t workspace_bytes, long long* n_voxels_host, long long* dropped_host, void* stream);
int a3r_voxel_export(const float* xyz, const float* priority, const unsigned char* rgb, long long M, double voxel, int reduce,
                     int min_count, long long slots, void* workspace, size_t workspace_bytes, long long capacity, float* out_xyz,
                     unsigned char* out_rgb, int* out_index, int* out_count, long long* n_voxels_host, long long* dropped_host,
                     void* stream);

/* TSDF fusion (csrc/tsdf.hip): the aligned depth maps of a clip integrated into one dense grid of truncated signed distances, and
 * the grid's zero surface as one triangle mesh.  The reference has no such routine; this text is the specification.  All arithmetic
 * is float64, every operation rounded on its own (no fused products).
 * GRID: origin[3], voxel (the cell's edge), dims (nx, ny, nz).  Voxel (i, j, k) has the centre
 *     X = ox + ((double)i + 0.5) * voxel,  Y = oy + ((double)j + 0.5) * voxel,  Z = oz + ((double)k + 0.5) * voxel
 * and the linear index (k * ny + j) * nx + i: the arrays are [nz, ny, nx].
 * INPUTS: depth [N,P] fp32, weight [N,P] fp32, rgb [N,P,3] uint8 or NULL, a camera table [N] of a3r_tsdf_cam = a3r_render_cam plus
 * the image's own shape (h, w).  Pixel (row, col) of frame n sits at n * P + row * w + col (every map flattened and padded to P,
 * so frames of mixed shapes share one array).
 * INTEGRATE: a voxel walks the frames n = 0 .. N - 1 in ascending order with W = S = Wc = C[0..2] = 0:
 *   1. xc = (R00 * X + R01 * Y) + R02 * Z + t0, yc and zc likewise with rows 1 and 2 of w2c;  u = fx * (xc / zc) + cx,
 *      v = fy * (yc / zc) + cy  (the renderer's expressions).
 *   2. the frame is skipped unless  zc >= near,  |u| < 2^30 and |v| < 2^30,  col = rint(u) in [0, w) and row = rint(v) in [0, h)
 *      (half to even).
 *   3. d = (double)depth[p], wd = (double)weight[p]; skipped unless both are finite and  wd > 0,  d > 0,  d <= max_depth  (every
 *      comparison is false for a NaN).
 *   4. sdf = d - zc; skipped if sdf < -trunc (the voxel is hidden behind the surface).
 *   5. t = min(1.0, sdf / trunc);  W += wd;  S += wd * t.
 *   6. only where sdf <= trunc and rgb is given:  Wc += wd;  C[ch] += wd * (double)rgb[p][ch].
 * OUTPUTS, each element written once:  tsdf [nz,ny,nx] fp32 = (float)(S / W), 1.0f where W == 0;  wsum fp32 = (float)W;
 * out_rgb [nz,ny,nx,3] uint8 (or NULL) = rint(C[ch] / Wc) clipped to 255, 0 where Wc == 0.
 * Contract: the sums live in registers and are sequential in frame order, there are no atomics: the outputs are bitwise
 * reproducible and bitwise the numpy restatement (tests/tsdf_cases.py: tsdf_ref).  Swapping two frames may change the last bit.
 * a3r_tsdf_integrate is enqueue-only (no synchronisation; it can be captured into a graph).  cams_dev is read by the kernel,
 * cams_host (the same table in host memory) by the checks.  skip_stats: NULL, or two device words that the call ADDS to: the
 * (brick, frame) pairs it met and the pairs its brick test skipped (a measurement; the only atomics of the file).
 * A3R_EINVAL before anything is launched, naming the field: dims not positive or nx * ny * nz >= 2^31; voxel, trunc or near not
 * finite or <= 0; max_depth <= 0 or NaN (infinity = no limit); a non-finite origin; N or P negative, N * P >= 2^31; a null array
 * with N > 0; a non-finite camera entry; h or w <= 0, h * w > P; out_rgb without rgb.  N = 0 writes the empty grid.
 * a3r_tsdf_set_form: a developer's A/B switch that does not change the outputs (returns the previous value; values outside [0, 1]
 * only query).  Bit 0 set: no brick test.  Default 0: a workgroup (a brick of 32 x 8 x 1 voxels) first projects the corners of its
 * box of voxel centres into every frame and leaves out the frames in which, by margins far above the rounding error, every voxel
 * lies behind `near` or more than a pixel outside the image -- frames in which no voxel of the brick passes step 2.
 * SURFACE (surface nets; no case table) from tsdf and wsum:
 *   a voxel is OBSERVED iff (double)wsum >= min_weight (min_weight > 0);  inside(f) = f < 0.
 *   cell (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, has the corners c = dx + 2 dy + 4 dz = voxel (i + dx, j + dy, k + dz); it
 *     is ACTIVE iff all 8 corners are observed and their inside values differ.
 *   the cell's 12 edges are the corner pairs (a, b), a < b, that differ in one bit, in lexicographic order (0,1) (0,2) (0,4)
 *     (1,3) (1,5) (2,3) (2,6) (3,7) (4,5) (4,6) (5,7) (6,7).  An edge CROSSES iff inside(fa) != inside(fb); then
 *     s = (double)fa / ((double)fa - (double)fb) and the crossing is, per axis, da + s * (db - da) with da, db the corners' offsets.
 *   the cell's VERTEX: m = the per-axis sum of the crossings in edge order divided by their count;
 *     x = (float)(ox + (((double)i + 0.5) + m_x) * voxel), y and z likewise;  colour (with rgb) = (2 * sum + 8) / 16 per channel in
 *     integer arithmetic over the 8 corners.  Vertex ids = the rank of the active cells in linear order of (k, j, i).
 *   FACES: a grid edge from voxel g along axis a (g_a + 1 < n_a) whose ends differ in inside, with b = (a + 1) % 3,
 *     c = (a + 2) % 3 and 1 <= g_b <= n_b - 2, 1 <= g_c <= n_c - 2, has the four cells q0 = g - e_b - e_c, q1 = g - e_c, q2 = g,
 *     q3 = g - e_b; it carries a quad iff all four are active: the triangles (q0, q1, q2), (q0, q2, q3) when inside(f(g)),
 *     otherwise (q0, q2, q1), (q0, q3, q2).  Faces are ordered by (linear index of g, a).
 *   Compaction without atomics: a count pass by wave ballots that leaves a rank map, an exclusive scan, a placement pass.
 * Two phases, as a3r_voxel_count / _export:
 *   a3r_tsdf_mesh_count  : *n_vertices_host = V, *n_faces_host = F.
 *   a3r_tsdf_mesh_export : counts afresh; a capacity below V or F is refused with A3R_EINVAL, the message names both counts and
 *                          NOTHING is written; otherwise out_xyz [V,3] fp32, out_rgb [V,3] uint8 (or NULL) and out_faces [F,3]
 *                          int32 are written.  The counts are set in both cases.
 * Both synchronise `stream` once.  workspace: a3r_tsdf_mesh_workspace_bytes(nx, ny, nz) bytes, 16-byte aligned:
 * 2 * 4 (ceil(nvox / 1024) + 1) + 4 nvox, each part rounded up to 256 (0 for refused sizes).  A3R_EINVAL as above for the grid, and
 * for nx * ny * nz above 2^31 / 6 (the face count is an int), min_weight not finite or <= 0, a null tsdf / wsum / count pointer, a
 * workspace that is too small or misaligned, a negative capacity, a null output with a positive capacity, out_rgb without rgb. */
typedef struct { double w2c[12]; double fx, fy, cx, cy; int h, w; } a3r_tsdf_cam;
int a3r_tsdf_integrate(const float* depth, const float* weight, const unsigned char* rgb, const a3r_tsdf_cam* cams_dev,
                       const a3r_tsdf_cam* cams_host, int N, long long P, const double origin[3], double voxel, int nx, int ny, int nz,
                       double trunc, double near_z, double max_depth, float* tsdf, float* wsum, unsigned char* out_rgb,
                       unsigned long long* skip_stats, void* stream);
int a3r_tsdf_set_form(int form);
size_t a3r_tsdf_mesh_workspace_bytes(int nx, int ny, int nz);
int a3r_tsdf_mesh_count(const float* tsdf, const float* wsum, int nx, int ny, int nz, double min_weight, void* workspace,
                        size_t workspace_bytes, long long* n_vertices_host, long long* n_faces_host, void* stream);
int a3r_tsdf_mesh_export(const float* tsdf, const float* wsum, const unsigned char* rgb, int nx, int ny, int nz, const double origin[3],
                         double voxel, double min_weight, void* workspace, size_t workspace_bytes, long long vertex_capacity,
                         long long face_capacity, float* out_xyz, unsigned char* out_rgb, int* out_faces, long long* n_vertices_host,
                         long long* n_faces_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A3R_H */
