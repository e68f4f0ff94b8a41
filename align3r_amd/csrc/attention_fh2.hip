// Flash-style attention for head_dim 64 on the fp16 matrix cores from two-plane fp16 operands ("fh2", fh2.h).
//
// Replaces  attn = softmax(q @ k^T * hd^-0.5); x = attn @ v   of
//   Attention.forward      croco/models/blocks.py:105-109
//   CrossAttention.forward croco/models/blocks.py:164-168
// like attention_bf3.hip, with every product evaluated as THREE exact fp16 x fp16 MFMA passes (h0 g0 + h0 g1 + h1 g0) instead of
// six bf16 ones: q, k, v arrive in fh2 form from the projection GEMM (RoPE + out_fh2 epilogue, gemm_fh2.hip), S^T = K Q^T and
// O^T = V^T P^T run on v_mfma_f32_32x32x16_f16, the online softmax is fp32 on the accumulators, and P -- in [0, 1] -- is split into
// two fp16 planes of 1024 p in registers (22 significant bits down to p = 2^-13, absolute error 2^-35 below that) and used directly
// as the B operand; the factor 1024 is divided out with the softmax normaliser.  O is written in fh2 form for the output
// projection.  The first form has the structure, staging and LDS layouts of attention_bf3.hip (AttnStaged<2>, attention_tile.h: K tiles
// by LDS-DMA into a double buffer, V tiles through registers into a transposed, key-permuted image, two 32-key online-softmax blocks
// per 64-key tile); the two-plane images are 53 KB per workgroup.
#include "attention_tile.h"
#include "dedup.h"
#include <cmath>
#include <atomic>
#include <cstdlib>
#include <string>

namespace a3r {

typedef AttnStaged<2> A4S;

struct Attn4Args {
    const char *q, *k, *v;
    char* o;
    size_t pq, pk, pv, po;                  // row pitches in bytes (4 x leading dimension)
    int B, H, Nq, Nk;
    float scale_log2e;                      // hd^-0.5 log2(e) / (q_scale k_scale): the exp2 argument's factor on the raw scores
    float out_mul;                          // out_scale / v_scale, applied with the softmax normaliser
    unsigned* out_absmax;                   // range statistics of the stored output (fh2.h), or null
    // a3r_attention_fh2_mapped (attn_fh2_v2_kernel only): batch b reads the q rows of image q_map[b] and the k / v rows of image
    // kv_map[b] (device, B words each; null: image b) and writes the o rows of image b
    const int *q_map, *kv_map;
};

// what both forms end with: O = oacc out_mul / l (P and l both carry the factor 2^10: it cancels) in fh2 form, and the statistic
__device__ __forceinline__ void attn_fh2_finish(const Attn4Args& a, const f32x16 (&oacc)[2], float l_run, int b, int h, int q_row, int half) {
    float amax = 0.f;
    char* op = a.o + ((size_t)b * a.Nq + q_row) * a.po;
    attn_normalise_store(oacc, l_run, a.out_mul, q_row < a.Nq, h, half, [&](int col, f32x4 v) {
        amax = fh2_amax4(amax, v);
        fh2_store4(op, col, v);
    });
    __shared__ unsigned s_amax[ATTN_T / 64];
    fh2_publish_block(a.out_absmax, amax, s_amax);
}

__global__ __launch_bounds__(ATTN_T, 2) void attn_fh2_kernel(Attn4Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qi = lane & 31, half = lane >> 5;
    int b, h, q_row, q_ld;
    if (!attn_place(a.Nq, a.B, a.H, wave, qi, b, h, q_row, q_ld)) return;

    // Q operand (B of S^T = K Q^T): lane (query, half) holds, per 16-deep d-step s and plane p, unit (2 s + half) 2 + p of its head
    f16x8 qf[4][2];
    {
        const char* qp = a.q + ((size_t)b * a.Nq + q_ld) * a.pq + h * A4S::HEAD_BYTES;
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int p = 0; p < 2; p++) qf[s][p] = *reinterpret_cast<const f16x8*>(qp + ((2 * s + half) * 2 + p) * 16);
    }
    A4S stage(smem, a.k + (size_t)b * a.Nk * a.pk + h * A4S::HEAD_BYTES, a.v + (size_t)b * a.Nk * a.pv + h * A4S::HEAD_BYTES, a.pk, a.pv,
              a.Nk, tid, wave);

    f32x16 oacc[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int e = 0; e < 16; e++) oacc[i][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float SCALE_LOG2E = a.scale_log2e;                    // hd^-0.5 (and the operands' power-of-two scales) folded into the exp2 argument

    const int kfrag = A4S::kfrag(qi, half), vfrag = A4S::vfrag(qi, half);
    const int ntiles = (a.Nk + ATTN_K - 1) / ATTN_K;
    stage.issue_k(0, 0);
    stage.load_v(0);
    stage.store_v();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < ntiles; t++) {
        const int k0 = t * ATTN_K;
        if (t + 1 < ntiles) {
            stage.issue_k(k0 + ATTN_K, (t + 1) & 1);        // that buffer was last read in iteration t-1: every wave has passed a barrier since
            stage.load_v(k0 + ATTN_K);
        }
        const char* Kt = stage.Ks + (t & 1) * A4S::KS_BYTES;
        // two 32-key blocks, each a full online-softmax step (keeps one score tile live at a time)
#pragma unroll
        for (int kb = 0; kb < 2; kb++) {
            // ---- S^T = K Q^T
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; e++) s[e] = 0.f;
#pragma unroll
            for (int st = 0; st < 4; st++) {
                f16x8 kf[2];
#pragma unroll
                for (int p = 0; p < 2; p++)
                    kf[p] = *reinterpret_cast<const f16x8*>(Kt + kfrag + kb * 32 * A4S::KROW + st * 64 + p * 16);
                fh2_mma32<3>(s, kf, qf[st]);
            }
            attn_softmax32<ATTN_EXP_FMA>(s, k0 + kb * 32, half, a.Nk, SCALE_LOG2E, m_run, l_run, oacc);
            // ---- O^T += V^T P^T: split 1024 P into two fp16 planes (k-step s2 = accumulator elements 8 s2 .. 8 s2 + 7)
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                u32x4 pf[2];
#pragma unroll
                for (int mm = 0; mm < 4; mm++) {
                    uint32_t p0, p1;
                    fh2_split2(s[8 * s2 + 2 * mm], s[8 * s2 + 2 * mm + 1], p0, p1);
                    pf[0][mm] = p0; pf[1][mm] = p1;
                }
                const f16x8 pb[2] = {__builtin_bit_cast(f16x8, pf[0]), __builtin_bit_cast(f16x8, pf[1])};
#pragma unroll
                for (int db = 0; db < 2; db++) {
                    f16x8 vf[2];
#pragma unroll
                    for (int p = 0; p < 2; p++)
                        vf[p] = *reinterpret_cast<const f16x8*>(stage.Vt + vfrag + (p * 64 + db * 32) * A4S::VROW + (kb * 4 + s2 * 2) * 16);
                    fh2_mma32<3>(oacc[db], vf, pb);
                }
            }
        }
        __syncthreads();                       // every wave is done with this tile's V^T image
        if (t + 1 < ntiles) stage.store_v();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's K DMAs for tile t+1 have landed
        __syncthreads();
    }
    attn_fh2_finish(a, oacc, l_run, b, h, q_row, half);
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Second form (round 3, default): V arrives like K -- by LDS-DMA into a row-major [key][256 B] image -- and its transposed MFMA
// operand is read with gfx950's ds_read_b64_tr_b16 (4 keys x 16 channels per 16-lane group, delivered column-major): no register
// staging of V (16 VGPRs live across the whole tile in the first form), no 2-byte transposition stores (32 per thread and tile).
// The registers that frees pay for a one-deep prefetch of the K and V fragments: the first form's read -> wait -> multiply order
// exposed the LDS latency eight times per 32-key block of each product, and prefetching there cost the third workgroup per CU.
// LDS image of a 64-key tile (K and V alike): row = key, 256 bytes = 16 chunks of 16 bytes in the LOGICAL order [plane 0: channel
// groups 0..7 | plane 1: channel groups 0..7] (the DMA's source address de-interleaves the fh2 row), stored at physical chunk
// c ^ swz(row), swz(row) = ((row & 3) << 2) | ((row >> 2) & 3): conflict-free for the row reads of the 32x32x16 A operand (S^T = K Q^T)
// and for the transposed reads (cdna_hip_programming.md T10, image (b)).  K double-buffered, V single-buffered (its DMA for tile t + 1
// is issued when every wave has finished tile t and has the first block's QK^T and softmax to land): 48 KB, three workgroups per CU.
#define B4_PIN() __builtin_amdgcn_sched_barrier(0)
constexpr int B4_ROW = 256;
constexpr int B4_TILE = ATTN_K * B4_ROW;       // 16 KB
constexpr int B4_LDS_BYTES = 3 * B4_TILE;      // K[2] + V
typedef short b4_s16x4 __attribute__((ext_vector_type(4)));
typedef short b4_s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int b4_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ b4_s16x4 b4_tr_read(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) b4_s16x4*)(p));
}

// PASSES 1 (a3r_fh2_set_passes(1)): first planes only -- q0 k0 and v0 p0 with p rounded to one fp16 -- the 16-bit operand mode.
template <int PASSES>
__global__ __launch_bounds__(ATTN_T, 3) void attn_fh2_v2_kernel(Attn4Args a) {
    constexpr int NPL = PASSES == 1 ? 1 : 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                                // [2][64 keys][256 B]
    char* Vs = smem + 2 * B4_TILE;                  // [64 keys][256 B]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qi = lane & 31, half = lane >> 5;
    int b, h, q_row, q_ld;
    if (!attn_place(a.Nq, a.B, a.H, wave, qi, b, h, q_row, q_ld)) return;

    const int bq = a.q_map ? a.q_map[b] : b, bkv = a.kv_map ? a.kv_map[b] : b;      // uniform
    f16x8 qf[4][NPL];
    {
        const char* qp = a.q + ((size_t)bq * a.Nq + q_ld) * a.pq + h * 256;
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int p = 0; p < NPL; p++) qf[s][p] = *reinterpret_cast<const f16x8*>(qp + ((2 * s + half) * 2 + p) * 16);
    }
    // ---- DMA: slot u = tid + 256 i -> (row = (tid >> 4) + 16 i, physical chunk tid & 15); swz(row) does not depend on i
    const int drow = tid >> 4;
    const int dch = (tid & 15) ^ b4_swz(drow);                         // logical chunk this thread fetches
    const int dsrc = ((dch & 7) * 2 + (dch >> 3)) * 16;                // its byte offset in the fh2 row slice of the head
    const char* kbase = a.k + (size_t)bkv * a.Nk * a.pk + h * 256 + dsrc;
    const char* vbase = a.v + (size_t)bkv * a.Nk * a.pv + h * 256 + dsrc;
    auto issue = [&](const char* base, size_t pitch, int k0, char* buf) {
        char* dst = buf + wave * 1024;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int kk = min(k0 + drow + 16 * i, a.Nk - 1);          // keys past Nk: finite copies (masked to -inf / multiplied by p = 0)
            __builtin_amdgcn_global_load_lds((attn_gptr)(base + (size_t)kk * pitch), (attn_lptr)(dst + 4096 * i), 16, 0, 0);
        }
    };
    // ---- fragment addresses (bytes inside a tile)
    const int ksw = b4_swz(qi);
    int koff[4][2];                                                    // K row read: row qi (+ 32 kb), logical chunk p 8 + 2 st + half
#pragma unroll
    for (int st = 0; st < 4; st++)
#pragma unroll
        for (int p = 0; p < 2; p++) koff[st][p] = qi * B4_ROW + ((((p << 3) | (st << 1) | half) ^ ksw) << 4);
    const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3, dsub = (lane >> 4) & 1;
    int voff[2][2][2];                                                 // V transposed read [plane][d block][key group of 4]
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int db = 0; db < 2; db++)
#pragma unroll
            for (int g2 = 0; g2 < 2; g2++) {
                const int row = 4 * half + 8 * g2 + tq;                // (+ 16 s2 + 32 kb: immediates)
                const int ch = (p << 3) + 4 * db + 2 * dsub + (tp >> 1);
                const int sw = (tq << 2) | ((half + 2 * g2) & 3);      // = swz(row + 16 s2 + 32 kb)
                voff[p][db][g2] = row * B4_ROW + ((ch ^ sw) << 4) + 8 * (tp & 1);
            }

    f32x16 oacc[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int e = 0; e < 16; e++) oacc[i][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float SCALE_LOG2E = a.scale_log2e;
    const int ntiles = (a.Nk + ATTN_K - 1) / ATTN_K;
    issue(kbase, a.pk, 0, Ks);
    issue(vbase, a.pv, 0, Vs);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                   // Q and K tile 0 have landed (V tile 0 may be in flight)
    __syncthreads();
    for (int t = 0; t < ntiles; t++) {
        const int k0 = t * ATTN_K;
        const bool more = t + 1 < ntiles;                              // uniform
        if (more) issue(kbase, a.pk, k0 + ATTN_K, Ks + ((t + 1) & 1) * B4_TILE);      // that buffer was last read in tile t - 1
        const char* Kt = Ks + (t & 1) * B4_TILE;
#pragma unroll
        for (int kb = 0; kb < 2; kb++) {
            // ---- S^T = K Q^T, fragments of d-step st + 1 requested before the MFMAs of d-step st
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; e++) s[e] = 0.f;
            f16x8 kf[2][NPL];
#pragma unroll
            for (int p = 0; p < NPL; p++) kf[0][p] = *reinterpret_cast<const f16x8*>(Kt + kb * 32 * B4_ROW + koff[0][p]);
#pragma unroll
            for (int st = 0; st < 4; st++) {
                if (st < 3) {
#pragma unroll
                    for (int p = 0; p < NPL; p++) kf[(st + 1) & 1][p] = *reinterpret_cast<const f16x8*>(Kt + kb * 32 * B4_ROW + koff[st + 1][p]);
                }
                B4_PIN();
                fh2_mma32<PASSES>(s, kf[st & 1], qf[st]);
                B4_PIN();
            }
            attn_softmax32<ATTN_EXP_FMA>(s, k0 + kb * 32, half, a.Nk, SCALE_LOG2E, m_run, l_run, oacc);
            if (kb == 0) {
                // V tile t: this wave's DMAs (issued at the end of tile t - 1, i.e. BEFORE K tile t + 1's) have landed, then everybody's
                if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
            // ---- O^T += V^T P^T; the transposed V fragments of the next (s2, db) are requested before the current MFMAs
            f16x8 pb[2][NPL];
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                u32x4 pf[2];
#pragma unroll
                for (int mm = 0; mm < 4; mm++) {
                    uint32_t p0, p1;
                    fh2_split2(s[8 * s2 + 2 * mm], s[8 * s2 + 2 * mm + 1], p0, p1);
                    pf[0][mm] = p0; pf[1][mm] = p1;
                }
#pragma unroll
                for (int p = 0; p < NPL; p++) pb[s2][p] = __builtin_bit_cast(f16x8, pf[p]);      // (PASSES 1: the residual plane is dead code)
            }
            auto vread = [&](int step, f16x8 (&vf)[NPL]) {              // step = 2 s2 + db
                const int s2 = step >> 1, db = step & 1;
                const char* base = Vs + (kb * 32 + s2 * 16) * B4_ROW;
#pragma unroll
                for (int p = 0; p < NPL; p++) {
                    const b4_s16x4 lo = b4_tr_read(base + voff[p][db][0]), hi = b4_tr_read(base + voff[p][db][1]);
                    vf[p] = __builtin_bit_cast(f16x8, b4_s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
                }
            };
            f16x8 vf[2][NPL];
            vread(0, vf[0]);
#pragma unroll
            for (int step = 0; step < 4; step++) {
                if (step < 3) vread(step + 1, vf[(step + 1) & 1]);
                B4_PIN();
                fh2_mma32<PASSES>(oacc[step & 1], vf[step & 1], pb[step >> 1]);
                B4_PIN();
            }
        }
        // every wave is done with V tile t and K tile t; K tile t + 1 (issued at the top of this iteration) has landed for everybody
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (more) issue(vbase, a.pv, k0 + ATTN_K, Vs);
    }
    attn_fh2_finish(a, oacc, l_run, b, h, q_row, half);
}

// which kernel form a3r_attention_fh2 launches: 2 (default) or 1 (A3R_ATTN=v1 / a3r_attention_fh2_set_form)
static std::atomic<int> g_attn_form{(getenv("A3R_ATTN") && std::string(getenv("A3R_ATTN")) == "v1") ? 1 : 2};

}  // namespace a3r
using namespace a3r;

extern "C" int a3r_attention_fh2_set_form(int form) {
    A3R_CHECK_ARG(form == 1 || form == 2, "a3r_attention_fh2_set_form: form must be 1 or 2");
    return g_attn_form.exchange(form) ;
}

bool a3r::attention_fh2_takes_maps() { return g_attn_form.load(std::memory_order_relaxed) == 2 || fh2_passes() != 3; }

static int attention_fh2_launch(const void* q2, int ldq, const void* k2, int ldk, const void* v2, int ldv, void* o2, int ldo, int B, int H,
                                int Nq, int Nk, const a3r_fh2_attn_range* range, const int32_t* q_map, const int32_t* kv_map, void* stream) {
    if (int rc = attention_check_args("a3r_attention_fh2", q2, k2, v2, o2, ldq, ldk, ldv, ldo, B, H, Nq, Nk, 8)) return rc;
    a3r_fh2_attn_range r = range ? *range : a3r_fh2_attn_range{};
    float* rs[4] = {&r.q_scale, &r.k_scale, &r.v_scale, &r.out_scale};
    for (float* p : rs) {
        if (*p == 0.f) *p = 1.f;
        A3R_CHECK_ARG(*p > 0.f && std::isfinite(*p), "a3r_attention_fh2: scales must be positive and finite");
    }
    const Attn4Args a = {static_cast<const char*>(q2), static_cast<const char*>(k2), static_cast<const char*>(v2), static_cast<char*>(o2),
                         (size_t)ldq * 4, (size_t)ldk * 4, (size_t)ldv * 4, (size_t)ldo * 4, B, H, Nq, Nk,
                         0.125f * 1.4426950408889634f / (r.q_scale * r.k_scale), r.out_scale / r.v_scale, r.out_absmax, q_map, kv_map};
    if (g_attn_form.load(std::memory_order_relaxed) == 1 && fh2_passes() == 3)      // A/B switch: the register-staged V form
        return launch_attention<attn_fh2_kernel, A4S::LDS_BYTES>(PK_ATTENTION_FH2, a, stream);
    if (fh2_passes() == 1) return launch_attention<attn_fh2_v2_kernel<1>, B4_LDS_BYTES>(PK_ATTENTION_FH2, a, stream);
    return launch_attention<attn_fh2_v2_kernel<3>, B4_LDS_BYTES>(PK_ATTENTION_FH2, a, stream);
}

extern "C" int a3r_attention_fh2(const void* q2, int ldq, const void* k2, int ldk, const void* v2, int ldv, void* o2, int ldo,
                                 int B, int H, int Nq, int Nk, const a3r_fh2_attn_range* range, void* stream) {
    return attention_fh2_launch(q2, ldq, k2, ldk, v2, ldv, o2, ldo, B, H, Nq, Nk, range, nullptr, nullptr, stream);
}

extern "C" int a3r_attention_fh2_mapped(const void* q2, int ldq, const void* k2, int ldk, const void* v2, int ldv, void* o2, int ldo,
                                        int B, int H, int Nq, int Nk, const a3r_fh2_attn_range* range, const int32_t* q_map,
                                        const int32_t* kv_map, void* stream) {
    A3R_CHECK_ARG((!q_map && !kv_map) || attention_fh2_takes_maps(), "a3r_attention_fh2_mapped: kernel form 1 takes no image maps");
    return attention_fh2_launch(q2, ldq, k2, ldk, v2, ldv, o2, ldo, B, H, Nq, Nk, range, q_map, kv_map, stream);
}
