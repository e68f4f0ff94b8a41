// Flash-style attention for head_dim 64 on the bf16 matrix cores, fp32-accurate ("bf3" operands, bf3.h).
//
// Replaces  attn = softmax(q @ k^T * hd^-0.5); x = attn @ v   of
//   Attention.forward      croco/models/blocks.py:105-109
//   CrossAttention.forward croco/models/blocks.py:164-168
// like attention.hip, but both products run as six exact bf16 x bf16 MFMA passes over three-plane splits:
//   * q, k, v arrive in bf3 form straight from the projection GEMM (RoPE + out_bf3 epilogue, gemm_bf3.hip);
//   * S^T = K Q^T  (v_mfma_f32_32x32x16_bf16; a lane's K / Q operand is one 16-byte bf3 unit per plane);
//   * online softmax in fp32 on the accumulators (a query is a lane, its keys sit in the registers);
//   * P is split into three bf16 planes in registers (exactly: p = p0 + p1 + p2) and is directly the B operand of
//     O^T = V^T P^T; V^T needs 8 consecutive KEYS per lane, so the V tile is staged through LDS transposed, with the
//     keys of each 16-key step permuted to the order the S^T accumulator holds them (the contraction order is free);
//   * O is written in bf3 form, the input format of the output projection GEMM.
// A workgroup = 4 waves = 128 queries of one (batch, head), each wave 32 queries; two workgroups share a CU.  K tiles of 64 keys are prefetched by
// LDS-DMA into a double buffer, V tiles global -> registers during the tile's MFMAs and scattered to LDS between two
// barriers (AttnStaged<3>, attention_tile.h); inside a tile each 32-key block is a complete online-softmax step (one score accumulator live).
#include "attention_tile.h"

namespace a3r {

typedef AttnStaged<3> A3S;

struct Attn3Args {
    const char *q, *k, *v;
    char* o;
    size_t pq, pk, pv, po;                  // row pitches in bytes (6 x leading dimension)
    int B, H, Nq, Nk;
    int ldo, out_pair;                      // o: leading dimension in elements; row-pair layout (bf3.h) for a GEMM-only consumer
    int out_fh2;                            // o in fh2 form (fh2.h, scale 1, plain rows) for an a3r_linear_fh2 output projection
};

template <int NP>
__global__ __launch_bounds__(ATTN_T, 2) void attn_bf3_kernel(Attn3Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qi = lane & 31, half = lane >> 5;
    int b, h, q_row, q_ld;
    if (!attn_place(a.Nq, a.B, a.H, wave, qi, b, h, q_row, q_ld)) return;

    // Q operand (B of S^T = K Q^T): lane (query, half) holds, per 16-deep d-step s and plane p, unit (2 s + half) 3 + p
    bf16x8 qf[4][3];
    {
        const char* qp = a.q + ((size_t)b * a.Nq + q_ld) * a.pq + h * A3S::HEAD_BYTES;
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int p = 0; p < 3; p++) qf[s][p] = *reinterpret_cast<const bf16x8*>(qp + ((2 * s + half) * 3 + p) * 16);
    }
    A3S stage(smem, a.k + (size_t)b * a.Nk * a.pk + h * A3S::HEAD_BYTES, a.v + (size_t)b * a.Nk * a.pv + h * A3S::HEAD_BYTES, a.pk, a.pv,
              a.Nk, tid, wave);

    f32x16 oacc[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int e = 0; e < 16; e++) oacc[i][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float SCALE_LOG2E = 0.125f * 1.4426950408889634f;     // hd^-0.5 folded into the exp2 argument

    const int kfrag = A3S::kfrag(qi, half), vfrag = A3S::vfrag(qi, half);
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
        const char* Kt = stage.Ks + (t & 1) * A3S::KS_BYTES;
        // two 32-key blocks, each a full online-softmax step (keeps one score tile live at a time)
#pragma unroll
        for (int kb = 0; kb < 2; kb++) {
            // ---- S^T = K Q^T
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; e++) s[e] = 0.f;
#pragma unroll
            for (int st = 0; st < 4; st++) {
                bf16x8 kf[3];
#pragma unroll
                for (int p = 0; p < 3; p++)
                    kf[p] = *reinterpret_cast<const bf16x8*>(Kt + kfrag + kb * 32 * A3S::KROW + st * 96 + p * 16);
                bf3_mma32<NP>(s, kf, qf[st]);
            }
            attn_softmax32<ATTN_EXP_SUB>(s, k0 + kb * 32, half, a.Nk, SCALE_LOG2E, m_run, l_run, oacc);
            // ---- O^T += V^T P^T: split P into planes (k-step s2 = accumulator elements 8 s2 .. 8 s2 + 7)
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                u32x4 pf[3];
#pragma unroll
                for (int mm = 0; mm < 4; mm++) {
                    uint32_t p0, p1, p2;
                    bf3_split2(s[8 * s2 + 2 * mm], s[8 * s2 + 2 * mm + 1], p0, p1, p2);
                    pf[0][mm] = p0; pf[1][mm] = p1; pf[2][mm] = p2;
                }
                const bf16x8 pb[3] = {__builtin_bit_cast(bf16x8, pf[0]), __builtin_bit_cast(bf16x8, pf[1]), __builtin_bit_cast(bf16x8, pf[2])};
#pragma unroll
                for (int db = 0; db < 2; db++) {
                    bf16x8 vf[3];
#pragma unroll
                    for (int p = 0; p < 3; p++)
                        vf[p] = *reinterpret_cast<const bf16x8*>(stage.Vt + vfrag + (p * 64 + db * 32) * A3S::VROW + (kb * 4 + s2 * 2) * 16);
                    bf3_mma32<NP>(oacc[db], vf, pb);
                }
            }
        }
        __syncthreads();                       // every wave is done with this tile's V^T image
        if (t + 1 < ntiles) stage.store_v();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's K DMAs for tile t+1 have landed
        __syncthreads();
    }
    char* op = a.out_fh2 ? a.o + ((size_t)b * a.Nq + q_row) * fh2_row_bytes(a.ldo)
                         : a.o + bf3_row_offset((long)b * a.Nq + q_row, a.ldo, a.out_pair);
    attn_normalise_store(oacc, l_run, 1.f, q_row < a.Nq, h, half, [&](int col, f32x4 v) {     // half a bf3 (or fh2) unit per plane
        if (a.out_fh2) fh2_store4(op, col, v);
        else bf3_store4(op, col, v, a.out_pair);
    });
}

}  // namespace a3r
using namespace a3r;

template <int NP>
static int launch_bf3(const Attn3Args& a, void* stream) { return launch_attention<attn_bf3_kernel<NP>, A3S::LDS_BYTES>(PK_ATTENTION_BF3, a, stream); }

static int attention_bf3_impl(const void* q3, int ldq, const void* k3, int ldk, const void* v3, int ldv, void* o3, int ldo,
                              int B, int H, int Nq, int Nk, int out_pair, int out_fh2, void* stream) {
    if (int rc = attention_check_args("a3r_attention_bf3", q3, k3, v3, o3, ldq, ldk, ldv, ldo, B, H, Nq, Nk, 8)) return rc;
    A3R_CHECK_ARG(!out_pair || ldo % 32 == 0, "a3r_attention_bf3: the row-pair output layout needs ldo %% 32 == 0");
    const Attn3Args a = {static_cast<const char*>(q3), static_cast<const char*>(k3), static_cast<const char*>(v3), static_cast<char*>(o3),
                         (size_t)ldq * 6, (size_t)ldk * 6, (size_t)ldv * 6, (size_t)ldo * 6, B, H, Nq, Nk, ldo, out_pair ? 1 : 0, out_fh2 ? 1 : 0};
    const int np = bf3_products();       // process-wide arithmetic mode (a3r_bf3_set_products)
    return np == 6 ? launch_bf3<6>(a, stream) : np == 3 ? launch_bf3<3>(a, stream) : launch_bf3<1>(a, stream);
}

extern "C" int a3r_attention_bf3(const void* q3, int ldq, const void* k3, int ldk, const void* v3, int ldv, void* o3, int ldo,
                                 int B, int H, int Nq, int Nk, int out_pair, void* stream) {
    return attention_bf3_impl(q3, ldq, k3, ldk, v3, ldv, o3, ldo, B, H, Nq, Nk, out_pair, 0, stream);
}

extern "C" int a3r_attention_bf3_fh2out(const void* q3, int ldq, const void* k3, int ldk, const void* v3, int ldv, void* o2, int ldo,
                                        int B, int H, int Nq, int Nk, void* stream) {
    return attention_bf3_impl(q3, ldq, k3, ldk, v3, ldv, o2, ldo, B, H, Nq, Nk, 0, 1, stream);
}
