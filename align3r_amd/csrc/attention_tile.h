// Scaffold shared by the attention kernels of liba3r (attention.hip, attention_bf3.hip, attention_fh2.hip).  All of them compute
// S^T = K Q^T (a query is a lane, its keys sit in the accumulator registers), a per-lane online softmax, then O^T = V^T P^T, with
// 4 waves x 32 queries per workgroup.  Shared here: the workgroup id -> (batch, head, query block) map and its grid, the key mask
// and online-softmax step of one 32-key block, the product ladders on the 32x32x16 MFMAs, the staged operands of the two
// register-staged-V kernels (attn_bf3_kernel, attn_fh2_kernel), the normalise-and-store epilogue, and on the host the entry checks
// and the launch.  As in gemm_tile.h, a device helper lives here only where the kernels that use it were compared against the
// parent commit: bit for bit on the GPU (tests/test_gpu_attention_parent.py), by compiler resources and instruction classes, and by
// time (DESIGN.md section 4 has the figures).
// Written out on purpose:
//   * attn_kernel (exact fp32) keeps its own softmax step: it takes the maximum over two 32-key blocks at once and rescales the
//     output accumulators unconditionally; under the ballot of attn_softmax32 its instruction stream and timing would change.
//   * the two exp-argument forms are different arithmetic and stay apart (ATTN_EXP_SUB / ATTN_EXP_FMA): never unify them.
//   * attn_fh2_v2_kernel keeps its own operand path (LDS-DMA of K and V into swizzled row-major images, transposed reads).
#pragma once
#include "common.h"
#include "bf3.h"
#include "fh2.h"

namespace a3r {

constexpr int ATTN_Q = 128;                 // queries per workgroup: 4 waves x 32
constexpr int ATTN_T = 256;                 // threads per workgroup
constexpr int ATTN_K = 64;                  // keys per tile
constexpr float ATTN_PSHIFT = 10.f;         // fh2: P is carried as 2^10 p in its two fp16 planes (p <= 1: 1024 p keeps 21+ bits above fp16's subnormal range)

typedef const __attribute__((address_space(1))) void* attn_gptr;
typedef __attribute__((address_space(3))) void* attn_lptr;

// ---- placement.  XCD-aware: the query blocks of one (batch, head) re-read the same K / V, and workgroup ids are dealt round-robin
// over the 8 XCDs (private L2s), so all query blocks of a head go to ONE XCD.  False for the surplus workgroups of the grid
// (uniform per workgroup: return at once).  q_row: this lane's query; q_ld: the row it loads (clamped)
__device__ __forceinline__ bool attn_place(int Nq, int B, int H, int wave, int qi, int& b, int& h, int& q_row, int& q_ld) {
    const int nqb = (Nq + ATTN_Q - 1) / ATTN_Q;
    const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
    const int group = (seq / nqb) * 8 + xcd, qb = seq - (seq / nqb) * nqb;
    if (group >= B * H) return false;
    h = group % H; b = group / H;
    q_row = qb * ATTN_Q + wave * 32 + qi;
    q_ld = q_row < Nq ? q_row : Nq - 1;
    return true;
}
static inline unsigned attn_grid(int B, int H, int Nq) { return 8 * ((B * H + 7) / 8) * ((Nq + ATTN_Q - 1) / ATTN_Q); }

// ---- key mask and online-softmax step of one 32-key block on a lane's scores (keys of the lane: key0 + (e&3) + 8*(e>>2) + 4*half):
// mask, max, the cross-half exchange, alpha, the exponentials (left in s), l_run, and the rescale of the output accumulators where
// the running maximum moved for some query of the wave (rare after the first tiles).  m_new is finite: the first block of every
// tile has a valid key, and m_run carries it on.  c: the exp2 argument's factor on the raw scores.
//   ATTN_EXP_SUB (bf3): p = exp2((s - m) c)
//   ATTN_EXP_FMA (fh2): 2^10 p = exp2(fma(s, c, fma(-m, c, 10))), ONE fma per element: the power of two that the fp16 planes of P
//                       need rides in the exponent, and l accumulates the scaled values (an exact scaling: O / l is unchanged)
enum AttnExp { ATTN_EXP_SUB, ATTN_EXP_FMA };
template <AttnExp EXP>
__device__ __forceinline__ void attn_softmax32(f32x16& s, int key0, int half, int Nk, float c, float& m_run, float& l_run, f32x16 (&oacc)[2]) {
    if (key0 + 32 > Nk) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int key = key0 + (e & 3) + 8 * (e >> 2) + 4 * half;
            if (key >= Nk) s[e] = -INFINITY;
        }
    }
    float mx = s[0];
#pragma unroll
    for (int e = 1; e < 16; e++) mx = fmaxf(mx, s[e]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
    m_run = m_new;
    const float off = EXP == ATTN_EXP_FMA ? __fmaf_rn(-m_new, c, ATTN_PSHIFT) : 0.f;
    float lsum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const float p = __builtin_amdgcn_exp2f(EXP == ATTN_EXP_FMA ? __fmaf_rn(s[e], c, off) : (s[e] - m_new) * c);
        s[e] = p;
        lsum += p;
    }
    l_run = l_run * alpha + lsum;
    if (__builtin_amdgcn_ballot_w64(alpha != 1.f)) {
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int e = 0; e < 16; e++) oacc[i][e] *= alpha;
    }
}

// ---- product ladders on one 32x32 accumulator, smallest terms first (the order of the passes is part of the result), beside
// bf3_mma of gemm_tile.h.  bf3 (v_mfma_f32_32x32x16_bf16), NP: 6 = a0b0 + (a0b1 + a1b0) + (a0b2 + a1b1 + a2b0), 3 = without the
// last group, 1 = a0b0 alone.  fh2 (v_mfma_f32_32x32x16_f16), PASSES: 3 = a0b0 + (a0b1 + a1b0), 1 = a0b0 alone (NPL = 1 plane held).
template <int NP>
__device__ __forceinline__ void bf3_mma32(f32x16& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
    if (NP == 6) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
    }
    if (NP >= 3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}
template <int PASSES, int NPL>
__device__ __forceinline__ void fh2_mma32(f32x16& acc, const f16x8 (&a)[NPL], const f16x8 (&b)[NPL]) {
    static_assert((PASSES == 3 && NPL == 2) || (PASSES == 1 && NPL == 1), "3 passes on two planes or 1 pass on one");
    if constexpr (PASSES == 3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[NPL - 1], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[NPL - 1], acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[0], acc, 0, 0, 0);
}

// ---- staged operands of attn_bf3_kernel (PL = 3 planes per 16-byte-unit group) and attn_fh2_kernel (PL = 2): a row of q / k / v
// holds, per head, 8 d-groups x PL planes of 16-byte units.
// K tiles of 64 keys go by LDS-DMA into a double buffer of padded rows (8 PL + 1 units: an odd stride makes every ds_read_b128 of
// an MFMA operand conflict-free with plain immediate offsets): 64 x (8 PL + 1) slots, slot u = (row u / (8 PL + 1), unit u % (8 PL + 1)),
// the pad unit is DMA'd too (LDS-DMA writes lane-linear) and re-reads unit 0; the last slot of a thread exists on wave 0 only.
// V tiles go global -> registers during the tile's MFMAs and are scattered to LDS between two barriers, transposed ([plane][d][key],
// rows of 64 keys x 2 B + 1 pad unit) and with the keys of each 16-key step permuted to the order the S^T accumulator holds them
// (the contraction order is free): 512 PL units, 2 PL per thread; unit u -> (key = u & 63 = tid & 63, gp = u >> 6 = PL d-group + plane):
// a wave walks the keys of one (d-group, plane).
template <int PL>
struct AttnStaged {
    static constexpr int KUNITS = 8 * PL + 1, KROW = KUNITS * 16, KSLOTS = ATTN_K * KUNITS, KI = (KSLOTS + ATTN_T - 1) / ATTN_T;
    static constexpr int KDIV = 65536 / KUNITS + 1;                   // (u KDIV) >> 16 = u / KUNITS: the excess u (KDIV - 65536 / KUNITS) / 65536
    static_assert((KSLOTS - 1) * (KDIV * KUNITS - 65536) < 65536, "  stays below the 1 / KUNITS that the largest remainder leaves");
    static constexpr int KS_BYTES = ATTN_K * KROW;                    // one K tile (two of them)
    static constexpr int VI = 2 * PL, VROW = 9 * 16, VT_BYTES = PL * 64 * VROW;
    static constexpr int LDS_BYTES = 2 * KS_BYTES + VT_BYTES;        // bf3: 78,848 B (two workgroups per CU); fh2: 53,248 B (three)
    static constexpr int HEAD_BYTES = 64 * PL * 2;                    // one head's slice of a row
    const char *kbase, *vbase;                                        // (batch, head) slice of k / v
    size_t pk, pv;                                                    // row pitches in bytes
    char *Ks, *Vt;                                                    // LDS: [2][64 rows][KUNITS units], [PL][64 d][VROW]
    int Nk, tid, wave, vkey, vpos2;
    u32x4 rv[VI];

    __device__ __forceinline__ AttnStaged(char* smem, const char* k, const char* v, size_t pk_, size_t pv_, int Nk_, int tid_, int wave_)
        : kbase(k), vbase(v), pk(pk_), pv(pv_), Ks(smem), Vt(smem + 2 * KS_BYTES), Nk(Nk_), tid(tid_), wave(wave_), vkey(tid_ & 63) {
        // V^T position of this thread's key: pos = 32 kt + 16 s2 + 8 hh + j with t = key & 15: hh = (t >> 2) & 1, j = (t & 3) + 4 (t >> 3)
        const int vt = vkey & 15;
        vpos2 = ((vkey & 48) + ((vt >> 2) & 1) * 8 + (vt & 3) + 4 * (vt >> 3)) * 2;
    }
    __device__ __forceinline__ void issue_k(int k0, int buf) const {
        char* base = Ks + buf * KS_BYTES + wave * 1024;
#pragma unroll
        for (int i = 0; i < KI; i++) {
            if (i == KI - 1 && wave != 0) break;                      // the slots past 256 (KI - 1): one wave
            const int u = min(tid + ATTN_T * i, KSLOTS - 1);          // (loop-invariant: the compiler keeps what it has registers for)
            const int row = (u * KDIV) >> 16, cu = u - row * KUNITS;   // u / KUNITS for u < KSLOTS
            const int kk = min(k0 + row, Nk - 1);                     // keys past Nk: finite copies, masked to -inf by attn_softmax32
            __builtin_amdgcn_global_load_lds((attn_gptr)(kbase + (size_t)kk * pk + (cu == KUNITS - 1 ? 0 : cu) * 16),
                                             (attn_lptr)(base + ATTN_T * 16 * i), 16, 0, 0);
        }
    }
    __device__ __forceinline__ void load_v(int k0) {
        const int vk = min(k0 + vkey, Nk - 1);
        const char* src = vbase + (size_t)vk * pv + wave * 16;
#pragma unroll
        for (int i = 0; i < VI; i++) rv[i] = *reinterpret_cast<const u32x4*>(src + 4 * 16 * i);      // gp = wave + 4 i
    }
    __device__ __forceinline__ void store_v() const {
#pragma unroll
        for (int i = 0; i < VI; i++) {
            const unsigned gp = wave + 4 * i;                                                         // wave-uniform
            const int g = gp / PL, p = gp - PL * g;                // (unsigned: a signed gp / 2 costs attn_fh2_kernel its third workgroup per CU)
            char* dst = Vt + (p * 64 + 8 * g) * VROW + vpos2;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t w = rv[i][j >> 1];
                *reinterpret_cast<uint16_t*>(dst + j * VROW) = (j & 1) ? (uint16_t)(w >> 16) : (uint16_t)(w & 0xffffu);
            }
        }
    }
    // byte offsets of a lane's MFMA operands: K row qi (+ 32 kb), units (2 st + half) PL + p; V^T row d = qi (+ 32 db), unit 4 kb + 2 s2 + half
    static __device__ __forceinline__ int kfrag(int qi, int half) { return qi * KROW + half * PL * 16; }
    static __device__ __forceinline__ int vfrag(int qi, int half) { return qi * VROW + half * 16; }
};

// ---- epilogue: O = oacc * (out_mul / l) in groups of four consecutive d; lane (query, half) holds d = 32 db + 8 g + 4 half + (0..3)
// of head h, i.e. columns h 64 + ... of the row.  Every lane calls it (the halves exchange l); store(column, f32x4) runs for valid rows.
template <class Store>
__device__ __forceinline__ void attn_normalise_store(const f32x16 (&oacc)[2], float l_run, float out_mul, bool valid, int h, int half, Store&& store) {
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv_l = out_mul / l_tot;
    if (!valid) return;
#pragma unroll
    for (int db = 0; db < 2; db++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const f32x4 v = {oacc[db][4 * g] * inv_l, oacc[db][4 * g + 1] * inv_l, oacc[db][4 * g + 2] * inv_l, oacc[db][4 * g + 3] * inv_l};
            store(h * 64 + db * 32 + 8 * g + 4 * half, v);
        }
}

// ---- host side
// what the entry points share; ld_multiple: the elements one 16-byte unit of the operand form holds.  Returns before anything is launched.
static inline int attention_check_args(const char* who, const void* q, const void* k, const void* v, const void* o, int ldq, int ldk,
                                       int ldv, int ldo, int B, int H, int Nq, int Nk, int ld_multiple) {
    const int m = ld_multiple;
    A3R_CHECK_ARG(q && k && v && o, "%s: null pointer", who);
    A3R_CHECK_ARG(B > 0 && H > 0 && Nq > 0 && Nk > 0, "%s: bad shape B=%d H=%d Nq=%d Nk=%d", who, B, H, Nq, Nk);
    A3R_CHECK_ARG(ldq >= H * 64 && ldk >= H * 64 && ldv >= H * 64 && ldo >= H * 64, "%s: row strides < H*64", who);
    A3R_CHECK_ARG(ldq % m == 0 && ldk % m == 0 && ldv % m == 0 && ldo % m == 0, "%s: row strides must be multiples of %d", who, m);
    A3R_CHECK_ARG(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
                    reinterpret_cast<uintptr_t>(o)) & 15) == 0, "%s: pointers must be 16-byte aligned", who);
    return A3R_OK;
}

// one workgroup per (batch, head, query block) plus the surplus of the XCD map; the dynamic-LDS attribute of KERN is set once per device
template <auto KERN, int LDS, class Args>
static int launch_attention(int prof_kernel, const Args& a, void* stream) {
    static_assert(LDS <= 160 * 1024, "LDS budget");
    static PerDeviceOnce attr_once;
    A3R_HIP(attr_once.ensure([&] { return hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, LDS); }));
    ProfScope prof(prof_kernel, 4.0 * a.B * a.H * (double)a.Nq * a.Nk * 64, as_stream(stream));
    hipLaunchKernelGGL(KERN, dim3(attn_grid(a.B, a.H, a.Nq)), dim3(ATTN_T), LDS, as_stream(stream), a);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

}  // namespace a3r
