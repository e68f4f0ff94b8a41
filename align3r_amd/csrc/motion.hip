// Self-computed motion masks of the flow aligner for gfx950 (dust3r/cloud_opt_flow/optimizer.py:201-235 of the reference): what
// follows the pair geometry of get_motion_mask_from_pairs.  Per DIRECTED entry (a symmetric pair votes twice: image i with the
// ego flow i -> j, image j with j -> i) and pixel (x, y), in fp32 and in the reference's order of operations:
//
//   D    = r . pt + t                          depth: z of a pointmap (r, t) = (0, 0, 1, 0), or z of inv(rel_pose) applied to it
//   disp = 1 / (D + 1e-6)
//   tgt  = H (x, y, 1) + disp * Kt             H = K_tgt R_rel K_src^-1, Kt = K_tgt t_rel, built on the host (warp_by_disp)
//   tgt /= tgt_z + 1e-6
//   err  = | tgt_xy - (x, y) - flow(x, y) |
//
// then per entry nerr = (err - min) / (max - min) over the whole map, per image the mean of its entries' nerr in list order, and
// mask = mean > thre.  IEEE all the way, as torch evaluates it: a NaN anywhere in an entry's map (amin / amax propagate it) or a
// constant map (0 / 0) turns that entry's contribution into NaN at every pixel, and the images it votes for get an all-false mask.
//
// Three streaming kernels, HBM-bound (20 B read + 4 B written per entry-pixel, then 4 B re-read), no atomics, fixed-order
// reductions (min / max are exact in any order; the NaN flag is an OR), so the result is a function of the inputs alone:
//   motion_err_kernel   grid (chunks, 2M): a workgroup owns MCHUNK = 1024 consecutive pixels of one entry, a thread 4 consecutive
//                       pixels (16-byte loads when P % 4 == 0 and the buffers are 16-byte aligned, scalar loads otherwise); writes
//                       err [2M, P] and one (min, max, NaN flag) partial per chunk
//   motion_fold_kernel  grid (2M): one wave folds the partials of an entry into (min, max - min), both NaN when the flag is set
//   motion_vote_kernel  grid (chunks, N): walks the image's CSR list, normalises, accumulates in list order, writes the byte mask
//                       (and the mean itself when asked for)
#include "common.h"

#include <cmath>

namespace a3r {

constexpr int MPX = 4;                  // consecutive pixels per thread
constexpr int MTPB = 256;
constexpr int MCHUNK = MPX * MTPB;      // pixels per workgroup

static int motion_nchunks(int P) { return (P + MCHUNK - 1) / MCHUNK; }
static size_t motion_err_bytes(int M, int P) { return align_up((size_t)2 * M * P * sizeof(float), 256); }
static size_t motion_partial_bytes(int M, int P) { return align_up((size_t)2 * M * motion_nchunks(P) * 4 * sizeof(float), 256); }
static size_t motion_stats_bytes(int M) { return align_up((size_t)2 * M * 2 * sizeof(float), 256); }

struct MotionView {
    int M2, N, E, P, W, nch;
    float thre;
    const float* pred_i;
    const float* pred_j;
    const float* flow_ij;
    const float* flow_ji;
    const a3r_motion_entry* entries;
    const int* list_start;
    const int* list_entry;
    float* err;                         // [2M, P]
    float* partial;                     // [2M, nch, 4]: min, max, NaN flag, 0
    float* stats;                       // [2M, 2]: min, max - min
};

// grid (nch, 2M)
template <bool VEC>
__global__ __launch_bounds__(MTPB) void motion_err_kernel(MotionView v) {
#pragma clang fp contract(off)
    __shared__ float sh_mn[MTPB / 64], sh_mx[MTPB / 64];
    __shared__ int sh_nan[MTPB / 64];
    const int e = blockIdx.y, tid = threadIdx.x, p0 = blockIdx.x * MCHUNK + tid * MPX;
    const a3r_motion_entry* __restrict__ rec = v.entries + e;       // wave-uniform: scalar loads
    const int src = rec->depth_row, frow = rec->flow_row;
    const float r0 = rec->depth_rt[0], r1 = rec->depth_rt[1], r2 = rec->depth_rt[2], rt = rec->depth_rt[3];
    const float h00 = rec->Hm[0], h01 = rec->Hm[1], h02 = rec->Hm[2], h10 = rec->Hm[3], h11 = rec->Hm[4], h12 = rec->Hm[5];
    const float h20 = rec->Hm[6], h21 = rec->Hm[7], h22 = rec->Hm[8];
    const float k0 = rec->Kt[0], k1 = rec->Kt[1], k2 = rec->Kt[2];
    const float* __restrict__ pts = (src < v.E ? v.pred_i + (size_t)src * v.P * 3 : v.pred_j + (size_t)(src - v.E) * v.P * 3);
    const float* __restrict__ fl = (frow < v.E ? v.flow_ij + (size_t)frow * v.P * 2 : v.flow_ji + (size_t)(frow - v.E) * v.P * 2);
    float mn = INFINITY, mx = -INFINITY;
    int has_nan = 0;
    if (p0 < v.P) {
        float pt[MPX * 3], fx[MPX], fy[MPX], er[MPX];
        if (VEC) {                      // P % 4 == 0 and p0 % 4 == 0: the four pixels are inside P together
            const f32x4* q = reinterpret_cast<const f32x4*>(pts + (size_t)p0 * 3);
            const f32x4 a = q[0], b = q[1], c = q[2];
            pt[0] = a.x; pt[1] = a.y; pt[2] = a.z; pt[3] = a.w; pt[4] = b.x; pt[5] = b.y; pt[6] = b.z; pt[7] = b.w;
            pt[8] = c.x; pt[9] = c.y; pt[10] = c.z; pt[11] = c.w;
            const f32x4 u = *reinterpret_cast<const f32x4*>(fl + p0), w = *reinterpret_cast<const f32x4*>(fl + v.P + p0);
            fx[0] = u.x; fx[1] = u.y; fx[2] = u.z; fx[3] = u.w;
            fy[0] = w.x; fy[1] = w.y; fy[2] = w.z; fy[3] = w.w;
        } else {
#pragma unroll
            for (int i = 0; i < MPX; i++) {
                const bool in = p0 + i < v.P;
#pragma unroll
                for (int k = 0; k < 3; k++) pt[i * 3 + k] = in ? pts[(size_t)(p0 + i) * 3 + k] : 0.f;
                fx[i] = in ? fl[p0 + i] : 0.f;
                fy[i] = in ? fl[(size_t)v.P + p0 + i] : 0.f;
            }
        }
        int y = p0 / v.W, x = p0 - y * v.W;
#pragma unroll
        for (int i = 0; i < MPX; i++) {
            const float xf = (float)x, yf = (float)y;
            const float D = r0 * pt[i * 3] + r1 * pt[i * 3 + 1] + r2 * pt[i * 3 + 2] + rt;
            const float disp = 1.f / (D + 1e-6f);
            const float tx = (h00 * xf + h01 * yf + h02) + disp * k0;
            const float ty = (h10 * xf + h11 * yf + h12) + disp * k1;
            const float tz = (h20 * xf + h21 * yf + h22) + disp * k2;
            const float den = tz + 1e-6f;
            const float dx = (tx / den - xf) - fx[i], dy = (ty / den - yf) - fy[i];
            er[i] = sqrtf(dx * dx + dy * dy);
            if (p0 + i < v.P) {
                has_nan |= er[i] != er[i];
                mn = fminf(mn, er[i]);
                mx = fmaxf(mx, er[i]);
            }
            if (++x == v.W) { x = 0; y++; }
        }
        float* o = v.err + (size_t)e * v.P + p0;
        if (VEC) {
            *reinterpret_cast<f32x4*>(o) = f32x4{er[0], er[1], er[2], er[3]};
        } else {
#pragma unroll
            for (int i = 0; i < MPX; i++)
                if (p0 + i < v.P) o[i] = er[i];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
        has_nan |= __shfl_xor(has_nan, o);
    }
    if ((tid & 63) == 0) { sh_mn[tid >> 6] = mn; sh_mx[tid >> 6] = mx; sh_nan[tid >> 6] = has_nan; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < MTPB / 64; k++) { mn = fminf(mn, sh_mn[k]); mx = fmaxf(mx, sh_mx[k]); has_nan |= sh_nan[k]; }
        *reinterpret_cast<f32x4*>(v.partial + ((size_t)e * v.nch + blockIdx.x) * 4) = f32x4{mn, mx, has_nan ? 1.f : 0.f, 0.f};
    }
}

// grid (2M), one wave
__global__ __launch_bounds__(64) void motion_fold_kernel(MotionView v) {
#pragma clang fp contract(off)
    const int e = blockIdx.x, lane = threadIdx.x;
    float mn = INFINITY, mx = -INFINITY, flag = 0.f;
    for (int c = lane; c < v.nch; c += 64) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(v.partial + ((size_t)e * v.nch + c) * 4);
        mn = fminf(mn, q.x); mx = fmaxf(mx, q.y); flag = fmaxf(flag, q.z);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
        flag = fmaxf(flag, __shfl_xor(flag, o));
    }
    if (lane == 0) {
        const float nan = __builtin_nanf("");
        v.stats[e * 2 + 0] = flag > 0.f ? nan : mn;
        v.stats[e * 2 + 1] = flag > 0.f ? nan : mx - mn;       // inf - inf = NaN, as torch has it
    }
}

// grid (nch, N)
template <bool VEC, bool MEAN>
__global__ __launch_bounds__(MTPB) void motion_vote_kernel(MotionView v, unsigned char* __restrict__ masks, float* __restrict__ mean_err) {
#pragma clang fp contract(off)
    const int n = blockIdx.y, p0 = blockIdx.x * MCHUNK + threadIdx.x * MPX;
    if (p0 >= v.P) return;
    const int lo = v.list_start[n], hi = v.list_start[n + 1];
    float acc[MPX] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = lo; k < hi; k++) {
        const int e = v.list_entry[k];
        const float mn = v.stats[e * 2], den = v.stats[e * 2 + 1];
        const float* __restrict__ row = v.err + (size_t)e * v.P + p0;
        float er[MPX];
        if (VEC) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(row);
            er[0] = q.x; er[1] = q.y; er[2] = q.z; er[3] = q.w;
        } else {
#pragma unroll
            for (int i = 0; i < MPX; i++) er[i] = p0 + i < v.P ? row[i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < MPX; i++) acc[i] += (er[i] - mn) / den;
    }
    const float cnt = (float)(hi - lo);
    float mean[MPX];
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < MPX; i++) {
        mean[i] = acc[i] / cnt;
        bits |= (mean[i] > v.thre ? 1u : 0u) << (8 * i);         // NaN: false
    }
    const size_t o = (size_t)n * v.P + p0;
    if (VEC) {
        *reinterpret_cast<unsigned*>(masks + o) = bits;
        if (MEAN) *reinterpret_cast<f32x4*>(mean_err + o) = f32x4{mean[0], mean[1], mean[2], mean[3]};
    } else {
#pragma unroll
        for (int i = 0; i < MPX; i++)
            if (p0 + i < v.P) {
                masks[o + i] = (unsigned char)((bits >> (8 * i)) & 1u);
                if (MEAN) mean_err[o + i] = mean[i];
            }
    }
}

}  // namespace a3r

// =============================================================================================== host
using namespace a3r;

extern "C" size_t a3r_motion_workspace_bytes(int M, int N, int P) {
    if (M <= 0 || N <= 0 || P <= 0) return 0;
    return motion_err_bytes(M, P) + motion_partial_bytes(M, P) + motion_stats_bytes(M);
}

// Enqueues three kernels on `stream`: no allocation, no synchronisation, nothing read back (graph-capturable).
extern "C" int a3r_motion_masks(const a3r_motion_desc* d, void* ws, size_t ws_bytes, unsigned char* masks, float* mean_err, void* stream) {
    const char* who = "a3r_motion_masks";
    A3R_CHECK_ARG(d, "%s: null descriptor", who);
    A3R_CHECK_ARG(d->M > 0 && d->N > 0 && d->H > 0 && d->W > 0 && d->E > 0, "%s: M, N, E, H and W must be positive (M=%d N=%d E=%d H=%d W=%d)", who,
                  d->M, d->N, d->E, d->H, d->W);
    A3R_CHECK_ARG((long long)d->H * d->W < (1ll << 30), "%s: H * W = %lld is too large", who, (long long)d->H * d->W);
    A3R_CHECK_ARG(d->M <= 32767 && d->N <= 65535, "%s: M = %d / N = %d exceed the launch grid", who, d->M, d->N);
    A3R_CHECK_ARG(d->pred_i && d->pred_j && d->flow_ij && d->flow_ji, "%s: null pointmap or flow buffer", who);
    A3R_CHECK_ARG(d->entries && d->entries_host && d->list_start && d->list_start_host && d->list_entry && d->list_entry_host,
                  "%s: null entry table or image list", who);
    A3R_CHECK_ARG(masks, "%s: null mask buffer", who);
    A3R_CHECK_ARG(d->motion_mask_thre == d->motion_mask_thre, "%s: motion_mask_thre is NaN", who);
    const int M2 = 2 * d->M, P = d->H * d->W;
    const size_t need = a3r_motion_workspace_bytes(d->M, d->N, P);
    if (int rc = check_workspace(who, ws, ws_bytes, need)) return rc;
    for (int e = 0; e < M2; e++) {
        const a3r_motion_entry& r = d->entries_host[e];
        A3R_CHECK_ARG(r.depth_row >= 0 && r.depth_row < 2 * d->E, "%s: entry %d: depth_row %d is outside [0, %d)", who, e, r.depth_row, 2 * d->E);
        A3R_CHECK_ARG(r.flow_row >= 0 && r.flow_row < 2 * d->E, "%s: entry %d: flow_row %d is outside [0, %d)", who, e, r.flow_row, 2 * d->E);
        A3R_CHECK_ARG(r.image >= 0 && r.image < d->N, "%s: entry %d: image %d is outside [0, %d)", who, e, r.image, d->N);
    }
    A3R_CHECK_ARG(d->list_start_host[0] == 0, "%s: list_start[0] must be 0", who);
    for (int n = 0; n < d->N; n++) {
        const int lo = d->list_start_host[n], hi = d->list_start_host[n + 1];
        A3R_CHECK_ARG(hi > lo, "%s: image %d has an empty list", who, n);
        A3R_CHECK_ARG(hi <= M2, "%s: image %d: list end %d is beyond the %d entries", who, n, hi, M2);
        for (int k = lo; k < hi; k++)
            A3R_CHECK_ARG(d->list_entry_host[k] >= 0 && d->list_entry_host[k] < M2, "%s: image %d: list entry %d is outside [0, %d)", who, n,
                          d->list_entry_host[k], M2);
    }
    hipStream_t st = as_stream(stream);
    MotionView v;
    v.M2 = M2; v.N = d->N; v.E = d->E; v.P = P; v.W = d->W; v.nch = motion_nchunks(P);
    v.thre = d->motion_mask_thre;
    v.pred_i = d->pred_i; v.pred_j = d->pred_j; v.flow_ij = d->flow_ij; v.flow_ji = d->flow_ji;
    v.entries = d->entries; v.list_start = d->list_start; v.list_entry = d->list_entry;
    char* w = static_cast<char*>(ws);
    v.err = reinterpret_cast<float*>(w);
    v.partial = reinterpret_cast<float*>(w + motion_err_bytes(d->M, P));
    v.stats = reinterpret_cast<float*>(w + motion_err_bytes(d->M, P) + motion_partial_bytes(d->M, P));
    const bool vec = P % 4 == 0 && aligned_to(d->pred_i, 16) && aligned_to(d->pred_j, 16) && aligned_to(d->flow_ij, 16) && aligned_to(d->flow_ji, 16) &&
                     aligned_to(masks, 4) && (!mean_err || aligned_to(mean_err, 16));
    const dim3 block(MTPB);
    if (vec) hipLaunchKernelGGL((motion_err_kernel<true>), dim3(v.nch, M2), block, 0, st, v);
    else     hipLaunchKernelGGL((motion_err_kernel<false>), dim3(v.nch, M2), block, 0, st, v);
    hipLaunchKernelGGL(motion_fold_kernel, dim3(M2), dim3(64), 0, st, v);
#define A3R_MOTION_VOTE(VECV, MEANV) hipLaunchKernelGGL((motion_vote_kernel<VECV, MEANV>), dim3(v.nch, d->N), block, 0, st, v, masks, mean_err)
    if (vec) { if (mean_err) A3R_MOTION_VOTE(true, true); else A3R_MOTION_VOTE(true, false); }
    else     { if (mean_err) A3R_MOTION_VOTE(false, true); else A3R_MOTION_VOTE(false, false); }
#undef A3R_MOTION_VOTE
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
