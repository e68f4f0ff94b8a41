// Point correspondences for gfx950: exact 3-D nearest neighbours by brute force and the reciprocity test of the reference's
// find_reciprocal_matches (dust3r/utils/geometry.py:351-367, two KD-trees on the host there).
//
//   dx = (double)q.x - (double)data[k].x  (dy, dz likewise);  d2 = (dx * dx + dy * dy) + dz * dz, every operation rounded on its own
//   nn(q) = the SMALLEST k with d2(q, k) = min over { k : d2(q, k) < +inf },  -1 if there is none
//
// (this file is compiled with -ffp-contract=off: a product fused into the following sum would change the last bit and with it the
// winner of a near tie).  The running best starts at (+inf, -1) and is replaced on a strict `<` while k ascends, so the lowest index
// of a tie wins, and a NaN or infinite d2 -- a NaN or infinite coordinate on either side -- never wins and never becomes an index.
// Passes, no atomics, no data-dependent control flow: the output is a function of the inputs alone.
//   * search: grid (query blocks, chunks).  A thread keeps NN_QPT queries in registers as doubles; the data set is cut into `chunks`
//     contiguous ranges (the second grid axis, so that a small query count still fills the device), and a workgroup streams its
//     range through LDS in tiles of NN_TILE points, converted to double once on the way in.  All lanes read the same LDS address
//     in the same instruction (the broadcast case: no bank conflicts), so a point costs two LDS reads against NN_QPT * 12 vector
//     instructions.  Each (query, chunk) leaves one partial (d2, index) in the workspace, laid out [chunk][query].
//   * fold: one thread per query walks its partials in ascending chunk order with the same strict `<`: since the ranges ascend,
//     that is the definition's answer whatever the chunk count.
//   * reciprocity: flags, then the flagged k2 compacted by the count / scan / place scheme of compact.h.
#include "common.h"
#include "compact.h"
#include <cmath>

namespace a3r {

constexpr int NN_TPB = 256;
constexpr int NN_QPT = 4;                       // queries per thread
constexpr int NN_QBLOCK = NN_TPB * NN_QPT;      // queries per workgroup
constexpr int NN_TILE = 512;                    // data points per LDS tile: 12 KB as doubles
constexpr int NN_UNROLL = 4;                    // a tile is padded with NaN points to a multiple of this
constexpr int NN_MAX_CHUNKS = 65535;            // the second grid axis
constexpr int RM_PER = 4;                       // consecutive k2 per thread in the reciprocity passes
constexpr int RM_BLOCK = NN_TPB * RM_PER;

// grid (ceil(nq / NN_QBLOCK), chunks).  Query j of a thread is blockIdx.x * NN_QBLOCK + j * NN_TPB + tid (consecutive lanes on
// consecutive queries).  Chunk c owns the data range [nd * c / chunks, nd * (c + 1) / chunks), empty when chunks > nd.
__global__ __launch_bounds__(NN_TPB) void nn_search_kernel(const float* __restrict__ query, int nq, const float* __restrict__ data, int nd,
                                                          int chunks, double* __restrict__ part_d2, int* __restrict__ part_idx) {
    __shared__ double tile[NN_TILE * 3];
    const int tid = threadIdx.x, c = blockIdx.y;
    const int lo = (int)((long long)nd * c / chunks), hi = (int)((long long)nd * (c + 1) / chunks);
    const long long q0 = (long long)blockIdx.x * NN_QBLOCK + tid;              // 64-bit: q0 + j * NN_TPB may pass 2^31 in the last block
    double qx[NN_QPT], qy[NN_QPT], qz[NN_QPT], best[NN_QPT];
    int bidx[NN_QPT];
#pragma unroll
    for (int j = 0; j < NN_QPT; j++) {
        const long long q = q0 + j * NN_TPB;
        const bool in = q < nq;
        qx[j] = in ? (double)query[(size_t)q * 3 + 0] : 0.0;
        qy[j] = in ? (double)query[(size_t)q * 3 + 1] : 0.0;
        qz[j] = in ? (double)query[(size_t)q * 3 + 2] : 0.0;
        best[j] = INFINITY;
        bidx[j] = -1;
    }
    for (long long t0 = lo; t0 < hi; t0 += NN_TILE) {           // workgroup-uniform bounds
        const int n = (int)min((long long)NN_TILE, hi - t0);
        const int npad = (n + NN_UNROLL - 1) / NN_UNROLL * NN_UNROLL;
        __syncthreads();                                         // the previous tile has been consumed
        const float* __restrict__ src = data + (size_t)t0 * 3;
        for (int i = tid; i < npad * 3; i += NN_TPB) tile[i] = i < n * 3 ? (double)src[i] : (double)NAN;
        __syncthreads();
        for (int k = 0; k < npad; k += NN_UNROLL) {
#pragma unroll
            for (int u = 0; u < NN_UNROLL; u++) {
                const double px = tile[(k + u) * 3 + 0], py = tile[(k + u) * 3 + 1], pz = tile[(k + u) * 3 + 2];
#pragma unroll
                for (int j = 0; j < NN_QPT; j++) {
                    const double dx = qx[j] - px, dy = qy[j] - py, dz = qz[j] - pz;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    const bool lt = d2 < best[j];                // false for NaN, and for +inf against the start value
                    best[j] = lt ? d2 : best[j];
                    bidx[j] = lt ? (int)t0 + k + u : bidx[j];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NN_QPT; j++) {
        const long long q = q0 + j * NN_TPB;
        if (q < nq) {
            part_d2[(size_t)c * nq + q] = best[j];
            part_idx[(size_t)c * nq + q] = bidx[j];
        }
    }
}

// one thread per query: the partials in ascending chunk order.  chunks = 0 (an empty data set) writes the start value.
__global__ __launch_bounds__(NN_TPB) void nn_fold_kernel(const double* __restrict__ part_d2, const int* __restrict__ part_idx, int nq,
                                                        int chunks, int* __restrict__ out_index, double* __restrict__ out_d2) {
    const long long q = (long long)blockIdx.x * NN_TPB + threadIdx.x;
    if (q >= nq) return;
    double best = INFINITY;
    int idx = -1;
    for (int c = 0; c < chunks; c++) {
        const double d = part_d2[(size_t)c * nq + q];
        const int i = part_idx[(size_t)c * nq + q];
        if (d < best) { best = d; idx = i; }
    }
    out_index[q] = idx;
    if (out_d2) out_d2[q] = best;
}

// ------------------------------------------------------------------------------------------- reciprocity
// grid (ceil(n2 / RM_BLOCK)); a thread owns RM_PER consecutive k2.  WRITE = false: the flags and the block's count.  WRITE = true:
// the pairs (nn2[k2], k2) of the flagged k2 go to offsets[block] + (their rank inside the block): ascending k2.
template <bool WRITE>
__global__ __launch_bounds__(NN_TPB) void reciprocal_kernel(const int* __restrict__ nn2, const int* __restrict__ nn1, int n1, int n2,
                                                           unsigned char* flags, int* offsets, int* __restrict__ out_pairs) {
    __shared__ int wave_total[NN_TPB / 64];
    const int tid = threadIdx.x;
    const long long k0 = (long long)blockIdx.x * RM_BLOCK + tid * RM_PER;
    bool keep[RM_PER];
    int k1[RM_PER];
#pragma unroll
    for (int i = 0; i < RM_PER; i++) {
        const long long k2 = k0 + i;
        k1[i] = k2 < n2 ? nn2[k2] : -1;
        if (WRITE) keep[i] = k2 < n2 && flags[k2] != 0;
        else       keep[i] = k1[i] >= 0 && k1[i] < n1 && nn1[k1[i]] == k2;
    }
    int first, total;
    block_rank<NN_TPB, RM_PER>(keep, wave_total, &first, &total);
    if (!WRITE) {
#pragma unroll
        for (int i = 0; i < RM_PER; i++)
            if (k0 + i < n2) flags[k0 + i] = keep[i] ? 1 : 0;
        if (tid == 0) offsets[blockIdx.x] = total;
        return;
    }
    const int lim = offsets[blockIdx.x + 1];                     // the count pass saw the same flags; stay inside the range regardless
    int pos = offsets[blockIdx.x] + first;
#pragma unroll
    for (int i = 0; i < RM_PER; i++) {
        if (!keep[i]) continue;
        if (pos < lim) { out_pairs[(size_t)pos * 2 + 0] = k1[i]; out_pairs[(size_t)pos * 2 + 1] = (int)(k0 + i); }
        pos++;
    }
}

// The chunk count of a search.  Forced: as given.  Chosen: enough (query blocks x chunks) workgroups for sixteen per CU of the 256
// -- a CU holds seven at a time, and with only four or five each the last round is uneven: the sweep of forced values in
// profiles/matches.json has the count of a four-per-CU rule slower than this one (DESIGN 6.12 quotes the rows) --, never more
// ranges than tiles of data, at most 64.
static int nn_resolve_chunks(long long nq, long long nd, int chunks) {
    if (chunks > 0) return chunks;
    if (nq <= 0 || nd <= 0) return 1;
    const long long qblocks = (nq + NN_QBLOCK - 1) / NN_QBLOCK, tiles = (nd + NN_TILE - 1) / NN_TILE;
    long long want = (4096 + qblocks - 1) / qblocks;
    if (want > tiles) want = tiles;
    if (want > 64) want = 64;
    return (int)(want < 1 ? 1 : want);
}

static size_t nn_part_d2_bytes(long long nq, int chunks) { return align_up((size_t)nq * chunks * sizeof(double), 256); }
static size_t nn_part_idx_bytes(long long nq, int chunks) { return align_up((size_t)nq * chunks * sizeof(int), 256); }
static bool nn_size_ok(long long n) { return n >= 0 && n < (1ll << 31); }

static size_t nn_workspace_bytes(long long nq, long long nd, int chunks) {
    if (!nn_size_ok(nq) || !nn_size_ok(nd) || chunks < 0 || chunks > NN_MAX_CHUNKS || nq == 0 || nd == 0) return 0;
    const int ch = nn_resolve_chunks(nq, nd, chunks);
    return nn_part_d2_bytes(nq, ch) + nn_part_idx_bytes(nq, ch);
}

// search + fold, arguments already validated; the workspace holds nn_workspace_bytes(nq, nd, chunks) bytes, 16-byte aligned
static void nn_enqueue(const float* query, long long nq, const float* data, long long nd, int chunks, void* workspace, int* out_index,
                       double* out_d2, hipStream_t st) {
    if (nq == 0) return;
    const dim3 fold_grid((unsigned)((nq + NN_TPB - 1) / NN_TPB));
    if (nd == 0) {
        hipLaunchKernelGGL(nn_fold_kernel, fold_grid, dim3(NN_TPB), 0, st, static_cast<const double*>(nullptr), static_cast<const int*>(nullptr),
                           (int)nq, 0, out_index, out_d2);
        return;
    }
    const int ch = nn_resolve_chunks(nq, nd, chunks);
    double* pd = static_cast<double*>(workspace);
    int* pi = reinterpret_cast<int*>(static_cast<char*>(workspace) + nn_part_d2_bytes(nq, ch));
    hipLaunchKernelGGL(nn_search_kernel, dim3((unsigned)((nq + NN_QBLOCK - 1) / NN_QBLOCK), ch), dim3(NN_TPB), 0, st, query, (int)nq, data,
                       (int)nd, ch, pd, pi);
    hipLaunchKernelGGL(nn_fold_kernel, fold_grid, dim3(NN_TPB), 0, st, pd, pi, (int)nq, ch, out_index, out_d2);
}

// match workspace: search partials (the larger direction) | nn1_in_p2 [n1] int32 | block offsets [nblk + 1] int32, each rounded to 256
static size_t rm_search_bytes(long long n1, long long n2, int chunks) {
    const size_t a = nn_workspace_bytes(n2, n1, chunks), b = nn_workspace_bytes(n1, n2, chunks);
    return a > b ? a : b;
}
static size_t rm_nn1_bytes(long long n1) { return align_up((size_t)n1 * sizeof(int), 256); }
static long long rm_blocks(long long n2) { return (n2 + RM_BLOCK - 1) / RM_BLOCK; }

}  // namespace a3r

// =============================================================================================== host
using namespace a3r;

extern "C" int a3r_nn_chunks(long long n_query, long long n_data, int chunks) {
    if (!nn_size_ok(n_query) || !nn_size_ok(n_data) || chunks < 0 || chunks > NN_MAX_CHUNKS) return 0;
    return nn_resolve_chunks(n_query, n_data, chunks);
}

extern "C" size_t a3r_nn_workspace_bytes(long long n_query, long long n_data, int chunks) { return nn_workspace_bytes(n_query, n_data, chunks); }

extern "C" int a3r_nn_search(const float* query, long long n_query, const float* data, long long n_data, int chunks, void* workspace,
                             size_t workspace_bytes, int* out_index, double* out_dist2, void* stream) {
    const char* who = "a3r_nn_search";
    A3R_CHECK_ARG(nn_size_ok(n_query) && nn_size_ok(n_data), "%s: n_query = %lld, n_data = %lld: sizes are in [0, 2^31)", who, n_query, n_data);
    A3R_CHECK_ARG(chunks >= 0 && chunks <= NN_MAX_CHUNKS, "%s: chunks = %d is outside [0, %d]", who, chunks, NN_MAX_CHUNKS);
    A3R_CHECK_ARG(query || n_query == 0, "%s: null query", who);
    A3R_CHECK_ARG(data || n_data == 0, "%s: null data", who);
    A3R_CHECK_ARG(out_index || n_query == 0, "%s: null out_index", who);
    const size_t need = nn_workspace_bytes(n_query, n_data, chunks);
    if (need != 0)
        if (int rc = check_workspace(who, workspace, workspace_bytes, need)) return rc;
    nn_enqueue(query, n_query, data, n_data, chunks, workspace, out_index, out_dist2, as_stream(stream));
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" size_t a3r_match_workspace_bytes(long long n1, long long n2, int chunks) {
    if (!nn_size_ok(n1) || !nn_size_ok(n2) || chunks < 0 || chunks > NN_MAX_CHUNKS || n1 == 0 || n2 == 0) return 0;
    return rm_search_bytes(n1, n2, chunks) + rm_nn1_bytes(n1) + compact_offsets_bytes((size_t)rm_blocks(n2));
}

extern "C" int a3r_reciprocal_matches(const float* p1, long long n1, const float* p2, long long n2, int chunks, void* workspace,
                                      size_t workspace_bytes, int* nn2_in_p1, int* nn1_in_p2, unsigned char* reciprocal_in_p2,
                                      long long capacity, int* out_pairs, long long* n_matches_host, void* stream) {
    const char* who = "a3r_reciprocal_matches";
    A3R_CHECK_ARG(n_matches_host, "%s: null n_matches_host", who);
    *n_matches_host = 0;
    A3R_CHECK_ARG(nn_size_ok(n1) && nn_size_ok(n2), "%s: n1 = %lld, n2 = %lld: sizes are in [0, 2^31)", who, n1, n2);
    A3R_CHECK_ARG(chunks >= 0 && chunks <= NN_MAX_CHUNKS, "%s: chunks = %d is outside [0, %d]", who, chunks, NN_MAX_CHUNKS);
    A3R_CHECK_ARG(capacity >= 0, "%s: negative capacity", who);
    A3R_CHECK_ARG(p1 || n1 == 0, "%s: null p1", who);
    A3R_CHECK_ARG(p2 || n2 == 0, "%s: null p2", who);
    A3R_CHECK_ARG((nn2_in_p1 && reciprocal_in_p2) || n2 == 0, "%s: null nn2_in_p1 / reciprocal_in_p2", who);
    const size_t need = a3r_match_workspace_bytes(n1, n2, chunks);
    if (need != 0)
        if (int rc = check_workspace(who, workspace, workspace_bytes, need)) return rc;
    hipStream_t st = as_stream(stream);
    if (n1 == 0 || n2 == 0) {           // no neighbour on either side: -1 everywhere, nothing reciprocal
        if (n2 > 0) {
            nn_enqueue(p2, n2, p1, 0, chunks, nullptr, nn2_in_p1, nullptr, st);
            A3R_HIP(hipMemsetAsync(reciprocal_in_p2, 0, (size_t)n2, st));
        }
        if (n1 > 0 && nn1_in_p2) nn_enqueue(p1, n1, p2, 0, chunks, nullptr, nn1_in_p2, nullptr, st);
        A3R_LAUNCH_CHECK();
        A3R_HIP(hipStreamSynchronize(st));
        return A3R_OK;
    }
    char* ws = static_cast<char*>(workspace);
    int* nn1 = reinterpret_cast<int*>(ws + rm_search_bytes(n1, n2, chunks));
    int* offsets = reinterpret_cast<int*>(ws + rm_search_bytes(n1, n2, chunks) + rm_nn1_bytes(n1));
    const int nblk = (int)rm_blocks(n2);
    nn_enqueue(p2, n2, p1, n1, chunks, ws, nn2_in_p1, nullptr, st);
    nn_enqueue(p1, n1, p2, n2, chunks, ws, nn1, nullptr, st);             // stream order: the first search's fold has read its partials
    hipLaunchKernelGGL((reciprocal_kernel<false>), dim3(nblk), dim3(NN_TPB), 0, st, nn2_in_p1, nn1, (int)n1, (int)n2, reciprocal_in_p2, offsets,
                       static_cast<int*>(nullptr));
    compact_scan(offsets, nblk, st);
    A3R_LAUNCH_CHECK();
    if (nn1_in_p2) A3R_HIP(hipMemcpyAsync(nn1_in_p2, nn1, (size_t)n1 * sizeof(int), hipMemcpyDeviceToDevice, st));
    int total = 0;
    A3R_HIP(compact_read_total(offsets, nblk, &total, st));
    A3R_HIP(hipStreamSynchronize(st));
    *n_matches_host = total;
    if (!out_pairs) return A3R_OK;
    A3R_CHECK_ARG(total <= capacity, "%s: capacity %lld is smaller than the %d matches (no pair was written)", who, capacity, total);
    if (total == 0) return A3R_OK;
    hipLaunchKernelGGL((reciprocal_kernel<true>), dim3(nblk), dim3(NN_TPB), 0, st, nn2_in_p1, nn1, (int)n1, (int)n2, reciprocal_in_p2, offsets,
                       out_pairs);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
