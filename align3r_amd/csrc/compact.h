// Deterministic stream compaction, no atomics (scene.hip: kept pixels and faces; voxel.hip: winners; tsdf.hip: cells and quads;
// match.hip: reciprocal pairs; metrics.hip: valid pixels).  A workgroup owns a chunk of consecutive items, a thread ITEMS consecutive
// ones.  Count pass: the kernel flags its items and block_rank gives the chunk's count, which goes to cnt[chunk].  compact_scan turns
// the T counts into exclusive offsets in place and leaves the total in cnt[T].  Placement pass: the kernel flags again, and a flagged
// item goes to cnt[chunk] + its rank: the output is in item order, a function of the inputs alone.
#pragma once
#include "common.h"

namespace a3r {

// Ranks of a thread's flagged items among the workgroup's, for SETS independent flag sets (set s: flag[s * ITEMS + item]) at once.
// first[s] = the rank of the thread's first flagged item of set s, in (thread, item) order -- its later ones follow consecutively --,
// total[s] = the workgroup's count.  Wave64; TPB threads, every one of which calls it (it contains one __syncthreads());
// wave_total is LDS that nothing else touches around the call.
template <int TPB, int ITEMS, int SETS = 1>
__device__ __forceinline__ void block_rank(const bool (&flag)[SETS * ITEMS], int (&wave_total)[SETS * (TPB / 64)], int* first, int* total) {
    const int tid = threadIdx.x, wave = tid >> 6;
    int below[SETS], in_wave[SETS];
#pragma unroll
    for (int s = 0; s < SETS; s++) below[s] = in_wave[s] = 0;
#pragma unroll
    for (int q = 0; q < ITEMS; q++) {
#pragma unroll
        for (int s = 0; s < SETS; s++) {
            const unsigned long long b = __ballot(flag[s * ITEMS + q]);
            below[s] += __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
            in_wave[s] += __popcll(b);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int s = 0; s < SETS; s++) wave_total[s * (TPB / 64) + wave] = in_wave[s];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SETS; s++) {
        int before = 0;
        total[s] = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; w++) {
            const int t = wave_total[s * (TPB / 64) + w];
            if (w < wave) before += t;
            total[s] += t;
        }
        first[s] = before + below[s];
    }
}

constexpr int SCAN_TPB = 1024;

// One workgroup: cnt[0 .. T) (chunk counts) -> exclusive offsets in place, cnt[T] = total; per-image counts when asked for.
// A thread owns a contiguous segment; the SCAN_TPB segment sums are scanned through LDS.
static __global__ __launch_bounds__(SCAN_TPB) void compact_scan_kernel(int* cnt, int T, int N, int nchunks, int* counts_img) {
    __shared__ int sh[2][SCAN_TPB];
    const int tid = threadIdx.x;
    const int seg = (T + SCAN_TPB - 1) / SCAN_TPB;
    const int lo = min(tid * seg, T), hi = min(lo + seg, T);
    int sum = 0;
    for (int k = lo; k < hi; k++) sum += cnt[k];
    int cur = 0;
    sh[0][tid] = sum;
    __syncthreads();
    for (int off = 1; off < SCAN_TPB; off <<= 1) {       // inclusive Hillis-Steele scan, double-buffered
        int val = sh[cur][tid];
        if (tid >= off) val += sh[cur][tid - off];
        sh[cur ^ 1][tid] = val;
        cur ^= 1;
        __syncthreads();
    }
    int run = sh[cur][tid] - sum;
    for (int k = lo; k < hi; k++) {
        const int t = cnt[k];
        cnt[k] = run;
        run += t;
    }
    if (tid == SCAN_TPB - 1) cnt[T] = sh[cur][tid];
    __syncthreads();                                     // the offsets are read back by other threads below
    if (counts_img)
        for (int n = tid; n < N; n += SCAN_TPB) counts_img[n] = cnt[(n + 1) * nchunks] - cnt[n * nchunks];
}

// ---- host side.  cnt holds T counts and the total: compact_offsets_bytes(T) bytes of a workspace.  T stays below 2^21 everywhere
// (2^31 items in chunks of 1024), so tid * seg of the scan stays inside an int.
static size_t compact_offsets_bytes(size_t T) { return align_up((T + 1) * sizeof(int), 256); }

// enqueues the scan; counts_img[n] = the items of image n's nchunks consecutive chunks when given
static void compact_scan(int* cnt, int T, hipStream_t st, int N = 0, int nchunks = 0, int* counts_img = nullptr) {
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, st, cnt, T, N, nchunks, counts_img);
}

// enqueues the copy of the total into *total_host, which holds it once the caller has synchronised the stream
static hipError_t compact_read_total(const int* cnt, int T, int* total_host, hipStream_t st) {
    return hipMemcpyAsync(total_host, cnt + T, sizeof(int), hipMemcpyDeviceToHost, st);
}

}  // namespace a3r
