// The scan between a counting pass and a placement pass (scene.hip: kept pixels and faces per chunk; voxel.hip: winners per chunk).
#pragma once
#include "common.h"

namespace a3r {

constexpr int SCAN_TPB = 1024;

// One workgroup: cnt[0 .. T) (chunk counts) -> exclusive offsets in place, cnt[T] = total; per-image counts when asked for.
// A thread owns a contiguous segment; the SCAN_TPB segment sums are scanned through LDS.
static __global__ __launch_bounds__(SCAN_TPB) void scene_scan_kernel(int* cnt, int T, int N, int nchunks, int* counts_img) {
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

}  // namespace a3r
