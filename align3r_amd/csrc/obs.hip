// Packed fp16 storage of the aligner's pair observations (a3r_align_desc.obs_format = 1): the packer.
//
// The format, per edge side (one row of pred_i or pred_j [P, 3] with its weights [P]):
//   m = max |v| over the finite components of the row;  k = 0 if m == 0 or nothing is finite, else clamp(14 - ilogb(m), -100, 100),
//   so the largest finite magnitude lands in [2^14, 2^15) and rounds to at most 32768 (finite in fp16);
//   record of pixel p (8 bytes) = {half(x 2^k), half(y 2^k), half(z 2^k), half(w)}, round to nearest even, 2^k exact.
// Decoded, pred' = float(h) 2^-k and w' = float(h_w) are exact fp32 numbers; align.hip's packed kernels run the fp32 loop on them.
// align3r_amd/obs16.py restates the rule in numpy; the tests compare the two bit for bit.
#include "common.h"
#include <cmath>

namespace a3r {

constexpr int PACK_TPB = 1024;
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float finite_max(float m, float v) {
    const float a = fabsf(v);
    return a < INFINITY ? fmaxf(m, a) : m;      // NaN compares false
}

__device__ __forceinline__ f16x4 pack_record(float x, float y, float z, float w, int k) {
    return f16x4{(_Float16)ldexpf(x, k), (_Float16)ldexpf(y, k), (_Float16)ldexpf(z, k), (_Float16)w};
}

// One workgroup per row: the row's maximum (a maximum does not depend on the order: deterministic as it stands), then the conversion.
// The second pass re-reads a row that the first one has just pulled through the caches (a row is 16 P bytes, 3 MB at 384 x 512).
template <bool VEC>
__global__ __launch_bounds__(PACK_TPB) void align_pack_obs_kernel(const float* __restrict__ pred, const float* __restrict__ w, long P,
                                                                  f16x4* __restrict__ obs, int* __restrict__ exps) {
    __shared__ float sh[PACK_TPB / 64];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const float* X = pred + row * (size_t)P * 3;
    const float* Wt = w + row * (size_t)P;
    f16x4* O = obs + row * (size_t)P;
    float m = 0.f;
    if (VEC) {
        const f32x4* X4 = reinterpret_cast<const f32x4*>(X);
        const long n4 = P * 3 / 4;
        for (long q = tid; q < n4; q += PACK_TPB) {
            const f32x4 v = X4[q];
            m = finite_max(finite_max(finite_max(finite_max(m, v.x), v.y), v.z), v.w);
        }
    } else {
        for (long q = tid; q < P * 3; q += PACK_TPB) m = finite_max(m, X[q]);
    }
    m = wave_max(m);
    if ((tid & 63) == 0) sh[tid >> 6] = m;
    __syncthreads();
    m = sh[0];
#pragma unroll
    for (int i = 1; i < PACK_TPB / 64; i++) m = fmaxf(m, sh[i]);
    int k = 0;
    if (m > 0.f) {
        int e;
        frexpf(m, &e);                        // m = f 2^e, f in [0.5, 1): ilogb(m) = e - 1, subnormal m included
        k = min(max(14 - (e - 1), -100), 100);
    }
    if (tid == 0) exps[row] = k;
    if (VEC) {
        // four pixels per thread: three 16-byte loads of points, one of weights, two 16-byte stores
        const long nq = P / 4;
        for (long q = tid; q < nq; q += PACK_TPB) {
            const f32x4* xp = reinterpret_cast<const f32x4*>(X + q * 12);
            const f32x4 a = xp[0], b = xp[1], c = xp[2], ww = *reinterpret_cast<const f32x4*>(Wt + q * 4);
            const f16x4 r0 = pack_record(a.x, a.y, a.z, ww.x, k), r1 = pack_record(a.w, b.x, b.y, ww.y, k);
            const f16x4 r2 = pack_record(b.z, b.w, c.x, ww.z, k), r3 = pack_record(c.y, c.z, c.w, ww.w, k);
            f16x8* o = reinterpret_cast<f16x8*>(O + q * 4);
            o[0] = __builtin_shufflevector(r0, r1, 0, 1, 2, 3, 4, 5, 6, 7);
            o[1] = __builtin_shufflevector(r2, r3, 0, 1, 2, 3, 4, 5, 6, 7);
        }
    } else {
        for (long p = tid; p < P; p += PACK_TPB) O[p] = pack_record(X[p * 3], X[p * 3 + 1], X[p * 3 + 2], Wt[p], k);
    }
}

}  // namespace a3r

using namespace a3r;

extern "C" int a3r_align_pack_obs(const float* pred, const float* w, int rows, long P, void* obs, int32_t* exps, void* stream) {
    A3R_CHECK_ARG(pred && w && obs && exps, "a3r_align_pack_obs: null argument");
    A3R_CHECK_ARG(rows > 0 && P > 0, "a3r_align_pack_obs: rows and P must be positive (rows = %d, P = %ld)", rows, P);
    A3R_CHECK_ARG((reinterpret_cast<uintptr_t>(obs) & 7) == 0, "a3r_align_pack_obs: obs must be 8-byte aligned");
    hipStream_t st = as_stream(stream);
    const bool vec = P % 4 == 0 && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(obs)) & 15) == 0;
    f16x4* o = static_cast<f16x4*>(obs);
    if (vec) hipLaunchKernelGGL(align_pack_obs_kernel<true>, dim3(rows), dim3(PACK_TPB), 0, st, pred, w, P, o, exps);
    else hipLaunchKernelGGL(align_pack_obs_kernel<false>, dim3(rows), dim3(PACK_TPB), 0, st, pred, w, P, o, exps);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
