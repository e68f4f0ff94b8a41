// Renders a point cloud into pictures for gfx950: every point projected into every camera, square splats, a depth test by integer
// minimum.  The definition (include/a3r.h has it in full), per camera c and point m = (x, y, z) fp32, in float64 with every
// operation rounded on its own:
//
//   xc = (R00 * x + R01 * y) + R02 * z + t0   (yc, zc likewise);   u = fx * (xc / zc) + cx,  v = fy * (yc / zc) + cy;   zf = (float)zc
//   drawn  iff  zc >= near, zf finite, u and v finite, |u|, |v| < 2^30
//   col = (int)rint(u), row = (int)rint(v)  (half to even);  footprint = the pixels (row + dy, col + dx), |dx|, |dy| <= radius, inside
//   every footprint pixel takes  key = (bits(zf) << 32) | m;   the pixel's result is the MINIMUM key
//
// (this file is compiled with -ffp-contract=off: a product fused into the following sum would move u across a rounding boundary and
// the point into the neighbouring pixel).  zf > 0, so the bits of zf order as zf does: the minimum key is the nearest point and, at
// equal zf, the lowest point index.  A minimum of integers does not depend on the order of its operands, so the picture is a
// function of the inputs alone although the splat runs on atomics.
// Three kernels in stream order:
//   * fill: every key of the planes [n_cams, H, W] becomes all ones (no drawn point has that key: bits(zf) < 0x7f800000).
//   * splat: a thread owns one point.  Forms (a3r_render_set_form; DESIGN 6.13 has the measurements):
//       camera loop  -- grid (point blocks): the point stays in registers and the thread walks the cameras, whose 16 doubles come
//                       through scalar loads (the camera index is wave-uniform);
//       camera axis  -- grid (point blocks, cameras): more workgroups for a small cloud, the points are read once per camera.
//     Before its atomic a thread reads the pixel's current key (an agent-scope load, served by L2 where the atomics land) and skips
//     the atomic when that key is already at or below its own: keys only decrease, so a skipped atomic would not have changed the
//     word -- even a stale value read there is an upper bound of the current one.  With many more points than pixels almost every
//     atomic is skipped.  A footprint of more than one pixel is walked in batches of RD_BATCH pixels: the batch's reads are issued
//     together and waited for once, then come the atomics that are still needed -- one memory latency per batch instead of one
//     per pixel (the wait of a read also waits for the atomics issued before it).  The other forms read one pixel at a time, or
//     issue every atomic without reading.
//   * resolve: a thread owns one pixel: key -> depth (the high word's float, 0 when empty), index (the low word, -1), colour
//     (rgb[m], background).
#include "common.h"
#include <cmath>

namespace a3r {

constexpr int RD_TPB = 256;
constexpr int RD_MAX_RADIUS = 8;
constexpr unsigned long long RD_EMPTY = ~0ull;
constexpr int RD_BATCH = 9;                     // footprint pixels whose keys are read together: the whole footprint at radius 1
constexpr int RD_FORM_CAM_AXIS = 1;             // bit 0: a grid axis over the cameras instead of the loop inside the thread
constexpr int RD_FORM_NO_READ = 2;              // bit 1: every atomic is issued, no read of the current key first
constexpr int RD_FORM_READ_ONE = 4;             // bit 2: the keys are read one pixel at a time instead of RD_BATCH at a time
constexpr int RD_FORM_MAX = 7;

static std::atomic<int> g_render_form{0};

// n2 = number of 16-byte pairs of keys; an odd last key is written by thread 0
__global__ __launch_bounds__(RD_TPB) void render_fill_kernel(unsigned long long* __restrict__ keys, long long n) {
    const long long i = (long long)blockIdx.x * RD_TPB + threadIdx.x;
    const long long n2 = n >> 1;
    if (i < n2) reinterpret_cast<ulonglong2*>(keys)[i] = make_ulonglong2(RD_EMPTY, RD_EMPTY);
    if (i == 0 && (n & 1)) keys[n - 1] = RD_EMPTY;
}

// One point into one camera: the footprint's atomics on `plane` [H, W].
// BATCH: 0 = no read before the atomic; otherwise the number of footprint pixels whose keys are read together.
template <int BATCH>
__device__ __forceinline__ void splat_one(const a3r_render_cam& cam, double x, double y, double z, unsigned m, int H, int W, int radius,
                                          double near_z, unsigned long long* __restrict__ plane) {
    const double* R = cam.w2c;
    const double xc = (R[0] * x + R[1] * y) + R[2] * z + R[3];
    const double yc = (R[4] * x + R[5] * y) + R[6] * z + R[7];
    const double zc = (R[8] * x + R[9] * y) + R[10] * z + R[11];
    const double u = cam.fx * (xc / zc) + cam.cx;
    const double v = cam.fy * (yc / zc) + cam.cy;
    const float zf = (float)zc;
    const double lim = 1073741824.0;             // 2^30: rint(u) fits an int with room for the radius
    // every comparison is false for a NaN operand
    if (!(zc >= near_z && zf < INFINITY && fabs(u) < lim && fabs(v) < lim)) return;
    const int col = (int)rint(u), row = (int)rint(v);
    const int r0 = max(row - radius, 0), r1 = min(row + radius, H - 1);
    const int c0 = max(col - radius, 0), c1 = min(col + radius, W - 1);
    if (r0 > r1 || c0 > c1) return;              // the footprint misses the picture
    const unsigned long long key = ((unsigned long long)__float_as_uint(zf) << 32) | m;
    if constexpr (BATCH == 0) {
        for (int r = r0; r <= r1; r++)
            for (int c = c0; c <= c1; c++) atomicMin(plane + ((size_t)r * W + c), key);
    } else {
        // the footprint's pixels in row-major order, BATCH at a time; (rr, cc) walks them
        const int n = (r1 - r0 + 1) * (c1 - c0 + 1);             // at most 17 * 17
        int rr = r0, cc = c0;
        for (int k = 0; k < n; k += BATCH) {
            unsigned off[BATCH];                                 // rr * W + cc, inside the plane (H * W < 2^31)
            unsigned long long cur[BATCH];
            // The reads carry no branch, so that they are issued back to back and waited for once: a slot beyond the footprint
            // reads the footprint's first pixel again (inside the plane) and its value is dropped.
#pragma unroll
            for (int j = 0; j < BATCH; j++) {
                off[j] = k + j < n ? (unsigned)rr * (unsigned)W + (unsigned)cc : (unsigned)r0 * (unsigned)W + (unsigned)c0;
                cur[j] = __hip_atomic_load(plane + off[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (++cc > c1) { cc = c0; rr++; }
            }
#pragma unroll
            for (int j = 0; j < BATCH; j++)
                if (k + j < n && cur[j] > key) atomicMin(plane + off[j], key);
        }
    }
}

// CAM_AXIS = false: grid (ceil(M / RD_TPB)), the thread walks cameras 0 .. n_cams - 1.  true: grid (ceil(M / RD_TPB), n_cams).
template <bool CAM_AXIS, int BATCH>
__global__ __launch_bounds__(RD_TPB) void render_splat_kernel(const float* __restrict__ xyz, int M, const a3r_render_cam* __restrict__ cams,
                                                             int n_cams, int H, int W, int radius, double near_z,
                                                             unsigned long long* __restrict__ keys) {
    const long long m = (long long)blockIdx.x * RD_TPB + threadIdx.x;
    if (m >= M) return;
    const double x = (double)xyz[(size_t)m * 3 + 0], y = (double)xyz[(size_t)m * 3 + 1], z = (double)xyz[(size_t)m * 3 + 2];
    const size_t plane = (size_t)H * W;
    if (CAM_AXIS) {
        const int c = blockIdx.y;
        splat_one<BATCH>(cams[c], x, y, z, (unsigned)m, H, W, radius, near_z, keys + plane * c);
    } else {
        for (int c = 0; c < n_cams; c++) splat_one<BATCH>(cams[c], x, y, z, (unsigned)m, H, W, radius, near_z, keys + plane * c);
    }
}

// one thread per pixel of [n_cams, H, W]
__global__ __launch_bounds__(RD_TPB) void render_resolve_kernel(const unsigned long long* __restrict__ keys, long long n,
                                                               const unsigned char* __restrict__ rgb, unsigned bg0, unsigned bg1, unsigned bg2,
                                                               float* __restrict__ depth, unsigned char* __restrict__ out_rgb,
                                                               int* __restrict__ index) {
    const long long i = (long long)blockIdx.x * RD_TPB + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    const bool hit = key != RD_EMPTY;
    const unsigned m = (unsigned)key;
    depth[i] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    if (index) index[i] = hit ? (int)m : -1;
    if (out_rgb) {
        out_rgb[(size_t)i * 3 + 0] = hit ? rgb[(size_t)m * 3 + 0] : (unsigned char)bg0;
        out_rgb[(size_t)i * 3 + 1] = hit ? rgb[(size_t)m * 3 + 1] : (unsigned char)bg1;
        out_rgb[(size_t)i * 3 + 2] = hit ? rgb[(size_t)m * 3 + 2] : (unsigned char)bg2;
    }
}

static bool render_sizes_ok(int n_cams, int H, int W) {
    if (n_cams <= 0 || H <= 0 || W <= 0) return false;
    const long long hw = (long long)H * W;                       // below 2^62
    return hw < (1ll << 31) && hw * n_cams < (1ll << 31);        // then the product is below 2^62 as well
}

}  // namespace a3r

// =============================================================================================== host
using namespace a3r;

extern "C" int a3r_render_set_form(int form) {
    const int old = g_render_form.load();
    if (form >= 0 && form <= RD_FORM_MAX) g_render_form.store(form);
    return old;
}

extern "C" size_t a3r_render_workspace_bytes(int n_cams, int H, int W) {
    if (!render_sizes_ok(n_cams, H, W)) return 0;
    return align_up((size_t)n_cams * H * W * sizeof(unsigned long long), 256);
}

extern "C" int a3r_render_points(const float* xyz, const unsigned char* rgb, long long M, const a3r_render_cam* cams_dev,
                                 const a3r_render_cam* cams_host, int n_cams, int H, int W, int radius, double near_z,
                                 const unsigned char background[3], void* ws, size_t ws_bytes, float* depth, unsigned char* out_rgb,
                                 int* index, void* stream_) {
    const char* who = "a3r_render_points";
    hipStream_t stream = as_stream(stream_);
    A3R_CHECK_ARG(M >= 0 && M < (1ll << 31), "%s: M = %lld: the point count is in [0, 2^31)", who, M);
    A3R_CHECK_ARG(n_cams > 0, "%s: n_cams = %d must be positive", who, n_cams);
    A3R_CHECK_ARG(H > 0 && W > 0, "%s: the image size %d x %d must be positive", who, H, W);
    A3R_CHECK_ARG(render_sizes_ok(n_cams, H, W), "%s: n_cams * H * W = %d * %d * %d must stay below 2^31", who, n_cams, H, W);
    A3R_CHECK_ARG(radius >= 0 && radius <= RD_MAX_RADIUS, "%s: radius = %d is outside [0, %d]", who, radius, RD_MAX_RADIUS);
    A3R_CHECK_ARG(std::isfinite(near_z) && near_z > 0, "%s: near_z = %g must be finite and positive", who, near_z);
    A3R_CHECK_ARG(xyz || M == 0, "%s: null xyz", who);
    A3R_CHECK_ARG(cams_dev && cams_host, "%s: null cams_dev / cams_host", who);
    A3R_CHECK_ARG(depth, "%s: null depth", who);
    A3R_CHECK_ARG(!out_rgb || rgb || M == 0, "%s: out_rgb needs rgb", who);
    A3R_CHECK_ARG(!out_rgb || background, "%s: null background", who);
    for (int c = 0; c < n_cams; c++) {
        const double* e = cams_host[c].w2c;          // 12 + 4 doubles, contiguous in the struct
        for (int k = 0; k < 16; k++)
            A3R_CHECK_ARG(std::isfinite(e[k]), "%s: camera %d: entry %d (w2c[0..11], fx, fy, cx, cy) is not finite", who, c, k);
    }
    const size_t need = a3r_render_workspace_bytes(n_cams, H, W);
    if (int rc = check_workspace(who, ws, ws_bytes, need)) return rc;

    unsigned long long* keys = static_cast<unsigned long long*>(ws);
    const long long n = (long long)n_cams * H * W;
    const int form = g_render_form.load();
    const dim3 tpb(RD_TPB);
    hipLaunchKernelGGL(render_fill_kernel, dim3((unsigned)(((n + 1) / 2 + RD_TPB - 1) / RD_TPB)), tpb, 0, stream, keys, n);
    if (M > 0) {
        const unsigned pb = (unsigned)((M + RD_TPB - 1) / RD_TPB);
        // the second grid axis holds at most 65535 workgroups: beyond that the loop form takes over
        const bool axis = (form & RD_FORM_CAM_AXIS) != 0 && n_cams <= 65535;
        const int batch = (form & RD_FORM_NO_READ) ? 0 : (form & RD_FORM_READ_ONE) || radius == 0 ? 1 : RD_BATCH;
        const dim3 grid(pb, axis ? n_cams : 1);
#define A3R_RD_SPLAT(AX, BT) \
        hipLaunchKernelGGL((render_splat_kernel<AX, BT>), grid, tpb, 0, stream, xyz, (int)M, cams_dev, n_cams, H, W, radius, near_z, keys)
#define A3R_RD_SPLAT_READ(AX) \
        do { if (batch == RD_BATCH) A3R_RD_SPLAT(AX, RD_BATCH); else if (batch == 1) A3R_RD_SPLAT(AX, 1); else A3R_RD_SPLAT(AX, 0); } while (0)
        if (axis) A3R_RD_SPLAT_READ(true); else A3R_RD_SPLAT_READ(false);
#undef A3R_RD_SPLAT_READ
#undef A3R_RD_SPLAT
    }
    const unsigned char* bg = background;
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((n + RD_TPB - 1) / RD_TPB)), tpb, 0, stream, keys, n, rgb,
                       out_rgb ? bg[0] : 0u, out_rgb ? bg[1] : 0u, out_rgb ? bg[2] : 0u, depth, out_rgb, index);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
