// Follows points through a clip for gfx950: 3-D tracks and scene flow by chaining the optical-flow fields of the scene's edges.
// The definition (include/a3r.h has it in full).  A chain is a list of steps (frame_from, frame_to, edge, reversed); the forward
// field of a step is reversed ? flow_b[edge] : flow_a[edge] and the backward field the other one.  In float64 on float64 copies,
// every operation rounded on its own:
//
//   bilinear(F, x, y):  x0 = floor(x), x1 = min(x0 + 1, W - 1), ax = x - x0  (y likewise)
//                       top = F[y0,x0] + ax * (F[y0,x1] - F[y0,x0]),  bot likewise on row y1,  val = top + ay * (bot - top)
//   a track starts at its seed, alive iff x, y are finite and inside [0, W-1] x [0, H-1]; it is recorded at t = 0, then per step:
//     f = bilinear(fwd, x, y);  xn = x + f.x, yn = y + f.y;        ends unless xn, yn are finite and inside the image
//     b = bilinear(bwd, xn, yn);  dx = f.x + b.x, dy = f.y + b.y;  ends unless dx * dx + dy * dy < fb_thr * fb_thr
//     (x, y) = (xn, yn), recorded at t = s + 1 in frame_to
//   record(t, n): col = rint(x), row = rint(y) (half to even), pix = row * W + col; state 2 where keep[n,pix] is set and xyz[n,pix]
//                 is finite (the point is copied), else 1 (followed, not visible: zeros); an ended track: state 0, pix -1, zeros.
//
// (this file is compiled with -ffp-contract=off: a product fused into the following sum would move a position across a half and
// the track into the neighbouring pixel, or a disagreement across the threshold).
// One kernel, one thread per (chain, track) with the steps in a loop: no atomics, no LDS, nothing allocated or synchronised.  A
// workgroup holds tracks of one chain, so a step's four integers are wave-uniform and come through scalar loads.  The outputs are
// planar, [C, S+1, M, ...]: at every t the threads of a wave store neighbouring tracks.  The gathers are the kernel's cost: eight
// fp32 words per field and position, sixteen per step; seeds that are neighbours in the image keep them in neighbouring lines.
#include "common.h"
#include <cmath>

namespace a3r {

constexpr int TK_TPB = 256;

// both channels of F [2,H,W] at (x, y), 0 <= x <= W - 1 and 0 <= y <= H - 1
__device__ __forceinline__ void track_bilinear(const float* __restrict__ F, double x, double y, int H, int W, double& vx, double& vy) {
    const double xf = floor(x), yf = floor(y);
    const int x0 = (int)xf, y0 = (int)yf;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const double ax = x - xf, ay = y - yf;
    const size_t plane = (size_t)H * W;
    const size_t r0 = (size_t)y0 * W, r1 = (size_t)y1 * W;
    double v[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float* G = F + plane * k;
        const double f00 = (double)G[r0 + x0], f01 = (double)G[r0 + x1], f10 = (double)G[r1 + x0], f11 = (double)G[r1 + x1];
        const double top = f00 + ax * (f01 - f00);
        const double bot = f10 + ax * (f11 - f10);
        v[k] = top + ay * (bot - top);
    }
    vx = v[0];
    vy = v[1];
}

// every comparison is false for a NaN operand, and an infinite coordinate is outside
__device__ __forceinline__ bool track_inside(double x, double y, int H, int W) {
    return x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1);
}

// o = (c * (S + 1) + t) * M + m: the track's slot in the planar outputs
__device__ __forceinline__ void track_record(bool alive, double x, double y, const float* __restrict__ xyz, const unsigned char* __restrict__ keep,
                                             int n, int H, int W, size_t o, float* __restrict__ out_xy, float* __restrict__ out_xyz,
                                             int* __restrict__ out_pix, unsigned char* __restrict__ out_state) {
    float px = 0.f, py = 0.f, pz = 0.f, ox = 0.f, oy = 0.f;
    int pix = -1;
    unsigned char state = 0;
    if (alive) {
        pix = (int)rint(y) * W + (int)rint(x);                       // inside: 0 <= rint(x) <= W - 1, and H * W < 2^31
        const size_t p = (size_t)n * H * W + pix;
        ox = (float)x;
        oy = (float)y;
        state = 1;
        if (keep[p]) {
            const float a = xyz[p * 3 + 0], b = xyz[p * 3 + 1], c = xyz[p * 3 + 2];
            if (fabsf(a) < INFINITY && fabsf(b) < INFINITY && fabsf(c) < INFINITY) {
                px = a; py = b; pz = c;
                state = 2;
            }
        }
    }
    out_xy[o * 2 + 0] = ox;
    out_xy[o * 2 + 1] = oy;
    out_xyz[o * 3 + 0] = px;
    out_xyz[o * 3 + 1] = py;
    out_xyz[o * 3 + 2] = pz;
    out_pix[o] = pix;
    out_state[o] = state;
}

// grid (C * ceil(M / TK_TPB)): workgroup b serves chain b / bpc and the tracks of block b % bpc
__global__ __launch_bounds__(TK_TPB) void track_points_kernel(const float* __restrict__ xyz, const unsigned char* __restrict__ keep, int H, int W,
                                                             const float* __restrict__ flow_a, const float* __restrict__ flow_b,
                                                             const int* __restrict__ steps, int S, const float* __restrict__ seeds, int M,
                                                             unsigned bpc, double thr2, float* __restrict__ out_xy,
                                                             float* __restrict__ out_xyz, int* __restrict__ out_pix,
                                                             unsigned char* __restrict__ out_state) {
    const int c = blockIdx.x / bpc;
    const int m = (int)(blockIdx.x % bpc) * TK_TPB + threadIdx.x;
    if (m >= M) return;
    double x, y;
    if (seeds) {
        x = (double)seeds[(size_t)m * 2 + 0];
        y = (double)seeds[(size_t)m * 2 + 1];
    } else {
        x = (double)(m % W);
        y = (double)(m / W);
    }
    bool alive = track_inside(x, y, H, W);
    const int* st = steps + (size_t)c * S * 4;                       // never read with S = 0
    const size_t field = (size_t)2 * H * W;
    size_t o = (size_t)c * (S + 1) * M + m;
    track_record(alive, x, y, xyz, keep, S > 0 ? st[0] : 0, H, W, o, out_xy, out_xyz, out_pix, out_state);
    for (int s = 0; s < S; s++) {
        const int to = st[s * 4 + 1], e = st[s * 4 + 2], rev = st[s * 4 + 3];
        if (alive) {
            const float* fwd = (rev ? flow_b : flow_a) + field * e;
            const float* bwd = (rev ? flow_a : flow_b) + field * e;
            double fx, fy, bx, by;
            track_bilinear(fwd, x, y, H, W, fx, fy);
            const double xn = x + fx, yn = y + fy;
            alive = track_inside(xn, yn, H, W);
            if (alive) {
                track_bilinear(bwd, xn, yn, H, W, bx, by);
                const double dx = fx + bx, dy = fy + by;
                alive = dx * dx + dy * dy < thr2;
                x = xn;
                y = yn;
            }
        }
        o += M;
        track_record(alive, x, y, xyz, keep, to, H, W, o, out_xy, out_xyz, out_pix, out_state);
    }
}

}  // namespace a3r

// =============================================================================================== host
using namespace a3r;

extern "C" int a3r_track_points(const float* xyz, const unsigned char* keep, int N, int H, int W, const float* flow_a, const float* flow_b,
                                int E, const int* steps_dev, const int* steps_host, int C, int S, const float* seeds, long long M,
                                double fb_thr, float* out_xy, float* out_xyz, int* out_pix, unsigned char* out_state, void* stream_) {
    const char* who = "a3r_track_points";
    hipStream_t stream = as_stream(stream_);
    A3R_CHECK_ARG(H > 0 && W > 0, "%s: the image size %d x %d must be positive", who, H, W);
    const long long hw = (long long)H * W;
    A3R_CHECK_ARG(hw < (1ll << 31), "%s: H * W = %d * %d must stay below 2^31", who, H, W);
    A3R_CHECK_ARG(N > 0 && E >= 0, "%s: N = %d frames must be positive and E = %d edges not negative", who, N, E);
    A3R_CHECK_ARG(C >= 0 && S >= 0, "%s: C = %d chains and S = %d steps must not be negative", who, C, S);
    A3R_CHECK_ARG(M >= 0 && M < (1ll << 31), "%s: M = %lld: the track count is in [0, 2^31)", who, M);
    A3R_CHECK_ARG(seeds || M == hw || M == 0, "%s: null seeds mean every pixel: M = %lld must be H * W = %lld", who, M, hw);
    // three factors below 2^31 each: the first product is below 2^62, the comparison by division keeps the second from overflowing
    A3R_CHECK_ARG(C == 0 || M == 0 || (long long)C * (S + 1ll) <= ((1ll << 31) - 1) / M,
                  "%s: C * (S + 1) * M = %d * %lld * %lld must stay below 2^31", who, C, S + 1ll, M);
    A3R_CHECK_ARG(!std::isnan(fb_thr) && fb_thr >= 0, "%s: fb_thr = %g must be a number >= 0 (inf switches the check off)", who, fb_thr);
    if (M == 0 || C == 0) return A3R_OK;
    A3R_CHECK_ARG(xyz && keep, "%s: null xyz / keep", who);
    A3R_CHECK_ARG(out_xy && out_xyz && out_pix && out_state, "%s: null output (xy, xyz, pix, state)", who);
    if (S > 0) {
        A3R_CHECK_ARG(flow_a && flow_b, "%s: null flow_a / flow_b", who);
        A3R_CHECK_ARG(steps_dev && steps_host, "%s: null steps_dev / steps_host", who);
        for (int c = 0; c < C; c++)
            for (int s = 0; s < S; s++) {
                const int* r = steps_host + ((size_t)c * S + s) * 4;
                A3R_CHECK_ARG(r[0] >= 0 && r[0] < N && r[1] >= 0 && r[1] < N,
                              "%s: chain %d step %d: frames %d -> %d are outside [0, %d)", who, c, s, r[0], r[1], N);
                A3R_CHECK_ARG(r[2] >= 0 && r[2] < E, "%s: chain %d step %d: edge %d is outside [0, %d)", who, c, s, r[2], E);
                A3R_CHECK_ARG(r[3] == 0 || r[3] == 1, "%s: chain %d step %d: reversed = %d is neither 0 nor 1", who, c, s, r[3]);
                A3R_CHECK_ARG(s == 0 || r[0] == r[-3], "%s: chain %d step %d: frame_from = %d does not continue frame_to = %d of step %d",
                              who, c, s, r[0], r[-3], s - 1);
            }
    }
    const unsigned bpc = (unsigned)((M + TK_TPB - 1) / TK_TPB);
    // C * bpc <= C * M < 2^31: inside the grid's first axis
    hipLaunchKernelGGL(track_points_kernel, dim3((unsigned)C * bpc), dim3(TK_TPB), 0, stream, xyz, keep, H, W, flow_a, flow_b, steps_dev, S,
                       seeds, (int)M, bpc, fb_thr * fb_thr, out_xy, out_xyz, out_pix, out_state);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
