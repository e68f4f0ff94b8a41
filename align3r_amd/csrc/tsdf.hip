// TSDF fusion of depth maps into a dense voxel grid, and the grid's zero surface as one triangle mesh (surface nets), for gfx950.
// The definition (include/a3r.h has it in full), float64 with every operation rounded on its own (this file is compiled with
// -ffp-contract=off):
//
//   voxel (i, j, k):  X = ox + ((double)i + 0.5) * voxel  (Y, Z likewise),  linear index (k * ny + j) * nx + i
//   per frame n = 0 .. N - 1, ascending:  xc = (R00 * X + R01 * Y) + R02 * Z + t0  (yc, zc likewise),  u = fx * (xc / zc) + cx
//     gates:  zc >= near,  |u|, |v| < 2^30,  col = rint(u) in [0, w),  row = rint(v) in [0, h);   p = n * P + row * w + col
//             d = depth[p], wd = weight[p] finite,  wd > 0,  d > 0,  d <= max_depth;   sdf = d - zc >= -trunc
//     W += wd,  S += wd * min(1, sdf / trunc);   where sdf <= trunc and colours are given:  Wc += wd,  C[ch] += wd * rgb[p][ch]
//   tsdf = (float)(S / W) (1 where W == 0),  wsum = (float)W,  out_rgb = min(rint(C / Wc), 255) (0 where Wc == 0)
//
// Integration: a thread owns one voxel and walks the frames with its six sums in registers; every output element is written once,
// there are no atomics, and the sums are sequential in frame order, so the result is bitwise the numpy restatement
// (tests/tsdf_cases.py).  A workgroup owns a brick of TS_BX x TS_BY voxels of one z slice, x the fast thread axis: the depth gathers
// of a wave fall on neighbouring pixels and the outputs are written coalesced.  The frame index is wave-uniform, so the camera's
// 18 words come through scalar loads.  Brick test (form bit 0 clear): before the walk, thread t of the workgroup projects the eight
// corners of the brick's box of voxel centres into frame base + t and proves, with margins far above the rounding error, that
// either every voxel lies behind `near` or every voxel projects outside the image by more than a pixel; the frames that survive
// are a bit mask (wave ballots through LDS) that every thread walks in ascending order.  A skipped frame is one that no voxel of
// the brick could have passed gate 2 in, so the sums do not depend on the test.
//
// Surface: cells of 2 x 2 x 2 voxels whose corners are all observed (wsum >= min_weight) and differ in sign carry one vertex, the
// mean of the zero crossings of the cell's edges; a grid edge whose ends differ in sign carries a quad between the vertices of its
// four cells.  Compaction by the count / scan / place scheme of compact.h, the count pass leaving a rank map; vertex ids are
// the ranks of the active cells in linear order, faces are ordered by (voxel, axis).
#include "common.h"
#include "compact.h"
#include <cmath>

namespace a3r {

constexpr int TS_TPB = 256;
constexpr int TS_BX = 32, TS_BY = 8;            // the brick: TS_BX x TS_BY x 1 voxels, thread (tid & 31, tid >> 5)
constexpr int TS_FORM_NO_SKIP = 1;              // bit 0: no brick test, every voxel walks every frame
constexpr int TS_FORM_MAX = 1;
constexpr int TM_PPT = 4;                       // consecutive voxels per thread of the surface passes
constexpr int TM_CHUNK = TS_TPB * TM_PPT;
constexpr long long TM_MAX_VOXELS = (1ll << 31) / 6;   // three quads = six triangles per voxel at most: the face count stays an int

static std::atomic<int> g_tsdf_form{0};

struct TsdfGrid {
    double ox, oy, oz, voxel;
    int nx, ny, nz;
};

struct TsdfArgs {
    const float* depth;             // [N, P]
    const float* weight;            // [N, P]
    const unsigned char* rgb;       // [N, P, 3] or null
    const a3r_tsdf_cam* cams;       // [N]
    int N;
    long long P;
    TsdfGrid g;
    double trunc, near_z, max_depth;
    float* tsdf;                    // [nz, ny, nx]
    float* wsum;
    unsigned char* out_rgb;         // [nz, ny, nx, 3] or null
    unsigned long long* stats;      // [2] or null: brick-frames tested, brick-frames skipped (a measurement, not a result)
    int nbx, nby;
};

struct TsdfSums {
    double W, S, Wc, C0, C1, C2;
};

// One voxel against one frame: steps 1 to 6 of the definition.
template <bool RGB>
__device__ __forceinline__ void tsdf_frame(const TsdfArgs& a, const a3r_tsdf_cam& cam, int n, bool live, double X, double Y, double Z,
                                           TsdfSums& s) {
    const double* R = cam.w2c;
    const double xc = (R[0] * X + R[1] * Y) + R[2] * Z + R[3];
    const double yc = (R[4] * X + R[5] * Y) + R[6] * Z + R[7];
    const double zc = (R[8] * X + R[9] * Y) + R[10] * Z + R[11];
    const double u = cam.fx * (xc / zc) + cam.cx;
    const double v = cam.fy * (yc / zc) + cam.cy;
    const double lim = 1073741824.0;             // 2^30
    // every comparison is false for a NaN operand
    if (!(live && zc >= a.near_z && fabs(u) < lim && fabs(v) < lim)) return;
    const int col = (int)rint(u), row = (int)rint(v);
    if (col < 0 || col >= cam.w || row < 0 || row >= cam.h) return;
    const size_t p = (size_t)n * (size_t)a.P + (size_t)row * (size_t)cam.w + (size_t)col;
    const double d = (double)a.depth[p], wd = (double)a.weight[p];
    if (!(wd > 0.0 && wd < INFINITY && d > 0.0 && d < INFINITY && d <= a.max_depth)) return;
    const double sdf = d - zc;
    if (sdf < -a.trunc) return;
    const double t = fmin(1.0, sdf / a.trunc);
    s.W += wd;
    s.S += wd * t;
    if (RGB && sdf <= a.trunc) {
        const unsigned char* c = a.rgb + p * 3;
        s.Wc += wd;
        s.C0 += wd * (double)c[0];
        s.C1 += wd * (double)c[1];
        s.C2 += wd * (double)c[2];
    }
}

// The brick test: true where no voxel whose centre lies in the box [x0, x1] x [y0, y1] x [z0, z1] can pass gate 2 of frame `cam`.
// zc and, in front of the camera, u and v of a box lie between their values at the box's corners.  The computed values differ from
// the exact ones by a few ulp of `mag`, the sum of the magnitudes that enter them; the margins are 10^6 times that and one pixel.
__device__ __forceinline__ bool tsdf_brick_skips(const a3r_tsdf_cam& cam, const double (&bx)[2], const double (&by)[2], const double (&bz)[2],
                                                 double near_z) {
    const double* R = cam.w2c;
    const double ax = fmax(fabs(bx[0]), fabs(bx[1])), ay = fmax(fabs(by[0]), fabs(by[1])), az = fmax(fabs(bz[0]), fabs(bz[1]));
    double mag = 1.0;
#pragma unroll
    for (int r = 0; r < 3; r++) mag = fmax(mag, fabs(R[4 * r]) * ax + fabs(R[4 * r + 1]) * ay + fabs(R[4 * r + 2]) * az + fabs(R[4 * r + 3]));
    double xc[8], yc[8], zc[8];
    double zmin = INFINITY, zmax = -INFINITY;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const double X = bx[c & 1], Y = by[(c >> 1) & 1], Z = bz[c >> 2];
        xc[c] = (R[0] * X + R[1] * Y) + R[2] * Z + R[3];
        yc[c] = (R[4] * X + R[5] * Y) + R[6] * Z + R[7];
        zc[c] = (R[8] * X + R[9] * Y) + R[10] * Z + R[11];
        zmin = fmin(zmin, zc[c]);
        zmax = fmax(zmax, zc[c]);
    }
    if (!(mag < INFINITY) || zmin != zmin || zmax != zmax) return false;
    if (zmax < near_z - 1e-9 * mag) return true;            // every voxel is behind the near plane
    if (!(zmin > 1e-6 * mag)) return false;                 // the box is not safely in front of the camera: no statement about u, v
    double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const double u = cam.fx * (xc[c] / zc[c]) + cam.cx, v = cam.fy * (yc[c] / zc[c]) + cam.cy;
        umin = fmin(umin, u); umax = fmax(umax, u);
        vmin = fmin(vmin, v); vmax = fmax(vmax, v);
    }
    if (umin != umin || umax != umax || vmin != vmin || vmax != vmax) return false;
    const double mu = 1.0 + 1e-6 * (fabs(cam.fx) + fmax(fabs(umin), fabs(umax)));
    const double mv = 1.0 + 1e-6 * (fabs(cam.fy) + fmax(fabs(vmin), fabs(vmax)));
    return umax < -0.5 - mu || umin > ((double)cam.w - 0.5) + mu || vmax < -0.5 - mv || vmin > ((double)cam.h - 0.5) + mv;
}

// grid (nbx * nby * nz): workgroup b owns the brick (b % nbx, (b / nbx) % nby) of slice b / (nbx * nby).
template <bool SKIP, bool RGB>
__global__ __launch_bounds__(TS_TPB) void tsdf_integrate_kernel(TsdfArgs a) {
    __shared__ unsigned long long sh_mask[TS_TPB / 64];
    const int tid = threadIdx.x;
    const unsigned b = blockIdx.x;
    const int bi = (int)(b % (unsigned)a.nbx), bj = (int)((b / (unsigned)a.nbx) % (unsigned)a.nby), k = (int)(b / ((unsigned)a.nbx * (unsigned)a.nby));
    const int i = bi * TS_BX + (tid & (TS_BX - 1)), j = bj * TS_BY + tid / TS_BX;
    const bool live = i < a.g.nx && j < a.g.ny;
    const double X = a.g.ox + ((double)i + 0.5) * a.g.voxel;
    const double Y = a.g.oy + ((double)j + 0.5) * a.g.voxel;
    const double Z = a.g.oz + ((double)k + 0.5) * a.g.voxel;
    TsdfSums s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const a3r_tsdf_cam* __restrict__ cams = a.cams;
    if (SKIP) {
        // the box of the brick's voxel centres: the centre is monotonic in the index, rounding included
        const int i0 = bi * TS_BX, i1 = min(i0 + TS_BX, a.g.nx) - 1, j0 = bj * TS_BY, j1 = min(j0 + TS_BY, a.g.ny) - 1;
        const double bx[2] = {a.g.ox + ((double)i0 + 0.5) * a.g.voxel, a.g.ox + ((double)i1 + 0.5) * a.g.voxel};
        const double by[2] = {a.g.oy + ((double)j0 + 0.5) * a.g.voxel, a.g.oy + ((double)j1 + 0.5) * a.g.voxel};
        const double bz[2] = {Z, Z};
        unsigned skipped = 0;
        for (int base = 0; base < a.N; base += TS_TPB) {
            const int mine = base + tid;
            const bool walk = mine < a.N && !tsdf_brick_skips(cams[mine], bx, by, bz, a.near_z);
            const unsigned long long m = __ballot(walk);
            if ((tid & 63) == 0) sh_mask[tid >> 6] = m;
            __syncthreads();
#pragma unroll 1
            for (int w = 0; w < TS_TPB / 64; w++) {
                const unsigned long long full = sh_mask[w];
                unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)full), hi = __builtin_amdgcn_readfirstlane((unsigned)(full >> 32));
                skipped += (unsigned)(min(max(a.N - base - w * 64, 0), 64) - __popc(lo) - __popc(hi));
                while (lo) {
                    const int n = base + w * 64 + __builtin_ctz(lo);
                    lo &= lo - 1;
                    tsdf_frame<RGB>(a, cams[n], n, live, X, Y, Z, s);
                }
                while (hi) {
                    const int n = base + w * 64 + 32 + __builtin_ctz(hi);
                    hi &= hi - 1;
                    tsdf_frame<RGB>(a, cams[n], n, live, X, Y, Z, s);
                }
            }
            __syncthreads();            // the masks are rewritten by the next round
        }
        if (a.stats && tid == 0) {
            atomicAdd(a.stats, (unsigned long long)a.N);
            atomicAdd(a.stats + 1, (unsigned long long)skipped);
        }
    } else {
        for (int n = 0; n < a.N; n++) tsdf_frame<RGB>(a, cams[n], n, live, X, Y, Z, s);
        if (a.stats && tid == 0) atomicAdd(a.stats, (unsigned long long)a.N);
    }
    if (!live) return;
    const size_t lin = ((size_t)k * a.g.ny + j) * a.g.nx + i;
    a.tsdf[lin] = s.W == 0.0 ? 1.0f : (float)(s.S / s.W);
    a.wsum[lin] = (float)s.W;
    if (a.out_rgb) {
        const bool any = RGB && s.Wc != 0.0;
        a.out_rgb[lin * 3 + 0] = any ? (unsigned char)fmin(rint(s.C0 / s.Wc), 255.0) : (unsigned char)0;
        a.out_rgb[lin * 3 + 1] = any ? (unsigned char)fmin(rint(s.C1 / s.Wc), 255.0) : (unsigned char)0;
        a.out_rgb[lin * 3 + 2] = any ? (unsigned char)fmin(rint(s.C2 / s.Wc), 255.0) : (unsigned char)0;
    }
}

// ------------------------------------------------------------------------------------------- surface
struct TsdfMesh {
    const float* tsdf;
    const float* wsum;
    const unsigned char* rgb;       // [nvox, 3] or null
    TsdfGrid g;
    double min_weight;
    long long nvox;
    int* voff;                      // [T + 1]: active cells per chunk, then their offsets
    int* foff;                      // [T + 1]: quads per chunk, then their offsets
    int* rank;                      // [nvox]: an active cell's rank inside its chunk, -1 otherwise
    float* out_xyz;                 // [V, 3]
    unsigned char* out_rgb;         // [V, 3] or null
    int* out_faces;                 // [F, 3]
};

__device__ __forceinline__ bool tsdf_inside(float f) { return f < 0.0f; }

// voxel l -> (i, j, k)
__device__ __forceinline__ void tsdf_unravel(const TsdfGrid& g, long long l, int& i, int& j, int& k) {
    i = (int)(l % g.nx);
    const long long r = l / g.nx;
    j = (int)(r % g.ny);
    k = (int)(r / g.ny);
}

// the cell whose corner 0 is voxel (i, j, k): active iff it exists, all corners are observed and their signs differ; f = the corners
__device__ __forceinline__ bool tsdf_cell_active(const TsdfMesh& m, int i, int j, int k, float (&f)[8]) {
    if (i >= m.g.nx - 1 || j >= m.g.ny - 1 || k >= m.g.nz - 1) return false;
    bool observed = true, any_in = false, any_out = false;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const size_t l = ((size_t)(k + (c >> 2)) * m.g.ny + (j + ((c >> 1) & 1))) * m.g.nx + (i + (c & 1));
        f[c] = m.tsdf[l];
        observed = observed && (double)m.wsum[l] >= m.min_weight;
        any_in = any_in || tsdf_inside(f[c]);
        any_out = any_out || !tsdf_inside(f[c]);
    }
    return observed && any_in && any_out;
}

// grid (T).  WRITE = false: rank[l] = the cell's rank inside the chunk or -1, voff[chunk] = active cells of the chunk.
// WRITE = true: the vertex of every active cell goes to row voff[chunk] + rank.
template <bool WRITE>
__global__ __launch_bounds__(TS_TPB) void tsdf_cells_kernel(TsdfMesh m) {
    __shared__ int wave_total[TS_TPB / 64];
    const long long l0 = (long long)blockIdx.x * TM_CHUNK + threadIdx.x * TM_PPT;
    bool act[TM_PPT];
    float f[TM_PPT][8];
    int ci[TM_PPT], cj[TM_PPT], ck[TM_PPT];
#pragma unroll
    for (int q = 0; q < TM_PPT; q++) {
        act[q] = false;
        ci[q] = cj[q] = ck[q] = 0;
        if (l0 + q < m.nvox) {
            tsdf_unravel(m.g, l0 + q, ci[q], cj[q], ck[q]);
            act[q] = tsdf_cell_active(m, ci[q], cj[q], ck[q], f[q]);
        }
    }
    int first, total;
    block_rank<TS_TPB, TM_PPT>(act, wave_total, &first, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) m.voff[blockIdx.x] = total;
        int r = first;
#pragma unroll
        for (int q = 0; q < TM_PPT; q++)
            if (l0 + q < m.nvox) m.rank[l0 + q] = act[q] ? r++ : -1;
        return;
    }
    const long long end = m.voff[blockIdx.x + 1];        // stay inside the chunk's range whatever the workspace holds
    long long row = (long long)m.voff[blockIdx.x] + first;
#pragma unroll
    for (int q = 0; q < TM_PPT; q++) {
        if (!act[q] || row >= end) continue;
        // the mean of the crossings of the 12 edges (a, b), a < b differing in one bit, in lexicographic order
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int cnt = 0;
#pragma unroll
        for (int ca = 0; ca < 8; ca++) {
#pragma unroll
            for (int bit = 0; bit < 3; bit++) {
                const int cb = ca | (1 << bit);
                if (cb == ca) continue;
                const float fa = f[q][ca], fb = f[q][cb];
                if (tsdf_inside(fa) == tsdf_inside(fb)) continue;
                const double t = (double)fa / ((double)fa - (double)fb);
                const double ax = (double)(ca & 1), ay = (double)((ca >> 1) & 1), az = (double)(ca >> 2);
                sx += ax + t * ((double)(cb & 1) - ax);
                sy += ay + t * ((double)((cb >> 1) & 1) - ay);
                sz += az + t * ((double)(cb >> 2) - az);
                cnt++;
            }
        }
        const double n = (double)cnt;
        m.out_xyz[row * 3 + 0] = (float)(m.g.ox + (((double)ci[q] + 0.5) + sx / n) * m.g.voxel);
        m.out_xyz[row * 3 + 1] = (float)(m.g.oy + (((double)cj[q] + 0.5) + sy / n) * m.g.voxel);
        m.out_xyz[row * 3 + 2] = (float)(m.g.oz + (((double)ck[q] + 0.5) + sz / n) * m.g.voxel);
        if (m.out_rgb) {
            unsigned sum[3] = {0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const size_t l = ((size_t)(ck[q] + (c >> 2)) * m.g.ny + (cj[q] + ((c >> 1) & 1))) * m.g.nx + (ci[q] + (c & 1));
#pragma unroll
                for (int ch = 0; ch < 3; ch++) sum[ch] += m.rgb[l * 3 + ch];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) m.out_rgb[row * 3 + ch] = (unsigned char)((2u * sum[ch] + 8u) / 16u);
        }
        row++;
    }
}

// grid (T), after tsdf_cells_kernel<false>.  WRITE = false: foff[chunk] = quads of the chunk's voxels.  WRITE = true (after the
// scans): every quad's two triangles go to rows 2 (foff[chunk] + rank) and the next, vertex ids = voff[chunk of cell] + rank[cell].
template <bool WRITE>
__global__ __launch_bounds__(TS_TPB) void tsdf_faces_kernel(TsdfMesh m) {
    __shared__ int wave_total[TS_TPB / 64];
    const long long l0 = (long long)blockIdx.x * TM_CHUNK + threadIdx.x * TM_PPT;
    const long long step[3] = {1, m.g.nx, (long long)m.g.nx * m.g.ny};
    const int dims[3] = {m.g.nx, m.g.ny, m.g.nz};
    bool quad[TM_PPT * 3];
    bool in_g[TM_PPT];
#pragma unroll
    for (int q = 0; q < TM_PPT; q++) {
        const long long l = l0 + q;
        in_g[q] = false;
#pragma unroll
        for (int a = 0; a < 3; a++) quad[q * 3 + a] = false;
        if (l >= m.nvox) continue;
        int g[3];
        tsdf_unravel(m.g, l, g[0], g[1], g[2]);
        in_g[q] = tsdf_inside(m.tsdf[l]);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int bb = (a + 1) % 3, cc = (a + 2) % 3;
            if (g[a] + 1 >= dims[a] || g[bb] < 1 || g[bb] > dims[bb] - 2 || g[cc] < 1 || g[cc] > dims[cc] - 2) continue;
            if (tsdf_inside(m.tsdf[l + step[a]]) == in_g[q]) continue;
            quad[q * 3 + a] = m.rank[l - step[bb] - step[cc]] >= 0 && m.rank[l - step[cc]] >= 0 && m.rank[l] >= 0 && m.rank[l - step[bb]] >= 0;
        }
    }
    int first, total;
    block_rank<TS_TPB, TM_PPT * 3>(quad, wave_total, &first, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) m.foff[blockIdx.x] = total;
        return;
    }
    const long long end = m.foff[blockIdx.x + 1];
    long long row = (long long)m.foff[blockIdx.x] + first;
#pragma unroll
    for (int q = 0; q < TM_PPT; q++) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!quad[q * 3 + a] || row >= end) continue;
            const int bb = (a + 1) % 3, cc = (a + 2) % 3;
            const long long l = l0 + q;
            const long long cell[4] = {l - step[bb] - step[cc], l - step[cc], l, l - step[bb]};
            int v[4];
#pragma unroll
            for (int c = 0; c < 4; c++) v[c] = m.voff[cell[c] / TM_CHUNK] + m.rank[cell[c]];
            int* o = m.out_faces + row * 6;
            o[0] = v[0]; o[3] = v[0];
            if (in_g[q]) { o[1] = v[1]; o[2] = v[2]; o[4] = v[2]; o[5] = v[3]; }
            else         { o[1] = v[2]; o[2] = v[1]; o[4] = v[3]; o[5] = v[2]; }
            row++;
        }
    }
}

static long long tsdf_nvox(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0) return -1;
    const long long xy = (long long)nx * ny;                // below 2^62
    if (xy >= (1ll << 31)) return 1ll << 31;
    return xy * nz >= (1ll << 31) ? 1ll << 31 : xy * nz;    // xy * nz below 2^62
}
static long long tsdf_nchunks(long long nvox) { return (nvox + TM_CHUNK - 1) / TM_CHUNK; }
static size_t tsdf_off_bytes(long long nvox) { return compact_offsets_bytes((size_t)tsdf_nchunks(nvox)); }

}  // namespace a3r

// =============================================================================================== host
using namespace a3r;

extern "C" int a3r_tsdf_set_form(int form) {
    const int old = g_tsdf_form.load();
    if (form >= 0 && form <= TS_FORM_MAX) g_tsdf_form.store(form);
    return old;
}

static int tsdf_grid_args(const char* who, const double* origin, double voxel, int nx, int ny, int nz, TsdfGrid* g) {
    A3R_CHECK_ARG(nx > 0 && ny > 0 && nz > 0, "%s: dims = (%d, %d, %d) must be positive", who, nx, ny, nz);
    A3R_CHECK_ARG(tsdf_nvox(nx, ny, nz) < (1ll << 31), "%s: dims: nx * ny * nz = %d * %d * %d must stay below 2^31", who, nx, ny, nz);
    A3R_CHECK_ARG(std::isfinite(voxel) && voxel > 0, "%s: voxel = %g must be finite and positive", who, voxel);
    A3R_CHECK_ARG(origin, "%s: null origin", who);
    A3R_CHECK_ARG(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "%s: origin = (%g, %g, %g) is not finite",
                  who, origin[0], origin[1], origin[2]);
    *g = TsdfGrid{origin[0], origin[1], origin[2], voxel, nx, ny, nz};
    return A3R_OK;
}

extern "C" int a3r_tsdf_integrate(const float* depth, const float* weight, const unsigned char* rgb, const a3r_tsdf_cam* cams_dev,
                                  const a3r_tsdf_cam* cams_host, int N, long long P, const double origin[3], double voxel, int nx, int ny,
                                  int nz, double trunc, double near_z, double max_depth, float* tsdf, float* wsum, unsigned char* out_rgb,
                                  unsigned long long* skip_stats, void* stream_) {
    const char* who = "a3r_tsdf_integrate";
    hipStream_t stream = as_stream(stream_);
    TsdfArgs a{};
    if (int rc = tsdf_grid_args(who, origin, voxel, nx, ny, nz, &a.g)) return rc;
    A3R_CHECK_ARG(std::isfinite(trunc) && trunc > 0, "%s: trunc = %g must be finite and positive", who, trunc);
    A3R_CHECK_ARG(std::isfinite(near_z) && near_z > 0, "%s: near = %g must be finite and positive", who, near_z);
    A3R_CHECK_ARG(max_depth > 0, "%s: max_depth = %g must be positive (infinity = no limit)", who, max_depth);
    A3R_CHECK_ARG(N >= 0 && P >= 0, "%s: N = %d and P = %lld must not be negative", who, N, P);
    A3R_CHECK_ARG(P < (1ll << 31) && (long long)N * P < (1ll << 31), "%s: N * P = %d * %lld must stay below 2^31", who, N, P);
    A3R_CHECK_ARG(N == 0 || (depth && weight && cams_dev && cams_host), "%s: null depth / weight / cams_dev / cams_host", who);
    A3R_CHECK_ARG(tsdf && wsum, "%s: null tsdf / wsum", who);
    A3R_CHECK_ARG(!out_rgb || rgb || N == 0, "%s: out_rgb needs rgb", who);
    for (int n = 0; n < N; n++) {
        const a3r_tsdf_cam& c = cams_host[n];
        for (int e = 0; e < 16; e++)
            A3R_CHECK_ARG(std::isfinite(c.w2c[e]), "%s: camera %d: entry %d (w2c[0..11], fx, fy, cx, cy) is not finite", who, n, e);
        A3R_CHECK_ARG(c.h > 0 && c.w > 0, "%s: camera %d: the image size h x w = %d x %d must be positive", who, n, c.h, c.w);
        A3R_CHECK_ARG((long long)c.h * c.w <= P, "%s: camera %d: h * w = %d * %d exceeds P = %lld", who, n, c.h, c.w, P);
    }
    a.depth = depth; a.weight = weight; a.rgb = out_rgb ? rgb : nullptr; a.cams = cams_dev;
    a.N = N; a.P = P;
    a.trunc = trunc; a.near_z = near_z; a.max_depth = max_depth;
    a.tsdf = tsdf; a.wsum = wsum; a.out_rgb = out_rgb; a.stats = skip_stats;
    a.nbx = (nx + TS_BX - 1) / TS_BX;
    a.nby = (ny + TS_BY - 1) / TS_BY;
    const long long blocks = (long long)a.nbx * a.nby * nz;         // at most nvox
    const bool skip = (g_tsdf_form.load() & TS_FORM_NO_SKIP) == 0;
    const dim3 grid((unsigned)blocks), tpb(TS_TPB);
    const bool colour = a.rgb != nullptr;
#define A3R_TS_LAUNCH(SK, CL) hipLaunchKernelGGL((tsdf_integrate_kernel<SK, CL>), grid, tpb, 0, stream, a)
    if (skip) { if (colour) A3R_TS_LAUNCH(true, true); else A3R_TS_LAUNCH(true, false); }
    else      { if (colour) A3R_TS_LAUNCH(false, true); else A3R_TS_LAUNCH(false, false); }
#undef A3R_TS_LAUNCH
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" size_t a3r_tsdf_mesh_workspace_bytes(int nx, int ny, int nz) {
    const long long nvox = tsdf_nvox(nx, ny, nz);
    if (nvox <= 0 || nvox > TM_MAX_VOXELS) return 0;
    return 2 * tsdf_off_bytes(nvox) + align_up((size_t)nvox * sizeof(int), 256);
}

// cells, quads, two scans; V and F come back to the host (synchronises the stream)
static int tsdf_mesh_count(const char* who, const float* tsdf, const float* wsum, int nx, int ny, int nz, const double* origin, double voxel,
                           double min_weight, void* ws, size_t ws_bytes, hipStream_t st, TsdfMesh* m, long long* V, long long* F) {
    if (int rc = tsdf_grid_args(who, origin, voxel, nx, ny, nz, &m->g)) return rc;
    const long long nvox = tsdf_nvox(nx, ny, nz);
    A3R_CHECK_ARG(nvox <= TM_MAX_VOXELS, "%s: dims: nx * ny * nz = %lld is above the %lld voxels whose faces an int counts", who, nvox,
                  TM_MAX_VOXELS);
    A3R_CHECK_ARG(min_weight > 0 && min_weight < INFINITY, "%s: min_weight = %g must be finite and positive", who, min_weight);
    A3R_CHECK_ARG(tsdf && wsum, "%s: null tsdf / wsum", who);
    const size_t need = a3r_tsdf_mesh_workspace_bytes(nx, ny, nz);
    if (int rc = check_workspace(who, ws, ws_bytes, need)) return rc;
    char* p = static_cast<char*>(ws);
    m->tsdf = tsdf; m->wsum = wsum; m->min_weight = min_weight; m->nvox = nvox;
    m->voff = reinterpret_cast<int*>(p);   p += tsdf_off_bytes(nvox);
    m->foff = reinterpret_cast<int*>(p);   p += tsdf_off_bytes(nvox);
    m->rank = reinterpret_cast<int*>(p);
    const int T = (int)tsdf_nchunks(nvox);
    const dim3 grid(T), tpb(TS_TPB);
    hipLaunchKernelGGL((tsdf_cells_kernel<false>), grid, tpb, 0, st, *m);
    hipLaunchKernelGGL((tsdf_faces_kernel<false>), grid, tpb, 0, st, *m);
    compact_scan(m->voff, T, st);
    compact_scan(m->foff, T, st);
    A3R_LAUNCH_CHECK();
    int nv = 0, nq = 0;
    A3R_HIP(compact_read_total(m->voff, T, &nv, st));
    A3R_HIP(compact_read_total(m->foff, T, &nq, st));
    A3R_HIP(hipStreamSynchronize(st));
    *V = nv;
    *F = 2ll * nq;
    return A3R_OK;
}

extern "C" int a3r_tsdf_mesh_count(const float* tsdf, const float* wsum, int nx, int ny, int nz, double min_weight, void* ws, size_t ws_bytes,
                                   long long* n_vertices_host, long long* n_faces_host, void* stream) {
    const char* who = "a3r_tsdf_mesh_count";
    A3R_CHECK_ARG(n_vertices_host && n_faces_host, "%s: null n_vertices_host / n_faces_host", who);
    const double origin[3] = {0.0, 0.0, 0.0};
    TsdfMesh m{};
    return tsdf_mesh_count(who, tsdf, wsum, nx, ny, nz, origin, 1.0, min_weight, ws, ws_bytes, as_stream(stream), &m, n_vertices_host,
                           n_faces_host);
}

extern "C" int a3r_tsdf_mesh_export(const float* tsdf, const float* wsum, const unsigned char* rgb, int nx, int ny, int nz,
                                    const double origin[3], double voxel, double min_weight, void* ws, size_t ws_bytes,
                                    long long vertex_capacity, long long face_capacity, float* out_xyz, unsigned char* out_rgb, int* out_faces,
                                    long long* n_vertices_host, long long* n_faces_host, void* stream) {
    const char* who = "a3r_tsdf_mesh_export";
    A3R_CHECK_ARG(n_vertices_host && n_faces_host, "%s: null n_vertices_host / n_faces_host", who);
    A3R_CHECK_ARG(vertex_capacity >= 0 && face_capacity >= 0, "%s: negative capacity", who);
    A3R_CHECK_ARG(out_xyz || vertex_capacity == 0, "%s: null out_xyz (only a capacity of 0 needs no buffer)", who);
    A3R_CHECK_ARG(out_faces || face_capacity == 0, "%s: null out_faces (only a capacity of 0 needs no buffer)", who);
    A3R_CHECK_ARG(!out_rgb || rgb, "%s: out_rgb needs the grid's rgb", who);
    hipStream_t st = as_stream(stream);
    TsdfMesh m{};
    // the count is always taken afresh: the rank map and the offsets in the workspace then belong to exactly these inputs
    if (int rc = tsdf_mesh_count(who, tsdf, wsum, nx, ny, nz, origin, voxel, min_weight, ws, ws_bytes, st, &m, n_vertices_host, n_faces_host))
        return rc;
    const long long V = *n_vertices_host, F = *n_faces_host;
    A3R_CHECK_ARG(V <= vertex_capacity && F <= face_capacity,
                  "%s: capacities %lld vertices, %lld faces are smaller than the mesh's %lld vertices, %lld faces (nothing was written)", who,
                  vertex_capacity, face_capacity, V, F);
    if (V == 0) return A3R_OK;
    m.rgb = out_rgb ? rgb : nullptr;
    m.out_xyz = out_xyz; m.out_rgb = out_rgb; m.out_faces = out_faces;
    const dim3 grid((unsigned)tsdf_nchunks(m.nvox)), tpb(TS_TPB);
    hipLaunchKernelGGL((tsdf_cells_kernel<true>), grid, tpb, 0, st, m);
    if (F > 0) hipLaunchKernelGGL((tsdf_faces_kernel<true>), grid, tpb, 0, st, m);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
