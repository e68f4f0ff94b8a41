// Scene out for gfx950: the aligned scene of an aligner handle as world points, dense ([N,P,3]) or compacted to the pixels a
// confidence threshold and a dynamic mask keep (what get_3D_model_from_scene of the reference's tool/demo.py builds on the host
// from get_pts3d() and get_masks()).
//
//   world = R_n * (d (x - ppx) / f, d (y - ppy) / f, d) + t_n,   d = exp(log_depth)  |  mono * exp(scalemap) + shift
//
// with R, t, f, pp, shift read from the handle's img_xf rows (build_transforms of align.hip: the decoding the iteration uses) and
// the arithmetic of align_main_kernel's pixel_forward.  Streaming kernels, HBM-bound:
//   * a workgroup owns SCHUNK = 1024 consecutive pixels of one image, a thread 4 CONSECUTIVE pixels (16-byte loads when P % 4 == 0
//     and the buffers are 16-byte aligned, scalar loads otherwise);
//   * compaction by the count / scan / place scheme of compact.h: pass 1 counts the kept pixels of every chunk, pass 2 recomputes
//     the points and places them at offset[chunk] + rank: image-major, row-major, a function of the inputs alone.
//   * pass 2 stages a workgroup's points in LDS (its output range is contiguous) and writes them with consecutive lanes on
//     consecutive addresses.
//   * the triangle mesh over the kept pixels (pts3d_to_trimesh / cat_meshes of dust3r/viz.py) repeats the scheme for faces: pass 1
//     also leaves every pixel's rank inside its chunk in the workspace, a face count pass and a face placement pass read nothing
//     but that map and the scanned offsets.
#include "common.h"
#include "scene.h"
#include "compact.h"

namespace a3r {

constexpr int SPX = 4;                  // consecutive pixels per thread
constexpr int STPB = 256;
constexpr int SCHUNK = SPX * STPB;      // pixels per workgroup

struct SceneCam {
    float R[9], T[3], inv_f, ppx, ppy, shift;
    int W, area;
};

// wave-uniform reads (noalias tables, uniform index): scalar loads
__device__ __forceinline__ SceneCam load_cam(const float* __restrict__ img_xf, const int* __restrict__ imw, const int* __restrict__ imarea, int n) {
    SceneCam c;
    const float* ix = img_xf + n * 16;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        c.R[r * 3 + 0] = ix[r * 4 + 0]; c.R[r * 3 + 1] = ix[r * 4 + 1]; c.R[r * 3 + 2] = ix[r * 4 + 2];
        c.T[r] = ix[r * 4 + 3];
    }
    c.inv_f = 1.f / ix[12]; c.ppx = ix[13]; c.ppy = ix[14]; c.shift = ix[15];
    c.W = imw[n]; c.area = imarea[n];
    return c;
}

// world point of pixel (x, y) from the raw depth parameter (align_main_kernel: pixel_forward, then R * rel + T)
template <bool MONO>
__device__ __forceinline__ void scene_point(const SceneCam& c, int x, int y, float rawv, float monov, float* w) {
    const float dep = MONO ? monov * expf(rawv) + c.shift : expf(rawv);
    const float r0 = dep * ((float)x - c.ppx) * c.inv_f;
    const float r1 = dep * ((float)y - c.ppy) * c.inv_f;
#pragma unroll
    for (int r = 0; r < 3; r++) w[r] = c.R[r * 3] * r0 + c.R[r * 3 + 1] * r1 + c.R[r * 3 + 2] * dep + c.T[r];
}

// the thread's 4 raw depth parameters (and mono values); pixels at and beyond P read as 0
template <bool MONO, bool VEC>
__device__ __forceinline__ void load_depth4(const SceneView& v, int n, int p0, float* raw, float* mono) {
    const size_t base = (size_t)n * v.P;
    if (VEC) {                      // P % 4 == 0 and p0 % 4 == 0: the four pixels are inside P together
        f32x4 r4 = {0.f, 0.f, 0.f, 0.f}, m4 = {0.f, 0.f, 0.f, 0.f};
        if (p0 < v.P) {
            r4 = *reinterpret_cast<const f32x4*>(v.depth + base + p0);
            if (MONO) m4 = *reinterpret_cast<const f32x4*>(v.mono + base + p0);
        }
        raw[0] = r4.x; raw[1] = r4.y; raw[2] = r4.z; raw[3] = r4.w;
        mono[0] = m4.x; mono[1] = m4.y; mono[2] = m4.z; mono[3] = m4.w;
    } else {
#pragma unroll
        for (int i = 0; i < SPX; i++) {
            const bool in = p0 + i < v.P;
            raw[i] = in ? v.depth[base + p0 + i] : 0.f;
            mono[i] = (MONO && in) ? v.mono[base + p0 + i] : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------- dense
// grid (nchunks, N).  out[n, p, :] for every p < P; zeros at the padding pixels p >= h_n * w_n of a mixed-shape scene.
template <bool MONO, bool VEC>
__global__ __launch_bounds__(STPB) void scene_points_kernel(SceneView v, float* __restrict__ out, const float* __restrict__ img_xf,
                                                           const int* __restrict__ imw, const int* __restrict__ imarea) {
    const int n = blockIdx.y, p0 = blockIdx.x * SCHUNK + threadIdx.x * SPX;
    if (p0 >= v.P) return;
    const SceneCam c = load_cam(img_xf, imw, imarea, n);
    float raw[SPX], mono[SPX], w[SPX][3];
    load_depth4<MONO, VEC>(v, n, p0, raw, mono);
    int y = p0 / c.W, x = p0 - y * c.W;
#pragma unroll
    for (int i = 0; i < SPX; i++) {
        scene_point<MONO>(c, x, y, raw[i], mono[i], w[i]);
        if (p0 + i >= c.area) w[i][0] = w[i][1] = w[i][2] = 0.f;
        if (++x == c.W) { x = 0; y++; }
    }
    float* o = out + ((size_t)n * v.P + p0) * 3;
    if (VEC) {                      // 48 contiguous bytes, 16-byte aligned
        f32x4* o4 = reinterpret_cast<f32x4*>(o);
        o4[0] = f32x4{w[0][0], w[0][1], w[0][2], w[1][0]};
        o4[1] = f32x4{w[1][1], w[1][2], w[2][0], w[2][1]};
        o4[2] = f32x4{w[2][2], w[3][0], w[3][1], w[3][2]};
    } else {
#pragma unroll
        for (int i = 0; i < SPX; i++)
            if (p0 + i < v.P) { o[i * 3 + 0] = w[i][0]; o[i * 3 + 1] = w[i][1]; o[i * 3 + 2] = w[i][2]; }
    }
}

// ------------------------------------------------------------------------------------------- compaction
struct SceneSel {
    const float* conf;              // [N, P]
    const unsigned char* dyn;       // [N, P] or null
    const unsigned char* rgb;       // [N, P, 3] or null (pass 2)
    float thr;
    int* offsets;                   // [N * nchunks + 1]: pass 1 writes the chunk counts, the scan turns them into offsets
    float* out_xyz;                 // pass 2
    unsigned char* out_rgb;
    int* out_index;
    int* rank;                      // [N, P] or null (pass 1, mesh): a kept pixel's rank inside its chunk, -1 for a dropped one
};

typedef int i32x4 __attribute__((ext_vector_type(4)));

// grid (nchunks, N).  WRITE = false: offsets[chunk] = kept pixels of the chunk.  WRITE = true: the kept pixels go to
// offsets[chunk] + (their rank inside the chunk).
template <bool MONO, bool VEC, bool WRITE>
__global__ __launch_bounds__(STPB) void scene_compact_kernel(SceneView v, SceneSel s, const float* __restrict__ img_xf,
                                                            const int* __restrict__ imw, const int* __restrict__ imarea) {
    __shared__ int wave_total[STPB / 64];
    __shared__ float st_xyz[WRITE ? SCHUNK * 3 : 1];
    __shared__ int st_index[WRITE ? SCHUNK : 1];
    __shared__ unsigned char st_rgb[WRITE ? SCHUNK * 3 : 4];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int nchunks = gridDim.x, p0 = blockIdx.x * SCHUNK + tid * SPX;
    const SceneCam c = load_cam(img_xf, imw, imarea, n);
    const size_t base = (size_t)n * v.P;
    float raw[SPX], mono[SPX], cf[SPX], w[SPX][3];
    unsigned dy[SPX];
    load_depth4<MONO, VEC>(v, n, p0, raw, mono);
    if (VEC) {
        f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
        unsigned d4 = 0;
        if (p0 < v.P) {
            c4 = *reinterpret_cast<const f32x4*>(s.conf + base + p0);
            if (s.dyn) d4 = *reinterpret_cast<const unsigned*>(s.dyn + base + p0);
        }
        cf[0] = c4.x; cf[1] = c4.y; cf[2] = c4.z; cf[3] = c4.w;
#pragma unroll
        for (int i = 0; i < SPX; i++) dy[i] = (d4 >> (8 * i)) & 0xffu;
    } else {
#pragma unroll
        for (int i = 0; i < SPX; i++) {
            const bool in = p0 + i < v.P;
            cf[i] = in ? s.conf[base + p0 + i] : 0.f;
            dy[i] = (in && s.dyn) ? s.dyn[base + p0 + i] : 0u;
        }
    }
    // the kept rule: inside the image, confidence strictly above the threshold, not dynamic, all three coordinates finite
    bool keep[SPX];
    int y = p0 < v.P ? p0 / c.W : 0, x = p0 - y * c.W;
#pragma unroll
    for (int i = 0; i < SPX; i++) {
        scene_point<MONO>(c, x, y, raw[i], mono[i], w[i]);
        keep[i] = p0 + i < c.area && cf[i] > s.thr && dy[i] == 0u &&
                  __builtin_isfinite(w[i][0]) && __builtin_isfinite(w[i][1]) && __builtin_isfinite(w[i][2]);
        if (++x == c.W) { x = 0; y++; }
    }
    // the threads own consecutive pixel quads, so the order is (thread, i)
    int first, total;
    block_rank<STPB, SPX>(keep, wave_total, &first, &total);
    if (!WRITE) {
        if (s.rank) {
            int l = first, r[SPX];
#pragma unroll
            for (int i = 0; i < SPX; i++) r[i] = keep[i] ? l++ : -1;
            int* o = s.rank + base + p0;
            if (VEC) {
                if (p0 < v.P) *reinterpret_cast<i32x4*>(o) = i32x4{r[0], r[1], r[2], r[3]};
            } else {
#pragma unroll
                for (int i = 0; i < SPX; i++)
                    if (p0 + i < v.P) o[i] = r[i];
            }
        }
        if (tid == 0) s.offsets[n * nchunks + blockIdx.x] = total;
        return;
    }
    if (total == 0) return;         // workgroup-uniform
    unsigned c3[3] = {0u, 0u, 0u};
    const bool any = keep[0] || keep[1] || keep[2] || keep[3];
    if (s.rgb && any) {
        const unsigned char* src = s.rgb + (base + p0) * 3;
        if (VEC) {                  // 12 contiguous bytes, 4-byte aligned
            const unsigned* s4 = reinterpret_cast<const unsigned*>(src);
            c3[0] = s4[0]; c3[1] = s4[1]; c3[2] = s4[2];
        } else {
#pragma unroll
            for (int k = 0; k < SPX * 3; k++)
                if (p0 + k / 3 < v.P) c3[k >> 2] |= (unsigned)src[k] << (8 * (k & 3));
        }
    }
    int l = first;
#pragma unroll
    for (int i = 0; i < SPX; i++) {
        if (!keep[i]) continue;
        st_xyz[l * 3 + 0] = w[i][0]; st_xyz[l * 3 + 1] = w[i][1]; st_xyz[l * 3 + 2] = w[i][2];
        st_index[l] = (int)(base + p0 + i);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int byte = i * 3 + k;
            st_rgb[l * 3 + k] = (unsigned char)(c3[byte >> 2] >> (8 * (byte & 3)));
        }
        l++;
    }
    __syncthreads();
    const int slot = n * nchunks + blockIdx.x;
    const size_t o = (size_t)s.offsets[slot];
    // pass 1 saw the same inputs, so this is its count; should the caller have rewritten them in between, stay inside the range
    total = min(total, s.offsets[slot + 1] - s.offsets[slot]);
    for (int k = tid; k < total * 3; k += STPB) s.out_xyz[o * 3 + k] = st_xyz[k];
    if (s.out_index)
        for (int k = tid; k < total; k += STPB) s.out_index[o + k] = st_index[k];
    if (s.out_rgb)
        for (int k = tid; k < total * 3; k += STPB) s.out_rgb[o * 3 + k] = st_rgb[k];
}

// ------------------------------------------------------------------------------------------- mesh
// The triangles of pts3d_to_trimesh / cat_meshes (dust3r/viz.py) over the kept pixels, vertex ids = ranks among the kept pixels.
// Quad (y, x), x < w - 1, y < h - 1, of image n: A = (tl, tr, bl) and B = (tr, bl, br), each present iff its three pixels are kept.
// Validity and ids come from the rank map pass 1 left in the workspace (rank inside the chunk, -1 = dropped) and the vertex
// offsets of the scan: vertex id of pixel q = voff[n, q / SCHUNK] + rank[n, q].  No depth, no pose is decoded here.
// Face blocks of an image: [A, B] (nblk = 2) or [A, A', B, B'] (nblk = 4; the primed blocks are the same triangles wound backwards);
// foff is laid out [n][block][chunk], so one flat exclusive scan gives every (image, block, chunk) its output range.
struct SceneMesh {
    const int* rank;                // [N, P]
    const int* voff;                // [N * nchunks + 1] vertex offsets
    int* foff;                      // [N * nblk * nchunks + 1]: the count pass writes counts, the scan turns them into offsets
    const unsigned char* rgb;       // [N, P, 3] or null
    int* out_faces;                 // [F, 3]
    unsigned char* out_rgb;         // [F, 3] or null
    int P, nblk;
};

// grid (nchunks, N); a thread owns 4 consecutive top-left pixels.  WRITE = false: the chunk's A and B counts.  WRITE = true: the
// faces are staged in LDS (A in the first SCHUNK slots, B in the second) and written with consecutive lanes on consecutive addresses.
template <bool VEC, bool WRITE>
__global__ __launch_bounds__(STPB) void scene_faces_kernel(SceneMesh m, const int* __restrict__ imw) {
    __shared__ int wave_total[2 * (STPB / 64)];
    __shared__ int st_face[WRITE ? 2 * SCHUNK * 3 : 1];
    __shared__ unsigned char st_rgb[WRITE ? 2 * SCHUNK * 3 : 4];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int nchunks = gridDim.x, p0 = blockIdx.x * SCHUNK + tid * SPX;
    const int W = imw[n], P = m.P;
    const size_t base = (size_t)n * P;
    const int* __restrict__ rk = m.rank + base;
    // ranks of the row p0 .. p0 + 4 and of the row below it; everything at and beyond P reads as dropped.  The padding pixels
    // p >= h * w of a smaller image hold -1 themselves, which also ends the last row: its "row below" is padding or beyond P.
    int top[SPX + 1], bot[SPX + 1];
#pragma unroll
    for (int i = 0; i <= SPX; i++) top[i] = bot[i] = -1;
    const int q0 = p0 + W;
    if (VEC) {                      // P % 4 == 0, p0 % 4 == 0: four pixels are inside P together; the row below when W % 4 == 0 too
        if (p0 < P) {
            const i32x4 t = *reinterpret_cast<const i32x4*>(rk + p0);
            top[0] = t.x; top[1] = t.y; top[2] = t.z; top[3] = t.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < SPX; i++)
            if (p0 + i < P) top[i] = rk[p0 + i];
    }
    if (p0 + SPX < P) top[SPX] = rk[p0 + SPX];
    if (VEC && (W & 3) == 0) {      // block-uniform
        if (q0 < P) {
            const i32x4 t = *reinterpret_cast<const i32x4*>(rk + q0);
            bot[0] = t.x; bot[1] = t.y; bot[2] = t.z; bot[3] = t.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < SPX; i++)
            if (q0 + i < P) bot[i] = rk[q0 + i];
    }
    if (q0 + SPX < P) bot[SPX] = rk[q0 + SPX];
    bool face[2 * SPX];               // the two flag sets of one block_rank: A, then B
    bool* const fa = face;
    bool* const fb = face + SPX;
    int x = p0 % W;
#pragma unroll
    for (int i = 0; i < SPX; i++) {
        const bool diag = x < W - 1 && top[i + 1] >= 0 && bot[i] >= 0;       // no quad wraps from the end of a row to the next
        fa[i] = diag && top[i] >= 0;
        fb[i] = diag && bot[i + 1] >= 0;
        if (++x == W) x = 0;
    }
    // A and B ranked apart under one barrier: quad order is (thread, i)
    int first[2], total[2];
    block_rank<STPB, SPX, 2>(face, wave_total, first, total);
    const int total_a = total[0], total_b = total[1];
    const int slot_a = n * m.nblk * nchunks + blockIdx.x, slot_b = slot_a + (m.nblk >> 1) * nchunks;
    const bool two = m.nblk == 4;
    if (!WRITE) {
        if (tid == 0) {
            m.foff[slot_a] = total_a; m.foff[slot_b] = total_b;
            if (two) { m.foff[slot_a + nchunks] = total_a; m.foff[slot_b + nchunks] = total_b; }
        }
        return;
    }
    if (total_a + total_b == 0) return;      // workgroup-uniform
    const int* __restrict__ vo = m.voff + n * nchunks;
    const bool colour = m.out_rgb != nullptr;
    int la = first[0], lb = SCHUNK + first[1];
#pragma unroll
    for (int i = 0; i < SPX; i++) {
        if (!(fa[i] || fb[i])) continue;
        const int p = p0 + i;
        const int tr = vo[(p + 1) / SCHUNK] + top[i + 1], bl = vo[(p + W) / SCHUNK] + bot[i];
        if (fa[i]) {
            st_face[la * 3 + 0] = vo[p / SCHUNK] + top[i]; st_face[la * 3 + 1] = tr; st_face[la * 3 + 2] = bl;
            if (colour) {
                const unsigned char* src = m.rgb + (base + p) * 3;                  // the colour of the top-left pixel
                st_rgb[la * 3 + 0] = src[0]; st_rgb[la * 3 + 1] = src[1]; st_rgb[la * 3 + 2] = src[2];
            }
            la++;
        }
        if (fb[i]) {
            st_face[lb * 3 + 0] = tr; st_face[lb * 3 + 1] = bl; st_face[lb * 3 + 2] = vo[(p + W + 1) / SCHUNK] + bot[i + 1];
            if (colour) {
                const unsigned char* src = m.rgb + (base + p + W + 1) * 3;          // the colour of the bottom-right pixel
                st_rgb[lb * 3 + 0] = src[0]; st_rgb[lb * 3 + 1] = src[1]; st_rgb[lb * 3 + 2] = src[2];
            }
            lb++;
        }
    }
    __syncthreads();
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
        const bool b_side = blk >= 2, rev = blk & 1;
        if (rev && !two) continue;
        const int slot = (b_side ? slot_b : slot_a) + (rev ? nchunks : 0), l0 = b_side ? SCHUNK : 0;
        const size_t o = (size_t)m.foff[slot];
        // the count pass saw the same rank map, so this is its count; stay inside the range whatever the workspace holds
        const int total = min(b_side ? total_b : total_a, m.foff[slot + 1] - m.foff[slot]);
        for (int k = tid; k < total * 3; k += STPB) {
            const int f = k / 3, c = k - f * 3;
            m.out_faces[o * 3 + k] = st_face[(l0 + f) * 3 + (rev ? 2 - c : c)];
        }
        if (colour)
            for (int k = tid; k < total * 3; k += STPB) m.out_rgb[o * 3 + k] = st_rgb[l0 * 3 + k];
    }
}

// ------------------------------------------------------------------------------------------- clean_pointcloud
// cloud_opt/base_opt.py:468-503 on the handle's state.  conf[i,p] drops to bad_conf when some other view j sees the world point of
// (i,p) in front of its own depth map (z < (1 - tol) * depth_j[v,u] at the rounded projection (u,v)) while being the more
// confident of the two (conf[i,p] < conf[j,v,u]).  Image i reads the FINISHED rows of the images below it, so the images are N
// launches in stream order; inside launch i every pixel is independent, row i is the only row written and never read.
//
// World-to-camera table, CLEAN_CAM floats per image: R^T (9), t (3), f, ppx, ppy, W, H, pad to 20 (five 16-byte scalar loads).
constexpr int CLEAN_CAM = 20;

static size_t clean_cam_bytes(int N) { return align_up((size_t)N * CLEAN_CAM * sizeof(float), 256); }

// grid (nchunks, N).  dense[n,p] = the depth scene_point uses (same expf, same fma order); the first thread of chunk 0 writes the
// table row of image n.  Padding pixels p >= h_n * w_n are written too (never read: the padding of an image is never visible).
template <bool MONO, bool VEC>
__global__ __launch_bounds__(STPB) void scene_clean_prep_kernel(SceneView v, float* __restrict__ cam, float* __restrict__ dense,
                                                               const float* __restrict__ img_xf, const int* __restrict__ imw,
                                                               const int* __restrict__ imarea) {
    const int n = blockIdx.y, p0 = blockIdx.x * SCHUNK + threadIdx.x * SPX;
    const float* ix = img_xf + n * 16;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float* o = cam + n * CLEAN_CAM;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            o[r * 3 + 0] = ix[0 * 4 + r]; o[r * 3 + 1] = ix[1 * 4 + r]; o[r * 3 + 2] = ix[2 * 4 + r];     // row r of R^T
            o[9 + r] = ix[r * 4 + 3];
        }
        const int W = imw[n];
        o[12] = ix[12]; o[13] = ix[13]; o[14] = ix[14];
        o[15] = (float)W; o[16] = (float)(W > 0 ? imarea[n] / W : 0);
        o[17] = o[18] = o[19] = 0.f;
    }
    if (p0 >= v.P) return;
    const float shift = ix[15];
    float raw[SPX], mono[SPX], d[SPX];
    load_depth4<MONO, VEC>(v, n, p0, raw, mono);
#pragma unroll
    for (int i = 0; i < SPX; i++) d[i] = MONO ? mono[i] * expf(raw[i]) + shift : expf(raw[i]);
    float* o = dense + (size_t)n * v.P + p0;
    if (VEC) {
        *reinterpret_cast<f32x4*>(o) = f32x4{d[0], d[1], d[2], d[3]};
    } else {
#pragma unroll
        for (int i = 0; i < SPX; i++)
            if (p0 + i < v.P) o[i] = d[i];
    }
}

// grid (nchunks): target image `img`.  A thread owns 4 consecutive pixels and walks the other views in increasing order until
// each of its pixels is clipped; the walk ends for the whole wave when no lane has a live pixel (a wave-uniform exit, so the
// table reads stay scalar loads).  Skipped outright: padding pixels, confidences already <= bad_conf (NaN included: the compare
// is false) and non-finite world points.  A non-finite projection fails the float range tests before it becomes an index.
template <bool MONO, bool VEC>
__global__ __launch_bounds__(STPB) void scene_clean_kernel(SceneView v, float* conf, int img, const float* __restrict__ cam,
                                                          const float* __restrict__ dense, float keep_frac, float bad_conf,
                                                          const float* __restrict__ img_xf, const int* __restrict__ imw,
                                                          const int* __restrict__ imarea) {
    const int p0 = blockIdx.x * SCHUNK + threadIdx.x * SPX;
    const bool inside = p0 < v.P;
    const SceneCam c = load_cam(img_xf, imw, imarea, img);
    float raw[SPX], mono[SPX], cf[SPX], w[SPX][3];
    load_depth4<MONO, VEC>(v, img, p0, raw, mono);
    float* row = conf + (size_t)img * v.P;
    if (VEC) {
        f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
        if (inside) c4 = *reinterpret_cast<const f32x4*>(row + p0);
        cf[0] = c4.x; cf[1] = c4.y; cf[2] = c4.z; cf[3] = c4.w;
    } else {
#pragma unroll
        for (int i = 0; i < SPX; i++) cf[i] = p0 + i < v.P ? row[p0 + i] : 0.f;
    }
    bool live[SPX], hit[SPX];
    int y = inside ? p0 / c.W : 0, x = p0 - y * c.W;
#pragma unroll
    for (int i = 0; i < SPX; i++) {
        scene_point<MONO>(c, x, y, raw[i], mono[i], w[i]);
        live[i] = p0 + i < c.area && cf[i] > bad_conf &&
                  __builtin_isfinite(w[i][0]) && __builtin_isfinite(w[i][1]) && __builtin_isfinite(w[i][2]);
        hit[i] = false;
        if (++x == c.W) { x = 0; y++; }
    }
    for (int j = 0; j < v.N; j++) {
        if (__ballot(live[0] || live[1] || live[2] || live[3]) == 0ull) break;
        if (j == img) continue;
        const float* cj = cam + j * CLEAN_CAM;
        const float f = cj[12], ppx = cj[13], ppy = cj[14], Wf = cj[15], Hf = cj[16];
        const float* dj = dense + (size_t)j * v.P;
        const float* fj = conf + (size_t)j * v.P;
        float z[SPX], dep[SPX], oc[SPX];
        bool vis[SPX];
#pragma unroll
        for (int i = 0; i < SPX; i++) {     // all gathers of the step are issued before the first is consumed
            const float d0 = w[i][0] - cj[9], d1 = w[i][1] - cj[10], d2 = w[i][2] - cj[11];
            const float cx = cj[0] * d0 + cj[1] * d1 + cj[2] * d2;
            const float cy = cj[3] * d0 + cj[4] * d1 + cj[5] * d2;
            z[i] = cj[6] * d0 + cj[7] * d1 + cj[8] * d2;
            const float iz = 1.f / z[i];
            const float u = rintf(f * cx * iz + ppx), vv = rintf(f * cy * iz + ppy);
            vis[i] = live[i] && z[i] > 0.f && u >= 0.f && u < Wf && vv >= 0.f && vv < Hf;      // NaN / inf: every compare is false
            dep[i] = 0.f; oc[i] = 0.f;
            if (vis[i]) {
                const int q = (int)vv * (int)Wf + (int)u;
                dep[i] = dj[q]; oc[i] = fj[q];
            }
        }
#pragma unroll
        for (int i = 0; i < SPX; i++)
            if (vis[i] && z[i] < keep_frac * dep[i] && cf[i] < oc[i]) { hit[i] = true; live[i] = false; }
    }
    if (!(hit[0] || hit[1] || hit[2] || hit[3])) return;
    if (VEC) {                          // the quad goes back whole: the unclipped lanes hold the bits that were loaded
        *reinterpret_cast<f32x4*>(row + p0) = f32x4{hit[0] ? bad_conf : cf[0], hit[1] ? bad_conf : cf[1], hit[2] ? bad_conf : cf[2],
                                                    hit[3] ? bad_conf : cf[3]};
    } else {
#pragma unroll
        for (int i = 0; i < SPX; i++)
            if (hit[i]) row[p0 + i] = bad_conf;
    }
}

static int scene_nchunks(int P) { return (P + SCHUNK - 1) / SCHUNK; }

}  // namespace a3r

// =============================================================================================== host
using namespace a3r;

extern "C" size_t a3r_align_scene_workspace_bytes(int N, int P) {
    if (N <= 0 || P <= 0) return 0;
    return compact_offsets_bytes((size_t)N * scene_nchunks(P));
}

extern "C" int a3r_align_scene_points(a3r_align_t a, float* out_xyz, void* stream) {
    A3R_CHECK_ARG(out_xyz, "a3r_align_scene_points: null output");
    hipStream_t st = as_stream(stream);
    SceneView v;
    if (int rc = align_scene_view(a, st, &v, "a3r_align_scene_points")) return rc;
    const bool vec = v.P % 4 == 0 && aligned_to(v.depth, 16) && aligned_to(out_xyz, 16) && (!v.mono || aligned_to(v.mono, 16));
    const dim3 grid(scene_nchunks(v.P), v.N), block(STPB);
#define A3R_SCENE_LAUNCH(MONOV, VECV) \
    hipLaunchKernelGGL((scene_points_kernel<MONOV, VECV>), grid, block, 0, st, v, out_xyz, v.img_xf, v.imw, v.imarea)
    if (v.mono) { if (vec) A3R_SCENE_LAUNCH(true, true); else A3R_SCENE_LAUNCH(true, false); }
    else        { if (vec) A3R_SCENE_LAUNCH(false, true); else A3R_SCENE_LAUNCH(false, false); }
#undef A3R_SCENE_LAUNCH
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

template <bool WRITE>
static void launch_compact(const SceneView& v, const SceneSel& s, bool vec, hipStream_t st) {
    const dim3 grid(scene_nchunks(v.P), v.N), block(STPB);
#define A3R_SCENE_LAUNCH(MONOV, VECV) \
    hipLaunchKernelGGL((scene_compact_kernel<MONOV, VECV, WRITE>), grid, block, 0, st, v, s, v.img_xf, v.imw, v.imarea)
    if (v.mono) { if (vec) A3R_SCENE_LAUNCH(true, true); else A3R_SCENE_LAUNCH(true, false); }
    else        { if (vec) A3R_SCENE_LAUNCH(false, true); else A3R_SCENE_LAUNCH(false, false); }
#undef A3R_SCENE_LAUNCH
}

// pass 1 + scan; the kept count of the whole scene comes back to the host (synchronises the stream)
static int scene_count(a3r_align_t a, const char* who, const float* conf, float thr, const uint8_t* dyn, const uint8_t* rgb,
                       void* workspace, size_t workspace_bytes, int* counts_dev, hipStream_t st, SceneView* v, SceneSel* s, bool* vec,
                       long long* total) {
    A3R_CHECK_ARG(conf, "%s: null confidence buffer", who);
    if (int rc = align_scene_view(a, st, v, who)) return rc;
    A3R_CHECK_ARG((size_t)v->N * v->P < (1ull << 31), "%s: N * P = %zu does not fit the int32 point index", who, (size_t)v->N * v->P);
    const size_t need = a3r_align_scene_workspace_bytes(v->N, v->P);
    A3R_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    A3R_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "%s: workspace must be 4-byte aligned", who);
    *vec = v->P % 4 == 0 && aligned_to(v->depth, 16) && aligned_to(conf, 16) && (!v->mono || aligned_to(v->mono, 16)) && (!dyn || aligned_to(dyn, 16)) &&
           (!rgb || aligned_to(rgb, 16));
    s->conf = conf; s->dyn = dyn; s->rgb = rgb; s->thr = thr; s->offsets = static_cast<int*>(workspace);
    s->out_xyz = nullptr; s->out_rgb = nullptr; s->out_index = nullptr; s->rank = nullptr;
    const int nch = scene_nchunks(v->P), T = v->N * nch;
    launch_compact<false>(*v, *s, *vec, st);
    compact_scan(s->offsets, T, st, v->N, nch, counts_dev);
    A3R_LAUNCH_CHECK();
    int total_i = 0;
    A3R_HIP(compact_read_total(s->offsets, T, &total_i, st));
    A3R_HIP(hipStreamSynchronize(st));
    *total = total_i;
    return A3R_OK;
}

extern "C" int a3r_align_scene_count(a3r_align_t a, const float* conf, float thr, const uint8_t* dyn, void* workspace,
                                     size_t workspace_bytes, int* counts_dev, long long* total_host, void* stream) {
    A3R_CHECK_ARG(total_host, "a3r_align_scene_count: null total_host");
    SceneView v;
    SceneSel s;
    bool vec;
    return scene_count(a, "a3r_align_scene_count", conf, thr, dyn, nullptr, workspace, workspace_bytes, counts_dev, as_stream(stream), &v, &s,
                       &vec, total_host);
}

extern "C" int a3r_align_scene_export(a3r_align_t a, const float* conf, float thr, const uint8_t* dyn, const uint8_t* rgb, void* workspace,
                                      size_t workspace_bytes, long long capacity, float* out_xyz, uint8_t* out_rgb, int* out_index,
                                      long long* n_written_host, void* stream) {
    A3R_CHECK_ARG(n_written_host, "a3r_align_scene_export: null n_written_host");
    A3R_CHECK_ARG(capacity >= 0, "a3r_align_scene_export: negative capacity");
    A3R_CHECK_ARG(out_xyz || capacity == 0, "a3r_align_scene_export: null out_xyz (only a capacity of 0 needs no buffer)");
    A3R_CHECK_ARG(!out_rgb || rgb, "a3r_align_scene_export: out_rgb needs the rgb source buffer");
    hipStream_t st = as_stream(stream);
    SceneView v;
    SceneSel s;
    bool vec;
    long long total = 0;
    *n_written_host = 0;
    // the count is always taken afresh: the offsets in the workspace then belong to exactly these inputs
    if (int rc = scene_count(a, "a3r_align_scene_export", conf, thr, dyn, out_rgb ? rgb : nullptr, workspace, workspace_bytes, nullptr, st, &v,
                             &s, &vec, &total))
        return rc;
    *n_written_host = total;
    A3R_CHECK_ARG(total <= capacity, "a3r_align_scene_export: capacity %lld is smaller than the %lld kept points (nothing was written)",
                  capacity, total);
    if (total == 0) return A3R_OK;
    s.out_xyz = out_xyz; s.out_rgb = out_rgb; s.out_index = out_index;
    launch_compact<true>(v, s, vec, st);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

// mesh workspace: vertex offsets [T + 1] | face offsets [4 T + 1] | rank map [N, P], each part rounded up to 256 bytes (T = N * nchunks)
extern "C" size_t a3r_align_scene_mesh_workspace_bytes(int N, int P) {
    if (N <= 0 || P <= 0) return 0;
    const size_t T = (size_t)N * scene_nchunks(P);
    return compact_offsets_bytes(T) + compact_offsets_bytes(4 * T) + align_up((size_t)N * P * sizeof(int), 256);
}

template <bool WRITE>
static void launch_faces(const SceneView& v, const SceneMesh& m, hipStream_t st) {
    const dim3 grid(scene_nchunks(v.P), v.N), block(STPB);
    if (v.P % 4 == 0) hipLaunchKernelGGL((scene_faces_kernel<true, WRITE>), grid, block, 0, st, m, v.imw);
    else              hipLaunchKernelGGL((scene_faces_kernel<false, WRITE>), grid, block, 0, st, m, v.imw);
}

// pass 1 (vertex counts + rank map), scan, face counts, scan; both totals come back to the host (synchronises the stream)
static int mesh_count(a3r_align_t a, const char* who, const float* conf, float thr, const uint8_t* dyn, const uint8_t* rgb, void* workspace,
                      size_t workspace_bytes, int double_sided, hipStream_t st, SceneView* v, SceneSel* s, SceneMesh* m, bool* vec,
                      long long* n_vertices, long long* n_faces) {
    A3R_CHECK_ARG(conf, "%s: null confidence buffer", who);
    A3R_CHECK_ARG(double_sided == 0 || double_sided == 1, "%s: double_sided = %d is neither 0 nor 1", who, double_sided);
    if (int rc = align_scene_view(a, st, v, who)) return rc;
    const int nblk = double_sided ? 4 : 2;
    // vertex ids are int32; the faces of an image are at most 2 (4) per pixel, and their offsets are int32 as well
    A3R_CHECK_ARG((size_t)v->N * v->P < (1ull << 31), "%s: N * P = %zu does not fit the int32 vertex index", who, (size_t)v->N * v->P);
    A3R_CHECK_ARG((size_t)nblk * v->N * v->P < (1ull << 31), "%s: up to %d * N * P = %zu faces do not fit the int32 face offsets", who, nblk,
                  (size_t)nblk * v->N * v->P);
    const size_t need = a3r_align_scene_mesh_workspace_bytes(v->N, v->P);
    if (int rc = check_workspace(who, workspace, workspace_bytes, need)) return rc;
    *vec = v->P % 4 == 0 && aligned_to(v->depth, 16) && aligned_to(conf, 16) && (!v->mono || aligned_to(v->mono, 16)) && (!dyn || aligned_to(dyn, 16)) &&
           (!rgb || aligned_to(rgb, 16));
    const int nch = scene_nchunks(v->P), T = v->N * nch, TF = T * nblk;
    char* ws = static_cast<char*>(workspace);
    int* voff = reinterpret_cast<int*>(ws);
    int* foff = reinterpret_cast<int*>(ws + compact_offsets_bytes(T));
    int* rank = reinterpret_cast<int*>(ws + compact_offsets_bytes(T) + compact_offsets_bytes(4 * (size_t)T));
    s->conf = conf; s->dyn = dyn; s->rgb = rgb; s->thr = thr; s->offsets = voff;
    s->out_xyz = nullptr; s->out_rgb = nullptr; s->out_index = nullptr; s->rank = rank;
    m->rank = rank; m->voff = voff; m->foff = foff; m->rgb = nullptr; m->out_faces = nullptr; m->out_rgb = nullptr;
    m->P = v->P; m->nblk = nblk;
    launch_compact<false>(*v, *s, *vec, st);
    compact_scan(voff, T, st);
    launch_faces<false>(*v, *m, st);
    compact_scan(foff, TF, st);
    A3R_LAUNCH_CHECK();
    int totals[2] = {0, 0};
    A3R_HIP(compact_read_total(voff, T, &totals[0], st));
    A3R_HIP(compact_read_total(foff, TF, &totals[1], st));
    A3R_HIP(hipStreamSynchronize(st));
    *n_vertices = totals[0];
    *n_faces = totals[1];
    return A3R_OK;
}

extern "C" int a3r_align_scene_mesh_count(a3r_align_t a, const float* conf, float thr, const uint8_t* dyn, void* workspace,
                                          size_t workspace_bytes, int double_sided, long long* n_vertices_host, long long* n_faces_host,
                                          void* stream) {
    A3R_CHECK_ARG(n_vertices_host && n_faces_host, "a3r_align_scene_mesh_count: null n_vertices_host / n_faces_host");
    SceneView v;
    SceneSel s;
    SceneMesh m;
    bool vec;
    *n_vertices_host = *n_faces_host = 0;
    return mesh_count(a, "a3r_align_scene_mesh_count", conf, thr, dyn, nullptr, workspace, workspace_bytes, double_sided, as_stream(stream), &v,
                      &s, &m, &vec, n_vertices_host, n_faces_host);
}

extern "C" int a3r_align_scene_mesh_export(a3r_align_t a, const float* conf, float thr, const uint8_t* dyn, const uint8_t* rgb, void* workspace,
                                           size_t workspace_bytes, int double_sided, long long vertex_capacity, long long face_capacity,
                                           float* out_xyz, uint8_t* out_vertex_rgb, int* out_faces, uint8_t* out_face_rgb,
                                           long long* n_vertices_host, long long* n_faces_host, void* stream) {
    const char* who = "a3r_align_scene_mesh_export";
    A3R_CHECK_ARG(n_vertices_host && n_faces_host, "%s: null n_vertices_host / n_faces_host", who);
    A3R_CHECK_ARG(vertex_capacity >= 0 && face_capacity >= 0, "%s: negative capacity", who);
    A3R_CHECK_ARG(out_xyz || vertex_capacity == 0, "%s: null out_xyz (only a vertex capacity of 0 needs no buffer)", who);
    A3R_CHECK_ARG(out_faces || face_capacity == 0, "%s: null out_faces (only a face capacity of 0 needs no buffer)", who);
    A3R_CHECK_ARG(!out_vertex_rgb || rgb, "%s: out_vertex_rgb needs the rgb source buffer", who);
    A3R_CHECK_ARG(!out_face_rgb || rgb, "%s: out_face_rgb needs the rgb source buffer", who);
    hipStream_t st = as_stream(stream);
    SceneView v;
    SceneSel s;
    SceneMesh m;
    bool vec;
    long long nv = 0, nf = 0;
    *n_vertices_host = *n_faces_host = 0;
    // the counts are always taken afresh: the offsets and the rank map in the workspace then belong to exactly these inputs
    if (int rc = mesh_count(a, who, conf, thr, dyn, out_vertex_rgb ? rgb : nullptr, workspace, workspace_bytes, double_sided, st, &v, &s, &m,
                            &vec, &nv, &nf))
        return rc;
    *n_vertices_host = nv;
    *n_faces_host = nf;
    A3R_CHECK_ARG(nv <= vertex_capacity, "%s: vertex capacity %lld is smaller than the %lld kept pixels (nothing was written)", who,
                  vertex_capacity, nv);
    A3R_CHECK_ARG(nf <= face_capacity, "%s: face capacity %lld is smaller than the %lld faces (nothing was written)", who, face_capacity, nf);
    if (nv == 0) return A3R_OK;
    s.out_xyz = out_xyz; s.out_rgb = out_vertex_rgb; s.rank = nullptr;
    launch_compact<true>(v, s, vec, st);
    if (nf > 0) {
        m.rgb = rgb; m.out_faces = out_faces; m.out_rgb = out_face_rgb;
        launch_faces<true>(v, m, st);
    }
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" size_t a3r_align_scene_clean_workspace_bytes(int N, int P) {
    if (N <= 0 || P <= 0) return 0;
    return clean_cam_bytes(N) + align_up((size_t)N * P * sizeof(float), 256);
}

// Enqueues 1 + N kernels on `stream`: no allocation, no synchronisation, nothing read back (graph-capturable).
extern "C" int a3r_align_scene_clean(a3r_align_t a, float* conf, float tol, float bad_conf, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    const char* who = "a3r_align_scene_clean";
    A3R_CHECK_ARG(conf, "%s: null confidence buffer", who);
    A3R_CHECK_ARG(tol >= 0.f && tol < 1.f, "%s: tol = %g is outside [0, 1)", who, (double)tol);          // false for NaN too
    A3R_CHECK_ARG(bad_conf == bad_conf, "%s: bad_conf is NaN", who);
    hipStream_t st = as_stream(stream);
    SceneView v;
    if (int rc = align_scene_view(a, st, &v, who)) return rc;
    const size_t need = a3r_align_scene_clean_workspace_bytes(v.N, v.P);
    if (int rc = check_workspace(who, workspace, workspace_bytes, need)) return rc;
    float* cam = static_cast<float*>(workspace);
    float* dense = reinterpret_cast<float*>(static_cast<char*>(workspace) + clean_cam_bytes(v.N));
    const bool vec = v.P % 4 == 0 && aligned_to(v.depth, 16) && aligned_to(conf, 16) && (!v.mono || aligned_to(v.mono, 16));
    const float keep_frac = (float)(1.0 - (double)tol);
    const int nch = scene_nchunks(v.P);
#define A3R_SCENE_LAUNCH(MONOV, VECV)                                                                                                      \
    do {                                                                                                                                   \
        hipLaunchKernelGGL((scene_clean_prep_kernel<MONOV, VECV>), dim3(nch, v.N), dim3(STPB), 0, st, v, cam, dense, v.img_xf, v.imw,      \
                           v.imarea);                                                                                                      \
        for (int i = 0; i < v.N; i++)                                                                                                      \
            hipLaunchKernelGGL((scene_clean_kernel<MONOV, VECV>), dim3(nch), dim3(STPB), 0, st, v, conf, i, cam, dense, keep_frac,         \
                               bad_conf, v.img_xf, v.imw, v.imarea);                                                                       \
    } while (0)
    if (v.mono) { if (vec) A3R_SCENE_LAUNCH(true, true); else A3R_SCENE_LAUNCH(true, false); }
    else        { if (vec) A3R_SCENE_LAUNCH(false, true); else A3R_SCENE_LAUNCH(false, false); }
#undef A3R_SCENE_LAUNCH
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
