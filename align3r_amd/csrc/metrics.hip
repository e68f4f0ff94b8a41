// Video-depth evaluation for gfx950 (tool/depth_metrics.py of the package; the reference's tool/depth_test.py:689-835): one scale and
// shift for the whole clip by the chosen rule, a clip to [1e-5, depth_max], AbsRel / SqRel / RMSE / logRMSE / delta.
//
// pred, gt: float32 [n].  A pixel is valid iff 1e-3 < gt < depth_max, compared in float32 as numpy compares a float32 array with a
// Python float (both strict: a NaN gt is invalid).  Validity is evaluated on the fly in every pass (only 'scale' compacts).  All
// arithmetic on a valid pixel is float64 on the float32 inputs, every operation rounded on its own (no FMA: s * p + t rounds as
// numpy rounds it).
//
// Streaming passes, 8 B per pixel each:
//   depth_pass_kernel<MODE>   grid (<= DGRID workgroups, grid stride): per-thread float64 sums, a shuffle reduction per wave, the
//                             four wave sums added in wave order by thread 0, one partial row per workgroup.  16-byte loads when
//                             pred and gt are both 16-byte aligned (the n % 4 tail goes to the first threads), scalar loads otherwise.
//                             MODE: first moments, centred second moments, the LAD sums, the metric sums.
//   'scale' (mean ratio + 10 IRLS passes) is the exception: it compacts the valid pixels in order (the workgroup rank of compact.h)
//   and adds with numpy's summation tree, bit for bit the host's sums (see there for why).
//   depth_hist_kernel         one 8-bit digit of the radix select, for four order statistics at once (the two middle ones of the valid
//                             pred and of the valid gt): LDS histograms, integer atomics to the global ones.
// One-wave kernels between the passes fold the partial rows in a fixed order (lane l adds rows l, l + 64, ..., then a butterfly)
// and write the next point into the state block in the workspace; the pass kernels read their parameters from there, so a whole
// solve is enqueued without a host synchronisation.  No floating-point atomics anywhere: the result is a function of the inputs.
//
// LAD: minimise f(s, t) = sum |s p + t - g|, convex and piecewise linear, by the central-cut ellipsoid method in two dimensions on
// (u, v) = (s / s0, t / T), s0 = median(g) / |median(p)|, T = median(g).  Start: centre (1, 0), the disc of radius 4.  A pass
// evaluates f and the subgradient (s0 sum sign(r) p, T sum sign(r)) at the centre; the best centre seen is kept.  lad_passes(0) = 150
// passes; if the best point is then farther than half the radius from (1, 0) the minimiser may lie outside the disc: the radius
// grows fourfold and the search restarts (at most LAD_ROUNDS rounds; the best point is kept across rounds).  All rounds are enqueued;
// once the solve is done the remaining kernels return at their first instruction.
#include "common.h"
#include "compact.h"

#include <cmath>

#pragma clang fp contract(off)

namespace a3r {

constexpr int DTPB = 256;
constexpr int DGRID = 1024;                     // workgroups of a pass at most: 4 per CU
constexpr int DNS = 8;                          // doubles of a partial row
constexpr int LAD_ROUNDS = 3;
__host__ __device__ constexpr int lad_passes(int round) { return 150 + 50 * round; }      // a fourfold radius costs about 11 more cuts

enum { DP_MOM1 = 0, DP_MOM2, DP_LAD, DP_METRICS };

// the state block of one call (workspace); written by the one-wave kernels only
struct DepthState {
    double s, t;                                // the point the next pass evaluates: (scale, shift), (mean p, mean g) for DP_MOM2
    double n_valid;
    double os[4];                               // order statistics: pred lower / upper middle, gt lower / upper middle
    double med_p, med_g;
    double s0, T;                               // LAD normalisation
    double cu, cv, p11, p12, p22, radius;       // ellipsoid: centre and shape matrix in (u, v)
    double best_f, best_s, best_t, best_u, best_v;
    double passes, rounds;
    unsigned prefix[4], rank[4];                // radix select: key bits fixed so far, rank inside that bucket
    int round_pass, done, bad;                  // bad: fewer than 2 valid pixels
    unsigned m;                                 // 'scale': valid pixels (the length of the compacted arrays)
};

static size_t dws_partial_bytes() { return align_up((size_t)DGRID * DNS * sizeof(double), 256); }
static size_t dws_state_bytes() { return align_up(sizeof(DepthState), 256); }
static size_t dws_hist_bytes() { return 4 * 256 * sizeof(unsigned); }
// 'scale' only: per-chunk counts, the compacted valid pred and gt, the sums of numpy's reduction buffers
constexpr int SCH = 1024;                       // elements of a compaction chunk (one workgroup)
constexpr int NPB = 8192;                       // numpy's reduction buffer: np.sum adds the pairwise sums of 8192 consecutive elements in order
constexpr int NPL = 128;                        // the leaf of numpy's pairwise sum
constexpr int NPT = 128;                        // threads of a buffer's workgroup: the leaves of a tree of depth 7
static size_t dws_cnt_bytes(long long n) { return align_up((size_t)((n + SCH - 1) / SCH) * sizeof(unsigned), 256); }
static size_t dws_compact_bytes(long long n) { return align_up((size_t)n * sizeof(float), 256); }
static size_t dws_csum_bytes(long long n) { return align_up((size_t)((n + NPB - 1) / NPB) * 2 * sizeof(double), 256); }

struct DepthView {
    const float* pred;
    const float* gt;
    long long n;
    float lo, hi;                               // validity bounds in float32
    double dmax;
    int G;                                      // workgroups of a pass
    double* partial;                            // [G, DNS]
    DepthState* st;
    unsigned* hist;                             // [4, 256]
    unsigned* cnt;                              // [ceil(n / SCH)]: valid pixels per chunk, then their exclusive prefix sums
    float* cp;                                  // [n]: the valid pred in order
    float* cg;                                  // [n]: the valid gt in order
    double* csum;                               // [ceil(n / NPB), 2]
};

template <int MODE> struct DpSums { static constexpr int n = MODE == DP_METRICS ? 8 : MODE == DP_MOM2 ? 2 : 4; };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// order-preserving uint32 key of a float32 (negative values below positive ones, -0 below +0)
__device__ __forceinline__ unsigned f32_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

template <int MODE>
__device__ __forceinline__ void dp_pixel(float pf, float gf, float lo, float hi, double a, double b, double dmax, double (&acc)[DpSums<MODE>::n]) {
    if (!(gf > lo && gf < hi)) return;
    const double p = (double)pf, g = (double)gf;
    if (MODE == DP_MOM1) {                      // nanmean(pred): sum and count of the non-NaN; mean(gt)
        if (p == p) { acc[0] += p; acc[1] += 1.0; }
        acc[2] += g;
        acc[3] += 1.0;
    } else if (MODE == DP_MOM2) {               // a = mean p, b = mean g
        const double dp = p - a, dg = g - b;
        acc[0] += dp * dp;
        acc[1] += dp * dg;
    } else if (MODE == DP_LAD) {                // a = s, b = t
        const double r = (a * p + b) - g;
        const double sg = r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0);
        acc[0] += fabs(r);
        acc[1] += sg * p;
        acc[2] += sg;
        acc[3] += 1.0;
    } else {                                    // a = s, b = t
        double x = a * p + b;
        x = x != x ? x : fmin(fmax(x, 1e-5), dmax);
        const double d = x - g, d2 = d * d, l = log(x) - log(g);
        const double ratio = fmax(x / g, g / x);
        acc[0] += fabs(d) / g;
        acc[1] += d2 / g;
        acc[2] += d2;
        acc[3] += l * l;
        acc[4] += ratio < 1.25 ? 1.0 : 0.0;
        acc[5] += ratio < 1.5625 ? 1.0 : 0.0;
        acc[6] += ratio < 1.953125 ? 1.0 : 0.0;
        acc[7] += 1.0;
    }
}

// grid (v.G), grid stride.  STOPPABLE: returns at once when the solve is done.
template <int MODE, bool VEC, bool STOPPABLE>
__global__ __launch_bounds__(DTPB) void depth_pass_kernel(DepthView v) {
    constexpr int NS = DpSums<MODE>::n;
    __shared__ double sh[DTPB / 64][NS];
    if (STOPPABLE && v.st->done) return;
    const double a = v.st->s, b = v.st->t;
    const int tid = threadIdx.x;
    const long long gtid = (long long)blockIdx.x * DTPB + tid, stride = (long long)gridDim.x * DTPB;
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] = 0.0;
    if (VEC) {
        const long long n4 = v.n >> 2;
        const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(v.pred);
        const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(v.gt);
#pragma unroll 2
        for (long long i = gtid; i < n4; i += stride) {
            const f32x4 p = p4[i], g = g4[i];
            dp_pixel<MODE>(p.x, g.x, v.lo, v.hi, a, b, v.dmax, acc);
            dp_pixel<MODE>(p.y, g.y, v.lo, v.hi, a, b, v.dmax, acc);
            dp_pixel<MODE>(p.z, g.z, v.lo, v.hi, a, b, v.dmax, acc);
            dp_pixel<MODE>(p.w, g.w, v.lo, v.hi, a, b, v.dmax, acc);
        }
        const long long i = (n4 << 2) + gtid;   // the tail: at most three elements
        if (i < v.n) dp_pixel<MODE>(v.pred[i], v.gt[i], v.lo, v.hi, a, b, v.dmax, acc);
    } else {
#pragma unroll 4
        for (long long i = gtid; i < v.n; i += stride) dp_pixel<MODE>(v.pred[i], v.gt[i], v.lo, v.hi, a, b, v.dmax, acc);
    }
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] = wave_sum_f64(acc[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS; k++) sh[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid == 0) {
        double* o = v.partial + (size_t)blockIdx.x * DNS;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            double s = acc[k];
#pragma unroll
            for (int w = 1; w < DTPB / 64; w++) s += sh[w][k];
            o[k] = s;
        }
    }
}

// one wave: the sums of the first NS columns of the partial rows, in a fixed order; every lane gets them
template <int NS>
__device__ __forceinline__ void depth_fold(const DepthView& v, double (&sum)[NS]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; k++) sum[k] = 0.0;
    for (int c = lane; c < v.G; c += 64) {
#pragma unroll
        for (int k = 0; k < NS; k++) sum[k] += v.partial[(size_t)c * DNS + k];
    }
#pragma unroll
    for (int k = 0; k < NS; k++) sum[k] = wave_sum_f64(sum[k]);
}

// grid (v.G), grid stride: digit `d` (0 = most significant byte) of the four selects
template <bool VEC>
__global__ __launch_bounds__(DTPB) void depth_hist_kernel(DepthView v, int d) {
    __shared__ unsigned sh[4 * 256];
    const int tid = threadIdx.x;
    for (int i = tid; i < 4 * 256; i += DTPB) sh[i] = 0;
    const unsigned mask = d == 0 ? 0u : 0xFFFFFFFFu << (32 - 8 * d);
    const int shift = 24 - 8 * d;
    unsigned pre[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pre[k] = d == 0 ? 0u : v.st->prefix[k];
    __syncthreads();
    auto pixel = [&](float pf, float gf) {
        if (!(gf > v.lo && gf < v.hi)) return;
        const unsigned kp = f32_key(pf), kg = f32_key(gf);
        const unsigned bp = (kp >> shift) & 255u, bg = (kg >> shift) & 255u;
        if ((kp & mask) == pre[0]) atomicAdd(&sh[bp], 1u);
        if ((kp & mask) == pre[1]) atomicAdd(&sh[256 + bp], 1u);
        if ((kg & mask) == pre[2]) atomicAdd(&sh[512 + bg], 1u);
        if ((kg & mask) == pre[3]) atomicAdd(&sh[768 + bg], 1u);
    };
    const long long gtid = (long long)blockIdx.x * DTPB + tid, stride = (long long)gridDim.x * DTPB;
    if (VEC) {
        const long long n4 = v.n >> 2;
        const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(v.pred);
        const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(v.gt);
        for (long long i = gtid; i < n4; i += stride) {
            const f32x4 p = p4[i], g = g4[i];
            pixel(p.x, g.x); pixel(p.y, g.y); pixel(p.z, g.z); pixel(p.w, g.w);
        }
        const long long i = (n4 << 2) + gtid;
        if (i < v.n) pixel(v.pred[i], v.gt[i]);
    } else {
        for (long long i = gtid; i < v.n; i += stride) pixel(v.pred[i], v.gt[i]);
    }
    __syncthreads();
    for (int i = tid; i < 4 * 256; i += DTPB)
        if (sh[i]) atomicAdd(&v.hist[i], sh[i]);
}

// one wave: zero the state and the histograms
__global__ __launch_bounds__(64) void depth_init_kernel(DepthView v) {
    const int lane = threadIdx.x;
    unsigned* w = reinterpret_cast<unsigned*>(v.st);
    for (int i = lane; i < (int)(sizeof(DepthState) / sizeof(unsigned)); i += 64) w[i] = 0u;
    for (int i = lane; i < 4 * 256; i += 64) v.hist[i] = 0u;
}

// one wave: pick the bucket of digit d for each of the four selects, clear the histograms for the next digit; after the last digit
// the order statistics and the medians (np.median: the mean of the two middle values)
__global__ __launch_bounds__(64) void depth_select_kernel(DepthView v, int d) {
    __shared__ unsigned sh[4 * 256];
    const int lane = threadIdx.x;
    for (int i = lane; i < 4 * 256; i += 64) { sh[i] = v.hist[i]; v.hist[i] = 0u; }
    __syncthreads();
    DepthState* st = v.st;
    float val = 0.f;
    if (lane < 4) {
        const unsigned* h = sh + lane * 256;
        unsigned rank;
        if (d == 0) {
            unsigned m = 0;
            for (int b = 0; b < 256; b++) m += h[b];
            rank = m == 0 ? 0u : ((lane & 1) ? m / 2 : (m - 1) / 2);
            if (lane == 0) {
                st->n_valid = (double)m;
                if (m < 2) { st->bad = 1; st->done = 1; }
            }
        } else {
            rank = st->rank[lane];
        }
        unsigned cum = 0, bucket = 255;
        for (int b = 0; b < 256; b++) {
            const unsigned c = h[b];
            if (rank < cum + c) { bucket = b; break; }
            cum += c;
        }
        const unsigned pre = (d == 0 ? 0u : st->prefix[lane]) | (bucket << (24 - 8 * d));
        st->prefix[lane] = pre;
        st->rank[lane] = rank - cum;
        val = f32_unkey(pre);
    }
    if (d == 3) {
        const double o0 = (double)__shfl(val, 0), o1 = (double)__shfl(val, 1), o2 = (double)__shfl(val, 2), o3 = (double)__shfl(val, 3);
        if (lane == 0) {
            st->os[0] = o0; st->os[1] = o1; st->os[2] = o2; st->os[3] = o3;
            st->med_p = (o0 + o1) / 2.0;
            st->med_g = (o2 + o3) / 2.0;
        }
    }
}

// one wave: the start of a LAD round
__device__ __forceinline__ void lad_start_round(DepthState* st, double radius) {
    st->radius = radius;
    st->cu = 1.0; st->cv = 0.0;
    st->p11 = radius * radius; st->p12 = 0.0; st->p22 = radius * radius;
    st->round_pass = 0;
    st->s = st->s0; st->t = 0.0;
}

__global__ __launch_bounds__(64) void depth_lad_init_kernel(DepthView v) {
    DepthState* st = v.st;
    if (threadIdx.x != 0 || st->done) return;
    const double r = st->med_g / fabs(st->med_p);
    st->s0 = (r > 0.0 && r < INFINITY) ? r : 1.0;       // a zero or NaN median of pred: search around s = 1
    st->T = st->med_g;                                  // valid gt is positive: median |g| = median g
    st->best_f = INFINITY;
    st->best_s = st->s0; st->best_t = 0.0; st->best_u = 1.0; st->best_v = 0.0;
    lad_start_round(st, 4.0);
}

// one wave: fold the LAD sums at the centre, keep the best point, cut the ellipsoid through its centre
__global__ __launch_bounds__(64) void depth_lad_step_kernel(DepthView v) {
    DepthState* st = v.st;
    if (st->done) return;
    double sum[4];
    depth_fold<4>(v, sum);
    if (threadIdx.x != 0) return;
    const double f = sum[0], gu = st->s0 * sum[1], gv = st->T * sum[2];
    double cu = st->cu, cv = st->cv, p11 = st->p11, p12 = st->p12, p22 = st->p22;
    if (f < st->best_f) { st->best_f = f; st->best_s = st->s; st->best_t = st->t; st->best_u = cu; st->best_v = cv; }
    const double pg0 = p11 * gu + p12 * gv, pg1 = p12 * gu + p22 * gv;
    const double q = gu * pg0 + gv * pg1;
    const int round = (int)st->rounds;
    int rp = st->round_pass + 1;
    st->passes += 1.0;
    if (q > 0.0 && q < INFINITY) {
        const double sq = sqrt(q);                      // n = 2: c -= P g / (3 sqrt(g'Pg)), P = 4/3 (P - 2/3 P g g' P / g'Pg)
        cu -= pg0 / sq / 3.0;
        cv -= pg1 / sq / 3.0;
        p11 = (4.0 / 3.0) * (p11 - (2.0 / 3.0) * (pg0 * pg0 / q));
        p12 = (4.0 / 3.0) * (p12 - (2.0 / 3.0) * (pg0 * pg1 / q));
        p22 = (4.0 / 3.0) * (p22 - (2.0 / 3.0) * (pg1 * pg1 / q));
    } else {
        rp = lad_passes(round);                         // a zero subgradient (the centre is a minimiser) or a degenerate ellipsoid
    }
    if (rp >= lad_passes(round)) {
        const double du = st->best_u - 1.0, dv = st->best_v, half = 0.5 * st->radius;
        if (du * du + dv * dv <= half * half || round == LAD_ROUNDS - 1) {
            st->done = 1;
        } else {
            st->rounds = (double)(round + 1);
            lad_start_round(st, 4.0 * st->radius);
        }
        return;
    }
    st->cu = cu; st->cv = cv; st->p11 = p11; st->p12 = p12; st->p22 = p22;
    st->round_pass = rp;
    st->s = st->s0 * cu; st->t = st->T * cv;
}

// one wave: after DP_MOM1: (mean p, mean g) for the centred pass
__global__ __launch_bounds__(64) void depth_mom1_step_kernel(DepthView v) {
    double sum[4];
    depth_fold<4>(v, sum);
    if (threadIdx.x != 0) return;
    DepthState* st = v.st;
    st->n_valid = sum[3];
    if (sum[3] < 2.0) st->bad = 1;
    const double mp = sum[0] / sum[1], mg = sum[2] / sum[3];
    st->s = mp; st->t = mg; st->med_p = mp; st->med_g = mg;
}

__global__ __launch_bounds__(64) void depth_mom2_step_kernel(DepthView v) {
    double sum[2];
    depth_fold<2>(v, sum);
    if (threadIdx.x != 0) return;
    DepthState* st = v.st;
    const double s = sum[1] / sum[0];
    st->best_s = s;
    st->best_t = st->med_g - s * st->med_p;
}

// ---- 'scale': mean ratio + 10 IRLS passes with weights 1 / (|s p - g| + 1e-8).  The passes expand: a pixel whose residual passes near
// zero weighs up to 1e8 ordinary ones, and a last-bit difference in the first sums grows about 1e12 times over the ten passes (the
// host's own answer moves by 1e-3 when its pixels are merely reordered).  So this rule is evaluated with THE HOST'S SUMS, bit for bit:
// the valid pixels compacted in order, every term by the host's expression, and numpy's summation tree -- np.sum of a contiguous
// float64 array starts at 0 and adds, in order, one pairwise sum per reduction buffer of 8192 elements; a pairwise sum splits n > 128
// into n2 = n / 2 rounded down to a multiple of 8 and n - n2, and adds a leaf of 8 <= n <= 128 with eight strided accumulators,
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 tail in order (fewer than 8 elements: in order from 0).

// grid (ceil(n / SCH)): valid pixels of the chunk
__global__ __launch_bounds__(DTPB) void depth_count_kernel(DepthView v) {
    __shared__ int wave_total[DTPB / 64];
    const long long e0 = (long long)blockIdx.x * SCH + threadIdx.x * 4;
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        ok[k] = false;
        if (e0 + k < v.n) { const float g = v.gt[e0 + k]; ok[k] = g > v.lo && g < v.hi; }
    }
    int first, total;
    block_rank<DTPB, 4>(ok, wave_total, &first, &total);
    if (threadIdx.x == 0) v.cnt[blockIdx.x] = (unsigned)total;
}

// one workgroup: exclusive prefix sums of the nb chunk counts, in place; the total
__global__ __launch_bounds__(DTPB) void depth_scan_kernel(DepthView v, int nb) {
    __shared__ unsigned sh[DTPB];
    const int tid = threadIdx.x, per = (nb + DTPB - 1) / DTPB;
    const long long lo = (long long)tid * per;
    const int b0 = (int)(lo < nb ? lo : nb), b1 = b0 + per < nb ? b0 + per : nb;
    unsigned sum = 0;
    for (int b = b0; b < b1; b++) sum += v.cnt[b];
    sh[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned run = 0;
        for (int t = 0; t < DTPB; t++) { const unsigned x = sh[t]; sh[t] = run; run += x; }
        v.st->m = run;
        v.st->n_valid = (double)run;
        if (run < 2) v.st->bad = 1;
    }
    __syncthreads();
    unsigned run = sh[tid];
    for (int b = b0; b < b1; b++) { const unsigned x = v.cnt[b]; v.cnt[b] = run; run += x; }
}

// grid (ceil(n / SCH)): the valid pixels of the chunk to their places in the compacted arrays, in order
__global__ __launch_bounds__(DTPB) void depth_scatter_kernel(DepthView v) {
    __shared__ int wave_total[DTPB / 64];
    const long long e0 = (long long)blockIdx.x * SCH + threadIdx.x * 4;
    float p[4], g[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        ok[k] = false; p[k] = 0.f; g[k] = 0.f;
        if (e0 + k < v.n) { p[k] = v.pred[e0 + k]; g[k] = v.gt[e0 + k]; ok[k] = g[k] > v.lo && g[k] < v.hi; }
    }
    int first, total;
    block_rank<DTPB, 4>(ok, wave_total, &first, &total);
    unsigned r = v.cnt[blockIdx.x] + (unsigned)first;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (ok[k]) { v.cp[r] = p[k]; v.cg[r] = g[k]; r++; }
}

// the two terms of compacted pixel j.  IRLS: (w p g, w p^2) as the host writes them; otherwise (p, g)
template <bool IRLS>
__device__ __forceinline__ void sc_terms(const DepthView& v, unsigned j, double s, double& a, double& b) {
    const double p = (double)v.cp[j], g = (double)v.cg[j];
    if (IRLS) {
        const double w = 1.0 / (fabs(s * p - g) + 1e-8);
        a = (w * p) * g;
        b = w * (p * p);
    } else {
        a = p;
        b = g;
    }
}

// grid (ceil(n / NPB)) x NPT threads: numpy's pairwise sum of one reduction buffer [c NPB, min(m, (c + 1) NPB)).  Thread t walks the
// summation tree from the root by the bits of t, high bit first; the thread whose remaining bits are zero when the walk reaches a
// leaf owns it.  Then the tree is folded level by level: an inner node's value is left + right, kept at its leftmost leaf's thread.
template <bool IRLS>
__global__ __launch_bounds__(NPT) void depth_scale_sum_kernel(DepthView v) {
    __shared__ double va[NPT], vb[NPT];
    __shared__ int depth_of[NPT];
    const unsigned m = v.st->m;
    const unsigned c0 = blockIdx.x * (unsigned)NPB;
    if (c0 >= m) return;
    const double s = v.st->s;
    const int t = threadIdx.x;
    unsigned j = c0, n = m - c0 < (unsigned)NPB ? m - c0 : (unsigned)NPB;
    int depth = 0;
    bool own = true;
    for (int bit = 6; bit >= 0 && n > (unsigned)NPL; bit--, depth++) {
        unsigned n2 = n / 2;
        n2 -= n2 % 8;
        if ((t >> bit) & 1) { j += n2; n -= n2; } else { n = n2; }
    }
    own = (t & ((1 << (7 - depth)) - 1)) == 0;      // 7 splits always reach a leaf: 8191 / 128 + 8 < 128
    double A = 0.0, B = 0.0;
    if (own) {
        double a, b;
        if (n < 8) {
            for (unsigned i = 0; i < n; i++) { sc_terms<IRLS>(v, j + i, s, a, b); A += a; B += b; }
        } else {
            double ra[8], rb[8];
#pragma unroll
            for (int k = 0; k < 8; k++) sc_terms<IRLS>(v, j + k, s, ra[k], rb[k]);
            unsigned i = 8;
            for (; i < n - (n % 8); i += 8) {
#pragma unroll
                for (int k = 0; k < 8; k++) { sc_terms<IRLS>(v, j + i + k, s, a, b); ra[k] += a; rb[k] += b; }
            }
            A = ((ra[0] + ra[1]) + (ra[2] + ra[3])) + ((ra[4] + ra[5]) + (ra[6] + ra[7]));
            B = ((rb[0] + rb[1]) + (rb[2] + rb[3])) + ((rb[4] + rb[5]) + (rb[6] + rb[7]));
            for (; i < n; i++) { sc_terms<IRLS>(v, j + i, s, a, b); A += a; B += b; }
        }
    }
    va[t] = A; vb[t] = B;
    depth_of[t] = own ? depth : 8;
    __syncthreads();
    for (int l = 6; l >= 0; l--) {
        const int span = 1 << (7 - l);
        if ((t & (span - 1)) == 0 && depth_of[t] > l) { va[t] += va[t + span / 2]; vb[t] += vb[t + span / 2]; }
        __syncthreads();
    }
    if (t == 0) { v.csum[2 * (size_t)blockIdx.x] = va[0]; v.csum[2 * (size_t)blockIdx.x + 1] = vb[0]; }
}

// one wave: np.sum's outer loop -- from 0, the buffer sums in order -- and the next s
template <bool IRLS>
__global__ __launch_bounds__(64) void depth_scale_step_kernel(DepthView v) {
    DepthState* st = v.st;
    const int lane = threadIdx.x;
    const unsigned m = st->m;
    const int nc = (int)((m + NPB - 1) / NPB);
    double A = 0.0, B = 0.0;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane, cnt = nc - c0 < 64 ? nc - c0 : 64;
        const double a = c < nc ? v.csum[2 * (size_t)c] : 0.0, b = c < nc ? v.csum[2 * (size_t)c + 1] : 0.0;
        for (int k = 0; k < cnt; k++) { A += __shfl(a, k); B += __shfl(b, k); }
    }
    if (lane != 0) return;
    if (IRLS) { st->s = A / B; st->passes += 1.0; }
    else      { st->s = (B / (double)m) / (A / (double)m); st->t = 0.0; }       // np.nanmean(gt) / np.nanmean(pred)
}

// one wave: (scale, shift) and the info block
__global__ __launch_bounds__(64) void depth_align_finish_kernel(DepthView v, int mode, double* __restrict__ st_dev, double* __restrict__ info) {
    if (threadIdx.x != 0) return;
    const DepthState* st = v.st;
    double s, t;
    if (mode == A3R_DEPTH_ALIGN_LAD || mode == A3R_DEPTH_ALIGN_LSTSQ) { s = st->best_s; t = st->best_t; }
    else if (mode == A3R_DEPTH_ALIGN_SCALE) { s = fmax(st->s, 1e-3); t = 0.0; }
    else { s = st->med_g / st->med_p; t = 0.0; }
    if (st->bad) s = t = __builtin_nan("");
    st_dev[0] = s; st_dev[1] = t;
    const bool sel = mode == A3R_DEPTH_ALIGN_LAD || mode == A3R_DEPTH_ALIGN_MEDIAN;
    info[0] = st->n_valid;
    info[1] = mode == A3R_DEPTH_ALIGN_LAD ? st->best_f : 0.0;
    info[2] = st->passes;
    info[3] = st->rounds;
#pragma unroll
    for (int k = 0; k < 4; k++) info[4 + k] = sel ? st->os[k] : 0.0;
    info[8] = sel ? st->med_p : 0.0;
    info[9] = sel ? st->med_g : 0.0;
    info[10] = st->s0;
    info[11] = st->T;
#pragma unroll
    for (int k = 12; k < A3R_DEPTH_INFO_DOUBLES; k++) info[k] = 0.0;
}

// one wave: the metric means from the sums
__global__ __launch_bounds__(64) void depth_metrics_finish_kernel(DepthView v, double* __restrict__ out) {
    double sum[8];
    depth_fold<8>(v, sum);
    if (threadIdx.x != 0) return;
    const double n = sum[7];
    out[0] = sum[0] / n;
    out[1] = sum[1] / n;
    out[2] = sqrt(sum[2] / n);
    out[3] = sqrt(sum[3] / n);
    out[4] = sum[4] / n;
    out[5] = sum[5] / n;
    out[6] = sum[6] / n;
    out[7] = n;
}

// one wave: (scale, shift) from the caller's buffer into the state block the metric pass reads
__global__ __launch_bounds__(64) void depth_metrics_init_kernel(DepthView v, const double* __restrict__ st_dev) {
    if (threadIdx.x != 0) return;
    v.st->s = st_dev[0];
    v.st->t = st_dev[1];
}

}  // namespace a3r

// =============================================================================================== host
using namespace a3r;

extern "C" size_t a3r_depth_eval_workspace_bytes(long n) {
    if (n <= 0) return 0;
    return dws_partial_bytes() + dws_state_bytes() + dws_hist_bytes() + dws_cnt_bytes(n) + 2 * dws_compact_bytes(n) + dws_csum_bytes(n);
}

static int depth_check(const char* who, const float* pred, const float* gt, long n, double depth_max, void* ws, size_t ws_bytes, DepthView& v) {
    A3R_CHECK_ARG(pred, "%s: null pred", who);
    A3R_CHECK_ARG(gt, "%s: null gt", who);
    A3R_CHECK_ARG(n > 0, "%s: n = %ld must be positive", who, n);
    A3R_CHECK_ARG((long long)n < (1ll << 31), "%s: n = %ld is too large (the select counts in 32 bits)", who, n);
    A3R_CHECK_ARG(depth_max > 1e-3, "%s: depth_max = %g must be above 1e-3", who, depth_max);      // false for a NaN
    A3R_CHECK_ARG(ws, "%s: null workspace", who);
    const size_t need = a3r_depth_eval_workspace_bytes(n);
    A3R_CHECK_ARG(ws_bytes >= need, "%s: workspace_bytes too small (%zu < %zu)", who, ws_bytes, need);
    A3R_CHECK_ARG(aligned_to(ws, 16), "%s: workspace must be 16-byte aligned", who);
    v.pred = pred; v.gt = gt; v.n = n;
    v.lo = (float)1e-3; v.hi = (float)depth_max; v.dmax = depth_max;
    const long long per = (long long)DTPB * 4;
    const long long blocks = ((long long)n + per - 1) / per;
    v.G = (int)(blocks < DGRID ? blocks : DGRID);
    char* w = static_cast<char*>(ws);
    v.partial = reinterpret_cast<double*>(w);
    v.st = reinterpret_cast<DepthState*>(w + dws_partial_bytes());
    v.hist = reinterpret_cast<unsigned*>(w + dws_partial_bytes() + dws_state_bytes());
    char* x = w + dws_partial_bytes() + dws_state_bytes() + dws_hist_bytes();
    v.cnt = reinterpret_cast<unsigned*>(x);
    v.cp = reinterpret_cast<float*>(x + dws_cnt_bytes(n));
    v.cg = reinterpret_cast<float*>(x + dws_cnt_bytes(n) + dws_compact_bytes(n));
    v.csum = reinterpret_cast<double*>(x + dws_cnt_bytes(n) + 2 * dws_compact_bytes(n));
    return A3R_OK;
}

template <int MODE, bool STOPPABLE>
static void depth_pass(const DepthView& v, bool vec, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((depth_pass_kernel<MODE, true, STOPPABLE>), dim3(v.G), dim3(DTPB), 0, st, v);
    else     hipLaunchKernelGGL((depth_pass_kernel<MODE, false, STOPPABLE>), dim3(v.G), dim3(DTPB), 0, st, v);
}

// Enqueue-only: nothing is allocated, synchronised or read back; the caller reads st_dev / info_dev after the stream.
extern "C" int a3r_depth_align(const float* pred, const float* gt, long n, double depth_max, int mode, void* workspace, size_t workspace_bytes,
                               double* st_dev, double* info_dev, void* stream) {
    const char* who = "a3r_depth_align";
    DepthView v;
    const int rc = depth_check(who, pred, gt, n, depth_max, workspace, workspace_bytes, v);
    if (rc != A3R_OK) return rc;
    A3R_CHECK_ARG(mode >= A3R_DEPTH_ALIGN_LAD && mode <= A3R_DEPTH_ALIGN_MEDIAN, "%s: unknown mode %d (0 lad, 1 lstsq, 2 scale, 3 median)", who, mode);
    A3R_CHECK_ARG(st_dev, "%s: null st_dev", who);
    A3R_CHECK_ARG(info_dev, "%s: null info_dev", who);
    hipStream_t st = as_stream(stream);
    const bool vec = aligned_to(pred, 16) && aligned_to(gt, 16);
    const dim3 one(1), wave(64);
    hipLaunchKernelGGL(depth_init_kernel, one, wave, 0, st, v);
    if (mode == A3R_DEPTH_ALIGN_LAD || mode == A3R_DEPTH_ALIGN_MEDIAN) {
        for (int d = 0; d < 4; d++) {
            if (vec) hipLaunchKernelGGL(depth_hist_kernel<true>, dim3(v.G), dim3(DTPB), 0, st, v, d);
            else     hipLaunchKernelGGL(depth_hist_kernel<false>, dim3(v.G), dim3(DTPB), 0, st, v, d);
            hipLaunchKernelGGL(depth_select_kernel, one, wave, 0, st, v, d);
        }
    }
    if (mode == A3R_DEPTH_ALIGN_LAD) {
        hipLaunchKernelGGL(depth_lad_init_kernel, one, wave, 0, st, v);
        for (int r = 0; r < LAD_ROUNDS; r++)
            for (int k = 0; k < lad_passes(r); k++) {
                depth_pass<DP_LAD, true>(v, vec, st);
                hipLaunchKernelGGL(depth_lad_step_kernel, one, wave, 0, st, v);
            }
    } else if (mode == A3R_DEPTH_ALIGN_LSTSQ) {
        depth_pass<DP_MOM1, false>(v, vec, st);
        hipLaunchKernelGGL(depth_mom1_step_kernel, one, wave, 0, st, v);
        depth_pass<DP_MOM2, false>(v, vec, st);
        hipLaunchKernelGGL(depth_mom2_step_kernel, one, wave, 0, st, v);
    } else if (mode == A3R_DEPTH_ALIGN_SCALE) {
        const int nb = (int)(((long long)n + SCH - 1) / SCH), nnp = (int)(((long long)n + NPB - 1) / NPB);
        hipLaunchKernelGGL(depth_count_kernel, dim3(nb), dim3(DTPB), 0, st, v);
        hipLaunchKernelGGL(depth_scan_kernel, one, dim3(DTPB), 0, st, v, nb);
        hipLaunchKernelGGL(depth_scatter_kernel, dim3(nb), dim3(DTPB), 0, st, v);
        hipLaunchKernelGGL(depth_scale_sum_kernel<false>, dim3(nnp), dim3(NPT), 0, st, v);
        hipLaunchKernelGGL(depth_scale_step_kernel<false>, one, wave, 0, st, v);
        for (int k = 0; k < 10; k++) {
            hipLaunchKernelGGL(depth_scale_sum_kernel<true>, dim3(nnp), dim3(NPT), 0, st, v);
            hipLaunchKernelGGL(depth_scale_step_kernel<true>, one, wave, 0, st, v);
        }
    }
    hipLaunchKernelGGL(depth_align_finish_kernel, one, wave, 0, st, v, mode, st_dev, info_dev);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}

extern "C" int a3r_depth_metrics(const float* pred, const float* gt, long n, double depth_max, const double* st_dev, void* workspace,
                                 size_t workspace_bytes, double* out_dev, void* stream) {
    const char* who = "a3r_depth_metrics";
    DepthView v;
    const int rc = depth_check(who, pred, gt, n, depth_max, workspace, workspace_bytes, v);
    if (rc != A3R_OK) return rc;
    A3R_CHECK_ARG(st_dev, "%s: null st_dev", who);
    A3R_CHECK_ARG(out_dev, "%s: null out_dev", who);
    hipStream_t st = as_stream(stream);
    const bool vec = aligned_to(pred, 16) && aligned_to(gt, 16);
    hipLaunchKernelGGL(depth_metrics_init_kernel, dim3(1), dim3(64), 0, st, v, st_dev);
    depth_pass<DP_METRICS, false>(v, vec, st);
    hipLaunchKernelGGL(depth_metrics_finish_kernel, dim3(1), dim3(64), 0, st, v, out_dev);
    A3R_LAUNCH_CHECK();
    return A3R_OK;
}
