// Body of the aligner's main kernel (align.hip), included once per storage form of the observations: the statements between the
// braces of align_main_kernel (fp32 rows) and of align_main_packed_kernel (packed fp16 rows).  The text is shared by inclusion and
// not through a function: as an inlined function the fp32 kernels came out with other instructions (and four more bytes of
// scratch) than before, and they must not move.  In scope at the point of inclusion: the template parameters MONO, L2, MODE, the
// constants FORM (an ObsForm) and VEC, the kernel arguments, and the two macros that name the form's load and decode:
//   A3R_OBS_LOAD(code, buf)            request the raw registers of one (edge, side)
//   A3R_OBS_UNPACK(code, ed, x, w)     raw registers -> points x[PXT][3], weights w[PXT]
    __shared__ float red[2][EB][16][16];
#ifdef A3R_ALIGN_STAMPS
    unsigned long long stamp[6] = {0, 0, 0, 0, 0, 0};
#endif
    A3R_STAMP(0);
    // images are dispatched longest first (order[] sorts them by their number of incident edge sides): the last round of
    // workgroups is then made of the short ones.  A dispatch slot's row of the table is {image, first and last incidence slot, the
    // first two (edge, side) codes}: ONE scalar load after which the first two edge sides are requested, before anything else --
    // the prologue used to be a chain of five dependent memory round trips (order -> inc_ptr -> inc -> LDS -> edge data) during
    // which the workgroup streamed nothing (15 % of its lifetime by s_memtime stamps, tools/align_stamps.py)
    const int* tb = order + blockIdx.y * 8;
    const int n = tb[0], kbeg = tb[1], kend = tb[2];
    const bool depth_frozen = (tb[6] & FREEZE_DEPTH) != 0;          // workgroup-uniform: the image is fixed per workgroup
    const int chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = d.P;
    constexpr int PSTEP = VEC ? 1 : TPB;
    const int pix0 = chunk * CHUNK + (VEC ? tid * PXT : tid);       // pixel i of this thread: pix0 + i * PSTEP
    bool valid[PXT];
#pragma unroll
    for (int i = 0; i < PXT; i++) valid[i] = pix0 + i * PSTEP < P;
    EdgeData<FORM> ea, eb;
    const float* ix = img_xf + n * 16;
    float R[9], T[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        R[r * 3 + 0] = ix[r * 4 + 0]; R[r * 3 + 1] = ix[r * 4 + 1]; R[r * 3 + 2] = ix[r * 4 + 2];
        T[r] = ix[r * 4 + 3];
    }
    const float f = ix[12], ppx = ix[13], ppy = ix[14], shift = ix[15];
    const int W = imw[n], area = imarea[n];
    const float invW = 1.f / (float)W, inv_f = 1.f / f;

    // forward of the image side: depth -> camera point -> world point (optimizer.py:190-200,244-251)
    auto pixel_forward = [&](int i, float rawv, float monov, float& dep, float& ddp, float& gxm, float& gym, float* rel) {
        const int p = pix0 + i * PSTEP;
        float gx = 0.f, gy = 0.f;
        if (p < area) {
            int y = (int)((float)p * invW);          // p < 2^24: exact up to +-1, fixed below
            int x = p - y * W;
            if (x < 0) { y--; x += W; }
            if (x >= W) { y++; x -= W; }
            gx = (float)x; gy = (float)y;
        }
        if (MONO) {
            const float es = expf(rawv);
            dep = monov * es + shift;
            ddp = monov * es;
        } else {
            dep = expf(rawv);
            ddp = dep;
        }
        gxm = gx - ppx; gym = gy - ppy;
        rel[0] = dep * gxm * inv_f;  // optimizer.py:251: depth * (pixel_grid - pp) / focal  (1/f: one IEEE divide per thread)
        rel[1] = dep * gym * inv_f;
        rel[2] = dep;
    };

    float raw[PXT], monov[PXT], proj[PXT][3], gp[PXT][3];
    if (VEC) {
        f32x4 r4 = {0.f, 0.f, 0.f, 0.f}, m4 = {0.f, 0.f, 0.f, 0.f};
        if (valid[0]) {
            r4 = *reinterpret_cast<const f32x4*>(d.depth + (size_t)n * P + pix0);
            if (MONO) m4 = *reinterpret_cast<const f32x4*>(d.mono + (size_t)n * P + pix0);
        }
        // the first two edge sides are requested right behind the depth: the memory counter retires in order, so the forward
        // arithmetic below waits for the depth alone and runs while the edge data is still on its way
        if (kbeg < kend) A3R_OBS_LOAD(tb[3], ea);
        if (kbeg + 1 < kend) A3R_OBS_LOAD(tb[4], eb);
        raw[0] = r4.x; raw[1] = r4.y; raw[2] = r4.z; raw[3] = r4.w;
        monov[0] = m4.x; monov[1] = m4.y; monov[2] = m4.z; monov[3] = m4.w;
    } else {
#pragma unroll
        for (int i = 0; i < PXT; i++) {
            const size_t off = (size_t)n * P + (valid[i] ? pix0 + i * PSTEP : 0);
            raw[i] = valid[i] ? d.depth[off] : 0.f;
            monov[i] = (MONO && valid[i]) ? d.mono[off] : 0.f;
        }
        if (kbeg < kend) A3R_OBS_LOAD(tb[3], ea);
        if (kbeg + 1 < kend) A3R_OBS_LOAD(tb[4], eb);
    }
#pragma unroll
    for (int i = 0; i < PXT; i++) {
        float dep, ddp, gxm, gym, rel[3];
        pixel_forward(i, raw[i], monov[i], dep, ddp, gxm, gym, rel);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            proj[i][r] = R[r * 3] * rel[0] + R[r * 3 + 1] * rel[1] + R[r * 3 + 2] * rel[2] + T[r];
            gp[i][r] = 0.f;
        }
    }
    if (MODE != 0 && d.flow_on) {
        // ego-flow term (align_flow_kernel): its gradient w.r.t. this pixel's world point, scaled by weight / sum(mask)
        const float c0 = d.flow_state[0], c1 = d.flow_state[1];
        const size_t NP3 = (size_t)d.N * P * 3;
#pragma unroll
        for (int i = 0; i < PXT; i++) {
            if (!valid[i]) continue;
            const float* gf = d.gflow + ((size_t)n * P + pix0 + i * PSTEP) * 3;
#pragma unroll
            for (int r = 0; r < 3; r++) gp[i][r] = c0 * gf[r] + c1 * gf[NP3 + r];
        }
    }

    // one (edge, side): residuals, loss, gradient w.r.t. the world point, per-edge sums (12 + loss)
    auto consume = [&](int code, const EdgeData<FORM>& ed, int buf, int kb) {
        float ex[PXT][3], ew[PXT];
        A3R_OBS_UNPACK(code, ed, ex, ew);
        const int e = code >> 1, side = code & 1;
        const float* M = edge_xf + e * 16;
        const float m00 = M[0], m01 = M[1], m02 = M[2], m03 = M[3];
        const float m10 = M[4], m11 = M[5], m12 = M[6], m13 = M[7];
        const float m20 = M[8], m21 = M[9], m22 = M[10], m23 = M[11];
        const float inva = side ? d.inv_area_j : d.inv_area_i;
        float acc[13];
#pragma unroll
        for (int j = 0; j < 13; j++) acc[j] = 0.f;
#pragma unroll
        for (int i = 0; i < PXT; i++) {
            const float x0 = ex[i][0], x1 = ex[i][1], x2 = ex[i][2], w = valid[i] ? ew[i] : 0.f;
            const float r0 = proj[i][0] - (m00 * x0 + m01 * x1 + m02 * x2 + m03);
            const float r1 = proj[i][1] - (m10 * x0 + m11 * x1 + m12 * x2 + m13);
            const float r2 = proj[i][2] - (m20 * x0 + m21 * x1 + m22 * x2 + m23);
            const float sq = r0 * r0 + r1 * r1 + r2 * r2;
            float cf;
            if (L2) {
                acc[12] += sq * w * inva;
                cf = 2.f * w * inva;
            } else {
                // v_rsq_f32 (1 ulp) instead of an IEEE sqrt + an IEEE divide: this loop is VALU-bound (PMC:
                // 68 % VALU-active at 4 TB/s), and the two expansions were a quarter of its instructions
                const float inv = sq > 0.f ? __builtin_amdgcn_rsqf(sq) : 0.f;
                const float wa = w * inva;
                acc[12] += sq * inv * wa;
                cf = wa * inv;
            }
            if (MODE != 0) {
                const float g0 = cf * r0, g1 = cf * r1, g2 = cf * r2;
                gp[i][0] += g0; gp[i][1] += g1; gp[i][2] += g2;
                acc[0] += g0 * x0; acc[1] += g0 * x1; acc[2] += g0 * x2;
                acc[3] += g1 * x0; acc[4] += g1 * x1; acc[5] += g1 * x2;
                acc[6] += g2 * x0; acc[7] += g2 * x1; acc[8] += g2 * x2;
                acc[9] += g0; acc[10] += g1; acc[11] += g2;
            }
        }
        if (MODE == 0) {
            const float s = dpp_row_sum16(acc[12]);
            if ((lane & 15) == 0) red[buf][kb][wave * 4 + (lane >> 4)][12] = s;
        } else {
            // the 13 sums of a 16-lane row by a reduce-scatter (common.h): 29 VALU operations and ONE 16-byte LDS store per quad
            // instead of 13 four-step butterflies with a masked 4-byte store each -- this loop is bound by instruction issue
            // (tools/align_stream_lab.hip: its access pattern alone streams at 6.3 TB/s), and the butterflies, their DPP wait
            // states and the 13 exec-masked stores were a third of its instructions
            float v16[16], u[4];
#pragma unroll
            for (int j = 0; j < 13; j++) v16[j] = acc[j];
            v16[13] = v16[14] = v16[15] = 0.f;
            row_reduce_scatter16<13>(v16, u);
            if ((lane & 3) == 0) *reinterpret_cast<f32x4*>(&red[buf][kb][wave * 4 + (lane >> 4)][lane & 12]) = f32x4{u[0], u[1], u[2], u[3]};
        }
    };

    // The incidence codes are read with SCALAR loads (a uniform index into a noalias table: s_load, counted on lgkmcnt): a vector
    // load here would need s_waitcnt vmcnt(0) before its value could form the next address and would drain the edge data in flight.
    // (Rounds 1-2 copied the image's codes to LDS first, which cost the prologue a vector load, an LDS pass and a barrier.)
    auto code_at = [&](int k) { return inc[__builtin_amdgcn_readfirstlane(k)]; };
    int buf = 0;
    A3R_STAMP(1);
    // one flat loop, two edge sides per trip, each register buffer re-requested right after it has been consumed (one edge side
    // in flight behind the one being worked on); the LDS batch of EB slots is flushed inside
    int kb = 0, k0 = kbeg;
#pragma unroll 1
    for (int k = kbeg; k < kend; k += 2) {
        const bool has1 = k + 1 < kend;
        consume(code_at(k), ea, buf, kb);
#ifdef A3R_ALIGN_STAMPS
        if (k == kbeg) { asm volatile("" :: "v"(gp[0][0])); A3R_STAMP(2); }
#endif
        if (k + 2 < kend) A3R_OBS_LOAD(code_at(k + 2), ea);
        if (has1) {
            consume(code_at(k + 1), eb, buf, kb + 1);
            if (k + 3 < kend) A3R_OBS_LOAD(code_at(k + 3), eb);
        }
        kb += 2;
        if (kb == EB || k + 2 >= kend) {
            __syncthreads();
            if (tid < EB * 4) {
                // one 16-byte quarter of a slot's row per thread, rows r added in order (the row is handed to the image's last workgroup)
                const int sb = tid >> 2, q = tid & 3, ks = k0 + sb;
                if (ks < kend) {
                    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int r = 0; r < 16; r++) s4 += *reinterpret_cast<const f32x4*>(&red[buf][sb][r][4 * q]);
                    store16_wt(d.partE, (unsigned)(((size_t)ks * d.nchunks + chunk) * 64 + 16 * q), s4);
                }
            }
            buf ^= 1; kb = 0; k0 += EB;
        }
    }
    A3R_STAMP(3);
    if (MODE != 0) {
    // the Adam moments of this thread's pixels are requested now: their latency runs under the per-image sums below
    f32x4 m4 = {0.f, 0.f, 0.f, 0.f}, v4 = {0.f, 0.f, 0.f, 0.f};
    if (VEC && MODE == 2 && valid[0] && !depth_frozen) {
        const size_t off = (size_t)n * P + pix0;
        m4 = *reinterpret_cast<const f32x4*>(d.adam_depth + off);
        v4 = *reinterpret_cast<const f32x4*>(d.adam_depth + (size_t)d.N * P + off);
    }

    // per-image sums and the per-pixel parameter (forward quantities are recomputed: cheaper than keeping them live)
    float accN[16], gout[PXT];
#pragma unroll
    for (int j = 0; j < 16; j++) accN[j] = 0.f;
#pragma unroll
    for (int i = 0; i < PXT; i++) {
        float dep, ddp, gxm, gym, rel[3];
        pixel_forward(i, raw[i], monov[i], dep, ddp, gxm, gym, rel);
        const float h0 = R[0] * gp[i][0] + R[3] * gp[i][1] + R[6] * gp[i][2];
        const float h1 = R[1] * gp[i][0] + R[4] * gp[i][1] + R[7] * gp[i][2];
        const float h2 = R[2] * gp[i][0] + R[5] * gp[i][1] + R[8] * gp[i][2];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            accN[r * 3 + 0] += gp[i][r] * rel[0];
            accN[r * 3 + 1] += gp[i][r] * rel[1];
            accN[r * 3 + 2] += gp[i][r] * rel[2];
            accN[9 + r] += gp[i][r];
        }
        const float gd = h0 * gxm * inv_f + h1 * gym * inv_f + h2;
        accN[12] += -(h0 * rel[0] + h1 * rel[1]) / d.focal_break;
        accN[13] += -h0 * dep * inv_f * 10.f;
        accN[14] += -h1 * dep * inv_f * 10.f;
        accN[15] += gd;
        gout[i] = gd * ddp;
    }
    if (MODE != 0 && d.gprior) {      // depth prior (align_depth_prior_kernel): already w.r.t. the log-depth parameter
#pragma unroll
        for (int i = 0; i < PXT; i++)
            if (valid[i]) gout[i] += d.gprior[(size_t)n * P + pix0 + i * PSTEP];
    }
    const size_t NP = (size_t)d.N * P;
    if (VEC) {
        if (valid[0]) {
            const size_t off = (size_t)n * P + pix0;
            if (MODE == 1) {
                f32x4 g4 = {gout[0], gout[1], gout[2], gout[3]};
                if (depth_frozen) g4 = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(g_depth + off) = g4;
            } else if (!depth_frozen) {       // a frozen depth map and its Adam moments are not touched
                float pm[4] = {m4.x, m4.y, m4.z, m4.w}, pv[4] = {v4.x, v4.y, v4.z, v4.w}, pp[4];
#pragma unroll
                for (int i = 0; i < PXT; i++) { pp[i] = raw[i]; adam_update(pp[i], gout[i], pm[i], pv[i], ad); }
                f32x4 o0 = {pp[0], pp[1], pp[2], pp[3]}, o1 = {pm[0], pm[1], pm[2], pm[3]}, o2 = {pv[0], pv[1], pv[2], pv[3]};
                *reinterpret_cast<f32x4*>(d.depth + off) = o0;
                *reinterpret_cast<f32x4*>(d.adam_depth + off) = o1;
                *reinterpret_cast<f32x4*>(d.adam_depth + NP + off) = o2;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < PXT; i++) {
            if (!valid[i]) continue;
            const size_t off = (size_t)n * P + pix0 + i * PSTEP;
            if (MODE == 1) {
                g_depth[off] = depth_frozen ? 0.f : gout[i];
            } else if (!depth_frozen) {
                float m = d.adam_depth[off], v = d.adam_depth[NP + off], pv = raw[i];
                adam_update(pv, gout[i], m, v, ad);
                d.depth[off] = pv; d.adam_depth[off] = m; d.adam_depth[NP + off] = v;
            }
        }
    }
    A3R_STAMP(4);
    __syncthreads();   // red[] may still be read by the last batch
    {
        float u[4];
        row_reduce_scatter16<16>(accN, u);
        if ((lane & 3) == 0) *reinterpret_cast<f32x4*>(&red[0][0][wave * 4 + (lane >> 4)][lane & 12]) = f32x4{u[0], u[1], u[2], u[3]};
    }
    __syncthreads();
    if (tid < 4) {
        f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; r++) s4 += *reinterpret_cast<const f32x4*>(&red[0][0][r][4 * tid]);
        store16_wt(d.partN, (unsigned)(((size_t)n * d.nchunks + chunk) * 64 + 16 * tid), s4);
    }
    }   // MODE != 0
#ifdef A3R_ALIGN_STAMPS
    A3R_STAMP(5);
    if (tid == 0 && MODE == 2) {
        unsigned long long* o = g_align_stamps + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) % 8192 * 8;
        for (int i = 0; i < 6; i++) o[i] = stamp[i];
        o[6] = (unsigned long long)(kend - kbeg);
        o[7] = ((unsigned long long)n << 32) | (unsigned)chunk;
    }
#endif
    if (!d.fused_tail) return;

    // ---- tail of the iteration inside this launch (no finalize launches): last-block-done tickets, two levels.
    // Level 1, per image: the workgroup that completes image n adds the chunk partials of the image's incidence slots and of the
    // image itself in a fixed order (one wave per row set: the order does not depend on who runs it -> bitwise reproducible).
    __syncthreads();                                   // red[] is free again
    int* flag = reinterpret_cast<int*>(&red[0][0][0][0]);
    if (!arrive_last(d.tick + n, gridDim.x, flag)) return;
    for (int k = kbeg + wave; k < kend; k += TPB / 64) {
        const f32x4 t = wave_sum_rows(d.partE + (size_t)k * d.nchunks * 16, d.nchunks, lane);
        if (lane < 4) store16_wt(d.sumE, (unsigned)(k * 64 + 16 * lane), t);
    }
    if (MODE != 0 && wave == 0) {
        const f32x4 t = wave_sum_rows(d.partN + (size_t)n * d.nchunks * 16, d.nchunks, lane);
        if (lane < 4) store16_wt(d.sumN, (unsigned)(n * 64 + 16 * lane), t);
    }
    // Level 2: the workgroup that completes the last image runs the chain rules of all edges and images, then the single-block
    // finalisation (scale coupling, loss, Adam on the small parameters, next iteration's transforms).
    if (!arrive_last(d.tick + d.N, d.N, flag)) return;
    for (int e = tid; e < d.E; e += TPB) {
        const float* s0 = d.sumE + d.slot_of[e * 2 + 0] * 16;
        const float* s1 = d.sumE + d.slot_of[e * 2 + 1] * 16;
        double s[13];
#pragma unroll
        for (int j = 0; j < 13; j++) s[j] = (double)s0[j] + (double)s1[j];
        edge_chain(d, e, s, MODE == 0);
    }
    for (int m = tid; m < d.N; m += TPB) {
        double s[16];
#pragma unroll
        for (int j = 0; j < 16; j++) s[j] = (double)d.sumN[m * 16 + j];
        image_chain(d, m, s);
    }
    for (int i = tid; i <= d.N; i += TPB)              // counters back to zero for the next launch (write-through stores)
        __hip_atomic_store(d.tick + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();                                   // the chain-rule results are visible to the whole workgroup
    float* sh = &red[0][0][0][0];
    double (*shd)[4] = reinterpret_cast<double (*)[4]>(&red[1][0][0][0]);
    finalize_b_body<MODE>(d, ad, tout, sh, shd);
