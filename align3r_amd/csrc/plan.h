// Host-side core of the two launch plans (model.hip: the pair network, raft.hip: the flow network).  Held once here: the weight
// table, the workspace arena, the operand forms and their sizes, the packed twins of the weights, the re-targeting of a plan's
// epilogue requests to a form, and the per-form dispatch of the matrix ops -- the only code that names the _bf3 / _fh2 entry points
// of linear, grouped linear, 3x3 conv, split and 2x up-sample.  What stays with each network: its plan (allocation, site and launch
// order) and its range policy, i.e. which scale an fh2 operand carries and which statistics word an fh2 output reports to.
#pragma once
#include "common.h"
#include <cmath>
#include <map>
#include <string>
#include <vector>

namespace a3r {

// ---- weights as the caller registered them: name -> (device pointer, shape)
struct WeightTable {
    struct Ref { const float* p = nullptr; std::vector<int64_t> shape; };
    std::map<std::string, Ref> w;
    int set(const char* who, const char* name, const float* ptr, int ndim, const int64_t* shape) {
        A3R_CHECK_ARG(name && ptr && ndim >= 1 && ndim <= 4 && shape, "%s: bad argument", who);
        A3R_CHECK_ARG((reinterpret_cast<uintptr_t>(ptr) & 15) == 0, "%s: %s is not 16-byte aligned", who, name);
        Ref& r = w[name];
        r.p = ptr;
        r.shape.assign(shape, shape + ndim);
        return A3R_OK;
    }
    const Ref* find(const std::string& name) const {
        auto it = w.find(name);
        return it == w.end() ? nullptr : &it->second;
    }
    int need(const std::string& name, const std::vector<int64_t>& shape, const char* who, const float** out) const {
        const Ref* r = find(name);
        if (!r) {
            set_error("%s: missing weight '%s'", who, name.c_str());
            return A3R_ESTATE;
        }
        if (r->shape != shape) {
            std::string got, want;
            for (auto d : r->shape) got += std::to_string(d) + ",";
            for (auto d : shape) want += std::to_string(d) + ",";
            set_error("%s: weight '%s' has shape [%s] but [%s] is required", who, name.c_str(), got.c_str(), want.c_str());
            return A3R_EINVAL;
        }
        *out = r->p;
        return A3R_OK;
    }
};

// ---- bump allocator over the caller's workspace.  dry: the sizing pass (null pointers, only `peak` matters).  A launch pass that
// asks for more than the workspace holds -- the two passes disagree, an internal bug -- gets the base pointer and is stopped by skip()
struct Arena {
    char* base; size_t off, cap; bool dry; size_t peak; bool overflow = false;
    float* alloc(size_t nfloat) {
        size_t o = off;
        off = align_up(off + nfloat * 4, 256);
        if (off > peak) peak = off;
        if (!dry && off > cap) { overflow = true; return reinterpret_cast<float*>(base); }
        return dry ? nullptr : reinterpret_cast<float*>(base + o);
    }
    // true when the plan must not launch: sizing pass, an earlier error (rc), or an overflow (then reported through rc)
    bool skip(int& rc, const char* who) const {
        if (overflow && !rc) {
            set_error("%s: internal workspace plan overflow (sizing pass and launch pass disagree)", who);
            rc = A3R_ESTATE;
        }
        return dry || rc != A3R_OK;
    }
};
// a stage's scratch: what is allocated inside the scope is released, back to the mark, when the scope ends (`peak` keeps counting
// it; what the stage enqueued still runs first: stream order)
struct ArenaScope {
    Arena& ar;
    const size_t mark;
    explicit ArenaScope(Arena& a) : ar(a), mark(a.off) {}
    ~ArenaScope() { ar.off = mark; }
    ArenaScope(const ArenaScope&) = delete;
};

// ---- the form a matrix operand [rows, K] is stored in: plain fp32; three bf16 planes (bf3.h, 6 K bytes per row); two fp16 planes of
// scale * x (fh2.h, 4 K bytes per row: exactly the fp32 matrix's)
enum class Form { F32, BF3, FH2 };
inline size_t form_floats(Form f, size_t rows, size_t K) { return f == Form::BF3 ? rows * K * 3 / 2 : rows * K; }

// ---- packed twins of the weights: the bf3 image and / or the fh2 image with the power-of-two scale it was stored with
struct Twin { const void* bf3 = nullptr; const void* fh2 = nullptr; float scale = 1.f; };
template <class Key> struct TwinTable {
    std::map<Key, Twin> t;
    const Twin* get(const Key& key, Form f, const char* who, int& rc) const {
        auto it = t.find(key);
        if (it != t.end() && (f == Form::BF3 ? it->second.bf3 : it->second.fh2)) return &it->second;
        if (!rc) {
            set_error("%s: a weight was not packed in %s form", who, f == Form::BF3 ? "bf3" : "fh2");
            rc = A3R_ESTATE;
        }
        return nullptr;
    }
    // image of the [N, K] fp32 weight `src` in form f at dst.  BF3: the row-pair weight layout.  FH2: scale = the power of two that
    // puts max|w| into [2^12, 2^13), from one small reduction into the device word `scratch` and its read-back
    int pack(const Key& key, Form f, const float* src, void* dst, int N, int K, float* scratch, const char* who, const char* name, void* stream) {
        if (f == Form::BF3) {
            if (int rc = a3r_split_bf3_w(src, K, dst, N, K, stream)) return rc;
            t[key].bf3 = dst;
            return A3R_OK;
        }
        if (int rc = a3r_absmax(src, (long)N * K, scratch, stream)) return rc;
        float amax = 0.f;
        A3R_HIP(hipMemcpyAsync(&amax, scratch, 4, hipMemcpyDeviceToHost, as_stream(stream)));
        A3R_HIP(hipStreamSynchronize(as_stream(stream)));
        A3R_CHECK_ARG(std::isfinite(amax), "%s: weight '%s' contains non-finite values", who, name);
        const float scale = a3r_fh2_weight_scale(amax);
        if (int rc = a3r_split_fh2(src, K, dst, N, K, scale, nullptr, stream)) return rc;
        Twin& tw = t[key];
        tw.fh2 = dst; tw.scale = scale;
        return A3R_OK;
    }
};

// ---- what a plan asks of a matrix op beyond its fp32 result, in words that do not name a form.  out_op: write y in the operand form
// of its consumer INSTEAD of fp32; aux_op: ALSO write the result (through a ReLU if aux_relu) in that form there
struct OpEpi : a3r_epilogue { int out_op = 0; void* aux_op = nullptr; };

// the epilogue of the launch in form f.  F32 has no operand-form outputs (the requests are dropped); under FH2 `range(e)` fills the
// range fields (x_scale, out_scale, out_absmax) by the network's policy
template <class Range> a3r_epilogue retarget(const OpEpi& r, Form f, Range&& range) {
    a3r_epilogue e = r;
    if (f == Form::BF3) { e.out_bf3 = r.out_op; e.aux_bf3 = r.aux_op; }
    if (f == Form::FH2) { e.out_fh2 = r.out_op; e.aux_fh2 = r.aux_op; range(e); }
    return e;
}

// ---- dispatch on the operand form.  w: the fp32 weight (F32 only); tw: its twin (BF3 / FH2); scale, stat: the power of two an fh2
// output is stored with and the device word that receives its max |stored value| (FH2 only)
inline int op_linear(Form f, const float* x, int lda, const float* w, const Twin* tw, float* y, int ldc, int M, int N, int K,
                     const a3r_epilogue& e, void* stream) {
    if (f == Form::F32) return a3r_linear(x, lda, w, y, ldc, M, N, K, &e, stream);
    if (f == Form::BF3) return a3r_linear_bf3(x, tw->bf3, y, ldc, M, N, K, &e, stream);
    return a3r_linear_fh2(x, tw->fh2, tw->scale, y, ldc, M, N, K, &e, stream);
}
// two same-shape problems in one launch; one output site for both (out_scale, out_stat), each side's own operand scale
struct GroupSide { const float* x; const float* w; const Twin* tw; float* y; const float* bias; const float* resid; float x_scale; };
inline int op_linear_grouped(Form f, const GroupSide (&s)[2], float out_scale, unsigned* out_stat, int lda, int ldc, int M, int N, int K,
                             const a3r_epilogue& e, void* stream) {
    if (f == Form::F32) {
        a3r_group_ptrs g[2] = {{s[0].x, s[0].w, s[0].y, s[0].bias, s[0].resid, nullptr}, {s[1].x, s[1].w, s[1].y, s[1].bias, s[1].resid, nullptr}};
        return a3r_linear_grouped(g, 2, lda, ldc, M, N, K, &e, stream);
    }
    if (f == Form::BF3) {
        a3r_group_ptrs_bf3 g[2] = {{s[0].x, s[0].tw->bf3, s[0].y, s[0].bias, s[0].resid, nullptr},
                                   {s[1].x, s[1].tw->bf3, s[1].y, s[1].bias, s[1].resid, nullptr}};
        return a3r_linear_bf3_grouped(g, 2, ldc, M, N, K, &e, stream);
    }
    a3r_group_ptrs_fh2 g[2] = {{s[0].x, s[0].tw->fh2, s[0].y, s[0].bias, s[0].resid, nullptr, s[0].tw->scale, s[0].x_scale, out_scale, out_stat},
                               {s[1].x, s[1].tw->fh2, s[1].y, s[1].bias, s[1].resid, nullptr, s[1].tw->scale, s[1].x_scale, out_scale, out_stat}};
    return a3r_linear_fh2_grouped(g, 2, ldc, M, N, K, &e, stream);
}
inline int op_conv3x3(Form f, const float* x, const float* wp, const Twin* tw, float* y, int B, int H, int W, int Cin, int Cout, int stride,
                      const a3r_epilogue& e, void* stream) {
    if (f == Form::F32) return a3r_conv3x3(x, wp, y, B, H, W, Cin, Cout, stride, &e, stream);
    if (f == Form::BF3) return a3r_conv3x3_bf3(x, tw->bf3, y, B, H, W, Cin, Cout, stride, &e, stream);
    return a3r_conv3x3_fh2(x, tw->fh2, tw->scale, y, B, H, W, Cin, Cout, stride, &e, stream);
}
// fp32 x [M, ldx] -> operand form y (not for F32).  row_pair (BF3 only): the row-pair layout of weights and pair-mode activations
inline int op_split(Form f, const float* x, int ldx, void* y, long M, int K, bool row_pair, float scale, unsigned* stat, void* stream) {
    if (f == Form::FH2) return a3r_split_fh2(x, ldx, y, M, K, scale, stat, stream);
    return row_pair ? a3r_split_bf3_w(x, ldx, y, M, K, stream) : a3r_split_bf3(x, ldx, y, M, K, stream);
}
inline int op_upsample2x(Form f, const float* x, float* y, int B, int H, int W, int C, int Hc, int Wc, float scale, unsigned* stat, void* stream) {
    if (f == Form::F32) return a3r_upsample2x(x, y, B, H, W, C, Hc, Wc, stream);
    if (f == Form::BF3) return a3r_upsample2x_bf3(x, y, B, H, W, C, Hc, Wc, stream);
    return a3r_upsample2x_fh2(x, y, B, H, W, C, Hc, Wc, scale, stat, stream);
}

}  // namespace a3r
