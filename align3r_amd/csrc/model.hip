// AsymmetricCroCo3DStereo.forward as a fixed launch plan over liba3r's kernels (host code only).
//
// Mirrors, step for step (paths inside the reference project):
//   forward / _encode_image_pairs / _encode_image   dust3r/model.py:241-257,151-174
//   _decoder (+ dec_blocks_pc / zero_convs branch)  dust3r/model.py:201-233
//   Block / DecoderBlock                             croco/models/blocks.py:114-191
//   DPTOutputAdapter_fix.forward                     dust3r/heads/dpt_head.py:34-66
//   postprocess                                      dust3r/heads/postprocess.py:10-58
// Data layout: tokens [rows, C] with rows = (side, batch, token): the first B*N rows belong to view 1,
// the next B*N rows to view 2 (this is the reference's torch.cat((img1, img2)) batch order), maps are
// channels-last.  All buffers live in the caller's workspace; nothing here allocates device memory, except the handle's key / map
// words for the duplicate search (find_distinct, about 140 KB).  The frames, depth priors and head products kept across calls live in
// storage the caller installs (a3r_model_set_frame_cache, a3r_model_set_frame_products, a3r_model_set_head_products).
#include "plan.h"
#include "dedup.h"
#include <algorithm>
#include <new>
#include <cstdlib>
#include <cstring>

namespace a3r {

struct BlockW {
    const float *n1w, *n1b, *qkvw, *qkvb, *projw, *projb, *n2w, *n2b, *fc1w, *fc1b, *fc2w, *fc2b;
    // decoder only
    const float *qw, *qb, *kvw, *kvb, *cprojw, *cprojb, *n3w, *n3b, *nyw, *nyb;
};

struct RcuW { const float *c1w, *c1b, *c2w, *c2b; };
struct FusionW { RcuW r1, r2; const float *ow, *ob; };
struct HeadW {
    const float *a0w, *a0b, *a0tw, *a0tb, *a1w, *a1b, *a1tw, *a1tb, *a2w, *a2b, *a3w, *a3b, *a3cw, *a3cb;
    const float* rn[4];
    FusionW ref[4];   // ref[0] = refinenet1 ... ref[3] = refinenet4
    const float *h0w, *h0b, *h2w, *h2b, *h4w, *h4b;
};

}  // namespace a3r
using namespace a3r;

struct a3r_model_s {
    a3r_model_config cfg;
    WeightTable w;
    bool finalized = false;
    std::vector<BlockW> enc, pc, dec1, dec2;
    HeadW head[2];
    const float *pe_w, *pe_b, *pepc_w, *pepc_b, *encn_w, *encn_b, *de_w, *de_b, *decn_w, *decn_b;
    std::vector<const float*> zc_w, zc_b;
    const float *rope_cos = nullptr, *rope_sin = nullptr;
    std::vector<float> host_cos, host_sin;
    std::map<std::string, std::pair<const float*, size_t>> taps;
    // arithmetic mode, decoded once in a3r_model_create from A3R_GEMM x A3R_CONV ("Arithmetic modes")
    Form gemm_form = Form::FH2;   // operands of the transformer GEMMs (nn.Linear inputs and weights) and of attention
    Form map_form = Form::FH2;    // DPT maps: operands of the 3x3 convs and of the fusion blocks' 1x1 out_conv
    int fh2_passes = 3;       // fh2 matrix passes per product: 3 = fp32-grade; A3R_GEMM=f16 -> 1 (plain fp16 operands, reduced precision)
    int products = 6;         // bf3 plane products per multiply: 6 = fp32-accurate; A3R_GEMM=bf3x3 -> 3, A3R_GEMM=bf16 -> 1 (reduced precision)
    // fp32 weight pointer (nn.Linear weight or packed conv weight) -> its twin in `packed`, in the form of the GEMMs / maps that read it
    TwinTable<const float*> twins;
    static constexpr int MAX_POS = 256;
    // fh2 range control (fh2.h, RANGE; a3r_model_range_check): one power-of-two scale per fh2-producing site of the launch plan, kept
    // per plan phase (forward / encode / decode walk different plans), and the device words the sites record max |stored value| in
    static constexpr int MAX_SITES = 1024;
    std::vector<float> site_scale[3];
    unsigned* stats = nullptr;       // [MAX_SITES], inside the packed buffer
    int last_phase = -1, last_sites = 0;
    // LayerNorm -> fh2 sites need no run-time statistics: |y| <= max|gamma| sqrt(D) + max|beta| whatever the input, so their scale is
    // fixed at finalize from the two weight vectors (gamma pointer -> scale); see ln_static_scale
    std::map<const float*, float> ln_scale;
    int tap_level = 0;               // a3r_model_set_tap_level: decoder level copied to the taps "level" / "pc0" (parity tests), 0 = none
    // duplicate inputs (dedup.h; a3r_model_set_dedup): 0 = every slot is encoded, 1 = the frame-only parts of the plan run once per
    // distinct image / pred_depth map of the batch, 2 = as 1 with a constant key (debugging: the verification alone decides)
    int dedup_mode = 1;
    // a3r_model_set_dedup_head: the DPT heads' level-0 branch runs once per distinct frame of a side (run_plan, HeadMerge)
    int dedup_head = 1;
    int dedup_head_fold = 1;         // A/B switch (A3R_DEDUP_HEAD_FOLD=0): 0 = the combine runs as a pass of its own after the 2x up-sample
    // a3r_model_set_dedup_decoder: decoder_embed, the zero-convs and block 0's frame-only half on distinct rows (decoder_stage)
    int dedup_decoder = 1;
    // what the planner decided for the last forward or decode call (dedup.h): the counts that a3r_model_last_dedup, _sides,
    // _entries, a3r_model_last_frame_cache, _frame_products and _head_products report
    CallPlan last;
    // the handle's own small buffers (the only device memory it allocates, at its first merging call): keys, representatives and
    // flag, the uploaded lists (CallLists), and the pinned host words of the one read-back and the one upload of a call
    void* dd_dev = nullptr;
    int32_t* dd_host = nullptr;
    // A storage the caller installs for what is kept across calls: device memory, 256-byte aligned, the caller's
    struct Storage {
        void* buf = nullptr;
        size_t bytes = 0;
        int set(void* b, size_t n, const char* who) {      // (null or no bytes: removes it)
            buf = nullptr;
            bytes = 0;
            if (!b || !n) return A3R_OK;
            A3R_CHECK_ARG((reinterpret_cast<uintptr_t>(b) & 255) == 0, "%s: storage must be 256-byte aligned", who);
            buf = b;
            bytes = n;
            return A3R_OK;
        }
    };
    // frames kept across calls (a3r_model_set_frame_cache): the caller's storage, the host table of its entries (dedup.h) and the
    // resolution they were stored at
    Storage fc;
    FrameCacheTable fc_table;
    int fc_H = 0, fc_W = 0;
    // frame products kept across calls (a3r_model_set_frame_products): the caller's second storage, which holds as many depth priors
    // with their zero-conv outputs as the frame cache holds frames, and the table of those entries
    Storage fp;
    FrameCacheTable pd_table;
    // head products kept across calls (a3r_model_set_head_products): the caller's third storage, indexed by the frame cache's
    // entries, one valid bit per (entry, side) (dedup.h)
    Storage hp;
    HeadBits hp_bits;
    // the frame cache's table emptied or resized: the head products' bits name its entries
    void reset_frames(int capacity) {
        fc_table.reset(capacity);
        hp_bits.flush();
    }
    // whatever was stored under other weights, scales, keys or after a failed call is forgotten
    void drop_stored() {
        fc_table.flush();
        pd_table.flush();
        hp_bits.flush();
    }
    ~a3r_model_s() {
        if (dd_dev) (void)hipFree(dd_dev);
        if (dd_host) (void)hipHostFree(dd_host);
    }
};

static int n_pc_blocks(const a3r_model_config& c) { return c.dec_depth / 2 - 2; }

extern "C" int a3r_model_create(const a3r_model_config* cfg, a3r_model_t* out) {
    A3R_CHECK_ARG(cfg && out, "a3r_model_create: null argument");
    A3R_CHECK_ARG(cfg->enc_embed_dim == cfg->enc_num_heads * 64 && cfg->dec_embed_dim == cfg->dec_num_heads * 64,
                  "a3r_model_create: head_dim must be 64 (enc %d/%d, dec %d/%d)", cfg->enc_embed_dim, cfg->enc_num_heads,
                  cfg->dec_embed_dim, cfg->dec_num_heads);
    A3R_CHECK_ARG(cfg->patch_size == 16, "a3r_model_create: patch_size must be 16");
    A3R_CHECK_ARG(cfg->dec_depth > 9, "a3r_model_create: dec_depth must be > 9 (dpt_head.py:101)");
    A3R_CHECK_ARG(cfg->enc_embed_dim % 32 == 0 && cfg->dec_embed_dim % 32 == 0 && cfg->feature_dim % 32 == 0 &&
                      cfg->last_dim % 32 == 0, "a3r_model_create: widths must be multiples of 32");
    for (int i = 0; i < 4; i++) A3R_CHECK_ARG(cfg->layer_dims[i] % 32 == 0, "a3r_model_create: layer_dims must be multiples of 32");
    a3r_model_s* m = new (std::nothrow) a3r_model_s();
    A3R_CHECK_ARG(m, "out of host memory");
    m->cfg = *cfg;
    // f32: the exact-fp32 MFMA kernels; bf3: GEMMs, attention and DPT maps on the exact three-plane bf16 form (6 products); bf3x3 /
    // bf16: the same kernels with 3 / 1 products (reduced precision); f16: the fh2 kernels with ONE pass per product (plain fp16
    // operands under the same range control: the fast 16-bit mode); anything else (unset, "fh2"): everything on the two-plane fp16
    // form, 3 passes.  Under fh2 GEMMs A3R_CONV=bf3 keeps the DPT maps on the three-plane bf16 kernels.
    struct Mode { const char* name; Form gemm; int products, passes; };
    static const Mode modes[] = {{"f32", Form::F32, 6, 3}, {"bf3", Form::BF3, 6, 3}, {"bf3x3", Form::BF3, 3, 3}, {"bf16", Form::BF3, 1, 3},
                                 {"f16", Form::FH2, 6, 1}};
    const char *gemm = getenv("A3R_GEMM"), *conv = getenv("A3R_CONV");
    for (const Mode& md : modes)
        if (gemm && !strcmp(gemm, md.name)) { m->gemm_form = md.gemm; m->products = md.products; m->fh2_passes = md.passes; }
    m->map_form = m->gemm_form == Form::FH2 && conv && !strcmp(conv, "bf3") ? Form::BF3 : m->gemm_form;
    if (const char* dd = getenv("A3R_DEDUP"))      // the default of new handles (a3r_model_set_dedup); anything but 0 / 2 leaves it on
        m->dedup_mode = !strcmp(dd, "0") ? 0 : !strcmp(dd, "2") ? 2 : 1;
    if (const char* dh = getenv("A3R_DEDUP_HEAD")) m->dedup_head = strcmp(dh, "0") != 0;      // (a3r_model_set_dedup_head)
    if (const char* df = getenv("A3R_DEDUP_HEAD_FOLD")) m->dedup_head_fold = strcmp(df, "0") != 0;
    if (const char* dc = getenv("A3R_DEDUP_DEC")) m->dedup_decoder = strcmp(dc, "0") != 0;    // (a3r_model_set_dedup_decoder)
    // sized here so that the host-side sizing pass (a3r_model_workspace_bytes) works before finalize
    m->enc.assign(cfg->enc_depth, BlockW());
    m->pc.assign(n_pc_blocks(*cfg), BlockW());
    m->dec1.assign(cfg->dec_depth, BlockW());
    m->dec2.assign(cfg->dec_depth, BlockW());
    m->zc_w.assign(n_pc_blocks(*cfg) + 1, nullptr);
    m->zc_b.assign(n_pc_blocks(*cfg) + 1, nullptr);
    *out = m;
    return A3R_OK;
}

extern "C" int a3r_model_destroy(a3r_model_t m) {
    delete m;
    return A3R_OK;
}

extern "C" int a3r_model_set_weight(a3r_model_t m, const char* name, const float* ptr, int ndim, const int64_t* shape) {
    A3R_CHECK_ARG(m, "a3r_model_set_weight: bad argument");
    if (int rc = m->w.set("a3r_model_set_weight", name, ptr, ndim, shape)) return rc;
    m->finalized = false;
    m->drop_stored();          // stored rows belong to the weights they were computed with
    return A3R_OK;
}

// ------------------------------------------------------------------------------------------- packing plan
namespace {
// CONV3X3 [Cout=a,Cin=b]; CONVT [Cin=a,Cout=b,s]; KV_CONCAT (D=a); ROPE tables; TWIN of the [a, b] weight `name` in Form s (an fh2
// twin has 256 bytes behind it: scratch of the max|w| reduction that fixes its scale); STATS: the range statistics words
enum class Pack { CONV3X3, CONVT, KV_CONCAT, ROPE, TWIN, STATS };
struct PackItem { std::string name; Pack kind; int a, b, s; size_t off; };

std::vector<PackItem> pack_plan(a3r_model_s* m, size_t* total) {
    const a3r_model_config& c = m->cfg;
    std::vector<PackItem> v;
    size_t off = 0;
    auto add = [&](const std::string& n, Pack kind, int a, int b, int s, size_t nfloat) {
        v.push_back({n, kind, a, b, s, off});
        off = align_up(off + nfloat * 4, 256);
    };
    const int F = c.feature_dim;
    for (int h = 1; h <= 2; h++) {
        const std::string p = "downstream_head" + std::to_string(h) + ".dpt.";
        for (int i = 0; i < 4; i++) add(p + "scratch.layer" + std::to_string(i + 1) + "_rn.weight", Pack::CONV3X3, F, c.layer_dims[i], 0, (size_t)F * c.layer_dims[i] * 9);
        for (int r = 1; r <= 4; r++)
            for (int u = 1; u <= 2; u++)
                for (int k = 1; k <= 2; k++)
                    add(p + "scratch.refinenet" + std::to_string(r) + ".resConfUnit" + std::to_string(u) + ".conv" + std::to_string(k) + ".weight", Pack::CONV3X3, F, F, 0, (size_t)F * F * 9);
        add(p + "head.0.weight", Pack::CONV3X3, F / 2, F, 0, (size_t)(F / 2) * F * 9);
        add(p + "head.2.weight", Pack::CONV3X3, c.last_dim, F / 2, 0, (size_t)c.last_dim * (F / 2) * 9);
        add(p + "act_postprocess.3.1.weight", Pack::CONV3X3, c.layer_dims[3], c.layer_dims[3], 0, (size_t)c.layer_dims[3] * c.layer_dims[3] * 9);
        add(p + "act_postprocess.0.1.weight", Pack::CONVT, c.layer_dims[0], c.layer_dims[0], 4, (size_t)c.layer_dims[0] * c.layer_dims[0] * 16);
        add(p + "act_postprocess.1.1.weight", Pack::CONVT, c.layer_dims[1], c.layer_dims[1], 2, (size_t)c.layer_dims[1] * c.layer_dims[1] * 4);
    }
    const int D = c.dec_embed_dim;
    for (int d = 0; d < 2; d++)
        for (int i = 0; i < c.dec_depth; i++) {
            const std::string p = std::string(d ? "dec_blocks2." : "dec_blocks.") + std::to_string(i) + ".cross_attn.";
            add(p + "kv", Pack::KV_CONCAT, D, 0, 0, (size_t)2 * D * D + 2 * D);
        }
    v.push_back({"rope", Pack::ROPE, 0, 0, 0, off});
    off = align_up(off + (size_t)2 * a3r_model_s::MAX_POS * 16 * 4, 256);
    v.push_back({"range_stats", Pack::STATS, 0, 0, 0, off});
    off = align_up(off + (size_t)a3r_model_s::MAX_SITES * 4, 256);
    if (m->gemm_form != Form::F32) {
        auto twin = [&](const std::string& n, int N, int K, Form f) {
            v.push_back({n, Pack::TWIN, N, K, (int)f, off});
            off = align_up(off + (f == Form::FH2 ? a3r_fh2_bytes(N, K) + 256 : a3r_bf3_w_bytes(N, K)), 256);
        };
        auto twin_lin = [&](const std::string& n, int N, int K) { twin(n, N, K, m->gemm_form); };
        auto block = [&](const std::string& p, int Dm, bool cross) {
            twin_lin(p + ".attn.qkv.weight", 3 * Dm, Dm); twin_lin(p + ".attn.proj.weight", Dm, Dm);
            twin_lin(p + ".mlp.fc1.weight", Dm * c.mlp_ratio, Dm); twin_lin(p + ".mlp.fc2.weight", Dm, Dm * c.mlp_ratio);
            if (cross) {
                twin_lin(p + ".cross_attn.projq.weight", Dm, Dm); twin_lin(p + ".cross_attn.kv", 2 * Dm, Dm);
                twin_lin(p + ".cross_attn.proj.weight", Dm, Dm);
            }
        };
        const int E = c.enc_embed_dim;
        for (int i = 0; i < c.enc_depth; i++) block("enc_blocks." + std::to_string(i), E, false);
        for (int i = 0; i < n_pc_blocks(c); i++) block("dec_blocks_pc." + std::to_string(i), D, false);
        for (int i = 0; i < c.dec_depth; i++) {
            block("dec_blocks." + std::to_string(i), D, true);
            block("dec_blocks2." + std::to_string(i), D, true);
        }
        twin_lin("patch_embed.proj.weight", E, 768);
        twin_lin("patch_embed_point_cloud.proj.weight", D, 768);
        twin_lin("decoder_embed.weight", D, E);
        for (int i = 0; i <= n_pc_blocks(c); i++) twin_lin("zero_convs." + std::to_string(i) + ".0.weight", D, D);
        if (m->gemm_form == Form::FH2)        // the 1x1 adapters of the DPT heads (act_postprocess.*.0): [layer_dim, D or E, 1, 1] = an nn.Linear weight
            for (int h = 1; h <= 2; h++) {
                const std::string p = "downstream_head" + std::to_string(h) + ".dpt.act_postprocess.";
                twin_lin(p + "0.0.weight", c.layer_dims[0], E);
                for (int i = 1; i < 4; i++) twin_lin(p + std::to_string(i) + ".0.weight", c.layer_dims[i], D);
            }
        // DPT heads: every packed 3x3 conv weight [Cout, 9 Cin] and the 1x1 out_conv of the fusion blocks
        std::vector<PackItem> convs;
        for (const PackItem& it : v)
            if (it.kind == Pack::CONV3X3) convs.push_back(it);
        for (const PackItem& it : convs) twin(it.name, it.a, 9 * it.b, m->map_form);
        for (int h = 1; h <= 2; h++)
            for (int r = 1; r <= 4; r++)
                twin("downstream_head" + std::to_string(h) + ".dpt.scratch.refinenet" + std::to_string(r) + ".out_conv.weight", F, F, m->map_form);
    }
    *total = off;
    return v;
}
}  // namespace

extern "C" size_t a3r_model_packed_bytes(a3r_model_t m) {
    if (!m) return 0;
    size_t total = 0;
    pack_plan(m, &total);
    return total;
}

#define NEED(name, out, ...)                                                                        \
    do {                                                                                            \
        if (int rc__ = m->w.need(name, {__VA_ARGS__}, "a3r_model_finalize", out)) return rc__; \
    } while (0)

static int bind_block(a3r_model_s* m, const std::string& p, int D, int hidden, bool cross, BlockW* b) {
    NEED(p + ".norm1.weight", &b->n1w, D); NEED(p + ".norm1.bias", &b->n1b, D);
    NEED(p + ".attn.qkv.weight", &b->qkvw, 3 * D, D); NEED(p + ".attn.qkv.bias", &b->qkvb, 3 * D);
    NEED(p + ".attn.proj.weight", &b->projw, D, D); NEED(p + ".attn.proj.bias", &b->projb, D);
    NEED(p + ".norm2.weight", &b->n2w, D); NEED(p + ".norm2.bias", &b->n2b, D);
    NEED(p + ".mlp.fc1.weight", &b->fc1w, hidden, D); NEED(p + ".mlp.fc1.bias", &b->fc1b, hidden);
    NEED(p + ".mlp.fc2.weight", &b->fc2w, D, hidden); NEED(p + ".mlp.fc2.bias", &b->fc2b, D);
    if (cross) {
        const float* t;
        NEED(p + ".cross_attn.projq.weight", &b->qw, D, D); NEED(p + ".cross_attn.projq.bias", &b->qb, D);
        NEED(p + ".cross_attn.projk.weight", &t, D, D); NEED(p + ".cross_attn.projk.bias", &t, D);
        NEED(p + ".cross_attn.projv.weight", &t, D, D); NEED(p + ".cross_attn.projv.bias", &t, D);
        NEED(p + ".cross_attn.proj.weight", &b->cprojw, D, D); NEED(p + ".cross_attn.proj.bias", &b->cprojb, D);
        NEED(p + ".norm3.weight", &b->n3w, D); NEED(p + ".norm3.bias", &b->n3b, D);
        NEED(p + ".norm_y.weight", &b->nyw, D); NEED(p + ".norm_y.bias", &b->nyb, D);
    }
    return A3R_OK;
}

// Scale of a LayerNorm -> fh2 output from its weights alone.  Hard bound: |y| <= g sqrt(D) + b (g = max|gamma|, b = max|beta|; the
// normalised row has unit variance, so no entry exceeds sqrt(D - 1)).  1 unless that bound could pass 2^15 (then the power of two that
// keeps it below) or the typical magnitude g + b is under 2^-3 (then raised until g + b reaches [2^-1, 1), never past the bound).
static float ln_static_scale(float g, float b, int D) {
    const double bound = (double)g * std::sqrt((double)D) + (double)b, typ = (double)g + (double)b;
    if (!(bound > 0.0)) return 1.f;
    int e;
    std::frexp(bound, &e);                         // bound = f 2^e, f in [0.5, 1)
    const int kmax = 15 - e;                       // 2^kmax * bound < 2^15
    int k = 0;
    if (typ < 0.125) {
        int et;
        std::frexp(typ > 0.0 ? typ : bound, &et);
        k = -et;                                   // 2^k * typ in [0.5, 1)
    }
    if (k > kmax) k = kmax;
    k = k < -40 ? -40 : k > 40 ? 40 : k;
    return std::ldexp(1.f, k);
}

using PackedPtrs = std::map<std::string, const float*>;

// the repacked weights of the plan (everything but the twins, which follow the binding: shapes are validated there) -> pk
static int repack_weights(a3r_model_s* m, const std::vector<PackItem>& plan, char* pk, void* stream, PackedPtrs& packed_ptr) {
    const a3r_model_config& c = m->cfg;
    const int D = c.dec_embed_dim;
    hipStream_t st = as_stream(stream);
    for (const PackItem& it : plan) {
        float* dst = reinterpret_cast<float*>(pk + it.off);
        if (it.kind == Pack::TWIN) continue;
        if (it.kind == Pack::STATS) {
            m->stats = reinterpret_cast<unsigned*>(dst);
            A3R_HIP(hipMemsetAsync(dst, 0, (size_t)a3r_model_s::MAX_SITES * 4, st));
            continue;
        }
        if (it.kind == Pack::CONV3X3) {
            const float* src;
            NEED(it.name, &src, it.a, it.b, 3, 3);
            if (int rc = a3r_pack_conv3x3(src, dst, it.a, it.b, stream)) return rc;
        } else if (it.kind == Pack::CONVT) {
            const float* src;
            NEED(it.name, &src, it.a, it.b, it.s, it.s);
            if (int rc = a3r_pack_convT(src, dst, it.a, it.b, it.s, stream)) return rc;
        } else if (it.kind == Pack::KV_CONCAT) {
            const std::string p = it.name.substr(0, it.name.size() - 2);   // strip "kv"
            const float *kw, *kb, *vw, *vb;
            NEED(p + "projk.weight", &kw, D, D); NEED(p + "projk.bias", &kb, D);
            NEED(p + "projv.weight", &vw, D, D); NEED(p + "projv.bias", &vb, D);
            const size_t DD = (size_t)D * D * 4;
            A3R_HIP(hipMemcpyAsync(dst, kw, DD, hipMemcpyDeviceToDevice, st));
            A3R_HIP(hipMemcpyAsync(dst + (size_t)D * D, vw, DD, hipMemcpyDeviceToDevice, st));
            A3R_HIP(hipMemcpyAsync(dst + (size_t)2 * D * D, kb, D * 4, hipMemcpyDeviceToDevice, st));
            A3R_HIP(hipMemcpyAsync(dst + (size_t)2 * D * D + D, vb, D * 4, hipMemcpyDeviceToDevice, st));
        } else {
            m->host_cos.resize(a3r_model_s::MAX_POS * 16);
            m->host_sin.resize(a3r_model_s::MAX_POS * 16);
            a3r_rope_table_host(m->host_cos.data(), m->host_sin.data(), a3r_model_s::MAX_POS, c.rope_base);
            A3R_HIP(hipMemcpyAsync(dst, m->host_cos.data(), m->host_cos.size() * 4, hipMemcpyHostToDevice, st));
            A3R_HIP(hipMemcpyAsync(dst + a3r_model_s::MAX_POS * 16, m->host_sin.data(), m->host_sin.size() * 4, hipMemcpyHostToDevice, st));
            m->rope_cos = dst;
            m->rope_sin = dst + a3r_model_s::MAX_POS * 16;
        }
        packed_ptr[it.name] = dst;
    }
    return A3R_OK;
}

static int bind_head(a3r_model_s* m, int h, PackedPtrs& packed_ptr) {
    const a3r_model_config& c = m->cfg;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim, F = c.feature_dim, L = c.last_dim;
    HeadW& H = m->head[h];
    const std::string p = "downstream_head" + std::to_string(h + 1) + ".dpt.";
    const int* ld = c.layer_dims;
    NEED(p + "act_postprocess.0.0.weight", &H.a0w, ld[0], E, 1, 1); NEED(p + "act_postprocess.0.0.bias", &H.a0b, ld[0]);
    NEED(p + "act_postprocess.0.1.bias", &H.a0tb, ld[0]);
    NEED(p + "act_postprocess.1.0.weight", &H.a1w, ld[1], D, 1, 1); NEED(p + "act_postprocess.1.0.bias", &H.a1b, ld[1]);
    NEED(p + "act_postprocess.1.1.bias", &H.a1tb, ld[1]);
    NEED(p + "act_postprocess.2.0.weight", &H.a2w, ld[2], D, 1, 1); NEED(p + "act_postprocess.2.0.bias", &H.a2b, ld[2]);
    NEED(p + "act_postprocess.3.0.weight", &H.a3w, ld[3], D, 1, 1); NEED(p + "act_postprocess.3.0.bias", &H.a3b, ld[3]);
    NEED(p + "act_postprocess.3.1.bias", &H.a3cb, ld[3]);
    H.a0tw = packed_ptr[p + "act_postprocess.0.1.weight"];
    H.a1tw = packed_ptr[p + "act_postprocess.1.1.weight"];
    H.a3cw = packed_ptr[p + "act_postprocess.3.1.weight"];
    for (int i = 0; i < 4; i++) H.rn[i] = packed_ptr[p + "scratch.layer" + std::to_string(i + 1) + "_rn.weight"];
    for (int r = 0; r < 4; r++) {
        const std::string q = p + "scratch.refinenet" + std::to_string(r + 1) + ".";
        NEED(q + "out_conv.weight", &H.ref[r].ow, F, F, 1, 1); NEED(q + "out_conv.bias", &H.ref[r].ob, F);
        RcuW* rr[2] = {&H.ref[r].r1, &H.ref[r].r2};
        for (int u = 0; u < 2; u++) {
            const std::string qq = q + "resConfUnit" + std::to_string(u + 1) + ".";
            rr[u]->c1w = packed_ptr[qq + "conv1.weight"]; rr[u]->c2w = packed_ptr[qq + "conv2.weight"];
            NEED(qq + "conv1.bias", &rr[u]->c1b, F); NEED(qq + "conv2.bias", &rr[u]->c2b, F);
        }
    }
    H.h0w = packed_ptr[p + "head.0.weight"]; NEED(p + "head.0.bias", &H.h0b, F / 2);
    H.h2w = packed_ptr[p + "head.2.weight"]; NEED(p + "head.2.bias", &H.h2b, L);
    NEED(p + "head.4.weight", &H.h4w, 4, L, 1, 1); NEED(p + "head.4.bias", &H.h4b, 4);
    return A3R_OK;
}

// static scales of the LayerNorm -> fh2 sites (fh2 mode)
static int ln_scales(a3r_model_s* m, void* stream) {
    const int E = m->cfg.enc_embed_dim, D = m->cfg.dec_embed_dim;
    hipStream_t st = as_stream(stream);
    m->ln_scale.clear();
    if (m->gemm_form != Form::FH2) return A3R_OK;
    std::vector<std::pair<const float*, const float*>> lns;      // (gamma, beta) of every LayerNorm whose output feeds a GEMM
    auto add_block = [&](const BlockW& b, bool cross) {
        lns.push_back({b.n1w, b.n1b}); lns.push_back({b.n2w, b.n2b});
        if (cross) { lns.push_back({b.n3w, b.n3b}); lns.push_back({b.nyw, b.nyb}); }
    };
    for (const BlockW& b : m->enc) add_block(b, false);
    for (const BlockW& b : m->pc) add_block(b, false);
    for (const BlockW& b : m->dec1) add_block(b, true);
    for (const BlockW& b : m->dec2) add_block(b, true);
    float* scratch = reinterpret_cast<float*>(m->stats);          // two words of the (still unused) statistics area
    for (size_t i = 0; i < lns.size(); i++) {
        const int Dn = i < 2 * m->enc.size() ? E : D;
        float gb[2] = {0.f, 0.f};
        if (int rc = a3r_absmax(lns[i].first, Dn, scratch, stream)) return rc;
        if (int rc = a3r_absmax(lns[i].second, Dn, scratch + 1, stream)) return rc;
        A3R_HIP(hipMemcpyAsync(gb, scratch, 8, hipMemcpyDeviceToHost, st));
        A3R_HIP(hipStreamSynchronize(st));
        if (!std::isfinite(gb[0]) || !std::isfinite(gb[1])) {
            set_error("a3r_model_finalize: a LayerNorm weight contains non-finite values");
            return A3R_EINVAL;
        }
        m->ln_scale[lns[i].first] = ln_static_scale(gb[0], gb[1], Dn);
    }
    A3R_HIP(hipMemsetAsync(m->stats, 0, 8, st));
    return A3R_OK;
}

extern "C" int a3r_model_finalize(a3r_model_t m, void* packed, size_t packed_bytes, void* stream) {
    A3R_CHECK_ARG(m && packed, "a3r_model_finalize: null argument");
    size_t total = 0;
    std::vector<PackItem> plan = pack_plan(m, &total);
    A3R_CHECK_ARG(packed_bytes >= total, "a3r_model_finalize: packed buffer too small (%zu < %zu)", packed_bytes, total);
    A3R_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & 255) == 0, "a3r_model_finalize: packed buffer must be 256-byte aligned");
    const a3r_model_config& c = m->cfg;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim;
    char* pk = static_cast<char*>(packed);
    PackedPtrs packed_ptr;
    if (int rc = repack_weights(m, plan, pk, stream, packed_ptr)) return rc;
    // --- bind
    NEED("patch_embed.proj.weight", &m->pe_w, E, 3, 16, 16); NEED("patch_embed.proj.bias", &m->pe_b, E);
    NEED("patch_embed_point_cloud.proj.weight", &m->pepc_w, D, 3, 16, 16); NEED("patch_embed_point_cloud.proj.bias", &m->pepc_b, D);
    NEED("enc_norm.weight", &m->encn_w, E); NEED("enc_norm.bias", &m->encn_b, E);
    NEED("decoder_embed.weight", &m->de_w, D, E); NEED("decoder_embed.bias", &m->de_b, D);
    NEED("dec_norm.weight", &m->decn_w, D); NEED("dec_norm.bias", &m->decn_b, D);
    m->enc.assign(c.enc_depth, BlockW());
    for (int i = 0; i < c.enc_depth; i++)
        if (int rc = bind_block(m, "enc_blocks." + std::to_string(i), E, E * c.mlp_ratio, false, &m->enc[i])) return rc;
    const int npc = n_pc_blocks(c);
    m->pc.assign(npc, BlockW());
    for (int i = 0; i < npc; i++)
        if (int rc = bind_block(m, "dec_blocks_pc." + std::to_string(i), D, D * c.mlp_ratio, false, &m->pc[i])) return rc;
    m->dec1.assign(c.dec_depth, BlockW());
    m->dec2.assign(c.dec_depth, BlockW());
    for (int i = 0; i < c.dec_depth; i++) {
        if (int rc = bind_block(m, "dec_blocks." + std::to_string(i), D, D * c.mlp_ratio, true, &m->dec1[i])) return rc;
        if (int rc = bind_block(m, "dec_blocks2." + std::to_string(i), D, D * c.mlp_ratio, true, &m->dec2[i])) return rc;
        const float* kv1 = packed_ptr["dec_blocks." + std::to_string(i) + ".cross_attn.kv"];
        const float* kv2 = packed_ptr["dec_blocks2." + std::to_string(i) + ".cross_attn.kv"];
        m->dec1[i].kvw = kv1; m->dec1[i].kvb = kv1 + (size_t)2 * D * D;
        m->dec2[i].kvw = kv2; m->dec2[i].kvb = kv2 + (size_t)2 * D * D;
    }
    m->zc_w.assign(npc + 1, nullptr);
    m->zc_b.assign(npc + 1, nullptr);
    for (int i = 0; i <= npc; i++) {
        NEED("zero_convs." + std::to_string(i) + ".0.weight", &m->zc_w[i], D, D, 1);
        NEED("zero_convs." + std::to_string(i) + ".0.bias", &m->zc_b[i], D);
    }
    for (int h = 0; h < 2; h++)
        if (int rc = bind_head(m, h, packed_ptr)) return rc;
    if (int rc = ln_scales(m, stream)) return rc;
    // --- twins of the nn.Linear and conv weights
    m->twins.t.clear();
    for (const PackItem& it : plan) {
        if (it.kind != Pack::TWIN) continue;
        auto pit = packed_ptr.find(it.name);                             // a repacked weight (3x3 convs, the concatenated cross-attention k/v) ...
        const float* src = pit != packed_ptr.end() ? pit->second : m->w.find(it.name)->p;      // ... or one bound (and shape-checked) above
        float* scratch = reinterpret_cast<float*>(pk + it.off + a3r_fh2_bytes(it.a, it.b));
        if (int rc = m->twins.pack(src, (Form)it.s, src, pk + it.off, it.a, it.b, scratch, "a3r_model_finalize", it.name.c_str(), stream)) return rc;
    }
    m->finalized = true;
    m->drop_stored();
    return A3R_OK;
}

// ------------------------------------------------------------------------------------------- launch plan
namespace {

// What one of the stores kept across calls does in a call (device lists; dedup.h, CallLists).  The branch whose products are kept
// runs on the n_fresh distinct items that are not stored, uniq_fresh [n_fresh] (slots); item k of the call's U distinct ones is
// entry ent[k]'s when miss[k] < 0, else the miss[k]-th of those, whose products go to entry ent[k] when that is >= 0 (n_store of
// them do).  src: where the pass that consumes the products finds those of a slot, in an entry (>= 0) or among the fresh blocks
// (~j) (prior_lists, head_lists; null for the frame cache, whose exchange pass reads ent / miss).
// With n_fresh == 0 the branch's ops are walked muted (Plan::mute) on one item's rows.
struct StoreCall {
    int n_fresh, n_store; const int32_t *uniq_fresh, *ent, *miss, *src;
    int frames() const { return n_fresh ? n_fresh : 1; }      // items the branch's ops are walked with
};
// the frame cache (images, U = n_img) and the stored priors (pred_depth maps, U = n_pd; src [2 B], src_ent [2 n_ent]: the z rows
// of a slot / of a block-0 entry): the storage as entries, and the call's keys of that kind
struct FrameCall : StoreCall {
    FrameCacheLayout lay; const void* keys; const int32_t* src_ent;
    unsigned* stat_words() const { return reinterpret_cast<unsigned*>(lay.stats); }      // [cap][FC_STAT_WORDS]
};
// the head products of one side (U = n_side[s], src [B]: the c and r0 of a slot)
struct HeadCall : StoreCall { HeadStore st; };

struct Plan {
    a3r_model_s* m;
    Arena ar;
    void* stream;
    int rc = A3R_OK;
    bool trace = getenv("A3R_TRACE") != nullptr;   // debugging aid: name + synchronise every op
    int opno = 0;
    bool dry() const { return ar.dry; }
    // mute: the ops are walked -- allocations, sites and their scales as ever -- but launch nothing (the encoder stage of a call
    // whose every frame was found in the frame cache)
    bool mute = false;
    // the sites of the branches whose products are kept across calls (StoreScope), whose words the entries read complete: the
    // encoder's, the depth-prior branch's, the level-0 branch's of each head
    SiteMask enc_sites, prior_sites, head_sites[2];
    // ---- fh2 range control: every op that WRITES an fh2 tensor is a site (numbered in plan order) with its own power-of-two
    // scale; the scale travels with the buffer pointer to the ops that read it
    int phase = 0, site_no = 0;
    std::map<const void*, float> buf_scale;
    struct Site { float scale; unsigned* stat; };
    Site site(const void* buf, const void* alias = nullptr) {
        const int id = site_no++;
        if (dry() || rc != A3R_OK) return {1.f, nullptr};
        if (id >= a3r_model_s::MAX_SITES) {
            set_error("a3r_model_forward: more than %d fh2 sites in the launch plan", a3r_model_s::MAX_SITES);
            rc = A3R_ESTATE;
            return {1.f, nullptr};
        }
        std::vector<float>& sc = m->site_scale[phase];
        if ((int)sc.size() <= id) sc.resize(id + 1, 1.f);
        buf_scale[buf] = sc[id];
        if (alias) buf_scale[alias] = sc[id];
        return {sc[id], m->stats + id};
    }
    float scale_of(const void* buf) {
        if (dry() || rc != A3R_OK) return 1.f;
        auto it = buf_scale.find(buf);
        if (it == buf_scale.end()) {
            set_error("a3r_model_forward: internal: an fh2 operand without a recorded scale");
            rc = A3R_ESTATE;
            return 1.f;
        }
        return it->second;
    }
    static constexpr const char* WHO = "a3r_model_forward";
    bool skip() { return ar.skip(rc, WHO); }
    void traced(const char* what, int a = 0, int b = 0, int c = 0) {
        if (!trace || dry()) return;
        hipError_t e = hipStreamSynchronize(as_stream(stream));
        fprintf(stderr, "[a3r trace] op %d before %s(%d,%d,%d): previous ops %s\n", opno++, what, a, b, c,
                e == hipSuccess ? "ok" : hipGetErrorString(e));
        fflush(stderr);
    }

    OpEpi epi(int kind, const float* bias, const float* resid = nullptr, const float* resid2 = nullptr) {
        OpEpi e = {};
        e.epi = kind; e.bias = bias; e.resid = resid; e.resid2 = resid2;
        return e;
    }
    // ---- operand forms.  gf: the "GEMM input" (gin) buffers -- [rows, K] rows that only feed a transformer GEMM -- and the attention
    // operands (q / k / v written by the RoPE projections); mf: the DPT maps that only feed a conv or the fusion blocks' 1x1 out_conv
    Form gf = Form::FH2, mf = Form::FH2;
    // BF3 GEMMs only: buffers that are only ever read as the A operand of a GEMM (LayerNorm / attention / fc1+GELU outputs, split
    // activations) are kept in the row-pair form of the layout (bf3.h) when the row counts of both views are even
    // (pair_all: the call's; a stage on fewer rows than both views' needs that row count to be even too: rows)
    bool pair = false, pair_all = false;
    void rows(long M) { pair = pair_all && M % 2 == 0; }
    float* gin_alloc(size_t rows, int K) { return ar.alloc(form_floats(gf, rows, K)); }
    float* gin_scratch(size_t rows, int K) { return ar.alloc(gf == Form::F32 ? 0 : form_floats(gf, rows, K)); }     // only needed for splitting
    template <class T> T* gin_at(T* base, size_t rows, int K) const { return base + form_floats(gf, rows, K); }
    // column `col` (a multiple of 8) of a gin row
    const float* gin_col(const float* base, int col) const { return base + form_floats(gf, 1, col); }
    float* map_alloc(size_t rows, int K) { return ar.alloc(form_floats(mf, rows, K)); }
    // the site of an output written in form f (only fh2 outputs are sites)
    Site out_site(Form f, const void* buf) { return f == Form::FH2 ? site(buf) : Site{1.f, nullptr}; }
    // fp32 [M, K] -> form f, which is not F32
    void split(Form f, bool row_pair, const char* what, const float* x, float* y, long M, int K) {
        if (skip()) return;
        traced(what, (int)M, K);
        const Site s = out_site(f, y);
        if (!rc && !mute) rc = op_split(f, x, K, y, M, K, row_pair, s.scale, s.stat, stream);
    }
    // fp32 activation -> GEMM input: a split pass into `scratch`, the array itself on the exact-fp32 kernels
    const float* gin_from(const float* x, float* scratch, long M, int K) {
        if (gf == Form::F32) return x;
        split(gf, pair, "split_gin", x, scratch, M, K);
        return scratch;
    }
    const Twin* twin(const float* w, Form f) { return f == Form::F32 ? nullptr : m->twins.get(w, f, WHO, rc); }
    // the range fields of an fh2 launch: the operand's scale, and a site for the fh2 output (y itself or the aux twin)
    void range_epi(a3r_epilogue& e, const void* x2, const void* y) {
        e.x_scale = scale_of(x2);
        if (e.out_fh2 || e.aux_fh2) {
            const Site s = site(e.out_fh2 ? y : e.aux_fh2);
            e.out_scale = s.scale; e.out_absmax = s.stat;
        }
    }
    // nn.Linear on a GEMM-input buffer; plain_x: xg is a DPT map instead (map form, plain rows)
    void linear(const float* xg, int lda, const float* w, float* y, int ldc, int M, int N, int K, const OpEpi& e0, bool plain_x = false) {
        if (skip()) return;
        traced("linear", M, N, K);
        const Form f = plain_x ? mf : gf;
        const Twin* tw = twin(w, f);
        a3r_epilogue e = retarget(e0, f, [&](a3r_epilogue& r) { range_epi(r, xg, y); });
        e.x_pair = (f == Form::BF3 && pair && !plain_x) ? 1 : 0;
        if (!rc && !mute) rc = op_linear(f, xg, lda, w, tw, y, ldc, M, N, K, e, stream);
    }
    // nn.Linear / 1x1 conv on a plain fp32 activation (DPT adapters), exact-fp32 MFMA
    void linear_f32(const float* x, int lda, const float* w, float* y, int ldc, int M, int N, int K, const a3r_epilogue& e) {
        if (skip()) return;
        traced("linear_f32", M, N, K);
        if (!mute) rc = a3r_linear(x, lda, w, y, ldc, M, N, K, &e, stream);
    }
    // the same-shape projection of both decoders (dec_blocks[i] on view 1, dec_blocks2[i] on view 2) in one launch
    void linear2(const float* x0, const float* x1, int lda, const float* w0, const float* w1, const float* b0, const float* b1,
                 float* y0, float* y1, int ldc, int M, int N, int K, const OpEpi& e0, const float* r0 = nullptr, const float* r1 = nullptr) {
        if (skip()) return;
        traced("linear2", M, N, K);
        const Twin *t0 = twin(w0, gf), *t1 = twin(w1, gf);
        if (rc) return;
        const bool fh2 = gf == Form::FH2;
        // the two sides' outputs are ONE site (one scale: the attention kernel reads both sides in one launch)
        const Site so = fh2 && e0.out_op ? site(y0, y1) : Site{1.f, nullptr};
        const GroupSide g[2] = {{x0, w0, t0, y0, b0, r0, fh2 ? scale_of(x0) : 1.f}, {x1, w1, t1, y1, b1, r1, fh2 ? scale_of(x1) : 1.f}};
        a3r_epilogue e = retarget(e0, gf, [](a3r_epilogue&) {});      // (the grouped entry point takes the range fields per side)
        e.x_pair = pair ? 1 : 0;
        if (!rc) rc = op_linear_grouped(gf, g, so.scale, so.stat, lda, ldc, M, N, K, e, stream);
    }
    // ---- the DPT heads' ops on maps in operand form.  F32 maps are the degenerate operand form: the form of x is x itself (map_twin
    // allocates nothing, split_map does nothing), an auxiliary output has nowhere to go (aux), and a consumer that wants relu(x)
    // applies the ReLU as it loads (relu_a, rcu_conv1)
    float* map_twin(float* x, size_t rows, int K) { return mf == Form::F32 ? x : map_alloc(rows, K); }
    void split_map(const float* x, float* ym, long M, int K) { if (mf != Form::F32) split(mf, false, "split_map", x, ym, M, K); }
    void aux(OpEpi& e, float* twin, bool relu) { if (mf != Form::F32) { e.aux_op = twin; e.aux_relu = relu ? 1 : 0; } }
    void conv(const float* xm, const float* wp, float* y, int B, int H, int W, int Cin, int Cout, int stride, const OpEpi& e0) {
        if (skip()) return;
        traced("conv3x3", H, W, Cin);
        const Twin* tw = twin(wp, mf);
        const a3r_epilogue e = retarget(e0, mf, [&](a3r_epilogue& r) { range_epi(r, xm, y); });
        if (!rc && !mute) rc = op_conv3x3(mf, xm, wp, tw, y, B, H, W, Cin, Cout, stride, e, stream);
    }
    // bilinear 2x of an fp32 map, written in form f (the map form, or F32 for a consumer that needs the values)
    void up(Form f, const float* x, float* y, int B, int H, int W, int C, int Hc, int Wc) {
        if (skip()) return;
        traced("upsample2x", H, W, C);
        const Site s = out_site(f, y);
        if (!rc) rc = op_upsample2x(f, x, y, B, H, W, C, Hc, Wc, s.scale, s.stat, stream);
    }
    // s = c[map] + (r[map] + extra) and the fh2 form of relu(s): the RESID2 epilogue + aux output of a conv that ran on distinct frames
    // hc (head products of side hs): c and r are the fresh frames' blocks, and every slot reads its own where hc->src says, in
    // the storage or there
    void combine_map(const float* c, const float* r, const float* extra, const int32_t* map, float* s, float* sr2, int S, long px, int C,
                     const HeadCall* hc, int hs) {
        if (skip()) return;
        traced("combine_resid", S, (int)px, C);
        const Site st = site(sr2);
        if (rc) return;
        if (hc) rc = a3r_combine_resid_fh2_src(c, r, hc->st.c(hs), hc->st.r0(hs), hc->st.stride(), hc->src, extra, s, sr2, S, px, C, st.scale, st.stat, stream);
        else rc = a3r_combine_resid_fh2(c, r, extra, map, s, sr2, S, px, C, st.scale, st.stat, stream);
    }
    // the same with extra = the bilinear 2x of x [S, H, W, C] made inside the kernel
    void up_combine_map(const float* x, const float* c, const float* r, const int32_t* map, float* s, float* sr2, int S, int H, int W,
                        int C, int Hc, int Wc, const HeadCall* hc, int hs) {
        if (skip()) return;
        traced("upsample2x_combine", H, W, C);
        const Site st = site(sr2);
        if (rc) return;
        if (hc) rc = a3r_upsample2x_combine_fh2_src(x, c, r, hc->st.c(hs), hc->st.r0(hs), hc->st.stride(), hc->src, s, sr2, S, H, W, C, Hc, Wc, st.scale, st.stat, stream);
        else rc = a3r_upsample2x_combine_fh2(x, c, r, map, s, sr2, S, H, W, C, Hc, Wc, st.scale, st.stat, stream);
    }
    // LayerNorm whose output feeds a GEMM (written directly in the GEMMs' operand form)
    void ln(const float* x, const float* w, const float* b, float* yg, int M, int D) {
        if (skip()) return;
        traced("layernorm", M, D);
        if (gf == Form::FH2) {
            // static scale (ln_static_scale): no statistics, the kernel keeps its one-row-per-wave grid
            auto it = m->ln_scale.find(w);
            const float sc = it == m->ln_scale.end() ? 1.f : it->second;
            buf_scale[yg] = sc;
            if (!mute) rc = a3r_layernorm_fh2(x, w, b, yg, M, D, 1e-6f, sc, nullptr, stream);
        } else if (!mute) rc = gf == Form::BF3 ? a3r_layernorm_bf3(x, w, b, yg, M, D, 1e-6f, pair, stream) : a3r_layernorm(x, w, b, yg, M, D, 1e-6f, stream);
    }
    void ln_f32(const float* x, const float* w, const float* b, float* y, int M, int D) {
        if (skip()) return;
        traced("layernorm_f32", M, D);
        if (!mute) rc = a3r_layernorm(x, w, b, y, M, D, 1e-6f, stream);
    }
    // q, k, v, o are gin buffers (operand forms: straight from / to the projection GEMMs, no fp32 round trip)
    // kv_buf: the buffer k and v are columns of when it is not q's (cross-attention); o_alias: the second side's rows of o when the
    // consumer addresses them by their own pointer (linear2)
    // q_map / kv_map (fh2 only, device, B words): image b reads the q rows of image q_map[b] and the k / v rows of image kv_map[b]
    void attn(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo, int B, int H, int Nq, int Nk,
              const float* kv_buf = nullptr, const float* o_alias = nullptr, const int32_t* q_map = nullptr, const int32_t* kv_map = nullptr) {
        if (skip()) return;
        traced("attention", B, Nq, Nk);
        if (gf == Form::FH2) {
            const float sq = scale_of(q), skv = kv_buf ? scale_of(kv_buf) : sq;
            const Site so = site(o, o_alias);
            const a3r_fh2_attn_range r = {sq, skv, skv, so.scale, so.stat};
            if (!rc && !mute) rc = a3r_attention_fh2_mapped(q, ldq, k, ldk, v, ldv, o, ldo, B, H, Nq, Nk, &r, q_map, kv_map, stream);
            return;
        }
        if (mute) return;
        rc = gf == Form::BF3 ? a3r_attention_bf3(q, ldq, k, ldk, v, ldv, o, ldo, B, H, Nq, Nk, pair, stream)
                   : a3r_attention(q, ldq, k, ldk, v, ldv, o, ldo, B, H, Nq, Nk, stream);
    }
    // projection feeding attention: RoPE on the leading columns, output in gin form
    OpEpi rope_epi(const float* bias, int rope_cols, int ntok, int gw) {
        OpEpi e = epi(A3R_EPI_ROPE, bias);
        e.out_op = 1;
        e.rope_cols = rope_cols; e.tokens_per_image = ntok; e.grid_w = gw;
        e.rope_cos = m->rope_cos; e.rope_sin = m->rope_sin;
        return e;
    }

    // Block.forward blocks.py:127-130 on x [M, D] in place (self-attention over images of ntok tokens)
    // xn [M, D], qkv [M, 3 D], att [M, D]: gin buffers
    void self_block(const BlockW& w, float* x, const float* resid_src, int M, int D, int H, int ntok, int gw, float* xn,
                    float* qkv, float* att) {
        // x_out = resid_src + attn(LN1(resid_src)); then MLP in place on x
        ln(resid_src, w.n1w, w.n1b, xn, M, D);
        linear(xn, D, w.qkvw, qkv, 3 * D, M, 3 * D, D, rope_epi(w.qkvb, 2 * D, ntok, gw));
        attn(qkv, 3 * D, gin_col(qkv, D), 3 * D, gin_col(qkv, 2 * D), 3 * D, att, D, M / ntok, H, ntok, ntok);
        linear(att, D, w.projw, x, D, M, D, D, epi(A3R_EPI_RESID, w.projb, resid_src));
    }
    // hid: gin [M, hidden] -- fc1's GELU epilogue writes the GEMM-input form directly (Mlp blocks.py:73-77)
    OpEpi gin_epi(int kind, const float* bias) {
        OpEpi e = epi(kind, bias);
        e.out_op = 1;
        e.out_pair = pair ? 1 : 0;
        return e;
    }
    void mlp(const BlockW& w, const float* nw, const float* nb, float* x, int M, int D, int hidden, float* xn, float* hid) {
        ln(x, nw, nb, xn, M, D);
        linear(xn, D, w.fc1w, hid, hidden, M, hidden, D, gin_epi(A3R_EPI_GELU, w.fc1b));
        linear(hid, hidden, w.fc2w, x, D, M, D, hidden, epi(A3R_EPI_RESID, w.fc2b, x));
    }
};

// ---- the DPT blocks on maps in operand form (F32, bf3 or fh2).  A conv input lives in operand form; where the fp32 value is also
// needed (skip connections) the producer writes both (Plan::aux), pre-activated when the consumer is an RCU (which starts with a ReLU).
// first conv of an rcu (dpt_block.py:120-142): tmp3 = operand form of relu(conv1(relu(x))), xr3 being the operand form of relu(x)
void rcu_conv1(Plan& P, const RcuW& w, const float* xr3, float* tmp3, int B, int H, int W, int F) {
    OpEpi e1 = P.epi(A3R_EPI_RELU, w.c1b);
    e1.out_op = 1;
    e1.relu_a = P.mf == Form::F32;      // xr3 is x itself there
    P.conv(xr3, w.c1w, tmp3, B, H, W, F, F, 1, e1);
}
// rcu: out = conv2(relu(conv1(relu(x)))) + x (+ extra).  x: fp32 [B,H,W,F]; xr3: operand form of relu(x); tmp3: operand-form scratch;
// out: fp32; out_r3: operand form of relu(out) or null (aux_relu = false: of out itself, for a consumer that does not start with a ReLU)
void rcu_map(Plan& P, const RcuW& w, const float* x, const float* xr3, const float* extra, float* tmp3, float* out, float* out_r3,
             int B, int H, int W, int F, bool aux_relu = true) {
    rcu_conv1(P, w, xr3, tmp3, B, H, W, F);
    OpEpi e2 = extra ? P.epi(A3R_EPI_RESID2, w.c2b, x, extra) : P.epi(A3R_EPI_RESID, w.c2b, x);
    if (out_r3) P.aux(e2, out_r3, aux_relu);
    P.conv(tmp3, w.c2w, out, B, H, W, F, F, 1, e2);
}

// The level-0 branch of a head on the distinct frames of its side (fh2 maps): x1 / x1r3 of fusion_map hold U < B images, slot b's
// being map[b] (device).  fold: x0 of fusion_map is not there -- the previous fusion block left its output before the bilinear 2x
// (x0_lo [B, lo_h, lo_w, F]) and the combine pass interpolates it on the fly.
// hc (head products kept across calls, side `side`): the branch runs on the hc->n_fresh frames of the U that are not stored -- the
// buffers keep their size, fewer rows of them are used -- and the combine pass reads every slot's c and r0 where hc->src says.
struct HeadMerge { int U; const int32_t* map; bool fold; const float* x0_lo; int lo_h, lo_w; const HeadCall* hc; int side; };
// The ops of a branch whose products store `sc` keeps (null: none does), walked while one of these lives: launched on the fresh
// items' rows, or not at all (Plan::mute) when every item is stored, and their sites noted in `sites` for the statistics pass
// that follows the branch (stats_sites_words)
struct StoreScope {
    Plan& P;
    const StoreCall* sc;
    SiteMask& sites;
    int lo;
    StoreScope(Plan& P_, const StoreCall* sc_, SiteMask& sites_) : P(P_), sc(sc_), sites(sites_), lo(P_.site_no) { if (sc) P.mute = sc->n_fresh == 0; }
    ~StoreScope() {
        if (!sc) return;
        P.mute = false;
        sites.add(lo, P.site_no);
    }
};
static bool dpt_ref_order() {       // A/B switch: up-sample first, as the reference does
    static const bool on = getenv("A3R_DPT_REF_ORDER") != nullptr;
    return on;
}

// FeatureFusionBlock_custom.forward (dpt_block.py:186-218) on x0 (the previous block's output; x0r3: its pre-activated operand form,
// read only when the block has no xs[1]) and x1 = xs[1] (`two` says whether it exists: pointers are null during the dry sizing pass).
// Returns fp32 [B, Hc, Wc, F] with (Hc, Wc) = crop of (2H, 2W), or its operand form when `last` (refinenet1's output only feeds
// head.0's 3x3 conv).
// hm: resConfUnit1 depends on the pair through the residual x0 alone -- its two convs run on hm->U images, the second with the
// bias-only epilogue, and combine_map adds the skip and x0 per slot in the RESID2 epilogue's order and writes the fh2 twin (that
// conv's auxiliary site: the sites keep their number and order).  lo_out: leave the block's output before the bilinear 2x there
// and return null (the fp32 up-sample has no site) -- the next block's combine pass makes the 2x map itself (HeadMerge::fold).
float* fusion_map(Plan& P, const FusionW& w, const float* x0, const float* x0r3, const float* x1, const float* x1r3, bool two, int B,
                  int H, int W, int F, int Hc, int Wc, bool last, const HeadMerge* hm = nullptr, const float** lo_out = nullptr) {
    Arena& ar = P.ar;
    const size_t px = (size_t)B * H * W, n = px * F, opx = (size_t)B * Hc * Wc;
    float* tmp3 = P.map_alloc(px, F);
    const float *cur, *cur3;
    if (two) {
        float* s = ar.alloc(n);
        float* sr3 = P.map_twin(s, px, F);
        if (hm) {
            float* c = ar.alloc((size_t)hm->U * H * W * F);
            const HeadCall* hc = hm->hc;
            const int Uf = hc ? hc->frames() : hm->U;
            {
                StoreScope scope(P, hc, P.head_sites[hm->side]);
                rcu_conv1(P, w.r1, x1r3, tmp3, Uf, H, W, F);
                P.conv(tmp3, w.r1.c2w, c, Uf, H, W, F, F, 1, P.epi(A3R_EPI_NONE, w.r1.c2b));
            }
            if (hc && hc->n_store && !P.skip()) P.rc = head_products_store(hc->st, hm->side, hc->ent, hc->miss, hm->U, x1, c, P.stream);
            if (hm->fold) P.up_combine_map(hm->x0_lo, c, x1, hm->map, s, sr3, B, hm->lo_h, hm->lo_w, F, H, W, hc, hm->side);
            else P.combine_map(c, x1, x0, hm->map, s, sr3, B, (long)H * W, F, hc, hm->side);
        } else
            rcu_map(P, w.r1, x1, x1r3, x0, tmp3, s, sr3, B, H, W, F);     // output + resConfUnit1(xs[1])
        cur = s; cur3 = sr3;
    } else {
        cur = x0; cur3 = x0r3;
    }
    float* o = ar.alloc(n);
    if (dpt_ref_order() || P.mf == Form::F32) {
        // the reference's order: up-sample, then out_conv.  F32 maps always run it (a map has no operand form to hand to the 1x1 GEMM)
        rcu_map(P, w.r2, cur, cur3, nullptr, tmp3, o, nullptr, B, H, W, F);
        float* u3 = P.map_alloc(opx, F);
        P.up(P.mf, o, u3, B, H, W, F, Hc, Wc);
        OpEpi e = P.epi(A3R_EPI_NONE, w.ob);
        e.out_op = last;
        float* r = last ? P.map_alloc(opx, F) : ar.alloc(opx * F);
        P.linear(u3, F, w.ow, r, F, (int)opx, F, F, e, /*plain_x=*/true);
        return r;
    }
    // out_conv (1x1, dpt_block.py:216) is applied BEFORE the bilinear 2x instead of after it: both are linear maps over
    // different axes (channels / pixels) and the interpolation weights sum to one, so conv(up(x)) + b == up(conv(x) + b) up
    // to fp32 rounding -- a quarter of the 1x1 GEMM's rows, and the full-resolution map is written once instead of three times.
    float* o3 = P.map_alloc(px, F);
    rcu_map(P, w.r2, cur, cur3, nullptr, tmp3, o, o3, B, H, W, F, /*aux_relu=*/false);
    float* lo = ar.alloc(n);
    P.linear(o3, F, w.ow, lo, F, (int)px, F, F, P.epi(A3R_EPI_NONE, w.ob), /*plain_x=*/true);
    if (lo_out) { *lo_out = lo; return nullptr; }
    float* r = last ? P.map_alloc(opx, F) : ar.alloc(opx * F);
    P.up(last ? P.mf : Form::F32, lo, r, B, H, W, F, Hc, Wc);
    return r;
}

// The distinct inputs of a call (dedup.h): n_img / n_pd of the 2 B images / pred_depth maps are distinct (2 B: that kind is not
// merged).  Device lists: uniq_* [n] the distinct slots, map_* [2 B] each slot's row in that list (null in the sizing pass).
// Per side s (slots [s B, (s + 1) B) of the first kind): n_side[s] distinct frames when the head of that side merges its level-0
// branch (head_merge_fits), B when it does not; uniq_side[s] [n_side[s]] the first slot of the side holding each, map_side[s] [B].
struct Distinct {
    int n_img, n_pd; const int32_t *uniq_img, *map_img, *uniq_pd, *map_pd;
    int n_side[2]; const int32_t *uniq_side[2], *map_side[2];
    // Decoder block 0 on entries (dedup_group_entries; 0: it runs per slot): n_ent = Um entries per side, padded; ent_img / ent_pd
    // [2 Um] the image / prior row of each side's entries, map_eo [2 B] the row s Um + e of slot (s, b)'s entry e among the 2 Um, and
    // map_ekv [2 B] that of the other side's slot b inside side s's block, s Um + map_e[1 - s][b]: where slot (s, b)'s keys live
    int n_ent; const int32_t *ent_img, *ent_pd, *map_eo, *map_ekv;
    // Frames kept across calls (null: none are): the encoder runs on the images that were not found, and image k < n_img takes
    // its enc_norm rows from its entry or from the encoded ones, which go to their entries (frame_cache_exchange).  The image
    // stage then runs on the distinct list even when that holds all 2 B slots.
    const FrameCall* fc = nullptr;
    // Depth priors kept across calls with their zero-conv outputs (null: none are): the prior branch -- patch embedding,
    // dec_blocks_pc, zero-convs -- runs on the priors that were not found, whose z rows and map go to their entries; the
    // gather-add pass finds the z rows where src / src_ent say.  The prior stage then runs on the distinct list even when that
    // holds all 2 B slots.
    const FrameCall* pp = nullptr;
    // Head products kept across calls, per side (null: that side's head computes its level-0 branch for all its n_side[s] frames)
    const HeadCall* hp[2] = {nullptr, nullptr};
};
// the sizing pass: counts, no lists
Distinct distinct_counts(int n_img, int n_pd, int n_side) {
    return {n_img, n_pd, nullptr, nullptr, nullptr, nullptr, {n_side, n_side}, {nullptr, nullptr}, {nullptr, nullptr}, 0, nullptr, nullptr,
            nullptr, nullptr};
}

// ---- one call of the plan.  phase: 0 = whole forward from images; 1 = encoder only (img[0] [B,...] -> feat_out [B,N,E]);
// 2 = decoder + heads from cached encoder features (feat_in [B,N,E] per view).  dry: the sizing pass (every pointer null).
// dd: run the parts of the plan that depend on one frame alone -- the encoder, and the depth-prior token branch -- on the distinct
// frames only and copy their rows to every slot.  The ops, their order and so the fh2 site numbers are those of the plain plan;
// only row counts differ, and every row is computed as it is there.  dd->n_side: the same for the level-0 branch of each DPT head
// (fh2 maps only), whose rows are put back by the combine pass (fusion_map).
struct Call {
    int phase = 0, B = 0, H = 0, W = 0;
    bool dry = false;
    const float *img[2] = {nullptr, nullptr}, *pd[2] = {nullptr, nullptr};      // the two views' inputs ...
    float *pts[2] = {nullptr, nullptr}, *conf[2] = {nullptr, nullptr};          // ... and outputs
    const float* feat_in[2] = {nullptr, nullptr};
    float* feat_out = nullptr;
    void *ws = nullptr, *stream = nullptr;
    size_t ws_bytes = 0;
    const Distinct* dd = nullptr;
};

// its shapes: widths, the token grid, rows of one view (BN) and of both (M2), and the rows of the image / depth-prior stages: Mi / Mp
// < M2 for a merged kind (d_img, d_pd).  The distinct frames' enc_norm rows wait in the first three decoder level buffers, which
// must hold them: E <= 3 D at least.
struct Dims {
    const a3r_model_config& c;
    int B, H, W, E, D, F, L, nh, nw, N, BN, M2;
    bool d_img, d_pd;
    int Mi, Mp;
    const FrameCall* pp;      // the stored priors of this call, and the rows the prior branch then runs on (one image's when muted)
    int prior_rows() const { return pp ? pp->frames() * N : Mp; }
    Dims(const a3r_model_config& c_, const Call& k)
        : c(c_), B(k.B), H(k.H), W(k.W), E(c.enc_embed_dim), D(c.dec_embed_dim), F(c.feature_dim), L(c.last_dim), nh(k.H / 16),
          nw(k.W / 16), N(nh * nw), BN(B * N), M2(2 * BN),
          d_img(k.dd && k.phase == 0 && (k.dd->n_img < 2 * B || k.dd->fc) && (size_t)k.dd->n_img * N * E <= 3 * (size_t)M2 * D),
          d_pd(k.dd && (k.dd->n_pd < 2 * B || k.dd->pp)), Mi(d_img ? k.dd->n_img * N : M2), Mp(d_pd ? k.dd->n_pd * N : M2),
          pp(k.dd ? k.dd->pp : nullptr) {}
};

// the buffers that outlive a stage (allocated below the arena mark the stages reset to), and what the stages hand on in them
struct Levels {
    float *feat, *pc, *fbuf[4], *dec_last;      // enc_norm output = level 0; depth-prior tokens; ping, pong, hook A, hook B; dec_norm
    float *tap_lvl, *tap_pc0;                   // debug taps (a3r_model_set_tap_level) or null
    // Distinct inputs only: no allocation is added.  The depth-prior tokens of the distinct maps, pcu [Mp, D], live in hook buffer
    // B, which the decoder first writes at level hook_b, after the last dec_blocks_pc block (dec_depth / 2 - 2 < hook_b); the
    // distinct frames' enc_norm rows wait in fbuf[0..2] (contiguous, idle until the decoder starts) for their copy to `feat`.
    float *featu, *pcu;
    const float *lvl_a = nullptr, *lvl_b = nullptr;      // the decoder levels the heads hook (decoder_stage)
};

// distinct rows -> the rows of all 2 B slots
void copy_rows(Plan& P, const Dims& g, const float* src, float* dst, const int32_t* map, int C) {
    if (!P.skip()) P.rc = gather_rows(src, dst, map, 2 * g.B, g.N, C, P.stream);
}
void tap_copy(Plan& P, const Dims& g, float* dst, const float* src) {
    if (P.dry() || P.rc != A3R_OK || !dst) return;
    if (hipMemcpyAsync(dst, src, (size_t)g.M2 * g.D * 4, hipMemcpyDeviceToDevice, as_stream(P.stream)) != hipSuccess) {
        set_error("a3r_model_forward: tap copy failed");
        P.rc = A3R_EHIP;
    }
}

// ViT encoder (_encode_image model.py:151-163) on M = n N rows: the images of k.img -- the distinct ones (d_img; with a frame
// cache those of them it does not hold), both views', or the B frames of an encode call (img[1] null) -- patchified into cols,
// enc_norm rows to `out`.  Under P.mute (no image left to encode) M is one image's rows and nothing is launched.
void encoder_stage(Plan& P, const Call& k, const Dims& g, float* cols, float* cols3, int M, float* out) {
    a3r_model_s* m = P.m;
    const int E = g.E, hidden = E * g.c.mlp_ratio;
    float* x = P.ar.alloc((size_t)M * E);
    float* xn = P.gin_alloc(M, E);
    float* qkv = P.gin_alloc(M, 3 * E);
    float* att = P.gin_alloc(M, E);
    float* hid = P.gin_alloc(M, hidden);
    if (!P.skip() && !P.mute) {
        const long sb = 3L * g.H * g.W, sc = (long)g.H * g.W, sy = g.W, sx = 1;
        const FrameCall* fc = g.d_img ? k.dd->fc : nullptr;
        if (fc) P.rc = patchify_indexed(k.img[0], k.img[1], fc->uniq_fresh, fc->n_fresh, g.B, cols, 3, g.H, g.W, sb, sc, sy, sx, P.stream);
        else if (g.d_img) P.rc = patchify_indexed(k.img[0], k.img[1], k.dd->uniq_img, k.dd->n_img, g.B, cols, 3, g.H, g.W, sb, sc, sy, sx, P.stream);
        else if (!(P.rc = a3r_patchify(k.img[0], cols, g.B, 3, g.H, g.W, sb, sc, sy, sx, P.stream)) && k.img[1])
            P.rc = a3r_patchify(k.img[1], cols + (size_t)g.BN * 768, g.B, 3, g.H, g.W, sb, sc, sy, sx, P.stream);
    }
    P.rows(M);
    P.linear(P.gin_from(cols, cols3, M, 768), 768, m->pe_w, x, E, M, E, 768, P.epi(A3R_EPI_NONE, m->pe_b));
    for (const BlockW& w : m->enc) {
        P.self_block(w, x, x, M, E, g.c.enc_num_heads, g.N, g.nw, xn, qkv, att);
        P.mlp(w, w.n2w, w.n2b, x, M, E, hidden, xn, hid);
    }
    P.rows(g.M2);
    P.ln_f32(x, m->encn_w, m->encn_b, out, M, E);
}

// decode call: the cached per-frame features of the two views, gathered into the [2 B N, E] layout the decoder expects
void load_features(Plan& P, const Call& k, const Dims& g, float* feat) {
    if (P.skip()) return;
    const size_t bytes = (size_t)g.BN * g.E * sizeof(float);
    hipError_t e1 = hipMemcpyAsync(feat, k.feat_in[0], bytes, hipMemcpyDeviceToDevice, as_stream(P.stream));
    hipError_t e2 = hipMemcpyAsync(feat + (size_t)g.BN * g.E, k.feat_in[1], bytes, hipMemcpyDeviceToDevice, as_stream(P.stream));
    if (e1 != hipSuccess || e2 != hipSuccess) { set_error("a3r_model_decode: feature copy failed"); P.rc = A3R_EHIP; }
}

// point-map patch embedding (model.py:244-248) of the Mp rows of the (distinct) depth priors -> pcu; pred_depth is [B,H,W,3]:
// channel stride 1
// With stored priors (g.pp) the rows are those of the priors not found, and their maps and keys go to their entries.
void embed_pc_stage(Plan& P, const Call& k, const Dims& g, float* cols, float* cols3, float* pcu) {
    const FrameCall* pp = g.pp;
    const int Mq = g.prior_rows();
    {
        StoreScope scope(P, pp, P.prior_sites);
        if (!P.skip() && !P.mute) {
            const long sb = 3L * g.H * g.W, sc = 1, sy = 3L * g.W, sx = 3;
            if (pp) P.rc = patchify_indexed(k.pd[0], k.pd[1], pp->uniq_fresh, pp->n_fresh, g.B, cols, 3, g.H, g.W, sb, sc, sy, sx, P.stream);
            else if (g.d_pd) P.rc = patchify_indexed(k.pd[0], k.pd[1], k.dd->uniq_pd, k.dd->n_pd, g.B, cols, 3, g.H, g.W, sb, sc, sy, sx, P.stream);
            else if (!(P.rc = a3r_patchify(k.pd[0], cols, g.B, 3, g.H, g.W, sb, sc, sy, sx, P.stream)))
                P.rc = a3r_patchify(k.pd[1], cols + (size_t)g.BN * 768, g.B, 3, g.H, g.W, sb, sc, sy, sx, P.stream);
        }
        P.rows(Mq);
        P.linear(P.gin_from(cols, cols3, Mq, 768), 768, P.m->pepc_w, pcu, g.D, Mq, g.D, 768, P.epi(A3R_EPI_NONE, P.m->pepc_b));
        P.rows(g.M2);
    }
    if (pp && pp->n_store && !P.skip())
        P.rc = frame_cache_store(k.pd[0], k.pd[1], g.B, pp->keys, pp->lay, k.dd->uniq_pd, pp->ent, pp->miss, k.dd->n_pd, nullptr, 0, 0, P.stream);
}

// gin buffers of the decoder, [2 B N, .] rows: side 1 of each starts at gin_at(., BN, .)
struct DecBufs { float *xn, *yn, *qkv, *qb, *kv, *att, *hid; };

// DecoderBlock.forward (blocks.py:186-191) of dec_blocks[i] on view 1 and dec_blocks2[i] on view 2, cur -> nxt [2 B N, D].  Both
// decoders advance together: side s reads x = cur[s], y = cur[1-s] (model.py:218-220) and every same-shape projection of the two
// sides is one grouped launch.
void decoder_block_pair(Plan& P, const Dims& g, const BlockW& w0, const BlockW& w1, const float* cur, float* nxt, const DecBufs& t) {
    const int B = g.B, N = g.N, BN = g.BN, D = g.D, nw = g.nw, heads = g.c.dec_num_heads, hidden = D * g.c.mlp_ratio;
    const size_t S = (size_t)BN * D;                   // side stride in a [2*BN, D] buffer
    const float *x0 = cur, *x1 = cur + S;
    float *o0 = nxt, *o1 = nxt + S;
    float *xn = t.xn, *yn = t.yn, *qkv = t.qkv, *qb = t.qb, *kv = t.kv, *att = t.att, *hid = t.hid;
    // x = x + attn(norm1(x))                                   blocks.py:187
    float* xn1 = P.gin_at(xn, BN, D);                  // side 1 of the gin buffers
    float* yn1 = P.gin_at(yn, BN, D);
    P.ln(x0, w0.n1w, w0.n1b, xn, BN, D);
    P.ln(x1, w1.n1w, w1.n1b, xn1, BN, D);
    float* att1 = P.gin_at(att, BN, D);
    P.linear2(xn, xn1, D, w0.qkvw, w1.qkvw, w0.qkvb, w1.qkvb, qkv, P.gin_at(qkv, BN, 3 * D), 3 * D, BN, 3 * D, D,
              P.rope_epi(nullptr, 2 * D, N, nw));
    P.attn(qkv, 3 * D, P.gin_col(qkv, D), 3 * D, P.gin_col(qkv, 2 * D), 3 * D, att, D, 2 * B, heads, N, N, nullptr, att1);
    P.linear2(att, att1, D, w0.projw, w1.projw, w0.projb, w1.projb, o0, o1, D, BN, D, D, P.epi(A3R_EPI_RESID, nullptr), x0, x1);
    // y_ = norm_y(y); x = x + cross_attn(norm2(x), y_, y_)     blocks.py:188-189
    P.ln(x1, w0.nyw, w0.nyb, yn, BN, D);               // side 0 attends to view 2's tokens
    P.ln(x0, w1.nyw, w1.nyb, yn1, BN, D);
    P.ln(o0, w0.n2w, w0.n2b, xn, BN, D);
    P.ln(o1, w1.n2w, w1.n2b, xn1, BN, D);
    P.linear2(xn, xn1, D, w0.qw, w1.qw, w0.qb, w1.qb, qb, P.gin_at(qb, BN, D), D, BN, D, D, P.rope_epi(nullptr, D, N, nw));
    P.linear2(yn, yn1, D, w0.kvw, w1.kvw, w0.kvb, w1.kvb, kv, P.gin_at(kv, BN, 2 * D), 2 * D, BN, 2 * D, D,
              P.rope_epi(nullptr, D, N, nw));
    P.attn(qb, D, kv, 2 * D, P.gin_col(kv, D), 2 * D, att, D, 2 * B, heads, N, N, kv, att1);
    P.linear2(att, att1, D, w0.cprojw, w1.cprojw, w0.cprojb, w1.cprojb, o0, o1, D, BN, D, D, P.epi(A3R_EPI_RESID, nullptr), o0, o1);
    // x = x + mlp(norm3(x))                                    blocks.py:190
    P.ln(o0, w0.n3w, w0.n3b, xn, BN, D);
    P.ln(o1, w1.n3w, w1.n3b, xn1, BN, D);
    float* hid1 = P.gin_at(hid, BN, hidden);
    P.linear2(xn, xn1, D, w0.fc1w, w1.fc1w, w0.fc1b, w1.fc1b, hid, hid1, hidden, BN, hidden, D, P.gin_epi(A3R_EPI_GELU, nullptr));
    P.linear2(hid, hid1, hidden, w0.fc2w, w1.fc2w, w0.fc2b, w1.fc2b, o0, o1, D, BN, D, hidden, P.epi(A3R_EPI_RESID, nullptr), o0, o1);
}

// The same block on ENTRIES (dedup_group_entries): everything before the cross-attention product reads one side's level-0 rows
// alone, so it runs on xe [2 Um N, D] -- the level-0 rows of each side's Um distinct (image, prior) entries, side 1 at Um N rows --
// with the ops, their order and their sites as above.  Side s's keys and values are made from side 1 - s's entries with side s's
// weights.  The self-attention residual goes back into xe in place, one gather puts it into the per-slot nxt, and the
// cross-attention runs on the 2 B slots with image maps into the entries' q and k / v (dd.map_eo, dd.map_ekv).
void decoder_block_entries(Plan& P, const Dims& g, const BlockW& w0, const BlockW& w1, float* xe, float* nxt, const DecBufs& t,
                           const Distinct& dd) {
    const int B = g.B, N = g.N, BN = g.BN, D = g.D, nw = g.nw, heads = g.c.dec_num_heads, hidden = D * g.c.mlp_ratio;
    const int Um = dd.n_ent, Ue = Um * N;
    float *xe0 = xe, *xe1 = xe + (size_t)Ue * D;
    float *o0 = nxt, *o1 = nxt + (size_t)BN * D;
    float *xn = t.xn, *yn = t.yn, *qkv = t.qkv, *qb = t.qb, *kv = t.kv, *att = t.att, *hid = t.hid;
    float *xn1 = P.gin_at(xn, Ue, D), *yn1 = P.gin_at(yn, Ue, D), *att1 = P.gin_at(att, Ue, D);
    P.ln(xe0, w0.n1w, w0.n1b, xn, Ue, D);
    P.ln(xe1, w1.n1w, w1.n1b, xn1, Ue, D);
    P.ln(xe1, w0.nyw, w0.nyb, yn, Ue, D);              // norm_y before the residual goes back into xe (LayerNorm outputs have no site)
    P.ln(xe0, w1.nyw, w1.nyb, yn1, Ue, D);
    P.linear2(xn, xn1, D, w0.qkvw, w1.qkvw, w0.qkvb, w1.qkvb, qkv, P.gin_at(qkv, Ue, 3 * D), 3 * D, Ue, 3 * D, D,
              P.rope_epi(nullptr, 2 * D, N, nw));
    P.attn(qkv, 3 * D, P.gin_col(qkv, D), 3 * D, P.gin_col(qkv, 2 * D), 3 * D, att, D, 2 * Um, heads, N, N, nullptr, att1);
    P.linear2(att, att1, D, w0.projw, w1.projw, w0.projb, w1.projb, xe0, xe1, D, Ue, D, D, P.epi(A3R_EPI_RESID, nullptr), xe0, xe1);
    P.ln(xe0, w0.n2w, w0.n2b, xn, Ue, D);
    P.ln(xe1, w1.n2w, w1.n2b, xn1, Ue, D);
    P.linear2(xn, xn1, D, w0.qw, w1.qw, w0.qb, w1.qb, qb, P.gin_at(qb, Ue, D), D, Ue, D, D, P.rope_epi(nullptr, D, N, nw));
    P.linear2(yn, yn1, D, w0.kvw, w1.kvw, w0.kvb, w1.kvb, kv, P.gin_at(kv, Ue, 2 * D), 2 * D, Ue, 2 * D, D,
              P.rope_epi(nullptr, D, N, nw));
    if (!P.skip()) P.rc = gather_rows(xe, nxt, dd.map_eo, 2 * B, N, D, P.stream);
    att1 = P.gin_at(att, BN, D);
    P.attn(qb, D, kv, 2 * D, P.gin_col(kv, D), 2 * D, att, D, 2 * B, heads, N, N, kv, att1, dd.map_eo, dd.map_ekv);
    P.linear2(att, att1, D, w0.cprojw, w1.cprojw, w0.cprojb, w1.cprojb, o0, o1, D, BN, D, D, P.epi(A3R_EPI_RESID, nullptr), o0, o1);
    xn1 = P.gin_at(xn, BN, D);
    P.ln(o0, w0.n3w, w0.n3b, xn, BN, D);
    P.ln(o1, w1.n3w, w1.n3b, xn1, BN, D);
    float* hid1 = P.gin_at(hid, BN, hidden);
    P.linear2(xn, xn1, D, w0.fc1w, w1.fc1w, w0.fc1b, w1.fc1b, hid, hid1, hidden, BN, hidden, D, P.gin_epi(A3R_EPI_GELU, nullptr));
    P.linear2(hid, hid1, hidden, w0.fc2w, w1.fc2w, w0.fc2b, w1.fc2b, o0, o1, D, BN, D, hidden, P.epi(A3R_EPI_RESID, nullptr), o0, o1);
}

// _decoder (model.py:201-233): decoder_embed, the two decoders with the dec_blocks_pc / zero_convs branch on the depth-prior tokens,
// dec_norm.  Leaves the hooked levels in v.lvl_a / v.lvl_b and the last one in v.dec_last.
void decoder_stage(Plan& P, const Call& k, const Dims& g, Levels& v) {
    a3r_model_s* m = P.m;
    const a3r_model_config& c = g.c;
    const int D = g.D, E = g.E, M2 = g.M2, hidden = D * c.mlp_ratio;
    const int hook_a = c.dec_depth * 2 / 4, hook_b = c.dec_depth * 3 / 4;   // levels 6 and 9 for depth 12
    const DecBufs t = {P.gin_alloc(M2, D), P.gin_alloc(M2, D), P.gin_alloc(M2, 3 * D), P.gin_alloc(M2, D), P.gin_alloc(M2, 2 * D),
                       P.gin_alloc(M2, D), P.gin_alloc(M2, hidden)};      // (a braced list is evaluated in order: so are the allocations)
    float* pc3 = P.gin_scratch(M2, D);
    float* cur = v.fbuf[0];
    float* feat3 = P.gin_scratch(M2, E);
    // Distinct inputs (fh2 GEMM inputs, a3r_model_set_dedup_decoder): a linear that reads one frame's rows runs on the distinct rows
    // with the bias-only epilogue, and a gather-add pass makes the sum the RESID epilogue makes per slot (fp32 addition commutes).
    // The split is the same site over the same set of values.  No buffer is added: the zero-conv's rows z go to v.pc, which holds
    // nothing once the tokens live in pcu, and decoder_embed's to dec_last, which is written after the last block.
    const bool on = P.gf == Form::FH2 && m->dedup_decoder;
    const bool pc_rows = (on && g.d_pd) || g.pp, l0_rows = on && pc_rows && g.d_img;      // (stored priors need the gather-add form)
    // block 0 on entries: level 0 is made for the 2 Um entries only (nothing else reads it)
    const bool entries = l0_rows && k.dd->n_ent > 0;
    // Stored priors (g.pp; with or without the switch): the branch runs on the Mq rows of the priors not found, each zero-conv's fresh rows
    // z_i go to their entries, and the gather-add reads every slot's z_i where it lies, in an entry or among the fresh rows.
    const FrameCall* pp = g.pp;
    const int Mq = g.prior_rows();
    const long zw = (long)g.N * D;                     // words of one z_i in an entry
    // x[s] = z_i[prior of s] + b[mb[s]] (b null: + x[s]) for S row blocks; mz / sz: the priors' rows in v.pc / their sources (pp)
    auto gather_add = [&](int i, const int32_t* mz, const int32_t* sz, const float* b, const int32_t* mb, float* x, int S) {
        if (P.skip()) return;
        if (pp) P.rc = a3r_gather_add_rows_src(reinterpret_cast<const float*>(pp->lay.feat) + i * zw, pp->lay.words_feat, v.pc, sz, b, mb, x, S, g.N, D, P.stream);
        else P.rc = a3r_gather_add_rows(v.pc, mz, b, mb, x, S, g.N, D, P.stream);
    };
    // zero_convs[i] of the depth-prior tokens, added to level x in place (distinct maps without the switch: their tokens are copied
    // to all slots' rows first, so the zero-conv and its epilogue stay as they are)
    auto zero_conv_rows = [&](int i) {
        {
            StoreScope scope(P, pp, P.prior_sites);
            P.linear(P.gin_from(v.pcu, pc3, Mq, D), D, m->zc_w[i], v.pc, D, Mq, D, D, P.epi(A3R_EPI_NONE, m->zc_b[i]));
        }
        if (pp && pp->n_store && !P.skip())
            P.rc = frame_cache_store(nullptr, nullptr, g.B, nullptr, pp->lay, k.dd->uniq_pd, pp->ent, pp->miss, k.dd->n_pd, v.pc, i * zw, zw, P.stream);
    };
    auto add_pc = [&](int i, float* x) {
        if (pc_rows) {
            zero_conv_rows(i);
            gather_add(i, k.dd->map_pd, pp ? pp->src : nullptr, nullptr, nullptr, x, 2 * g.B);
            return;
        }
        if (g.d_pd) copy_rows(P, g, v.pcu, v.pc, k.dd->map_pd, D);
        P.linear(P.gin_from(v.pc, pc3, M2, D), D, m->zc_w[i], x, D, M2, D, D, P.epi(A3R_EPI_RESID, m->zc_b[i], x));
    };
    if (l0_rows) {
        // level 0 = zero_convs[0](tokens of the slot's prior) + decoder_embed(rows of the slot's frame); featu shares cur's memory and
        // is dead once it is split
        P.linear(P.gin_from(v.featu, feat3, g.Mi, E), E, m->de_w, v.dec_last, D, g.Mi, D, E, P.epi(A3R_EPI_NONE, m->de_b));
        zero_conv_rows(0);
        if (entries) gather_add(0, k.dd->ent_pd, pp ? pp->src_ent : nullptr, v.dec_last, k.dd->ent_img, cur, 2 * k.dd->n_ent);
        else gather_add(0, k.dd->map_pd, pp ? pp->src : nullptr, v.dec_last, k.dd->map_img, cur, 2 * g.B);
    } else {
        P.linear(P.gin_from(v.feat, feat3, M2, E), E, m->de_w, cur, D, M2, D, E, P.epi(A3R_EPI_NONE, m->de_b));
        add_pc(0, cur);
    }
    const int npc = n_pc_blocks(c);
    for (int i = 0; i < c.dec_depth; i++) {
        const int level = i + 1;
        float* nxt = level == hook_a ? v.fbuf[2] : level == hook_b ? v.fbuf[3] : cur == v.fbuf[0] ? v.fbuf[1] : v.fbuf[0];
        if (i == 0 && entries) decoder_block_entries(P, g, m->dec1[i], m->dec2[i], cur, nxt, t, *k.dd);
        else decoder_block_pair(P, g, m->dec1[i], m->dec2[i], cur, nxt, t);
        if (i < npc) {   // model.py:223-226
            {
                StoreScope scope(P, pp, P.prior_sites);
                P.rows(Mq);
                P.self_block(m->pc[i], v.pcu, v.pcu, Mq, D, c.dec_num_heads, g.N, g.nw, t.xn, t.qkv, t.att);
                P.mlp(m->pc[i], m->pc[i].n2w, m->pc[i].n2b, v.pcu, Mq, D, hidden, t.xn, t.hid);
                P.rows(M2);
            }
            add_pc(i + 1, nxt);
        }
        if (level == hook_a) v.lvl_a = nxt;
        if (level == hook_b) v.lvl_b = nxt;
        if (level == m->tap_level) tap_copy(P, g, v.tap_lvl, nxt);
        cur = nxt;
    }
    // the prior branch's statistics words: kept with the entries this call filled, completed from those it read
    if (pp && !P.skip()) P.rc = stats_sites_words(pp->stat_words(), pp->lay.cap, pp->ent, pp->miss, k.dd->n_pd, m->stats, P.prior_sites, P.stream);
    P.ln_f32(cur, m->decn_w, m->decn_b, v.dec_last, M2, D);   // model.py:231-232
}

// act_postprocess (dpt_block.py:353-405) of the head of side s: the four hooked levels -> the maps l[0..3] that layer_rn reads, in
// operand form (l[3] is written in it; the others are split: small maps, plain split passes).  Level 0 (enc_norm rows) depends on
// the frame alone: B0 images, the side's distinct ones when its head merges.
// hc (head products): the level-0 ops run on the hc->n_fresh frames of the B0 that are not stored, in the buffers of B0.
void head_levels(Plan& P, const Call& k, const Dims& g, const Levels& v, int s, int B0, const HeadCall* hc, float* (&l)[4]) {
    Arena& ar = P.ar;
    const HeadW& Hd = P.m->head[s];
    const int *ld = g.c.layer_dims, nh = g.nh, nw = g.nw, B = g.B, BN = g.BN, E = g.E, D = g.D;
    const int h3 = (nh + 2 - 3) / 2 + 1, w3 = (nw + 2 - 3) / 2 + 1;
    auto side = [&](const float* x, int cols) { return x ? x + (size_t)s * BN * cols : nullptr; };      // (null in the sizing pass)
    // 1x1 adapters: in fh2 mode a split pass + the fh2 GEMM (5x the exact-fp32 MFMA kernel's rate) instead of a3r_linear
    auto adapter = [&](const float* t, int K, const float* w, const float* b, float* y, int cout, int rows) {
        if (P.gf != Form::FH2) { P.linear_f32(t, K, w, y, cout, rows, cout, K, P.epi(A3R_EPI_NONE, b)); return; }
        ArenaScope scope(ar);                                   // the split is dead once the GEMM is enqueued (stream order)
        float* tg = P.gin_scratch(rows, K);
        P.linear(P.gin_from(t, tg, rows, K), K, w, y, cout, rows, cout, K, P.epi(A3R_EPI_NONE, b));
    };
    // the transposed conv (kernel = stride = ps) behind an adapter: a GEMM whose epilogue scatters the ps x ps pixels
    auto pixshuf = [&](const float* a, const float* w, const float* b, float* y, int ps, int C, int rows) {
        OpEpi e = P.epi(A3R_EPI_PIXSHUF, b);
        e.ps_s = ps; e.ps_h = nh; e.ps_w = nw; e.ps_cout = C;
        P.linear_f32(a, C, w, y, C, rows, ps * ps * C, C, e);
    };
    const size_t BN0 = (size_t)B0 * g.N;
    const int R0 = (hc ? hc->frames() : B0) * g.N;             // rows the level-0 ops run on (one frame's when muted)
    const float* t0 = side(v.feat, E);
    float *a0, *l0;
    {
        StoreScope scope(P, hc, P.head_sites[s]);
        if (B0 < B) {
            float* fu = ar.alloc(BN0 * E);
            if (!P.skip() && !P.mute)
                P.rc = gather_rows(v.feat, fu, hc ? hc->uniq_fresh : k.dd->uniq_side[s], R0 / g.N, g.N, E, P.stream);
            t0 = fu;
        }
        a0 = ar.alloc(BN0 * ld[0]);
        adapter(t0, E, Hd.a0w, Hd.a0b, a0, ld[0], R0);
        l0 = ar.alloc(BN0 * 16 * ld[0]);
        pixshuf(a0, Hd.a0tw, Hd.a0tb, l0, 4, ld[0], R0);
    }
    float* a1 = ar.alloc((size_t)BN * ld[1]);
    adapter(side(v.lvl_a, D), D, Hd.a1w, Hd.a1b, a1, ld[1], BN);
    float* l1 = ar.alloc((size_t)BN * 4 * ld[1]);
    pixshuf(a1, Hd.a1tw, Hd.a1tb, l1, 2, ld[1], BN);
    float* l2 = ar.alloc((size_t)BN * ld[2]);
    adapter(side(v.lvl_b, D), D, Hd.a2w, Hd.a2b, l2, ld[2], BN);
    float* a3 = ar.alloc((size_t)BN * ld[3]);
    adapter(side(v.dec_last, D), D, Hd.a3w, Hd.a3b, a3, ld[3], BN);
    l[3] = P.map_alloc((size_t)B * h3 * w3, ld[3]);
    float* a33 = P.map_twin(a3, BN, ld[3]);
    P.split_map(a3, a33, BN, ld[3]);
    OpEpi e = P.epi(A3R_EPI_NONE, Hd.a3cb);
    e.out_op = 1;
    P.conv(a33, Hd.a3cw, l[3], B, nh, nw, ld[3], ld[3], 2, e);
    l[0] = P.map_twin(l0, BN0 * 16, ld[0]);
    {
        StoreScope scope(P, hc, P.head_sites[s]);
        P.split_map(l0, l[0], (long)R0 * 16, ld[0]);
    }
    l[1] = P.map_twin(l1, (size_t)BN * 4, ld[1]);
    P.split_map(l1, l[1], (long)BN * 4, ld[1]);
    l[2] = P.map_twin(l2, BN, ld[2]);
    P.split_map(l2, l[2], BN, ld[2]);
}

// One DPT head (dpt_head.py:34-66), the one of side s: act_postprocess, scratch.layer_rn, the four fusion blocks, head.0 / .2 / .4
// and the postprocess.  Every map is fp32 with a twin in operand form where a conv reads it (under F32 the map itself).
void head_stage(Plan& P, const Call& k, const Dims& g, const Levels& v, int s) {
    a3r_model_s* m = P.m;
    Arena& ar = P.ar;
    const HeadW& Hd = m->head[s];
    const int *ld = g.c.layer_dims, nh = g.nh, nw = g.nw, B = g.B, H = g.H, W = g.W, BN = g.BN, F = g.F, L = g.L;
    const int h3 = (nh + 2 - 3) / 2 + 1, w3 = (nw + 2 - 3) / 2 + 1;
    const int B0 = k.dd && P.mf == Form::FH2 ? k.dd->n_side[s] : B;
    // (the combine pass folded into refinenet2's 2x up-sample, whose fp32 output only it would read)
    const HeadCall* hc = k.dd && B0 < B ? k.dd->hp[s] : nullptr;
    HeadMerge hmerge = {B0, k.dd ? k.dd->map_side[s] : nullptr, B0 < B && m->dedup_head_fold && !dpt_ref_order(), nullptr, 2 * nh, 2 * nw,
                        hc, s};
    const size_t BN0 = (size_t)B0 * g.N;
    float* l[4];
    head_levels(P, k, g, v, s, B0, hc, l);
    // scratch.layer_rn (no bias): fp32 for the skip connection + pre-activated map form for the first RCU conv
    float* r0 = ar.alloc(BN0 * 16 * F);
    float* r0r3 = P.map_twin(r0, BN0 * 16, F);
    float* r1 = ar.alloc((size_t)BN * 4 * F);
    float* r1r3 = P.map_twin(r1, (size_t)BN * 4, F);
    float* r2 = ar.alloc((size_t)BN * F);
    float* r2r3 = P.map_twin(r2, BN, F);
    float* r3 = ar.alloc((size_t)B * h3 * w3 * F);
    float* r3r3 = P.map_twin(r3, (size_t)B * h3 * w3, F);
    auto rn_epi = [&](float* twin) { OpEpi e = P.epi(A3R_EPI_NONE, nullptr); P.aux(e, twin, true); return e; };
    {
        StoreScope scope(P, hc, P.head_sites[s]);
        P.conv(l[0], Hd.rn[0], r0, hc ? hc->frames() : B0, 4 * nh, 4 * nw, ld[0], F, 1, rn_epi(r0r3));
    }
    P.conv(l[1], Hd.rn[1], r1, B, 2 * nh, 2 * nw, ld[1], F, 1, rn_epi(r1r3));
    P.conv(l[2], Hd.rn[2], r2, B, nh, nw, ld[2], F, 1, rn_epi(r2r3));
    P.conv(l[3], Hd.rn[3], r3, B, h3, w3, ld[3], F, 1, rn_epi(r3r3));
    // refinement (dpt_head.py:57-60)
    float* p4 = fusion_map(P, Hd.ref[3], r3, r3r3, nullptr, nullptr, false, B, h3, w3, F, nh, nw, false);
    float* p3 = fusion_map(P, Hd.ref[2], p4, nullptr, r2, r2r3, true, B, nh, nw, F, 2 * nh, 2 * nw, false);
    float* p2 = fusion_map(P, Hd.ref[1], p3, nullptr, r1, r1r3, true, B, 2 * nh, 2 * nw, F, 4 * nh, 4 * nw, false, nullptr,
                           hmerge.fold ? &hmerge.x0_lo : nullptr);
    float* p13 = fusion_map(P, Hd.ref[0], p2, nullptr, r0, r0r3, true, B, 4 * nh, 4 * nw, F, 8 * nh, 8 * nw, true, B0 < B ? &hmerge : nullptr);
    // the level-0 branch's statistics words: kept with the (entry, side) this call filled, completed from those it read
    if (hc && !P.skip()) P.rc = stats_sites_words(hc->st.side_words(s), hc->st.cap, hc->ent, hc->miss, B0, m->stats, P.head_sites[s], P.stream);
    // head (dpt_block.py:323-330)
    const int Hh = 8 * nh, Wh = 8 * nw;
    float* h0 = ar.alloc((size_t)B * Hh * Wh * (F / 2));
    P.conv(p13, Hd.h0w, h0, B, Hh, Wh, F, F / 2, 1, P.epi(A3R_EPI_NONE, Hd.h0b));
    float* hu3 = P.map_alloc((size_t)B * H * W, F / 2);
    P.up(P.mf, h0, hu3, B, Hh, Wh, F / 2, H, W);
    if (P.mf == Form::FH2 && L == 128) {
        // head.2 (3x3 conv + ReLU), head.4 (1x1 conv 128 -> 4) and the postprocess in ONE launch: the [B H W, 128] map is
        // neither written nor read back (8.4 GB per head and step at 42 pairs), dpt_block.py:323-329 + postprocess.py:10-58
        OpEpi e = P.epi(A3R_EPI_HEAD, Hd.h2b);
        e.head_w = Hd.h4w; e.head_b = Hd.h4b; e.head_conf = k.conf[s];
        P.conv(hu3, Hd.h2w, k.pts[s], B, H, W, F / 2, L, 1, e);
        return;
    }
    float* h2 = ar.alloc((size_t)B * H * W * L);
    P.conv(hu3, Hd.h2w, h2, B, H, W, F / 2, L, 1, P.epi(A3R_EPI_RELU, Hd.h2b));
    if (!P.skip()) P.rc = a3r_head_final(h2, Hd.h4w, Hd.h4b, k.pts[s], k.conf[s], (long)B * H * W, L, P.stream);
}

// a process-wide arithmetic mode (a3r_bf3_set_products, a3r_fh2_set_passes) set to the handle's for the duration of a plan
template <int (*Set)(int)> struct ModeGuard {
    int prev = 0; bool on;
    ModeGuard(bool on_, int v) : on(on_) { if (on) prev = Set(v); }
    ~ModeGuard() { if (on) Set(prev); }
};

// The plan of one call: the persistent buffers, then the stages, each starting from the same arena mark.  The order of the
// allocations and of the sites, both observable ("Where a fused producer or consumer is wired in"), is the order of the
// stage calls here and of the lines inside each stage.
int run_plan(a3r_model_s* m, const Call& k, size_t* peak = nullptr) {
    const Dims g(m->cfg, k);
    const bool dry = k.dry;
    ModeGuard<a3r_bf3_set_products> products_guard(!dry && m->gemm_form != Form::F32, m->products);
    ModeGuard<a3r_fh2_set_passes> passes_guard(!dry && m->gemm_form == Form::FH2, m->fh2_passes);
    Plan P;
    P.m = m; P.stream = k.stream; P.phase = k.phase; P.gf = m->gemm_form; P.mf = m->map_form;
    if (!dry && P.gf == Form::FH2) {
        if (hipMemsetAsync(m->stats, 0, (size_t)a3r_model_s::MAX_SITES * 4, as_stream(k.stream)) != hipSuccess) {
            set_error("a3r_model_forward: clearing the range statistics failed");
            return A3R_EHIP;
        }
        m->last_phase = k.phase;
        m->last_sites = 0;
    }
    struct SitesGuard {      // however the plan returns: how many sites it walked
        a3r_model_s* m; Plan* P; bool on;
        ~SitesGuard() { if (on) m->last_sites = P->site_no < a3r_model_s::MAX_SITES ? P->site_no : a3r_model_s::MAX_SITES; }
    } sites_guard{m, &P, !dry};
    static const bool plain_act = getenv("A3R_BF3_PLAIN_ACT") != nullptr;      // A/B switch: keep every activation in plain rows
    P.pair = P.pair_all = P.gf == Form::BF3 && g.BN % 2 == 0 && !plain_act;
    P.ar = {static_cast<char*>(k.ws), 0, k.ws_bytes, dry, 0};
    Arena& ar = P.ar;
    const int D = g.D, E = g.E, M2 = g.M2;
    if (k.phase == 1) {
        // encoder only: per-frame features for caching.  The reference re-encodes a frame for every pair it appears in; the result
        // does not depend on the pair.
        float* cols = ar.alloc((size_t)g.BN * 768);
        float* cols3 = P.gin_scratch(g.BN, 768);
        encoder_stage(P, k, g, cols, cols3, g.BN, k.feat_out);
        if (peak) *peak = ar.peak;
        return P.rc;
    }
    // ---------------- persistent buffers
    Levels v;
    v.feat = ar.alloc((size_t)M2 * E);
    v.pc = ar.alloc((size_t)M2 * D);
    for (int i = 0; i < 4; i++) v.fbuf[i] = ar.alloc((size_t)M2 * D);
    v.dec_last = ar.alloc((size_t)M2 * D);
    // debug taps: copies of one decoder level and of the point-cloud tokens before their first block
    v.tap_lvl = m->tap_level > 0 ? ar.alloc((size_t)M2 * D) : nullptr;
    v.tap_pc0 = m->tap_level > 0 ? ar.alloc((size_t)M2 * D) : nullptr;
    v.pcu = g.d_pd ? v.fbuf[3] : v.pc;
    v.featu = g.d_img ? v.fbuf[0] : v.feat;
    if (!dry && g.d_img && (v.fbuf[1] != v.fbuf[0] + (size_t)M2 * D || v.fbuf[2] != v.fbuf[1] + (size_t)M2 * D)) {
        set_error("a3r_model_forward: internal: the decoder level buffers are not contiguous");
        return A3R_ESTATE;
    }
    // ---------------- encoder (or the cached features) and the depth-prior embedding, which share the patch columns
    {
        ArenaScope stage(ar);
        const int Mc = k.phase == 2 ? g.Mp : g.Mi > g.Mp ? g.Mi : g.Mp;
        float* cols = ar.alloc((size_t)Mc * 768);
        float* cols3 = P.gin_scratch(Mc, 768);
        if (k.phase == 2) load_features(P, k, g, v.feat);
        else if (const FrameCall* fc = g.d_img ? k.dd->fc : nullptr) {
            // Frames kept across calls: the encoder runs on the images the cache does not hold and leaves their rows in `feat`, idle
            // until the copy below; the exchange pass puts every distinct frame's rows, stored or fresh, into featu and the fresh ones
            // with their images into their entries.  The encoder's sites keep their numbers; their statistics words are completed
            // from the entries' (stats_sites_words).
            {
                StoreScope scope(P, fc, P.enc_sites);
                encoder_stage(P, k, g, cols, cols3, fc->frames() * g.N, v.feat);
            }
            if (!P.skip())
                P.rc = frame_cache_exchange(k.img[0], k.img[1], g.B, fc->keys, fc->lay, k.dd->uniq_img, fc->ent, fc->miss, k.dd->n_img, v.feat,
                                            v.featu, P.stream);
            if (!P.skip() && P.gf == Form::FH2)
                P.rc = stats_sites_words(fc->stat_words(), fc->lay.cap, fc->ent, fc->miss, k.dd->n_img, m->stats, P.enc_sites, P.stream);
            copy_rows(P, g, v.featu, v.feat, k.dd->map_img, E);
        } else {
            encoder_stage(P, k, g, cols, cols3, g.Mi, v.featu);
            if (g.d_img) copy_rows(P, g, v.featu, v.feat, k.dd->map_img, E);
        }
        embed_pc_stage(P, k, g, cols, cols3, v.pcu);
    }
    tap_copy(P, g, v.tap_pc0, v.pc);
    // ---------------- decoder
    {
        ArenaScope stage(ar);
        decoder_stage(P, k, g, v);
    }
    if (!dry) {
        m->taps.clear();
        m->taps["feat"] = {v.feat, (size_t)M2 * E};
        m->taps["hook_a"] = {v.lvl_a, (size_t)M2 * D};
        m->taps["hook_b"] = {v.lvl_b, (size_t)M2 * D};
        m->taps["dec_last"] = {v.dec_last, (size_t)M2 * D};
        if (v.tap_lvl) { m->taps["level"] = {v.tap_lvl, (size_t)M2 * D}; m->taps["pc0"] = {v.tap_pc0, (size_t)M2 * D}; }
    }
    // ---------------- DPT heads, one per view
    for (int s = 0; s < 2; s++) {
        ArenaScope stage(ar);
        head_stage(P, k, g, v, s);
    }
    if (peak) *peak = ar.peak;
    return P.rc;
}
}  // namespace

// ---- the distinct inputs of one call: key, representative and verify kernels, ONE read-back (with one stream synchronise, at the
// start of the call), the host planner (dedup.h, plan_call) and one upload of its lists.  a1 / a2: the items of the first kind, words_a words each --
// the images of a forward (encode: they are merged for the encoder too), the cached features of a decode call, which only the heads'
// level-0 branch merges (null: a decode call that does not look at them).  *use = false: run the plain plan (switched off, parity taps
// on, a batch beyond DEDUP_MAX_SLOTS, nothing to merge, or a slot that differs from its representative: a key collision).
namespace {
// pinned host words: rep + flag + the frame cache's answer for the 2 B image slots (B <= FC_MAX_PAIRS) + the prior storage's for
// the 2 B pred_depth slots | the lists (dedup.h, CallLists)
constexpr size_t DD_HOST_LIST = (DEDUP_REP_INTS + 4 * FC_MAX_PAIRS + 63) / 64 * 64;
constexpr size_t DD_REP_OFF = DEDUP_KEY_BYTES;                     // device bytes: keys | rep + flag + answer | the lists
constexpr size_t DD_LIST_OFF = DD_REP_OFF + DD_HOST_LIST * 4;
constexpr size_t DD_DEV_BYTES = DD_LIST_OFF + sizeof(CallLists);
static_assert(FC_STAT_WORDS == a3r_model_s::MAX_SITES, "an entry stores one word per site");

// The storage of the frame cache as entries of this resolution (dedup.h); a change of resolution empties the table
FrameCacheLayout frame_cache_at(a3r_model_s* m, int H, int W) {
    const FrameCacheLayout lay = frame_cache_layout(m->fc.buf, m->fc.bytes, 3L * H * W, (long)(H / 16) * (W / 16) * m->cfg.enc_embed_dim);
    if (H != m->fc_H || W != m->fc_W || lay.cap != m->fc_table.cap) {
        m->reset_frames(lay.cap);
        m->pd_table.reset(0);
        m->fc_H = H;
        m->fc_W = W;
    }
    return lay;
}
// Words of an entry of the products storage at this resolution: the pred_depth map, and the rows z_0 .. z_n of the zero-convs
long prior_words_map(int H, int W) { return 3L * H * W; }
long prior_words_rows(const a3r_model_config& c, int H, int W) { return (long)(n_pc_blocks(c) + 1) * (H / 16) * (W / 16) * c.dec_embed_dim; }
// The products storage as `cap` entries (the frame cache's count, after frame_cache_at) of this resolution; cap 0 in the answer:
// it has no room for that many and is not used
FrameCacheLayout prior_store_at(a3r_model_s* m, int H, int W, int cap) {
    const long wm = prior_words_map(H, W), wr = prior_words_rows(m->cfg, H, W);
    const size_t need = (size_t)cap * frame_cache_entry_bytes(wm, wr);
    const FrameCacheLayout lay = frame_cache_layout(m->fp.buf && m->fp.bytes >= need ? m->fp.buf : nullptr, need, wm, wr);
    if (lay.cap != m->pd_table.cap) m->pd_table.reset(lay.cap);
    return lay;
}

// Words of one r0 / c block of the head products at this resolution: [16 N, F]
long head_words(const a3r_model_config& c, int H, int W) { return 16L * (H / 16) * (W / 16) * c.feature_dim; }

int find_distinct(a3r_model_s* m, const float* a1, const float* a2, long words_a, bool encode, const float* pd1, const float* pd2, int B,
                  int H, int W, void* stream, Distinct* d, bool* use, FrameCall* cc = nullptr, FrameCall* pc = nullptr,
                  HeadCall* hc = nullptr) {
    *use = false;
    m->last = CallPlan(B);
    if (m->dedup_mode == 0 || m->tap_level > 0 || 4 * B > DEDUP_MAX_SLOTS) return A3R_OK;
    if (!m->dd_dev) A3R_HIP(hipMalloc(&m->dd_dev, DD_DEV_BYTES));
    if (!m->dd_host) A3R_HIP(hipHostMalloc(reinterpret_cast<void**>(&m->dd_host), DD_HOST_LIST * sizeof(int32_t) + sizeof(CallLists), hipHostMallocDefault));
    char* dev = static_cast<char*>(m->dd_dev);
    int32_t* rep_dev = reinterpret_cast<int32_t*>(dev + DD_REP_OFF);
    const bool first_kind = a1 && a2;
    const int S = 2 * B, first = first_kind ? 0 : S;
    if (int rc = dedup_find(a1, a2, pd1, pd2, B, words_a, 3L * H * W, first, m->dedup_mode == 2, dev, rep_dev, stream)) return rc;
    hipStream_t st = as_stream(stream);
    const a3r_model_config& c = m->cfg;
    // frames kept across calls: the lookup's answer for the 2 B image slots follows the flag in the same read-back
    const bool cached = cc && m->fc.buf && encode && first_kind && B <= FC_MAX_PAIRS;
    if (cached) {
        cc->lay = frame_cache_at(m, H, W);
        cc->keys = dev;
        A3R_CHECK_ARG(cc->lay.cap > 0, "a3r_model_forward: the frame cache's storage (%zu bytes) is smaller than one entry at %d x %d (%zu bytes)",
                      m->fc.bytes, H, W, frame_cache_entry_bytes(cc->lay.words_img, cc->lay.words_feat));
        if (int rc = frame_cache_lookup(a1, a2, B, dev, rep_dev, cc->lay, m->fc_table.mask(), rep_dev + 2 * S + 1, stream)) return rc;
    }
    // priors kept across calls: the same lookup on the pred_depth slots (keys and representatives of the second kind), its answer
    // behind the images'.  They ride on the frame cache (as many entries, dropped and bypassed with it) and feed the decoder's
    // gather-add form, whatever a3r_model_set_dedup_decoder says: a handle with that switch off reads the same stored words.
    bool stored_pd = cached && pc && m->fp.buf && m->gemm_form == Form::FH2;
    if (stored_pd) {
        pc->lay = prior_store_at(m, H, W, cc->lay.cap);
        pc->keys = dev + (size_t)S * 16;
        stored_pd = pc->lay.cap > 0;
        if (stored_pd)
            if (int rc = frame_cache_lookup(pd1, pd2, B, pc->keys, rep_dev + S, pc->lay, m->pd_table.mask(), rep_dev + 3 * S + 1, stream)) return rc;
    }
    // head products kept across calls: no lookup of their own, a storage with room for every entry of the frame cache
    HeadStore hst = head_store_layout(nullptr, 0, 0);
    if (cached && hc && m->hp.buf) {
        const long words = head_words(c, H, W);
        hst = head_store_layout(m->hp.bytes >= (size_t)cc->lay.cap * head_products_entry_bytes(words) ? m->hp.buf : nullptr, cc->lay.cap, words);
    }
    A3R_HIP(hipMemcpyAsync(m->dd_host, rep_dev, (size_t)(2 * S + 1 + (cached ? S : 0) + (stored_pd ? S : 0)) * sizeof(int32_t),
                           hipMemcpyDeviceToHost, st));
    A3R_HIP(hipStreamSynchronize(st));
    const int32_t* rep = m->dd_host;
    const CallInputs in = {rep, rep[2 * S], cached ? rep + 2 * S + 1 : nullptr, stored_pd ? rep + 3 * S + 1 : nullptr, B, H, W,
                           c.enc_embed_dim, c.dec_embed_dim, c.feature_dim, c.layer_dims[0], encode, first_kind, m->dedup_head != 0,
                           m->dedup_decoder != 0, m->gemm_form == Form::FH2, m->map_form == Form::FH2, attention_fh2_takes_maps(),
                           hst.cap > 0};
    CallLists& host = *reinterpret_cast<CallLists*>(m->dd_host + DD_HOST_LIST);
    const CallPlan p = m->last = plan_call(in, m->fc_table, m->pd_table, m->hp_bits, host);
    if (p.drop) m->drop_stored();
    if (!p.use) return A3R_OK;
    A3R_HIP(hipMemcpyAsync(dev + DD_LIST_OFF, &host, sizeof(CallLists), hipMemcpyHostToDevice, st));
    const CallLists* L = reinterpret_cast<const CallLists*>(dev + DD_LIST_OFF);      // (the device's: its members are device addresses)
    *d = {p.n_img, p.n_pd, L->uniq_img, L->map_img, L->uniq_pd, L->map_pd, {p.n_side[0], p.n_side[1]}, {L->uniq_side, L->uniq_side + B},
          {L->map_side, L->map_side + B}, p.n_ent, L->ent_img, L->ent_pd, L->map_eo, L->map_ekv};
    if (p.fc) {
        static_cast<StoreCall&>(*cc) = {p.fc_fresh, p.fc_store, L->fc_fresh, L->fc_ent, L->fc_miss, nullptr};
        cc->src_ent = nullptr;
        d->fc = cc;
    }
    if (p.pd) {
        static_cast<StoreCall&>(*pc) = {p.pd_fresh, p.pd_store, L->pd_fresh, L->pd_ent, L->pd_miss, L->pd_src};
        pc->src_ent = L->pd_src_ent;
        d->pp = pc;
    }
    for (int s = 0; s < 2; s++)
        if (p.hp[s]) {
            const int off = s * B;
            static_cast<StoreCall&>(hc[s]) = {p.hp_fresh[s], p.hp_store[s], L->hp_fresh + off, L->hp_ent + off, L->hp_miss + off, L->hp_src + off};
            hc[s].st = hst;
            d->hp[s] = &hc[s];
        }
    *use = true;
    return A3R_OK;
}

// the sizing pass of phase `phase` with the distinct counts d (or none)
size_t plan_peak(a3r_model_s* m, int phase, int B, int H, int W, const Distinct* d) {
    Call k;
    k.phase = phase; k.B = B; k.H = H; k.W = W;
    k.dry = true;
    k.dd = d;
    size_t peak = 0;
    run_plan(m, k, &peak);
    return peak;
}

// what every entry point that launches a plan checks first
int check_forward_args(a3r_model_t m, int B, int H, int W, const void* workspace, const char* who) {
    A3R_CHECK_ARG(m, "%s: null handle", who);
    if (!m->finalized) {
        set_error("%s: a3r_model_finalize has not been called", who);
        return A3R_ESTATE;
    }
    A3R_CHECK_ARG(workspace, "%s: null workspace", who);
    A3R_CHECK_ARG(B > 0, "%s: batch must be positive", who);
    A3R_CHECK_ARG(H > 0 && H % 16 == 0, "Input image height (%d) is not a multiple of patch size (16).", H);
    A3R_CHECK_ARG(W > 0 && W % 16 == 0, "Input image width (%d) is not a multiple of patch size (16).", W);
    A3R_CHECK_ARG(H / 16 < a3r_model_s::MAX_POS && W / 16 < a3r_model_s::MAX_POS, "%s: image too large for the RoPE table", who);
    A3R_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    return A3R_OK;
}
}  // namespace

extern "C" size_t a3r_model_workspace_bytes(a3r_model_t m, int B, int H, int W) {
    if (!m || B <= 0 || H <= 0 || W <= 0 || H % 16 || W % 16) return 0;
    // the largest of the plain plan and the plans on distinct inputs: those only shrink stages and reuse idle buffers, largest with
    // one duplicate (2 B - 1 distinct), of the depth priors alone or of both kinds; and the heads' merged level-0 branch at the
    // largest number of distinct frames a side is admitted with (head_merge_fits: its buffers grow with that number)
    int u_max = B - 1;
    const a3r_model_config& c = m->cfg;
    while (u_max > 0 && !head_merge_fits(c.enc_embed_dim, c.feature_dim, c.layer_dims[0], (H / 16) * (W / 16), B, u_max)) u_max--;
    const int u_side = u_max > 0 && m->map_form == Form::FH2 ? u_max : B;
    const Distinct cases[4] = {distinct_counts(2 * B, 2 * B, B), distinct_counts(2 * B, 2 * B - 1, B), distinct_counts(2 * B - 1, 2 * B - 1, B),
                               distinct_counts(2 * B, 2 * B, u_side)};
    size_t need = 0;
    for (const Distinct& d : cases) need = std::max(need, plan_peak(m, 0, B, H, W, &d));
    return need;
}

extern "C" int a3r_model_forward(a3r_model_t m, const float* img1, const float* img2, const float* pd1, const float* pd2,
                                 int B, int H, int W, float* pts1, float* conf1, float* pts2, float* conf2, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args(m, B, H, W, workspace, "a3r_model_forward")) return rc;
    A3R_CHECK_ARG(img1 && img2 && pd1 && pd2 && pts1 && conf1 && pts2 && conf2, "a3r_model_forward: null pointer");
    const size_t need_bytes = a3r_model_workspace_bytes(m, B, H, W);
    A3R_CHECK_ARG(workspace_bytes >= need_bytes, "a3r_model_forward: workspace too small (%zu < %zu)", workspace_bytes, need_bytes);
    Distinct d;
    bool merge = false;
    FrameCall cc, pc;
    HeadCall hc[2];
    int rc = find_distinct(m, img1, img2, 3L * H * W, true, pd1, pd2, B, H, W, stream, &d, &merge, &cc, &pc, hc);
    Call k;
    k.phase = 0; k.B = B; k.H = H; k.W = W;
    k.img[0] = img1; k.img[1] = img2; k.pd[0] = pd1; k.pd[1] = pd2;
    k.pts[0] = pts1; k.pts[1] = pts2; k.conf[0] = conf1; k.conf[1] = conf2;
    k.ws = workspace; k.ws_bytes = workspace_bytes; k.stream = stream;
    k.dd = merge ? &d : nullptr;
    if (!rc) rc = run_plan(m, k);
    if (rc) m->drop_stored();          // entries this call was to fill may not have been written
    return rc;
}

extern "C" size_t a3r_model_encode_workspace_bytes(a3r_model_t m, int B, int H, int W) {
    if (!m || B <= 0 || H <= 0 || W <= 0 || H % 16 || W % 16) return 0;
    return plan_peak(m, 1, B, H, W, nullptr);
}

extern "C" int a3r_model_encode(a3r_model_t m, const float* img, int B, int H, int W, float* feat_out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args(m, B, H, W, workspace, "a3r_model_encode")) return rc;
    A3R_CHECK_ARG(img && feat_out, "a3r_model_encode: null pointer");
    const size_t need_bytes = a3r_model_encode_workspace_bytes(m, B, H, W);
    A3R_CHECK_ARG(workspace_bytes >= need_bytes, "a3r_model_encode: workspace too small (%zu < %zu)", workspace_bytes, need_bytes);
    Call k;
    k.phase = 1; k.B = B; k.H = H; k.W = W;
    k.img[0] = img; k.feat_out = feat_out;
    k.ws = workspace; k.ws_bytes = workspace_bytes; k.stream = stream;
    return run_plan(m, k);
}

extern "C" int a3r_model_decode(a3r_model_t m, const float* feat1, const float* feat2, const float* pd1, const float* pd2, int B,
                                int H, int W, float* pts1, float* conf1, float* pts2, float* conf2, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args(m, B, H, W, workspace, "a3r_model_decode")) return rc;
    A3R_CHECK_ARG(feat1 && feat2 && pd1 && pd2 && pts1 && conf1 && pts2 && conf2, "a3r_model_decode: null pointer");
    const size_t need_bytes = a3r_model_workspace_bytes(m, B, H, W);      // the whole-forward plan bounds the decode plan
    A3R_CHECK_ARG(workspace_bytes >= need_bytes, "a3r_model_decode: workspace too small (%zu < %zu)", workspace_bytes, need_bytes);
    Distinct d;
    bool merge = false;
    // (the features are only looked at for the heads' level-0 branch: fh2 maps, a3r_model_set_dedup_head)
    const bool look = m->dedup_head && m->map_form == Form::FH2;
    const long words_f = (long)(H / 16) * (W / 16) * m->cfg.enc_embed_dim;
    if (int rc = find_distinct(m, look ? feat1 : nullptr, look ? feat2 : nullptr, words_f, false, pd1, pd2, B, H, W, stream, &d, &merge))
        return rc;
    Call k;
    k.phase = 2; k.B = B; k.H = H; k.W = W;
    k.feat_in[0] = feat1; k.feat_in[1] = feat2; k.pd[0] = pd1; k.pd[1] = pd2;
    k.pts[0] = pts1; k.pts[1] = pts2; k.conf[0] = conf1; k.conf[1] = conf2;
    k.ws = workspace; k.ws_bytes = workspace_bytes; k.stream = stream;
    k.dd = merge ? &d : nullptr;
    return run_plan(m, k);
}
extern "C" int a3r_model_set_dedup(a3r_model_t m, int mode) {
    A3R_CHECK_ARG(m && mode >= 0 && mode <= 2, "a3r_model_set_dedup: mode must be 0 (off), 1 (on) or 2 (constant key)");
    if (mode != m->dedup_mode) m->drop_stored();      // (stored keys are those of the mode they were made in)
    m->dedup_mode = mode;
    return A3R_OK;
}

extern "C" size_t a3r_model_frame_cache_bytes(a3r_model_t m, int H, int W, int frames) {
    if (!m || H <= 0 || W <= 0 || H % 16 || W % 16 || frames <= 0 || frames > FC_MAX_ENTRIES) return 0;
    return (size_t)frames * frame_cache_entry_bytes(3L * H * W, (long)(H / 16) * (W / 16) * m->cfg.enc_embed_dim);
}

extern "C" int a3r_model_set_frame_cache(a3r_model_t m, void* buf, size_t bytes) {
    A3R_CHECK_ARG(m, "a3r_model_set_frame_cache: null handle");
    m->reset_frames(0);
    m->pd_table.reset(0);
    m->fc_H = m->fc_W = 0;
    if (int rc = m->fc.set(buf, bytes, "a3r_model_set_frame_cache")) return rc;
    const size_t least = a3r_model_frame_cache_bytes(m, 16, 16, 1);
    if (!m->fc.buf || bytes >= least) return A3R_OK;
    m->fc = {};
    set_error("a3r_model_set_frame_cache: storage too small for one entry of the smallest image (%zu < %zu)", bytes, least);
    return A3R_EINVAL;
}

extern "C" int a3r_model_last_frame_cache(a3r_model_t m, int* hits, int* misses, int* evictions) {
    A3R_CHECK_ARG(m && hits && misses && evictions, "a3r_model_last_frame_cache: null argument");
    *hits = m->last.fc_n[0];
    *misses = m->last.fc_n[1];
    *evictions = m->last.fc_n[2];
    return A3R_OK;
}

extern "C" size_t a3r_model_frame_products_bytes(a3r_model_t m, int H, int W, int frames) {
    if (!m || H <= 0 || W <= 0 || H % 16 || W % 16 || frames <= 0 || frames > FC_MAX_ENTRIES) return 0;
    return (size_t)frames * frame_cache_entry_bytes(prior_words_map(H, W), prior_words_rows(m->cfg, H, W));
}

extern "C" int a3r_model_set_frame_products(a3r_model_t m, void* buf, size_t bytes) {
    A3R_CHECK_ARG(m, "a3r_model_set_frame_products: null handle");
    m->pd_table.reset(0);
    return m->fp.set(buf, bytes, "a3r_model_set_frame_products");
}

extern "C" int a3r_model_last_frame_products(a3r_model_t m, int* hits, int* misses, int* evictions) {
    A3R_CHECK_ARG(m && hits && misses && evictions, "a3r_model_last_frame_products: null argument");
    *hits = m->last.pd_n[0];
    *misses = m->last.pd_n[1];
    *evictions = m->last.pd_n[2];
    return A3R_OK;
}

extern "C" size_t a3r_model_head_products_bytes(a3r_model_t m, int H, int W, int frames) {
    if (!m || H <= 0 || W <= 0 || H % 16 || W % 16 || frames <= 0 || frames > FC_MAX_ENTRIES) return 0;
    return (size_t)frames * head_products_entry_bytes(head_words(m->cfg, H, W));
}

extern "C" int a3r_model_set_head_products(a3r_model_t m, void* buf, size_t bytes) {
    A3R_CHECK_ARG(m, "a3r_model_set_head_products: null handle");
    m->hp_bits.flush();
    return m->hp.set(buf, bytes, "a3r_model_set_head_products");
}

extern "C" int a3r_model_last_head_products(a3r_model_t m, int* hits, int* misses) {
    A3R_CHECK_ARG(m && hits && misses, "a3r_model_last_head_products: null argument");
    for (int s = 0; s < 2; s++) {
        hits[s] = m->last.hp_hits(s);
        misses[s] = m->last.hp_misses(s);
    }
    return A3R_OK;
}

extern "C" int a3r_model_set_dedup_head(a3r_model_t m, int on) {
    A3R_CHECK_ARG(m, "a3r_model_set_dedup_head: null handle");
    m->dedup_head = on != 0;
    return A3R_OK;
}

extern "C" int a3r_model_set_dedup_decoder(a3r_model_t m, int on) {
    A3R_CHECK_ARG(m, "a3r_model_set_dedup_decoder: null handle");
    m->dedup_decoder = on != 0;
    return A3R_OK;
}

extern "C" int a3r_model_last_dedup_entries(a3r_model_t m, int* u1, int* u2, int* merged) {
    A3R_CHECK_ARG(m && u1 && u2 && merged, "a3r_model_last_dedup_entries: null argument");
    *u1 = m->last.ent_unique[0];
    *u2 = m->last.ent_unique[1];
    *merged = m->last.n_ent > 0;
    return A3R_OK;
}

extern "C" int a3r_model_last_dedup_sides(a3r_model_t m, int* u1, int* u2, int* merged1, int* merged2) {
    A3R_CHECK_ARG(m && u1 && u2 && merged1 && merged2, "a3r_model_last_dedup_sides: null argument");
    *u1 = m->last.side_unique[0];
    *u2 = m->last.side_unique[1];
    *merged1 = m->last.side_merged[0];
    *merged2 = m->last.side_merged[1];
    return A3R_OK;
}

extern "C" int a3r_model_last_dedup(a3r_model_t m, int* n_img_unique, int* n_pd_unique, int* fell_back) {
    A3R_CHECK_ARG(m && n_img_unique && n_pd_unique && fell_back, "a3r_model_last_dedup: null argument");
    *n_img_unique = m->last.n_img;
    *n_pd_unique = m->last.n_pd;
    *fell_back = m->last.fell_back;
    return A3R_OK;
}

extern "C" int a3r_model_set_tap_level(a3r_model_t m, int level) {
    A3R_CHECK_ARG(m && level >= 0 && level <= m->cfg.dec_depth, "a3r_model_set_tap_level: level must be in 0..dec_depth");
    m->tap_level = level;
    return A3R_OK;
}

extern "C" int a3r_model_tap(a3r_model_t m, const char* name, const float** ptr, size_t* count) {
    A3R_CHECK_ARG(m && name && ptr && count, "a3r_model_tap: null argument");
    auto it = m->taps.find(name);
    A3R_CHECK_ARG(it != m->taps.end(), "a3r_model_tap: unknown tap '%s' (run a forward first)", name);
    *ptr = it->second.first;
    *count = it->second.second;
    return A3R_OK;
}

// ------------------------------------------------------------------------------------------- fh2 range control
extern "C" int a3r_model_range_check(a3r_model_t m, void* stream, int* n_adjusted, int* n_nonfinite) {
    A3R_CHECK_ARG(m && n_adjusted && n_nonfinite, "a3r_model_range_check: null argument");
    *n_adjusted = 0;
    *n_nonfinite = 0;
    if (m->gemm_form != Form::FH2 || m->last_phase < 0 || m->last_sites <= 0) return A3R_OK;     // fp32-range modes / nothing ran
    std::vector<unsigned> st((size_t)m->last_sites);
    A3R_HIP(hipMemcpyAsync(st.data(), m->stats, st.size() * 4, hipMemcpyDeviceToHost, as_stream(stream)));
    A3R_HIP(hipStreamSynchronize(as_stream(stream)));
    std::vector<float>& sc = m->site_scale[m->last_phase];
    if (sc.size() < st.size()) sc.resize(st.size(), 1.f);
    for (size_t i = 0; i < st.size(); i++) {
        float stored;                                        // max |scale * x| the site wrote
        static_assert(sizeof(float) == sizeof(unsigned), "bit pattern");
        memcpy(&stored, &st[i], 4);
        if (st[i] == 0) continue;                            // an all-zero tensor (or a site that did not run) says nothing
        if (!std::isfinite(stored)) { (*n_nonfinite)++; continue; }
        if (stored >= 0.25f && stored <= 32768.f) continue;  // [2^-2, 2^15]: fp32-grade (fh2.h)
        // new scale: the power of two that puts max |x| = stored / scale into [2^11, 2^12)
        int e;
        std::frexp(stored / sc[i], &e);                      // = f 2^e, f in [0.5, 1)   (the division by a power of two is exact)
        int k = 12 - e;
        k = k < -40 ? -40 : k > 40 ? 40 : k;              // (products of two scales stay far inside fp32)
        sc[i] = std::ldexp(1.f, k);
        (*n_adjusted)++;
    }
    // a call that has to be repeated stored nothing worth keeping, and stored rows do not outlive the scales they were made with
    if (*n_adjusted || *n_nonfinite) m->drop_stored();
    return A3R_OK;
}

extern "C" int a3r_model_range_stats(a3r_model_t m, void* stream, float* stored_absmax, int capacity, int* n_sites) {
    A3R_CHECK_ARG(m && n_sites && (stored_absmax || capacity == 0), "a3r_model_range_stats: bad argument");
    *n_sites = m->last_sites;
    const int n = capacity < m->last_sites ? capacity : m->last_sites;
    if (n <= 0 || !m->stats) return A3R_OK;
    A3R_HIP(hipMemcpyAsync(stored_absmax, m->stats, (size_t)n * 4, hipMemcpyDeviceToHost, as_stream(stream)));
    A3R_HIP(hipStreamSynchronize(as_stream(stream)));
    return A3R_OK;
}

extern "C" int a3r_model_range_scales(a3r_model_t m, int phase, float* scales, int capacity, int* n_sites) {
    A3R_CHECK_ARG(m && n_sites && phase >= 0 && phase < 3 && (scales || capacity == 0), "a3r_model_range_scales: bad argument");
    const std::vector<float>& sc = m->site_scale[phase];
    *n_sites = (int)sc.size();
    for (int i = 0; i < capacity && i < (int)sc.size(); i++) scales[i] = sc[i];
    return A3R_OK;
}

extern "C" int a3r_model_reset_ranges(a3r_model_t m) {
    A3R_CHECK_ARG(m, "a3r_model_reset_ranges: null handle");
    for (auto& v : m->site_scale) v.clear();
    m->drop_stored();
    return A3R_OK;
}
