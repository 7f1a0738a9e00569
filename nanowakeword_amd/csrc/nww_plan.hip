// nww_plan.hip - the plan knobs and the launch plans nww_finalize builds from the loaded weights: plan helpers, one planner per head.
#include "nww_internal.h"
#include "bc_chain.h"

const Knobs& nww_knobs() {
    static const Knobs k = [] {
        auto env = [](const char* name, int d) { const char* e = getenv(name); return e ? atoi(e) : d; };
        Knobs r;
        r.trunk = env("NWW_TRUNK", 1); r.conv_mfma = env("NWW_CONV_MFMA", 1); r.conv3_x3 = env("NWW_CONV3_X3", 1);
        r.gemm_x3 = env("NWW_GEMM_X3", 1); r.lin_x3 = env("NWW_LIN_X3", 1); r.ffn_fused = env("NWW_FFN_FUSED", 1);
        r.attn_fused = env("NWW_ATTN_FUSED", 1); r.merge_fused = env("NWW_MERGE_FUSED", 1); r.qn_fused = env("NWW_QN_FUSED", 1); r.raw_fused = env("NWW_RAW_FUSED", 1); r.conv2s_x3 = env("NWW_CONV2S_X3", 1); r.rnn_ih_fused = env("NWW_RNN_IH_FUSED", 1); r.mha_mfma = env("NWW_MHA_MFMA", 1); r.bc_front = env("NWW_BC_FRONT", 1);
        r.bc_chain = env("NWW_BC_CHAIN", 1); r.tail = env("NWW_TAIL", 1); r.stream_inc = env("NWW_STREAM_INC", 3); r.rec_shared = env("NWW_REC_SHARED", 1); r.gemm_pp = env("NWW_GEMM_PP", 1);
        r.f16_range_log2 = env("NWW_F16_RANGE_LOG2", 16);
        return r;
    }();
    return k;
}
double f16_range_factor() { return std::ldexp(1.0, nww_knobs().f16_range_log2); }      // plan_host.h: F16Range's window, from its knob

// ------------------------------------------------------------------------------------------ plan helpers
namespace {

// what src() / dst() take beside a workspace buffer's index (>= 0): the head input x, the embedding, the classifier's hidden row, the logits
enum : int { BUF_X = -1, BUF_EMB = -2, BUF_HID = -3, BUF_LOGITS = -4, BUF_NONE = 99 };

struct PlanCtx {
    nww_handle* h;
    const float* W(const std::string& k) const {
        auto it = h->tensors.find(k);
        return it == h->tensors.end() || !it->second.loaded ? nullptr : h->d_weights + it->second.dev_off;
    }
    void need(int buf, size_t floats_per_clip) {
        if (h->buf_per_clip[buf] < floats_per_clip) h->buf_per_clip[buf] = floats_per_clip;
    }
    void add(const std::string& name, std::function<hipError_t(Run&)> fn) { h->plan.push_back({name, std::move(fn)}); }
    void pop_last() { if (!h->plan.empty()) h->plan.pop_back(); }        // a step just planned is re-planned in another form
    // the head's last Linear (-> embedding), deferred so that it can be fused with the classifier into one launch
    std::string tail_name; int tail_in = BUF_NONE, tail_K = 0; const float *tail_W = nullptr, *tail_b = nullptr;
    // DNN: LayerNorm1 + blocks run inside the tail's launch (TailArgs::ln0_w); mid[i]: block i's fcn_layer weight, bias, layer_norm weight, bias
    struct DnnBody { bool on = false; const float *ln0_w = nullptr, *ln0_b = nullptr; int n_mid = 0; const float* mid[4][4] = {}; } dnn;
    // Device memory for the packed weight images of one step (a single image, a pair or a list), all or nothing: pack() allocates an
    // image and runs the pack launch handed to it (on own_stream, nothing waits) - nullptr and nothing held if either fails -,
    // commit() hands the images to the handle, which frees them at nww_destroy, and what was not committed is freed when the scope ends
    struct Packs {
        nww_handle* h;
        std::vector<void*> held;
        explicit Packs(PlanCtx& p) : h(p.h) {}
        Packs(const Packs&) = delete;
        ~Packs() { for (void* d : held) (void)hipFree(d); }
        void* alloc(size_t bytes) { void* d = nullptr; if (hipMalloc(&d, bytes) != hipSuccess) return nullptr; held.push_back(d); return d; }
        template <class Launch> void* pack(size_t bytes, Launch&& launch) {      // launch(void* image) -> hipError_t
            void* d = alloc(bytes);
            if (d && launch(d) != hipSuccess) { held.pop_back(); (void)hipFree(d); d = nullptr; }
            return d;
        }
        void commit() { h->packed_weights.insert(h->packed_weights.end(), held.begin(), held.end()); held.clear(); }
    };
    // a single image: kept if it was built, else nullptr
    template <class Launch> void* pack_one(size_t bytes, Launch&& launch) { Packs pk(*this); void* d = pk.pack(bytes, launch); pk.commit(); return d; }
};

// ---- two-term binary16 arithmetic (NWW_ARITH_F16X3): plan-time bounds and power-of-two scales (the arithmetic itself: plan_host.h)
// n values of the weight arena at device pointer d, read from the arena's host image (nww_handle::h_weights; no HIP call); an absent
// tensor (d = nullptr: a bias or BatchNorm a layer does not have) reads as zeros.  A pointer that is not the arena's is a programming
// error: nww_finalize fails with it
std::vector<float> f16_fetch(nww_handle* h, const float* d, size_t n) {
    if (!d) return std::vector<float>(n, 0.0f);
    const uintptr_t a = reinterpret_cast<uintptr_t>(d), a0 = reinterpret_cast<uintptr_t>(h->d_weights);
    const size_t size = h->h_weights.size(), off = a >= a0 ? (size_t)(a - a0) / sizeof(float) : size + 1;
    if ((a - a0) % sizeof(float) != 0 || off > size || n > size - off) {
        if (h->plan_error.empty()) h->plan_error = "plan-time read of " + std::to_string(n) + " weights outside the weight arena";
        return std::vector<float>(n, 0.0f);
    }
    return std::vector<float>(h->h_weights.begin() + off, h->h_weights.begin() + off + n);
}
// |LayerNorm(x)_k| <= sqrt(D) |w_k| + |b_k| whatever x holds: a bound on a LayerNorm's output from its weights alone
double f16_ln_bound(nww_handle* h, const float* w, const float* b, int D) {
    const auto hw = f16_fetch(h, w, D), hb = f16_fetch(h, b, D);
    double bound = 0.0;
    for (int k = 0; k < D; ++k) bound = std::fmax(bound, std::sqrt((double)D) * std::fabs((double)hw[k]) + std::fabs((double)hb[k]));
    return bound;
}
bool f16_all_nonneg(nww_handle* h, const float* d, int n) {      // folded-BN factors: max-pool commutes with BN + ReLU when none is negative
    for (float v : f16_fetch(h, d, n)) if (!(v >= 0.0f)) return false;
    return true;
}

const F16Range F16_FEATURES{NWW_F16_FEATURE_BOUND, 32.0};

// a step's input / output: one of the named selectors above or a workspace buffer
inline const float* src(Run& r, int id) { return id == BUF_X ? r.x : id == BUF_EMB ? r.emb : id == BUF_HID ? r.hid : r.buf[id]; }
inline float* dst(Run& r, int id) { return id == BUF_EMB ? r.emb : id == BUF_HID ? r.hid : id == BUF_LOGITS ? r.logits : r.buf[id]; }

struct GemmOpts {
    const float *alpha = nullptr, *beta = nullptr;       // a folded BatchNorm behind the bias
    int res_id = BUF_NONE; float rscale = 1.f;           // out = res + rscale act(...)
    bool* a_blocked_inout = nullptr;                     // in: the producer can write A as this kernel's tiles; out: it has to
    bool feeds_tail = false, feeds_ln = false;           // the consumer (the fused tail / a LayerNorm) can sum split-K partials itself
    F16Range a_range; bool a_bound_assumed = false;      // the range of A, for the two-term form; assumed: the kernel enforces it by clamping A
};
// rows_per_clip: M = B*rows_per_clip
void add_gemm(PlanCtx& p, const std::string& name, int in_id, int out_id, int rows_per_clip, int N, int K,
              const float* W, const float* bias, int act, const GemmOpts& o = GemmOpts{}) {
    const double a_bound = o.a_range.ok() ? o.a_range.bound : 0.0;
    const int tail_E = p.h->cfg.embedding_dim;
    if (out_id >= 0) p.need(out_id, (size_t)rows_per_clip * N);
    // Contractions run on the bf16 matrix cores by exact operand splitting (gemm_x3.hip) where that kernel wins -
    // measured per shape on the Conformer / GRU / CNN heads at full batch (ms, split-operand vs float32 MFMA):
    // (N,K) = (576,144) 0.32 / 0.46, (144,576) 0.41 / 0.51, (432,144) 0.26 / 0.33, (288,144) 0.18 / 0.24,
    // (144,64) 0.05 / 0.07, (384,64) 0.23 / 0.29, (128,12800) 0.09 / 0.14 - and stay on the float32 MFMA kernel for the
    // small square ones, (144,144) 0.23 / 0.18, whose single padded column tile wastes the wide kernel.  Long-K layers
    // get a fine split-K.  The choice depends on (N, K) only, so batch invariance is kept.
    // NWW_GEMM_X3 = 0: never, 2: every shape with N, K >= 32, 3: the round-1 rule (K >= 4096 only).
    const int x3_mode = nww_knobs().gemm_x3;
    const bool small_square = N <= 160 && K > 64 && K <= 160;
    const bool use_x3 = p.h->conv_products != 0 &&
                        (x3_mode == 2 ? (N >= 32 && K >= 32)
                         : x3_mode == 3 ? (K >= 4096 && N >= 64 && N <= 256)
                         : (x3_mode == 1 && N >= 64 && K >= 32 && !small_square));
    const void* wx3 = nullptr;
    // two binary16 terms (NWW_ARITH_F16X3) when the caller knows a bound on |A|: A times a_scale stays inside the binary16 range
    float h2_as = 0.0f, h2_ws = 0.0f;
    if (use_x3 && p.h->f16 && a_bound > 0.0) {
        const auto hW = f16_fetch(p.h, W, (size_t)N * K);
        // A's channels are contiguous blocks of K / channels columns (the trunk's [C][H / 4][W / 4] output, flattened): the bound is held
        // against what the quietest row of W sees of them (f16_rows_ok), and W's rows against its largest weight
        bool rows_ok = true;
        const int nch = (int)o.a_range.ch.size();
        if (nch > 0 && K % nch == 0) {
            const int per = K / nch;
            const F16Rows m = f16_rows_moments(N, K, [&](int q, int co) { return hW[(size_t)co * K + q]; }, [&](int q) { return q / per; }, o.a_range.ch);
            rows_ok = f16_rows_ok(a_bound, m) && f16_rows_weights_ok(m, K);
        }
        h2_as = rows_ok ? f16_scale(a_bound) : 0.0f;
        if (h2_as > 0.0f) h2_ws = f16_wscale(hW);
    }
    const bool h2_req = h2_as > 0.0f && h2_ws > 0.0f;
    if (use_x3) {
        // the packed image comes in two formats (scaled binary16 terms / bf16 terms): the cache is keyed on the weight AND the format
        // (with its scale), so a second layer on the same W with a different decision gets its own image
        const X3Key key{W, h2_req ? 1 : 0, h2_req ? h2_ws : 0.0f};
        auto it = p.h->x3_weights.find(key);
        if (it == p.h->x3_weights.end()) {
            void* d = nullptr;
            if (hipMalloc(&d, gemm_x3_weight_bytes(N, K)) == hipSuccess &&
                (h2_req ? launch_split_weights_h2(W, d, N, K, h2_ws, p.h->own_stream) : launch_split_weights_x3(W, d, N, K, p.h->own_stream)) == hipSuccess)
                it = p.h->x3_weights.emplace(key, d).first;
            else if (d) (void)hipFree(d);
        }
        if (it != p.h->x3_weights.end()) wx3 = it->second;
    }
    const bool h2 = h2_req && wx3 != nullptr;                  // the two-term epilogue only with its image
    if (h2 && o.a_bound_assumed && in_id == BUF_X) p.h->clamps_features = true;
    // the producer may write A directly as this kernel's [128][32] tiles (the fused trunk feeding fc1)
    const int a_blocked = (o.a_blocked_inout && *o.a_blocked_inout && wx3 && K % 32 == 0 && rows_per_clip == 1) ? K / 32 : 0;
    if (o.a_blocked_inout) *o.a_blocked_inout = a_blocked != 0;
    if (K >= 2048 && (size_t)16 * rows_per_clip * N > p.h->splitk_per_clip) p.h->splitk_per_clip = (size_t)16 * rows_per_clip * N;
    p.add("gemm:" + name + (h2 && wx3 ? " [f16x3]" : ""), [=](Run& r) {
        GemmArgs g;
        g.A = src(r, in_id); g.lda = K; g.W = W; g.C = dst(r, out_id); g.ldc = N;
        g.M = r.B * rows_per_clip; g.N = N; g.K = K; g.bias = bias; g.alpha = o.alpha; g.beta = o.beta; g.act = act;
        g.res = o.res_id == BUF_NONE ? nullptr : src(r, o.res_id); g.ldres = N; g.rscale = o.rscale;
        g.Wx3 = wx3;
        if (h2) { g.h2 = 1; g.a_scale = h2_as; g.c_scale = 1.0f / (h2_as * h2_ws); g.a_clamp = o.a_bound_assumed ? (float)a_bound : 0.0f; }
        g.a_blocked = a_blocked;
        g.pp = nww_knobs().gemm_pp;
        g.splitk = gemm_recommended_splitk(g.M, N, K, r.cu_count);
        // split-operand layers: chunks of ~16-25 k-tiles, so that a small batch's chunk is ONE round of gemm_x3_chain_kernel
        // (32 k-tiles in flight) on a few dozen CUs - K = 12 800: 16 chunks of 25, K = 6 464: 12 of 17, K = 3 920 (C1): 7 of 18
        if (wx3 && x3_mode != 2 && K >= 2048) { g.splitk = K >= 8192 ? K / 800 : K / 512; if (g.splitk > 16) g.splitk = 16; if (g.splitk < 1) g.splitk = 1; }
        g.splitk_ws = r.splitk_ws;
        if (g.splitk > 1 && (size_t)g.splitk * g.M * N > r.splitk_floats) g.splitk = 1;
        r.deferred.active = false;
        // only the MFMA kernels leave split-K partials; the VALU fallback (K % 4 != 0 or an A pointer that is not 16-byte aligned)
        // writes C itself, so nothing may be deferred to the consumer then
        const bool partials = g.splitk > 1 && g.splitk_ws && gemm_writes_partials(g);
        // the fused tail sums the partials itself, in the reduce kernel's order: one dependent launch and the round trip of this layer's
        // output less.  A handful of clips (the interpreter's calls; B = 1: 62 -> 58 us back-to-back) on the latency kernel, large batches
        // where the persistent tail runs (tail_batch_runs, the predicate launch_classifier_tail itself uses; B = 4096: reduce + tail
        // 0.0076 + 0.0167 -> 0.0121 ms).  In between the reduce launch stays: the latency kernel's few workgroups read the partials slower.
        if (o.feeds_tail && partials && !g.res && (g.M <= 8 || tail_batch_runs(g.M, N, tail_E, false, g.splitk))) {
            g.defer_reduce = true;
            r.deferred.active = true; r.deferred.out_id = out_id; r.deferred.parts = g.splitk; r.deferred.stride = (size_t)g.M * N;
            r.deferred.bias = bias; r.deferred.alpha = o.alpha; r.deferred.beta = o.beta; r.deferred.act = act;
        }
        // a LayerNorm right behind a split-K Linear (DNN layer1) sums the partials itself, at every batch size: the reduce launch
        // and its round trip go (the caller's LayerNorm step checks r.deferred)
        if (o.feeds_ln && partials && !g.res && !o.alpha && act == ACT_NONE && N <= 256) {
            g.defer_reduce = true;
            r.deferred.active = true; r.deferred.out_id = out_id; r.deferred.parts = g.splitk; r.deferred.stride = (size_t)g.M * N;
            r.deferred.bias = bias; r.deferred.alpha = nullptr; r.deferred.beta = nullptr; r.deferred.act = ACT_NONE;
        }
        return launch_gemm(g, r.stream);
    });
}

// Short-K Linear on the input-stationary split-operand kernel (lin_x3.hip); false -> the caller plans the general GEMM.
// LIN_BIAS: out = y + b; LIN_RES: out = res + rscale (y + b); LIN_GLU: W = [2N][K], out = a * sigmoid(b);
// LIN_RES_TAB: out = rscale (y + b) + res_tab[(row % qkv_T) N ..] (a [>= qkv_T][N] table, the Transformer's positional encoding)
enum LinEpi : int { LIN_BIAS = 0, LIN_RES = 1, LIN_GLU = 2, LIN_RES_TAB = 3 };
struct LinOpts {
    int epi = LIN_BIAS, res_id = BUF_NONE; float rscale = 1.f; const float* res_tab = nullptr;
    const float *ln_w = nullptr, *ln_b = nullptr;        // LayerNorm of the input rows first (LIN_GLU, and LIN_BIAS at the widths that have it)
    int qkv_T = 0, qkv_dh = 0;                           // q | k | v written head-major: the clip's rows and the head width
};
bool add_lin_x3(PlanCtx& p, const std::string& name, int in_id, int out_id, int rows_per_clip, int N, int K, const float* W,
                const float* bias, const LinOpts& o = LinOpts{}) {
    if (!nww_knobs().lin_x3 || p.h->conv_products != 6 || !lin_x3_supported(K, N, true)) return false;
    if (o.ln_w && o.epi != LIN_GLU && !(o.epi == LIN_BIAS && lin_x3_ln_plain_supported(K))) return false;
    const int parts = o.epi == LIN_GLU ? 2 : 1;
    // under NWW_ARITH_F16X3: two binary16 terms per operand, the input rows scaled per row in the kernel (LinArgs::h2: no bound on the
    // tensor needed); conv_arith = bf16x6 keeps the three-term bf16 form
    float ws = 0.0f;
    if (p.h->f16) ws = f16_wscale(f16_fetch(p.h, W, (size_t)parts * N * K));
    const bool h2 = ws > 0.0f;
    if (!lin_x3_supported(K, N, h2)) return false;                 // K = 192 / 256 exist in the two-term form only
    const int terms = h2 ? 2 : 3;
    void* packed = p.pack_one(lin_x3_packed_bytes(K, N, parts, terms), [&](void* d) { return launch_lin_x3_pack(W, bias, d, K, N, parts, N, p.h->own_stream, terms, h2 ? ws : 1.0f); });
    if (!packed) return false;
    p.need(out_id, (size_t)rows_per_clip * N);
    const float w_un = h2 ? 1.0f / ws : 1.0f;
    p.add("lin_x3:" + name + (h2 ? " [f16x3]" : ""), [=](Run& r) {
        LinArgs a;
        a.x = src(r, in_id); a.ldx = K; a.out = dst(r, out_id); a.ldc = N;
        a.res = o.res_tab ? o.res_tab : o.res_id == BUF_NONE ? nullptr : src(r, o.res_id); a.ldres = N; a.rscale = o.rscale;
        a.ln_w = o.ln_w; a.ln_b = o.ln_b; a.packed = static_cast<const unsigned char*>(packed);
        a.M = r.B * rows_per_clip; a.N = N; a.qkv_T = o.qkv_T; a.qkv_dh = o.qkv_dh;
        a.h2 = h2 ? 1 : 0; a.w_un = w_un;
        return launch_lin_x3(a, K, o.epi, o.ln_w != nullptr, r.stream);
    });
    return true;
}

// A Linear (+ residual res_id times rscale) on the short-K kernel where it applies, else on the general GEMM with the same operands
void add_linear(PlanCtx& p, const std::string& name, int in_id, int out_id, int rows_per_clip, int N, int K, const float* W,
                const float* bias, int res_id = BUF_NONE, float rscale = 1.f) {
    LinOpts lo; lo.epi = res_id == BUF_NONE ? LIN_BIAS : LIN_RES; lo.res_id = res_id; lo.rscale = rscale;
    GemmOpts go; go.res_id = res_id; go.rscale = rscale;
    if (!add_lin_x3(p, name, in_id, out_id, rows_per_clip, N, K, W, bias, lo))
        add_gemm(p, name, in_id, out_id, rows_per_clip, N, K, W, bias, ACT_NONE, go);
}

void set_tail(PlanCtx& p, const std::string& name, int in_id, int K, const float* W, const float* b) {
    p.tail_name = name; p.tail_in = in_id; p.tail_K = K; p.tail_W = W; p.tail_b = b;
}

void add_conv(PlanCtx& p, const std::string& name, int in_id, int out_id, int Cin, int Cout, int H, int W,
              const float* w, const float* bias, const float* alpha, const float* beta, int act, int pool, int nhwc_out = 0) {
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    p.need(out_id, (size_t)Cout * Ho * Wo);
    p.add("conv3x3:" + name, [=](Run& r) {
        Conv3Args a{src(r, in_id), w, bias, alpha, beta, dst(r, out_id), r.B, Cin, Cout, H, W, act, pool};
        a.nhwc_out = nhwc_out;
        return launch_conv3x3(a, r.stream);
    });
}

static int trunk_fits(int C1, int H, int W) { int per_cu = 0; return trunk_pick_strips(C1, H, W, &per_cu); }
// out_blocked, read at run time: the output as the consumer GEMM's A tiles (add_gemm decides); the two-term form: the input's range in, the output's out
struct TrunkOpts { const bool* out_blocked = nullptr; F16Range in_range; F16Range* out_range = nullptr; };
// fused conv1+pool+conv2+pool (trunk.hip) when the 1->16->32 pattern fits LDS; returns false if not applicable
bool add_trunk(PlanCtx& p, const std::string& name, int in_id, int out_id, int C1, int C2, int H, int W,
               const float* w1, const float* b1, const float* al1, const float* be1, const float* w2,
               const float* b2, const float* al2, const float* be2, int act, const TrunkOpts& o = TrunkOpts{}) {
    if (o.out_range) *o.out_range = F16Range{};
    const double in_bound = o.in_range.ok() ? o.in_range.bound : 0.0;
    if (!nww_knobs().trunk || C1 != 16 || C2 != 32 || H < 4 || W < 4 || trunk_fits(C1, H, W) == 0) return false;
    p.need(out_id, (size_t)C2 * (H / 4) * (W / 4));
    const int max_grid = p.h->cu_count;
    // both convolutions on the bf16 matrix cores by exact operand splitting (trunk_b.hip) or on the float32 MFMA (nww_config.conv_arith)
    const int x3 = p.h->conv_products;
    if ((x3 == 6 || x3 == 9) && trunk_b_pick_strips(H, W) > 0) {
        // both convolutions' weights as the MFMA register images, split into bf16 terms once (trunk_b.hip)
        // NWW_ARITH_F16X3: two binary16 terms per operand when the input is bounded; the scales from bounds on conv1's / conv2's outputs
        float f_in = 0.0f, f_s1 = 0.0f, f_w1 = 0.0f, f_w2 = 0.0f;
        double bound2 = 0.0, typ2 = 0.0;
        std::vector<double> ch2;
        if (p.h->f16 && x3 == 6 && in_bound > 0.0 && (act == ACT_RELU || act == ACT_GELU || act == ACT_SILU)) {
            const auto hw1 = f16_fetch(p.h, w1, (size_t)C1 * 9), hw2 = f16_fetch(p.h, w2, (size_t)C2 * C1 * 9);
            const auto hb1 = f16_fetch(p.h, b1, C1), hb2 = f16_fetch(p.h, b2, C2);
            const auto ha1 = f16_fetch(p.h, al1, C1), he1 = f16_fetch(p.h, be1, C1), ha2 = f16_fetch(p.h, al2, C2), he2 = f16_fetch(p.h, be2, C2);
            const double bound1 = f16_layer_bound(hw1, C1, 9, hb1, b1 != nullptr, ha1, he1, al1 != nullptr, in_bound);
            bound2 = f16_layer_bound(hw2, C2, C1 * 9, hb2, b2 != nullptr, ha2, he2, al2 != nullptr, bound1);
            const F16Range r1{bound1, f16_layer_typ(hw1, C1, 9, ha1, al1 != nullptr, o.in_range.typ)};
            typ2 = f16_layer_typ(hw2, C2, C1 * 9, ha2, al2 != nullptr, r1.typ);
            // per channel: conv1's output as conv2's quietest row sees it against bound1, and both layers' rows against their largest weight
            const std::vector<double> tin = o.in_range.ch.size() == 1 ? o.in_range.ch : std::vector<double>(1, o.in_range.typ);
            const F16Rows m1 = f16_rows_moments(C1, 9, [&](int q, int co) { return hw1[(size_t)co * 9 + q]; }, [](int) { return 0; }, tin);
            const F16Rows m2 = f16_rows_moments(C2, C1 * 9, [&](int q, int co) { return hw2[(size_t)co * C1 * 9 + q]; }, [](int q) { return q / 9; },
                                                f16_rows_typ(m1, hb1, b1 != nullptr, ha1, he1, al1 != nullptr));
            ch2 = f16_rows_typ(m2, hb2, b2 != nullptr, ha2, he2, al2 != nullptr);
            if (r1.ok() && f16_rows_ok(bound1, m2) && f16_rows_weights_ok(m1, 9) && f16_rows_weights_ok(m2, C1 * 9)) {
                f_in = f16_scale(in_bound); f_s1 = f16_scale(bound1); f_w1 = f16_wscale(hw1); f_w2 = f16_wscale(hw2);
            }
        }
        const bool f16 = f_in > 0.0f && f_s1 > 0.0f && f_w1 > 0.0f && f_w2 > 0.0f;
        void* packed = p.pack_one(trunk_b_packed_bytes(), [&](void* d) {
            return f16 ? launch_trunk_b_pack_f16(w1, w2, static_cast<unsigned char*>(d), f_w1, f_w2, p.h->own_stream)
                       : launch_trunk_b_pack(w1, w2, static_cast<unsigned char*>(d), p.h->own_stream);
        });
        if (!packed) return false;
        if (f16 && o.out_range) *o.out_range = F16Range{bound2, typ2, ch2};
        const int products = f16 ? 3 : x3;
        // BN + ReLU stems (CRNN, E2E): all folded-BN factors of both layers non-negative (gamma > 0, the usual case) -> the pooled value is
        // the window's maximum pushed through BN + ReLU (trunk_b.hip: POS instance)
        const int bn_pos = f16 && al1 && al2 && act == ACT_RELU && f16_all_nonneg(p.h, al1, C1) && f16_all_nonneg(p.h, al2, C2);
        if (in_id == BUF_X && !p.h->e2e_transposed) p.h->x_stride_ok = true;                // this step reads the head input with any clip stride
        if (f16 && in_id == BUF_X) p.h->clamps_features = true;
        p.add("trunk_x3:" + name + (f16 ? " [f16x3]" : ""), [=](Run& r) {
            TrunkArgs a{src(r, in_id), w1, b1, al1, be1, w2, b2, al2, be2, dst(r, out_id), r.B, H, W, act};
            if (o.out_blocked && *o.out_blocked) a.out_blocked = C2 * (H / 4) * (W / 4) / 32;     // decided by the consumer (add_gemm) at plan time
            a.wpack = static_cast<const unsigned char*>(packed);
            if (f16) { a.f16_in = f_in; a.f16_k1 = f_in * f_w1; a.f16_s1 = f_s1; a.f16_k2 = f_s1 * f_w2; a.f16_so = 1.0f; a.f16_clamp = (float)in_bound; }
            a.bn_pos = bn_pos;
            const HopView& v = r.hop;
            if (in_id == BUF_X) a.in_clip_stride = v.x_stride;
            if (v.mode) {                               // streaming hop: pooled rows into the per-stream rings, all of them or the invalidated ones
                a.out = v.a2_ring; a.out_ring_rows = v.a2_rows; a.out_row0 = v.a2_row0;
                a.out_ch_stride = v.a2_ch_stride; a.out_clip_stride = v.a2_clip_stride;
                a.n_sub = v.a2_nsub;
                for (int q = 0; q < a.n_sub; ++q) { a.sub_a[q] = v.a2_sub_a[q]; a.sub_b[q] = v.a2_sub_b[q]; }
            }
            return launch_cnn_trunk_b(a, products, max_grid, r.stream);
        });
        return true;
    }
    p.add("trunk:" + name, [=](Run& r) {
        TrunkArgs a{src(r, in_id), w1, b1, al1, be1, w2, b2, al2, be2, dst(r, out_id), r.B, H, W, act};
        return launch_cnn_trunk(a, C1, C2, max_grid, r.stream);
    });
    return true;
}

struct ConvMfmaOpts {
    int avg_kw = 0, avg_sw = 0, avg_ow = 0, avg_y = 0;   // an average pool behind the conv: window, stride, outputs (0: none); along y instead of x
    bool* seq_inout = nullptr;                           // in: write the recurrent layers' sequence layout; out: whether this instance does
    bool* ring_in = nullptr;                             // in: the input may come from the streaming rings; out: whether this instance reads them
    F16Range in_range; F16Range* out_range = nullptr;    // the two-term form: the input's range in, the output's out
    int scratch_id = BUF_NONE;                           // raw sums of the k-split passes (more than 32 input channels)
};
// 3x3 conv stage with 32 input channels on MFMA (trunk.hip) when it fits; false -> caller uses the VALU kernel
bool add_conv_mfma(PlanCtx& p, const std::string& name, int in_id, int out_id, int Cin, int Cout, int H, int W,
                   const float* w, const float* bias, const float* alpha, const float* beta, int act, int pool,
                   const ConvMfmaOpts& o = ConvMfmaOpts{}) {
    if (o.out_range) *o.out_range = F16Range{};
    double in_bound = o.in_range.ok() ? o.in_range.bound : 0.0;
    const int enabled = nww_knobs().conv_mfma, x3_enabled = nww_knobs().conv3_x3;
    // the input's bound against what this stage's quietest row sees of its channels (f16_rows_ok), the rows against their largest weight
    F16Rows rows;
    const auto hw = p.h->f16 && in_bound > 0.0 ? f16_fetch(p.h, w, (size_t)Cout * Cin * 9) : std::vector<float>();
    if (p.h->f16 && in_bound > 0.0 && (int)o.in_range.ch.size() == Cin) {
        rows = f16_rows_moments(Cout, Cin * 9, [&](int q, int co) { return hw[(size_t)co * Cin * 9 + q]; }, [](int q) { return q / 9; }, o.in_range.ch);
        if (!(f16_rows_ok(in_bound, rows) && f16_rows_weights_ok(rows, Cin * 9))) in_bound = 0.0;
    }
    // 64 input channels (a fourth CRNN stage): conv3_x3's wide instance - two-term arithmetic on a bounded input only
    bool wide = Cin == 64 && enabled && x3_enabled && pool && o.avg_ow == 0 && !o.avg_y && p.h->conv_products == 6 && p.h->f16 && in_bound > 0.0 &&
                Cout % 32 == 0 && conv3_x3_wide_fits(Cin, H, W, Cout);
    if (wide && (f16_scale(in_bound) <= 0.0f || f16_wscale(hw) <= 0.0f)) wide = false;
    // more than 32 input channels without a usable bound (the worst-case bound of a fourth stage is usually too loose for two terms): the
    // 32-channel three-term instance once per 32 input channels - every pass but the last leaves raw, un-pooled sums in a scratch buffer, the
    // next one starts its accumulators from them (k-split; the planes of such stages are a few hundred pixels)
    if (!wide && Cin > 32) {
        if (!enabled || !x3_enabled || Cin % 32 != 0 || Cin > 256 || !pool || o.avg_ow > 0 || o.avg_y || p.h->conv_products != 6 || o.scratch_id == BUF_NONE ||
            Cout % 32 != 0) return false;
        const bool whole = conv3_x3_fits(H, W, Cout, 0, 1) && conv3_x3_fits(H, W, Cout, 0, 0);
        const int sh = whole ? 0 : conv3_x3_strip_rows(H, W, Cout);          // larger planes: in strips of rows
        if (!whole && sh == 0) return false;
        if (o.ring_in) *o.ring_in = false;
        p.need(out_id, (size_t)Cout * (H / 2) * (W / 2));
        p.need(o.scratch_id, (size_t)Cout * H * W);
        const int np = Cin / 32, grid = p.h->cu_count * ((sh ? conv3_x3_strip_lds_bytes(sh, W) : conv3_x3_lds_bytes(H, W, 0)) * 2 <= 160 * 1024 ? 2 : 1);
        const int seq_out = (o.seq_inout && *o.seq_inout) ? 1 : 0;
        for (int pass = 0; pass < np; ++pass) {
            const bool fin = pass == np - 1;
            p.add(std::string(fin && seq_out ? "conv3_x3+seq:" : "conv3_x3:") + name + " (input channels " + std::to_string(32 * pass) + "-" + std::to_string(32 * pass + 31) +
                      (fin ? ", epilogue)" : ", raw sums)"), [=](Run& r) {
                ConvMfmaArgs a{src(r, in_id), w, fin ? bias : nullptr, fin ? alpha : nullptr, fin ? beta : nullptr, fin ? dst(r, out_id) : r.buf[o.scratch_id],
                               r.B, H, W, Cout, fin ? act : (int)ACT_NONE, fin ? 1 : 0};
                a.w_cin = Cin; a.w_cin_off = 32 * pass; a.acc_in = pass ? r.buf[o.scratch_id] : nullptr; a.seq_out = fin ? seq_out : 0; a.strip_h = sh;
                return launch_conv3_x3(a, grid, r.stream);
            });
        }
        return true;
    }
    if (wide) {
        if (o.ring_in) *o.ring_in = false;
    } else if (!enabled || Cin != 32 || Cout % 32 != 0 || H < 2 || W < 2)
        return false;
    // (the float32-MFMA instance shares its 8 waves among the 32-channel groups; conv3_x3 takes one group per workgroup)
    // (... and its fused average pool keeps 8 waves x 64 channels x 4 sums in the plane's LDS: launch_conv3x3_mfma refuses a plane smaller than that)
    const bool f32_fits = !wide && (8 % (Cout / 32)) == 0 && conv_mfma_lds_bytes(Cin, H, W) <= 160 * 1024 &&
                          !(o.avg_ow > 0 && (o.avg_ow > 4 || (size_t)8 * 64 * 4 * sizeof(float) > conv_mfma_lds_bytes(Cin, H, W)));
    // pooled planes of more than 512 pixels (clips longer than ~1.3 s, a second stage behind an unfused first one): conv3_x3 in strips of rows
    const int strip_h = (!wide && pool && o.avg_ow == 0 && !o.avg_y && !conv3_x3_fits(H, W, Cout, o.avg_ow, pool)) ? conv3_x3_strip_rows(H, W, Cout) : 0;
    const bool x3_shape = strip_h > 0 || conv3_x3_fits(H, W, Cout, o.avg_ow, pool);
    if (!wide && !f32_fits && !(x3_enabled && p.h->conv_products == 6 && x3_shape)) return false;
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    p.need(out_id, o.avg_ow > 0 ? (size_t)Cout * o.avg_ow : (size_t)Cout * Ho * Wo);
    const int max_grid = p.h->cu_count;
    // split-operand bf16 instance (conv3_x3.hip) under the same arithmetic switch as the fused trunk; the 9-product
    // mode keeps the float32-MFMA kernel (the conv3 instance implements the 6-product form only)
    if (wide || (x3_enabled && p.h->conv_products == 6 && x3_shape)) {
        const size_t lds = wide ? conv3_x3_wide_lds_bytes(Cin, H, W) : strip_h ? conv3_x3_strip_lds_bytes(strip_h, W) : conv3_x3_lds_bytes(H, W, o.avg_ow);
        if (strip_h && o.ring_in) *o.ring_in = false;                                             // strips read dense planes
        const int per_cu = lds * 2 <= 160 * 1024 ? 2 : 1;
        const int seq_out = (o.seq_inout && *o.seq_inout && pool && o.avg_ow == 0) ? 1 : 0;      // the caller wants the sequence layout
        const bool ring_ok = o.ring_in && *o.ring_in;                                             // ... and may hand the input over in rings
        // NWW_ARITH_F16X3: two binary16 terms when the input is bounded (the fused trunk's plan-time bound)
        float h2_in = 0.0f, h2_w = 0.0f;
        if (p.h->f16 && in_bound > 0.0) {
            h2_in = f16_scale(in_bound); h2_w = f16_wscale(hw);
            if (o.out_range && h2_in > 0.0f && h2_w > 0.0f) {
                const auto hal = f16_fetch(p.h, alpha, Cout), hbe = f16_fetch(p.h, beta, Cout), hbi = f16_fetch(p.h, bias, Cout);
                *o.out_range = F16Range{f16_layer_bound(hw, Cout, Cin * 9, hbi, bias != nullptr, hal, hbe, alpha != nullptr, in_bound),
                                      f16_layer_typ(hw, Cout, Cin * 9, hal, alpha != nullptr, o.in_range.typ)};
                if (!rows.sig2.empty()) o.out_range->ch = f16_rows_typ(rows, hbi, bias != nullptr, hal, hbe, alpha != nullptr);
            }
        }
        const bool h2 = h2_in > 0.0f && h2_w > 0.0f;
        p.add(std::string(o.avg_ow > 0 ? "conv3_x3+avgpool:" : seq_out ? "conv3_x3+seq:" : "conv3_x3:") + name + (strip_h ? " (strips of " + std::to_string(strip_h) + " rows)" : "") + (h2 ? " [f16x3]" : ""), [=](Run& r) {
            ConvMfmaArgs a{src(r, in_id), w, bias, alpha, beta, dst(r, out_id), r.B, H, W, Cout, act, pool};
            a.Cin = Cin; a.w_cin = Cin; a.strip_h = strip_h;
            a.avg_kw = o.avg_kw; a.avg_sw = o.avg_sw; a.avg_ow = o.avg_ow; a.seq_out = seq_out; a.avg_y = o.avg_y;
            if (h2) { a.h2_in = h2_in; a.h2_w = h2_w; }
            const HopView& v = r.hop;
            if (ring_ok && v.mode) {                    // streaming hop: the fused trunk's pooled rows are read from their rings
                a.in = v.a2_ring; a.in_ring_rows = v.a2_rows; a.in_row0 = v.a2_row0;
                a.in_ch_stride = v.a2_ch_stride; a.in_clip_stride = v.a2_clip_stride;
                if (seq_out && v.seq_new) {             // ... and the sequence rows a hop does not invalidate are carried over from the previous hop's buffer
                    r.buf[out_id] = v.seq_new;          // (the recurrent layers planned behind this step read r.buf[out_id])
                    a.out = v.seq_new;
                    a.seq_prev = v.seq_prev; a.keep_lo = v.a3_lo; a.keep_hi = v.a3_hi; a.keep_shift = v.a3_shift;
                }
            }
            return launch_conv3_x3(a, max_grid * per_cu, r.stream);
        });
        return true;
    }
    if (o.avg_y) return false;                                   // only conv3_x3 pools along y (the caller checked e2e_transposed_ok)
    if (o.seq_inout) *o.seq_inout = false;                         // the float32-MFMA instance writes planes
    if (o.ring_in) *o.ring_in = false;                             // ... and reads dense planes
    p.add(std::string(o.avg_ow > 0 ? "conv3x3_mfma+avgpool:" : "conv3x3_mfma:") + name, [=](Run& r) {
        ConvMfmaArgs a{src(r, in_id), w, bias, alpha, beta, dst(r, out_id), r.B, H, W, Cout, act, pool};
        a.avg_kw = o.avg_kw; a.avg_sw = o.avg_sw; a.avg_ow = o.avg_ow;
        return launch_conv3x3_mfma(a, Cin, max_grid, r.stream);
    });
    return true;
}

// The E2E head can run on the TRANSPOSED plane (frames, n_mels) = (101, 64) instead of (64, 101): the fused trunk's 32-pixel
// conv1 groups and 16-column conv2 tiles waste 28 % on a 101-wide plane and nothing on a 64-wide one, conv3's 2 x 16 tiles 22 %
// against 4 %, and the frontend's frames-major output is its fast path.  Needs the split-operand kernels (default arithmetic).
bool e2e_transposed_ok(PlanCtx& p, int n_mels, int frames) {
    const Knobs& k = nww_knobs();
    const int H = frames, W = n_mels;
    return k.trunk && k.conv_mfma && k.conv3_x3 && p.h->conv_products == 6 && H >= 16 && W >= 4 && trunk_b_pick_strips(H, W) > 0 &&
           conv_mfma_lds_bytes(32, H / 4, W / 4) <= 160 * 1024 && conv3_x3_fits(H / 4, W / 4, 64, 4, 0);
}

// nn.GRU / nn.LSTM (bidirectional; G = 3 / 4 gates) -> rnn_out[:, -1, :] into buffer `last_id` [B][2H]; uses buffers
// xg_id, seqA, seqB.
void add_bigru_last(PlanCtx& p, const std::string& prefix, int in_id, int T, int I, int H, int layers, int xg_id,
                    int seqA, int seqB, int last_id, int G = 3) {
    p.need(xg_id, (size_t)(T + 1) * G * H);                  // + one row per clip: the reverse direction's last-frame projection
    p.need(last_id, (size_t)2 * H);
    // the recurrent product follows the handle's arithmetic switch; NWW_ARITH_F16X3: two binary16 terms (|h| <= 1 bounds the one
    // operand, W_hh's scale comes from the weights)
    const int products = p.h->f16 ? 3 : p.h->conv_products;
    RnnArgs probe; probe.H = H; probe.products = products;
    probe.w_hh = p.W(prefix + ".weight_hh_l" + std::to_string(layers - 1));       // the pointer the fused launch will really get (alignment test)
    const bool streamed = rnn_stream_usable(probe);      // 128 < H <= 256: W_hh streamed from L2 (rnn_stream.hip)
    bool x3 = probe.w_hh != nullptr && (rnn_x3_usable(probe) || streamed);
    if (x3 && H != 32 && H != 64 && H != 128) {              // zero-padded / streamed instances: two-term form only, so the last layer's W_hh must scale
        const float* wl = probe.w_hh;
        if (!(f16_wscale(f16_fetch(p.h, wl, (size_t)G * H * H)) > 0.0f)) x3 = false;
    }
    int cur_in = in_id, cur_I = I;
    for (int l = 0; l < layers; ++l) {
        const bool last = l == layers - 1;
        const int seq_out = (l % 2 == 0) ? seqA : seqB;
        if (!last) p.need(seq_out, (size_t)T * 2 * H);
        // rnn_out[:, -1] needs ONE step of the last layer's reverse direction, hence the input projection of frame T-1 only (a
        // strided GEMM over M = B rows instead of B*T, into the row behind the forward direction's xg) - and with h = 0 that
        // step has no recurrent product: rnn_x3 computes it in the forward direction's launch.
        const bool fold = last && x3;
        // GRU / RNN head, first layer fed by the head's own input features (GRU: 32 / 64 per frame; LSTM at H = 32 / 64: 32 / 64 / 96), two-term arithmetic: the forward direction's input
        // projection is computed inside the recurrence kernel - x_t W_ih^T on the matrix pipe beside h W_hh^T - instead of a GEMM that
        // writes T x 3H gate pre-activations per clip to HBM for the recurrence to read back (635 MB each way at B = 4096, T = 101, H = 128).
        const float* wih_f = p.W(prefix + ".weight_ih_l" + std::to_string(l));
        // (the LSTM's 101 x 256 pre-activations per clip at H = 64: 423 MB each way at B = 4096); NWW_RNN_IH_FUSED = 0 keeps the GEMM for both cells
        const bool fin_shape = G == 3 ? (cur_I == 32 || cur_I == 64) && (H == 32 || H == 64 || H == 128)
                                      : (cur_I == 32 || cur_I == 64 || cur_I == 96) && (H == 32 || H == 64);
        const float wi_scale = (nww_knobs().rnn_ih_fused && fold && l == 0 && in_id == BUF_X && products == 3 && fin_shape &&
                                wih_f && (reinterpret_cast<uintptr_t>(wih_f) & 15) == 0)
                                   ? f16_wscale(f16_fetch(p.h, wih_f, (size_t)G * H * cur_I)) : 0.0f;
        const float* whh_fwd = p.W(prefix + ".weight_hh_l" + std::to_string(l));
        const bool fuse_ih = wi_scale > 0.0f && f16_scale(F16_FEATURES.bound) > 0.0f && (H % 4) == 0 && H <= 256 &&
                             whh_fwd && f16_wscale(f16_fetch(p.h, whh_fwd, (size_t)G * H * H)) > 0.0f;      // ... and the recurrence itself takes the two-term form
        for (int dir = 0; dir < 2; ++dir) {
            const std::string sfx = "_l" + std::to_string(l) + (dir ? "_reverse" : "");
            const float* wih = p.W(prefix + ".weight_ih" + sfx);
            const float* whh = p.W(prefix + ".weight_hh" + sfx);
            const float* bih = p.W(prefix + ".bias_ih" + sfx);
            const float* bhh = p.W(prefix + ".bias_hh" + sfx);
            if (last && dir) {
                const int Iin = cur_I, in_buf = cur_in;
                p.add("gemm:" + prefix + ".ih" + sfx + "(last frame)", [=](Run& r) {
                    GemmArgs g;
                    g.A = src(r, in_buf) + (size_t)(T - 1) * Iin; g.lda = T * Iin; g.W = wih;
                    if (fold) { g.C = r.buf[xg_id] + (size_t)r.B * T * G * H; g.ldc = G * H; }      // behind the forward direction's rows
                    else { g.C = r.buf[xg_id] + (size_t)(T - 1) * G * H; g.ldc = T * G * H; }       // in place (the forward recurrence is done)
                    g.M = r.B; g.N = G * H; g.K = Iin; g.bias = bih; g.alpha = nullptr; g.beta = nullptr; g.act = ACT_NONE;
                    g.res = nullptr; g.ldres = 0; g.rscale = 1.f;
                    return launch_gemm(g, r.stream);
                });
            } else if (fuse_ih && dir == 0) {
                // (the forward direction's input projection runs inside its recurrence: RnnArgs::fin)
            } else {
                // short-K input projections (the GRU head's 64 mel bins) on the input-stationary kernel; the rest on the general GEMM
                add_linear(p, prefix + ".ih" + sfx, cur_in, xg_id, T, G * H, cur_I, wih, bih);
            }
            if (fold && dir == 0) continue;                  // the forward recurrence is launched after the reverse projection
            const int in_T = T;
            const float* whh_f = fold ? p.W(prefix + ".weight_hh_l" + std::to_string(l)) : whh;
            // (from the tensor itself, before the padded image takes its place: the any-width kernel reads neither w_scale nor products)
            const float w_scale = products == 3 ? f16_wscale(f16_fetch(p.h, whh_f, (size_t)G * H * H)) : 1.0f;
            // widths the register-resident / 32-units-per-wave kernels do not take: zero-padded weight rows for the any-width kernel
            int ldw = 0;
            if (H % 4 != 0 || H > 256) {
                void* padded = p.pack_one(rnn_wide_weight_bytes(G, H), [&](void* d) { return launch_rnn_pad_weights(whh_f, static_cast<float*>(d), G, H, p.h->own_stream); });
                if (padded) { whh_f = static_cast<const float*>(padded); ldw = (H + 7) & ~7; }
            }
            const float* bhh_f = fold ? p.W(prefix + ".bias_hh_l" + std::to_string(l)) : bhh;
            const std::string nm = fold ? (G == 4 ? "lstm:" : "gru:") + prefix + "_l" + std::to_string(l) + " + first reverse step"
                                        : (G == 4 ? "lstm:" : "gru:") + prefix + sfx;
            const int products_l = (products == 3 && !(w_scale > 0.0f)) ? p.h->conv_products : products;
            const void* w_packed = nullptr;
            if (streamed && products_l == 3 && ldw == 0) {
                w_packed = p.pack_one(rnn_stream_packed_bytes(G, H), [&](void* d) { return launch_rnn_stream_pack(whh_f, d, G, H, w_scale, p.h->own_stream); });
                // the folded form (reverse step inside the forward launch) exists only on the streamed kernel for these widths: without its
                // packed W_hh every forward would fail at run time - fail the finalize instead
                if (!w_packed && fold) p.h->plan_error = "out of device memory for the streamed W_hh image of " + prefix;
            }
            const bool fused_here = fuse_ih && fold && products_l == 3 && ldw == 0;
            const float* bih_f = p.W(prefix + ".bias_ih_l" + std::to_string(l));
            const int fin = cur_I;
            if (fused_here) p.h->clamps_features = true;       // the fused input projection clamps the features it splits
            p.add(nm + (fused_here ? " + input projection" : "") + (products_l == 3 && x3 && ldw == 0 ? (w_packed ? " [f16x3, W_hh streamed]" : " [f16x3]") : ""), [=](Run& r) {
                RnnArgs a;
                a.gates = G; a.products = products_l; a.w_scale = w_scale; a.w_packed = w_packed;
                if (fused_here) {
                    a.x_in = r.x; a.w_ih = wih_f; a.b_ih = bih_f; a.fin = fin;
                    a.x_scale = f16_scale(F16_FEATURES.bound); a.x_clamp = (float)F16_FEATURES.bound; a.wi_scale = wi_scale;
                }
                a.xg = r.buf[xg_id]; a.w_hh = whh_f; a.b_hh = bhh_f;
                a.seq_out = last ? nullptr : r.buf[seq_out]; a.ld_seq = 2 * H;
                a.last_out = last ? r.buf[last_id] : nullptr; a.ld_last = 2 * H;
                a.B = r.B; a.T = in_T; a.H = H; a.ldw = ldw; a.cu_count = r.cu_count;
                if (fold) {
                    a.col_off = 0; a.reverse = 0; a.steps = in_T;
                    a.xg2 = r.buf[xg_id] + (size_t)r.B * in_T * G * H; a.xg2_bstride = (size_t)G * H; a.b_hh2 = bhh; a.col_off2 = H;
                } else {
                    a.col_off = dir ? H : 0; a.reverse = dir;
                    a.steps = (last && dir) ? 1 : in_T;      // reverse half of rnn_out[:, -1] is its first step
                }
                return launch_rnn(a, r.stream);
            });
        }
        cur_in = seq_out; cur_I = 2 * H;
    }
}

// ------------------------------------------------------------------------------------------ attention modules
// The E-Branchformer's attention branch: the module reads LayerNorm(ln_w, ln_b)(h) - ln_name: that LayerNorm's module,
// ".attn_branch_norm" - and writes buffer `out` WITHOUT the residual, which the merge takes
struct AttnBranch { const float *ln_w = nullptr, *ln_b = nullptr; int out = BUF_NONE; const char* ln_name = ""; };
// The Conformer's whole attention module (in_proj, per-head softmax(q k^T) v, out_proj, residual) in one launch per clip-resident
// workgroup (attn_x3.hip) under the default arithmetic at the compiled shape; false: nothing planned (NWW_ATTN_FUSED = 0 among others)
// br (the E-Branchformer's branch): LayerNorm of the rows in front, no residual, the result in buffer br.out beside h
bool add_attn_x3(PlanCtx& p, const std::string& q, int hb, int T, int D, int NH, const AttnBranch& br = AttnBranch{}) {
    if (!(nww_knobs().attn_fused && p.h->f16 && p.h->conv_products == 6 && attn_x3_supported(T, D, NH))) return false;
    const float *iw = p.W(q + ".attention.in_proj_weight"), *ib = p.W(q + ".attention.in_proj_bias");
    const float *ow = p.W(q + ".attention.out_proj.weight"), *ob = p.W(q + ".attention.out_proj.bias");
    const auto hiw = f16_fetch(p.h, iw, (size_t)3 * D * D), how = f16_fetch(p.h, ow, (size_t)D * D);
    const float ws_in = f16_wscale(hiw), ws_out = f16_wscale(how);
    // |raw k / v accumulator| <= 2^15 (the clip-scaled rows) x the L1 norm of the scaled weight row: powers of two that keep them below 2^15
    auto l1max = [&](int r0) {
        double worst = 0;
        for (int r = r0; r < r0 + D; ++r) {
            double t = 0;
            for (int k = 0; k < D; ++k) t += std::fabs((double)hiw[(size_t)r * D + k]);
            worst = std::fmax(worst, t);
        }
        return worst;
    };
    const double lk = l1max(D) * ws_in * 1.02, lv = l1max(2 * D) * ws_in * 1.02;
    if (!(ws_in > 0.0f && ws_out > 0.0f && lk < 1e30 && lv < 1e30)) return false;
    PlanCtx::Packs pk(p);
    void *packed = pk.alloc(attn_x3_packed_bytes(D, NH)), *bc = packed ? pk.alloc((size_t)D * sizeof(float)) : nullptr;      // one launch fills both
    if (!bc || launch_attn_x3_pack(iw, ib, ow, ob, packed, static_cast<float*>(bc), D, NH, ws_in, ws_out, p.h->own_stream) != hipSuccess) return false;
    pk.commit();
    const float cK = lk > 1e-30 ? (float)f16_pow2_floor(1.0 / lk) : 1.0f, cV = lv > 1e-30 ? (float)f16_pow2_floor(1.0 / lv) : 1.0f;
    const float w_un = 1.0f / ws_in, o_un = 1.0f / (ws_out * ws_in * cV), qs = 1.0f / std::sqrt((float)(D / NH));
    if (br.ln_w) p.need(br.out, (size_t)T * D);
    p.add("attn_x3:" + q + (br.ln_w ? ".attention (ln+in_proj+softmax(qk)v+out_proj) [f16x3]" : ".attention (in_proj+softmax(qk)v+out_proj+res) [f16x3]"), [=](Run& r) {
        AttnArgs a{r.buf[hb], r.buf[br.ln_w ? br.out : hb], static_cast<const unsigned char*>(packed), static_cast<const float*>(bc), r.B, T, w_un, cK, cV, o_un, qs};
        if (br.ln_w) { a.ln_w = br.ln_w; a.ln_b = br.ln_b; }
        return launch_attn_x3(a, D, NH, r.cu_count, r.stream);
    });
    return true;
}

// h <- h + out_proj(softmax(q k^T / sqrt(dh)) v), q | k | v = in_proj(h), in three launches: block q's module `module` (".attention" /
// ".self_attn"); buffers hb (h), big (q | k | v), t1 (the heads' outputs)
// br (the E-Branchformer's branch): q | k | v = in_proj(LayerNorm(h)) - the LayerNorm inside the short-K in_proj where that
// kernel runs, else on its own into br.out - and out_proj WITHOUT the residual into buffer br.out
void add_attention_module(PlanCtx& p, const std::string& q, const char* module, int hb, int big, int t1, int T, int D, int NH,
                          const AttnBranch& br = AttnBranch{}) {
    const std::string m = q + module;
    // in_proj writes q, k, v head-major when the matrix-core attention consumes them: every (clip, head) block is then
    // one contiguous run for its LDS-DMA
    const int mha_mfma = nww_knobs().mha_mfma;
    const bool want_hm = mha_mfma && mha_mfma_supported(T, D, NH) && 3 * D <= 1024;
    const float *iw = p.W(m + ".in_proj_weight"), *ib = p.W(m + ".in_proj_bias");
    bool head_major = false;
    const std::string in_name = m + (want_hm ? ".in_proj(head-major)" : ".in_proj");
    int in_id = hb;
    LinOpts lo;
    if (want_hm) { lo.qkv_T = T; lo.qkv_dh = D / NH; }
    LinOpts lo_ln = lo; lo_ln.ln_w = br.ln_w; lo_ln.ln_b = br.ln_b;
    if (add_lin_x3(p, br.ln_w ? q + br.ln_name + "+" + std::string(module).substr(1) + (want_hm ? ".in_proj(head-major)" : ".in_proj") : in_name, hb, big, T, 3 * D, D, iw, ib, lo_ln)) {
        head_major = want_hm;
    } else {
        if (br.ln_w) {                                        // the LayerNorm on its own, into `br.out` (free until out_proj writes it)
            p.need(br.out, (size_t)T * D);
            p.add("layernorm:" + q + br.ln_name, [=](Run& r) { return launch_layernorm(r.buf[hb], r.buf[br.out], br.ln_w, br.ln_b, r.B * T, D, ACT_NONE, r.stream); });
            in_id = br.out;
        }
        if (add_lin_x3(p, in_name, in_id, big, T, 3 * D, D, iw, ib, lo))
            head_major = want_hm;
        else
            add_gemm(p, m + ".in_proj", in_id, big, T, 3 * D, D, iw, ib, ACT_NONE);
    }
    const int hm = head_major ? 1 : 0;
    if (mha_mfma && p.h->f16 && mha_h2_supported(T, D, NH))
        p.add("mha_h2:" + q + " [f16x3]", [=](Run& r) { return launch_mha_h2(r.buf[big], r.buf[t1], r.B, T, D, NH, r.cu_count, r.stream, hm); });
    else if (mha_mfma && mha_mfma_supported(T, D, NH))
        p.add("mha_mfma:" + q, [=](Run& r) { return launch_mha_mfma(r.buf[big], r.buf[t1], r.B, T, D, NH, r.cu_count, r.stream, hm); });
    else
        p.add("mha_core:" + q, [=](Run& r) { return launch_mha_core(r.buf[big], r.buf[t1], r.B, T, D, NH, r.stream); });
    if (br.ln_w) add_linear(p, m + ".out_proj", t1, br.out, T, D, D, p.W(m + ".out_proj.weight"), p.W(m + ".out_proj.bias"));
    else add_linear(p, m + ".out_proj+res", t1, hb, T, D, D, p.W(m + ".out_proj.weight"), p.W(m + ".out_proj.bias"), hb, 1.0f);
}

// ------------------------------------------------------------------------------------------ feed-forward and convolution modules
// A feed-forward module's weights, the LayerNorm in front included (the Transformer's norm1)
struct FfnWeights { const float *ln_w, *ln_b, *w1, *b1, *w2, *b2; };
FfnWeights ffn_weights(PlanCtx& p, const std::string& ln, const std::string& m) {      // ln: the LayerNorm's module, m: the Linears' parent
    return {p.W(ln + ".weight"), p.W(ln + ".bias"), p.W(m + ".linear1.weight"), p.W(m + ".linear1.bias"), p.W(m + ".linear2.weight"), p.W(m + ".linear2.bias")};
}
// NWW_ARITH_F16X3: both operands of both products are bounded whatever the residual stream holds - |LayerNorm(h)_i| <= sqrt(D) |w_i|
// + |b_i|, |swish(v)| <= |v|, relu(v) <= |v| - so the scales need nothing but the weights
struct FfnScales {
    float fx = 0.0f, fw1 = 0.0f, fh = 0.0f, fw2 = 0.0f;
    bool ok() const { return fx > 0.0f && fw1 > 0.0f && fh > 0.0f && fw2 > 0.0f; }
};
FfnScales ffn_f16_scales(PlanCtx& p, const FfnWeights& w, int D) {
    FfnScales s;
    const double bx = f16_ln_bound(p.h, w.ln_w, w.ln_b, D);
    const auto w1 = f16_fetch(p.h, w.w1, (size_t)4 * D * D), w2 = f16_fetch(p.h, w.w2, (size_t)4 * D * D), b1 = f16_fetch(p.h, w.b1, (size_t)4 * D);
    const double bh = f16_layer_bound(w1, 4 * D, D, b1, true, b1, b1, false, bx);
    s.fx = f16_scale(bx); s.fw1 = f16_wscale(w1); s.fh = f16_scale(bh); s.fw2 = f16_wscale(w2);
    return s;
}
// The module in three launches: LayerNorm(hb) -> ln_out, linear1 + act -> big, hb <- hb + rscale linear2
void add_ffn_unfused(PlanCtx& p, const FfnWeights& w, int act, float rscale, int hb, int ln_out, int big, int T, int D,
                     const std::string& ln_name, const std::string& l1_name, const std::string& l2_name) {
    p.add("layernorm:" + ln_name, [=](Run& r) { return launch_layernorm(r.buf[hb], r.buf[ln_out], w.ln_w, w.ln_b, r.B * T, D, ACT_NONE, r.stream); });
    add_gemm(p, l1_name, ln_out, big, T, 4 * D, D, w.w1, w.b1, act);
    GemmOpts res; res.res_id = hb; res.rscale = rscale;
    add_gemm(p, l2_name, big, hb, T, D, 4 * D, w.w2, w.b2, ACT_NONE, res);
}

// round 6: the row-local Linears next to a feed-forward module run INSIDE its launch (FfnArgs::px: input_proj in front of the first
// block's ff1, conv2 + residual in front of every ff2), and the last block's LayerNorm + time average behind its ff2
// (FfnArgs::msum); NWW_FFN_FUSED = 0 and the other arithmetics keep the separate launches.
// kind: 0 none, 1 input_proj (x = the head input), 2 conv_module.conv2 + residual (x = the depthwise output in t3); name: the
// Linear's step when it is planned on its own because the form planned does not take it
struct FfnPro { int kind = 0; std::string name; const float *w = nullptr, *b = nullptr; int k = 0; };
// the block's final LayerNorm + mean over time (block: its name, for the step that finishes the mean)
struct FfnEpi { bool want = false; std::string block; const float *ln_w = nullptr, *ln_b = nullptr; };
// The pre-norm module (swish) hb <- hb + rscale ffn(hb) in block-scope buffers hb, t1, t3, big; `name`: the module's.  A step takes one
// of four forms, richest first: prologue + epilogue, prologue, plain ffn_x3, unfused (LayerNorm + two GEMMs).  Returns whether the
// epilogue was fused.
bool add_ffn(PlanCtx& p, const std::string& name, const FfnWeights& w, float rscale, int hb, int t1, int t3, int big, int T, int D,
             const FfnPro& pro = FfnPro{}, const FfnEpi& epi = FfnEpi{}) {
    struct Form { int pro = 0; bool epi = false, fused = false, h2 = false; FfnScales s; float pws = 0.0f, mscale = 0.0f; } f;
    // the richest feasible form with at most the requested prologue / epilogue: plan-time scales only, nothing allocated or launched.
    // LayerNorm + linear1 + swish + linear2 + residual in one kernel (ffn_x3.hip); same arithmetic switch as the split-operand GEMMs
    // it replaces
    if (nww_knobs().ffn_fused && p.h->conv_products == 6 && ffn_x3_supported(D, p.h->f16)) {
        if (p.h->f16) f.s = ffn_f16_scales(p, w, D);
        f.h2 = f.s.ok();
        f.fused = ffn_x3_supported(D, f.h2);
    }
    if (f.fused && f.h2) {                                 // the prologue / epilogue instances: two-term form only
        // the prologue Linear's weights (two binary16 terms; its input rows are scaled per row in the kernel)
        if (pro.kind && ffn_x3_pro_supported(D, pro.k) && pro.b) {
            f.pws = f16_wscale(f16_fetch(p.h, pro.w, (size_t)D * pro.k));
            if (f.pws > 0.0f) f.pro = pro.kind;
        }
        if (epi.want && f.pro == pro.kind && ffn_x3_epi_supported(D, T)) {
            f.mscale = f16_mean_scale(f16_ln_bound(p.h, epi.ln_w, epi.ln_b, D));
            f.epi = f.mscale > 0.0f;
        }
    }
    const char* res = rscale == 0.5f ? "0.5res" : "res";
    // allocates, packs and plans form f; false (an allocation or a pack failed): nothing planned, nothing kept
    auto build = [&]() -> bool {
        if (!f.fused) {
            add_ffn_unfused(p, w, ACT_SILU, rscale, hb, t1, big, T, D, name, name + ".linear1+swish", name + ".linear2+" + res);
            return true;
        }
        const int kind = f.pro, pk = kind ? pro.k : 0;
        PlanCtx::Packs packs(p);
        const void* ppk = !kind ? nullptr : packs.pack(ffn_x3_pro_tile_bytes(pk) * ((D + 31) / 32), [&](void* d) { return launch_ffn_x3_pro_pack(pro.w, d, D, pk, f.pws, p.h->own_stream); });
        if (kind && !ppk) return false;
        const void* packed = packs.pack(ffn_x3_packed_bytes(D), [&](void* d) {
            return launch_ffn_x3_pack(w.w1, w.b1, w.w2, d, D, p.h->own_stream, f.h2 ? f.s.fw1 : 0.0f, f.h2 ? f.s.fw2 : 0.0f, kind ? 1 : 0);
        });
        if (!packed) return false;
        packs.commit();
        const float *lw = w.ln_w, *lb = w.ln_b, *b2 = w.b2, *pbias = kind ? pro.b : nullptr, *l2w = epi.ln_w, *l2b = epi.ln_b;
        const float p_un = kind ? 1.0f / f.pws : 1.0f, mscale = f.mscale;
        const bool fepi = f.epi, h2 = f.h2;
        const FfnScales s = f.s;                           // (the launches keep copies: f changes when a build fails)
        // the epilogue's exact partial sums: per 32-row tile two segments x two planes of D floats (the idle wide scratch buffer)
        if (fepi) p.need(big, (size_t)((T + 31) / 32 + 1) * 4 * D + (size_t)16 * D);
        const std::string what = std::string(kind == 1 ? "input_proj+" : kind == 2 ? "conv2(pw)+res+" : "") + "ln+linear1+swish+linear2+" + res + (fepi ? "+layernorm+time sums" : "");
        p.add("ffn_x3:" + name + " (" + what + ")" + (h2 ? " [f16x3]" : ""), [=](Run& r) {
            FfnArgs a{r.buf[hb], lw, lb, static_cast<const unsigned char*>(packed), b2, r.B * T, rscale};
            if (h2) { a.h2_x = s.fx; a.h2_w1 = s.fw1; a.h2_h = s.fh; a.h2_w2 = s.fw2; }
            if (kind) {
                a.px = kind == 1 ? r.x : r.buf[t3]; a.ppacked = static_cast<const unsigned char*>(ppk); a.pb = pbias;
                a.pro_k = pk; a.pro_res = kind == 2 ? 1 : 0; a.p_un = p_un;
            }
            if (fepi) { a.ln2_w = l2w; a.ln2_b = l2b; a.msum = r.buf[big]; a.T = T; a.m_scale = mscale; }
            return launch_ffn_x3(a, D, r.stream);
        });
        if (fepi)
            p.add("mean_finish:" + epi.block + " (time average of the exact tile sums)", [=](Run& r) {
                return launch_ffn_x3_mean_finish(r.buf[big], r.buf[t1], r.B, T, D, mscale, r.stream);
            });
        return true;
    };
    auto separate_pro = [&] { add_linear(p, pro.name, pro.kind == 1 ? BUF_X : t3, hb, T, D, pro.k, pro.w, pro.b, pro.kind == 2 ? hb : BUF_NONE); };
    // the richest form that can be built, one form down after each failed build
    if (pro.kind && !f.pro) separate_pro();
    while (!build()) {
        if (f.epi) f.epi = false;
        else if (f.pro) { f.pro = 0; separate_pro(); }
        else f.fused = false;
    }
    return f.epi;
}

// The ConvolutionModule `m` up to its depthwise stage: LayerNorm + conv1 + GLU (hb -> t1), depthwise + BN + swish (-> t3)
// (the whole module as ONE clip-resident launch was built and measured: bit-identical, 0.27 ms against 0.25 for the three launches
// below - tools/ubench/convmod_x3.hip)
void add_conv_module_front(PlanCtx& p, const std::string& m, int hb, int t1, int t3, int big, int T, int D) {
    const float *lw = p.W(m + ".layer_norm.weight"), *lb = p.W(m + ".layer_norm.bias");
    const float *dw = p.W(m + ".depthwise_conv.weight"), *db = p.W(m + ".depthwise_conv.bias");
    const float *ba = p.W(m + ".batch_norm.alpha"), *bb = p.W(m + ".batch_norm.beta");
    // LayerNorm + pointwise conv1 + GLU in one launch (lin_x3.hip), else the three separate ones
    LinOpts glu; glu.epi = LIN_GLU; glu.ln_w = lw; glu.ln_b = lb;
    if (!add_lin_x3(p, m + ".layer_norm+conv1(pw)+glu", hb, t1, T, D, D, p.W(m + ".conv1.weight"), p.W(m + ".conv1.bias"), glu)) {
        p.add("layernorm:" + m, [=](Run& r) { return launch_layernorm(r.buf[hb], r.buf[t1], lw, lb, r.B * T, D, ACT_NONE, r.stream); });
        add_gemm(p, m + ".conv1(pw)", t1, big, T, 2 * D, D, p.W(m + ".conv1.weight"), p.W(m + ".conv1.bias"), ACT_NONE);
        p.add("glu:" + m, [=](Run& r) { return launch_glu(r.buf[big], r.buf[t1], r.B * T, D, r.stream); });
    }
    p.add("dwconv1d+bn+swish:" + m, [=](Run& r) { return launch_dwconv1d_bn_swish(r.buf[t1], dw, db, ba, bb, r.buf[t3], r.B, T, D, 31, r.stream); });
}

// ------------------------------------------------------------------------------------------ per-head plans
// Each plans the head's body up to its last Linear, which it leaves to plan_tail (set_tail); NWW_OK or the fail() code.

int plan_dnn(PlanCtx& p) {                          // Net: architectures.py:110-126
    const nww_config& c = p.h->cfg;
    const int T = c.in_rows, F = c.in_cols, L = c.layer_dim, nb = c.n_blocks, act = c.activation;
    GemmOpts l1; l1.feeds_ln = true; l1.a_range = F16_FEATURES; l1.a_bound_assumed = true;
    add_gemm(p, "layer1", BUF_X, 0, 1, L, T * F, p.W("model.layer1.weight"), p.W("model.layer1.bias"), ACT_NONE, l1);
    // Everything behind layer1 runs inside the tail's launch (layers.hip: TailArgs::ln0_w) when the widths allow: LayerNorm1 on
    // layer1's split-K partials, the blocks' Linear + LayerNorm, last_layer, classifier - two launches per forward instead of six
    if (nww_knobs().tail && L <= 256 && nb <= 4 && tail_supported(L, c.embedding_dim)) {
        p.dnn.on = true;
        p.dnn.ln0_w = p.W("model.layernorm1.weight"); p.dnn.ln0_b = p.W("model.layernorm1.bias");
        p.dnn.n_mid = nb;
        for (int i = 0; i < nb; ++i) {
            const std::string q = "model.blocks." + std::to_string(i);
            p.dnn.mid[i][0] = p.W(q + ".fcn_layer.weight"); p.dnn.mid[i][1] = p.W(q + ".fcn_layer.bias");
            p.dnn.mid[i][2] = p.W(q + ".layer_norm.weight"); p.dnn.mid[i][3] = p.W(q + ".layer_norm.bias");
        }
        set_tail(p, "layernorm1+blocks+last_layer", 0, L, p.W("model.last_layer.weight"), p.W("model.last_layer.bias"));
        return NWW_OK;
    }
    const float *lw1 = p.W("model.layernorm1.weight"), *lb1 = p.W("model.layernorm1.bias");
    p.add("layernorm:layernorm1", [=](Run& r) {
        if (r.deferred.active && r.deferred.out_id == 0) {           // layer1 left its split-K partials: sum them here
            r.deferred.active = false;
            return launch_layernorm_parts(r.splitk_ws, r.deferred.parts, r.deferred.stride, r.deferred.bias, r.buf[0], lw1, lb1, r.B, L, act, r.stream);
        }
        return launch_layernorm(r.buf[0], r.buf[0], lw1, lb1, r.B, L, act, r.stream);
    });
    int cur = 0;
    for (int i = 0; i < nb; ++i) {
        const std::string q = "model.blocks." + std::to_string(i);
        const int nxt = cur ^ 1;
        add_gemm(p, q + ".fcn_layer", cur, nxt, 1, L, L, p.W(q + ".fcn_layer.weight"), p.W(q + ".fcn_layer.bias"), ACT_NONE);
        const float *lw = p.W(q + ".layer_norm.weight"), *lb = p.W(q + ".layer_norm.bias");
        p.add("layernorm:" + q, [=](Run& r) { return launch_layernorm(r.buf[nxt], r.buf[nxt], lw, lb, r.B, L, act, r.stream); });
        cur = nxt;
    }
    set_tail(p, "last_layer", cur, L, p.W("model.last_layer.weight"), p.W("model.last_layer.bias"));
    return NWW_OK;
}

int plan_cnn(PlanCtx& p) {                          // CNNModel: architectures.py:51-80
    nww_handle* h = p.h;
    const nww_config& c = h->cfg;
    const int T = c.in_rows, F = c.in_cols, act = c.activation;
    // trunk -> fc1 hand-over as the GEMM's own A tiles when both run on the split-operand path and the geometry allows
    // 16-byte stores inside a 32-feature tile row
    const int H2 = T / 4, W2 = F / 4;
    h->trunk_blocked = (h->conv_products == 6 || h->conv_products == 9) && trunk_b_pick_strips(T, F) > 0 &&
                       (W2 % 4) == 0 && ((H2 * W2) % 4) == 0 && ((32 * H2 * W2) % 32) == 0;
    F16Range a2_bound;                    // NWW_ARITH_F16X3: the range of the trunk's output, fc1's operand
    TrunkOpts to; to.out_blocked = &h->trunk_blocked; to.in_range = F16_FEATURES; to.out_range = &a2_bound;
    const bool fused = add_trunk(p, "conv1+pool+conv2+pool", BUF_X, 1, 16, 32, T, F, p.W("model.conv1.weight"), p.W("model.conv1.bias"), nullptr, nullptr,
                                 p.W("model.conv2.weight"), p.W("model.conv2.bias"), nullptr, nullptr, act, to);
    if (!fused) {
        h->trunk_blocked = false;
        add_conv(p, "conv1", BUF_X, 0, 1, 16, T, F, p.W("model.conv1.weight"), p.W("model.conv1.bias"), nullptr, nullptr, act, 1);
        add_conv(p, "conv2", 0, 1, 16, 32, T / 2, F / 2, p.W("model.conv2.weight"), p.W("model.conv2.bias"), nullptr, nullptr, act, 1);
    }
    // fc1's split-K partials are reduced by the classifier tail itself when that is the fused kernel
    GemmOpts fc1; fc1.a_blocked_inout = &h->trunk_blocked; fc1.feeds_tail = nww_knobs().tail && tail_supported(128, c.embedding_dim); fc1.a_range = a2_bound;
    add_gemm(p, "fc1", 1, 0, 1, 128, 32 * H2 * W2, p.W("model.fc1.weight"), p.W("model.fc1.bias"), act, fc1);
    set_tail(p, "fc2", 0, 128, p.W("model.fc2.weight"), p.W("model.fc2.bias"));
    return NWW_OK;
}

// The E2E head on the transposed plane (e2e_transposed_ok); whatever goes wrong while it is built (a shape one of its kernels does
// not take after all, an allocation) drops what was planned, and plan_e2e_dnn falls back to the reference's orientation
bool plan_e2e_dnn_transposed(PlanCtx& p) {
    nww_handle* h = p.h;
    const int Hh = h->cfg.in_rows, Ww = h->cfg.in_cols, act = h->cfg.activation;     // (n_mels, frames)
    if (!e2e_transposed_ok(p, Hh, Ww)) return false;
    const size_t steps_before = h->plan.size();
    const int Ht = Ww, Wt = Hh;       // the plane the kernels see: (frames, n_mels)
    // the three filters with their taps transposed (transpose_e2e_filters, nww_weights.hip)
    const float* wts[3] = {p.W("model.conv_block.0.weight_t"), p.W("model.conv_block.4.weight_t"), p.W("model.conv_block.8.weight_t")};
    if (!wts[0] || !wts[1] || !wts[2]) return false;
    h->e2e_transposed = true;
    p.need(2, (size_t)Hh * Ww);
    p.add("transpose:mel-major features -> frames-major (skipped after the frontend)", [=](Run& r) {
        if (r.x_frames_major) return hipSuccess;
        const hipError_t e = launch_transpose_planes(r.x, r.buf[2], r.B, Hh, Ww, r.stream);
        r.x = r.buf[2];
        return e;
    });
    const int h3 = Ht / 4, w3 = Wt / 4;           // (25, 16): AdaptiveAvgPool2d((1,4))'s windows run along the FRAMES, here y
    const int sw4 = h3 / 4, kw4 = h3 - 3 * sw4;
    F16Range tbound;                              // NWW_ARITH_F16X3: the range of the trunk's output, the third conv's operand
    TrunkOpts to; to.in_range = F16_FEATURES; to.out_range = &tbound;
    auto undo = [&] { h->plan.resize(steps_before); h->e2e_transposed = false; return false; };
    if (!(add_trunk(p, "conv_block.0-7 (transposed plane)", BUF_X, 1, 16, 32, Ht, Wt, wts[0], p.W("model.conv_block.0.bias"),
                    p.W("model.conv_block.1.alpha"), p.W("model.conv_block.1.beta"), wts[1], p.W("model.conv_block.4.bias"),
                    p.W("model.conv_block.5.alpha"), p.W("model.conv_block.5.beta"), act, to) &&
          h->plan.back().name.rfind("trunk_x3:", 0) == 0 && h3 >= 4)) return undo();
    ConvMfmaOpts co; co.avg_kw = kw4; co.avg_sw = sw4; co.avg_ow = 4; co.avg_y = 1; co.in_range = tbound;
    if (!add_conv_mfma(p, "model.conv_block.8 (transposed plane)", 1, 0, 32, 64, h3, w3, wts[2], p.W("model.conv_block.8.bias"),
                       p.W("model.conv_block.9.alpha"), p.W("model.conv_block.9.beta"), act, 0, co)) return undo();
    GemmOpts bn1; bn1.alpha = p.W("model.bn1.alpha"); bn1.beta = p.W("model.bn1.beta");
    add_gemm(p, "fc1+bn1", 0, 1, 1, 128, 256, p.W("model.fc1.weight"), p.W("model.fc1.bias"), act, bn1);
    set_tail(p, "out", 1, 128, p.W("model.out.weight"), p.W("model.out.bias"));
    return true;
}

int plan_e2e_dnn(PlanCtx& p) {                      // E2E_MelSpectrogram_CNN body: architectures.py:840-865,877-889
    if (plan_e2e_dnn_transposed(p)) return NWW_OK;
    nww_handle* h = p.h;
    const int Hh = h->cfg.in_rows, Ww = h->cfg.in_cols, act = h->cfg.activation;     // (n_mels, frames)
    const int ch[3] = {16, 32, 64};
    int cin = 1, hh = Hh, ww = Ww, cur = BUF_X;
    int first = 0;
    bool fused_pool = false;
    F16Range cbound;                                  // NWW_ARITH_F16X3: range of the current stage's input (empty: unknown)
    TrunkOpts to; to.in_range = F16_FEATURES; to.out_range = &cbound;
    if (add_trunk(p, "conv_block.0-7", BUF_X, 1, 16, 32, Hh, Ww, p.W("model.conv_block.0.weight"), p.W("model.conv_block.0.bias"),
                  p.W("model.conv_block.1.alpha"), p.W("model.conv_block.1.beta"), p.W("model.conv_block.4.weight"),
                  p.W("model.conv_block.4.bias"), p.W("model.conv_block.5.alpha"), p.W("model.conv_block.5.beta"), act, to)) {
        first = 2; cin = 32; hh = Hh / 4; ww = Ww / 4; cur = 1;
    }
    for (int i = first; i < 3; ++i) {
        const std::string cw = "model.conv_block." + std::to_string(4 * i), bnp = "model.conv_block." + std::to_string(4 * i + 1);
        const int out = (i % 2 == 0) ? 0 : 1;
        if (i == 2 && ww >= 4) {
            // conv3 + AdaptiveAvgPool2d((1,4)) in its exported AvgPool2d form, fused when the MFMA kernel applies
            ConvMfmaOpts po; po.avg_sw = ww / 4; po.avg_kw = ww - 3 * po.avg_sw; po.avg_ow = 4; po.in_range = cbound;
            if (add_conv_mfma(p, cw, cur, out, cin, ch[i], hh, ww, p.W(cw + ".weight"), p.W(cw + ".bias"), p.W(bnp + ".alpha"), p.W(bnp + ".beta"), act, 0, po)) {
                fused_pool = true; cin = ch[i]; cur = out;
                continue;
            }
        }
        F16Range nb;
        ConvMfmaOpts co; co.in_range = cbound; co.out_range = &nb;
        if (!add_conv_mfma(p, cw, cur, out, cin, ch[i], hh, ww, p.W(cw + ".weight"), p.W(cw + ".bias"), p.W(bnp + ".alpha"), p.W(bnp + ".beta"), act, i < 2, co))
            add_conv(p, cw, cur, out, cin, ch[i], hh, ww, p.W(cw + ".weight"), p.W(cw + ".bias"), p.W(bnp + ".alpha"), p.W(bnp + ".beta"), act, i < 2);
        cbound = nb;
        if (i < 2) { hh /= 2; ww /= 2; }
        cin = ch[i]; cur = out;
    }
    if (hh < 1 || ww < 4) return fail(h, NWW_ERR_INVALID, "e2e_dnn input too small for AdaptiveAvgPool2d((1,4))");
    // AdaptiveAvgPool2d((1,4)) in its exported AvgPool2d form (_export/onnx.py:146-152)
    const int sh = hh / 1, kh = hh, sw = ww / 4, kw = ww - 3 * sw;
    int fc_in = cur;                                  // buffer holding [B][256] after the pool
    if (!fused_pool) {
        const int pin = cur, pout = cur ^ 1;
        p.need(pout, 256);
        p.add("avgpool:export(1,4)", [=](Run& r) { return launch_avgpool(r.buf[pin], r.buf[pout], r.B * 64, hh, ww, kh, kw, sh, sw, 1, 4, r.stream); });
        fc_in = pout;
    }
    const int fc_out = fc_in ^ 1;
    GemmOpts bn1; bn1.alpha = p.W("model.bn1.alpha"); bn1.beta = p.W("model.bn1.beta");
    add_gemm(p, "fc1+bn1", fc_in, fc_out, 1, 128, 256, p.W("model.fc1.weight"), p.W("model.fc1.bias"), act, bn1);
    set_tail(p, "out", fc_out, 128, p.W("model.out.weight"), p.W("model.out.bias"));
    return NWW_OK;
}

int plan_crnn(PlanCtx& p) {                         // CRNNModel: architectures.py:209-287
    nww_handle* h = p.h;
    const nww_config& c = h->cfg;
    const int T = c.in_rows, F = c.in_cols, L = c.layer_dim, nb = c.n_blocks, act = c.activation;
    int cin = 1, hh = T, ww = F, cur = BUF_X;
    int first = 0;
    bool seq_written = false;
    F16Range cbound;                                  // NWW_ARITH_F16X3: range of the current stage's input (empty: unknown)
    const size_t steps_before = h->plan.size();
    TrunkOpts to; to.in_range = F16_FEATURES; to.out_range = &cbound;
    if (c.n_crnn_channels >= 2 && c.crnn_channels[0] == 16 && c.crnn_channels[1] == 32 &&
        add_trunk(p, "cnn.0-7", BUF_X, 1, 16, 32, T, F, p.W("model.cnn.0.weight"), p.W("model.cnn.0.bias"), p.W("model.cnn.1.alpha"),
                  p.W("model.cnn.1.beta"), p.W("model.cnn.4.weight"), p.W("model.cnn.4.bias"), p.W("model.cnn.5.alpha"),
                  p.W("model.cnn.5.beta"), act, to)) {
        first = 2; cin = 32; hh = T / 4; ww = F / 4; cur = 1;
    }
    for (int i = first; i < c.n_crnn_channels; ++i) {
        const std::string cw = "model.cnn." + std::to_string(4 * i), bnp = "model.cnn." + std::to_string(4 * i + 1);
        const int out = (i % 2 == 0) ? 0 : 1;
        // the last conv stage may write the recurrent layers' [W][C * H] sequence layout itself (conv3_x3.hip)
        bool seq = i == c.n_crnn_channels - 1;
        // the stage right behind a fused split-operand trunk may take its input from the streaming rings (nww_stream.hip)
        bool ring = i == 2 && first == 2 && h->plan.size() == steps_before + 1 && h->plan.back().name.rfind("trunk_x3:", 0) == 0 && ((F / 4) % 4) == 0;
        F16Range nbr;
        ConvMfmaOpts co; co.seq_inout = &seq; co.ring_in = &ring; co.in_range = cbound; co.out_range = &nbr;
        co.scratch_id = 2;                                // the recurrent layers' xg buffer, idle until they run
        const bool mf = add_conv_mfma(p, cw, cur, out, cin, c.crnn_channels[i], hh, ww, p.W(cw + ".weight"), p.W(cw + ".bias"), p.W(bnp + ".alpha"), p.W(bnp + ".beta"), act, 1, co);
        cbound = nbr;
        if (!mf) {
            ring = false;
            seq = false;
            add_conv(p, cw, cur, out, cin, c.crnn_channels[i], hh, ww, p.W(cw + ".weight"), p.W(cw + ".bias"), p.W(bnp + ".alpha"), p.W(bnp + ".beta"), act, 1);
        }
        if (ring) {
            h->stream_conv = true; h->stream_H = T; h->stream_W = F;
            h->stream_seq = seq && i == c.n_crnn_channels - 1;
            h->seq_floats = (size_t)c.crnn_channels[i] * (hh / 2) * (ww / 2);
        }
        seq_written = seq;
        hh /= 2; ww /= 2; cin = c.crnn_channels[i]; cur = out;
    }
    if (hh < 1 || ww < 1) return fail(h, NWW_ERR_INVALID, "crnn input too small for the conv stack");
    const int seq = seq_written ? cur : cur ^ 1, C = cin, Hc = hh, Wc = ww;
    if (!seq_written) {
        p.need(seq, (size_t)C * Hc * Wc);
        p.add("crnn_seq", [=](Run& r) { return launch_crnn_seq(r.buf[cur], r.buf[seq], r.B, C, Hc, Wc, r.stream); });
    }
    add_bigru_last(p, "model.rnn", seq, Wc, C * Hc, L, nb, 2, seq ^ 1, 3, 4, c.crnn_rnn_lstm ? 4 : 3);      // seq ^ 1: the free one of buffers 0 / 1
    set_tail(p, "fc", 4, 2 * L, p.W("model.fc.weight"), p.W("model.fc.bias"));
    return NWW_OK;
}

int plan_gru(PlanCtx& p) {                          // GRUModel: architectures.py:129-145
    const nww_config& c = p.h->cfg;
    add_bigru_last(p, "model.gru", BUF_X, c.in_rows, c.in_cols, c.layer_dim, c.n_blocks, 2, 0, 1, 4);
    set_tail(p, "fc", 4, 2 * c.layer_dim, p.W("model.fc.weight"), p.W("model.fc.bias"));
    return NWW_OK;
}

int plan_rnn(PlanCtx& p) {                          // RNNModel: architectures.py:149-161 (bidirectional nn.LSTM, hidden size 64 whatever layer_dim says)
    const nww_config& c = p.h->cfg;
    add_bigru_last(p, "model.layer1", BUF_X, c.in_rows, c.in_cols, 64, c.n_blocks, 2, 0, 1, 4, 4);
    set_tail(p, "layer2", 4, 128, p.W("model.layer2.weight"), p.W("model.layer2.bias"));
    return NWW_OK;
}

int plan_bcresnet(PlanCtx& p) {                     // BcResNetModel: architectures.py:620-687, channels-last on the GPU
    nww_handle* h = p.h;
    const nww_config& c = h->cfg;
    const int T = c.in_rows, F = c.in_cols, act = c.activation;
    // init conv (+BN+act+pool) writes [B][H1][W1][32]; each block: one depthwise kernel emits d = dw3x3(x) and
    // xs = x at the strided centres, then two MFMA GEMMs over M = B*Ho*Wo pixels:
    //   R = BN_s(xs . Wsc^T) ;  out = act(BN_1(d . Wpw^T)) + R      (activation BEFORE the residual add, :646-647)
    const int ic_mfma = nww_knobs().conv_mfma;
    // init conv fused with block1's depthwise (trunk.hip: the 32-channel planes never reach HBM)
    const int bc_front = nww_knobs().bc_front;
    const bool front_fused = ic_mfma && bc_front && conv1_pool_nhwc_mfma_fits(T, F) && conv1_pool_dw_rows(T, F, 2) > 0;
    // nww_config.act_dtype = NWW_ACT_DTYPE_BF16 / _F16: every activation tensor between the kernels of this head is stored in 16
    // bits (arithmetic and accumulation stay float32); implemented on the fused front + split-operand block path only.
    // binary16 (11 significant bits against bf16's 8) stores value x a power of two fixed here from a bound on the tensor
    // (features within +-NWW_F16_FEATURE_BOUND as in the f16x3 arithmetic; the bound is not allowed to sit more than 2^16 above
    // the tensor's typical magnitude, and the stores saturate), and a block's weights are two binary16 terms of weight x scale.
    const int act16 = c.act_dtype;                       // NWW_ACT_DTYPE_* == ACT16_* (split_h2.h)
    const bool act_bf16 = act16 != NWW_ACT_DTYPE_F32;    // any 16-bit storage
    const bool act_f16 = act16 == NWW_ACT_DTYPE_F16;
    if (act_bf16 && !(front_fused && p.h->conv_products == 6))
        return fail(h, NWW_ERR_UNSUPPORTED, "act_dtype = bf16 / f16 needs the fused BcResNet front kernel and a split-operand conv_arith for this input shape");
    float s_h[4] = {1.f, 1.f, 1.f, 1.f}, s_d[4] = {1.f, 1.f, 1.f, 1.f};     // scales of h_i (block i's output, h_0 = init conv) and d_i
    DualPackScales dps[4];
    if (act_f16) {
        auto cap = [](F16Range r) { return f16_scale(std::fmin(r.bound, r.typ * 65536.0)); };
        auto dw_range = [&](const float* wt, int C, F16Range in) {      // wt [9][C] tap-major
            const auto w = f16_fetch(p.h, wt, (size_t)9 * C);
            double worst = 0, typ = 0;
            for (int ch = 0; ch < C; ++ch) {
                double l1 = 0, l2 = 0;
                for (int k = 0; k < 9; ++k) { const double v = w[(size_t)k * C + ch]; l1 += std::fabs(v); l2 += v * v; }
                worst = std::fmax(worst, l1); typ += std::sqrt(l2);
            }
            return F16Range{worst * in.bound, typ / C * in.typ};
        };
        const auto hw0 = f16_fetch(p.h, p.W("model.init_conv.0.weight"), 32 * 9);
        const float *pa0 = p.W("model.init_conv.1.alpha"), *pb0 = p.W("model.init_conv.1.beta");
        const auto ha0 = f16_fetch(p.h, pa0, 32), hb0 = f16_fetch(p.h, pb0, 32);
        F16Range rh{f16_layer_bound(hw0, 32, 9, hb0, false, ha0, hb0, pa0 != nullptr, F16_FEATURES.bound),
                    f16_layer_typ(hw0, 32, 9, ha0, pa0 != nullptr, F16_FEATURES.typ)};
        s_h[0] = cap(rh);
        const int chs[4] = {32, 64, 128, 256};
        for (int i = 1; i <= 3; ++i) {
            const std::string q = "model.block" + std::to_string(i);
            const int ci = chs[i - 1], co = chs[i];
            const F16Range rd = dw_range(p.W(q + ".depthwise.weight_t"), ci, rh);
            s_d[i] = cap(rd);
            const float *pa1 = p.W(q + ".bn1.alpha"), *pas = p.W(q + ".shortcut.1.alpha");
            const auto wpw = f16_fetch(p.h, p.W(q + ".pointwise.weight"), (size_t)co * ci), wsc = f16_fetch(p.h, p.W(q + ".shortcut.0.weight"), (size_t)co * ci);
            const auto ha1 = f16_fetch(p.h, pa1, co), hb1 = f16_fetch(p.h, p.W(q + ".bn1.beta"), co);
            const auto has = f16_fetch(p.h, pas, co), hbs = f16_fetch(p.h, p.W(q + ".shortcut.1.beta"), co);
            dps[i].pw_ws = f16_wscale(wpw); dps[i].sc_ws = f16_wscale(wsc);
            if (!(s_d[i] > 0.f && s_h[i - 1] > 0.f && dps[i].pw_ws > 0.f && dps[i].sc_ws > 0.f))
                return fail(h, NWW_ERR_UNSUPPORTED, "act_dtype = f16: no finite bound on the tensors of block %d", i);
            dps[i].pw_un = 1.0f / (dps[i].pw_ws * s_d[i]); dps[i].sc_un = 1.0f / (dps[i].sc_ws * s_h[i - 1]);
            const F16Range rpw{f16_layer_bound(wpw, co, ci, hb1, false, ha1, hb1, pa1 != nullptr, rd.bound), f16_layer_typ(wpw, co, ci, ha1, pa1 != nullptr, rd.typ)};
            const F16Range rsc{f16_layer_bound(wsc, co, ci, hbs, false, has, hbs, pas != nullptr, rh.bound), f16_layer_typ(wsc, co, ci, has, pas != nullptr, rh.typ)};
            rh = F16Range{rpw.bound + rsc.bound, std::hypot(rpw.typ, rsc.typ)};
            s_h[i] = cap(rh);
        }
    }
    if (front_fused) {
        const float *w0 = p.W("model.init_conv.0.weight"), *a0 = p.W("model.init_conv.1.alpha"), *b0 = p.W("model.init_conv.1.beta");
        const float* dwt1 = p.W("model.block1.depthwise.weight_t");
        const int ho1 = (T / 2 - 1) / 2 + 1, wo1 = (F / 2 - 1) / 2 + 1;
        p.need(2, (size_t)32 * ho1 * wo1); p.need(3, (size_t)32 * ho1 * wo1);
        const int max_grid = p.h->cu_count;
        // the convolution from split operands on the bf16 matrix cores (trunk_b.hip) under the handle's arithmetic switch;
        // NWW_BC_FRONT = 2 keeps the float32-MFMA kernel
        int fprod = p.h->conv_products;
        // under NWW_ARITH_F16X3 (BN present): two binary16 terms per operand, features clamped to +-NWW_F16_FEATURE_BOUND as in the
        // CNN trunk
        float fin = 0.0f, fws = 1.0f;
        if (p.h->f16 && fprod == 6 && a0 && bc_front != 2) {
            fin = f16_scale(F16_FEATURES.bound); fws = f16_wscale(f16_fetch(p.h, w0, 32 * 9));
            if (fin > 0.0f && fws > 0.0f) fprod = 3;
        }
        void* fpack = nullptr;
        if ((fprod == 6 || fprod == 9 || fprod == 3) && bc_front != 2 && bc_front_b_rows(T, F, 2) > 0)
            fpack = p.pack_one(bc_front_b_packed_bytes(), [&](void* d) {
                return fprod == 3 ? launch_bc_front_b_pack_f16(w0, static_cast<unsigned char*>(d), fws, p.h->own_stream)
                                  : launch_bc_front_b_pack(w0, static_cast<unsigned char*>(d), p.h->own_stream);
            });
        const float f_un = 1.0f / (fin > 0.0f ? fin * fws : 1.0f);
        // all folded-BN factors non-negative (the usual case: gamma > 0): max-pool commutes with BN + ReLU through the maximum alone
        const int bn_pos = a0 && f16_all_nonneg(p.h, a0, 32);
        if (fpack) p.h->clamps_features = true;
        p.add(std::string(fpack ? "conv1_dw_x3" : "conv1_dw_mfma") + ":init_conv + block1.depthwise (nhwc" + (act_f16 ? ", f16 out)" : act_bf16 ? ", bf16 out)" : ")") + (fpack && fprod == 3 ? " [f16x3]" : ""), [=](Run& r) {
            Conv1DwArgs a{r.x, w0, nullptr, a0, b0, dwt1, r.buf[2], r.buf[3], r.B, T, F, act, 2, 2};
            a.bf16_out = act16; a.d_scale = s_d[1]; a.xs_scale = s_h[0];
            if (fpack) {
                a.wpack = static_cast<const unsigned char*>(fpack);
                a.f16_in = fin; a.f16_clamp = NWW_F16_FEATURE_BOUND; a.f16_unscale = f_un; a.bn_pos = bn_pos;
                return launch_bc_front_b(a, fprod, max_grid, r.stream);
            }
            return launch_conv1_pool_dw_nhwc(a, max_grid, r.stream);
        });
    } else if (ic_mfma && conv1_pool_nhwc_mfma_fits(T, F)) {
        const float *w0 = p.W("model.init_conv.0.weight"), *a0 = p.W("model.init_conv.1.alpha"), *b0 = p.W("model.init_conv.1.beta");
        p.need(0, (size_t)32 * (T / 2) * (F / 2));
        const int max_grid = p.h->cu_count;
        p.add("conv1_mfma:init_conv(nhwc)", [=](Run& r) {
            Conv1NhwcArgs a{r.x, w0, nullptr, a0, b0, r.buf[0], r.B, T, F, act};
            return launch_conv1_pool_nhwc_mfma(a, max_grid, r.stream);
        });
    } else {
        add_conv(p, "init_conv(nhwc)", BUF_X, 0, 1, 32, T, F, p.W("model.init_conv.0.weight"), nullptr, p.W("model.init_conv.1.alpha"), p.W("model.init_conv.1.beta"), act, 1, 1);
    }
    int hh = T / 2, ww = F / 2, cur = 0;
    bool mean_fused = false;
    const int ch[4] = {32, 64, 128, 256};
    // float32 activations under NWW_ARITH_F16X3: a block's d and xs rows are scaled per pixel in the kernel and its weights per tensor, which
    // needs no bound - but a channel (or its weight column) far off its neighbours loses bits (f16_pixel_rows_ok, plan_host.h).  ReLU models
    // were balanced at load time (balance_channel_gains); what is still spread here - GELU / SiLU BatchNorm gains - sends the block to the
    // three-term bf16 form, unchained.  Per-channel typical magnitudes as in add_trunk (f16_rows_typ), the two branches of a block by hypot
    bool h2_ok[4] = {false, true, true, true};
    if (p.h->f16 && !act_bf16) {
        const std::vector<float> none;
        const float *pa0 = p.W("model.init_conv.1.alpha"), *pb0 = p.W("model.init_conv.1.beta");
        const auto hw0 = f16_fetch(p.h, p.W("model.init_conv.0.weight"), 32 * 9);
        const auto ha0 = f16_fetch(p.h, pa0, 32), hb0 = f16_fetch(p.h, pb0, 32);
        const F16Rows m0 = f16_rows_moments(32, 9, [&](int q, int co) { return hw0[(size_t)co * 9 + q]; }, [](int) { return 0; }, std::vector<double>(1, F16_FEATURES.typ));
        std::vector<double> typ_h = f16_rows_typ(m0, none, false, ha0, hb0, pa0 != nullptr);
        for (int i = 1; i <= 3; ++i) {
            const std::string q = "model.block" + std::to_string(i);
            const int ci = ch[i - 1], co = ch[i];
            const auto dwt = f16_fetch(p.h, p.W(q + ".depthwise.weight_t"), (size_t)9 * ci);      // [9][ci] tap-major
            std::vector<double> typ_d(ci, 0.0);
            for (int cc = 0; cc < ci; ++cc) {
                double l2 = 0;
                for (int k = 0; k < 9; ++k) l2 += (double)dwt[(size_t)k * ci + cc] * (double)dwt[(size_t)k * ci + cc];
                typ_d[cc] = std::sqrt(l2) * typ_h[cc];
            }
            const float *pa1 = p.W(q + ".bn1.alpha"), *pas = p.W(q + ".shortcut.1.alpha");
            const auto wpw = f16_fetch(p.h, p.W(q + ".pointwise.weight"), (size_t)co * ci), wsc = f16_fetch(p.h, p.W(q + ".shortcut.0.weight"), (size_t)co * ci);
            const auto ha1 = f16_fetch(p.h, pa1, co), hb1 = f16_fetch(p.h, p.W(q + ".bn1.beta"), co);
            const auto has = f16_fetch(p.h, pas, co), hbs = f16_fetch(p.h, p.W(q + ".shortcut.1.beta"), co);
            const F16Rows mpw = f16_rows_moments(co, ci, [&](int k, int o) { return wpw[(size_t)o * ci + k]; }, [](int k) { return k; }, typ_d);
            const F16Rows msc = f16_rows_moments(co, ci, [&](int k, int o) { return wsc[(size_t)o * ci + k]; }, [](int k) { return k; }, typ_h);
            h2_ok[i] = f16_pixel_rows_ok(mpw, typ_d) && f16_pixel_rows_ok(msc, typ_h);
            const std::vector<double> tpw = f16_rows_typ(mpw, none, false, ha1, hb1, pa1 != nullptr), tsc = f16_rows_typ(msc, none, false, has, hbs, pas != nullptr);
            typ_h.assign(co, 0.0);
            for (int o = 0; o < co; ++o) typ_h[o] = std::hypot(tpw[o], tsc[o]);
        }
    }
    const int st[3][2] = {{2, 2}, {2, 2}, {2, 1}};
    // d_i / xs_i (depthwise output and strided block input) of the coming block live in buffers dwb / xsb; have_dx: they are
    // already there - written by the fused front kernel or by the previous block's chained kernel (bc_chain.hip)
    int dwb = 2, xsb = 3;
    bool have_dx = front_fused;
    for (int i = 1; i <= 3; ++i) {
        const std::string q = "model.block" + std::to_string(i);
        const int ci = ch[i - 1], co = ch[i], sh = st[i - 1][0], sw = st[i - 1][1];
        const int ho = (hh - 1) / sh + 1, wo = (ww - 1) / sw + 1;
        int outb = 4;
        for (int cand : {0, 1, 4})
            if (cand != cur && cand != dwb && cand != xsb) { outb = cand; break; }
        p.need(dwb, (size_t)ci * ho * wo); p.need(xsb, (size_t)ci * ho * wo);
        const float* dwt = p.W(q + ".depthwise.weight_t");
        const int hin = hh, win = ww;
        if (!have_dx)
            p.add("dwconv3x3_nhwc:" + q, [=](Run& r) { return launch_dwconv3x3_nhwc(r.buf[cur], dwt, r.buf[dwb], r.buf[xsb], r.B, ci, hin, win, sh, sw, r.stream); });
        // one dual GEMM per block: shortcut and pointwise products in the same workgroup, no residual round trip
        {
            const float *wpw = p.W(q + ".pointwise.weight"), *a1 = p.W(q + ".bn1.alpha"), *b1 = p.W(q + ".bn1.beta");
            const float *wsc = p.W(q + ".shortcut.0.weight"), *as = p.W(q + ".shortcut.1.alpha"), *bs = p.W(q + ".shortcut.1.beta");
            const int rows = ho * wo;
            p.need(outb, (size_t)rows * co);
            // both products from split operands on the bf16 matrix cores (dual_x3.hip) under the same arithmetic switch
            // float32 activations under NWW_ARITH_F16X3: two binary16 terms per operand, the activation rows scaled per pixel in
            // the kernel (DualArgs::h2) - no tensor bound needed, the spread of the channels held by h2_ok above
            const bool dual_h2 = p.h->f16 && !act_bf16 && h2_ok[i];
            // blocks 1 and 2 chained with the next block's depthwise (bc_chain.hip; two-term weights in every storage mode)
            const bool will_chain = nww_knobs().bc_chain && i < 3 && have_dx && bc_chain_supported(ci, ho, wo) &&
                                    (act_f16 || dual_h2 || (act16 == NWW_ACT_DTYPE_BF16 && p.h->f16));
            if (dual_h2 || (will_chain && !act_f16)) {
                dps[i].pw_ws = f16_wscale(f16_fetch(p.h, wpw, (size_t)co * ci)); dps[i].sc_ws = f16_wscale(f16_fetch(p.h, wsc, (size_t)co * ci));
                if (!(dps[i].pw_ws > 0.f && dps[i].sc_ws > 0.f)) return fail(h, NWW_ERR_INVALID, "block %d: non-finite weights", i);
                dps[i].pw_un = 1.0f / dps[i].pw_ws; dps[i].sc_un = 1.0f / dps[i].sc_ws;
            }
            const int terms = act_f16 || dual_h2 || will_chain ? 2 : 3;
            if (p.h->conv_products == 6 && dual_x3_supported(ci, co)) {
                if (void* packed = p.pack_one(dual_x3_packed_bytes(ci, co, terms), [&](void* d) { return launch_dual_x3_pack(wpw, wsc, a1, b1, as, bs, d, ci, co, p.h->own_stream, terms, dps[i]); })) {
                    // when the block input is in HBM (every block but the one whose depthwise ran inside the fused front kernel) the
                    // shortcut rows are gathered from it and the depthwise kernel planned just above writes no copy of them
                    const bool gather = !have_dx;
                    if (gather) {
                        const float dw_mul = s_d[i] / s_h[i - 1];
                        p.pop_last();
                        p.add("dwconv3x3_nhwc:" + q, [=](Run& r) { return launch_dwconv3x3_nhwc(r.buf[cur], dwt, r.buf[dwb], nullptr, r.B, ci, hin, win, sh, sw, r.stream, act16, dw_mul); });
                    }
                    // blocks 1 and 2 chained with the next block's depthwise (bc_chain.hip): the block's output stays in LDS, the
                    // next block finds its d / xs rows in the other buffer pair
                    const char* suffix = act_f16 ? " (f16 activations)" : act_bf16 ? " (bf16 activations)" : dual_h2 ? " [f16x3]" : "";
                    if (will_chain) {
                        const std::string qn = "model.block" + std::to_string(i + 1);
                        const float* dwn = p.W(qn + ".depthwise.weight_t");
                        const int sh2 = st[i][0], sw2 = st[i][1], ho2 = (ho - 1) / sh2 + 1, wo2 = (wo - 1) / sw2 + 1;
                        const int odb = dwb == 2 ? 0 : 2, oxb = odb + 1, idb = dwb, ixb = xsb;
                        p.need(odb, (size_t)co * ho2 * wo2); p.need(oxb, (size_t)co * ho2 * wo2);
                        const float d_mul = s_d[i + 1], xs_mul = s_h[i];
                        const int max_grid = p.h->cu_count;
                        p.add("bc_chain:" + q + ".pointwise+bn+act + shortcut+bn -> " + qn + ".depthwise" + suffix, [=](Run& r) {
                            ChainArgs a{r.buf[idb], r.buf[ixb], r.buf[odb], r.buf[oxb], static_cast<const unsigned char*>(packed), dwn,
                                        r.B, ho, wo, sh2, sw2, ho2, wo2};
                            a.act16 = act16; a.d_mul = d_mul; a.xs_mul = xs_mul;
                            return launch_bc_chain(a, ci, act, max_grid, r.stream);
                        });
                        hh = ho; ww = wo; dwb = odb; xsb = oxb; have_dx = true;
                        continue;
                    }
                    // the last block feeds only the global average pool: averaged in the same launch, its output never reaches HBM
                    const bool fuse_mean = i == 3 && ci == 128 && dual_x3_mean_supported(rows);
                    if (fuse_mean) { mean_fused = true; p.need(5, 256); }
                    const float out_mul = fuse_mean ? 1.0f : s_h[i];
                    p.add(std::string(gather ? "dual_x3(xs gathered):" : "dual_x3:") + q + ".pointwise+bn+act + shortcut+bn" + (fuse_mean ? " + global_avg_pool" : "") + suffix, [=](Run& r) {
                        DualArgs a{r.buf[dwb], r.buf[xsb], r.buf[outb], static_cast<const unsigned char*>(packed), r.B * rows, co};
                        if (gather) { a.x = r.buf[cur]; a.H = hin; a.W = win; a.Ho = ho; a.Wo = wo; a.sh = sh; a.sw = sw; }
                        a.act16 = act16; a.out_mul = out_mul; a.h2 = dual_h2 ? 1 : 0;
                        if (fuse_mean) { a.mean_out = r.buf[5]; a.mean_P = rows; }
                        return launch_dual_x3(a, ci, act, r.stream);
                    });
                    hh = ho; ww = wo; cur = outb; have_dx = false; dwb = 2; xsb = 3;
                    continue;
                }
            }
            if (act_bf16) return fail(h, NWW_ERR_UNSUPPORTED, "act_dtype = bf16 / f16: block %d has no split-operand kernel (channels %d -> %d)", i, ci, co);
            p.add("gemm2:" + q + ".pointwise+bn+act + shortcut+bn", [=](Run& r) {
                GemmArgs g;
                g.A = r.buf[dwb]; g.lda = ci; g.W = wpw; g.K = ci; g.alpha = a1; g.beta = b1; g.bias = nullptr; g.act = act;
                g.A2 = r.buf[xsb]; g.lda2 = ci; g.W2 = wsc; g.K2 = ci; g.alpha2 = as; g.beta2 = bs;
                g.C = r.buf[outb]; g.ldc = co; g.M = r.B * rows; g.N = co;
                g.res = nullptr; g.ldres = 0; g.rscale = 1.0f;
                return launch_gemm(g, r.stream);
            });
            }
        hh = ho; ww = wo; cur = outb; have_dx = false; dwb = 2; xsb = 3;
    }
    const int hw = hh * ww;
    if (mean_fused) {
        set_tail(p, "fc", 5, 256, p.W("model.fc.weight"), p.W("model.fc.bias"));
        return NWW_OK;
    }
    p.need(2, 256);
    const float mean_un = act_f16 ? 1.0f / s_h[3] : 1.0f;
    p.add("mean:global_avg_pool", [=](Run& r) { return launch_mean_mid(r.buf[cur], r.buf[2], r.B, hw, 256, r.stream, act16, mean_un); });
    set_tail(p, "fc", 2, 256, p.W("model.fc.weight"), p.W("model.fc.bias"));
    return NWW_OK;
}

int plan_conformer(PlanCtx& p) {                    // ConformerModel: architectures.py:441-543
    const nww_config& c = p.h->cfg;
    const int T = c.in_rows, F = c.in_cols, nb = c.n_blocks;
    const int D = c.conformer_d_model, NH = c.conformer_n_head;
    const int hb = 0, t1 = 1, t3 = 2, big = 3;      // h, LN/glu/attn scratch, dwconv scratch, wide scratch
    bool last_fused = false;
    p.need(t1, (size_t)T * D); p.need(t3, (size_t)T * D);
    p.need(hb, (size_t)T * D);
    for (int i = 0; i < nb; ++i) {
        const std::string q = "model.conformer_blocks." + std::to_string(i), m = q + ".conv_module";
        const float *l2w = p.W(q + ".layer_norm.weight"), *l2b = p.W(q + ".layer_norm.bias");
        // input_proj inside the first block's ff1
        FfnPro in_proj;
        if (i == 0) { in_proj.kind = 1; in_proj.name = "input_proj"; in_proj.w = p.W("model.input_proj.weight"); in_proj.b = p.W("model.input_proj.bias"); in_proj.k = F; }
        add_ffn(p, q + ".ff1", ffn_weights(p, q + ".ff1.layer_norm", q + ".ff1"), 0.5f, hb, t1, t3, big, T, D, in_proj);
        // the attention module in one launch where attn_x3 takes it, else in three
        if (!add_attn_x3(p, q, hb, T, D, NH)) add_attention_module(p, q, ".attention", hb, big, t1, T, D, NH);
        add_conv_module_front(p, m, hb, t1, t3, big, T, D);
        // conv2 + residual inside ff2's launch, and behind the LAST block's ff2 its LayerNorm + the sums of the time average
        FfnPro conv2; conv2.kind = 2; conv2.name = m + ".conv2(pw)+res"; conv2.w = p.W(m + ".conv2.weight"); conv2.b = p.W(m + ".conv2.bias"); conv2.k = D;
        FfnEpi mean; mean.want = i == nb - 1; mean.block = q; mean.ln_w = l2w; mean.ln_b = l2b;
        const bool epi_fused = add_ffn(p, q + ".ff2", ffn_weights(p, q + ".ff2.layer_norm", q + ".ff2"), 0.5f, hb, t1, t3, big, T, D, conv2, mean);
        // the last block's LayerNorm feeds only the mean over time: one pass for both
        if (epi_fused) {
            last_fused = true;
        } else if (i == nb - 1 && D <= 256) {
            p.add("layernorm+mean:" + q + " + time", [=](Run& r) { return launch_ln_mean(r.buf[hb], r.buf[t1], l2w, l2b, r.B, T, D, r.stream); });
            last_fused = true;
        } else {
            p.add("layernorm:" + q, [=](Run& r) { return launch_layernorm(r.buf[hb], r.buf[hb], l2w, l2b, r.B * T, D, ACT_NONE, r.stream); });
        }
    }
    if (!last_fused) p.add("mean:time", [=](Run& r) { return launch_mean_mid(r.buf[hb], r.buf[t1], r.B, T, D, r.stream); });
    set_tail(p, "output_proj", t1, D, p.W("model.output_proj.weight"), p.W("model.output_proj.bias"));
    return NWW_OK;
}

int plan_transformer(PlanCtx& p) {                  // TransformerModel: architectures.py:164-206, nn.TransformerEncoderLayer defaults (post-norm, ReLU)
    nww_handle* h = p.h;
    const nww_config& c = h->cfg;
    const int T = c.in_rows, F = c.in_cols, nb = c.n_blocks;
    const int D = c.conformer_d_model, NH = c.conformer_n_head;
    const int hb = 0, t1 = 1, big = 3;              // h, attention output / time mean, qkv / hidden / time sums
    if (T > NWW_PE_MAX_LEN) return fail(h, NWW_ERR_UNSUPPORTED, "transformer: %d time steps exceed the positional table (%d rows)", T, NWW_PE_MAX_LEN);
    p.need(hb, (size_t)T * D); p.need(t1, (size_t)T * D);
    const float* pe = p.W("model.pos_encoder.pe");
    const float xs = std::sqrt((float)D);          // math.sqrt(d_model), applied in float32 as torch does
    // x = input_proj(x) sqrt(D) + pe[t]: the scale and the positional row in the short-K Linear's epilogue (LIN_RES_TAB), its
    // input rows scaled per row (no clamp of the features); else the general GEMM and one elementwise pass
    LinOpts pos; pos.epi = LIN_RES_TAB; pos.rscale = xs; pos.res_tab = pe; pos.qkv_T = T;
    if (!add_lin_x3(p, "input_proj*sqrt(d)+pe", BUF_X, hb, T, D, F, p.W("model.input_proj.weight"), p.W("model.input_proj.bias"), pos)) {
        add_gemm(p, "input_proj", BUF_X, hb, T, D, F, p.W("model.input_proj.weight"), p.W("model.input_proj.bias"), ACT_NONE);
        p.add("scale+pe:input_proj", [=](Run& r) { return launch_scale_add_pe(r.buf[hb], pe, r.B, T, D, xs, r.stream); });
    }
    bool mean_done = false;
    for (int i = 0; i < nb; ++i) {
        const std::string q = "model.transformer_encoder.layers." + std::to_string(i);
        const bool last = i == nb - 1;
        // ---- h <- h + self_attn(h): head-major in_proj, the attention core, out_proj + residual (as the Conformer's attention module)
        add_attention_module(p, q, ".self_attn", hb, big, t1, T, D, NH);
        // ---- h <- norm2(y + linear2(relu(linear1(y)))), y = norm1(h): one launch (ffn_x3 post-norm instance); the last layer's norm2 feeds
        // only the time mean: exact per-tile sums instead of the store
        const FfnWeights w = ffn_weights(p, q + ".norm1", q);
        const float *n1w = w.ln_w, *n1b = w.ln_b, *b2 = w.b2, *n2w = p.W(q + ".norm2.weight"), *n2b = p.W(q + ".norm2.bias");
        const void* packed = nullptr;
        if (nww_knobs().ffn_fused && p.h->f16 && p.h->conv_products == 6 && ffn_x3_post_supported(D)) {
            const FfnScales s = ffn_f16_scales(p, w, D);
            const float mscale = last ? f16_mean_scale(f16_ln_bound(p.h, n2w, n2b, D)) : 0.0f;
            if (s.ok() && (!last || mscale > 0.0f))
                packed = p.pack_one(ffn_x3_packed_bytes(D), [&](void* d) { return launch_ffn_x3_pack(w.w1, w.b1, w.w2, d, D, p.h->own_stream, s.fw1, s.fw2, 0); });
            if (packed) {
                if (last) p.need(big, (size_t)((T + 31) / 32 + 4) * ffn_x3_post_nseg(T) * 2 * D);
                p.add("ffn_x3:" + q + " (norm1+linear1+relu+linear2+res+norm2" + (last ? "+time sums" : "") + ", post-norm) [f16x3]", [=](Run& r) {
                    FfnArgs a{r.buf[hb], n1w, n1b, static_cast<const unsigned char*>(packed), b2, r.B * T, 1.0f};
                    a.h2_x = s.fx; a.h2_w1 = s.fw1; a.h2_h = s.fh; a.h2_w2 = s.fw2;
                    a.ln2_w = n2w; a.ln2_b = n2b;
                    if (last) { a.msum = r.buf[big]; a.T = T; a.m_scale = mscale; }
                    return launch_ffn_x3_post(a, D, r.stream);
                });
                if (last) {
                    p.add("mean_finish:" + q + " (time average of the exact tile sums)", [=](Run& r) {
                        return launch_ffn_x3_post_mean_finish(r.buf[big], r.buf[t1], r.B, T, D, mscale, r.stream);
                    });
                    mean_done = true;
                }
            }
        }
        if (!packed) {
            add_ffn_unfused(p, w, ACT_RELU, 1.0f, hb, hb, big, T, D, q + ".norm1", q + ".linear1+relu", q + ".linear2+res");
            if (last && D <= 256) {
                p.add("layernorm+mean:" + q + ".norm2 + time", [=](Run& r) { return launch_ln_mean(r.buf[hb], r.buf[t1], n2w, n2b, r.B, T, D, r.stream); });
                mean_done = true;
            } else {
                p.add("layernorm:" + q + ".norm2", [=](Run& r) { return launch_layernorm(r.buf[hb], r.buf[hb], n2w, n2b, r.B * T, D, ACT_NONE, r.stream); });
            }
        }
    }
    if (!mean_done) p.add("mean:time", [=](Run& r) { return launch_mean_mid(r.buf[hb], r.buf[t1], r.B, T, D, r.stream); });
    set_tail(p, "output_proj", t1, D, p.W("model.output_proj.weight"), p.W("model.output_proj.bias"));
    return NWW_OK;
}

int plan_e_branchformer(PlanCtx& p) {               // EBranchformerModel: architectures.py:546-616
    const nww_config& c = p.h->cfg;
    const int T = c.in_rows, F = c.in_cols, nb = c.n_blocks;
    const int D = c.conformer_d_model, NH = c.conformer_n_head;
    // x, glu output / heads' outputs / time mean, depthwise output, wide scratch (q | k | v, the ffn's hidden rows, the gate), the attention
    // branch's output, the conv branch's output (fallback only)
    const int hb = 0, t1 = 1, t3 = 2, big = 3, ab = 4, cb = 5;
    p.need(hb, (size_t)T * D); p.need(t1, (size_t)T * D); p.need(t3, (size_t)T * D); p.need(ab, (size_t)T * D);
    // both branches read input_proj's output, so it cannot ride in a later launch
    add_linear(p, "input_proj", BUF_X, hb, T, D, F, p.W("model.input_proj.weight"), p.W("model.input_proj.bias"));
    for (int i = 0; i < nb; ++i) {
        const std::string q = "model.branchformer_blocks." + std::to_string(i);
        // ---- a = MHA(LayerNorm(x)): no residual here, the merge takes it.  One launch where attn_x3 takes the shape, else three
        AttnBranch br; br.ln_w = p.W(q + ".attn_branch_norm.weight"); br.ln_b = p.W(q + ".attn_branch_norm.bias"); br.out = ab; br.ln_name = ".attn_branch_norm";
        if (!add_attn_x3(p, q, hb, T, D, NH, br)) add_attention_module(p, q, ".attention", hb, big, t1, T, D, NH, br);
        // ---- the ConvolutionModule up to its depthwise stage -> t3
        const std::string m = q + ".conv_branch";
        add_conv_module_front(p, m, hb, t1, t3, big, T, D);
        // ---- x <- final_norm(x + a g + c (1 - g)), c = conv2(t3), g = sigmoid(gate(c)): one row-local launch (merge_x3.hip) under the
        // default arithmetic - its rows are scaled one by one in the kernel, so it needs no bound on t3 or c - else four
        const float *c2w = p.W(m + ".conv2.weight"), *c2b = p.W(m + ".conv2.bias");
        const float *gw = p.W(q + ".merger.gate.weight"), *gb = p.W(q + ".merger.gate.bias");
        const float *fnw = p.W(q + ".final_norm.weight"), *fnb = p.W(q + ".final_norm.bias");
        bool merged = false;
        if (nww_knobs().merge_fused && p.h->f16 && p.h->conv_products == 6 && merge_x3_supported(D)) {
            const float wsc = f16_wscale(f16_fetch(p.h, c2w, (size_t)D * D)), wsg = f16_wscale(f16_fetch(p.h, gw, (size_t)D * D));
            const void* packed = !(wsc > 0.0f && wsg > 0.0f) ? nullptr : p.pack_one(merge_x3_packed_bytes(D), [&](void* d) { return launch_merge_x3_pack(c2w, gw, d, D, wsc, wsg, p.h->own_stream); });
            if (packed) {
                p.add("merge_x3:" + q + " (conv2(pw)+gate+blend+res+final_norm) [f16x3]", [=](Run& r) {
                    MergeArgs a{r.buf[t3], r.buf[ab], r.buf[hb], static_cast<const unsigned char*>(packed), c2b, gb, fnw, fnb, r.B * T, 1.0f / wsc, 1.0f / wsg};
                    return launch_merge_x3(a, D, r.stream);
                });
                merged = true;
            }
        }
        if (!merged) {
            add_linear(p, m + ".conv2(pw)", t3, cb, T, D, D, c2w, c2b);
            add_linear(p, q + ".merger.gate", cb, big, T, D, D, gw, gb);
            p.add("branch_merge:" + q + " (sigmoid+blend+res)", [=](Run& r) { return launch_branch_merge(r.buf[hb], r.buf[ab], r.buf[cb], r.buf[big], (size_t)r.B * T * D, r.stream); });
            p.add("layernorm:" + q + ".final_norm", [=](Run& r) { return launch_layernorm(r.buf[hb], r.buf[hb], fnw, fnb, r.B * T, D, ACT_NONE, r.stream); });
        }
        // ---- x <- x + ffn(x): the Conformer's FeedForwardModule with the FULL residual, in its plain fused form (ffn_x3.hip) or unfused
        const std::string ff = q + ".ffn";
        add_ffn(p, ff, ffn_weights(p, ff + ".layer_norm", ff), 1.0f, hb, t1, t3, big, T, D);
    }
    // no LayerNorm in front of the mean (unlike the Conformer), so no plan-time bound for the exact-sum epilogue: the plain mean
    p.add("mean:time", [=](Run& r) { return launch_mean_mid(r.buf[hb], r.buf[t1], r.B, T, D, r.stream); });
    set_tail(p, "output_proj", t1, D, p.W("model.output_proj.weight"), p.W("model.output_proj.bias"));
    return NWW_OK;
}

int plan_tcn(PlanCtx& p) {                          // TCNModel: architectures.py:290-367; the head reads tcn_out[:, :, T - 1] only
    const nww_config& c = p.h->cfg;
    const int T = c.in_rows, F = c.in_cols;
    const int k = c.layer_dim, nl = c.n_crnn_channels;
    const int* ch = c.crnn_channels;
    const int last = 5;                                    // [B][ch[nl - 1]]: the last block's output at t = T - 1
    p.need(last, (size_t)ch[nl - 1]);
    auto key = [](int i, const char* part) { return "model.tcn_blocks." + std::to_string(i) + "." + part; };
    // the whole stack in one launch over the last step's receptive-field cone (tcn_x3.hip), under the default arithmetic at the
    // shapes it takes (widths multiples of 32 up to 256, the cone inside the LDS): two binary16 terms per operand, every row scaled
    // by its own power of two - no bound on the features, no clamp
    bool fused = false;
    if (p.h->f16 && p.h->conv_products == 6) {
        TcnArgs a;
        a.T = T; a.F = F; a.L = nl; a.k = k;
        for (int i = 0; i < nl; ++i) a.ch[i] = ch[i];
        PlanCtx::Packs packs(p);
        bool ok = tcn_x3_plan(a);
        int cin = F;
        for (int i = 0; ok && i < nl; ++i) {
            auto pack = [&](const char* part, int ci, int taps, TcnConv& cv) {
                const float* w = p.W(key(i, (std::string(part) + ".weight").c_str()));
                const float ws = f16_wscale(f16_fetch(p.h, w, (size_t)ch[i] * ci * taps));
                if (!(ws > 0.0f)) return false;
                cv.packed = static_cast<const unsigned char*>(packs.pack(tcn_x3_packed_bytes(ci, ch[i], taps), [&](void* d) {
                    return launch_tcn_x3_pack(w, d, ci, ch[i], taps, ws, p.h->own_stream);
                }));
                if (!cv.packed) return false;
                cv.bias = p.W(key(i, (std::string(part) + ".bias").c_str()));
                cv.w_un = 1.0f / ws;
                return true;
            };
            ok = pack("conv1", cin, k, a.c1[i]) && pack("conv2", ch[i], k, a.c2[i]) && (cin == ch[i] || pack("downsample", cin, 1, a.ds[i]));
            cin = ch[i];
        }
        if (ok) {
            packs.commit();
            p.add("tcn_x3:" + std::to_string(nl) + " blocks, last " + std::to_string(a.S) + " steps of " + std::to_string(T) + " [f16x3]",
                  [=](Run& r) {
                      TcnArgs g = a;
                      g.x = r.x; g.out = r.buf[last]; g.B = r.B;
                      return launch_tcn_x3(g, r.stream);
                  });
            fused = true;
        }
    }
    if (!fused) {
        // every level over the whole sequence: causal im2col (taps x dilation, zero history), conv1 = GEMM + ReLU, conv2 = GEMM + ReLU
        // + the residual (or the downsample's GEMM), then the second ReLU; the last row of each clip feeds the tail
        const int col = 0, hid = 1, rsd = 4;
        int in = BUF_X, cin = F;
        for (int i = 0; i < nl; ++i) {
            const int co = ch[i], dil = 1 << i, out = i % 2 == 0 ? 2 : 3;
            const std::string q = "model.tcn_blocks." + std::to_string(i);
            p.need(col, (size_t)T * k * (cin > co ? cin : co));
            p.add("im2col:" + q + ".conv1", [=](Run& r) { return launch_tcn_im2col(src(r, in), r.buf[col], r.B, T, cin, k, dil, r.stream); });
            add_gemm(p, q + ".conv1+relu", col, hid, T, co, cin * k, p.W(key(i, "conv1.weight")), p.W(key(i, "conv1.bias")), ACT_RELU);
            p.add("im2col:" + q + ".conv2", [=](Run& r) { return launch_tcn_im2col(r.buf[hid], r.buf[col], r.B, T, co, k, dil, r.stream); });
            int res = in;
            if (cin != co) {
                add_gemm(p, q + ".downsample", in, rsd, T, co, cin, p.W(key(i, "downsample.weight")), p.W(key(i, "downsample.bias")), ACT_NONE);
                res = rsd;
            }
            GemmOpts ro; ro.res_id = res;
            add_gemm(p, q + ".conv2+relu+res", col, out, T, co, co * k, p.W(key(i, "conv2.weight")), p.W(key(i, "conv2.bias")), ACT_RELU, ro);
            p.add("unary:relu " + q, [=](Run& r) { return launch_unary(r.buf[out], r.buf[out], (size_t)r.B * T * co, ACT_RELU, r.stream); });
            in = out; cin = co;
        }
        const int fin = in, C = cin;
        p.add("last_row:tcn_out[:, :, T - 1]", [=](Run& r) { return launch_tcn_last_row(r.buf[fin], r.buf[last], r.B, T, C, r.stream); });
    }
    set_tail(p, "fc", last, ch[nl - 1], p.W("model.fc.weight"), p.W("model.fc.bias"));
    return NWW_OK;
}

// E2ERawQuartzNet (architectures.py:798-817): the raw-PCM frontend's launches, which run where the other heads' STFT frontend runs
// (nww_frontend_on_dev), so that nww_forward_features* is the backbone alone; the backbone and the tail are plan_quartznet's
void plan_raw_frontend(PlanCtx& p) {
    const nww_config& c = p.h->cfg;
    for (int i = 0, Cin = 1; i < c.n_blocks; ++i) {
        const int Cout = c.layer_dim << i, k = i == 0 ? 41 : 13, stride = i == 0 ? 16 : 4;
        const std::string conv = "model.frontend.conv_blocks." + std::to_string(3 * i);
        p.h->raw.push_back({"conv1d_strided:" + conv + " (k " + std::to_string(k) + " stride " + std::to_string(stride) + " " + std::to_string(Cin) + "->" +
                                std::to_string(Cout) + ")+bn+relu [f32]",
                            Cin, Cout, k, stride, p.W(conv + ".raw.w"), p.W(conv + ".raw.b")});
        Cin = Cout;
    }
    // ---- the whole frontend in one launch (raw_x3.hip) under the default arithmetic at the shapes it takes.  |x| <= 1 bounds every
    // stage through the folded weights' row 1-norms; the planes' powers of two come from those bounds, so nothing is clamped.
    // The bound compounds over the stages and follows the LOUDEST channel, so each plane is held to a range window as every other
    // plan-time-scaled layer is (F16Range): beside the bound a typical magnitude per channel, typ_co = sqrt(sum_q w_q^2 typ_q^2 + b^2)
    // from a typical |x| of 2^-5 (1024 LSB, -30 dBFS).  Per channel, not f16_layer_typ's mean: a channel whose folded BatchNorm gain is G
    // times the others' (and whose weights in the next stage are 1 / G) would put G / Cout into a mean and hide the others.  What the
    // plane's absolute error (2^-25 / scale on a value far below the bound) does to output channel co of the stage that reads it goes
    // through that row's 2-norm, so the plane's magnitude as co sees it is typ_co / ||w_co||_2, and the smallest of those is held against
    // the bound: within 2^4 f16_range_factor() (2^20: the quietest row keeps 20 bits, 1e-6; the window is taken against the quietest row
    // and not a mean, hence the 2^4) the launch is raw_x3, otherwise one conv1d_strided launch per stage (float32).  DESIGN.md 4.4f
    nww_handle* h = p.h;
    if (!(nww_knobs().raw_fused && h->f16 && h->conv_products == 6 && raw_x3_supported(c.layer_dim, c.n_blocks))) return;
    RawX3Args a;
    a.depth = c.n_blocks; a.C1 = c.layer_dim;
    PlanCtx::Packs pk(p);
    double bound = 1.0;
    std::vector<double> typ(1, 0.03125);                      // per channel of the stage's input
    for (int i = 0, Cin = 1; i < c.n_blocks; ++i) {
        const int Cout = c.layer_dim << i, k = i == 0 ? 41 : 13;
        const std::string conv = "model.frontend.conv_blocks." + std::to_string(3 * i);
        const HostTensor &w = h->tensors[conv + ".raw.w"], &b = h->tensors[conv + ".raw.b"];
        // w [k][Cin][Cout]: column q is channel q % Cin
        const F16Rows rows = f16_rows_moments(Cout, k * Cin, [&](int q, int co) { return w.data[(size_t)q * Cout + co]; }, [&](int q) { return q % Cin; }, typ);
        if (i == 0) {
            a.w1 = p.W(conv + ".raw.w"); a.b1 = p.W(conv + ".raw.b");
        } else {
            if (!f16_rows_ok(bound, rows)) return;               // the plane this stage reads, as its quietest output row sees it
            if (!p.W(conv + ".raw.wk")) return;
            const float ws = f16_wscale(w.data), sc = f16_scale(bound);
            if (!(ws > 0.0f) || !(sc > 0.0f)) return;
            a.packed[i - 1] = static_cast<const unsigned char*>(pk.pack((size_t)(Cout / 32) * (k * Cin / 16) * 2048, [&](void* d) {
                return launch_qn_x3_pack(p.W(conv + ".raw.wk"), d, Cout, k * Cin, ws, h->own_stream);
            }));
            if (!a.packed[i - 1]) return;
            a.bias[i - 1] = p.W(conv + ".raw.b");
            a.scale[i - 1] = sc; a.un[i - 1] = 1.0f / (ws * sc);
        }
        double worst = 0.0;                                   // this stage's output bound
        for (int co = 0; co < Cout; ++co) {
            double t = 0.0;
            for (int q = 0; q < k * Cin; ++q) t += std::fabs((double)w.data[(size_t)q * Cout + co]);
            worst = std::fmax(worst, t * bound + std::fabs((double)b.data[co]));
        }
        bound = worst * (1.0 + 1e-6);
        typ = f16_rows_typ(rows, b.data, true, b.data, b.data, false);
        Cin = Cout;
    }
    pk.commit();
    h->raw_x3 = a;
    h->raw_fused = true;
    h->raw_fused_name = "raw_x3:model.frontend (" + std::to_string(c.n_blocks) + " stages 1->" + std::to_string(c.layer_dim << (c.n_blocks - 1)) +
                        ", conv+bn+relu) [f16x3]";
}

// E2ERawCNN's RawAudioBackbone (architectures.py:739-776) behind the raw frontend: four conv + BatchNorm + activation stages on the
// channels-last plane the frontend writes ([rows][width] = the reference's image transposed; the 3x3 weights were transposed at
// nww_finalize, not the data), one launch each, then the mean over the plane and the Linear in the tail.  conv1 (one input channel, nine
// taps: VALU work) is a conv2d_strided launch; conv2 .. conv4 run on conv2s_x3 under the default arithmetic - the tile's power of two
// comes from the tile's data and the weights' from each output channel, so there is no bound to compound over the layers, no range
// window to guard and no clamp - and on conv2d_strided (float32) under every other arithmetic, with NWW_CONV2S_X3=0, or for a weight
// tensor whose per-row scale could not be formed.  DESIGN.md 4.4h
int plan_e2e_cnn(PlanCtx& p) {
    const nww_config& c = p.h->cfg;
    const RawCnnLayer* ly = nww_raw_cnn_layers();
    const int act = c.activation, mbuf = 2;
    const char* an = act == ACT_GELU ? "gelu" : act == ACT_SILU ? "silu" : "relu";
    int A = c.in_rows, Bd = c.in_cols, in = BUF_X;
    for (int i = 0; i < 4; ++i) {
        const int Cin = ly[i].cin, Cout = ly[i].cout, sA = ly[i].sA, sB = ly[i].sB, Ao = conv2s_out(A, sA), Bo = conv2s_out(Bd, sB), out = i % 2;
        const std::string q = "model.backbone.conv" + std::to_string(i + 1), conv = q + ".0";
        const std::string what = q + " (3x3 stride " + std::to_string(sB) + "x" + std::to_string(sA) + " " + std::to_string(Cin) + "->" + std::to_string(Cout) + ", " +
                                 std::to_string(Bd) + "x" + std::to_string(A) + "->" + std::to_string(Bo) + "x" + std::to_string(Ao) + ")+bn+" + an;
        const float *w = p.W(conv + ".c2.w"), *bias = p.W(conv + ".c2.b"), *wk = p.W(conv + ".c2.wk"), *un = p.W(conv + ".c2.un");
        p.need(out, (size_t)Ao * Bo * Cout);
        const void* packed = nullptr;
        if (nww_knobs().conv2s_x3 && p.h->f16 && p.h->conv_products == 6 && conv2s_x3_supported(Cin, Cout, sA, sB) && wk && un)
            packed = p.pack_one(conv2s_x3_packed_bytes(Cin, Cout), [&](void* d) {
                return launch_qn_x3_pack(wk, d, conv2s_x3_coutp(Cout), 9 * conv2s_x3_cp(Cin), 1.0f, p.h->own_stream);
            });
        const int Ai = A, Bi = Bd;
        if (packed)
            p.add("conv2s_x3:" + what + " [f16x3]", [=](Run& r) {
                Conv2sX3Args a;
                a.x = src(r, in); a.y = r.buf[out]; a.packed = static_cast<const unsigned char*>(packed); a.w_un = un; a.bias = bias;
                a.B = r.B; a.A = Ai; a.Bd = Bi; a.Cin = Cin; a.Cout = Cout; a.stride = sA; a.act = act;
                return launch_conv2s_x3(a, r.stream);
            });
        else
            p.add("conv2d_strided:" + what + " [f32]", [=](Run& r) {
                Conv2sArgs a;
                a.x = src(r, in); a.y = r.buf[out]; a.w = w; a.bias = bias;
                a.B = r.B; a.A = Ai; a.Bd = Bi; a.Cin = Cin; a.Cout = Cout; a.sA = sA; a.sB = sB; a.act = act;
                return launch_conv2d_strided(a, r.stream);
            });
        in = out; A = Ao; Bd = Bo;
    }
    const int fin = in, L = A * Bd;
    p.need(mbuf, 96);
    p.add("mean:plane", [=](Run& r) { return launch_mean_mid(r.buf[fin], r.buf[mbuf], r.B, L, 96, r.stream); });
    set_tail(p, "fc", mbuf, 96, p.W("model.backbone.fc.weight"), p.W("model.backbone.fc.bias"));
    return NWW_OK;
}

int plan_quartznet(PlanCtx& p) {                    // QuartzNetModel: architectures.py:370-437; time-major rows [T][C], as the head input is
    const nww_config& c = p.h->cfg;
    const std::string qp = nww_quartznet_prefix(c);
    const int T = c.in_rows;
    const auto blocks = nww_quartznet_blocks(c);
    const int nblk = (int)blocks.size();
    // ping-pong block outputs, depthwise output, pointwise output, projection output, time mean
    const int dbuf = 2, ybuf = 3, rbuf = 4, mbuf = 5;
    const int C_last = blocks.back().cout;
    p.need(mbuf, (size_t)C_last);
    int in = BUF_X;
    bool mean_done = false;
    for (int i = 0; i < nblk; ++i) {
        const int Cin = blocks[i].cin, Cout = blocks[i].cout, k = blocks[i].k, Cp = qn_x3_cp(Cin);
        const bool proj = Cin != Cout, last = i == nblk - 1;
        const std::string q = qp + "quartznet_blocks." + std::to_string(i);
        const int out = i % 2;
        const float *dwt = p.W(q + ".qn.dw_t"), *bias = p.W(q + ".qn.bias");
        // ---- the whole block in one clip-resident launch (qn_x3.hip) under the default arithmetic at the shapes it takes: two binary16 terms per
        // operand, each row scaled by its own power of two inside the kernel - no bound on the features, no clamp
        bool fused = false;
        if (nww_knobs().qn_fused && p.h->f16 && p.h->conv_products == 6 && qn_x3_supported(T, Cin, Cout, k) && p.W(q + ".qn.wcat")) {
            const HostTensor& cat = p.h->tensors[q + ".qn.wcat"];
            const float ws = f16_wscale(cat.data);
            const void* packed = !(ws > 0.0f) ? nullptr : p.pack_one(qn_x3_packed_bytes(Cin, Cout, proj), [&](void* d) {
                return launch_qn_x3_pack(p.W(q + ".qn.wcat"), d, Cout, qn_x3_ktot(Cin, proj), ws, p.h->own_stream);
            });
            if (packed) {
                const float amax = p.h->tensors[q + ".qn.amax"].data[0];
                if (!last) p.need(out, (size_t)T * Cout);
                p.add("qn_x3:" + q + " (dw" + std::to_string(k) + "+pw+bn" + (proj ? "+proj" : "+x") + "+relu" + (last ? "+mean:time" : "") + ") [f16x3]", [=](Run& r) {
                    QnArgs a;
                    a.x = src(r, in); a.out = last ? r.buf[mbuf] : r.buf[out]; a.packed = static_cast<const unsigned char*>(packed); a.dw = dwt; a.bias = bias;
                    a.B = r.B; a.T = T; a.Cin = Cin; a.Cp = Cp; a.Cout = Cout; a.k = k; a.proj = proj ? 1 : 0; a.mean = last ? 1 : 0;
                    a.amax = amax; a.w_un = 1.0f / ws;
                    return launch_qn_x3(a, r.cu_count, r.stream);
                });
                fused = true;
                mean_done = last;
            }
        }
        if (!fused) {
            // the same folded operands on the general launches: depthwise, pointwise (+ the folded bias), the projection, add + ReLU
            p.need(dbuf, (size_t)T * Cin); p.need(ybuf, (size_t)T * Cout); p.need(out, (size_t)T * Cout);
            p.add("dwconv1d:" + q + " (k " + std::to_string(k) + ")", [=](Run& r) { return launch_dwconv1d_same(src(r, in), dwt, r.buf[dbuf], r.B, T, Cin, k, Cp, r.stream); });
            add_linear(p, q + ".pointwise_conv+bn", dbuf, ybuf, T, Cout, Cin, p.W(q + ".qn.pw"), bias);
            int res = in;
            if (proj) {
                add_linear(p, q + ".residual_connector+bn", in, rbuf, T, Cout, Cin, p.W(q + ".qn.res"), nullptr);
                res = rbuf;
            }
            p.add("add+relu:" + q, [=](Run& r) { return launch_add_relu(r.buf[ybuf], src(r, res), r.buf[out], (size_t)r.B * T * Cout, r.stream); });
        }
        in = out;
    }
    if (!mean_done) {
        const int fin = in;
        p.add("mean:time", [=](Run& r) { return launch_mean_mid(r.buf[fin], r.buf[mbuf], r.B, T, C_last, r.stream); });
    }
    set_tail(p, "fc", mbuf, C_last, p.W(qp + "fc.weight"), p.W(qp + "fc.bias"));
    return NWW_OK;
}

// the head's last Linear (-> embedding) + Model.classifier (model.py:291-296) (+ sigmoid) -> emb [B][E], logits [B] (, probs [B])
void plan_tail(PlanCtx& p) {
    const int E = p.h->cfg.embedding_dim, act = p.h->cfg.activation;
    if (nww_knobs().tail && tail_supported(p.tail_K, E)) {
        const float *We = p.tail_W, *be = p.tail_b, *W0 = p.W("classifier.0.weight"), *b0 = p.W("classifier.0.bias"),
                    *w3 = p.W("classifier.3.weight"), *b3 = p.W("classifier.3.bias");
        const int tin = p.tail_in, tK = p.tail_K;
        const PlanCtx::DnnBody dnn = p.dnn;
        // the step's name says which kernel large batches get (the shape part of tail_batch_runs; small batches always the latency kernel)
        const bool batch_kernel = tail_batch_runs(1 << 20, tK, E, dnn.on, 0);
        p.add("tail:" + p.tail_name + "+classifier" + (batch_kernel ? " (large batches: persistent, weights in LDS)" : ""), [=](Run& r) {
            TailArgs t{src(r, tin), tK, We, be, E, W0, b0, w3, b3, r.emb, r.logits, r.probs, r.B, act};
            t.cu_count = r.cu_count;
            if (dnn.on) {
                t.ln0_w = dnn.ln0_w; t.ln0_b = dnn.ln0_b; t.n_mid = dnn.n_mid;
                for (int i = 0; i < dnn.n_mid; ++i) { t.mid_W[i] = dnn.mid[i][0]; t.mid_b[i] = dnn.mid[i][1]; t.mid_lnw[i] = dnn.mid[i][2]; t.mid_lnb[i] = dnn.mid[i][3]; }
            }
            if (r.deferred.active && r.deferred.out_id == tin) {
                t.parts = r.splitk_ws; t.nparts = r.deferred.parts; t.part_stride = r.deferred.stride;
                t.in_bias = r.deferred.bias; t.in_alpha = r.deferred.alpha; t.in_beta = r.deferred.beta; t.in_act = r.deferred.act;
            }
            r.deferred.active = false;
            r.need_sigmoid = false;
            if (r.done_flag && r.B <= 16) { t.done_flag = r.done_flag; t.done_seq = r.done_seq; r.done_armed = true; }
            return launch_classifier_tail(t, r.stream);
        });
    } else {
        add_gemm(p, p.tail_name, p.tail_in, BUF_EMB, 1, E, p.tail_K, p.tail_W, p.tail_b, ACT_NONE);
        add_gemm(p, "classifier.0", BUF_EMB, BUF_HID, 1, E / 2, E, p.W("classifier.0.weight"), p.W("classifier.0.bias"), act);
        add_gemm(p, "classifier.3", BUF_HID, BUF_LOGITS, 1, 1, E / 2, p.W("classifier.3.weight"), p.W("classifier.3.bias"), ACT_NONE);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------ finalize
extern "C" int nww_finalize(nww_handle* h) {
    if (!h) return NWW_ERR_INVALID;
    if (h->finalized) return NWW_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (const auto& k : h->keys)
        if (!h->tensors[k].loaded) return fail(h, NWW_ERR_MISSING, "Missing key(s) in state_dict: '%s'", k.c_str());
    balance_channel_gains(h);
    fold_batchnorms(h);
    if (h->cfg.head_type == NWW_HEAD_BCRESNET) transpose_depthwise(h);
    if (h->cfg.head_type == NWW_HEAD_E2E_DNN) transpose_e2e_filters(h);
    if (h->cfg.head_type == NWW_HEAD_QUARTZNET || h->cfg.head_type == NWW_HEAD_E2E_QUARTZNET) fold_quartznet(h);
    if (nww_raw_head(h->cfg)) fold_raw_frontend(h);
    if (h->cfg.head_type == NWW_HEAD_E2E_CNN) fold_raw_backbone(h);
    struct ArenaImage { nww_handle* h; ~ArenaImage() { std::vector<float>().swap(h->h_weights); } } image{h};      // held until this returns
    int rc = upload_weight_arena(h);
    if (rc == NWW_OK) rc = build_frontend_tables(h);
    if (rc != NWW_OK) return rc;
    PlanCtx p{h};
    switch (h->cfg.head_type) {
        case NWW_HEAD_DNN: rc = plan_dnn(p); break;
        case NWW_HEAD_CNN: rc = plan_cnn(p); break;
        case NWW_HEAD_E2E_DNN: rc = plan_e2e_dnn(p); break;
        case NWW_HEAD_CRNN: rc = plan_crnn(p); break;
        case NWW_HEAD_GRU: rc = plan_gru(p); break;
        case NWW_HEAD_BCRESNET: rc = plan_bcresnet(p); break;
        case NWW_HEAD_CONFORMER: rc = plan_conformer(p); break;
        case NWW_HEAD_TRANSFORMER: rc = plan_transformer(p); break;
        case NWW_HEAD_TCN: rc = plan_tcn(p); break;
        case NWW_HEAD_E_BRANCHFORMER: rc = plan_e_branchformer(p); break;
        case NWW_HEAD_QUARTZNET: rc = plan_quartznet(p); break;
        case NWW_HEAD_E2E_QUARTZNET: plan_raw_frontend(p); rc = plan_quartznet(p); break;
        case NWW_HEAD_RNN: rc = plan_rnn(p); break;
        case NWW_HEAD_E2E_CNN: plan_raw_frontend(p); rc = plan_e2e_cnn(p); break;
    }
    if (rc != NWW_OK) return rc;
    plan_tail(p);
    // the plan-time weight packings above were enqueued on own_stream; a forward may arrive on any caller stream
    HIP_TRY(h, hipStreamSynchronize(h->own_stream));
    if (!h->plan_error.empty()) return fail(h, NWW_ERR_HIP, "%s", h->plan_error.c_str());
    h->finalized = true;
    return NWW_OK;
}
