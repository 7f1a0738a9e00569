// nww_internal.h - what the translation units of the C-ABI share: the handle, a forward's run state, error helpers and the
// device-side entry points they call on each other.  nww_api.hip: create / load / run entry points; nww_weights.hip: state_dict spec
// and weight preparation; nww_plan.hip: the per-head launch plans (nww_finalize); nww_stream.hip: batched streaming (nww_stream_*); nww_comm.hip: RCCL gather;
// nww_emb.hip: embedding-mode state (nww_emb_*); nww_recording.hip: recording scoring (nww_recording_*, nww_forward_recording*);
// nww_cascade.hip: gate + verifier cascades (nww_cascade_*); nww_bank.hip: model banks (nww_bank_*: K heads on one frontend pass);
// nww_mix.hip: clips mixed on the device out of an arena (nww_mix_*; kernel in mix.hip, arithmetic in mix_plan.h);
// stream_plan.h: what a (window, hop) pair shares between windows (host-only arithmetic, used by the last two); stream_pool.h: the
// one ring state of a stream batch, moved by its lock-step calls and by the calls whose streams push and reset on their own (host-only
// too, used by nww_stream.hip and read by nww_cascade.hip); plan_host.h: the
// planner's arithmetic on the weights' values (host-only too, used by nww_plan.hip and nww_weights.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/nww.h"
#include "fe_tables.h"
#include "stream_plan.h"
#include "stream_pool.h"
#include "raw_plan.h"
#include "plan_host.h"
#include "frontend.h"
#include "layers.h"
#include "trunk.h"
#include "ffn_x3.h"
#include "lin_x3.h"
#include "attn_x3.h"
#include "dual_x3.h"
#include "emb_stream.h"
#include "merge_x3.h"
#include "tcn_x3.h"
#include "qn_x3.h"
#include "raw_conv.h"
#include "raw_x3.h"
#include "conv2s_x3.h"

// rows of the Transformer's positional-encoding buffer model.pos_encoder.pe [5000][1][d_model] (PositionalEncoding max_len,
// architectures.py:31)
#define NWW_PE_MAX_LEN 5000

struct Step {
    std::string name;
    std::function<hipError_t(struct Run&)> fn;
};

// What a streaming hop hands to the plan's steps (built by nww_stream.hip, which alone knows the rings' geometry; read by add_trunk and
// add_conv_mfma).  The default is no hop: a dense x, every row computed into the plan's workspace.
struct HopView {
    size_t x_stride = 0;        // floats between consecutive clips of x; 0 = dense (only first steps that say so at plan time take a stride)
    // set only for plans with nww_handle::stream_conv: 1 = the fused trunk writes its pooled rows into per-stream rings and the third
    // conv reads them there, 2 = and only the strips of rows a hop invalidates are computed
    int mode = 0;
    float* a2_ring = nullptr; int a2_rows = 0, a2_row0 = 0; size_t a2_ch_stride = 0, a2_clip_stride = 0;
    int a2_nsub = 0, a2_sub_a[4] = {0, 0, 0, 0}, a2_sub_b[4] = {0, 0, 0, 0};
    // the third conv's sequence output lives in two per-stream buffers that alternate from hop to hop: rows [a3_lo, a3_hi] of the new
    // one are rows + a3_shift of the previous one, the others are computed (mode 2); null: the plan's workspace buffer
    float* seq_new = nullptr; const float* seq_prev = nullptr; int a3_lo = 0, a3_hi = -1, a3_shift = 0;
};

// An open stream batch: S streams, a window of W samples, a score per hop.  nww_stream_open creates it, nww_stream_close frees its device
// memory and deletes it, nww_stream_reset rewinds it.
struct StreamState {
    int S = 0, W = 0, hop = 0;
    int16_t* d_ring = nullptr; int16_t* d_chunk = nullptr;   // [S][2 * W]: sample p of a stream lives at p and p + W; a host chunk's staging [S][hop]
    HopPlan plan;                  // what a lock-step hop keeps; each kept level has its buffers below
    // The state of the PCM and log-mel rings - position, fill, log-mel rotation and primed, of the batch while its streams are aligned
    // and of every stream once they are not - for the lock-step calls and the pool calls alike (stream_pool.h).
    StreamPool pool;
    // log-mel ring [S][2 * lm_rows][n_mels]: frame t of a stream's current window at row lm_pos + t of its ring and lm_rows away; a hop shifts it by plan.k
    float* d_lm_ring = nullptr; int lm_rows = 0;
    // What the lock-step path alone keeps.  Pooled conv rows [S][32][plan.a2_rows][stream_W / 4]: row R at (a2_pos + R) % a2_rows; a hop
    // shifts them by plan.a2_shift.  The third conv's sequence output, alternating from hop to hop (HopView::seq_new).  rows_held: both
    // hold the previous window; any pool call, reset or failed hop clears it, and the next lock-step hop computes its window whole.
    float* d_a2_ring = nullptr; int a2_pos = 0;
    float* d_seq[2] = {nullptr, nullptr}; int seq_cur = 0;
    bool rows_held = false;
    // The pool calls' device side, allocated by the first one: the frontend's scratch [S][T][row floats], POOL_TAB_SLOTS table slots on the
    // device and in pinned host memory (a call's table is written to the next slot once the event of that slot's previous call has
    // passed), and the dense [2][S] outputs of the host-pointer entry point
    float* d_lm_scratch = nullptr; unsigned char* d_tab = nullptr; unsigned char* pin_tab = nullptr; float* d_pool_out = nullptr;
    hipEvent_t ev_tab[4] = {nullptr, nullptr, nullptr, nullptr}; size_t tab_slot_bytes = 0; unsigned tab_seq = 0;
    int stat_scored = 0; long long stat_frames = 0;                   // nww_stream_pool_stats: the latest push_some
};
#define POOL_TAB_SLOTS 4

struct Run {
    int B = 0;
    hipStream_t stream = nullptr;
    const float* x = nullptr;   // head input [B][in_rows*in_cols]
    HopView hop;
    bool x_frames_major = false; // E2E head on the transposed plane: x came from the frontend as [B][frames][n_mels] already
    float* buf[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float* emb = nullptr;       // [B][E]
    float* hid = nullptr;       // [B][E/2]
    float* logits = nullptr;    // [B]
    float* probs = nullptr;     // [B] or null; a plan step that writes it clears `need_sigmoid`
    bool need_sigmoid = true;
    unsigned int* done_flag = nullptr; unsigned int done_seq = 0; bool done_armed = false;   // zero-copy small calls (classifier tail's completion word)
    float* splitk_ws = nullptr; size_t splitk_floats = 0; int cu_count = 256;
    // a split-K GEMM that left its partials for the classifier tail to reduce (GemmArgs::defer_reduce)
    struct { bool active = false; int out_id = 0, parts = 0; size_t stride = 0; const float *bias = nullptr, *alpha = nullptr, *beta = nullptr; int act = 0; } deferred;
};


// key of the packed-weight cache: the weight, the image format (0 = bf16 terms, 1 = scaled binary16 terms) and the latter's scale
struct X3Key {
    const float* w; int fmt; float scale;
    bool operator<(const X3Key& o) const { return w != o.w ? w < o.w : fmt != o.fmt ? fmt < o.fmt : scale < o.scale; }
};

struct nww_handle {
    bool e2e_transposed = false;                   // the E2E plan runs on the (frames, n_mels) plane: the frontend writes frames-major for it
    nww_config cfg;
    FeParams fe;
    std::string err;
    std::vector<std::string> keys;                 // required state_dict keys, in order
    std::map<std::string, HostTensor> tensors;     // required + optional + derived
    bool finalized = false;
    float* d_weights = nullptr;
    std::vector<float> h_weights;  // the arena's host image, offset for offset: what the planner reads weight values from; held while nww_finalize runs
    FeTables* d_tables = nullptr;
    std::vector<float> fe_window, fe_mel_fb;   // the window and filterbank the tables were built from, loaded or built in (what a bank compares: bank.h)
    Fe2MelPlan* d_melplan = nullptr;
    int mel_max_taps = 0;          // longest filter support of the mel filterbank
    hipStream_t own_stream = nullptr;
    std::vector<Step> plan;
    size_t buf_per_clip[6] = {0, 0, 0, 0, 0, 0};   // floats per clip of each workspace buffer
    // workspace (grown on demand)
    int cap_B = 0, cap_N = 0;
    bool trunk_blocked = false;    // CNN head: the fused trunk writes fc1's A operand as [128][32] tiles (decided at plan time)
    int cap_rows = 0;              // cap_B rounded up to 128: the blocked trunk -> fc1 buffer is written in 128-clip row blocks
    float* d_ws = nullptr;
    int16_t* d_pcm = nullptr;
    // the raw-PCM heads (nww_raw_head): the stages of the learned raw-PCM frontend (planned at nww_finalize) and the two buffers its
    // intermediate rows alternate between; its last stage writes d_logmel (time-major, what the backbone reads)
    struct RawStage { std::string name; int cin, cout, k, stride; const float *w, *b; };
    std::vector<RawStage> raw;
    // ... or the whole frontend as one raw_x3 launch (the default under f16x3 at the shapes it takes): its arguments but the run's own
    bool raw_fused = false; std::string raw_fused_name; RawX3Args raw_x3;
    float* d_raw[2] = {nullptr, nullptr};
    float* d_logmel = nullptr;     // [B][n_mels*frames]
    float* d_feats = nullptr;      // staging for host feature input
    float* d_emb = nullptr;
    float* d_hid = nullptr;
    float* d_logits = nullptr;
    float* d_probs = nullptr;
    float* d_splitk = nullptr;     // split-K partials
    std::string plan_error;        // plan time: a step that cannot be planned in ANY form (nww_finalize fails with it)
    bool clamps_features = false;  // plan time: a step that reads the head input clamps it to +-NWW_F16_FEATURE_BOUND (nww_feature_clamp)
    // plan-time capabilities: what the plan can take from a streaming hop (HopView)
    bool x_stride_ok = false;      // the first step takes HopView::x_stride (fused split-operand trunk)
    bool stream_conv = false;      // fused trunk -> conv3_x3 pair that takes HopView::mode (CRNN)
    int stream_H = 0, stream_W = 0;   // the plane that pair works on
    bool stream_seq = false;       // that third conv writes the recurrent layers' sequence layout (its rows can be carried over)
    size_t seq_floats = 0;         // ... floats per clip of it
    StreamState* stream = nullptr; // the open stream batch (nww_stream_*)
    EmbState* emb = nullptr;       // embedding-mode preprocessor state (nww_emb_*)
    // recording scoring (nww_recording.hip): the pool of a pass's interior frames [(B - 1) k + T][n_mels] (raw-PCM heads: rows of in_cols), and for the host-pointer entry
    // point the recording and its [2][nW] logits / probabilities; each grown on demand
    float* d_rec_pool = nullptr; int16_t* d_rec_pcm = nullptr; float* d_rec_out = nullptr;
    size_t rec_pool_bytes = 0, rec_pcm_bytes = 0, rec_out_bytes = 0;
    // cascade scoring (nww_cascade.hip), held by the VERIFIER's handle: the open windows' ascending indices [n], the dense [3][n] gate
    // probabilities / logits / probabilities of the host-pointer entry points, the select's per-block counts and total, and the pinned
    // word the count is read back through; the first two grown on demand
    int32_t* d_cas_idx = nullptr; float* d_cas_out = nullptr; int32_t* d_cas_counts = nullptr; int32_t* pin_cas_count = nullptr;
    size_t cas_idx_bytes = 0, cas_out_bytes = 0;
    // bank scoring (nww_bank.hip), held by the LEADER's handle: the dense [2][k][n] logits / probabilities of the host-pointer entry
    // points, grown on demand
    float* d_bank_out = nullptr; size_t bank_out_bytes = 0;
    struct MixState* mix = nullptr; // clip mixing (nww_mix.hip): the table slots and the host-pointer entry point's buffers, made by the first call
    struct ResampleState* resample = nullptr;   // recordings brought to the target rate (nww_resample.hip): ratios, table slots, the host form's buffers
    void* comm = nullptr;          // ncclComm_t of this rank (nww_comm_init)
    unsigned char* pin_in = nullptr; unsigned char* pin_out = nullptr;   // pinned staging for small host-pointer calls
    bool pin_in_busy = false;                                            // an async copy out of pin_in may still be in flight
    unsigned int done_seq = 0;                                           // completion-word sequence of the zero-copy small calls
    int comm_rank = 0, comm_world = 1;
    // the gather's own stream (nww_forward_pcm_gather_async_dev): step k's all-gather runs there behind ev_ready[k & 1] while step
    // k + 1's kernels run on the caller's stream; ev_gathered[k & 1] closes it, ev_start[k & 1] stamps the step's start (overlap probe)
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_ready[2] = {nullptr, nullptr}, ev_gathered[2] = {nullptr, nullptr}, ev_start[2] = {nullptr, nullptr};
    unsigned long long gather_seq = 0;
    const float* gather_buf[2] = {nullptr, nullptr};   // the d_all_logits each slot's gather last wrote
    long long gather_test_delay_us = 0;                // test hook, read ONCE at nww_comm_init (NWW_GATHER_TEST_DELAY_US)
    size_t splitk_per_clip = 0;    // floats per clip (max over the plan's split GEMMs)
    std::map<X3Key, void*> x3_weights;             // GEMM weights pre-split into bf16 terms / scaled binary16 terms (gemm_x3.hip)
    std::vector<void*> packed_weights;             // other plan-time weight packings (ffn_x3.hip)
    int conv_products = 0;                         // fused trunk: 0 = float32 MFMA, 6 | 9 = bf16 split products
    bool f16 = false;                              // NWW_ARITH_F16X3: conv_products = 6, and the layers that have a two-term binary16 instance and a bound on their input use it
    int cu_count = 256;
    // profiling: per forward, events[0..n] bracket the n launches; accumulated on nww_get_profile
    bool profiling = false;
    int prof_period = 1, prof_counter = 0;   // sampling: only every prof_period-th forward records events
    bool prof_active = false;
    std::vector<std::vector<hipEvent_t>> prof_runs;   // one event list per recorded forward
    std::vector<std::vector<int>> prof_ids;           // plan-entry id of each interval
    std::vector<hipEvent_t> event_pool;
    std::vector<double> prof_ms;                      // size plan+2 : [0]=frontend, [1..n]=plan, [n+1]=sigmoid
    std::vector<int> prof_cnt;
};


// ---- shared helpers (defined in nww_api.hip unless noted)
int nww_fail(nww_handle* h, int code, const char* fmt, ...);
std::string& nww_create_err();                 // nww_create / communicator errors: per thread
void nww_prof_mark(nww_handle* h, hipStream_t s, int id_of_next);
void nww_prof_begin(nww_handle* h);
int nww_check_run(nww_handle* h, int B);
int nww_ensure_ws(nww_handle* h, int B, int N);
int nww_grow(nww_handle* h, void** p, size_t* cap, size_t bytes);       // a device buffer grown on demand to hold `bytes`
// The followers of a bank call (nww_bank.hip): members[1 .. k) run their head plans on the dense head input the leader (members[0])
// has just written.  Follower j writes d_logits / d_probs + j * stride + offset (offset: the first item of a recording's pass), or with
// `own` its own nww_handle::d_logits / d_probs (a pool call, which scatters every member's scored results afterwards).
struct BankRun {
    nww_handle* const* members = nullptr; int k = 0;
    float* d_logits = nullptr; float* d_probs = nullptr;
    size_t stride = 0, offset = 0;
    bool own = false, probs = false;       // own: whether the followers compute probabilities
};
// a forward's optional inputs
struct RunOpts {
    bool x_frames_major = false;           // Run::x_frames_major
    unsigned int* done_flag = nullptr;     // zero-copy small calls: the completion word, its sequence number, and whether a step was armed to write it
    unsigned int done_seq = 0;
    bool* done_armed = nullptr;
    const HopView* hop = nullptr;          // a streaming hop
    const BankRun* bank = nullptr;         // a bank call: the followers run behind the leader's head
};
int nww_run_head(nww_handle* h, const float* d_x, int B, float* d_logits, float* d_probs, hipStream_t s, const RunOpts& o = RunOpts());
// the head of h on the dense frames-major d_x, then (o.bank) every follower's on the same d_x, all on s in member order
int nww_run_heads(nww_handle* h, const float* d_x, int B, float* d_logits, float* d_probs, hipStream_t s, const RunOpts& o);
int nww_frontend_on_dev(nww_handle* h, const int16_t* d_pcm, int B, int N, float* d_db, float* d_mel, int frames_major, hipStream_t s,
                        int* frames_out, size_t row_stride = 0, const Fe2Sub* sub = nullptr);
int nww_forward_pcm_on_dev(nww_handle* h, const int16_t* d_pcm, int B, int N, float* d_logits, float* d_probs, hipStream_t s,
                           size_t row_stride = 0, const RunOpts& o = RunOpts());
int nww_h2d_small(nww_handle* h, void* dst, const void* src, size_t bytes, hipStream_t s);
int nww_copy_out(nww_handle* h, int B, float* logits, float* probs, float* emb, hipStream_t s);
void nww_recording_free(nww_handle* h);        // nww_recording.hip, as the next two: what nww_cascade.hip scores a gate's recording with
long long nww_rec_count(long long n_samples, int W, int hop);
int nww_rec_forward_on_dev(nww_handle* h, const int16_t* d_pcm, long long n_samples, int W, int hop, int max_batch, float* d_logits, float* d_probs,
                           hipStream_t s, const BankRun* bank = nullptr);
// nww_stream.hip, as the next one: the checks every push_some shares (*done: n == 0, the call is complete), and the push itself on
// device pointers - what nww_cascade.hip runs a gate's pool call with
int nww_pool_push_check(nww_handle* h, const int32_t* idx, int32_t n, const void* chunk, bool* done);
int nww_pool_push_on_dev(nww_handle* h, const int32_t* idx, int n, const int16_t* d_chunk, float* d_logits, float* d_probs, hipStream_t s,
                         const PoolEntry** tab_out = nullptr, int* m_out = nullptr, const BankRun* bank = nullptr);
void nww_cascade_free(nww_handle* h);          // nww_cascade.hip
void nww_bank_free(nww_handle* h);             // nww_bank.hip
void nww_mix_free(nww_handle* h);              // nww_mix.hip
void nww_resample_free(nww_handle* h);         // nww_resample.hip
void nww_build_spec(nww_handle* h);            // nww_weights.hip, as the next eight: what nww_finalize does to the loaded weights before it plans
void balance_channel_gains(nww_handle* h);
void fold_batchnorms(nww_handle* h);
void transpose_depthwise(nww_handle* h);
void transpose_e2e_filters(nww_handle* h);
void fold_quartznet(nww_handle* h);
void fold_raw_frontend(nww_handle* h);
void fold_raw_backbone(nww_handle* h);
int upload_weight_arena(nww_handle* h);
int build_frontend_tables(nww_handle* h);
inline bool nww_raw_head(const nww_config& c) { return c.head_type == NWW_HEAD_E2E_QUARTZNET || c.head_type == NWW_HEAD_E2E_CNN; }
// floats per row of the frames-major head input: mel bins, or the channels of the raw-PCM frontend's last stage
inline int nww_row_floats(const nww_config& c) { return nww_raw_head(c) ? c.in_cols : c.n_mels; }
// rows the head's frontend yields for N samples: the STFT's frame count, or for the raw-PCM heads the strided convs' frame law
// (stage 0 stride 16, every later stage 4; zero padding, so any N >= 1 has rows)
inline int nww_pcm_rows(const nww_handle* h, int N) {
    if (!nww_raw_head(h->cfg)) return fe_num_frames(h->fe, N);
    int L = N;
    for (int i = 0; i < h->cfg.n_blocks; ++i) L = raw_conv_rows(L, i == 0 ? 16 : 4);
    return L < 1 ? -1 : L;
}
// a clip of N samples against the head: its rows T, the (rows, cols) feature shape they give, and whether that is the head's
struct ClipRows { int T, rows, cols; bool fits; };
inline ClipRows nww_clip_rows(const nww_handle* h, int N) {
    const nww_config& c = h->cfg;
    const int T = nww_pcm_rows(h, N);
    const int rows = c.mel_major_features ? c.n_mels : T, cols = nww_raw_head(c) ? c.in_cols : c.mel_major_features ? T : c.n_mels;
    return {T, rows, cols, T > 0 && rows == c.in_rows && cols == c.in_cols};
}
// ... and the error of a clip that has no rows, in the wording of its frontend
inline int nww_fail_short_clip(nww_handle* h, int N) {
    if (nww_raw_head(h->cfg)) return nww_fail(h, NWW_ERR_INVALID, "a clip needs at least one sample (got %d)", N);
    return nww_fail(h, NWW_ERR_INVALID, "clip of %d samples is too short for n_fft=%d (center=%d)", N, h->fe.n_fft, h->fe.center);
}
// window / hop rule and head shape of a stream batch or a recording, then what its hops share at NWW_STREAM_INC `level` (nww_stream.hip)
int nww_window_plan(nww_handle* h, int W, int hop, int level, HopPlan& p);
// the QuartzNet blocks' and fc's key prefix: the raw-PCM head holds them under model.backbone
// NWW_HEAD_E2E_CNN: RawAudioBackbone's four conv stages (architectures.py:739-762) on the channels-last plane [A = image W][Bd = image H]
struct RawCnnLayer { int cin, cout, sA, sB; };
inline const RawCnnLayer* nww_raw_cnn_layers() {
    static const RawCnnLayer L[4] = {{1, 24, 2, 1}, {24, 48, 2, 2}, {48, 64, 2, 2}, {64, 96, 1, 1}};
    return L;
}
inline std::string nww_quartznet_prefix(const nww_config& c) { return nww_raw_head(c) ? "model.backbone." : "model."; }
// NWW_HEAD_QUARTZNET: (Cin, Cout, k) of every block from the packed [channels, kernel, repetitions] entries (include/nww.h)
struct QnBlock { int cin, cout, k; };
inline std::vector<QnBlock> nww_quartznet_blocks(const nww_config& c) {
    std::vector<QnBlock> v;
    int cin = c.in_cols;
    for (int i = 0; i < c.n_crnn_channels && i < 4; ++i)
        for (int r = 0; r < (c.quartznet_kr[i] >> 16); ++r) { v.push_back({cin, c.crnn_channels[i], c.quartznet_kr[i] & 0xFFFF}); cin = c.crnn_channels[i]; }
    return v;
}

// The run-time knobs, read from the environment on the first call (nww_plan.hip).  Each selection knob defaults to the
// specialised kernel; setting it picks a general one.
struct Knobs {
    int trunk, conv_mfma, conv3_x3, gemm_x3, lin_x3, ffn_fused, attn_fused, merge_fused, qn_fused, raw_fused, conv2s_x3, rnn_ih_fused, mha_mfma, bc_front, bc_chain, tail, gemm_pp;
    int stream_inc;                            // NWW_STREAM_INC (nww_stream.hip)
    int rec_shared;                            // NWW_REC_SHARED (nww_recording.hip)
    int f16_range_log2;                        // test instrument: NWW_F16_RANGE_LOG2
};
const Knobs& nww_knobs();

#define fail nww_fail
#define HIP_TRY(h, expr)                                                                             \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail(h, NWW_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// the scores of n streams that hold no window yet: both outputs are 0, as the reference reports (nanointerpreter.py:785-786)
inline int nww_zero_scores(nww_handle* h, float* d_logits, float* d_probs, size_t n, hipStream_t s) {
    if (d_logits) HIP_TRY(h, hipMemsetAsync(d_logits, 0, n * sizeof(float), s));
    if (d_probs) HIP_TRY(h, hipMemsetAsync(d_probs, 0, n * sizeof(float), s));
    return NWW_OK;
}

