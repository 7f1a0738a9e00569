// nww_stream.hip - batched streaming: S lock-step device rings, one score per stream and hop (nww_stream_*).
#include "nww_internal.h"

// ------------------------------------------------------------------------------------------ streaming
__global__ void __launch_bounds__(256)
stream_push_kernel(int16_t* __restrict__ ring, const int16_t* __restrict__ chunk, int S, int W, int hop, int pos) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)S * hop) return;
    const int s = (int)(idx / hop), j = (int)(idx - (size_t)s * hop);
    int p = pos + j;
    if (p >= W) p -= W;
    const int16_t v = chunk[idx];
    int16_t* r = ring + (size_t)s * 2 * W;
    r[p] = v;
    r[p + W] = v;
}

// dense [B][n] <- the first n floats of every clip's slot (stride floats apart): the window of a log-mel ring for heads whose first
// kernel wants dense clips
__global__ void __launch_bounds__(256) stream_gather_kernel(const float4* __restrict__ src, float4* __restrict__ dst, int B, int n4, size_t stride4) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)B * n4) return;
    const int b = (int)(idx / n4), i = (int)(idx - (size_t)b * n4);
    dst[idx] = src[(size_t)b * stride4 + i];
}

extern "C" int nww_stream_close(nww_handle* h) {
    if (!h) return NWW_ERR_INVALID;
    if (!h->stream) return NWW_OK;
    (void)hipSetDevice(h->cfg.device);
    StreamState* st = h->stream;
    for (void* p : {(void*)st->d_ring, (void*)st->d_chunk, (void*)st->d_lm_ring, (void*)st->d_a2_ring, (void*)st->d_seq[0], (void*)st->d_seq[1]})
        if (p) (void)hipFree(p);
    delete st;
    h->stream = nullptr;
    return NWW_OK;
}

int nww_window_plan(nww_handle* h, int W, int hop, int level, HopPlan& p) {
    const nww_config& c = h->cfg;
    const ClipRows cr = nww_clip_rows(h, W);
    const bool fe_subsets = !nww_raw_head(c) && (!c.mel_major_features || h->e2e_transposed) && fe2_subset_supported(h->fe);
    // a raw-PCM head shares the rows of its last frontend stage where the one-launch frontend (and so its row-subset instance) is planned
    if (nww_raw_head(c)) p = nww_plan_hop_raw(c.n_blocks, W, hop, level, h->raw_fused);
    else p = nww_plan_hop(h->fe, cr.T, W, hop, level, fe_subsets, h->stream_conv && h->x_stride_ok && h->stream_H == cr.T, h->stream_seq,
                          [&](int a, int b) { return trunk_b_rows_fit(cr.T, h->stream_W, a, b); });
    if (!p.valid) return fail(h, NWW_ERR_INVALID, "window and hop must be positive multiples of 8 samples with hop <= window");
    if (!cr.fits)
        return fail(h, NWW_ERR_SHAPE, "a %d-sample window gives (%d,%d) features but the head expects (%d,%d)", W, cr.rows, cr.cols, c.in_rows, c.in_cols);
    return NWW_OK;
}

// NWW_STREAM_INC = 0: every hop re-scores the whole window (rounds 1-3), 1: frontend only, 2: + the fused trunk's rows, 3 (default):
// + the third conv's rows (HopPlan, stream_plan.h).  A raw-PCM head keeps the rows of its frontend's last stage in the same ring (rows of
// in_cols floats, raw_plan.h) wherever the hop is a whole number of them; otherwise it re-scores the whole window every hop.  One buffer per kept level.
static int stream_alloc(nww_handle* h, StreamState* st) {
    const int S = st->S, W = st->W;
    const HopPlan& p = st->plan;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMalloc(&st->d_ring, (size_t)S * 2 * W * sizeof(int16_t) + 16));
    HIP_TRY(h, hipMemset(st->d_ring, 0, (size_t)S * 2 * W * sizeof(int16_t)));
    HIP_TRY(h, hipMalloc(&st->d_chunk, (size_t)S * st->hop * sizeof(int16_t) + 16));
    if (p.shared) {
        st->lm_rows = (p.T + p.k - 1) / p.k * p.k;
        HIP_TRY(h, hipMalloc(&st->d_lm_ring, (size_t)S * 2 * st->lm_rows * nww_row_floats(h->cfg) * sizeof(float) + 16));
    }
    if (p.conv) HIP_TRY(h, hipMalloc(&st->d_a2_ring, (size_t)S * 32 * p.a2_rows * (h->stream_W / 4) * sizeof(float) + 16));
    for (int q = 0; q < 2 && p.seq; ++q) HIP_TRY(h, hipMalloc(&st->d_seq[q], (size_t)S * h->seq_floats * sizeof(float) + 16));
    return nww_ensure_ws(h, S, W);
}

extern "C" int nww_stream_open(nww_handle* h, int32_t S, int32_t W, int32_t hop) {
    int rc = nww_check_run(h, S);
    if (rc) return rc;
    HopPlan p;
    rc = nww_window_plan(h, W, hop, nww_knobs().stream_inc, p);
    if (rc) return rc;
    nww_stream_close(h);
    StreamState* st = h->stream = new StreamState();
    st->S = S; st->W = W; st->hop = hop; st->plan = p;
    rc = stream_alloc(h, st);
    if (rc) nww_stream_close(h);                    // no half-allocated stream batch stays open
    return rc;
}

extern "C" int nww_stream_reset(nww_handle* h) {
    if (!h || !h->stream) return fail(h, NWW_ERR_STATE, "no open stream batch");
    StreamState* st = h->stream;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemset(st->d_ring, 0, (size_t)st->S * 2 * st->W * sizeof(int16_t)));
    st->pos = 0; st->filled = 0;
    st->primed = false; st->lm_pos = 0; st->a2_pos = 0; st->seq_cur = 0;      // the next full window is computed whole
    return NWW_OK;
}

extern "C" int64_t nww_stream_filled(const nww_handle* h) { return h && h->stream ? h->stream->filled : 0; }

// What this hop hands to the plan's steps: the window's clip stride in the log-mel ring, and where the plan keeps pooled rows, the rings
// at their current rotation (mode 1: the first full window fills them, 2: a hop recomputes the plan's strips only).
static HopView stream_hop_view(const nww_handle* h, const StreamState* st, size_t x_stride) {
    const HopPlan& p = st->plan;
    HopView v;
    v.x_stride = x_stride;
    if (!p.conv) return v;
    v.mode = st->primed ? 2 : 1;
    v.a2_ring = st->d_a2_ring; v.a2_rows = p.a2_rows; v.a2_row0 = st->a2_pos;
    v.a2_ch_stride = (size_t)p.a2_rows * (h->stream_W / 4); v.a2_clip_stride = 32 * v.a2_ch_stride;
    if (p.seq) v.seq_new = st->d_seq[st->seq_cur];
    if (v.mode == 2) {
        v.a2_nsub = p.nsub;
        for (int q = 0; q < p.nsub; ++q) { v.a2_sub_a[q] = p.sub_a[q]; v.a2_sub_b[q] = p.sub_b[q]; }
        if (p.seq) { v.seq_prev = st->d_seq[st->seq_cur ^ 1]; v.a3_lo = p.a3_lo; v.a3_hi = p.a3_hi; v.a3_shift = p.a3_shift; }
    }
    return v;
}

// One hop on the incremental path: the invalidated frames (all of them for the first full window) -> log-mel ring -> head.
static int stream_hop_incremental(nww_handle* h, float* d_logits, float* d_probs, hipStream_t s) {
    const nww_config& c = h->cfg;
    StreamState* st = h->stream;
    const HopPlan& p = st->plan;
    const int S = st->S, W = st->W, T = p.T, k = p.k, cols = nww_row_floats(c);
    int rc = nww_ensure_ws(h, S, W);
    if (rc) return rc;
    nww_prof_begin(h);
    nww_prof_mark(h, s, 0);
    Fe2Sub sub;
    sub.ring_rows = st->lm_rows; sub.row0 = st->lm_pos; sub.out_clip_stride = (size_t)2 * st->lm_rows * cols;
    if (st->primed) {
        if (p.el > 0) { sub.t0[sub.nr] = 0; sub.t1[sub.nr] = p.el; ++sub.nr; }
        // the new interior frames, then the trailing edge frames as a group of their own (groups of up to eight frames)
        sub.t0[sub.nr] = T - p.er - k; sub.t1[sub.nr] = T - p.er; ++sub.nr;
        if (p.er > 0) { sub.t0[sub.nr] = T - p.er; sub.t1[sub.nr] = T; ++sub.nr; }
    }
    rc = nww_frontend_on_dev(h, st->d_ring + st->pos, S, W, st->d_lm_ring, nullptr, 1, s, nullptr, (size_t)2 * W, &sub);
    if (rc) return rc;
    const float* win = st->d_lm_ring + (size_t)st->lm_pos * cols;          // rows [lm_pos, lm_pos + T) of every stream's ring: its window
    RunOpts o;
    if (h->x_stride_ok) {
        const HopView v = stream_hop_view(h, st, sub.out_clip_stride);
        o.hop = &v;
        rc = nww_run_head(h, win, S, d_logits, d_probs, s, o);
    } else {
        const int n4 = T * cols / 4;
        const size_t total = (size_t)S * n4;
        hipLaunchKernelGGL(stream_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(win),
                           reinterpret_cast<float4*>(h->d_logmel), S, n4, sub.out_clip_stride / 4);
        HIP_TRY(h, hipGetLastError());
        o.x_frames_major = c.mel_major_features != 0;
        rc = nww_run_head(h, h->d_logmel, S, d_logits, d_probs, s, o);
    }
    if (rc) return rc;
    st->lm_pos = (st->lm_pos + k) % st->lm_rows;
    if (p.conv) st->a2_pos = (st->a2_pos + p.a2_shift) % p.a2_rows;
    if (p.seq) st->seq_cur ^= 1;
    st->primed = true;
    return NWW_OK;
}

static int stream_push_dev(nww_handle* h, const int16_t* d_chunk, float* d_logits, float* d_probs, hipStream_t s) {
    StreamState* st = h->stream;
    const int S = st->S, W = st->W, hop = st->hop;
    const size_t total = (size_t)S * hop;
    hipLaunchKernelGGL(stream_push_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st->d_ring, d_chunk, S, W, hop, st->pos);
    HIP_TRY(h, hipGetLastError());
    st->pos = (st->pos + hop) % W;
    st->filled += hop;
    // the last W samples of every stream are contiguous at ring + pos (double-written ring)
    if (st->filled < W) {       // window not full yet: the reference reports 0.0 (nanointerpreter.py:785-786)
        if (d_logits) HIP_TRY(h, hipMemsetAsync(d_logits, 0, (size_t)S * sizeof(float), s));
        if (d_probs) HIP_TRY(h, hipMemsetAsync(d_probs, 0, (size_t)S * sizeof(float), s));
        return NWW_OK;
    }
    if (st->plan.shared) {
        const int rc = stream_hop_incremental(h, d_logits, d_probs, s);
        if (rc) st->primed = false;           // the rings may hold a half-finished hop: the next hop computes its window whole
        return rc;
    }
    return nww_forward_pcm_on_dev(h, st->d_ring + st->pos, S, W, d_logits, d_probs, s, (size_t)2 * W);
}
extern "C" int nww_stream_push_dev(nww_handle* h, const int16_t* d_chunk, float* d_logits, float* d_probs, void* stream) {
    if (!h || !h->stream) return fail(h, NWW_ERR_STATE, "no open stream batch (nww_stream_open)");
    if (!d_chunk) return fail(h, NWW_ERR_INVALID, "null chunk pointer");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return stream_push_dev(h, d_chunk, d_logits, d_probs, stream ? (hipStream_t)stream : h->own_stream);
}

extern "C" int nww_stream_push(nww_handle* h, const int16_t* chunk, float* logits, float* probs) {
    if (!h || !h->stream) return fail(h, NWW_ERR_STATE, "no open stream batch (nww_stream_open)");
    if (!chunk) return fail(h, NWW_ERR_INVALID, "Input audio must be a non-null int16 array");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = h->own_stream;
    const int S = h->stream->S;
    { int rcs = nww_h2d_small(h, h->stream->d_chunk, chunk, (size_t)S * h->stream->hop * sizeof(int16_t), s); if (rcs) return rcs; }
    int rc = stream_push_dev(h, h->stream->d_chunk, h->d_logits, h->d_probs, s);
    if (rc) return rc;
    return nww_copy_out(h, S, logits, probs, nullptr, s);
}

