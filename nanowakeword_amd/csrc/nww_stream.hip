// nww_stream.hip - batched streaming: S device rings, one score per stream and hop (nww_stream_*).  The lock-step calls push every
// stream, the pool calls the listed ones; both move the one ring state of stream_pool.h, which also decides what a hop may reuse.
#include "nww_internal.h"
#include "cascade.h"

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

// ---- the pool's kernels (nww_stream_push_some): data movement only, one thread per 16 bytes, consecutive threads on consecutive
// addresses of one row; each follows the call's table (PoolEntry, stream_pool.h)
// chunk row i -> stream tab[i].stream's double-written PCM ring at the position the push started from (pos - hop, modulo W).  V: uint4
// (8 samples: positions, hop and W are multiples of 8, so a vector never straddles the ring's end) or int16_t for a chunk pointer that
// is not 16-byte aligned.
template <class V>
__global__ void __launch_bounds__(256)
pool_push_kernel(int16_t* __restrict__ ring, const int16_t* __restrict__ chunk, const PoolEntry* __restrict__ tab, int n, int W, int hop) {
    constexpr int E = (int)(sizeof(V) / sizeof(int16_t));
    const int per = hop / E;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * per) return;
    const int i = (int)(idx / per), j = (int)(idx - (size_t)i * per) * E;
    const PoolEntry e = tab[i];
    int p = e.pos - hop + j;
    if (p < 0) p += W;
    if (p >= W) p -= W;
    const V v = *reinterpret_cast<const V*>(chunk + (size_t)i * hop + j);
    int16_t* r = ring + (size_t)e.stream * 2 * W;
    *reinterpret_cast<V*>(r + p) = v;
    *reinterpret_cast<V*>(r + p + W) = v;
}

// Route 1: each scored stream's window out of its ring (at its own position) into row e.slot of the PCM staging [m][W]: a whole
// window, or for a primed stream only the samples the frames of its hop read - vectors [0, head8) and [tail8, W8) of the window
// (pool_primed_spans).  per: the most vectors any stream of the call has.
__global__ void __launch_bounds__(256)
pool_stage_kernel(const uint4* __restrict__ ring, uint4* __restrict__ pcm, const PoolEntry* __restrict__ tab, int n, int W8, int head8, int tail8, int per) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * per) return;
    const int i = (int)(idx / per), q = (int)(idx - (size_t)i * per);
    const PoolEntry e = tab[i];
    if (e.group == POOL_NOT_FULL || (e.group == POOL_PRIMED && q >= head8 + W8 - tail8)) return;
    const int v = (e.group == POOL_WHOLE || q < head8) ? q : tail8 + (q - head8);
    pcm[(size_t)e.slot * W8 + v] = ring[((size_t)e.stream * 2 * W8 + e.pos / 8) + v];
}

// The frontend's rows in the scratch [m][T][cols] -> each scored stream's own log-mel ring: frame t at row lm_row + t and again lm_rows
// away.  A primed stream's rows are the first el and the last k + er frames (r enumerates them); a whole window's are all T.  rows:
// the most rows any stream of the call has.
__global__ void __launch_bounds__(256)
pool_place_kernel(const float4* __restrict__ scratch, float4* __restrict__ lm_ring, const PoolEntry* __restrict__ tab, int n, int T, int cols4,
                  int lm_rows, int el, int tail, int rows) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int per = rows * cols4;
    if (idx >= (size_t)n * per) return;
    const int i = (int)(idx / per), q = (int)(idx - (size_t)i * per), r = q / cols4, c = q - r * cols4;
    const PoolEntry e = tab[i];
    if (e.group == POOL_NOT_FULL || (e.group == POOL_PRIMED && r >= el + tail)) return;
    const int t = (e.group == POOL_WHOLE || r < el) ? r : T - tail + (r - el);
    const int x = e.lm_row + t, y = x < lm_rows ? x + lm_rows : x - lm_rows;
    const float4 v = scratch[((size_t)e.slot * T + t) * cols4 + c];
    float4* base = lm_ring + (size_t)e.stream * 2 * lm_rows * cols4;
    base[(size_t)x * cols4 + c] = v;
    base[(size_t)y * cols4 + c] = v;
}

// each scored stream's window - the T rows at its own rotation lm_row - -> the dense head input [m][T][cols], row e.dense
__global__ void __launch_bounds__(256)
pool_gather_kernel(const float4* __restrict__ lm_ring, float4* __restrict__ dst, const PoolEntry* __restrict__ tab, int n, int n4, int cols4, int lm_rows) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * n4) return;
    const int i = (int)(idx / n4), q = (int)(idx - (size_t)i * n4);
    const PoolEntry e = tab[i];
    if (e.group == POOL_NOT_FULL) return;
    dst[(size_t)e.dense * n4 + q] = lm_ring[((size_t)e.stream * 2 * lm_rows + e.lm_row) * cols4 + q];
}

extern "C" int nww_stream_close(nww_handle* h) {
    if (!h) return NWW_ERR_INVALID;
    if (!h->stream) return NWW_OK;
    (void)hipSetDevice(h->cfg.device);
    StreamState* st = h->stream;
    for (void* p : {(void*)st->d_ring, (void*)st->d_chunk, (void*)st->d_lm_ring, (void*)st->d_a2_ring, (void*)st->d_seq[0], (void*)st->d_seq[1],
                    (void*)st->d_lm_scratch, (void*)st->d_tab, (void*)st->d_pool_out})
        if (p) (void)hipFree(p);
    if (st->pin_tab) { (void)hipDeviceSynchronize(); (void)hipHostFree(st->pin_tab); }       // (a table's upload may still be in flight)
    for (hipEvent_t e : st->ev_tab)
        if (e) (void)hipEventDestroy(e);
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
    if (rc) { nww_stream_close(h); return rc; }     // no half-allocated stream batch stays open
    // pool calls maintain the log-mel rings for the mel heads; a raw-PCM head re-scores whole windows in pool mode
    st->pool.open(S, W, hop);
    if (p.shared && nww_raw_head(h->cfg)) st->pool.keep_ring(st->lm_rows, p.k);
    else if (p.shared) {
        int head, tail;
        pool_primed_spans(h->fe, W, p.T, p.k, p.el, p.er, head, tail);
        st->pool.keep_frames(st->lm_rows, p.T, p.k, p.el, p.er, head, tail);
    }
    return NWW_OK;
}

extern "C" int nww_stream_reset(nww_handle* h) {
    if (!h || !h->stream) return fail(h, NWW_ERR_STATE, "no open stream batch");
    StreamState* st = h->stream;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemset(st->d_ring, 0, (size_t)st->S * 2 * st->W * sizeof(int16_t)));
    pool_reset_all(st->pool);                                  // every stream shares one state again; the next full window is computed whole
    st->a2_pos = 0; st->seq_cur = 0; st->rows_held = false;
    return NWW_OK;
}

// (the batch's count while its streams are aligned; afterwards what it was when alignment ended)
extern "C" int64_t nww_stream_filled(const nww_handle* h) { return h && h->stream ? h->stream->pool.all.filled : 0; }

// What this hop hands to the plan's steps: the window's clip stride in the log-mel ring, and where the plan keeps pooled rows, the rings
// at their current rotation (mode 1: the first full window fills them, 2: a hop recomputes the plan's strips only).
static HopView stream_hop_view(const nww_handle* h, const StreamState* st, size_t x_stride, bool primed) {
    const HopPlan& p = st->plan;
    HopView v;
    v.x_stride = x_stride;
    if (!p.conv) return v;
    v.mode = primed ? 2 : 1;
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

// One hop on the incremental path: the invalidated frames (all of them where a ring does not hold the previous window) -> log-mel ring
// -> head.
static int stream_hop_incremental(nww_handle* h, const LockHop& hp, float* d_logits, float* d_probs, hipStream_t s) {
    const nww_config& c = h->cfg;
    StreamState* st = h->stream;
    const HopPlan& p = st->plan;
    const int S = st->S, W = st->W, T = p.T, cols = nww_row_floats(c);
    const bool primed = hp.primed && (!p.conv || st->rows_held);           // every ring the plan keeps holds the previous window
    int rc = nww_ensure_ws(h, S, W);
    if (rc) return rc;
    nww_prof_begin(h);
    nww_prof_mark(h, s, 0);
    Fe2Sub sub;
    sub.ring_rows = st->lm_rows; sub.row0 = hp.lm_row; sub.out_clip_stride = (size_t)2 * st->lm_rows * cols;
    if (primed) nww_hop_ranges(T, p.k, p.el, p.er, sub);
    rc = nww_frontend_on_dev(h, st->d_ring + hp.pos, S, W, st->d_lm_ring, nullptr, 1, s, nullptr, (size_t)2 * W, &sub);
    if (rc) return rc;
    const float* win = st->d_lm_ring + (size_t)hp.lm_row * cols;           // rows [lm_row, lm_row + T) of every stream's ring: its window
    RunOpts o;
    if (h->x_stride_ok) {
        const HopView v = stream_hop_view(h, st, sub.out_clip_stride, primed);
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
    if (p.conv) st->a2_pos = (st->a2_pos + p.a2_shift) % p.a2_rows;
    if (p.seq) st->seq_cur ^= 1;
    return NWW_OK;
}

static int stream_push_dev(nww_handle* h, const int16_t* d_chunk, float* d_logits, float* d_probs, hipStream_t s) {
    StreamState* st = h->stream;
    const int S = st->S, W = st->W, hop = st->hop;
    const LockHop hp = pool_lock_plan(st->pool);
    const size_t total = (size_t)S * hop;
    hipLaunchKernelGGL(stream_push_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st->d_ring, d_chunk, S, W, hop, hp.at);
    HIP_TRY(h, hipGetLastError());
    // the last W samples of every stream are contiguous at ring + pos (double-written ring)
    const int rc = !hp.full ? nww_zero_scores(h, d_logits, d_probs, S, s)
                 : st->plan.shared ? stream_hop_incremental(h, hp, d_logits, d_probs, s)
                                   : nww_forward_pcm_on_dev(h, st->d_ring + hp.pos, S, W, d_logits, d_probs, s, (size_t)2 * W);
    pool_lock_commit(st->pool, hp, rc == NWW_OK);      // (a failed hop may have left the rings half-finished: the next one computes its window whole)
    st->rows_held = hp.full && rc == NWW_OK;
    return rc;
}
// the lock-step entry points run while every stream shares one state
static int stream_lockstep(nww_handle* h) {
    if (pool_lock_ok(h->stream->pool)) return NWW_OK;
    return fail(h, NWW_ERR_STATE, "the streams of this batch no longer share one state (nww_stream_push_some / nww_stream_reset_some made them "
                                  "differ): a lock-step push needs nww_stream_reset first");
}

extern "C" int nww_stream_push_dev(nww_handle* h, const int16_t* d_chunk, float* d_logits, float* d_probs, void* stream) {
    if (!h || !h->stream) return fail(h, NWW_ERR_STATE, "no open stream batch (nww_stream_open)");
    if (!d_chunk) return fail(h, NWW_ERR_INVALID, "null chunk pointer");
    { const int rc = stream_lockstep(h); if (rc) return rc; }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return stream_push_dev(h, d_chunk, d_logits, d_probs, stream ? (hipStream_t)stream : h->own_stream);
}

extern "C" int nww_stream_push(nww_handle* h, const int16_t* chunk, float* logits, float* probs) {
    if (!h || !h->stream) return fail(h, NWW_ERR_STATE, "no open stream batch (nww_stream_open)");
    if (!chunk) return fail(h, NWW_ERR_INVALID, "Input audio must be a non-null int16 array");
    { const int rc = stream_lockstep(h); if (rc) return rc; }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = h->own_stream;
    const int S = h->stream->S;
    { int rcs = nww_h2d_small(h, h->stream->d_chunk, chunk, (size_t)S * h->stream->hop * sizeof(int16_t), s); if (rcs) return rcs; }
    int rc = stream_push_dev(h, h->stream->d_chunk, h->d_logits, h->d_probs, s);
    if (rc) return rc;
    return nww_copy_out(h, S, logits, probs, nullptr, s);
}

// ------------------------------------------------------------------------------------------ streams that push, join and reset on their own
// The pool calls maintain the PCM and (route 1) log-mel rings, not the lock-step path's conv-row and sequence rings: each clears
// StreamState::rows_held.
static int pool_alloc(nww_handle* h, StreamState* st) {
    if (st->d_tab) return NWW_OK;
    const size_t S = (size_t)st->S;
    if (S * 2 * (size_t)st->W / 8 > 0x7fffffffull) return fail(h, NWW_ERR_UNSUPPORTED, "%d streams of %d samples: the rings exceed the table's 32-bit window offsets", st->S, st->W);
    st->tab_slot_bytes = (S * (sizeof(PoolEntry) + 2 * sizeof(int32_t)) + 15) & ~(size_t)15;
    HIP_TRY(h, hipMalloc(&st->d_tab, POOL_TAB_SLOTS * st->tab_slot_bytes));
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&st->pin_tab), POOL_TAB_SLOTS * st->tab_slot_bytes, hipHostMallocDefault));
    for (hipEvent_t& e : st->ev_tab) HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(h, hipMalloc(&st->d_pool_out, 2 * S * sizeof(float) + 16));
    if (st->pool.frames) HIP_TRY(h, hipMalloc(&st->d_lm_scratch, S * st->pool.T * nww_row_floats(h->cfg) * sizeof(float) + 16));
    return NWW_OK;
}

// (tab_out / m_out: the call's table [n] on the device and its count of scored streams, for a caller that enqueues on s right behind
// the call - nww_cascade.hip; the table's slot is rewritten POOL_TAB_SLOTS calls later at the earliest)
int nww_pool_push_on_dev(nww_handle* h, const int32_t* idx, int n, const int16_t* d_chunk, float* d_logits, float* d_probs, hipStream_t s,
                         const PoolEntry** tab_out, int* m_out, const BankRun* bank) {
    StreamState* st = h->stream;
    StreamPool& pool = st->pool;
    const int W = st->W, hop = st->hop;
    int rc = pool_alloc(h, st);
    if (!rc) rc = nww_ensure_ws(h, st->S, W);
    if (rc) return rc;
    st->rows_held = false;
    PoolCall c;
    pool_plan_push(pool, idx, n, c);
    const int m = c.m();
    st->stat_scored = m;
    st->stat_frames = pool.frames ? (long long)c.n_whole * pool.frames_of(POOL_WHOLE) + (long long)c.n_primed * pool.frames_of(POOL_PRIMED)
                                  : (long long)m * nww_pcm_rows(h, W);
    // the call's table: [n] entries, [m] window offsets (slot order), [m] output indices (dense order), through the next pinned slot
    const unsigned slot = st->tab_seq++ % POOL_TAB_SLOTS;
    unsigned char* pin = st->pin_tab + slot * st->tab_slot_bytes;
    unsigned char* dev = st->d_tab + slot * st->tab_slot_bytes;
    if (st->tab_seq > POOL_TAB_SLOTS) HIP_TRY(h, hipEventSynchronize(st->ev_tab[slot]));      // the slot's previous call has passed
    const size_t nb_e = (size_t)n * sizeof(PoolEntry), nb_m = (size_t)m * sizeof(int32_t);
    std::memcpy(pin, c.entries.data(), nb_e);
    if (m) { std::memcpy(pin + nb_e, c.win8.data(), nb_m); std::memcpy(pin + nb_e + nb_m, c.out.data(), nb_m); }
    HIP_TRY(h, hipMemcpyAsync(dev, pin, nb_e + 2 * nb_m, hipMemcpyHostToDevice, s));
    const PoolEntry* tab = reinterpret_cast<const PoolEntry*>(dev);
    const int32_t* d_win8 = reinterpret_cast<const int32_t*>(dev + nb_e);
    const int32_t* d_out = reinterpret_cast<const int32_t*>(dev + nb_e + nb_m);
    if (tab_out) *tab_out = tab;
    if (m_out) *m_out = m;
    auto launches = [&]() -> int {
        // (1) the chunk rows into the rings, each at its own position
        if ((uintptr_t)d_chunk % 16 == 0) {
            const size_t total = (size_t)n * (hop / 8);
            hipLaunchKernelGGL(pool_push_kernel<uint4>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st->d_ring, d_chunk, tab, n, W, hop);
        } else {
            const size_t total = (size_t)n * hop;
            hipLaunchKernelGGL(pool_push_kernel<int16_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st->d_ring, d_chunk, tab, n, W, hop);
        }
        HIP_TRY(h, hipGetLastError());
        // a listed stream that holds no window yet reports 0; the scored ones are scattered over that
        // (a bank's outputs are [k][n]: every member's row)
        const int k = bank ? bank->k : 1;
        if (m < n) {
            const int rcz = nww_zero_scores(h, d_logits, d_probs, (size_t)n * k, s);
            if (rcz) return rcz;
        }
        if (m == 0) return NWW_OK;
        hipError_t e;
        float* lg = h->d_logits;
        float* pr = d_probs ? h->d_probs : nullptr;
        RunOpts o;
        o.bank = bank;
        if (!pool.frames) {                                      // route 0: whole windows (slot order is dense order)
            // (2) the scored streams' windows out of their rings into the PCM staging [m][W]
            e = launch_cascade_gather(st->d_ring, d_win8, 8, W, m, h->d_pcm, s);
            if (e != hipSuccess) return fail(h, NWW_ERR_HIP, "launch 'cascade_gather' failed: %s", hipGetErrorString(e));
            const int rc0 = nww_forward_pcm_on_dev(h, h->d_pcm, m, W, lg, pr, s, 0, o);
            if (rc0) return rc0;
        } else {                                                 // route 1: shared frames
            const nww_config& cfg = h->cfg;
            const int T = pool.T, cols = nww_row_floats(cfg), tail = pool.k + pool.er;
            nww_prof_begin(h);
            nww_prof_mark(h, s, 0);
            // (2) the windows into the PCM staging, in slot order; of a primed stream's window only what its hop's frames read
            {
                const int W8 = W / 8, head8 = pool.head / 8, tail8 = pool.tail / 8, per = c.n_whole ? W8 : head8 + W8 - tail8;
                const size_t total = (size_t)n * per;
                hipLaunchKernelGGL(pool_stage_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const uint4*>(st->d_ring),
                                   reinterpret_cast<uint4*>(h->d_pcm), tab, n, W8, head8, tail8, per);
                HIP_TRY(h, hipGetLastError());
            }
            // (3) the frontend on the staging, a launch per group: whole windows, then the rows a hop invalidates (the row-subset instance,
            // dense output: each row at its place in the scratch [m][T][cols])
            if (c.n_whole) {
                const int rc1 = nww_frontend_on_dev(h, h->d_pcm, c.n_whole, W, st->d_lm_scratch, nullptr, 1, s, nullptr);
                if (rc1) return rc1;
            }
            if (c.n_primed) {
                Fe2Sub sub;
                nww_hop_ranges(T, pool.k, pool.el, pool.er, sub);
                const int rc1 = nww_frontend_on_dev(h, h->d_pcm + (size_t)c.n_whole * W, c.n_primed, W, st->d_lm_scratch + (size_t)c.n_whole * T * cols,
                                                    nullptr, 1, s, nullptr, (size_t)W, &sub);
                if (rc1) return rc1;
            }
            // (4) those rows into each stream's own ring, (5) each stream's window out of its own rotation into the dense head input
            const int cols4 = cols / 4, rows = c.n_whole ? T : pool.el + tail;
            size_t total = (size_t)n * rows * cols4;
            hipLaunchKernelGGL(pool_place_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(st->d_lm_scratch),
                               reinterpret_cast<float4*>(st->d_lm_ring), tab, n, T, cols4, pool.lm_rows, pool.el, tail, rows);
            HIP_TRY(h, hipGetLastError());
            total = (size_t)n * T * cols4;
            hipLaunchKernelGGL(pool_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(st->d_lm_ring),
                               reinterpret_cast<float4*>(h->d_logmel), tab, n, T * cols4, cols4, pool.lm_rows);
            HIP_TRY(h, hipGetLastError());
            o.x_frames_major = cfg.mel_major_features != 0;
            const int rc1 = nww_run_heads(h, h->d_logmel, m, lg, pr, s, o);
            if (rc1) return rc1;
        }
        // (6) the m results into the [n] outputs
        for (int j = 0; j < k && (d_logits || d_probs); ++j) {        // (a follower's results lie in its own d_logits / d_probs)
            const nww_handle* f = j ? bank->members[j] : h;
            e = launch_cascade_scatter(d_out, m, j ? f->d_logits : lg, !pr ? nullptr : j ? f->d_probs : pr, d_logits ? d_logits + (size_t)j * n : nullptr,
                                       d_probs ? d_probs + (size_t)j * n : nullptr, s);
            if (e != hipSuccess) return fail(h, NWW_ERR_HIP, "launch 'cascade_scatter' failed: %s", hipGetErrorString(e));
        }
        return NWW_OK;
    };
    rc = launches();
    (void)hipEventRecord(st->ev_tab[slot], s);
    pool_commit_push(pool, c, rc == NWW_OK);
    return rc;
}

// the checks every push_some shares; *done: the call is complete (n == 0)
int nww_pool_push_check(nww_handle* h, const int32_t* idx, int32_t n, const void* chunk, bool* done) {
    *done = false;
    if (!h) return NWW_ERR_INVALID;
    if (!h->stream) return fail(h, NWW_ERR_STATE, "no open stream batch (nww_stream_open)");
    if (!pool_idx_ok(idx, n, h->stream->S))
        return fail(h, NWW_ERR_INVALID, "idx must hold n >= 0 strictly ascending stream numbers in [0, %d)", h->stream->S);
    if (n == 0) { *done = true; h->stream->stat_scored = 0; h->stream->stat_frames = 0; return NWW_OK; }
    if (!chunk) return fail(h, NWW_ERR_INVALID, "null chunk pointer");
    return NWW_OK;
}

extern "C" int nww_stream_push_some_dev(nww_handle* h, const int32_t* idx, int32_t n, const int16_t* d_chunk, float* d_logits, float* d_probs, void* stream) {
    bool done;
    const int rc = nww_pool_push_check(h, idx, n, d_chunk, &done);
    if (rc || done) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return nww_pool_push_on_dev(h, idx, n, d_chunk, d_logits, d_probs, stream ? (hipStream_t)stream : h->own_stream);
}

extern "C" int nww_stream_push_some(nww_handle* h, const int32_t* idx, int32_t n, const int16_t* chunk, float* logits, float* probs) {
    bool done;
    int rc = nww_pool_push_check(h, idx, n, chunk, &done);
    if (rc || done) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    StreamState* st = h->stream;
    hipStream_t s = h->own_stream;
    rc = pool_alloc(h, st);
    if (rc) return rc;
    rc = nww_h2d_small(h, st->d_chunk, chunk, (size_t)n * st->hop * sizeof(int16_t), s);
    if (rc) return rc;
    float* out = st->d_pool_out;
    rc = nww_pool_push_on_dev(h, idx, n, st->d_chunk, logits ? out : nullptr, probs ? out + st->S : nullptr, s);
    if (!rc && logits) HIP_TRY(h, hipMemcpyAsync(logits, out, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (!rc && probs) HIP_TRY(h, hipMemcpyAsync(probs, out + st->S, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->pin_in_busy = false;
    return rc;
}

extern "C" int nww_stream_reset_some(nww_handle* h, const int32_t* idx, int32_t n) {
    if (!h) return NWW_ERR_INVALID;
    if (!h->stream) return fail(h, NWW_ERR_STATE, "no open stream batch (nww_stream_open)");
    StreamState* st = h->stream;
    if (!pool_idx_ok(idx, n, st->S)) return fail(h, NWW_ERR_INVALID, "idx must hold n >= 0 strictly ascending stream numbers in [0, %d)", st->S);
    if (n == 0) return NWW_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipDeviceSynchronize());
    const size_t row = (size_t)2 * st->W * sizeof(int16_t);
    for (int i = 0; i < n;) {                                    // one memset per run of consecutive streams
        int j = i + 1;
        while (j < n && idx[j] == idx[j - 1] + 1) ++j;
        HIP_TRY(h, hipMemset(reinterpret_cast<unsigned char*>(st->d_ring) + (size_t)idx[i] * row, 0, (size_t)(j - i) * row));
        i = j;
    }
    st->rows_held = false;
    pool_reset(st->pool, idx, n);
    return NWW_OK;
}

extern "C" int64_t nww_stream_filled_of(const nww_handle* h, int32_t stream) {
    if (!h || !h->stream || stream < 0 || stream >= h->stream->S) return 0;
    return h->stream->pool.of(stream).filled;
}

extern "C" int nww_stream_pool_stats(const nww_handle* h, int32_t* n_scored, int32_t* route, int64_t* frames_computed) {
    if (!h || !h->stream) return NWW_ERR_STATE;
    const StreamState* st = h->stream;
    if (n_scored) *n_scored = st->stat_scored;
    if (route) *route = st->pool.frames ? 1 : 0;
    if (frames_computed) *frames_computed = st->stat_frames;
    return NWW_OK;
}
