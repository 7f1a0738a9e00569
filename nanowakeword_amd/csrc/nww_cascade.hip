// nww_cascade.hip - gate + verifier cascades (nww_cascade_*): the gate scores every window, cascade_select compacts the open ones on the
// device, and the verifier runs nww_forward_pcm_on_dev on them alone - gathered into its own PCM staging, scattered back into dense
// per-window outputs.  Three inputs share one back half (cas_verify): a batch of clips (row_stride = N), every window of a recording
// (row_stride = hop) and S lock-step streams (the gate's PCM ring, row_stride = 2 W).  A fourth, the listed streams of a batch whose
// streams push on their own (cas_pool_push_dev), shares the verifier's chunk with it (cas_verify_chunk): its select walks the table of
// the gate's pool call and its gather follows ring offsets (row_stride = 8).  Launch-side code and the kernels of
// cascade.hip only: no frontend or head kernel is added or changed.  State (index lists, dense outputs of the host-pointer variants,
// block counts, the pinned count) lives on the VERIFIER's handle, and errors go to nww_last_error(verifier).
#include "nww_internal.h"
#include "cascade.h"

namespace {

int cas_check(nww_handle* g, nww_handle* v) {
    if (!v) return NWW_ERR_INVALID;
    if (!g) return fail(v, NWW_ERR_INVALID, "a cascade needs a gate handle");
    if (g == v) return fail(v, NWW_ERR_INVALID, "a cascade needs two distinct handles: the gate and the verifier are the same one");
    if (!g->finalized || !v->finalized)
        return fail(v, NWW_ERR_INVALID, "%s: model not finalized: call nww_finalize after loading the state_dict", g->finalized ? "verifier" : "gate");
    if (g->cfg.device != v->cfg.device)
        return fail(v, NWW_ERR_INVALID, "the gate is on device %d and the verifier on device %d: a cascade runs on one", g->cfg.device, v->cfg.device);
    return NWW_OK;
}

// an error of the gate's own calls, reported where a cascade's errors go
int cas_gate_fail(nww_handle* g, nww_handle* v, int rc) { return fail(v, rc, "gate: %s", g->err.c_str()); }

// a clip of N samples against one of the two heads, in nww_forward_pcm's wording
int cas_clip_fits(nww_handle* v, nww_handle* h, const char* who, int N) {
    const ClipRows cr = nww_clip_rows(h, N);
    if (cr.T <= 0) {
        nww_fail_short_clip(h, N);
        const std::string text = h->err;
        return fail(v, NWW_ERR_INVALID, "%s: %s", who, text.c_str());
    }
    if (!cr.fits)
        return fail(v, NWW_ERR_SHAPE, "%s: frontend yields (%d,%d) features for %d samples but the head was built for input_shape=(%d,%d)", who,
                    cr.rows, cr.cols, N, h->cfg.in_rows, h->cfg.in_cols);
    return NWW_OK;
}

// ... and a (window, hop) pair, in nww_stream_open's and nww_forward_recording's
int cas_window_fits(nww_handle* v, nww_handle* h, const char* who, int W, int hop) {
    HopPlan p;
    const int rc = nww_window_plan(h, W, hop, 0, p);
    if (!rc) return NWW_OK;
    const std::string text = h->err;
    return fail(v, rc, "%s: %s", who, text.c_str());
}

// the index list for n windows and `planes` dense [n] float outputs (3: a host-pointer call's gate probabilities, logits and probabilities;
// 1: the gate probabilities a _dev caller did not ask for, or nww_cascade_select's uploaded scores; 0: none)
// (lists = 2: a pool call's two index lists, ring offsets [n] then entries [n])
int cas_state(nww_handle* v, long long n, int planes, int lists = 1) {
    int rc = nww_grow(v, reinterpret_cast<void**>(&v->d_cas_idx), &v->cas_idx_bytes, (size_t)lists * n * sizeof(int32_t));
    if (rc) return rc;
    if (planes > 0) {
        rc = nww_grow(v, reinterpret_cast<void**>(&v->d_cas_out), &v->cas_out_bytes, (size_t)planes * n * sizeof(float));
        if (rc) return rc;
    }
    if (!v->d_cas_counts) HIP_TRY(v, hipMalloc(reinterpret_cast<void**>(&v->d_cas_counts), CASCADE_COUNT_INTS * sizeof(int32_t) + 16));
    if (!v->pin_cas_count) HIP_TRY(v, hipHostMalloc(reinterpret_cast<void**>(&v->pin_cas_count), 16, hipHostMallocDefault));
    return NWW_OK;
}

// a select's count read back: ONE 4-byte copy into pinned memory behind ONE synchronisation of s.  The count is checked before anything
// is sized by it.
int cas_read_count(nww_handle* v, long long n, int* n_open, hipStream_t s) {
    *v->pin_cas_count = -1;
    HIP_TRY(v, hipMemcpyAsync(v->pin_cas_count, v->d_cas_counts + CASCADE_MAX_BLOCKS, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(v, hipStreamSynchronize(s));
    const long long c = *v->pin_cas_count;
    if (c < 0 || c > n) return fail(v, NWW_ERR_HIP, "cascade_select counted %lld open windows among %lld: nothing is sized by that", c, n);
    *n_open = (int)c;
    return NWW_OK;
}

// select over n scores on the device, and its count
int cas_select(nww_handle* v, const float* d_gate_probs, long long n, double thr, float* fill_logits, float* fill_probs, int* n_open, hipStream_t s) {
    hipError_t e = launch_cascade_select(d_gate_probs, n, thr, v->d_cas_idx, v->d_cas_counts, fill_logits, fill_probs, s);
    if (e != hipSuccess) return fail(v, NWW_ERR_HIP, "launch 'cascade_select' failed: %s", hipGetErrorString(e));
    return cas_read_count(v, n, n_open, s);
}

// One chunk of the verifier: the b windows at src + from[j] * row_stride gathered into its PCM staging, nww_forward_pcm's own path on
// them, and result j scattered to output to[j].  (v's workspace holds b clips of N samples: nww_ensure_ws is the caller's.)
int cas_verify_chunk(nww_handle* v, const int16_t* src, const int32_t* from, size_t row_stride, int N, int b, const int32_t* to, float* d_logits,
                     float* d_probs, hipStream_t s) {
    hipError_t e = launch_cascade_gather(src, from, row_stride, N, b, v->d_pcm, s);
    if (e != hipSuccess) return fail(v, NWW_ERR_HIP, "launch 'cascade_gather' failed: %s", hipGetErrorString(e));
    const int rc = nww_forward_pcm_on_dev(v, v->d_pcm, b, N, v->d_logits, v->d_probs, s);
    if (rc) return rc;
    e = launch_cascade_scatter(to, b, v->d_logits, v->d_probs, d_logits, d_probs, s);
    if (e != hipSuccess) return fail(v, NWW_ERR_HIP, "launch 'cascade_scatter' failed: %s", hipGetErrorString(e));
    return NWW_OK;
}

// The back half of every entry point but the pool's.  d_gate_probs [n] are on the device (enqueued on s); window i is the N samples at
// src + i * row_stride.  Fills the dense outputs, then runs the verifier on consecutive chunks of at most `chunk_max` open windows.
int cas_verify(nww_handle* v, const float* d_gate_probs, long long n, double thr, const int16_t* src, size_t row_stride, int N, int chunk_max,
               float* d_logits, float* d_probs, int32_t* n_open_out, hipStream_t s) {
    int n_open = 0;
    int rc = cas_select(v, d_gate_probs, n, thr, d_logits, d_probs, &n_open, s);
    if (rc) return rc;
    if (n_open_out) *n_open_out = n_open;
    if (n_open == 0) return NWW_OK;                    // no verifier launch at all
    const int chunk = std::min(chunk_max, n_open);
    rc = nww_ensure_ws(v, chunk, N);
    if (rc) return rc;
    for (int j0 = 0; j0 < n_open; j0 += chunk) {
        const int b = std::min(chunk, n_open - j0);
        const int32_t* idx = v->d_cas_idx + j0;
        rc = cas_verify_chunk(v, src, idx, row_stride, N, b, idx, d_logits, d_probs, s);
        if (rc) return rc;
    }
    return NWW_OK;
}

int cas_forward_pcm_dev(nww_handle* g, nww_handle* v, const int16_t* d_pcm, int B, int N, double thr, float* d_gate_probs, float* d_logits,
                        float* d_probs, int32_t* n_open_out, hipStream_t s) {
    int rc = cas_clip_fits(v, g, "gate", N);
    if (!rc) rc = cas_clip_fits(v, v, "verifier", N);
    if (!rc) rc = cas_state(v, B, d_gate_probs ? 0 : 1);
    if (rc) return rc;
    if (!d_gate_probs) d_gate_probs = v->d_cas_out;
    rc = nww_forward_pcm_on_dev(g, d_pcm, B, N, nullptr, d_gate_probs, s);
    if (rc) return cas_gate_fail(g, v, rc);
    return cas_verify(v, d_gate_probs, B, thr, d_pcm, (size_t)N, N, B, d_logits, d_probs, n_open_out, s);
}

int cas_forward_recording_dev(nww_handle* g, nww_handle* v, const int16_t* d_pcm, long long n_samples, int W, int hop, int max_batch, double thr,
                              float* d_gate_probs, float* d_logits, float* d_probs, int32_t* n_open_out, hipStream_t s) {
    int rc = cas_window_fits(v, g, "gate", W, hop);
    if (!rc) rc = cas_window_fits(v, v, "verifier", W, hop);
    if (rc) return rc;
    if (n_open_out) *n_open_out = 0;
    const long long nW = nww_rec_count(n_samples, W, hop);
    if (nW == 0) return NWW_OK;
    if (max_batch <= 0) max_batch = 4096;
    rc = cas_state(v, nW, d_gate_probs ? 0 : 1);
    if (rc) return rc;
    if (!d_gate_probs) d_gate_probs = v->d_cas_out;
    // the gate runs to the end first: one select and one readback for the whole recording, not one per pass
    rc = nww_rec_forward_on_dev(g, d_pcm, n_samples, W, hop, max_batch, nullptr, d_gate_probs, s);
    if (rc) return cas_gate_fail(g, v, rc);
    return cas_verify(v, d_gate_probs, nW, thr, d_pcm, (size_t)hop, W, max_batch, d_logits, d_probs, n_open_out, s);
}

int cas_stream_push_dev(nww_handle* g, nww_handle* v, const int16_t* d_chunk, double thr, float* d_gate_probs, float* d_logits, float* d_probs,
                        int32_t* n_open_out, hipStream_t s) {
    StreamState* st = g->stream;
    const int S = st->S, W = st->W;
    int rc = cas_clip_fits(v, v, "verifier", W);
    if (!rc) rc = cas_state(v, S, d_gate_probs ? 0 : 1);
    if (rc) return rc;
    if (!d_gate_probs) d_gate_probs = v->d_cas_out;
    rc = nww_stream_push_dev(g, d_chunk, nullptr, d_gate_probs, s);
    if (rc) return cas_gate_fail(g, v, rc);
    if (n_open_out) *n_open_out = 0;
    const RingState& ring = st->pool.all;           // the push ran, so the batch is aligned: every stream's state
    if (ring.filled < W) return nww_zero_scores(v, d_logits, d_probs, S, s);      // no window yet: 0 for both models, as nww_stream_push reports
    // every stream's window is the W samples at ring + pos of its row (double-written ring), after the push has moved pos
    return cas_verify(v, d_gate_probs, S, thr, st->d_ring + ring.pos, (size_t)2 * W, W, S, d_logits, d_probs, n_open_out, s);
}

// The checks of a pool call that need no device, in the order the header gives: nothing has touched a ring when one of them fails.
// *done: n == 0, the call is complete.
int cas_pool_check(nww_handle* g, nww_handle* v, const int32_t* idx, int32_t n, const void* chunk, int32_t* n_open_out, bool* done) {
    *done = false;
    int rc = cas_check(g, v);
    if (rc) return rc;
    rc = nww_pool_push_check(g, idx, n, chunk, done);
    if (rc) return cas_gate_fail(g, v, rc);
    if (*done) {
        if (n_open_out) *n_open_out = 0;
        return NWW_OK;
    }
    return cas_clip_fits(v, v, "verifier", g->stream->W);
}

// The listed streams of the gate's batch, each in its own state: the gate's pool call (either route) leaves its table on the device and
// the listed streams' probabilities [n] in d_gate_probs; the pool select walks the table and leaves the open streams' ring offsets and
// entries; the verifier scores their windows out of the gate's PCM rings as ONE batch.
int cas_pool_push_dev(nww_handle* g, nww_handle* v, const int32_t* idx, int n, const int16_t* d_chunk, double thr, float* d_gate_probs, float* d_logits,
                      float* d_probs, int32_t* n_open_out, hipStream_t s) {
    StreamState* st = g->stream;
    const int W = st->W;
    int rc = cas_state(v, n, d_gate_probs ? 0 : 1, 2);
    if (rc) return rc;
    if (!d_gate_probs) d_gate_probs = v->d_cas_out;
    const PoolEntry* tab = nullptr;
    int m = 0;
    rc = nww_pool_push_on_dev(g, idx, n, d_chunk, nullptr, d_gate_probs, s, &tab, &m);
    if (rc) return cas_gate_fail(g, v, rc);
    if (n_open_out) *n_open_out = 0;
    if (m == 0) return nww_zero_scores(v, d_logits, d_probs, n, s);      // no listed stream holds a window yet: 0 for both models, nothing to select
    int32_t* ring8 = v->d_cas_idx;
    int32_t* entry = v->d_cas_idx + n;
    hipError_t e = launch_cascade_pool_select(tab, d_gate_probs, n, thr, W, ring8, entry, v->d_cas_counts, d_logits, d_probs, s);
    if (e != hipSuccess) return fail(v, NWW_ERR_HIP, "launch 'cascade_pool_select' failed: %s", hipGetErrorString(e));
    int n_open = 0;
    rc = cas_read_count(v, m, &n_open, s);
    if (rc) return rc;
    if (n_open_out) *n_open_out = n_open;
    if (n_open == 0) return NWW_OK;                    // no verifier launch at all
    rc = nww_ensure_ws(v, n_open, W);
    if (rc) return rc;
    // an open stream's window is the W samples at 8 * ring8[j] of the gate's double-written rings, after the push has moved its pos
    return cas_verify_chunk(v, st->d_ring, ring8, 8, W, n_open, entry, d_logits, d_probs, s);
}

// the dense [3][n] outputs of a host-pointer call -> the caller's arrays, then the call's second synchronisation
int cas_copy_out(nww_handle* g, nww_handle* v, long long n, float* gate_probs, float* logits, float* probs, hipStream_t s) {
    const size_t nb = (size_t)n * sizeof(float);
    if (gate_probs) HIP_TRY(v, hipMemcpyAsync(gate_probs, v->d_cas_out, nb, hipMemcpyDeviceToHost, s));
    if (logits) HIP_TRY(v, hipMemcpyAsync(logits, v->d_cas_out + n, nb, hipMemcpyDeviceToHost, s));
    if (probs) HIP_TRY(v, hipMemcpyAsync(probs, v->d_cas_out + 2 * n, nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(v, hipStreamSynchronize(s));
    g->pin_in_busy = false;
    return NWW_OK;
}

// a host-pointer call that fails after it staged its input through the gate's pinned buffer: the copy runs on the CASCADE's stream, which
// the gate's own next call would not wait for (nww_h2d_small synchronises the stream it is given) - wait here, then report rc
int cas_settle(nww_handle* g, hipStream_t s, int rc) {
    (void)hipStreamSynchronize(s);
    g->pin_in_busy = false;
    return rc;
}

}  // namespace

void nww_cascade_free(nww_handle* h) {
    for (void* p : {(void*)h->d_cas_idx, (void*)h->d_cas_out, (void*)h->d_cas_counts})
        if (p) (void)hipFree(p);
    if (h->pin_cas_count) (void)hipHostFree(h->pin_cas_count);
    h->d_cas_idx = nullptr; h->d_cas_out = nullptr; h->d_cas_counts = nullptr; h->pin_cas_count = nullptr;
    h->cas_idx_bytes = h->cas_out_bytes = 0;
}

extern "C" int nww_cascade_select(nww_handle* v, const float* probs, int32_t n, double thr, int32_t* idx_out, int32_t* n_open_out) {
    int rc = nww_check_run(v, n);
    if (rc) return rc;
    if (!probs || !idx_out) return fail(v, NWW_ERR_INVALID, "null pointer");
    HIP_TRY(v, hipSetDevice(v->cfg.device));
    hipStream_t s = v->own_stream;
    rc = cas_state(v, n, 1);
    if (rc) return rc;
    HIP_TRY(v, hipMemcpyAsync(v->d_cas_out, probs, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    int n_open = 0;
    rc = cas_select(v, v->d_cas_out, n, thr, nullptr, nullptr, &n_open, s);
    if (rc) return rc;
    if (n_open_out) *n_open_out = n_open;
    if (n_open > 0) {
        HIP_TRY(v, hipMemcpyAsync(idx_out, v->d_cas_idx, (size_t)n_open * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(v, hipStreamSynchronize(s));
    }
    return NWW_OK;
}

extern "C" int nww_cascade_forward_pcm_dev(nww_handle* g, nww_handle* v, const int16_t* d_pcm, int32_t B, int32_t N, double thr, float* d_gate_probs,
                                           float* d_logits, float* d_probs, int32_t* n_open_out, void* stream) {
    int rc = cas_check(g, v);
    if (!rc) rc = nww_check_run(v, B);
    if (rc) return rc;
    if (!d_pcm) return fail(v, NWW_ERR_INVALID, "null device pointer");
    HIP_TRY(v, hipSetDevice(v->cfg.device));
    return cas_forward_pcm_dev(g, v, d_pcm, B, N, thr, d_gate_probs, d_logits, d_probs, n_open_out, stream ? (hipStream_t)stream : v->own_stream);
}

extern "C" int nww_cascade_forward_pcm(nww_handle* g, nww_handle* v, const int16_t* pcm, int32_t B, int32_t N, double thr, float* gate_probs,
                                       float* logits, float* probs, int32_t* n_open_out) {
    int rc = cas_check(g, v);
    if (!rc) rc = nww_check_run(v, B);
    if (rc) return rc;
    if (!pcm) return fail(v, NWW_ERR_INVALID, "Input audio must be a non-null int16 array");
    HIP_TRY(v, hipSetDevice(v->cfg.device));
    hipStream_t s = v->own_stream;
    rc = cas_clip_fits(v, g, "gate", N);
    if (!rc) rc = cas_clip_fits(v, v, "verifier", N);
    if (!rc) rc = cas_state(v, B, 3);
    if (rc) return rc;
    // the clips go up once, into the gate's PCM staging: the gate reads them there and the gather takes the survivors from there
    rc = nww_ensure_ws(g, B, N);
    if (!rc) rc = nww_h2d_small(g, g->d_pcm, pcm, (size_t)B * N * sizeof(int16_t), s);
    if (rc) return cas_gate_fail(g, v, rc);
    float* out = v->d_cas_out;
    rc = cas_forward_pcm_dev(g, v, g->d_pcm, B, N, thr, out, out + B, out + 2 * (size_t)B, n_open_out, s);
    if (rc) return cas_settle(g, s, rc);
    return cas_copy_out(g, v, B, gate_probs, logits, probs, s);
}

extern "C" int nww_cascade_forward_recording_dev(nww_handle* g, nww_handle* v, const int16_t* d_pcm, int32_t n_samples, int32_t window, int32_t hop,
                                                 int32_t max_batch, double thr, float* d_gate_probs, float* d_logits, float* d_probs,
                                                 int32_t* n_open_out, void* stream) {
    int rc = cas_check(g, v);
    if (rc) return rc;
    if (!d_pcm || n_samples < 0) return fail(v, NWW_ERR_INVALID, "null device pointer or negative length");
    HIP_TRY(v, hipSetDevice(v->cfg.device));
    return cas_forward_recording_dev(g, v, d_pcm, n_samples, window, hop, max_batch, thr, d_gate_probs, d_logits, d_probs, n_open_out,
                                     stream ? (hipStream_t)stream : v->own_stream);
}

extern "C" int nww_cascade_forward_recording(nww_handle* g, nww_handle* v, const int16_t* pcm, int32_t n_samples, int32_t window, int32_t hop,
                                             int32_t max_batch, double thr, float* gate_probs, float* logits, float* probs, int32_t* n_windows_out,
                                             int32_t* n_open_out) {
    int rc = cas_check(g, v);
    if (rc) return rc;
    if (!pcm || n_samples < 0) return fail(v, NWW_ERR_INVALID, "Input audio must be a non-null int16 array");
    rc = cas_window_fits(v, g, "gate", window, hop);
    if (!rc) rc = cas_window_fits(v, v, "verifier", window, hop);
    if (rc) return rc;
    const long long nW = nww_rec_count(n_samples, window, hop);
    if (n_windows_out) *n_windows_out = (int32_t)nW;
    if (n_open_out) *n_open_out = 0;
    if (nW == 0) return NWW_OK;
    HIP_TRY(v, hipSetDevice(v->cfg.device));
    hipStream_t s = v->own_stream;
    // the recording goes up once, in pieces of 32 MiB, as in nww_forward_recording; the tail no window reads stays behind
    const size_t used = (size_t)((nW - 1) * hop + window), piece = (size_t)16 << 20;
    rc = nww_grow(v, reinterpret_cast<void**>(&v->d_rec_pcm), &v->rec_pcm_bytes, used * sizeof(int16_t));
    if (!rc) rc = cas_state(v, nW, 3);
    if (rc) return rc;
    for (size_t o = 0; o < used; o += piece)
        HIP_TRY(v, hipMemcpyAsync(v->d_rec_pcm + o, pcm + o, std::min(piece, used - o) * sizeof(int16_t), hipMemcpyHostToDevice, s));
    float* out = v->d_cas_out;
    rc = cas_forward_recording_dev(g, v, v->d_rec_pcm, (long long)used, window, hop, max_batch, thr, out, out + nW, out + 2 * nW, n_open_out, s);
    if (rc) return rc;
    return cas_copy_out(g, v, nW, gate_probs, logits, probs, s);
}

extern "C" int nww_cascade_stream_push_dev(nww_handle* g, nww_handle* v, const int16_t* d_chunk, double thr, float* d_gate_probs, float* d_logits,
                                           float* d_probs, int32_t* n_open_out, void* stream) {
    int rc = cas_check(g, v);
    if (rc) return rc;
    if (!g->stream) return fail(v, NWW_ERR_STATE, "gate: no open stream batch (nww_stream_open)");
    if (!d_chunk) return fail(v, NWW_ERR_INVALID, "null chunk pointer");
    HIP_TRY(v, hipSetDevice(v->cfg.device));
    return cas_stream_push_dev(g, v, d_chunk, thr, d_gate_probs, d_logits, d_probs, n_open_out, stream ? (hipStream_t)stream : v->own_stream);
}

extern "C" int nww_cascade_stream_push(nww_handle* g, nww_handle* v, const int16_t* chunk, double thr, float* gate_probs, float* logits,
                                       float* probs, int32_t* n_open_out) {
    int rc = cas_check(g, v);
    if (rc) return rc;
    if (!g->stream) return fail(v, NWW_ERR_STATE, "gate: no open stream batch (nww_stream_open)");
    if (!chunk) return fail(v, NWW_ERR_INVALID, "Input audio must be a non-null int16 array");
    HIP_TRY(v, hipSetDevice(v->cfg.device));
    hipStream_t s = v->own_stream;
    const int S = g->stream->S;
    rc = cas_state(v, S, 3);
    if (rc) return rc;
    rc = nww_h2d_small(g, g->stream->d_chunk, chunk, (size_t)S * g->stream->hop * sizeof(int16_t), s);
    if (rc) return cas_gate_fail(g, v, rc);
    float* out = v->d_cas_out;
    rc = cas_stream_push_dev(g, v, g->stream->d_chunk, thr, out, out + S, out + 2 * S, n_open_out, s);
    if (rc) return cas_settle(g, s, rc);
    return cas_copy_out(g, v, S, gate_probs, logits, probs, s);
}

extern "C" int nww_cascade_stream_push_some_dev(nww_handle* g, nww_handle* v, const int32_t* idx, int32_t n, const int16_t* d_chunk, double thr,
                                                float* d_gate_probs, float* d_logits, float* d_probs, int32_t* n_open_out, void* stream) {
    bool done;
    const int rc = cas_pool_check(g, v, idx, n, d_chunk, n_open_out, &done);
    if (rc || done) return rc;
    HIP_TRY(v, hipSetDevice(v->cfg.device));
    return cas_pool_push_dev(g, v, idx, n, d_chunk, thr, d_gate_probs, d_logits, d_probs, n_open_out, stream ? (hipStream_t)stream : v->own_stream);
}

extern "C" int nww_cascade_stream_push_some(nww_handle* g, nww_handle* v, const int32_t* idx, int32_t n, const int16_t* chunk, double thr,
                                            float* gate_probs, float* logits, float* probs, int32_t* n_open_out) {
    bool done;
    int rc = cas_pool_check(g, v, idx, n, chunk, n_open_out, &done);
    if (rc || done) return rc;
    HIP_TRY(v, hipSetDevice(v->cfg.device));
    hipStream_t s = v->own_stream;
    rc = cas_state(v, n, 3, 2);
    if (rc) return rc;
    rc = nww_h2d_small(g, g->stream->d_chunk, chunk, (size_t)n * g->stream->hop * sizeof(int16_t), s);
    if (rc) return cas_gate_fail(g, v, rc);
    float* out = v->d_cas_out;
    rc = cas_pool_push_dev(g, v, idx, n, g->stream->d_chunk, thr, out, out + n, out + 2 * n, n_open_out, s);
    if (rc) return cas_settle(g, s, rc);
    return cas_copy_out(g, v, n, gate_probs, logits, probs, s);
}

extern "C" int nww_cascade_stream_reset_some(nww_handle* g, nww_handle* v, const int32_t* idx, int32_t n) {
    int rc = cas_check(g, v);
    if (rc) return rc;
    rc = nww_stream_reset_some(g, idx, n);
    return rc ? cas_gate_fail(g, v, rc) : NWW_OK;
}
