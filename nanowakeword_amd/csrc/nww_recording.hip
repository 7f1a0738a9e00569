// nww_recording.hip - recording scoring: every window pcm[i * hop, i * hop + window) of ONE recording in a call (nww_recording_*,
// nww_forward_recording*): the offline counterpart of nww_stream_*.  The recording is read where it lies - nothing is cut into
// windows - on one of two routes per (window, hop):
//   strided  every pass of B windows is nww_forward_pcm_on_dev with row_stride = hop: all T frames of every window are computed
//   shared   a hop of k = hop / hop_length frames makes interior frame t of window w the frame t - k of window w + 1, bit for bit
//            (what a stream's log-mel ring relies on from hop to hop; HopPlan, stream_plan.h). Per pass: (1) the pass's span of (B - 1) hop + window
//            samples goes through the batch frontend as ONE clip, whose frames-major output is the pool - row w k + t is interior frame
//            t of window w; (2) the el + er frames of every window that touch its own reflect padding are computed by the frame-subset
//            instances straight into the dense head input; (3) rec_assemble_kernel copies every window's interior run out of the pool.
//            k + el + er frames per window instead of T.  Launch-side code only: no frontend instance is added or changed.
//            The raw-PCM heads take it with the rows of their learned frontend's last stage for frames (nww_plan_hop_raw, raw_plan.h):
//            the pool is launch_raw_x3 on the span, the edge rows - those that see the window's own zero padding - the row-subset
//            instance launch_raw_x3_sub, the assembly the same kernel on rows of in_cols floats.
#include "nww_internal.h"
#include "rec_windows.h"

namespace {

using RecPlan = HopPlan;

// the rules of nww_stream_open; the route is shared exactly where a stream would keep a log-mel ring (NWW_STREAM_INC level 1)
int rec_plan(nww_handle* h, int W, int hop, RecPlan& p) {
    const int rc = nww_check_run(h, 1);
    return rc ? rc : nww_window_plan(h, W, hop, nww_knobs().rec_shared ? 1 : 0, p);
}

// One pass on the shared route: B windows whose first sample is d_pcm[0].
int rec_pass_shared(nww_handle* h, const RecPlan& p, const int16_t* d_pcm, int B, int W, int hop, float* d_logits, float* d_probs, hipStream_t s,
                    const BankRun* bank) {
    const nww_config& c = h->cfg;
    const int span = (B - 1) * hop + W;
    nww_prof_begin(h);
    nww_prof_mark(h, s, 0);
    // (1) the pool: the span as one clip.  Its own edge frames (rows < el and the last er) are no window's interior frames.
    int rc = nww_frontend_on_dev(h, d_pcm, 1, span, h->d_rec_pool, nullptr, 1, s, nullptr);
    if (rc) return rc;
    // (2) every window's edge frames, with its own reflect padding, at their place in the dense tensor
    if (p.el + p.er > 0) {
        Fe2Sub sub;
        nww_hop_ranges(p.T, 0, p.el, p.er, sub);
        rc = nww_frontend_on_dev(h, d_pcm, B, W, h->d_logmel, nullptr, 1, s, nullptr, (size_t)hop, &sub);
        if (rc) return rc;
    }
    // (3) the interior runs
    hipError_t e = launch_rec_assemble(h->d_rec_pool, h->d_logmel, B, p.T, nww_row_floats(c), p.k, p.el, p.er, s);
    if (e != hipSuccess) return fail(h, NWW_ERR_HIP, "launch 'rec_assemble' failed: %s", hipGetErrorString(e));
    RunOpts o;
    o.x_frames_major = c.mel_major_features != 0;
    o.bank = bank;
    return nww_run_heads(h, h->d_logmel, B, d_logits, d_probs, s, o);
}

}  // namespace

long long nww_rec_count(long long n_samples, int W, int hop) { return n_samples < W ? 0 : 1 + (n_samples - W) / hop; }

int nww_rec_forward_on_dev(nww_handle* h, const int16_t* d_pcm, long long n_samples, int W, int hop, int max_batch, float* d_logits, float* d_probs,
                           hipStream_t s, const BankRun* bank) {
    RecPlan p;
    int rc = rec_plan(h, W, hop, p);
    if (rc) return rc;
    const long long nW = nww_rec_count(n_samples, W, hop);
    if (nW == 0) return NWW_OK;
    if (max_batch <= 0) max_batch = 4096;
    const int Bmax = (int)std::min<long long>(max_batch, nW);
    // the pool's frames as one clip: the span has to stay inside the frontend's 32-bit sample offsets, and the frame law has to give
    // the span every row the windows read (it does whenever hop is a multiple of the frame hop; checked, not assumed)
    const long long span = (long long)(Bmax - 1) * hop + W, rows = (long long)(Bmax - 1) * p.k + p.T;
    if (p.shared && (span >= (1ll << 30) || (nww_raw_head(h->cfg) ? nww_pcm_rows(h, (int)span) != rows : nww_pcm_rows(h, (int)span) < rows))) p.shared = false;
    rc = nww_ensure_ws(h, Bmax, W);
    if (rc) return rc;
    if (p.shared) {
        const size_t floats = (size_t)nww_pcm_rows(h, (int)span) * nww_row_floats(h->cfg);
        rc = nww_grow(h, reinterpret_cast<void**>(&h->d_rec_pool), &h->rec_pool_bytes, floats * sizeof(float));
        if (rc) return rc;
    }
    for (long long first = 0; first < nW; first += Bmax) {
        const int B = (int)std::min<long long>(Bmax, nW - first);
        const int16_t* x = d_pcm + first * hop;
        float* lg = d_logits ? d_logits + first : nullptr;
        float* pr = d_probs ? d_probs + first : nullptr;
        BankRun pass;                                            // a bank's followers write the same pass of their own rows
        RunOpts o;
        if (bank) { pass = *bank; pass.offset = (size_t)first; o.bank = &pass; }
        rc = p.shared ? rec_pass_shared(h, p, x, B, W, hop, lg, pr, s, o.bank) : nww_forward_pcm_on_dev(h, x, B, W, lg, pr, s, (size_t)hop, o);
        if (rc) return rc;
    }
    return NWW_OK;
}

void nww_recording_free(nww_handle* h) {
    for (void* p : {(void*)h->d_rec_pool, (void*)h->d_rec_pcm, (void*)h->d_rec_out})
        if (p) (void)hipFree(p);
    h->d_rec_pool = nullptr; h->d_rec_pcm = nullptr; h->d_rec_out = nullptr;
    h->rec_pool_bytes = h->rec_pcm_bytes = h->rec_out_bytes = 0;
}

extern "C" int nww_recording_windows(nww_handle* h, int32_t n_samples, int32_t window, int32_t hop) {
    RecPlan p;
    const int rc = rec_plan(h, window, hop, p);
    if (rc) return -rc;
    if (n_samples < 0) return -fail(h, NWW_ERR_INVALID, "a recording cannot have %d samples", n_samples);
    const long long n = nww_rec_count(n_samples, window, hop);
    return (int)n;
}

extern "C" int nww_recording_route(nww_handle* h, int32_t window, int32_t hop) {
    RecPlan p;
    const int rc = rec_plan(h, window, hop, p);
    return rc ? -rc : (p.shared ? 1 : 0);
}

// test instrument: the pool and the dense head input hold `value` everywhere, so that a pass which left a row unwritten shows
extern "C" int nww_recording_poison(nww_handle* h, float value) {
    const int rc = nww_check_run(h, 1);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = h->own_stream;
    HIP_TRY(h, launch_rec_fill(h->d_rec_pool, h->rec_pool_bytes / sizeof(float), value, s));
    const int T = h->cap_N > 0 ? nww_pcm_rows(h, h->cap_N) : 0;
    if (T > 0 && h->d_logmel) HIP_TRY(h, launch_rec_fill(h->d_logmel, (size_t)h->cap_B * T * nww_row_floats(h->cfg), value, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return NWW_OK;
}

extern "C" int nww_forward_recording_dev(nww_handle* h, const int16_t* d_pcm, int32_t n_samples, int32_t window, int32_t hop, int32_t max_batch,
                                         float* d_logits, float* d_probs, void* stream) {
    int rc = nww_check_run(h, 1);
    if (rc) return rc;
    if (!d_pcm || n_samples < 0) return fail(h, NWW_ERR_INVALID, "null device pointer or negative length");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return nww_rec_forward_on_dev(h, d_pcm, n_samples, window, hop, max_batch, d_logits, d_probs, stream ? (hipStream_t)stream : h->own_stream);
}

extern "C" int nww_forward_recording(nww_handle* h, const int16_t* pcm, int32_t n_samples, int32_t window, int32_t hop, int32_t max_batch,
                                     float* logits, float* probs, int32_t* n_windows_out) {
    int rc = nww_check_run(h, 1);
    if (rc) return rc;
    if (!pcm || n_samples < 0) return fail(h, NWW_ERR_INVALID, "Input audio must be a non-null int16 array");
    RecPlan p;
    rc = rec_plan(h, window, hop, p);
    if (rc) return rc;
    const long long nW = nww_rec_count(n_samples, window, hop);
    if (n_windows_out) *n_windows_out = (int32_t)nW;
    if (nW == 0) return NWW_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = h->own_stream;
    // the recording goes up once, 2 bytes per sample, in pieces of 32 MiB (16 Mi samples) - never as windows; the tail no window reads stays behind
    const size_t used = (size_t)((nW - 1) * hop + window), piece = (size_t)16 << 20;
    rc = nww_grow(h, reinterpret_cast<void**>(&h->d_rec_pcm), &h->rec_pcm_bytes, used * sizeof(int16_t));
    if (rc) return rc;
    rc = nww_grow(h, reinterpret_cast<void**>(&h->d_rec_out), &h->rec_out_bytes, (size_t)2 * nW * sizeof(float));
    if (rc) return rc;
    for (size_t o = 0; o < used; o += piece)
        HIP_TRY(h, hipMemcpyAsync(h->d_rec_pcm + o, pcm + o, std::min(piece, used - o) * sizeof(int16_t), hipMemcpyHostToDevice, s));
    float *dl = h->d_rec_out, *dp = probs ? h->d_rec_out + nW : nullptr;
    rc = nww_rec_forward_on_dev(h, h->d_rec_pcm, (long long)used, window, hop, max_batch, dl, dp, s);
    if (rc) return rc;
    if (logits) HIP_TRY(h, hipMemcpyAsync(logits, dl, (size_t)nW * sizeof(float), hipMemcpyDeviceToHost, s));
    if (probs) HIP_TRY(h, hipMemcpyAsync(probs, dp, (size_t)nW * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return NWW_OK;
}
