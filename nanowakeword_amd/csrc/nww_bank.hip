// nww_bank.hip - model banks (nww_bank_*): K finalized handles whose mel frontends are identical score the same audio on ONE frontend
// pass.  members[0], the leader, owns everything that is shared - PCM staging, the frontend's launches, the dense frames-major head
// input, the stream batch with its rings, the recording pool; members[1 .. k), the followers, run their head plans on the leader's
// head input (nww_run_heads, nww_api.hip) and hold no PCM.  A bank is not an object: like a cascade it is the list of handles passed
// with each call, and its rules (bank.h, host-only) are checked before anything is launched or any ring is touched.  Launch-side code
// only: no frontend or head kernel is added or changed, and the leader's calls are its own single-handle paths (nww_forward_pcm_on_dev,
// nww_rec_forward_on_dev, nww_pool_push_on_dev) with a BankRun riding along.  Outputs are member-major [k][n]; errors go to
// nww_last_error(members[0]); the dense [2][k][n] outputs of the host-pointer variants live on the leader's handle.
#include "nww_internal.h"
#include "bank.h"

namespace {

// the rules that need no window (bank.h), on what they read of each handle
int bank_members(nww_handle* const* members, int k) {
    std::string text;
    if (!members || k < 1) {
        const int rc = bank_members_check(nullptr, k, text);
        return fail(nullptr, rc, "%s", text.c_str());
    }
    std::vector<BankMember> m((size_t)k);
    for (int j = 0; j < k; ++j) {
        const nww_handle* h = members[j];
        if (!h) continue;
        BankMember& b = m[(size_t)j];
        b.handle = h; b.finalized = h->finalized; b.device = h->cfg.device; b.raw_head = nww_raw_head(h->cfg);
        b.frames_major = !h->cfg.mel_major_features || h->e2e_transposed;
        b.frontend.fe = h->fe;
        b.frontend.window = h->fe_window.data(); b.frontend.n_window = h->fe_window.size();
        b.frontend.mel_fb = h->fe_mel_fb.data(); b.frontend.n_mel_fb = h->fe_mel_fb.size();
    }
    const int rc = bank_members_check(m.data(), k, text);
    return rc ? fail(members[0], rc, "%s", text.c_str()) : NWW_OK;
}

// a clip or window of N samples against every member's own (in_rows, in_cols)
int bank_shape(nww_handle* const* members, int k, int N) {
    nww_handle* L = members[0];
    for (int j = 0; j < k; ++j) {
        const nww_handle* h = members[j];
        const ClipRows cr = nww_clip_rows(h, N);
        if (cr.T <= 0) return fail(L, NWW_ERR_INVALID, "member %d: clip of %d samples is too short for n_fft=%d (center=%d)", j, N, h->fe.n_fft, h->fe.center);
        if (!cr.fits)
            return fail(L, NWW_ERR_SHAPE, "member %d: frontend yields (%d,%d) features for %d samples but the head was built for input_shape=(%d,%d)", j,
                        cr.rows, cr.cols, N, h->cfg.in_rows, h->cfg.in_cols);
    }
    return NWW_OK;
}

int bank_check(nww_handle* const* members, int k, int window) {
    const int rc = bank_members(members, k);
    return rc ? rc : bank_shape(members, k, window);
}

// the followers hold no PCM: their workspaces are sized as nww_forward_features_dev sizes them, before the leader launches anything
int bank_reserve(nww_handle* const* members, int k, int B) {
    for (int j = 1; j < k; ++j) {
        nww_handle* f = members[j];
        const int rc = nww_ensure_ws(f, B, 0);
        if (rc) return fail(members[0], rc, "member %d: %s", j, f->err.c_str());
    }
    return NWW_OK;
}

BankRun bank_run(nww_handle* const* members, int k, float* d_logits, float* d_probs, size_t n, bool own) {
    BankRun b;
    b.members = members; b.k = k; b.d_logits = d_logits; b.d_probs = d_probs; b.stride = n; b.own = own; b.probs = d_probs != nullptr;
    return b;
}

int bank_forward_pcm_dev(nww_handle* const* members, int k, const int16_t* d_pcm, int B, int N, float* d_logits, float* d_probs, hipStream_t s) {
    const int rc = bank_reserve(members, k, B);
    if (rc) return rc;
    const BankRun b = bank_run(members, k, d_logits, d_probs, (size_t)B, false);
    RunOpts o;
    o.bank = &b;
    return nww_forward_pcm_on_dev(members[0], d_pcm, B, N, d_logits, d_probs, s, 0, o);
}

int bank_forward_recording_dev(nww_handle* const* members, int k, const int16_t* d_pcm, long long n_samples, int W, int hop, int max_batch, long long nW,
                               float* d_logits, float* d_probs, hipStream_t s) {
    const int Bmax = (int)std::min<long long>(max_batch <= 0 ? 4096 : max_batch, nW);
    const int rc = bank_reserve(members, k, Bmax);
    if (rc) return rc;
    const BankRun b = bank_run(members, k, d_logits, d_probs, (size_t)nW, false);
    return nww_rec_forward_on_dev(members[0], d_pcm, n_samples, W, hop, max_batch, d_logits, d_probs, s, &b);
}

// the checks of a stream call, none of which touches a ring; *done: n == 0, the call is complete
int bank_pool_check(nww_handle* const* members, int k, const int32_t* idx, int32_t n, const void* chunk, bool* done) {
    *done = false;
    int rc = bank_members(members, k);
    if (rc) return rc;
    nww_handle* L = members[0];
    if (!L->stream) return fail(L, NWW_ERR_STATE, "member 0: no open stream batch (nww_stream_open): the leader holds a bank's streams");
    rc = bank_shape(members, k, L->stream->W);
    if (rc) return rc;
    return nww_pool_push_check(L, idx, n, chunk, done);
}

int bank_pool_push_dev(nww_handle* const* members, int k, const int32_t* idx, int n, const int16_t* d_chunk, float* d_logits, float* d_probs, hipStream_t s) {
    nww_handle* L = members[0];
    const int rc = bank_reserve(members, k, L->stream->S);
    if (rc) return rc;
    const BankRun b = bank_run(members, k, d_logits, d_probs, (size_t)n, true);
    return nww_pool_push_on_dev(L, idx, n, d_chunk, d_logits, d_probs, s, nullptr, nullptr, &b);
}

// the dense [2][k][n] outputs of a host-pointer call
int bank_out(nww_handle* L, int k, long long n) {
    return nww_grow(L, reinterpret_cast<void**>(&L->d_bank_out), &L->bank_out_bytes, (size_t)2 * k * (size_t)n * sizeof(float));
}

// ... -> the caller's arrays, then the call's synchronisation
int bank_copy_out(nww_handle* L, int k, long long n, float* logits, float* probs, hipStream_t s) {
    const size_t kn = (size_t)k * (size_t)n;
    if (logits) HIP_TRY(L, hipMemcpyAsync(logits, L->d_bank_out, kn * sizeof(float), hipMemcpyDeviceToHost, s));
    if (probs) HIP_TRY(L, hipMemcpyAsync(probs, L->d_bank_out + kn, kn * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(L, hipStreamSynchronize(s));
    L->pin_in_busy = false;
    return NWW_OK;
}

// a host-pointer call that fails after it staged its input through the leader's pinned buffer: wait for that copy, then report rc
int bank_settle(nww_handle* L, hipStream_t s, int rc) {
    (void)hipStreamSynchronize(s);
    L->pin_in_busy = false;
    return rc;
}

}  // namespace

void nww_bank_free(nww_handle* h) {
    if (h->d_bank_out) (void)hipFree(h->d_bank_out);
    h->d_bank_out = nullptr; h->bank_out_bytes = 0;
}

extern "C" int nww_bank_check(nww_handle* const* members, int32_t k, int32_t window) { return bank_check(members, k, window); }

extern "C" int nww_bank_forward_pcm_dev(nww_handle* const* members, int32_t k, const int16_t* d_pcm, int32_t B, int32_t N, float* d_logits, float* d_probs,
                                        void* stream) {
    int rc = bank_members(members, k);
    if (rc) return rc;
    nww_handle* L = members[0];
    if (k == 1) return nww_forward_pcm_dev(L, d_pcm, B, N, d_logits, d_probs, stream);
    rc = nww_check_run(L, B);
    if (!rc) rc = bank_shape(members, k, N);
    if (rc) return rc;
    if (!d_pcm) return fail(L, NWW_ERR_INVALID, "null device pointer");
    HIP_TRY(L, hipSetDevice(L->cfg.device));
    return bank_forward_pcm_dev(members, k, d_pcm, B, N, d_logits, d_probs, stream ? (hipStream_t)stream : L->own_stream);
}

extern "C" int nww_bank_forward_pcm(nww_handle* const* members, int32_t k, const int16_t* pcm, int32_t B, int32_t N, float* logits, float* probs) {
    int rc = bank_members(members, k);
    if (rc) return rc;
    nww_handle* L = members[0];
    if (k == 1) return nww_forward_pcm(L, pcm, B, N, logits, probs);
    rc = nww_check_run(L, B);
    if (!rc) rc = bank_shape(members, k, N);
    if (rc) return rc;
    if (!pcm) return fail(L, NWW_ERR_INVALID, "Input audio must be a non-null int16 array");
    HIP_TRY(L, hipSetDevice(L->cfg.device));
    hipStream_t s = L->own_stream;
    // the clips go up once, into the leader's PCM staging
    rc = nww_ensure_ws(L, B, N);
    if (!rc) rc = bank_out(L, k, B);
    if (!rc) rc = bank_reserve(members, k, B);
    if (!rc) rc = nww_h2d_small(L, L->d_pcm, pcm, (size_t)B * N * sizeof(int16_t), s);
    if (rc) return rc;
    float* out = L->d_bank_out;
    rc = bank_forward_pcm_dev(members, k, L->d_pcm, B, N, out, probs ? out + (size_t)k * B : nullptr, s);
    if (rc) return bank_settle(L, s, rc);
    return bank_copy_out(L, k, B, logits, probs, s);
}

extern "C" int nww_bank_forward_recording_dev(nww_handle* const* members, int32_t k, const int16_t* d_pcm, int32_t n_samples, int32_t window, int32_t hop,
                                              int32_t max_batch, float* d_logits, float* d_probs, void* stream) {
    int rc = bank_members(members, k);
    if (rc) return rc;
    nww_handle* L = members[0];
    if (k == 1) return nww_forward_recording_dev(L, d_pcm, n_samples, window, hop, max_batch, d_logits, d_probs, stream);
    if (!d_pcm || n_samples < 0) return fail(L, NWW_ERR_INVALID, "null device pointer or negative length");
    const int nW = nww_recording_windows(L, n_samples, window, hop);      // the leader's window / hop rule and its own shape
    if (nW < 0) return -nW;
    rc = bank_shape(members, k, window);
    if (rc || nW == 0) return rc;
    HIP_TRY(L, hipSetDevice(L->cfg.device));
    return bank_forward_recording_dev(members, k, d_pcm, n_samples, window, hop, max_batch, nW, d_logits, d_probs, stream ? (hipStream_t)stream : L->own_stream);
}

extern "C" int nww_bank_forward_recording(nww_handle* const* members, int32_t k, const int16_t* pcm, int32_t n_samples, int32_t window, int32_t hop,
                                          int32_t max_batch, float* logits, float* probs, int32_t* n_windows_out) {
    int rc = bank_members(members, k);
    if (rc) return rc;
    nww_handle* L = members[0];
    if (k == 1) return nww_forward_recording(L, pcm, n_samples, window, hop, max_batch, logits, probs, n_windows_out);
    if (!pcm || n_samples < 0) return fail(L, NWW_ERR_INVALID, "Input audio must be a non-null int16 array");
    const int nW = nww_recording_windows(L, n_samples, window, hop);
    if (nW < 0) return -nW;
    rc = bank_shape(members, k, window);
    if (rc) return rc;
    if (n_windows_out) *n_windows_out = nW;
    if (nW == 0) return NWW_OK;
    HIP_TRY(L, hipSetDevice(L->cfg.device));
    hipStream_t s = L->own_stream;
    // the recording goes up once, in pieces of 32 MiB, as in nww_forward_recording; the tail no window reads stays behind
    const size_t used = (size_t)(nW - 1) * hop + window, piece = (size_t)16 << 20;
    rc = nww_grow(L, reinterpret_cast<void**>(&L->d_rec_pcm), &L->rec_pcm_bytes, used * sizeof(int16_t));
    if (!rc) rc = bank_out(L, k, nW);
    if (rc) return rc;
    for (size_t o = 0; o < used; o += piece)
        HIP_TRY(L, hipMemcpyAsync(L->d_rec_pcm + o, pcm + o, std::min(piece, used - o) * sizeof(int16_t), hipMemcpyHostToDevice, s));
    float* out = L->d_bank_out;
    rc = bank_forward_recording_dev(members, k, L->d_rec_pcm, (long long)used, window, hop, max_batch, nW, out, probs ? out + (size_t)k * nW : nullptr, s);
    if (rc) return bank_settle(L, s, rc);
    return bank_copy_out(L, k, nW, logits, probs, s);
}

extern "C" int nww_bank_stream_push_some_dev(nww_handle* const* members, int32_t k, const int32_t* idx, int32_t n, const int16_t* d_chunk, float* d_logits,
                                             float* d_probs, void* stream) {
    bool done;
    const int rc = bank_pool_check(members, k, idx, n, d_chunk, &done);
    if (rc || done) return rc;
    nww_handle* L = members[0];
    if (k == 1) return nww_stream_push_some_dev(L, idx, n, d_chunk, d_logits, d_probs, stream);
    HIP_TRY(L, hipSetDevice(L->cfg.device));
    return bank_pool_push_dev(members, k, idx, n, d_chunk, d_logits, d_probs, stream ? (hipStream_t)stream : L->own_stream);
}

extern "C" int nww_bank_stream_push_some(nww_handle* const* members, int32_t k, const int32_t* idx, int32_t n, const int16_t* chunk, float* logits,
                                         float* probs) {
    bool done;
    int rc = bank_pool_check(members, k, idx, n, chunk, &done);
    if (rc || done) return rc;
    nww_handle* L = members[0];
    if (k == 1) return nww_stream_push_some(L, idx, n, chunk, logits, probs);
    HIP_TRY(L, hipSetDevice(L->cfg.device));
    hipStream_t s = L->own_stream;
    StreamState* st = L->stream;
    rc = bank_out(L, k, n);
    if (!rc) rc = bank_reserve(members, k, st->S);
    if (!rc) rc = nww_h2d_small(L, st->d_chunk, chunk, (size_t)n * st->hop * sizeof(int16_t), s);
    if (rc) return rc;
    float* out = L->d_bank_out;
    rc = bank_pool_push_dev(members, k, idx, n, st->d_chunk, logits ? out : nullptr, probs ? out + (size_t)k * n : nullptr, s);
    if (rc) return bank_settle(L, s, rc);
    return bank_copy_out(L, k, n, logits, probs, s);
}
