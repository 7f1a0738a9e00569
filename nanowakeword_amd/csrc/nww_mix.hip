// nww_mix.hip - clips mixed on the device (nww_mix_*, include/nww.h): the host validates a call's items (mix_plan.h),
// the table goes up through the next of MIX_TAB_SLOTS = POOL_TAB_SLOTS slots of the handle's own pinned and device buffers - a slot is
// rewritten once the event behind its previous call has passed, as the pool tables' are (nww_stream.hip) - and mix.hip gathers, measures
// and mixes.  The forward and frontend forms mix into the handle's PCM staging and run the existing paths on it.
// nww_rir_* / nww_mix_rir_* (DESIGN.md 4.8h): the same calls with a second table naming a room impulse response per clip - it rides in
// the same slot - and rir.hip in mix.hip's place; response spectra are prepared once by nww_rir_prepare_dev (rir_plan.h).
// nww_pitch_set_ratios / nww_mix_aug_* (DESIGN.md 4.8i): a third table naming a pitch ratio per clip, in the same slot again; pitch.hip
// shifts the clips that name one (pitch_plan.h) ahead of the response and the tail.
#include "nww_internal.h"
#include "mix.h"
#include "mix_plan.h"
#include "pitch.h"
#include "pitch_plan.h"
#include "rir.h"
#include "rir_plan.h"

// a slot holds a call's nww_mix_item table and, right behind its B items, the nww_rir_item table of a call that has one, and behind
// that the nww_pitch_item table of a call that has one: ONE copy
constexpr size_t MIX_SLOT_ITEM_BYTES = sizeof(nww_mix_item) + sizeof(nww_rir_item) + sizeof(nww_pitch_item);

struct MixState {
    unsigned char* d_tab = nullptr; unsigned char* pin_tab = nullptr;  // [POOL_TAB_SLOTS][slot_items * MIX_SLOT_ITEM_BYTES]
    hipEvent_t ev[POOL_TAB_SLOTS] = {};
    size_t slot_items = 0; unsigned seq = 0;
    // the host-pointer entry point's arena and clips, grown on demand
    int16_t* d_arena = nullptr; int16_t* d_out = nullptr; size_t arena_bytes = 0, out_bytes = 0;
    // impulse responses (rir.hip): the twiddle table of each transform size, made by the first call that needs it
    float* d_tw[3] = {nullptr, nullptr, nullptr};
    // the segmented route's float32 clips before the tail [B][N] and, behind them, the segments' peaks [B][Q]
    void* d_seg = nullptr; size_t seg_bytes = 0;
    // pitch shift (pitch.hip): the ratios and their resampler tables (nww_pitch_set_ratios), the constant tables (made with the first
    // ratios), and the shifted clips' float32 scratch - w [rows][N], then s [rows][pitch_stride(N)] - grown on demand
    int n_ratios = 0;
    PitchRatio* d_ratios = nullptr; float* d_taps = nullptr; float* d_ptables = nullptr;
    void* d_pitch = nullptr; size_t pitch_bytes = 0;
};

void nww_mix_free(nww_handle* h) {
    MixState* m = h->mix;
    if (!m) return;
    if (m->d_tab) (void)hipFree(m->d_tab);
    if (m->pin_tab) (void)hipHostFree(m->pin_tab);
    for (hipEvent_t e : m->ev) if (e) (void)hipEventDestroy(e);
    if (m->d_arena) (void)hipFree(m->d_arena);
    if (m->d_out) (void)hipFree(m->d_out);
    for (float* t : m->d_tw) if (t) (void)hipFree(t);
    if (m->d_seg) (void)hipFree(m->d_seg);
    if (m->d_ratios) (void)hipFree(m->d_ratios);
    if (m->d_taps) (void)hipFree(m->d_taps);
    if (m->d_ptables) (void)hipFree(m->d_ptables);
    if (m->d_pitch) (void)hipFree(m->d_pitch);
    delete m;
    h->mix = nullptr;
}

// table slots for calls of B items (a larger call than any before waits for the device and replaces them)
static int mix_slots(nww_handle* h, size_t B) {
    if (!h->mix) h->mix = new MixState();
    MixState* m = h->mix;
    if (!m->ev[0]) for (hipEvent_t& e : m->ev) HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (B <= m->slot_items) return NWW_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    if (m->d_tab) (void)hipFree(m->d_tab);
    if (m->pin_tab) (void)hipHostFree(m->pin_tab);
    m->d_tab = nullptr; m->pin_tab = nullptr; m->slot_items = 0; m->seq = 0;
    const size_t items = (B + 255) & ~(size_t)255;
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&m->d_tab), POOL_TAB_SLOTS * items * MIX_SLOT_ITEM_BYTES));
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&m->pin_tab), POOL_TAB_SLOTS * items * MIX_SLOT_ITEM_BYTES, hipHostMallocDefault));
    m->slot_items = items;
    return NWW_OK;
}

// the twiddle table of transform size M on the device (rir_plan.h: float64, rounded once), made on first use
static int rir_twiddles(nww_handle* h, int M, const float** d_tw) {
    if (!h->mix) h->mix = new MixState();
    MixState* m = h->mix;
    if (M == NWW_RIR_SEGMENTED) M = RIR_M_MAX;
    const int k = M == 2048 ? 0 : M == 8192 ? 1 : 2;
    if (!m->d_tw[k]) {
        std::vector<RirC> T((size_t)rir_twiddle_count(M));
        rir_twiddles_host(M, T.data());
        float* d = nullptr;
        HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&d), T.size() * sizeof(RirC)));
        const hipError_t e = hipMemcpy(d, T.data(), T.size() * sizeof(RirC), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); return fail(h, NWW_ERR_HIP, "twiddle upload failed: %s", hipGetErrorString(e)); }
        m->d_tw[k] = d;
    }
    *d_tw = m->d_tw[k];
    return NWW_OK;
}

// what every entry point checks before anything is enqueued; *done: B == 0, the call is complete
static int mix_check(nww_handle* h, const void* d_arena, int64_t arena_samples, const nww_mix_item* items, int32_t B, int32_t N, bool* done) {
    *done = false;
    if (!h) return NWW_ERR_INVALID;
    if (!h->finalized) return fail(h, NWW_ERR_STATE, "model not finalized: call nww_finalize after loading the state_dict");
    if (B < 0) return fail(h, NWW_ERR_INVALID, "batch must not be negative (got %d)", B);
    if (B == 0) { *done = true; return NWW_OK; }
    if (N < 1) return fail(h, NWW_ERR_INVALID, "a clip needs at least one sample (got %d)", N);
    if (!d_arena || arena_samples < 1 || !items) return fail(h, NWW_ERR_INVALID, "null or empty arena, or null item table");
    const char* field = nullptr;
    const int64_t bad = mix_first_bad_item(items, B, arena_samples, N, &field);
    if (bad >= 0)
        return fail(h, NWW_ERR_INVALID, "mix item %lld: %s out of range (arena of %lld samples, clips of %d)", (long long)bad, field,
                    (long long)arena_samples, N);
    return NWW_OK;
}

// the validated tables through the next slot, then the kernels, on s.  rir_items == null: mix.hip; otherwise rir.hip at M.  With
// pitch_items, pitch.hip first shifts the clips that name a ratio: without responses it finishes them itself, behind mix.hip (which
// has written those rows in vain: its kernel and its bits stay what they are); with responses rir.hip's PITCH instances stage them.
static int mix_enqueue(nww_handle* h, const int16_t* d_arena, const nww_mix_item* items, int B, int N, int16_t* d_out, hipStream_t s,
                       const nww_rir_item* rir_items = nullptr, const float* d_spectra = nullptr, int M = 0,
                       const nww_pitch_item* pitch_items = nullptr) {
    int rc = mix_slots(h, (size_t)B);
    if (rc) return rc;
    MixState* m = h->mix;
    const float* d_tw = nullptr;
    const bool seg = rir_items && M == NWW_RIR_SEGMENTED;
    const size_t w_bytes = (size_t)B * (size_t)N * sizeof(float);
    if (rir_items) {
        rc = rir_twiddles(h, M, &d_tw);
        if (!rc && seg) rc = nww_grow(h, &m->d_seg, &m->seg_bytes, w_bytes + (size_t)B * (size_t)rir_segments(N) * sizeof(unsigned));
        if (rc) return rc;
    }
    size_t rows = 0;                                                   // the clips that name a ratio: their rows in the scratch
    if (pitch_items)
        for (int i = 0; i < B; ++i) rows += pitch_items[i].pitch_id >= 0;
    const int s_stride = rows ? pitch_stride(N) : 0;
    if (rows) {
        rc = nww_grow(h, &m->d_pitch, &m->pitch_bytes, rows * ((size_t)N + (size_t)s_stride) * sizeof(float));
        if (rc) return rc;
    }
    const unsigned slot = m->seq % POOL_TAB_SLOTS;
    if (m->seq >= POOL_TAB_SLOTS) HIP_TRY(h, hipEventSynchronize(m->ev[slot]));      // the slot's previous call has passed
    ++m->seq;
    unsigned char* pin = m->pin_tab + slot * m->slot_items * MIX_SLOT_ITEM_BYTES;
    unsigned char* dev = m->d_tab + slot * m->slot_items * MIX_SLOT_ITEM_BYTES;
    const size_t tab_bytes = (size_t)B * sizeof(nww_mix_item), rtab_bytes = rir_items ? (size_t)B * sizeof(nww_rir_item) : 0;
    const size_t ptab_bytes = rows ? (size_t)B * sizeof(nww_pitch_item) : 0;
    std::memcpy(pin, items, tab_bytes);
    if (rir_items) std::memcpy(pin + tab_bytes, rir_items, rtab_bytes);
    if (rows) {                                                        // as uploaded, `reserved` carries the clip's row
        nww_pitch_item* pt = reinterpret_cast<nww_pitch_item*>(pin + tab_bytes + rtab_bytes);
        uint32_t row = 0;
        for (int i = 0; i < B; ++i) pt[i] = {pitch_items[i].pitch_id, pitch_items[i].pitch_id >= 0 ? row++ : 0u};
    }
    HIP_TRY(h, hipMemcpyAsync(dev, pin, tab_bytes + rtab_bytes + ptab_bytes, hipMemcpyHostToDevice, s));
    const nww_mix_item* d_items = reinterpret_cast<const nww_mix_item*>(dev);
    const nww_rir_item* d_ritems = reinterpret_cast<const nww_rir_item*>(dev + tab_bytes);
    const nww_pitch_item* d_pitems = rows ? reinterpret_cast<const nww_pitch_item*>(dev + tab_bytes + rtab_bytes) : nullptr;
    float* d_y = static_cast<float*>(m->d_pitch);
    hipError_t e = hipSuccess;
    if (rows && rir_items)
        e = pitch_launch(d_arena, d_items, d_pitems, m->d_ratios, m->d_taps, m->d_ptables, B, N, d_y, d_y + rows * (size_t)N, s_stride, nullptr, s);
    if (e == hipSuccess)
        e = seg         ? rir_seg_mix_launch(d_arena, d_items, d_ritems, d_spectra, d_tw, B, N, static_cast<float*>(m->d_seg),
                                             reinterpret_cast<unsigned*>(static_cast<unsigned char*>(m->d_seg) + w_bytes), d_out, s, d_pitems, d_y)
            : rir_items ? rir_mix_launch(d_arena, d_items, d_ritems, d_spectra, M, d_tw, B, N, d_out, s, d_pitems, d_y)
                        : mix_launch(d_arena, d_items, B, N, d_out, h->cu_count, s);
    if (e == hipSuccess && rows && !rir_items)
        e = pitch_launch(d_arena, d_items, d_pitems, m->d_ratios, m->d_taps, m->d_ptables, B, N, d_y, d_y + rows * (size_t)N, s_stride, d_out, s);
    (void)hipEventRecord(m->ev[slot], s);
    if (e != hipSuccess)
        return fail(h, NWW_ERR_HIP, "launch '%s' failed: %s", rows ? "mix_aug" : rir_items ? "mix_rir" : "mix", hipGetErrorString(e));
    return NWW_OK;
}

extern "C" int nww_mix_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const nww_mix_item* items, int32_t B, int32_t N,
                           int16_t* d_out, void* stream) {
    bool done = false;
    int rc = mix_check(h, d_arena, arena_samples, items, B, N, &done);
    if (rc || done) return rc;
    if (!d_out) return fail(h, NWW_ERR_INVALID, "null device pointer");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return mix_enqueue(h, d_arena, items, B, N, d_out, stream ? (hipStream_t)stream : h->own_stream);
}

extern "C" int nww_mix(nww_handle* h, const int16_t* arena, int64_t arena_samples, const nww_mix_item* items, int32_t B, int32_t N, int16_t* out) {
    bool done = false;
    int rc = mix_check(h, arena, arena_samples, items, B, N, &done);
    if (rc || done) return rc;
    if (!out) return fail(h, NWW_ERR_INVALID, "null output pointer");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = mix_slots(h, (size_t)B);
    if (rc) return rc;
    MixState* m = h->mix;
    const size_t ab = (size_t)arena_samples * sizeof(int16_t), ob = (size_t)B * N * sizeof(int16_t);
    rc = nww_grow(h, reinterpret_cast<void**>(&m->d_arena), &m->arena_bytes, ab);
    if (!rc) rc = nww_grow(h, reinterpret_cast<void**>(&m->d_out), &m->out_bytes, ob);
    if (rc) return rc;
    hipStream_t s = h->own_stream;
    HIP_TRY(h, hipMemcpyAsync(m->d_arena, arena, ab, hipMemcpyHostToDevice, s));
    rc = mix_enqueue(h, m->d_arena, items, B, N, m->d_out, s);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, m->d_out, ob, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return NWW_OK;
}

extern "C" int nww_mix_forward_pcm_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const nww_mix_item* items, int32_t B, int32_t N,
                                       float* d_logits, float* d_probs, void* stream) {
    bool done = false;
    int rc = mix_check(h, d_arena, arena_samples, items, B, N, &done);
    if (rc || done) return rc;
    // the clip against the head before anything is enqueued, in nww_forward_pcm's wording
    const ClipRows cr = nww_clip_rows(h, N);
    if (cr.T <= 0) return nww_fail_short_clip(h, N);
    if (!cr.fits)
        return fail(h, NWW_ERR_SHAPE, "frontend yields (%d,%d) features for %d samples but the head was built for input_shape=(%d,%d)", cr.rows,
                    cr.cols, N, h->cfg.in_rows, h->cfg.in_cols);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = nww_ensure_ws(h, B, N);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->own_stream;
    rc = mix_enqueue(h, d_arena, items, B, N, h->d_pcm, s);
    if (rc) return rc;
    return nww_forward_pcm_on_dev(h, h->d_pcm, B, N, d_logits, d_probs, s);
}

extern "C" int nww_mix_frontend_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const nww_mix_item* items, int32_t B, int32_t N,
                                    float* d_logmel, int32_t frames_major, void* stream) {
    bool done = false;
    int rc = mix_check(h, d_arena, arena_samples, items, B, N, &done);
    if (rc || done) return rc;
    if (!d_logmel) return fail(h, NWW_ERR_INVALID, "null device pointer");
    if (nww_pcm_rows(h, N) <= 0) return nww_fail_short_clip(h, N);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = nww_ensure_ws(h, B, N);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->own_stream;
    rc = mix_enqueue(h, d_arena, items, B, N, h->d_pcm, s);
    if (rc) return rc;
    return nww_frontend_on_dev(h, h->d_pcm, B, N, d_logmel, nullptr, frames_major, s, nullptr);
}

// ---- ... through a room impulse response (rir.hip, rir_plan.h)
extern "C" int32_t nww_rir_fft_size(int32_t N, int32_t max_ir_len) { return rir_fft_size(N, max_ir_len); }
extern "C" int32_t nww_rir_parts(int32_t N, int32_t max_ir_len) { return rir_parts(N, max_ir_len); }
extern "C" int64_t nww_rir_spectra_floats(int32_t K, int32_t N, int32_t max_ir_len, int32_t M) { return rir_spectra_floats(K, N, max_ir_len, M); }

extern "C" int nww_rir_prepare_dev(nww_handle* h, const float* d_irs, const int64_t* ir_off, const int32_t* ir_len, int32_t K, int32_t N, int32_t M,
                                   float* d_spectra, void* stream) {
    if (!h) return NWW_ERR_INVALID;
    if (!h->finalized) return fail(h, NWW_ERR_STATE, "model not finalized: call nww_finalize after loading the state_dict");
    if (K < 0) return fail(h, NWW_ERR_INVALID, "the number of responses must not be negative (got %d)", K);
    if (K == 0) return NWW_OK;
    if (N < 1) return fail(h, NWW_ERR_INVALID, "a clip needs at least one sample (got %d)", N);
    if (!d_irs || !ir_off || !ir_len || !d_spectra) return fail(h, NWW_ERR_INVALID, "null response buffer, table or spectra");
    const bool seg = M == NWW_RIR_SEGMENTED;
    if (!seg && !rir_size_fits(M, N)) return fail(h, NWW_ERR_INVALID, "M = %d is not a transform size (2048, 8192, 32768) that holds clips of %d", M, N);
    const char* why = "";
    const int64_t bad = seg ? rir_seg_first_bad_response(ir_len, K) : rir_first_bad_response(ir_len, K, N, M, &why);
    if (bad >= 0) {
        if (why[0] == 'o')
            return fail(h, NWW_ERR_INVALID, "response %lld: %d taps against clips of %d need more than 32768 points: overlap-save not built",
                        (long long)bad, ir_len[bad], N);
        if (why[0] == 'M') return fail(h, NWW_ERR_INVALID, "response %lld: %d taps against clips of %d do not fit M = %d", (long long)bad, ir_len[bad], N, M);
        return fail(h, NWW_ERR_INVALID, "response %lld: ir_len out of range (got %d)", (long long)bad, ir_len[bad]);
    }
    for (int32_t k = 0; k < K; ++k)
        if (ir_off[k] < 0) return fail(h, NWW_ERR_INVALID, "response %d: ir_off out of range", k);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const float* d_tw = nullptr;
    int rc = rir_twiddles(h, M, &d_tw);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->own_stream;
    unsigned char* d_tab = nullptr;                                    // [K] offsets, then [K] lengths: freed once the stream has passed
    const size_t off_bytes = (size_t)K * sizeof(int64_t), len_bytes = (size_t)K * sizeof(int32_t);
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&d_tab), off_bytes + len_bytes));
    hipError_t e = hipMemcpyAsync(d_tab, ir_off, off_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab + off_bytes, ir_len, len_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        const int64_t* d_off = reinterpret_cast<const int64_t*>(d_tab);
        const int32_t* d_len = reinterpret_cast<const int32_t*>(d_tab + off_bytes);
        int32_t longest = 1;
        for (int32_t k = 0; k < K; ++k) longest = ir_len[k] > longest ? ir_len[k] : longest;
        e = seg ? rir_seg_prepare_launch(d_irs, d_off, d_len, K, N, rir_parts(N, longest), d_tw, d_spectra, s)
                : rir_prepare_launch(d_irs, d_off, d_len, K, N, M, d_tw, d_spectra, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s);
    (void)hipFree(d_tab);
    if (e != hipSuccess) return fail(h, NWW_ERR_HIP, "launch 'rir_prepare' failed: %s", hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(h, NWW_ERR_HIP, "rir_prepare failed: %s", hipGetErrorString(e2));
    return NWW_OK;
}

// what the rir calls check behind mix_check, before anything is enqueued (rir_items != null)
static int rir_check(nww_handle* h, const float* d_spectra, int32_t n_irs, int32_t M, const nww_rir_item* rir_items, int32_t B, int32_t N) {
    if (n_irs < 0) return fail(h, NWW_ERR_INVALID, "n_irs must not be negative (got %d)", n_irs);
    if (n_irs > 0 && !d_spectra) return fail(h, NWW_ERR_INVALID, "null spectra");
    if (M != NWW_RIR_SEGMENTED && !rir_size_fits(M, N))
        return fail(h, NWW_ERR_INVALID, "M = %d is not a transform size (2048, 8192, 32768) that holds clips of %d", M, N);
    const char* field = nullptr;
    const int64_t bad = rir_first_bad_item(rir_items, B, n_irs, &field);
    if (bad >= 0) return fail(h, NWW_ERR_INVALID, "rir item %lld: %s out of range (%d responses)", (long long)bad, field, n_irs);
    return NWW_OK;
}

extern "C" int nww_mix_rir_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                               const nww_mix_item* items, const nww_rir_item* rir_items, int32_t B, int32_t N, int16_t* d_out, void* stream) {
    if (!rir_items) return nww_mix_dev(h, d_arena, arena_samples, items, B, N, d_out, stream);
    bool done = false;
    int rc = mix_check(h, d_arena, arena_samples, items, B, N, &done);
    if (rc || done) return rc;
    rc = rir_check(h, d_spectra, n_irs, M, rir_items, B, N);
    if (rc) return rc;
    if (!d_out) return fail(h, NWW_ERR_INVALID, "null device pointer");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return mix_enqueue(h, d_arena, items, B, N, d_out, stream ? (hipStream_t)stream : h->own_stream, rir_items, d_spectra, M);
}

extern "C" int nww_mix_rir(nww_handle* h, const int16_t* arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                           const nww_mix_item* items, const nww_rir_item* rir_items, int32_t B, int32_t N, int16_t* out) {
    if (!rir_items) return nww_mix(h, arena, arena_samples, items, B, N, out);
    bool done = false;
    int rc = mix_check(h, arena, arena_samples, items, B, N, &done);
    if (rc || done) return rc;
    rc = rir_check(h, d_spectra, n_irs, M, rir_items, B, N);
    if (rc) return rc;
    if (!out) return fail(h, NWW_ERR_INVALID, "null output pointer");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = mix_slots(h, (size_t)B);
    if (rc) return rc;
    MixState* m = h->mix;
    const size_t ab = (size_t)arena_samples * sizeof(int16_t), ob = (size_t)B * N * sizeof(int16_t);
    rc = nww_grow(h, reinterpret_cast<void**>(&m->d_arena), &m->arena_bytes, ab);
    if (!rc) rc = nww_grow(h, reinterpret_cast<void**>(&m->d_out), &m->out_bytes, ob);
    if (rc) return rc;
    hipStream_t s = h->own_stream;
    HIP_TRY(h, hipMemcpyAsync(m->d_arena, arena, ab, hipMemcpyHostToDevice, s));
    rc = mix_enqueue(h, m->d_arena, items, B, N, m->d_out, s, rir_items, d_spectra, M);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, m->d_out, ob, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return NWW_OK;
}

extern "C" int nww_mix_rir_forward_pcm_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                                           const nww_mix_item* items, const nww_rir_item* rir_items, int32_t B, int32_t N, float* d_logits,
                                           float* d_probs, void* stream) {
    if (!rir_items) return nww_mix_forward_pcm_dev(h, d_arena, arena_samples, items, B, N, d_logits, d_probs, stream);
    bool done = false;
    int rc = mix_check(h, d_arena, arena_samples, items, B, N, &done);
    if (rc || done) return rc;
    rc = rir_check(h, d_spectra, n_irs, M, rir_items, B, N);
    if (rc) return rc;
    const ClipRows cr = nww_clip_rows(h, N);
    if (cr.T <= 0) return nww_fail_short_clip(h, N);
    if (!cr.fits)
        return fail(h, NWW_ERR_SHAPE, "frontend yields (%d,%d) features for %d samples but the head was built for input_shape=(%d,%d)", cr.rows,
                    cr.cols, N, h->cfg.in_rows, h->cfg.in_cols);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = nww_ensure_ws(h, B, N);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->own_stream;
    rc = mix_enqueue(h, d_arena, items, B, N, h->d_pcm, s, rir_items, d_spectra, M);
    if (rc) return rc;
    return nww_forward_pcm_on_dev(h, h->d_pcm, B, N, d_logits, d_probs, s);
}

extern "C" int nww_mix_rir_frontend_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                                        const nww_mix_item* items, const nww_rir_item* rir_items, int32_t B, int32_t N, float* d_logmel,
                                        int32_t frames_major, void* stream) {
    if (!rir_items) return nww_mix_frontend_dev(h, d_arena, arena_samples, items, B, N, d_logmel, frames_major, stream);
    bool done = false;
    int rc = mix_check(h, d_arena, arena_samples, items, B, N, &done);
    if (rc || done) return rc;
    rc = rir_check(h, d_spectra, n_irs, M, rir_items, B, N);
    if (rc) return rc;
    if (!d_logmel) return fail(h, NWW_ERR_INVALID, "null device pointer");
    if (nww_pcm_rows(h, N) <= 0) return nww_fail_short_clip(h, N);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = nww_ensure_ws(h, B, N);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->own_stream;
    rc = mix_enqueue(h, d_arena, items, B, N, h->d_pcm, s, rir_items, d_spectra, M);
    if (rc) return rc;
    return nww_frontend_on_dev(h, h->d_pcm, B, N, d_logmel, nullptr, frames_major, s, nullptr);
}

// ---- ... with a pitch shift between the gain and the response (pitch.hip, pitch_plan.h)
extern "C" int nww_pitch_set_ratios(nww_handle* h, const int32_t* num, const int32_t* den, int32_t K) {
    if (!h) return NWW_ERR_INVALID;
    if (!h->finalized) return fail(h, NWW_ERR_STATE, "model not finalized: call nww_finalize after loading the state_dict");
    if (K < 0 || K > PITCH_MAX_RATIOS) return fail(h, NWW_ERR_INVALID, "the number of pitch ratios must lie in [0, %d] (got %d)", PITCH_MAX_RATIOS, K);
    if (K > 0 && (!num || !den)) return fail(h, NWW_ERR_INVALID, "null ratio table");
    const int32_t bad = pitch_first_bad_ratio(num, den, K);
    if (bad >= 0)
        return fail(h, NWW_ERR_INVALID, "pitch ratio %d: %d / %d out of range (terms in [1, %d], 2^(-4/12) <= num / den <= 2^(4/12))", bad, num[bad],
                    den[bad], PITCH_MAX_TERM);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->mix) h->mix = new MixState();
    MixState* m = h->mix;
    // everything new is built and uploaded before anything of the handle's is replaced
    std::vector<PitchRatio> ratios((size_t)K);
    std::vector<float> taps;
    for (int32_t k = 0; k < K; ++k) {
        ratios[(size_t)k] = {num[k], den[k], (int32_t)taps.size(), 0};
        taps.resize(taps.size() + (size_t)den[k] * PITCH_TAPS);
        pitch_resample_table(num[k], den[k], taps.data() + ratios[(size_t)k].off);
    }
    PitchRatio* d_ratios = nullptr;
    float* d_taps = nullptr;
    float* d_tables = m->d_ptables;
    hipError_t e = hipSuccess;
    if (K > 0) {
        e = hipMalloc(reinterpret_cast<void**>(&d_ratios), ratios.size() * sizeof(PitchRatio));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_taps), taps.size() * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(d_ratios, ratios.data(), ratios.size() * sizeof(PitchRatio), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess && !d_tables) {
            const PitchTables tb;
            std::vector<float> all((size_t)PITCH_TAB_FLOATS);
            std::memcpy(all.data() + PITCH_TAB_TW, tb.T.data(), tb.T.size() * sizeof(RirC));
            std::memcpy(all.data() + PITCH_TAB_WIN, tb.win.data(), tb.win.size() * sizeof(float));
            std::memcpy(all.data() + PITCH_TAB_ENV, tb.env.data(), tb.env.size() * sizeof(float));
            e = hipMalloc(reinterpret_cast<void**>(&d_tables), all.size() * sizeof(float));
            if (e == hipSuccess) e = hipMemcpy(d_tables, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice);
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();                   // no call in flight reads the tables that go
    if (e != hipSuccess) {
        if (d_ratios) (void)hipFree(d_ratios);
        if (d_taps) (void)hipFree(d_taps);
        if (d_tables && d_tables != m->d_ptables) (void)hipFree(d_tables);
        return fail(h, NWW_ERR_HIP, "pitch table upload failed: %s", hipGetErrorString(e));
    }
    if (m->d_ratios) (void)hipFree(m->d_ratios);
    if (m->d_taps) (void)hipFree(m->d_taps);
    m->d_ratios = d_ratios; m->d_taps = d_taps; m->d_ptables = d_tables; m->n_ratios = K;
    return NWW_OK;
}

// what the aug calls check behind mix_check (and rir_check), before anything is enqueued (pitch_items != null)
static int pitch_check(nww_handle* h, const nww_pitch_item* pitch_items, int32_t B, int32_t N) {
    const int K = h->mix ? h->mix->n_ratios : 0;
    if (K < 1) return fail(h, NWW_ERR_INVALID, "no pitch ratios set: call nww_pitch_set_ratios first");
    if (!pitch_length_ok(N))
        return fail(h, NWW_ERR_INVALID, "N = %d: a clip shifted in pitch needs more than 256 samples for the reflect padding, and at most %d", N, PITCH_MAX_N);
    const char* field = nullptr;
    const int64_t bad = pitch_first_bad_item(pitch_items, B, K, &field);
    if (bad >= 0) return fail(h, NWW_ERR_INVALID, "pitch item %lld: %s out of range (%d ratios)", (long long)bad, field, K);
    return NWW_OK;
}

// the checks of an aug call with pitch_items; *done: B == 0
static int aug_check(nww_handle* h, const void* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                     const nww_mix_item* items, const nww_rir_item* rir_items, const nww_pitch_item* pitch_items, int32_t B, int32_t N, bool* done) {
    int rc = mix_check(h, d_arena, arena_samples, items, B, N, done);
    if (rc || *done) return rc;
    if (rir_items) {
        rc = rir_check(h, d_spectra, n_irs, M, rir_items, B, N);
        if (rc) return rc;
    }
    return pitch_check(h, pitch_items, B, N);
}

extern "C" int nww_mix_aug_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                               const nww_mix_item* items, const nww_rir_item* rir_items, const nww_pitch_item* pitch_items, int32_t B, int32_t N,
                               int16_t* d_out, void* stream) {
    if (!pitch_items) return nww_mix_rir_dev(h, d_arena, arena_samples, d_spectra, n_irs, M, items, rir_items, B, N, d_out, stream);
    bool done = false;
    const int rc = aug_check(h, d_arena, arena_samples, d_spectra, n_irs, M, items, rir_items, pitch_items, B, N, &done);
    if (rc || done) return rc;
    if (!d_out) return fail(h, NWW_ERR_INVALID, "null device pointer");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return mix_enqueue(h, d_arena, items, B, N, d_out, stream ? (hipStream_t)stream : h->own_stream, rir_items, d_spectra, M, pitch_items);
}

extern "C" int nww_mix_aug(nww_handle* h, const int16_t* arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs, int32_t M,
                           const nww_mix_item* items, const nww_rir_item* rir_items, const nww_pitch_item* pitch_items, int32_t B, int32_t N,
                           int16_t* out) {
    if (!pitch_items) return nww_mix_rir(h, arena, arena_samples, d_spectra, n_irs, M, items, rir_items, B, N, out);
    bool done = false;
    int rc = aug_check(h, arena, arena_samples, d_spectra, n_irs, M, items, rir_items, pitch_items, B, N, &done);
    if (rc || done) return rc;
    if (!out) return fail(h, NWW_ERR_INVALID, "null output pointer");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = mix_slots(h, (size_t)B);
    if (rc) return rc;
    MixState* m = h->mix;
    const size_t ab = (size_t)arena_samples * sizeof(int16_t), ob = (size_t)B * N * sizeof(int16_t);
    rc = nww_grow(h, reinterpret_cast<void**>(&m->d_arena), &m->arena_bytes, ab);
    if (!rc) rc = nww_grow(h, reinterpret_cast<void**>(&m->d_out), &m->out_bytes, ob);
    if (rc) return rc;
    hipStream_t s = h->own_stream;
    HIP_TRY(h, hipMemcpyAsync(m->d_arena, arena, ab, hipMemcpyHostToDevice, s));
    rc = mix_enqueue(h, m->d_arena, items, B, N, m->d_out, s, rir_items, d_spectra, M, pitch_items);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, m->d_out, ob, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return NWW_OK;
}

extern "C" int nww_mix_aug_forward_pcm_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs,
                                           int32_t M, const nww_mix_item* items, const nww_rir_item* rir_items, const nww_pitch_item* pitch_items,
                                           int32_t B, int32_t N, float* d_logits, float* d_probs, void* stream) {
    if (!pitch_items)
        return nww_mix_rir_forward_pcm_dev(h, d_arena, arena_samples, d_spectra, n_irs, M, items, rir_items, B, N, d_logits, d_probs, stream);
    bool done = false;
    int rc = aug_check(h, d_arena, arena_samples, d_spectra, n_irs, M, items, rir_items, pitch_items, B, N, &done);
    if (rc || done) return rc;
    const ClipRows cr = nww_clip_rows(h, N);
    if (cr.T <= 0) return nww_fail_short_clip(h, N);
    if (!cr.fits)
        return fail(h, NWW_ERR_SHAPE, "frontend yields (%d,%d) features for %d samples but the head was built for input_shape=(%d,%d)", cr.rows,
                    cr.cols, N, h->cfg.in_rows, h->cfg.in_cols);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = nww_ensure_ws(h, B, N);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->own_stream;
    rc = mix_enqueue(h, d_arena, items, B, N, h->d_pcm, s, rir_items, d_spectra, M, pitch_items);
    if (rc) return rc;
    return nww_forward_pcm_on_dev(h, h->d_pcm, B, N, d_logits, d_probs, s);
}

extern "C" int nww_mix_aug_frontend_dev(nww_handle* h, const int16_t* d_arena, int64_t arena_samples, const float* d_spectra, int32_t n_irs,
                                        int32_t M, const nww_mix_item* items, const nww_rir_item* rir_items, const nww_pitch_item* pitch_items,
                                        int32_t B, int32_t N, float* d_logmel, int32_t frames_major, void* stream) {
    if (!pitch_items)
        return nww_mix_rir_frontend_dev(h, d_arena, arena_samples, d_spectra, n_irs, M, items, rir_items, B, N, d_logmel, frames_major, stream);
    bool done = false;
    int rc = aug_check(h, d_arena, arena_samples, d_spectra, n_irs, M, items, rir_items, pitch_items, B, N, &done);
    if (rc || done) return rc;
    if (!d_logmel) return fail(h, NWW_ERR_INVALID, "null device pointer");
    if (nww_pcm_rows(h, N) <= 0) return nww_fail_short_clip(h, N);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = nww_ensure_ws(h, B, N);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->own_stream;
    rc = mix_enqueue(h, d_arena, items, B, N, h->d_pcm, s, rir_items, d_spectra, M, pitch_items);
    if (rc) return rc;
    return nww_frontend_on_dev(h, h->d_pcm, B, N, d_logmel, nullptr, frames_major, s, nullptr);
}
