// nww_mix.hip - clips mixed on the device (nww_mix_*, include/nww.h): the host validates a call's items (mix_plan.h),
// the table goes up through the next of MIX_TAB_SLOTS = POOL_TAB_SLOTS slots of the handle's own pinned and device buffers - a slot is
// rewritten once the event behind its previous call has passed, as the pool tables' are (nww_stream.hip) - and mix.hip gathers, measures
// and mixes.  The forward and frontend forms mix into the handle's PCM staging and run the existing paths on it.
#include "nww_internal.h"
#include "mix.h"
#include "mix_plan.h"

struct MixState {
    nww_mix_item* d_tab = nullptr; nww_mix_item* pin_tab = nullptr;    // [POOL_TAB_SLOTS][slot_items]
    hipEvent_t ev[POOL_TAB_SLOTS] = {};
    size_t slot_items = 0; unsigned seq = 0;
    // the host-pointer entry point's arena and clips, grown on demand
    int16_t* d_arena = nullptr; int16_t* d_out = nullptr; size_t arena_bytes = 0, out_bytes = 0;
};

void nww_mix_free(nww_handle* h) {
    MixState* m = h->mix;
    if (!m) return;
    if (m->d_tab) (void)hipFree(m->d_tab);
    if (m->pin_tab) (void)hipHostFree(m->pin_tab);
    for (hipEvent_t e : m->ev) if (e) (void)hipEventDestroy(e);
    if (m->d_arena) (void)hipFree(m->d_arena);
    if (m->d_out) (void)hipFree(m->d_out);
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
    HIP_TRY(h, hipMalloc(&m->d_tab, POOL_TAB_SLOTS * items * sizeof(nww_mix_item)));
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&m->pin_tab), POOL_TAB_SLOTS * items * sizeof(nww_mix_item), hipHostMallocDefault));
    m->slot_items = items;
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

// the validated table through the next slot, then the kernel, on s
static int mix_enqueue(nww_handle* h, const int16_t* d_arena, const nww_mix_item* items, int B, int N, int16_t* d_out, hipStream_t s) {
    int rc = mix_slots(h, (size_t)B);
    if (rc) return rc;
    MixState* m = h->mix;
    const unsigned slot = m->seq % POOL_TAB_SLOTS;
    if (m->seq >= POOL_TAB_SLOTS) HIP_TRY(h, hipEventSynchronize(m->ev[slot]));      // the slot's previous call has passed
    ++m->seq;
    nww_mix_item* pin = m->pin_tab + slot * m->slot_items;
    nww_mix_item* dev = m->d_tab + slot * m->slot_items;
    std::memcpy(pin, items, (size_t)B * sizeof(nww_mix_item));
    HIP_TRY(h, hipMemcpyAsync(dev, pin, (size_t)B * sizeof(nww_mix_item), hipMemcpyHostToDevice, s));
    const hipError_t e = mix_launch(d_arena, dev, B, N, d_out, h->cu_count, s);
    (void)hipEventRecord(m->ev[slot], s);
    if (e != hipSuccess) return fail(h, NWW_ERR_HIP, "launch 'mix' failed: %s", hipGetErrorString(e));
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
