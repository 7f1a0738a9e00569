// nww_resample.hip - recordings brought to the target rate on the device (nww_resample_*, include/nww.h): the host
// validates a call's items (resample_plan.h) and writes every item's first tile into the copy that goes up - a prefix over the table,
// which is how a workgroup of resample.hip finds its item - through the next of POOL_TAB_SLOTS slots of the handle's own pinned and
// device buffers, as nww_mix.hip's tables go.  The ratios and their tap tables live on the handle, apart from the pitch ratios.
#include <vector>

#include "nww_internal.h"
#include "resample.h"
#include "resample_plan.h"

struct ResampleState {
    nww_resample_item* d_tab = nullptr; nww_resample_item* pin_tab = nullptr;     // [POOL_TAB_SLOTS][slot_items]
    hipEvent_t ev[POOL_TAB_SLOTS] = {};
    size_t slot_items = 0; unsigned seq = 0;
    // the ratios (nww_resample_set_ratios): on the host for the checks, on the device with their tables for the kernel
    int n_ratios = 0, span_floats = 0;
    int32_t num[RESAMPLE_MAX_RATIOS] = {}, den[RESAMPLE_MAX_RATIOS] = {};
    ResampleRatio* d_ratios = nullptr; float* d_taps = nullptr;
    // the host-pointer entry point's source and destination, grown on demand
    void* d_src = nullptr; void* d_dst = nullptr; size_t src_bytes = 0, dst_bytes = 0;
};

void nww_resample_free(nww_handle* h) {
    ResampleState* m = h->resample;
    if (!m) return;
    if (m->d_tab) (void)hipFree(m->d_tab);
    if (m->pin_tab) (void)hipHostFree(m->pin_tab);
    for (hipEvent_t e : m->ev) if (e) (void)hipEventDestroy(e);
    if (m->d_ratios) (void)hipFree(m->d_ratios);
    if (m->d_taps) (void)hipFree(m->d_taps);
    if (m->d_src) (void)hipFree(m->d_src);
    if (m->d_dst) (void)hipFree(m->d_dst);
    delete m;
    h->resample = nullptr;
}

// table slots for calls of B items (a larger call than any before waits for the device and replaces them)
static int resample_slots(nww_handle* h, size_t B) {
    ResampleState* m = h->resample;
    if (!m->ev[0]) for (hipEvent_t& e : m->ev) HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (B <= m->slot_items) return NWW_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    if (m->d_tab) (void)hipFree(m->d_tab);
    if (m->pin_tab) (void)hipHostFree(m->pin_tab);
    m->d_tab = nullptr; m->pin_tab = nullptr; m->slot_items = 0; m->seq = 0;
    const size_t items = (B + 255) & ~(size_t)255;
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&m->d_tab), POOL_TAB_SLOTS * items * sizeof(nww_resample_item)));
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&m->pin_tab), POOL_TAB_SLOTS * items * sizeof(nww_resample_item), hipHostMallocDefault));
    m->slot_items = items;
    return NWW_OK;
}

extern "C" int64_t nww_resample_length(int64_t frames, int32_t num, int32_t den) {
    if (frames < 1 || frames > RESAMPLE_MAX_FRAMES || !resample_ratio_ok(num, den)) return 0;
    return resample_length(frames, num, den);
}

extern "C" int nww_resample_set_ratios(nww_handle* h, const int32_t* num, const int32_t* den, int32_t K) {
    if (!h) return NWW_ERR_INVALID;
    if (!h->finalized) return fail(h, NWW_ERR_STATE, "model not finalized: call nww_finalize after loading the state_dict");
    if (K < 0 || K > RESAMPLE_MAX_RATIOS)
        return fail(h, NWW_ERR_INVALID, "the number of resample ratios must lie in [0, %d] (got %d)", RESAMPLE_MAX_RATIOS, K);
    if (K > 0 && (!num || !den)) return fail(h, NWW_ERR_INVALID, "null ratio table");
    const int32_t bad = resample_first_bad_ratio(num, den, K);
    if (bad >= 0)
        return fail(h, NWW_ERR_INVALID, "resample ratio %d: %d / %d out of range (terms in [1, %d], 1/4 <= num / den <= 12)", bad, num[bad], den[bad],
                    RESAMPLE_MAX_TERM);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->resample) h->resample = new ResampleState();
    ResampleState* m = h->resample;
    // everything new is built and uploaded before anything of the handle's is replaced
    std::vector<ResampleRatio> ratios((size_t)K);
    std::vector<float> taps;
    int span = 0;
    for (int32_t k = 0; k < K; ++k) {
        ratios[(size_t)k] = resample_ratio(num[k], den[k], (int32_t)taps.size());
        taps.resize(taps.size() + (size_t)den[k] * (size_t)ratios[(size_t)k].taps);
        resample_table(num[k], den[k], taps.data() + ratios[(size_t)k].off);
        span = ratios[(size_t)k].span > span ? ratios[(size_t)k].span : span;
    }
    ResampleRatio* d_ratios = nullptr;
    float* d_taps = nullptr;
    hipError_t e = hipSuccess;
    if (K > 0) {
        e = hipMalloc(reinterpret_cast<void**>(&d_ratios), ratios.size() * sizeof(ResampleRatio));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_taps), taps.size() * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(d_ratios, ratios.data(), ratios.size() * sizeof(ResampleRatio), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();                   // no call in flight reads the tables that go
    if (e != hipSuccess) {
        if (d_ratios) (void)hipFree(d_ratios);
        if (d_taps) (void)hipFree(d_taps);
        return fail(h, NWW_ERR_HIP, "resample table upload failed: %s", hipGetErrorString(e));
    }
    if (m->d_ratios) (void)hipFree(m->d_ratios);
    if (m->d_taps) (void)hipFree(m->d_taps);
    m->d_ratios = d_ratios; m->d_taps = d_taps; m->n_ratios = K; m->span_floats = span;
    for (int32_t k = 0; k < K; ++k) { m->num[k] = num[k]; m->den[k] = den[k]; }
    return NWW_OK;
}

// what both entry points check before anything is enqueued; *done: B == 0, the call is complete.  *tiles: the table's tiles.
static int resample_check(nww_handle* h, const void* src, int64_t src_values, int32_t src_format, const nww_resample_item* items, int32_t B,
                          const void* dst, int64_t dst_values, int32_t dst_format, bool* done, unsigned* tiles) {
    *done = false;
    if (!h) return NWW_ERR_INVALID;
    if (!h->finalized) return fail(h, NWW_ERR_STATE, "model not finalized: call nww_finalize after loading the state_dict");
    if (B < 0) return fail(h, NWW_ERR_INVALID, "batch must not be negative (got %d)", B);
    if (B == 0) { *done = true; return NWW_OK; }
    if (!resample_format_ok(src_format)) return fail(h, NWW_ERR_INVALID, "src_format %d is neither NWW_PCM_S16 nor NWW_PCM_F32", src_format);
    if (!resample_format_ok(dst_format)) return fail(h, NWW_ERR_INVALID, "dst_format %d is neither NWW_PCM_S16 nor NWW_PCM_F32", dst_format);
    if (!src || src_values < 1 || !dst || dst_values < 1 || !items) return fail(h, NWW_ERR_INVALID, "null or empty source or destination, or null item table");
    const ResampleState* m = h->resample;
    const int K = m ? m->n_ratios : 0;
    if (K < 1)
        for (int32_t i = 0; i < B; ++i)
            if (items[i].rate_id >= 0) return fail(h, NWW_ERR_INVALID, "no resample ratios set: call nww_resample_set_ratios first (item %d names one)", i);
    const char* field = nullptr;
    const int64_t bad = resample_first_bad_item(items, B, src_values, dst_values, m ? m->num : nullptr, m ? m->den : nullptr, K, &field);
    if (bad >= 0)
        return fail(h, NWW_ERR_INVALID, "resample item %lld: %s out of range (source of %lld values, destination of %lld, %d ratios)", (long long)bad,
                    field, (long long)src_values, (long long)dst_values, K);
    int64_t total = 0;
    for (int32_t i = 0; i < B; ++i) total += resample_tiles(resample_item_length(items[i], m ? m->num : nullptr, m ? m->den : nullptr));
    if (total > 0x7fffffffLL) return fail(h, NWW_ERR_INVALID, "the table's %lld tiles of %d outputs exceed one launch: split it", (long long)total, RESAMPLE_TILE);
    *tiles = (unsigned)total;
    return NWW_OK;
}

// the validated table through the next slot, then the kernel, on s
static int resample_enqueue(nww_handle* h, const void* d_src, int32_t src_format, const nww_resample_item* items, int B, unsigned tiles, void* d_dst,
                            int32_t dst_format, hipStream_t s) {
    if (!h->resample) h->resample = new ResampleState();
    int rc = resample_slots(h, (size_t)B);
    if (rc) return rc;
    ResampleState* m = h->resample;
    const unsigned slot = m->seq % POOL_TAB_SLOTS;
    if (m->seq >= POOL_TAB_SLOTS) HIP_TRY(h, hipEventSynchronize(m->ev[slot]));      // the slot's previous call has passed
    ++m->seq;
    nww_resample_item* pin = m->pin_tab + slot * m->slot_items;
    nww_resample_item* dev = m->d_tab + slot * m->slot_items;
    uint32_t first = 0;                                                // as uploaded, `reserved` carries the item's first tile
    for (int i = 0; i < B; ++i) {
        pin[i] = items[i];
        pin[i].reserved = first;
        first += (uint32_t)resample_tiles(resample_item_length(items[i], m->num, m->den));
    }
    HIP_TRY(h, hipMemcpyAsync(dev, pin, (size_t)B * sizeof(nww_resample_item), hipMemcpyHostToDevice, s));
    const hipError_t e = resample_launch(d_src, src_format, dev, B, tiles, m->d_ratios, m->d_taps, m->span_floats, d_dst, dst_format, s);
    (void)hipEventRecord(m->ev[slot], s);
    if (e != hipSuccess) return fail(h, NWW_ERR_HIP, "launch 'resample' failed: %s", hipGetErrorString(e));
    return NWW_OK;
}

extern "C" int nww_resample_dev(nww_handle* h, const void* d_src, int64_t src_values, int32_t src_format, const nww_resample_item* items, int32_t B,
                                void* d_dst, int64_t dst_values, int32_t dst_format, void* stream) {
    bool done = false;
    unsigned tiles = 0;
    const int rc = resample_check(h, d_src, src_values, src_format, items, B, d_dst, dst_values, dst_format, &done, &tiles);
    if (rc || done) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return resample_enqueue(h, d_src, src_format, items, B, tiles, d_dst, dst_format, stream ? (hipStream_t)stream : h->own_stream);
}

extern "C" int nww_resample(nww_handle* h, const void* src, int64_t src_values, int32_t src_format, const nww_resample_item* items, int32_t B, void* dst,
                            int64_t dst_values, int32_t dst_format) {
    bool done = false;
    unsigned tiles = 0;
    int rc = resample_check(h, src, src_values, src_format, items, B, dst, dst_values, dst_format, &done, &tiles);
    if (rc || done) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->resample) h->resample = new ResampleState();
    ResampleState* m = h->resample;
    const size_t sv = src_format == NWW_PCM_F32 ? 4 : 2, dv = dst_format == NWW_PCM_F32 ? 4 : 2;
    rc = nww_grow(h, &m->d_src, &m->src_bytes, (size_t)src_values * sv);
    if (!rc) rc = nww_grow(h, &m->d_dst, &m->dst_bytes, (size_t)dst_values * dv);
    if (rc) return rc;
    hipStream_t s = h->own_stream;
    HIP_TRY(h, hipMemcpyAsync(m->d_src, src, (size_t)src_values * sv, hipMemcpyHostToDevice, s));
    rc = resample_enqueue(h, m->d_src, src_format, items, B, tiles, m->d_dst, dst_format, s);
    if (rc) return rc;
    // the items' ranges ascend: one copy per run of ranges that touch
    int64_t lo = items[0].dst_off, hi = lo;
    for (int32_t i = 0; i <= B; ++i) {
        if (i < B && items[i].dst_off == hi) { hi += resample_item_length(items[i], m->num, m->den); continue; }
        HIP_TRY(h, hipMemcpyAsync(static_cast<unsigned char*>(dst) + (size_t)lo * dv, static_cast<unsigned char*>(m->d_dst) + (size_t)lo * dv,
                                  (size_t)(hi - lo) * dv, hipMemcpyDeviceToHost, s));
        if (i < B) { lo = items[i].dst_off; hi = lo + resample_item_length(items[i], m->num, m->den); }
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return NWW_OK;
}
