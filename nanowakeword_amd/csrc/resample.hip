// resample.hip - recordings brought to the target rate on the device (include/nww.h, nww_resample_*): one kernel, a
// workgroup of 256 threads per TILE of RESAMPLE_TILE outputs, the tiles counted over ALL items of the table - 4 096 clips of a second
// and three recordings of ten minutes fill the chip alike.  A workgroup finds its item by bisection over the first tiles the host wrote
// into the table (uniform loads), then
//   stages the source frames under its tile once into LDS, downmixed to float32: at most ceil(1023 p / q) + taps of them, zeros outside
//   the recording (a product with an exact zero leaves the sum's bits alone - the sum starts at +0 and can never turn -0 - so the taps
//   the definition leaves out need no branch);
//   walks the taps in ascending j, a thread per output and four outputs a thread, against the phase's row of the ratio's table.
// Neighbouring lanes read LDS about p / q floats apart.  ds_read_b32 has 32 banks per half-wave: an odd or fractional stride spreads a
// half-wave over the banks, but an even integer stride (32 k -> 16 k: 2) puts lanes l and l + 16 on one bank.  For those ratios alone
// (PAD) element e is kept at e + (e >> 5), which moves every run of 32 floats up by one bank and makes strides 2 and 4 conflict-free;
// it costs three address instructions a tap, so every other ratio keeps the linear layout, whose tap offsets are immediates.
// A ratio with q == 1 has one row for every output (ONE_ROW): the row's address is uniform and the taps come as scalar loads; otherwise
// a lane reads its phase's row from L2 (q taps floats, at most 57 KB a ratio).
// A row with rate_id == -1 is downmixed and converted straight from memory.  Everything is resample_plan.h's arithmetic, shared with
// the CPU check; an output's bits depend on its item and its ratio alone.  No reductions, no atomics.
#include "resample.h"
#include "resample_plan.h"

namespace {

constexpr int RS_THREADS = 256;

template <bool PAD> __device__ inline int lds_at(int e) { return PAD ? e + (e >> 5) : e; }
inline int lds_floats(int span) { return span + (span >> 5) + 1; }    // lds_at<true>(span - 1) < lds_floats(span)

// one tile of a resampled item: the span into LDS, then the outputs.  Q1: r.q == 1, passed on as a literal.
template <bool PAD, bool ONE_ROW, typename S, typename D>
__device__ inline void tile(float* span, const S* __restrict__ s, int32_t L, int32_t C, const ResampleRatio& r, const float* __restrict__ g, int64_t n0,
                            int32_t count, D* __restrict__ o) {
    constexpr bool SRC_F32 = sizeof(S) == 4;
    const int tid = (int)threadIdx.x;
    const int32_t q = ONE_ROW ? 1 : r.q;
    int32_t base, r0, ph, k_lo, k_end;
    resample_tile_base(n0, r.p, q, base, r0);
    resample_place(base, r0, 0, r.p, q, r.j0, ph, k_lo);
    resample_place(base, r0, count - 1, r.p, q, r.j0, ph, k_end);
    const int32_t need = k_end + r.taps - k_lo;                        // <= r.span (resample_plan.h)
    for (int32_t e = tid; e < need; e += RS_THREADS) {
        const int32_t k = k_lo + e;
        span[lds_at<PAD>(e)] = k >= 0 && k < L ? resample_downmix(s + (size_t)k * C, C) : 0.0f;
    }
    __syncthreads();
    for (int32_t d = tid; d < count; d += RS_THREADS) {
        int32_t k0;
        resample_place(base, r0, d, r.p, q, r.j0, ph, k0);
        const float* row = ONE_ROW ? g : g + ph * r.taps;
        const int32_t at = k0 - k_lo;
        float acc = 0.0f;
        for (int32_t j = 0; j < r.taps; ++j) acc = resample_tap(acc, span[lds_at<PAD>(at + j)], row[j]);
        resample_store<SRC_F32>(acc, o + d);
    }
}

template <typename S, typename D>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const S* __restrict__ src, const nww_resample_item* __restrict__ tab, int B,
                                                              const ResampleRatio* __restrict__ ratios, const float* __restrict__ taps,
                                                              D* __restrict__ dst) {
    extern __shared__ float span[];
    constexpr bool SRC_F32 = sizeof(S) == 4;
    const unsigned t = blockIdx.x;
    const int tid = (int)threadIdx.x;
    int lo = 0, hi = B - 1;                                            // the last item whose first tile is <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].reserved <= t) lo = mid; else hi = mid - 1;
    }
    const nww_resample_item it = tab[lo];
    const int64_t n0 = (int64_t)(t - it.reserved) * RESAMPLE_TILE;
    const S* s = src + it.src_off;
    D* o = dst + it.dst_off + n0;
    const int32_t L = it.src_frames, C = it.channels;
    if (it.rate_id < 0) {
        const int32_t count = L - n0 < RESAMPLE_TILE ? (int32_t)(L - n0) : RESAMPLE_TILE;
        for (int32_t d = tid; d < count; d += RS_THREADS) resample_store<SRC_F32>(resample_downmix(s + (size_t)(n0 + d) * C, C), o + d);
        return;
    }
    const ResampleRatio r = ratios[it.rate_id];
    const float* g = taps + r.off;
    const int64_t M = resample_length(L, r.p, r.q);
    const int32_t count = M - n0 < RESAMPLE_TILE ? (int32_t)(M - n0) : RESAMPLE_TILE;
    // the same in every lane of the workgroup
    if (r.q != 1) tile<false, false>(span, s, L, C, r, g, n0, count, o);
    else if (r.p & 1) tile<false, true>(span, s, L, C, r, g, n0, count, o);
    else tile<true, true>(span, s, L, C, r, g, n0, count, o);
}

template <typename S, typename D>
void launch(const void* d_src, const nww_resample_item* d_tab, int B, unsigned tiles, const ResampleRatio* d_ratios, const float* d_taps, size_t lds,
            void* d_dst, hipStream_t stream) {
    hipLaunchKernelGGL((resample_kernel<S, D>), dim3(tiles), dim3(RS_THREADS), lds, stream, static_cast<const S*>(d_src), d_tab, B, d_ratios, d_taps,
                       static_cast<D*>(d_dst));
}

}  // namespace

hipError_t resample_launch(const void* d_src, int src_format, const nww_resample_item* d_tab, int B, unsigned tiles, const ResampleRatio* d_ratios,
                           const float* d_taps, int span_floats, void* d_dst, int dst_format, hipStream_t stream) {
    if (B <= 0 || tiles == 0) return hipSuccess;
    if (!resample_format_ok(src_format) || !resample_format_ok(dst_format) || span_floats < 0) return hipErrorInvalidValue;
    const size_t lds = ((size_t)lds_floats(span_floats)) * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const bool sf = src_format == NWW_PCM_F32, df = dst_format == NWW_PCM_F32;
    if (sf && df) launch<float, float>(d_src, d_tab, B, tiles, d_ratios, d_taps, lds, d_dst, stream);
    else if (sf) launch<float, int16_t>(d_src, d_tab, B, tiles, d_ratios, d_taps, lds, d_dst, stream);
    else if (df) launch<int16_t, float>(d_src, d_tab, B, tiles, d_ratios, d_taps, lds, d_dst, stream);
    else launch<int16_t, int16_t>(d_src, d_tab, B, tiles, d_ratios, d_taps, lds, d_dst, stream);
    return hipGetLastError();
}
