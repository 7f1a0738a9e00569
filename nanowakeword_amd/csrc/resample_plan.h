// resample_plan.h - the arithmetic of a recording brought to the target rate (include/nww.h, nww_resample_*) as the
// kernels of resample.hip and the CPU check tests/hostemu/resample_check.cpp both run it.  Restated in numpy by tests/resample_oracle.py.
// A recording has L frames of C interleaved channels; the ratio p / q is source rate over target rate, both divided by their gcd.
//  1  Downmix: m[k] = (0.0f + c_0[k] + .. + c_{C-1}[k]) / (float)C, channels in ascending order, ONE correctly rounded division; C = 1
//     is the sample itself.  An int16 sample is the float of its value.
//  2  Resample: M = ceil(L q / p) outputs; output n reads m[k0 + j], j < taps, k0 = floor(n p / q) + j0 = (n div q) p + ((n mod q) p) div
//     q + j0, against row n mod q of the ratio's table: v = 0.0f + the products m[k0 + j] g[phase][j] in ascending j, taps with k0 + j
//     outside [0, L) left out.  W = ceil(6 / c) with c = 0.99 min(1, q / p) - in integers, ceil(200 p / (33 q)) for p > q and 7 otherwise -
//     j0 = 1 - W, taps = 2 W.  g[phase][j] = c sinc(c x) cos^2(pi c x / 12) where |c x| < 6, an exact 0 elsewhere, x = frac - (j0 + j),
//     frac = ((phase p) mod q) / q: made in float64 and rounded once (resample_table).
//  3  Out: float32 is v 2^-15 from an int16 source (exact) and v from a float32 one; int16 is (int16) rint(clamp(u, -32768, 32767)),
//     nearest even, u = v from an int16 source and v 32768 from a float32 one (a NaN comes out as -32768).
// A row with rate_id == -1 is steps 1 and 3 alone.  The kernels walk an item in tiles of RESAMPLE_TILE outputs; a tile's first output
// is divided by q once (resample_tile_base) and every output of the tile is placed from there in 32-bit arithmetic (resample_place) -
// the walk below does the same, the restatement takes n p / q as it stands.
// Every float32 product and sum is rounded on its own (MIX_NO_CONTRACT; a g++ build passes -ffp-contract=off).
#pragma once
#include <vector>

#include "mix_plan.h"

#define RESAMPLE_TILE 1024             // outputs a workgroup produces per tile
#define RESAMPLE_MAX_TERM 1024
#define RESAMPLE_MAX_RATIOS 16
#define RESAMPLE_MAX_TAPS 146          // at 12 / 1
#define RESAMPLE_MAX_FRAMES (1 << 30)
#define RESAMPLE_MAX_CHANNELS 8

// 1 / 4 <= p / q <= 12, in integers
MIX_HD bool resample_ratio_ok(int32_t p, int32_t q) {
    if (p < 1 || q < 1 || p > RESAMPLE_MAX_TERM || q > RESAMPLE_MAX_TERM) return false;
    return q <= 4 * p && p <= 12 * q;
}
// W = ceil(6 / c): 6 / c = 200 p / (33 q) exactly where p > q
MIX_HD int32_t resample_half_width(int32_t p, int32_t q) { return p > q ? (200 * p + 33 * q - 1) / (33 * q) : 7; }
MIX_HD int32_t resample_taps(int32_t p, int32_t q) { return 2 * resample_half_width(p, q); }
MIX_HD int32_t resample_j0(int32_t p, int32_t q) { return 1 - resample_half_width(p, q); }
MIX_HD int64_t resample_length(int64_t L, int32_t p, int32_t q) { return (L * q + p - 1) / p; }
// the tiles of an item of M outputs
MIX_HD int64_t resample_tiles(int64_t M) { return (M + RESAMPLE_TILE - 1) / RESAMPLE_TILE; }
// the source frames under the outputs of one tile, first tap of the first to last tap of the last: floor(n p / q) moves by at most
// ceil((RESAMPLE_TILE - 1) p / q) over it
MIX_HD int32_t resample_span(int32_t p, int32_t q) { return ((RESAMPLE_TILE - 1) * p + q - 1) / q + resample_taps(p, q); }
// where a tile's first output n0 lies: base = (n0 div q) p - at most L, so 32 bits hold it - and r0 = n0 mod q
MIX_HD void resample_tile_base(int64_t n0, int32_t p, int32_t q, int32_t& base, int32_t& r0) {
    const int64_t mq = n0 / q;
    r0 = (int32_t)(n0 - mq * q);
    base = (int32_t)(mq * p);
}
// output n0 + d, d < RESAMPLE_TILE: its phase, and the frame under its first tap
MIX_HD void resample_place(int32_t base, int32_t r0, int32_t d, int32_t p, int32_t q, int32_t j0, int32_t& phase, int32_t& k0) {
    const int32_t r = r0 + d, mq = r / q;
    phase = r - mq * q;
    k0 = base + mq * p + (phase * p) / q + j0;
}

template <typename S> MIX_HD float resample_downmix(const S* frame, int32_t C) {
    MIX_NO_CONTRACT
    if (C == 1) return (float)frame[0];
    float a = 0.0f;
    for (int32_t c = 0; c < C; ++c) a = a + (float)frame[c];
    return a / (float)C;
}
MIX_HD float resample_tap(float acc, float m, float g) { MIX_NO_CONTRACT const float x = m * g; return acc + x; }
template <bool SRC_F32> MIX_HD float resample_out_f32(float v) { MIX_NO_CONTRACT return SRC_F32 ? v : v * 3.0517578125e-05f; }
template <bool SRC_F32> MIX_HD int16_t resample_out_s16(float v) {
    MIX_NO_CONTRACT
    float u = SRC_F32 ? v * 32768.0f : v;
    u = u > -32768.0f ? u : -32768.0f;                                 // a NaN takes this branch
    u = u < 32767.0f ? u : 32767.0f;
    return (int16_t)(int)rintf(u);
}
template <bool SRC_F32> MIX_HD void resample_store(float v, float* o) { *o = resample_out_f32<SRC_F32>(v); }
template <bool SRC_F32> MIX_HD void resample_store(float v, int16_t* o) { *o = resample_out_s16<SRC_F32>(v); }

// ---- host only
// a ratio as the kernels read it: the terms, the table's shape and where its q * taps floats start in the taps buffer
struct ResampleRatio { int32_t p, q, taps, j0, off, span, pad0, pad1; };

inline ResampleRatio resample_ratio(int32_t p, int32_t q, int32_t off) {
    return {p, q, resample_taps(p, q), resample_j0(p, q), off, resample_span(p, q), 0, 0};
}
// g [q][taps] of ratio p / q
inline void resample_table(int32_t p, int32_t q, float* g) {
    const double pi = 3.14159265358979323846;
    const double c = 0.99 * (q < p ? (double)q / (double)p : 1.0);
    const int32_t taps = resample_taps(p, q), j0 = resample_j0(p, q);
    for (int32_t ph = 0; ph < q; ++ph) {
        const double frac = (double)(((int64_t)ph * p) % q) / (double)q;
        for (int32_t j = 0; j < taps; ++j) {
            const double x = frac - (double)(j0 + j), cx = c * x;
            double v = 0.0;
            if (std::fabs(cx) < 6.0) {
                const double sinc = cx == 0.0 ? 1.0 : std::sin(pi * cx) / (pi * cx), h = std::cos(pi * cx / 12.0);
                v = c * sinc * h * h;
            }
            g[(size_t)ph * taps + j] = (float)v;
        }
    }
}
inline int32_t resample_first_bad_ratio(const int32_t* num, const int32_t* den, int32_t K) {
    for (int32_t k = 0; k < K; ++k)
        if (!resample_ratio_ok(num[k], den[k])) return k;
    return -1;
}
// an item's outputs against the ratios (num / den, K of them); the item has passed its own checks
inline int64_t resample_item_length(const nww_resample_item& it, const int32_t* num, const int32_t* den) {
    return it.rate_id < 0 ? (int64_t)it.src_frames : resample_length(it.src_frames, num[it.rate_id], den[it.rate_id]);
}
// the field of `it` that breaks a rule of include/nww.h, or null; dst_floor is where the item before it ends
inline const char* resample_item_bad_field(const nww_resample_item& it, int64_t src_values, int64_t dst_values, const int32_t* num,
                                           const int32_t* den, int32_t K, int64_t dst_floor) {
    if (it.src_frames < 1 || it.src_frames > RESAMPLE_MAX_FRAMES) return "src_frames";
    if (it.channels < 1 || it.channels > RESAMPLE_MAX_CHANNELS) return "channels";
    if (it.src_off < 0 || it.src_off > src_values - (int64_t)it.src_frames * it.channels) return "src_off";
    if (it.rate_id < -1 || it.rate_id >= K) return "rate_id";
    if (it.reserved != 0) return "reserved";
    if (it.dst_off < dst_floor || it.dst_off > dst_values - resample_item_length(it, num, den)) return "dst_off";
    return nullptr;
}
// the first bad item of a table: its index (and *field), or -1
inline int64_t resample_first_bad_item(const nww_resample_item* items, int64_t B, int64_t src_values, int64_t dst_values, const int32_t* num,
                                       const int32_t* den, int32_t K, const char** field) {
    int64_t floor_ = 0;
    for (int64_t i = 0; i < B; ++i) {
        const char* f = resample_item_bad_field(items[i], src_values, dst_values, num, den, K, floor_);
        if (f) { *field = f; return i; }
        floor_ = items[i].dst_off + resample_item_length(items[i], num, den);
    }
    return -1;
}
inline bool resample_format_ok(int32_t f) { return f == NWW_PCM_S16 || f == NWW_PCM_F32; }

// One item on the host, tile by tile as resample_kernel runs it (the CPU check's reference; the library never calls it): src is the
// item's first value, dst its first output.  g is the ratio's table (unread where r is null: a row with rate_id == -1).
template <typename S, typename D> inline void resample_item_host(const S* src, int32_t L, int32_t C, const ResampleRatio* r, const float* g, D* dst) {
    constexpr bool SRC_F32 = sizeof(S) == 4;
    if (!r) {
        for (int32_t k = 0; k < L; ++k) resample_store<SRC_F32>(resample_downmix(src + (size_t)k * C, C), dst + k);
        return;
    }
    const int64_t M = resample_length(L, r->p, r->q);
    for (int64_t n0 = 0; n0 < M; n0 += RESAMPLE_TILE) {
        int32_t base, r0;
        resample_tile_base(n0, r->p, r->q, base, r0);
        for (int32_t d = 0; d < RESAMPLE_TILE && n0 + d < M; ++d) {
            int32_t ph, k0;
            resample_place(base, r0, d, r->p, r->q, r->j0, ph, k0);
            float acc = 0.0f;
            for (int32_t j = 0; j < r->taps; ++j)
                if (k0 + j >= 0 && k0 + j < L) acc = resample_tap(acc, resample_downmix(src + (size_t)(k0 + j) * C, C), g[(size_t)ph * r->taps + j]);
            resample_store<SRC_F32>(acc, dst + n0 + d);
        }
    }
}
