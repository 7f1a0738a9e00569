// mix_plan.h - the arithmetic of a mixed clip (include/nww.h, nww_mix_*) as the kernel of mix.hip and the CPU check
// tests/hostemu/mix_check.cpp both run it: the scale from the exact integer statistics, the peak ratio, the per-sample formula, and
// (host only) the validation of an item.  Restated in numpy by tests/mix_oracle.py.
// Every float32 product and sum is rounded on its own: each function switches contraction off for its body (hipcc contracts device
// code by default); a g++ build passes -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/nww.h"

#if defined(__HIPCC__)
#define MIX_HD __host__ __device__ inline
#else
#define MIX_HD inline
#endif
#if defined(__clang__)
#define MIX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MIX_NO_CONTRACT
#endif

// the reference's has_real_background (augment_clips.py:218): peak > 1e-4, and 3 / 32768 < 1e-4 < 4 / 32768
MIX_HD bool mix_real_background(int32_t bg_len, int32_t P) { return bg_len > 0 && P >= 4; }

// _mix_snr's scale (augment_clips.py:58-74) in float64 from Sf = sum fg^2 and Sb = sum of the background's squares under the
// foreground, both over fg_len int16 samples; rounded to float32 once
MIX_HD float mix_scale(uint64_t Sf, uint64_t Sb, int32_t fg_len, float snr_linear) {
    MIX_NO_CONTRACT
    const double eps = 1.1920928955078125e-07;                 // 2^-23
    const double den = (double)fg_len * 1073741824.0;          // fg_len * 2^30: exact
    const double msf = (double)Sf / den, msb = (double)Sb / den;
    const double fr = sqrt(msf + eps);
    double br = sqrt(msb + eps);
    if (br < 0.005) br = 0.005;
    double scale = (double)snr_linear * br / fr;
    const double srms = sqrt(scale * scale * msf + eps);
    if (srms < 0.01) scale = scale * (0.01 / srms);
    return (float)scale;
}

// the factor behind the gain: level / peak with bit 0 (a silent clip's peak counts as 1, augment_clips.py:252), the level itself without
MIX_HD float mix_ratio(float level, uint32_t flags, float pk) {
    if (!(flags & NWW_MIX_PEAK_NORMALISE)) return level;
    if (pk < 1e-8f) pk = 1.0f;
    return level / pk;
}

// y of one clip sample: fg / bg are the int16 samples under it, in_fg whether it lies in the foreground's window ([start, start +
// fg_len) with a real background, [0, fg_len) without)
MIX_HD float mix_y(int fg, int bg, bool in_fg, bool real, float s, float gain) {
    MIX_NO_CONTRACT
    const float k = 1.0f / 32768.0f;
    const float f = (float)fg * k;
    float x;
    if (real) {
        const float b = (float)bg * k;
        const float fs = f * s;
        x = in_fg ? b + fs : b;
    } else {
        x = in_fg ? f : 0.0f;
    }
    return x * gain;
}

MIX_HD int16_t mix_out(float y, float r) {
    MIX_NO_CONTRACT
    float z = y * r;
    z = z < -1.0f ? -1.0f : z > 1.0f ? 1.0f : z;
    return (int16_t)(int)(z * 32767.0f);                       // toward zero, as astype(np.int16) (augment_clips.py:259)
}

// ---- host only
// the field of `it` that breaks a rule of include/nww.h, or null
inline const char* mix_item_bad_field(const nww_mix_item& it, int64_t arena_samples, int32_t N) {
    if (it.fg_len < 1 || it.fg_len > N) return "fg_len";
    if (it.fg_off < 0 || it.fg_off > arena_samples - it.fg_len) return "fg_off";
    if (it.bg_len < 0) return "bg_len";
    if (it.bg_len > 0) {
        if (it.bg_off < 0 || it.bg_off > arena_samples - it.bg_len) return "bg_off";
        if (it.bg_start < 0 || it.bg_start >= it.bg_len) return "bg_start";
    }
    if (it.start < 0 || it.start > N - it.fg_len) return "start";
    if (!(std::isfinite(it.snr_linear) && it.snr_linear > 0.0f)) return "snr_linear";
    if (!(std::isfinite(it.gain) && it.gain > 0.0f)) return "gain";
    if (!(std::isfinite(it.level) && it.level > 0.0f)) return "level";
    if (it.flags & ~NWW_MIX_PEAK_NORMALISE) return "flags";
    return nullptr;
}

// the first bad item of a table: its index (and *field), or -1
inline int64_t mix_first_bad_item(const nww_mix_item* items, int64_t B, int64_t arena_samples, int32_t N, const char** field) {
    for (int64_t i = 0; i < B; ++i) {
        const char* f = mix_item_bad_field(items[i], arena_samples, N);
        if (f) { *field = f; return i; }
    }
    return -1;
}

// One clip on the host, pass for pass as mix_kernel runs it (the CPU check's reference; the library never calls it).
inline void mix_clip_host(const int16_t* arena, const nww_mix_item& it, int32_t N, int16_t* out) {
    const int16_t* fg = arena + it.fg_off;
    const int16_t* bg = it.bg_len > 0 ? arena + it.bg_off : nullptr;
    auto bgs = [&](int64_t i) -> int { return bg[(it.bg_start + i) % it.bg_len]; };
    bool real = false;
    float s = 0.0f;
    if (bg) {
        uint64_t Sf = 0, Sb = 0;
        int32_t P = 0;
        for (int32_t j = 0; j < it.fg_len; ++j) {
            const int64_t f = fg[j], b = bgs((int64_t)it.start + j);
            Sf += (uint64_t)(f * f); Sb += (uint64_t)(b * b);
        }
        for (int32_t i = 0; i < N; ++i) { const int32_t a = bgs(i) < 0 ? -bgs(i) : bgs(i); P = a > P ? a : P; }
        real = mix_real_background(it.bg_len, P);
        if (real) s = mix_scale(Sf, Sb, it.fg_len, it.snr_linear);
    }
    const int64_t ws = real ? it.start : 0;
    auto y_at = [&](int32_t i) -> float {
        const bool in_fg = i >= ws && i < ws + it.fg_len;
        return mix_y(in_fg ? fg[i - ws] : 0, real ? bgs(i) : 0, in_fg, real, s, it.gain);
    };
    float pk = 0.0f;
    if (it.flags & NWW_MIX_PEAK_NORMALISE)
        for (int32_t i = 0; i < N; ++i) pk = std::fmax(pk, std::fabs(y_at(i)));
    const float r = mix_ratio(it.level, it.flags, pk);
    for (int32_t i = 0; i < N; ++i) out[i] = mix_out(y_at(i), r);
}
