// pitch_plan.h - the arithmetic of a clip shifted in pitch by a rational ratio p / q (include/nww.h, nww_pitch_* / nww_mix_aug_*;
// DESIGN.md 4.8i) as the kernels of pitch.hip and the CPU check tests/hostemu/pitch_check.cpp both run it.  Restated in numpy by
// tests/pitch_oracle.py.  The clip w[0 .. N) is mix_plan.h's y (float32, behind the gain); what comes out takes its place.
//
//  1  STFT: frame i is w at reflect(128 i + n - 256), n < 512, each sample times win[n] (ONE product); win is the periodic Hann window
//     made in float64 and rounded once (pitch_window_host).  The frame is transformed as rir_plan.h transforms a clip - 256 packed
//     complex values through the radix-4 network at four stages, twiddles from rir_twiddles_host(512) - and split pair by pair WHERE IT
//     LIES: position pos holds 2 X[rev(pos)], position 0 the two real bins (2 X[0], 2 X[256]).  Nothing is reordered: the vocoder
//     treats every bin alike, so it works on positions.
//  2  Vocoder, per position, frames in order (a recurrence, not a scan) - pitch_bin: unit(z) = z / sqrt(re re + im im), (1, 0) where
//     that sum is 0; alpha = (float)((t q) mod p) / (float)p, ONE correctly rounded division, 1 - alpha one subtraction; the magnitude
//     alpha |X1| + (1 - alpha) |X0| is two products and a sum; the frame is mag u; then u <- unit((u unit(X1)) conj(unit(X0))).
//     u_0 = unit(X[0]).  The two real bins of position 0 go through the same function as (x, 0).
//  3  ISTFT: the frame's pairs are packed again (rir_unsplit) and run through the inverse network, which ends in 1024 times the frame;
//     a sample is (v * 2^-10) * win[n] - an exact scaling and ONE product.  A sample of the stretched signal is the sum of the (up to
//     four) frames over it, 0.0f + o_a + o_b + .. in ascending frame order, DIVIDED (one correctly rounded division) by the envelope:
//     the float64 sum, in ascending frame order, of the squares of the float32 window values that were applied, rounded once
//     (pitch_env_host: a table over the sixteen sets of frames that can lie over a sample).
//  4  Resampler: PITCH_TAPS taps per output phase n mod q, stretched sample k = base + PITCH_TAP0 + j, base = (n div q) p + ((n mod q)
//     p) div q; the tap is g(frac - (PITCH_TAP0 + j)), frac = (((n mod q) p) mod q) / q, made in float64 and rounded once
//     (pitch_resample_table; exact zeros outside the window).  A sample is 0.0f plus the products s[k] g[j] in ascending j, taps with k
//     outside [0, S) left out.
// Every float32 product and sum is rounded on its own (MIX_NO_CONTRACT; a g++ build passes -ffp-contract=off), divisions and square
// roots are correctly rounded (hipcc's default), denormals are kept.
#pragma once
#include <vector>

#include "rir_plan.h"

#define PITCH_NFFT 512
#define PITCH_HOP 128
#define PITCH_H 256                    // packed complex values of a frame = 4^4
#define PITCH_TAPS 16
#define PITCH_TAP0 (-7)
#define PITCH_MAX_RATIOS 64
#define PITCH_MAX_TERM 256
#define PITCH_MIN_N 257
#define PITCH_MAX_N (1 << 28)          // keeps every index of a clip in int32

// 2^(-4/12) <= p / q <= 2^(4/12), in integers: p^3 <= 2 q^3 and q^3 <= 2 p^3
MIX_HD bool pitch_ratio_ok(int32_t p, int32_t q) {
    if (p < 1 || q < 1 || p > PITCH_MAX_TERM || q > PITCH_MAX_TERM) return false;
    const int64_t p3 = (int64_t)p * p * p, q3 = (int64_t)q * q * q;
    return p3 <= 2 * q3 && q3 <= 2 * p3;
}
MIX_HD int32_t pitch_frames(int32_t N) { return 1 + N / PITCH_HOP; }
MIX_HD int32_t pitch_out_frames(int32_t T, int32_t p, int32_t q) { return (int32_t)(((int64_t)T * p + q - 1) / q); }
MIX_HD int32_t pitch_stretched(int32_t T_out) { return PITCH_HOP * (T_out - 1); }
MIX_HD int32_t pitch_resampled(int32_t S, int32_t p, int32_t q) { return (int32_t)(((int64_t)S * q + p - 1) / p); }
// the stretched samples of the longest ratio the bounds allow, rounded up to whole frames: the row stride of the scratch
MIX_HD int32_t pitch_stride(int32_t N) { return PITCH_HOP * (int32_t)(((int64_t)pitch_frames(N) * 162 + 127) / 128); }   // 162 / 128 > 2^(1/3)
MIX_HD int32_t pitch_reflect(int32_t i, int32_t N) { return i < 0 ? -i : i >= N ? 2 * (N - 1) - i : i; }

// unit(z) and |z|
MIX_HD RirC pitch_polar(RirC z, float& mag) {
    MIX_NO_CONTRACT
    const float a = z.re * z.re, b = z.im * z.im, s = a + b;
    if (s == 0.0f) { mag = 0.0f; return {1.0f, 0.0f}; }
    const float r = sqrtf(s);
    mag = r;
    return {z.re / r, z.im / r};
}
MIX_HD RirC pitch_unit(RirC z) { float m; return pitch_polar(z, m); }
MIX_HD float pitch_alpha(int32_t m, int32_t p) { return (float)m / (float)p; }
// one bin of output frame t from the frames under it: the frame's value, and u advanced for the next
MIX_HD RirC pitch_bin(RirC x0, RirC x1, float alpha, RirC& u) {
    MIX_NO_CONTRACT
    float m0, m1;
    const RirC e0 = pitch_polar(x0, m0), e1 = pitch_polar(x1, m1);
    const float om = 1.0f - alpha;
    const float a = alpha * m1, b = om * m0, mag = a + b;
    const RirC y = {mag * u.re, mag * u.im};
    u = pitch_unit(rir_mulc(rir_mul(u, e1), e0));
    return y;
}
// position 0: the real bins 0 and 256 packed as (re, im), each with a u of its own
MIX_HD RirC pitch_bin0(RirC x0, RirC x1, float alpha, RirC& u, RirC& uh) {
    const RirC y0 = pitch_bin({x0.re, 0.0f}, {x1.re, 0.0f}, alpha, u), yh = pitch_bin({x0.im, 0.0f}, {x1.im, 0.0f}, alpha, uh);
    return {y0.re, yh.re};
}
MIX_HD float pitch_synth(float v, float win) { MIX_NO_CONTRACT const float x = v * 0.0009765625f; return x * win; }
MIX_HD float pitch_ola(float acc, float o) { MIX_NO_CONTRACT return acc + o; }
// the frames fl - c, c < 4, that exist among T_out: the envelope's row
MIX_HD int pitch_env_mask(int32_t fl, int32_t T_out) {
    int m = 0;
    for (int c = 0; c < 4; ++c)
        if (fl - c >= 0 && fl - c < T_out) m |= 1 << c;
    return m;
}
MIX_HD float pitch_tap(float acc, float s, float g) { MIX_NO_CONTRACT const float x = s * g; return acc + x; }
// output sample n of the resampler: its phase's row of the table and the stretched sample under its first tap
MIX_HD void pitch_phase(int32_t n, int32_t p, int32_t q, int32_t& phase, int32_t& k0) {
    const int32_t mq = n / q;
    phase = n - mq * q;
    k0 = mq * p + (phase * p) / q + PITCH_TAP0;
}

// ---- host only
inline void pitch_window_host(float* win) {
    for (int n = 0; n < PITCH_NFFT; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * (double)n / (double)PITCH_NFFT));
}
// env [16][128]: row = pitch_env_mask, column = the padded position modulo 128
inline void pitch_env_host(const float* win, float* env) {
    for (int m = 0; m < 16; ++m)
        for (int r = 0; r < PITCH_HOP; ++r) {
            double s = 0.0;
            for (int c = 3; c >= 0; --c)                               // ascending frames: fl - 3 first
                if (m >> c & 1) { const double v = (double)win[r + PITCH_HOP * c]; s += v * v; }
            env[m * PITCH_HOP + r] = (float)s;
        }
}
// g [q][PITCH_TAPS] of ratio p / q
inline void pitch_resample_table(int32_t p, int32_t q, float* g) {
    const double pi = 3.14159265358979323846;
    const double c = 0.99 * (q < p ? (double)q / (double)p : 1.0);
    for (int32_t ph = 0; ph < q; ++ph) {
        const double frac = (double)(((int64_t)ph * p) % q) / (double)q;
        for (int j = 0; j < PITCH_TAPS; ++j) {
            const double x = frac - (double)(PITCH_TAP0 + j), cx = c * x;
            double v = 0.0;
            if (std::fabs(cx) < 6.0) {
                const double sinc = cx == 0.0 ? 1.0 : std::sin(pi * cx) / (pi * cx), h = std::cos(pi * cx / 12.0);
                v = c * sinc * h * h;
            }
            g[(size_t)ph * PITCH_TAPS + j] = (float)v;
        }
    }
}

struct PitchTables {
    std::vector<RirC> T;               // rir_twiddles_host(512)
    std::vector<float> win, env;
    PitchTables() : T((size_t)rir_twiddle_count(PITCH_NFFT)), win(PITCH_NFFT), env(16 * PITCH_HOP) {
        rir_twiddles_host(PITCH_NFFT, T.data());
        pitch_window_host(win.data());
        pitch_env_host(win.data(), env.data());
    }
};

// frame i of the clip -> X [256] by position (zeros for i >= T)
inline void pitch_stft_frame_host(const float* w, int32_t N, int32_t i, const PitchTables& tb, RirC* X) {
    MIX_NO_CONTRACT
    float* f = reinterpret_cast<float*>(X);
    const int32_t T = pitch_frames(N);
    for (int n = 0; n < PITCH_NFFT; ++n) f[n] = i < T ? w[pitch_reflect(PITCH_HOP * i + n - PITCH_NFFT / 2, N)] * tb.win[n] : 0.0f;
    rir_forward_host(X, PITCH_NFFT, tb.T.data());
    const int D = rir_digits(PITCH_NFFT);
    for (int32_t u = 0; u < PITCH_H / 2; ++u) {
        const uint32_t pos = rir_task_pos((uint32_t)u), k = u ? rir_rev(pos, D) : (uint32_t)(PITCH_H / 2), pk = u ? pos : 2u,
                       pm = rir_rev((uint32_t)PITCH_H - k, D);
        RirC xk, xm;
        rir_split(X[pk], X[pm], tb.T[k], xk, xm);
        X[pm] = xm; X[pk] = xk;
    }
    X[0] = rir_split0(X[0]);
}
// an output frame's values by position (overwritten) -> its 512 windowed samples
inline void pitch_istft_frame_host(RirC* Y, const PitchTables& tb, float* o) {
    const int D = rir_digits(PITCH_NFFT);
    for (int32_t u = 0; u < PITCH_H / 2; ++u) {
        const uint32_t pos = rir_task_pos((uint32_t)u), k = u ? rir_rev(pos, D) : (uint32_t)(PITCH_H / 2), pk = u ? pos : 2u,
                       pm = rir_rev((uint32_t)PITCH_H - k, D);
        RirC zk, zm;
        rir_unsplit(Y[pk], Y[pm], tb.T[k], zk, zm);
        Y[pm] = zm; Y[pk] = zk;
    }
    Y[0] = rir_unsplit0(Y[0].re, Y[0].im);
    rir_inverse_host(Y, PITCH_NFFT, tb.T.data());
    const float* v = reinterpret_cast<const float*>(Y);
    for (int n = 0; n < PITCH_NFFT; ++n) o[n] = pitch_synth(v[n], tb.win[n]);
}

// stages 1 - 3 on the host as pitch_vocoder_kernel runs them: w [N] -> s [128 (T_out - 1)].  spec, if not null, receives the output
// frames by position [T_out][256] (the CPU check's rate-1 property).
inline void pitch_stretch_host(const float* w, int32_t N, int32_t p, int32_t q, const PitchTables& tb, float* s, RirC* spec = nullptr) {
    const int32_t T = pitch_frames(N), T_out = pitch_out_frames(T, p, q), S = pitch_stretched(T_out);
    std::vector<RirC> X((size_t)(T + 1) * PITCH_H), Y(PITCH_H), U(PITCH_H);
    for (int32_t i = 0; i <= T; ++i) pitch_stft_frame_host(w, N, i, tb, X.data() + (size_t)i * PITCH_H);
    std::vector<float> acc((size_t)PITCH_HOP * (T_out + 3), 0.0f), o(PITCH_NFFT);
    RirC uh = {1.0f, 0.0f};
    for (int32_t t = 0; t < T_out; ++t) {
        const int64_t tq = (int64_t)t * q;
        const int32_t i = (int32_t)(tq / p);
        const float alpha = pitch_alpha((int32_t)(tq % p), p);
        const RirC* X0 = X.data() + (size_t)i * PITCH_H;
        const RirC* X1 = X0 + PITCH_H;
        if (t == 0) {
            for (int pos = 1; pos < PITCH_H; ++pos) U[pos] = pitch_unit(X0[pos]);
            U[0] = pitch_unit({X0[0].re, 0.0f}); uh = pitch_unit({X0[0].im, 0.0f});
        }
        Y[0] = pitch_bin0(X0[0], X1[0], alpha, U[0], uh);
        for (int pos = 1; pos < PITCH_H; ++pos) Y[pos] = pitch_bin(X0[pos], X1[pos], alpha, U[pos]);
        if (spec) std::memcpy(spec + (size_t)t * PITCH_H, Y.data(), sizeof(RirC) * PITCH_H);
        pitch_istft_frame_host(Y.data(), tb, o.data());
        for (int n = 0; n < PITCH_NFFT; ++n) acc[(size_t)PITCH_HOP * t + n] = pitch_ola(acc[(size_t)PITCH_HOP * t + n], o[n]);
    }
    for (int32_t j = 0; j < S; ++j) {
        const int32_t P = j + PITCH_NFFT / 2;
        s[j] = acc[(size_t)P] / tb.env[(size_t)pitch_env_mask(P / PITCH_HOP, T_out) * PITCH_HOP + P % PITCH_HOP];
    }
}
// stage 4: s [S] -> y [N] against the ratio's table g
inline void pitch_resample_host(const float* s, int32_t S, int32_t p, int32_t q, const float* g, int32_t N, float* y) {
    const int32_t Ly = pitch_resampled(S, p, q);
    for (int32_t n = 0; n < N; ++n) {
        float acc = 0.0f;
        if (n < Ly) {
            int32_t ph, k0;
            pitch_phase(n, p, q, ph, k0);
            for (int j = 0; j < PITCH_TAPS; ++j)
                if (k0 + j >= 0 && k0 + j < S) acc = pitch_tap(acc, s[k0 + j], g[(size_t)ph * PITCH_TAPS + j]);
        }
        y[n] = acc;
    }
}
// One clip's w [N] shifted in place (the CPU check's reference; the library never calls it)
inline void pitch_clip_host(float* w, int32_t N, int32_t p, int32_t q, const PitchTables& tb) {
    const int32_t S = pitch_stretched(pitch_out_frames(pitch_frames(N), p, q));
    std::vector<float> s((size_t)S), g((size_t)q * PITCH_TAPS);
    pitch_stretch_host(w, N, p, q, tb, s.data());
    pitch_resample_table(p, q, g.data());
    pitch_resample_host(s.data(), S, p, q, g.data(), N, w);
}

// what the calls check beyond mix_first_bad_item and rir_first_bad_item
inline int32_t pitch_first_bad_ratio(const int32_t* num, const int32_t* den, int32_t K) {
    for (int32_t k = 0; k < K; ++k)
        if (!pitch_ratio_ok(num[k], den[k])) return k;
    return -1;
}
inline const char* pitch_item_bad_field(const nww_pitch_item& r, int32_t n_ratios) {
    if (r.pitch_id < -1 || r.pitch_id >= n_ratios) return "pitch_id";
    if (r.reserved != 0) return "reserved";
    return nullptr;
}
inline int64_t pitch_first_bad_item(const nww_pitch_item* items, int64_t B, int32_t n_ratios, const char** field) {
    for (int64_t i = 0; i < B; ++i) {
        const char* f = pitch_item_bad_field(items[i], n_ratios);
        if (f) { *field = f; return i; }
    }
    return -1;
}
inline bool pitch_length_ok(int32_t N) { return N >= PITCH_MIN_N && N <= PITCH_MAX_N; }
