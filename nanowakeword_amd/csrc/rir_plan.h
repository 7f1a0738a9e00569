// rir_plan.h - the arithmetic of a clip convolved with a room impulse response (include/nww.h, nww_mix_rir_* / nww_rir_*; DESIGN.md
// 4.8h) as the kernels of rir.hip and the CPU check tests/hostemu/rir_check.cpp both run it.  Restated in numpy by tests/rir_oracle.py.
//
// A real sequence of M points (the clip's N samples, or a response's first min(L, N) taps, then zeros) is packed as H = M / 2 complex
// values z[n] = y[2n] + i y[2n + 1], H = 4^D.  The forward transform is an in-place decimation-in-frequency radix-4 network of D stages
// (spans H/4, H/16 .. 1) that leaves Z[k] at position rev(k), k's D base-4 digits reversed.  The real-input spectrum is recovered pair
// by pair (k, H - k) WHERE IT LIES, multiplied by the response's spectrum - stored in the same order - and packed again; the inverse
// is the decimation-in-time network (spans 1 .. H/4) that consumes that order and ends in natural order.  Nothing is ever reordered.
// Twiddles are ONE table per M, T[t] = (cos, sin)(2 pi t / M) for t < 3M/4, computed in float64 and rounded once; the forward half
// multiplies by conj(T), the inverse by T.  All scales are powers of two: the split leaves 2 X, the stored response spectrum is
// 2 X_h / (8H), and the unnormalised inverse then ends in w itself.
// Every float32 product and sum is rounded on its own (MIX_NO_CONTRACT); a complex multiply is four products and two sums.
#pragma once
#include <cstring>
#include <vector>

#include "mix_plan.h"

struct RirC { float re, im; };

#define RIR_M_MAX 32768

// the smallest instance with N + min(L, N) - 1 <= M, or 0
MIX_HD int32_t rir_fft_size(int32_t N, int32_t L) {
    if (N < 1 || L < 1) return 0;
    const int64_t need = (int64_t)N + (L < N ? L : N) - 1;
    return need <= 2048 ? 2048 : need <= 8192 ? 8192 : need <= RIR_M_MAX ? RIR_M_MAX : 0;
}
MIX_HD bool rir_is_size(int32_t M) { return M == 2048 || M == 8192 || M == RIR_M_MAX; }
// H = M / 2 = 4^D; 512 is the transform of pitch_plan.h's frames (no response is prepared at it: rir_is_size)
MIX_HD int rir_digits(int32_t M) { return M == 512 ? 4 : M == 2048 ? 5 : M == 8192 ? 6 : 7; }

// k's D base-4 digits reversed: its 2D bits reversed, then the two bits of every digit swapped back
MIX_HD uint32_t rir_rev(uint32_t k, int D) {
    uint32_t r = 0;
    for (int d = 0; d < D; ++d) { r = (r << 2) | (k & 3u); k >>= 2; }
    return r;
}

MIX_HD RirC rir_add(RirC a, RirC b) { MIX_NO_CONTRACT return {a.re + b.re, a.im + b.im}; }
MIX_HD RirC rir_sub(RirC a, RirC b) { MIX_NO_CONTRACT return {a.re - b.re, a.im - b.im}; }
MIX_HD RirC rir_conj(RirC a) { return {a.re, -a.im}; }
// a * w and a * conj(w)
MIX_HD RirC rir_mul(RirC a, RirC w) {
    MIX_NO_CONTRACT
    const float p0 = a.re * w.re, p1 = a.im * w.im, p2 = a.re * w.im, p3 = a.im * w.re;
    return {p0 - p1, p2 + p3};
}
MIX_HD RirC rir_mulc(RirC a, RirC w) {
    MIX_NO_CONTRACT
    const float p0 = a.re * w.re, p1 = a.im * w.im, p2 = a.re * w.im, p3 = a.im * w.re;
    return {p0 + p1, p3 - p2};
}

// one forward butterfly: a[m] at positions j + m * span of a group, w[m] = T[m * j * M / (4 span)]
MIX_HD void rir_bfly_fwd(RirC (&a)[4], RirC w1, RirC w2, RirC w3) {
    const RirC b0 = rir_add(a[0], a[2]), b1 = rir_sub(a[0], a[2]), b2 = rir_add(a[1], a[3]), b3 = rir_sub(a[1], a[3]);
    const RirC ib3 = {-b3.im, b3.re};                                  // i b3
    a[0] = rir_add(b0, b2);
    a[1] = rir_mulc(rir_sub(b1, ib3), w1);
    a[2] = rir_mulc(rir_sub(b0, b2), w2);
    a[3] = rir_mulc(rir_add(b1, ib3), w3);
}
// ... and the inverse one
MIX_HD void rir_bfly_inv(RirC (&a)[4], RirC w1, RirC w2, RirC w3) {
    const RirC a1 = rir_mul(a[1], w1), a2 = rir_mul(a[2], w2), a3 = rir_mul(a[3], w3);
    const RirC b0 = rir_add(a[0], a2), b1 = rir_sub(a[0], a2), b2 = rir_add(a1, a3), b3 = rir_sub(a1, a3);
    const RirC ib3 = {-b3.im, b3.re};
    a[0] = rir_add(b0, b2);
    a[1] = rir_add(b1, ib3);
    a[2] = rir_sub(b0, b2);
    a[3] = rir_sub(b1, ib3);
}

// The pair (k, H - k), 0 < k <= H / 2, of the packed transform: zk = Z[k], zm = Z[H - k], w = T[k] -> 2 X[k], 2 X[H - k]
MIX_HD void rir_split(RirC zk, RirC zm, RirC w, RirC& xk, RirC& xm) {
    const RirC a = rir_add(zk, rir_conj(zm)), b = rir_sub(zk, rir_conj(zm));
    const RirC t = rir_mulc(b, w);
    const RirC d = {t.im, -t.re};                                      // -i t
    xk = rir_add(a, d);
    xm = rir_conj(rir_sub(a, d));
}
// bin 0 holds the two real terms: (2 X[0], 2 X[H])
MIX_HD RirC rir_split0(RirC z0) { MIX_NO_CONTRACT const float s = z0.re + z0.im, d = z0.re - z0.im; return {s + s, d + d}; }

// a response's pair as it is stored: scaled by 1 / (8H)
MIX_HD void rir_spectrum_pair(RirC zk, RirC zm, RirC w, float scale, RirC& sk, RirC& sm) {
    MIX_NO_CONTRACT
    RirC xk, xm;
    rir_split(zk, zm, w, xk, xm);
    sk = {xk.re * scale, xk.im * scale};
    sm = {xm.re * scale, xm.im * scale};
}
MIX_HD RirC rir_spectrum0(RirC z0, float scale) { MIX_NO_CONTRACT const RirC x = rir_split0(z0); return {x.re * scale, x.im * scale}; }

// the split's way back: the spectrum's pair (yk, ym) at bins k, H - k packed for the inverse network, which then ends in 2H times the
// real sequence whose M-point transform the pairs are
MIX_HD void rir_unsplit(RirC yk, RirC ym, RirC w, RirC& zk, RirC& zm) {
    MIX_NO_CONTRACT
    const RirC a = rir_add(yk, rir_conj(ym)), b = rir_sub(yk, rir_conj(ym));
    const RirC o = rir_mul(b, w);
    zk = {a.re - o.im, a.im + o.re};
    zm = {a.re + o.im, o.re - a.im};
}
MIX_HD RirC rir_unsplit0(float y0, float yh) { MIX_NO_CONTRACT return {y0 + yh, y0 - yh}; }

// a clip's pair: split, times the response's (sk, sm), packed again for the inverse - in place of zk, zm
MIX_HD void rir_pair(RirC& zk, RirC& zm, RirC w, RirC sk, RirC sm) {
    MIX_NO_CONTRACT
    RirC xk, xm;
    rir_split(zk, zm, w, xk, xm);
    const RirC yk = rir_mul(xk, sk), ym = rir_mul(xm, sm);
    rir_unsplit(yk, ym, w, zk, zm);
}
MIX_HD RirC rir_pair0(RirC z0, RirC s0) {
    MIX_NO_CONTRACT
    const RirC x = rir_split0(z0);
    const float y0 = x.re * s0.re, yh = x.im * s0.im;
    return rir_unsplit0(y0, yh);
}

// The pair tasks of a transform: task u < H / 2 works on positions p = 4 (u / 2) + (u & 1) - those whose k = rev(p) lies below H / 2 -
// and pm = rev(H - k); task 0 is bin 0 and, besides, the self-paired k = H / 2 at position 2.
MIX_HD uint32_t rir_task_pos(uint32_t u) { return ((u >> 1) << 2) | (u & 1u); }

// ---- host only
inline int32_t rir_twiddle_count(int32_t M) { return M / 4 * 3; }
inline void rir_twiddles_host(int32_t M, RirC* T) {
    for (int32_t t = 0; t < rir_twiddle_count(M); ++t) {
        const double a = 2.0 * 3.14159265358979323846 * (double)t / (double)M;
        T[t] = {(float)std::cos(a), (float)std::sin(a)};
    }
}

inline void rir_forward_host(RirC* z, int32_t M, const RirC* T) {
    const int32_t H = M / 2;
    for (int32_t s = H / 4; s >= 1; s /= 4) {
        const int32_t tw = M / (4 * s);
        for (int32_t u = 0; u < H / 4; ++u) {
            const int32_t j = u % s, g = (u / s) * 4 * s + j;
            RirC a[4] = {z[g], z[g + s], z[g + 2 * s], z[g + 3 * s]};
            rir_bfly_fwd(a, T[j * tw], T[2 * j * tw], T[3 * j * tw]);
            for (int m = 0; m < 4; ++m) z[g + m * s] = a[m];
        }
    }
}
inline void rir_inverse_host(RirC* z, int32_t M, const RirC* T) {
    const int32_t H = M / 2;
    for (int32_t s = 1; s <= H / 4; s *= 4) {
        const int32_t tw = M / (4 * s);
        for (int32_t u = 0; u < H / 4; ++u) {
            const int32_t j = u % s, g = (u / s) * 4 * s + j;
            RirC a[4] = {z[g], z[g + s], z[g + 2 * s], z[g + 3 * s]};
            rir_bfly_inv(a, T[j * tw], T[2 * j * tw], T[3 * j * tw]);
            for (int m = 0; m < 4; ++m) z[g + m * s] = a[m];
        }
    }
}

// a response's spectrum [M / 2] as nww_rir_prepare_dev writes it: the first min(L, N) taps
inline void rir_prepare_host(const float* h, int32_t L, int32_t N, int32_t M, const RirC* T, RirC* spec) {
    const int32_t H = M / 2, D = rir_digits(M), n = L < N ? L : N;
    std::vector<float> y((size_t)M, 0.0f);
    for (int32_t i = 0; i < n; ++i) y[(size_t)i] = h[i];
    RirC* z = reinterpret_cast<RirC*>(y.data());
    rir_forward_host(z, M, T);
    const float scale = 1.0f / (float)(8 * H);
    for (int32_t u = 0; u < H / 2; ++u) {
        const uint32_t p = rir_task_pos((uint32_t)u), k = u ? rir_rev(p, D) : (uint32_t)(H / 2), pk = u ? p : 2u, pm = rir_rev((uint32_t)H - k, D);
        RirC sk, sm;
        rir_spectrum_pair(z[pk], z[pm], T[k], scale, sk, sm);
        spec[pm] = sm; spec[pk] = sk;
    }
    spec[0] = rir_spectrum0(z[0], scale);
}

// y [M] (the clip's float32 samples, zeros behind them) -> w in place, against a prepared spectrum
inline void rir_convolve_host(float* y, int32_t M, const RirC* T, const RirC* spec) {
    const int32_t H = M / 2, D = rir_digits(M);
    RirC* z = reinterpret_cast<RirC*>(y);
    rir_forward_host(z, M, T);
    for (int32_t u = 0; u < H / 2; ++u) {
        const uint32_t p = rir_task_pos((uint32_t)u), k = u ? rir_rev(p, D) : (uint32_t)(H / 2), pk = u ? p : 2u, pm = rir_rev((uint32_t)H - k, D);
        RirC zk = z[pk], zm = z[pm];
        rir_pair(zk, zm, T[k], spec[pk], spec[pm]);
        z[pm] = zm; z[pk] = zk;
    }
    z[0] = rir_pair0(z[0], spec[0]);
    rir_inverse_host(z, M, T);
}

// One clip on the host as rir_kernel runs it (the CPU check's reference; the library never calls it): mix_plan.h's y, the convolution
// (spec == null: none), the tail.  w [M] is scratch and holds w[0 .. N) afterwards.
inline void rir_clip_host(const int16_t* arena, const nww_mix_item& it, const RirC* spec, int32_t N, int32_t M, const RirC* T, float* w,
                          int16_t* out) {
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
    for (int32_t i = 0; i < M; ++i) {
        const bool in_fg = i >= ws && i < ws + it.fg_len;
        w[i] = i < N ? mix_y(in_fg ? fg[i - ws] : 0, real ? bgs(i) : 0, in_fg, real, s, it.gain) : 0.0f;
    }
    if (spec) rir_convolve_host(w, M, T, spec);
    float pk = 0.0f;
    if (it.flags & NWW_MIX_PEAK_NORMALISE)
        for (int32_t i = 0; i < N; ++i) pk = std::fmax(pk, std::fabs(w[i]));
    const float r = mix_ratio(it.level, it.flags, pk);
    for (int32_t i = 0; i < N; ++i) out[i] = mix_out(w[i], r);
}

// ---- the segmented route (NWW_RIR_SEGMENTED): uniformly partitioned overlap-save on the M = 32768 transform, for clips and responses
// of any length.  A response's first Le = min(L, N) taps are cut into P = ceil(Le / RIR_SEG_LP) partitions, each prepared as a response
// of a RIR_SEG_V-sample clip is; the clip into Q = ceil(N / RIR_SEG_V) segments.  Segment q is the sum over p <= min(P - 1, q), in that
// order, of the upper half of the window y[(q - p - 1) V .. (q - p + 1) V) (zeros outside the clip) convolved with partition p.
#define RIR_SEG_V 16384
#define RIR_SEG_LP 16384
MIX_HD int32_t rir_parts(int32_t N, int32_t L) {
    if (N < 1 || L < 1) return 0;
    const int32_t Le = L < N ? L : N;
    return (int32_t)(((int64_t)Le + RIR_SEG_LP - 1) / RIR_SEG_LP);
}
// partition p's term c joins a segment's sum: ((c_0 + c_1) + c_2) + ..
MIX_HD float rir_seg_acc(int p, float acc, float c) { MIX_NO_CONTRACT return p ? acc + c : c; }
MIX_HD int32_t rir_segments(int32_t N) { return N < 1 ? 0 : (int32_t)(((int64_t)N + RIR_SEG_V - 1) / RIR_SEG_V); }
// The segmented spectra buffer, in floats: a header of int32 bit patterns - [0] the partitions every response has room for (P of the
// longest), [1] K, [2 + k] response k's own P - padded to four, then [K][P_max][M / 2] complex values.
MIX_HD int64_t rir_seg_header_floats(int32_t K) { return ((int64_t)K + 2 + 3) & ~(int64_t)3; }
// the size of d_spectra for either route (M a transform size: K * M), or 0 for bad arguments
MIX_HD int64_t rir_spectra_floats(int32_t K, int32_t N, int32_t max_ir_len, int32_t M) {
    if (K < 1 || N < 1 || max_ir_len < 1) return 0;
    if (M == NWW_RIR_SEGMENTED) return rir_seg_header_floats(K) + (int64_t)K * rir_parts(N, max_ir_len) * RIR_M_MAX;
    return rir_is_size(M) ? (int64_t)K * M : 0;
}

// a response's partitions [P][M / 2], each as rir_prepare_host leaves a response of at most RIR_SEG_LP taps (host only)
inline void rir_seg_prepare_host(const float* h, int32_t L, int32_t N, const RirC* T, RirC* spec) {
    const int32_t Le = L < N ? L : N, P = rir_parts(N, L);
    for (int32_t p = 0; p < P; ++p) {
        const int32_t lo = p * RIR_SEG_LP, n = Le - lo < RIR_SEG_LP ? Le - lo : RIR_SEG_LP;
        rir_prepare_host(h + lo, n, RIR_SEG_V, RIR_M_MAX, T, spec + (size_t)p * (RIR_M_MAX / 2));
    }
}

// One clip on the host as rir_seg_kernel and rir_seg_tail_kernel run it (the CPU check's reference; the library never calls it):
// spec == null is the clip without a response.  w [N] holds the clip before the tail afterwards.
inline void rir_seg_clip_host(const int16_t* arena, const nww_mix_item& it, const RirC* spec, int32_t P, int32_t N, const RirC* T, float* w,
                              int16_t* out) {
    const int32_t M = RIR_M_MAX, V = RIR_SEG_V;
    const int16_t* fg = arena + it.fg_off;
    const int16_t* bg = it.bg_len > 0 ? arena + it.bg_off : nullptr;
    auto bgs = [&](int64_t i) -> int { return bg[(it.bg_start + i) % it.bg_len]; };
    bool real = false;
    float s = 0.0f;
    if (bg) {
        uint64_t Sf = 0, Sb = 0;
        int32_t Pk = 0;
        for (int32_t j = 0; j < it.fg_len; ++j) {
            const int64_t f = fg[j], b = bgs((int64_t)it.start + j);
            Sf += (uint64_t)(f * f); Sb += (uint64_t)(b * b);
        }
        for (int32_t i = 0; i < N; ++i) { const int32_t a = bgs(i) < 0 ? -bgs(i) : bgs(i); Pk = a > Pk ? a : Pk; }
        real = mix_real_background(it.bg_len, Pk);
        if (real) s = mix_scale(Sf, Sb, it.fg_len, it.snr_linear);
    }
    const int64_t ws = real ? it.start : 0;
    auto y_at = [&](int64_t i) -> float {
        if (i < 0 || i >= N) return 0.0f;
        const bool in_fg = i >= ws && i < ws + it.fg_len;
        return mix_y(in_fg ? fg[i - ws] : 0, real ? bgs(i) : 0, in_fg, real, s, it.gain);
    };
    if (!spec) {
        for (int32_t i = 0; i < N; ++i) w[i] = y_at(i);
    } else {
        std::vector<float> x((size_t)M);
        const int32_t Q = rir_segments(N);
        for (int32_t q = 0; q < Q; ++q) {
            const int32_t n = N - q * V < V ? N - q * V : V;
            for (int32_t p = 0; p < P && p <= q; ++p) {
                const int64_t a0 = (int64_t)(q - p - 1) * V;
                for (int32_t t = 0; t < M; ++t) x[(size_t)t] = y_at(a0 + t);
                rir_convolve_host(x.data(), M, T, spec + (size_t)p * (M / 2));
                for (int32_t r = 0; r < n; ++r) w[(size_t)q * V + r] = rir_seg_acc(p, w[(size_t)q * V + r], x[(size_t)(V + r)]);
            }
        }
    }
    uint32_t m = 0;                                                    // the peak as the kernels take it: the max of the bit patterns
    if (it.flags & NWW_MIX_PEAK_NORMALISE)
        for (int32_t i = 0; i < N; ++i) {
            uint32_t a;
            std::memcpy(&a, &w[i], 4);
            a &= 0x7fffffffu;
            m = a > m ? a : m;
        }
    float pk;
    std::memcpy(&pk, &m, 4);
    const float r = mix_ratio(it.level, it.flags, pk);
    for (int32_t i = 0; i < N; ++i) out[i] = mix_out(w[i], r);
}
// what nww_rir_prepare_dev refuses on the segmented route: a response without taps
inline int64_t rir_seg_first_bad_response(const int32_t* ir_len, int64_t K) {
    for (int64_t i = 0; i < K; ++i)
        if (ir_len[i] < 1) return i;
    return -1;
}

// what the calls check beyond mix_first_bad_item: every rir item against the number of responses, and M against N (rir_size_fits)
inline const char* rir_item_bad_field(const nww_rir_item& r, int32_t n_irs) {
    if (r.ir_id < -1 || r.ir_id >= n_irs) return "ir_id";
    if (r.reserved != 0) return "reserved";
    return nullptr;
}
inline int64_t rir_first_bad_item(const nww_rir_item* items, int64_t B, int32_t n_irs, const char** field) {
    for (int64_t i = 0; i < B; ++i) {
        const char* f = rir_item_bad_field(items[i], n_irs);
        if (f) { *field = f; return i; }
    }
    return -1;
}
inline bool rir_size_fits(int32_t M, int32_t N) { return rir_is_size(M) && N <= M; }
// the first response nww_rir_prepare_dev refuses: its index and *why ("ir_len", "overlap-save not built", "M"), or -1
inline int64_t rir_first_bad_response(const int32_t* ir_len, int64_t K, int32_t N, int32_t M, const char** why) {
    for (int64_t i = 0; i < K; ++i) {
        if (ir_len[i] < 1) { *why = "ir_len"; return i; }
        const int32_t need = rir_fft_size(N, ir_len[i]);
        if (need == 0) { *why = "overlap-save not built"; return i; }
        if (need > M) { *why = "M"; return i; }
    }
    return -1;
}
