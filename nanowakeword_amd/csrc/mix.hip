// mix.hip - clips mixed on the device (include/nww.h, nww_mix_*): one workgroup of 256 threads per clip, the clips
// of a call over the grid.  A clip is three passes over its N samples in chunks of 8, a thread per chunk:
//   1 (only with a background)   Sf, Sb as 64-bit integer sums and P as an integer max - then the scale, in float64, by every thread
//   2 (only with flags bit 0)    pk = max |y| as a max over the bit patterns of the non-negative floats
//   3                            y again from the sources, scaled, clamped, truncated, stored
// Passes 2 and 3 read the sources again - from L1 / L2, a clip's 2 fg_len + 2 N bytes having just been read by its own workgroup -
// so that N is not bounded by registers or LDS; the same loader and the same mix_plan.h functions give the same y both times.  Every
// reduction is an integer add or max: a clip's bits depend on nothing but its item.
// Sources and output are aligned to 2 bytes only and independently of each other, so a chunk's 8 samples are moved as one 16-byte
// access on a 2-byte-aligned type (gfx950 takes a global access at any alignment; aligned ones are the one-line case of the same
// instruction); a chunk that straddles the background's wrap, an edge of the foreground's window or the clip's end goes sample by
// sample, and so does every chunk of a source shorter than 8 samples.  Nothing outside [fg_off, fg_off + fg_len) and [bg_off, bg_off +
// bg_len) is read.
#include "mix.h"
#include "mix_plan.h"

namespace {

constexpr int MIX_THREADS = 256;

struct __attribute__((packed, aligned(2))) Pcm8 { int16_t v[8]; };

struct MixClip {                   // a clip's geometry, the same in every lane
    const int16_t* fg; const int16_t* bg;          // bg: null when the pass reads no background
    int fg_len, bg_len, bg_start;
    int ws;                        // the foreground's window starts here
};

// how a pass reads its sources: MIX_SLOW sample by sample (a source shorter than 8 samples); otherwise every source has 8 samples or more
// and is read by ONE unconditional 16-byte load at the chunk's place clamped into the source, both loads issued before either is used
// - a chunk is one trip to memory - and only a chunk that is not 8 whole samples of a source is read again sample by sample
enum { MIX_SLOW = 0, MIX_FG = 1, MIX_FG_BG = 2 };

// samples [i0, i0 + n) of the clip, 1 <= n <= 8: the background's (0 without one) and the foreground's (0 outside its window, whose
// samples the returned bits mark)
template <int MODE>
__device__ inline unsigned mix_load8(const MixClip& c, unsigned i0, int n, int (&bgv)[8], int (&fgv)[8]) {
    const bool has_bg = MODE == MIX_FG_BG || (MODE == MIX_SLOW && c.bg);
    unsigned p = 0;
    if (has_bg) p = ((unsigned)c.bg_start + i0) % (unsigned)c.bg_len;              // both below 2^31
    const long long j0 = (long long)i0 - c.ws;
    bool bg_whole = false, fg_whole = false;
    Pcm8 vb = {}, vf = {};
    if (MODE != MIX_SLOW) {
        fg_whole = n == 8 && j0 >= 0 && j0 + 8 <= c.fg_len;
        const long long qf = j0 < 0 ? 0 : j0 + 8 <= c.fg_len ? j0 : c.fg_len - 8;
        if (MODE == MIX_FG_BG) {
            bg_whole = n == 8 && p + 8u <= (unsigned)c.bg_len;
            const unsigned qb = p + 8u <= (unsigned)c.bg_len ? p : (unsigned)c.bg_len - 8u;
            vb = *reinterpret_cast<const Pcm8*>(c.bg + qb);
        }
        vf = *reinterpret_cast<const Pcm8*>(c.fg + qf);
    }
    if (has_bg && !bg_whole) {
        Pcm8 t = {};
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < n) { t.v[k] = c.bg[p]; if (++p == (unsigned)c.bg_len) p = 0; }
        vb = t;
    }
    unsigned in = 0xffu;
    if (!fg_whole) {
        Pcm8 t = {};
        in = 0;
        if (j0 + n > 0 && j0 < c.fg_len) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long long j = j0 + k;
                if (k < n && j >= 0 && j < c.fg_len) { t.v[k] = c.fg[j]; in |= 1u << k; }
            }
        }
        vf = t;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { bgv[k] = vb.v[k]; fgv[k] = vf.v[k]; }
    return in;
}

__device__ inline int mix_mode(const MixClip& c) { return c.fg_len < 8 || (c.bg && c.bg_len < 8) ? MIX_SLOW : c.bg ? MIX_FG_BG : MIX_FG; }

__device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline unsigned wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned w = (unsigned)__shfl_xor((int)v, o, 64); v = w > v ? w : v; }
    return v;
}

constexpr unsigned MIX_STEP = MIX_THREADS * 8;         // samples per trip of a workgroup

// pass 1: this thread's share of Sf, Sb and P
template <int MODE>
__device__ inline void mix_pass_stats(const MixClip& c, int N, unsigned long long& Sf, unsigned long long& Sb, unsigned& P) {
    int bgv[8], fgv[8];
    for (unsigned i0 = threadIdx.x * 8; i0 < (unsigned)N; i0 += MIX_STEP) {
        const int n = (unsigned)N - i0 < 8u ? (int)((unsigned)N - i0) : 8;
        const unsigned in = mix_load8<MODE>(c, i0, n, bgv, fgv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned a = (unsigned)(bgv[k] < 0 ? -bgv[k] : bgv[k]);
            P = a > P ? a : P;
            if (in >> k & 1) { Sf += (unsigned)(fgv[k] * fgv[k]); Sb += (unsigned)(bgv[k] * bgv[k]); }
        }
    }
}

// pass 2: this thread's share of max |y|, as the bits of a non-negative float
template <int MODE>
__device__ inline unsigned mix_pass_peak(const MixClip& c, int N, bool real, float s, float gain) {
    int bgv[8], fgv[8];
    unsigned m = 0;
    for (unsigned i0 = threadIdx.x * 8; i0 < (unsigned)N; i0 += MIX_STEP) {
        const int n = (unsigned)N - i0 < 8u ? (int)((unsigned)N - i0) : 8;
        const unsigned in = mix_load8<MODE>(c, i0, n, bgv, fgv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {                                  // the samples past n are zeros: |y| = 0
            const unsigned a = __float_as_uint(mix_y(fgv[k], bgv[k], in >> k & 1, real, s, gain)) & 0x7fffffffu;
            m = a > m ? a : m;
        }
    }
    return m;
}

// pass 3: the clip's samples
template <int MODE>
__device__ inline void mix_pass_store(const MixClip& c, int N, bool real, float s, float gain, float r, int16_t* __restrict__ o) {
    int bgv[8], fgv[8];
    for (unsigned i0 = threadIdx.x * 8; i0 < (unsigned)N; i0 += MIX_STEP) {
        const int n = (unsigned)N - i0 < 8u ? (int)((unsigned)N - i0) : 8;
        const unsigned in = mix_load8<MODE>(c, i0, n, bgv, fgv);
        Pcm8 v;
#pragma unroll
        for (int k = 0; k < 8; ++k) v.v[k] = mix_out(mix_y(fgv[k], bgv[k], in >> k & 1, real, s, gain), r);
        if (n == 8) *reinterpret_cast<Pcm8*>(o + i0) = v;
        else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < n) o[i0 + k] = v.v[k];
        }
    }
}

__global__ __launch_bounds__(MIX_THREADS) void mix_kernel(const int16_t* __restrict__ arena, const nww_mix_item* __restrict__ tab, int B, int N,
                                                          int16_t* __restrict__ out) {
    __shared__ unsigned long long red_sum[2][MIX_THREADS / 64];
    __shared__ unsigned red_max[MIX_THREADS / 64];
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int clip = blockIdx.x; clip < B; clip += gridDim.x) {
        const nww_mix_item it = tab[clip];
        MixClip c;
        c.fg = arena + it.fg_off; c.fg_len = it.fg_len;
        c.bg = it.bg_len > 0 ? arena + it.bg_off : nullptr; c.bg_len = it.bg_len; c.bg_start = it.bg_start;
        c.ws = it.start;
        bool real = false;
        float s = 0.0f;
        if (c.bg) {                                                    // pass 1
            unsigned long long Sf = 0, Sb = 0;
            unsigned P = 0;
            if (mix_mode(c) == MIX_FG_BG) mix_pass_stats<MIX_FG_BG>(c, N, Sf, Sb, P);
            else mix_pass_stats<MIX_SLOW>(c, N, Sf, Sb, P);
            Sf = wave_sum(Sf); Sb = wave_sum(Sb); P = wave_max(P);
            __syncthreads();
            if (lane == 0) { red_sum[0][wave] = Sf; red_sum[1][wave] = Sb; red_max[wave] = P; }
            __syncthreads();
            Sf = Sb = 0; P = 0;
#pragma unroll
            for (int w = 0; w < MIX_THREADS / 64; ++w) { Sf += red_sum[0][w]; Sb += red_sum[1][w]; P = red_max[w] > P ? red_max[w] : P; }
            real = mix_real_background(it.bg_len, (int32_t)P);
            if (real) s = mix_scale(Sf, Sb, it.fg_len, it.snr_linear);
        }
        if (!real) { c.bg = nullptr; c.ws = 0; }                       // the foreground alone, at the clip's start
        const int mode = mix_mode(c);
        float pk = 0.0f;
        if (it.flags & NWW_MIX_PEAK_NORMALISE) {                       // pass 2
            unsigned m = mode == MIX_FG_BG ? mix_pass_peak<MIX_FG_BG>(c, N, real, s, it.gain)
                       : mode == MIX_FG    ? mix_pass_peak<MIX_FG>(c, N, real, s, it.gain)
                                           : mix_pass_peak<MIX_SLOW>(c, N, real, s, it.gain);
            m = wave_max(m);
            __syncthreads();
            if (lane == 0) red_max[wave] = m;
            __syncthreads();
            m = 0;
#pragma unroll
            for (int w = 0; w < MIX_THREADS / 64; ++w) m = red_max[w] > m ? red_max[w] : m;
            pk = __uint_as_float(m);
        }
        const float r = mix_ratio(it.level, it.flags, pk);
        int16_t* o = out + (size_t)clip * (size_t)N;
        if (mode == MIX_FG_BG) mix_pass_store<MIX_FG_BG>(c, N, real, s, it.gain, r, o);      // pass 3
        else if (mode == MIX_FG) mix_pass_store<MIX_FG>(c, N, real, s, it.gain, r, o);
        else mix_pass_store<MIX_SLOW>(c, N, real, s, it.gain, r, o);
    }
}

}  // namespace

hipError_t mix_launch(const int16_t* d_arena, const nww_mix_item* d_tab, int B, int N, int16_t* d_out, int cu_count, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    const int cap = cu_count * 32;                                     // a clip is a few trips of one workgroup: leave the tail to the dispatcher
    hipLaunchKernelGGL(mix_kernel, dim3((unsigned)(B < cap ? B : cap)), dim3(MIX_THREADS), 0, stream, d_arena, d_tab, B, N, d_out);
    return hipGetLastError();
}
