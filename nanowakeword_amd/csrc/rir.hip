// rir.hip - clips convolved with room impulse responses on the device (include/nww.h, nww_mix_rir_* / nww_rir_*): one
// workgroup per clip, the whole clip in LDS as M float32 = M / 2 packed complex values (128 KiB at M = 32768: one workgroup per CU).
//   1  mix.hip's pass 1 from the same mix_plan.h functions (integer Sf, Sb, P -> the scale), sample by sample
//   2  y = mix_y(...) straight into LDS, zeros behind the clip
//   3  ir_id >= 0 (the same in every lane): forward radix-4 network in place (digit-reversed result), the pair stage - real-input
//      split, product with the response's spectrum, packing for the inverse - where the values lie, inverse network (natural order)
//   4  peak over the first N (flags bit 0), ratio, mix_out
// Butterflies, split and product are rir_plan.h's, shared with the CPU check; twiddles and spectra are read from global memory (one
// table per M, L2-resident).  Every reduction is an integer add or max: a clip's bits depend on its item and its response alone.
// 1024 threads at M = 8192 and 32768 (4 waves per SIMD, which 8-byte LDS reads and writes need to reach their rate; a thread has four
// butterflies of a stage at M = 32768, one at 8192), 256 at M = 2048, whose stages have 256 butterflies.  Built without SLP (build.py).
#include "rir.h"
#include "layers.h"
#include "rir_plan.h"

namespace {

template <int M> struct RirCfg {
    static constexpr int H = M / 2, D = M == 2048 ? 5 : M == 8192 ? 6 : 7, THREADS = M == 2048 ? 256 : 1024;
    static_assert(H == 1 << (2 * D), "M / 2 is a power of four");
};

template <int D> __device__ inline uint32_t rev_dev(uint32_t k) {       // rir_rev on v_bfrev
    const uint32_t r = __brev(k) >> (32 - 2 * D);
    return ((r & 0xaaaaaaaau) >> 1) | ((r & 0x55555555u) << 1);
}

// One stage of either network: a thread's PER butterflies are read - twiddles from global memory, points from LDS - before the first
// is computed, so that a stage costs one trip to L2 and one to LDS, not PER of each behind one another.
template <int M, bool FWD> __device__ inline void fft_stage(RirC* z, const RirC* __restrict__ T, int s) {
    constexpr int H = RirCfg<M>::H, THREADS = RirCfg<M>::THREADS, PER = H / 4 / THREADS;
    static_assert(PER * THREADS * 4 == H, "a stage is PER butterflies per thread");
    const int tw = M / (4 * s);
    RirC a[PER][4], w[PER][3];
    int g[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int u = (int)threadIdx.x + i * THREADS, j = u & (s - 1);
        g[i] = ((u - j) << 2) + j;
#pragma unroll
        for (int m = 0; m < 3; ++m) w[i][m] = T[(m + 1) * j * tw];
    }
#pragma unroll
    for (int i = 0; i < PER; ++i)
#pragma unroll
        for (int m = 0; m < 4; ++m) a[i][m] = z[g[i] + m * s];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        if (FWD) rir_bfly_fwd(a[i], w[i][0], w[i][1], w[i][2]);
        else rir_bfly_inv(a[i], w[i][0], w[i][1], w[i][2]);
#pragma unroll
        for (int m = 0; m < 4; ++m) z[g[i] + m * s] = a[i][m];
    }
    __syncthreads();
}

template <int M> __device__ inline void fft_forward(RirC* z, const RirC* __restrict__ T) {
#pragma unroll 1
    for (int s = RirCfg<M>::H / 4; s >= 1; s >>= 2) fft_stage<M, true>(z, T, s);
}

template <int M> __device__ inline void fft_inverse(RirC* z, const RirC* __restrict__ T) {
#pragma unroll 1
    for (int s = 1; s <= RirCfg<M>::H / 4; s <<= 2) fft_stage<M, false>(z, T, s);
}

// the positions and the bin of pair task u (rir_plan.h): task 0 works on the self-paired k = H / 2
template <int M> __device__ inline void pair_task(uint32_t u, uint32_t& pk, uint32_t& pm, uint32_t& k) {
    constexpr int H = RirCfg<M>::H, D = RirCfg<M>::D;
    pk = u ? rir_task_pos(u) : 2u;
    k = u ? rev_dev<D>(pk) : (uint32_t)(H / 2);
    pm = rev_dev<D>((uint32_t)H - k);
}

template <int M>
__global__ __launch_bounds__(RirCfg<M>::THREADS) void rir_prepare_kernel(const float* __restrict__ irs, const int64_t* __restrict__ off,
                                                                         const int32_t* __restrict__ len, int N, const RirC* __restrict__ T,
                                                                         RirC* __restrict__ spectra) {
    constexpr int H = RirCfg<M>::H, THREADS = RirCfg<M>::THREADS;
    extern __shared__ __attribute__((aligned(16))) float rir_lds[];
    RirC* z = reinterpret_cast<RirC*>(rir_lds);
    const float* h = irs + off[blockIdx.x];
    const int L = len[blockIdx.x], n = L < N ? L : N;
    for (int i = threadIdx.x; i < M; i += THREADS) rir_lds[i] = i < n ? h[i] : 0.0f;
    __syncthreads();
    fft_forward<M>(z, T);
    RirC* spec = spectra + (size_t)blockIdx.x * H;
    const float scale = 1.0f / (float)(8 * H);
    for (uint32_t u = threadIdx.x; u < (uint32_t)(H / 2); u += THREADS) {
        uint32_t pk, pm, k;
        pair_task<M>(u, pk, pm, k);
        RirC sk, sm;
        rir_spectrum_pair(z[pk], z[pm], T[k], scale, sk, sm);
        spec[pm] = sm; spec[pk] = sk;
        if (u == 0) spec[0] = rir_spectrum0(z[0], scale);
    }
}

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

// PITCH: the instance of nww_mix_aug_* - a clip whose pitch_id >= 0 is staged from yf32 (pitch.hip's shifted clip, its row in the item's
// `reserved`) in place of steps 1 and 2; every other clip, and the instance without the flag, runs as it always has
template <int M, bool PITCH>
__global__ __launch_bounds__(RirCfg<M>::THREADS) void rir_mix_kernel(const int16_t* __restrict__ arena, const nww_mix_item* __restrict__ tab,
                                                                     const nww_rir_item* __restrict__ rtab, const RirC* __restrict__ spectra,
                                                                     const RirC* __restrict__ T, int N, int16_t* __restrict__ out,
                                                                     const nww_pitch_item* __restrict__ ptab, const float* __restrict__ yf32) {
    constexpr int H = RirCfg<M>::H, THREADS = RirCfg<M>::THREADS, WAVES = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) float rir_lds[];
    __shared__ unsigned long long red_sum[2][WAVES];
    __shared__ unsigned red_max[2][WAVES];
    RirC* z = reinterpret_cast<RirC*>(rir_lds);
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t clip = blockIdx.x;
    const nww_mix_item it = tab[clip];
    const int ir = rtab[clip].ir_id;
    const bool shifted = PITCH && ptab[clip].pitch_id >= 0;            // the same in every lane of the workgroup
    const int16_t* fg = arena + it.fg_off;
    const int16_t* bg = it.bg_len > 0 && !shifted ? arena + it.bg_off : nullptr;
    const unsigned bg_len = (unsigned)it.bg_len;
    // this thread's background samples: clip sample i = tid + t THREADS reads bg[p], p stepping modulo bg_len
    const unsigned p0 = bg ? ((unsigned)it.bg_start + tid) % bg_len : 0u, step = bg ? (unsigned)THREADS % bg_len : 0u;
    bool real = false;
    float s = 0.0f;
    if (bg) {                                                          // pass 1
        unsigned long long Sf = 0, Sb = 0;
        unsigned P = 0, p = p0;
#pragma unroll 4
        for (unsigned i = tid; i < (unsigned)N; i += THREADS) {
            const int b = bg[p];
            p += step; if (p >= bg_len) p -= bg_len;
            const unsigned a = (unsigned)(b < 0 ? -b : b);
            P = a > P ? a : P;
            const long long j = (long long)i - it.start;
            if (j >= 0 && j < it.fg_len) { const int f = fg[j]; Sf += (unsigned)(f * f); Sb += (unsigned)(b * b); }
        }
        Sf = wave_sum(Sf); Sb = wave_sum(Sb); P = wave_max(P);
        if (lane == 0) { red_sum[0][wave] = Sf; red_sum[1][wave] = Sb; red_max[0][wave] = P; }
        __syncthreads();
        Sf = Sb = 0; P = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { Sf += red_sum[0][w]; Sb += red_sum[1][w]; P = red_max[0][w] > P ? red_max[0][w] : P; }
        real = mix_real_background(it.bg_len, (int32_t)P);
        if (real) s = mix_scale(Sf, Sb, it.fg_len, it.snr_linear);
    }
    const long long ws = real ? it.start : 0;                          // without a real background: the foreground alone, at the clip's start
    if (shifted) {
        const float* y = yf32 + (size_t)ptab[clip].reserved * (size_t)N;
#pragma unroll 4
        for (unsigned i = tid; i < (unsigned)M; i += THREADS) rir_lds[i] = i < (unsigned)N ? y[i] : 0.0f;
    } else {
        unsigned p = p0;
#pragma unroll 4
        for (unsigned i = tid; i < (unsigned)M; i += THREADS) {
            float v = 0.0f;
            if (i < (unsigned)N) {
                const long long j = (long long)i - ws;
                const bool in_fg = j >= 0 && j < it.fg_len;
                int b = 0;
                if (real) { b = bg[p]; p += step; if (p >= bg_len) p -= bg_len; }
                v = mix_y(in_fg ? fg[j] : 0, b, in_fg, real, s, it.gain);
            }
            rir_lds[i] = v;
        }
    }
    __syncthreads();
    if (ir >= 0) {                                                     // the same in every lane of the workgroup
        fft_forward<M>(z, T);
        const RirC* spec = spectra + (size_t)ir * H;
        constexpr int PAIRS = H / 2 / THREADS, STEP = PAIRS < 4 ? PAIRS : 4;       // a thread's tasks, STEP at a time: their loads first
#pragma unroll 1
        for (int t0 = 0; t0 < PAIRS; t0 += STEP) {
            uint32_t pk[STEP], pm[STEP];
            RirC w[STEP], sk[STEP], sm[STEP], zk[STEP], zm[STEP];
#pragma unroll
            for (int i = 0; i < STEP; ++i) {
                uint32_t k;
                pair_task<M>(tid + (uint32_t)(t0 + i) * THREADS, pk[i], pm[i], k);
                w[i] = T[k]; sk[i] = spec[pk[i]]; sm[i] = spec[pm[i]];
                zk[i] = z[pk[i]]; zm[i] = z[pm[i]];
            }
#pragma unroll
            for (int i = 0; i < STEP; ++i) {
                rir_pair(zk[i], zm[i], w[i], sk[i], sm[i]);
                z[pm[i]] = zm[i]; z[pk[i]] = zk[i];
            }
        }
        if (tid == 0) z[0] = rir_pair0(z[0], spec[0]);
        __syncthreads();
        fft_inverse<M>(z, T);
    }
    float pk = 0.0f;
    if (it.flags & NWW_MIX_PEAK_NORMALISE) {                           // max |w| as a max over the bit patterns of the non-negative floats
        unsigned m = 0;
        for (unsigned i = tid; i < (unsigned)N; i += THREADS) { const unsigned a = __float_as_uint(rir_lds[i]) & 0x7fffffffu; m = a > m ? a : m; }
        m = wave_max(m);
        if (lane == 0) red_max[1][wave] = m;
        __syncthreads();
        m = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) m = red_max[1][w] > m ? red_max[1][w] : m;
        pk = __uint_as_float(m);
    }
    const float r = mix_ratio(it.level, it.flags, pk);
    int16_t* o = out + clip * (size_t)N;
#pragma unroll 4
    for (unsigned i = tid; i < (unsigned)N; i += THREADS) o[i] = mix_out(rir_lds[i], r);
}

// ---- the segmented route (rir_plan.h: RIR_SEG_*): partitions of RIR_SEG_LP taps, segments of RIR_SEG_V outputs, on the M = 32768 network
constexpr int SEG_M = RIR_M_MAX, SEG_H = SEG_M / 2, SEG_V = RIR_SEG_V, SEG_THREADS = RirCfg<SEG_M>::THREADS, SEG_PER = SEG_V / SEG_THREADS;
static_assert(SEG_V % SEG_THREADS == 0 && SEG_M == 2 * SEG_V && RIR_SEG_LP <= SEG_M - SEG_V + 1, "a window is two segments; its upper half is free of wrap-around");

// One workgroup per (response, partition): blockIdx.x = k * P_max + p.  Partition 0's workgroup also writes the response's count, and
// the first workgroup the header's two leading words.
__global__ __launch_bounds__(SEG_THREADS) void rir_seg_prepare_kernel(const float* __restrict__ irs, const int64_t* __restrict__ off,
                                                                      const int32_t* __restrict__ len, int K, int N, int P_max,
                                                                      const RirC* __restrict__ T, float* __restrict__ spectra) {
    extern __shared__ __attribute__((aligned(16))) float rir_lds[];
    RirC* z = reinterpret_cast<RirC*>(rir_lds);
    const int k = (int)(blockIdx.x / (unsigned)P_max), p = (int)(blockIdx.x % (unsigned)P_max);
    const int P = rir_parts(N, len[k]);
    int32_t* hdr = reinterpret_cast<int32_t*>(spectra);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) { hdr[0] = P_max; hdr[1] = K; }
        if (p == 0) hdr[2 + k] = P;
    }
    if (p >= P) return;                                                // the same in every lane of the workgroup
    const int L = len[k], Le = L < N ? L : N, lo = p * RIR_SEG_LP, n = Le - lo < RIR_SEG_LP ? Le - lo : RIR_SEG_LP;
    const float* h = irs + off[k] + lo;
    for (int i = threadIdx.x; i < SEG_M; i += SEG_THREADS) rir_lds[i] = i < n ? h[i] : 0.0f;
    __syncthreads();
    fft_forward<SEG_M>(z, T);
    RirC* spec = reinterpret_cast<RirC*>(spectra + rir_seg_header_floats(K)) + (size_t)blockIdx.x * SEG_H;
    const float scale = 1.0f / (float)(8 * SEG_H);
    for (uint32_t u = threadIdx.x; u < (uint32_t)(SEG_H / 2); u += SEG_THREADS) {
        uint32_t pk, pm, kk;
        pair_task<SEG_M>(u, pk, pm, kk);
        RirC sk, sm;
        rir_spectrum_pair(z[pk], z[pm], T[kk], scale, sk, sm);
        spec[pm] = sm; spec[pk] = sk;
        if (u == 0) spec[0] = rir_spectrum0(z[0], scale);
    }
}

// One workgroup per (clip, segment): blockIdx.x = clip * Q + q.  Pass 1 runs over the WHOLE clip in every one of a clip's workgroups
// (N int16 reads out of L2 against fifteen LDS passes per transform), so that a segment's bits are a function of its item and response
// alone.  A thread keeps its SEG_PER = 16 outputs r = tid + j THREADS of the segment in registers across the partitions.
// PITCH: as rir_mix_kernel's flag - a window of a clip whose pitch_id >= 0 is read from yf32
template <bool PITCH>
__global__ __launch_bounds__(SEG_THREADS) void rir_seg_kernel(const int16_t* __restrict__ arena, const nww_mix_item* __restrict__ tab,
                                                              const nww_rir_item* __restrict__ rtab, const float* __restrict__ spectra,
                                                              const RirC* __restrict__ T, int N, int Q, float* __restrict__ w_out,
                                                              unsigned* __restrict__ peaks, const nww_pitch_item* __restrict__ ptab,
                                                              const float* __restrict__ yf32) {
    constexpr int THREADS = SEG_THREADS, WAVES = THREADS / 64, M = SEG_M, H = SEG_H, V = SEG_V;
    extern __shared__ __attribute__((aligned(16))) float rir_lds[];
    __shared__ unsigned long long red_sum[2][WAVES];
    __shared__ unsigned red_max[2][WAVES];
    RirC* z = reinterpret_cast<RirC*>(rir_lds);
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t clip = blockIdx.x / (unsigned)Q;
    const int q = (int)(blockIdx.x % (unsigned)Q);
    const nww_mix_item it = tab[clip];
    const int ir = rtab[clip].ir_id;
    const bool shifted = PITCH && ptab[clip].pitch_id >= 0;            // the same in every lane of the workgroup
    const float* ysh = shifted ? yf32 + (size_t)ptab[clip].reserved * (size_t)N : nullptr;
    const int16_t* fg = arena + it.fg_off;
    const int16_t* bg = it.bg_len > 0 && !shifted ? arena + it.bg_off : nullptr;
    const unsigned bg_len = (unsigned)it.bg_len;
    const unsigned step = bg ? (unsigned)THREADS % bg_len : 0u;
    bool real = false;
    float s = 0.0f;
    if (bg) {                                                          // pass 1, as rir_mix_kernel's
        unsigned long long Sf = 0, Sb = 0;
        unsigned P = 0, p = ((unsigned)it.bg_start + tid) % bg_len;
#pragma unroll 4
        for (unsigned i = tid; i < (unsigned)N; i += THREADS) {
            const int b = bg[p];
            p += step; if (p >= bg_len) p -= bg_len;
            const unsigned a = (unsigned)(b < 0 ? -b : b);
            P = a > P ? a : P;
            const long long j = (long long)i - it.start;
            if (j >= 0 && j < it.fg_len) { const int f = fg[j]; Sf += (unsigned)(f * f); Sb += (unsigned)(b * b); }
        }
        Sf = wave_sum(Sf); Sb = wave_sum(Sb); P = wave_max(P);
        if (lane == 0) { red_sum[0][wave] = Sf; red_sum[1][wave] = Sb; red_max[0][wave] = P; }
        __syncthreads();
        Sf = Sb = 0; P = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { Sf += red_sum[0][w]; Sb += red_sum[1][w]; P = red_max[0][w] > P ? red_max[0][w] : P; }
        real = mix_real_background(it.bg_len, (int32_t)P);
        if (real) s = mix_scale(Sf, Sb, it.fg_len, it.snr_linear);
    }
    const long long ws = real ? it.start : 0;
    // y of clip samples a0 + tid + t THREADS, t in [t0, t1), into dst[tid + t THREADS]: zeros outside the clip; the background index is
    // taken modulo its length once and stepped from there
    auto stage = [&](long long a0, int t0, int t1, float* dst) {
        const long long first = a0 + tid + (long long)t0 * THREADS;
        unsigned p = real && first >= 0 ? (unsigned)(((unsigned long long)it.bg_start + (unsigned long long)first) % bg_len) : 0u;
#pragma unroll 4
        for (int t = t0; t < t1; ++t) {
            const long long i = a0 + tid + (long long)t * THREADS;
            float v = 0.0f;
            if (i >= 0 && i < N) {
                if (PITCH && shifted) {
                    v = ysh[i];
                } else {
                    const long long j = i - ws;
                    const bool in_fg = j >= 0 && j < it.fg_len;
                    int b = 0;
                    if (real) b = bg[p];
                    v = mix_y(in_fg ? fg[j] : 0, b, in_fg, real, s, it.gain);
                }
            }
            if (real) { p += step; if (p >= bg_len) p -= bg_len; }
            dst[tid + t * THREADS] = v;
        }
    };
    float acc[SEG_PER];
    if (ir < 0) {                                                      // the same in every lane of the workgroup: mix.hip's clip
        stage((long long)q * V, 0, SEG_PER, rir_lds);                  // a thread reads back what it wrote itself
#pragma unroll
        for (int j = 0; j < SEG_PER; ++j) acc[j] = rir_lds[tid + j * THREADS];
    } else {
        const int32_t* hdr = reinterpret_cast<const int32_t*>(spectra);
        const int P_max = hdr[0], P = hdr[2 + ir];
        const RirC* spec0 = reinterpret_cast<const RirC*>(spectra + rir_seg_header_floats(hdr[1])) + (size_t)ir * P_max * H;
        const int last = P - 1 < q ? P - 1 : q;
#pragma unroll 1
        for (int p = 0; p <= last; ++p) {
            const RirC* spec = spec0 + (size_t)p * H;
            // the window [(q - p - 1) V, (q - p + 1) V): with p == q its lower half lies before the clip
            if (p == q) {
#pragma unroll
                for (int t = 0; t < SEG_PER; ++t) rir_lds[tid + t * THREADS] = 0.0f;
                stage(-(long long)V, SEG_PER, 2 * SEG_PER, rir_lds);
            } else {
                stage((long long)(q - p - 1) * V, 0, 2 * SEG_PER, rir_lds);
            }
            __syncthreads();
            fft_forward<M>(z, T);
            constexpr int PAIRS = H / 2 / THREADS, STEP = 4;
#pragma unroll 1
            for (int t0 = 0; t0 < PAIRS; t0 += STEP) {
                uint32_t pk[STEP], pm[STEP];
                RirC w[STEP], sk[STEP], sm[STEP], zk[STEP], zm[STEP];
#pragma unroll
                for (int i = 0; i < STEP; ++i) {
                    uint32_t k;
                    pair_task<M>(tid + (uint32_t)(t0 + i) * THREADS, pk[i], pm[i], k);
                    w[i] = T[k]; sk[i] = spec[pk[i]]; sm[i] = spec[pm[i]];
                    zk[i] = z[pk[i]]; zm[i] = z[pm[i]];
                }
#pragma unroll
                for (int i = 0; i < STEP; ++i) {
                    rir_pair(zk[i], zm[i], w[i], sk[i], sm[i]);
                    z[pm[i]] = zm[i]; z[pk[i]] = zk[i];
                }
            }
            if (tid == 0) z[0] = rir_pair0(z[0], spec[0]);
            __syncthreads();
            fft_inverse<M>(z, T);                                      // ends in a barrier
#pragma unroll
            for (int j = 0; j < SEG_PER; ++j) acc[j] = rir_seg_acc(p, acc[j], rir_lds[V + tid + j * THREADS]);
            __syncthreads();                                           // the next window overwrites what was just read
        }
    }
    float* wrow = w_out + clip * (size_t)N + (size_t)q * V;
    const int n = N - q * V < V ? N - q * V : V;
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < SEG_PER; ++j) {
        const int r = (int)tid + j * THREADS;
        if (r < n) {
            wrow[r] = acc[j];
            const unsigned a = __float_as_uint(acc[j]) & 0x7fffffffu;
            m = a > m ? a : m;
        }
    }
    m = wave_max(m);
    if (lane == 0) red_max[1][wave] = m;
    __syncthreads();
    if (tid == 0) {
        m = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) m = red_max[1][w] > m ? red_max[1][w] : m;
        peaks[blockIdx.x] = m;
    }
}

// One workgroup per (clip, segment) again: the clip's peak out of its Q segments', the ratio, mix_out
__global__ __launch_bounds__(256) void rir_seg_tail_kernel(const nww_mix_item* __restrict__ tab, const float* __restrict__ w_in,
                                                           const unsigned* __restrict__ peaks, int N, int Q, int16_t* __restrict__ out) {
    __shared__ unsigned red_max[4];
    const unsigned tid = threadIdx.x;
    const size_t clip = blockIdx.x / (unsigned)Q;
    const int q = (int)(blockIdx.x % (unsigned)Q);
    const float level = tab[clip].level;
    const uint32_t flags = tab[clip].flags;
    float pk = 0.0f;
    if (flags & NWW_MIX_PEAK_NORMALISE) {
        unsigned m = 0;
        for (int i = (int)tid; i < Q; i += 256) { const unsigned a = peaks[clip * (size_t)Q + i]; m = a > m ? a : m; }
        m = wave_max(m);
        if ((tid & 63) == 0) red_max[tid >> 6] = m;
        __syncthreads();
        m = red_max[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) m = red_max[w] > m ? red_max[w] : m;
        pk = __uint_as_float(m);
    }
    const float r = mix_ratio(level, flags, pk);
    const size_t base = clip * (size_t)N + (size_t)q * SEG_V;
    const int n = N - q * SEG_V < SEG_V ? N - q * SEG_V : SEG_V;
#pragma unroll 4
    for (int i = (int)tid; i < n; i += 256) out[base + i] = mix_out(w_in[base + i], r);
}

template <int M>
hipError_t prepare_m(const float* d_irs, const int64_t* d_off, const int32_t* d_len, int K, int N, const float* d_tw, float* d_spectra, hipStream_t stream) {
    const size_t lds = (size_t)M * sizeof(float);
    const hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(&rir_prepare_kernel<M>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rir_prepare_kernel<M>, dim3((unsigned)K), dim3(RirCfg<M>::THREADS), lds, stream, d_irs, d_off, d_len, N,
                       reinterpret_cast<const RirC*>(d_tw), reinterpret_cast<RirC*>(d_spectra));
    return hipGetLastError();
}

template <int M, bool PITCH>
hipError_t mix_mp(const int16_t* d_arena, const nww_mix_item* d_tab, const nww_rir_item* d_rtab, const float* d_spectra, const float* d_tw, int B, int N,
                  int16_t* d_out, const nww_pitch_item* d_ptab, const float* d_y, hipStream_t stream) {
    const size_t lds = (size_t)M * sizeof(float);
    const hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(&rir_mix_kernel<M, PITCH>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((rir_mix_kernel<M, PITCH>), dim3((unsigned)B), dim3(RirCfg<M>::THREADS), lds, stream, d_arena, d_tab, d_rtab,
                       reinterpret_cast<const RirC*>(d_spectra), reinterpret_cast<const RirC*>(d_tw), N, d_out, d_ptab, d_y);
    return hipGetLastError();
}
template <int M>
hipError_t mix_m(const int16_t* d_arena, const nww_mix_item* d_tab, const nww_rir_item* d_rtab, const float* d_spectra, const float* d_tw, int B, int N,
                 int16_t* d_out, const nww_pitch_item* d_ptab, const float* d_y, hipStream_t stream) {
    return d_ptab ? mix_mp<M, true>(d_arena, d_tab, d_rtab, d_spectra, d_tw, B, N, d_out, d_ptab, d_y, stream)
                  : mix_mp<M, false>(d_arena, d_tab, d_rtab, d_spectra, d_tw, B, N, d_out, nullptr, nullptr, stream);
}

}  // namespace

hipError_t rir_prepare_launch(const float* d_irs, const int64_t* d_off, const int32_t* d_len, int K, int N, int M, const float* d_tw,
                              float* d_spectra, hipStream_t stream) {
    if (K <= 0) return hipSuccess;
    switch (M) {
    case 2048: return prepare_m<2048>(d_irs, d_off, d_len, K, N, d_tw, d_spectra, stream);
    case 8192: return prepare_m<8192>(d_irs, d_off, d_len, K, N, d_tw, d_spectra, stream);
    case 32768: return prepare_m<32768>(d_irs, d_off, d_len, K, N, d_tw, d_spectra, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t rir_seg_prepare_launch(const float* d_irs, const int64_t* d_off, const int32_t* d_len, int K, int N, int P_max, const float* d_tw,
                                  float* d_spectra, hipStream_t stream) {
    if (K <= 0) return hipSuccess;
    if (P_max < 1 || (int64_t)K * P_max > 0x7fffffff) return hipErrorInvalidValue;
    const size_t lds = (size_t)SEG_M * sizeof(float);
    const hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(&rir_seg_prepare_kernel), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rir_seg_prepare_kernel, dim3((unsigned)(K * P_max)), dim3(SEG_THREADS), lds, stream, d_irs, d_off, d_len, K, N, P_max,
                       reinterpret_cast<const RirC*>(d_tw), d_spectra);
    return hipGetLastError();
}

hipError_t rir_seg_mix_launch(const int16_t* d_arena, const nww_mix_item* d_tab, const nww_rir_item* d_rtab, const float* d_spectra,
                              const float* d_tw, int B, int N, float* d_w, unsigned* d_peaks, int16_t* d_out, hipStream_t stream,
                              const nww_pitch_item* d_ptab, const float* d_y) {
    if (B <= 0) return hipSuccess;
    const int Q = rir_segments(N);
    if (Q < 1 || (int64_t)B * Q > 0x7fffffff) return hipErrorInvalidValue;
    const size_t lds = (size_t)SEG_M * sizeof(float);
    const hipError_t e = nww_allow_lds(d_ptab ? reinterpret_cast<const void*>(&rir_seg_kernel<true>) : reinterpret_cast<const void*>(&rir_seg_kernel<false>), lds);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)(B * Q));
    if (d_ptab)
        hipLaunchKernelGGL(rir_seg_kernel<true>, grid, dim3(SEG_THREADS), lds, stream, d_arena, d_tab, d_rtab, d_spectra,
                           reinterpret_cast<const RirC*>(d_tw), N, Q, d_w, d_peaks, d_ptab, d_y);
    else
        hipLaunchKernelGGL(rir_seg_kernel<false>, grid, dim3(SEG_THREADS), lds, stream, d_arena, d_tab, d_rtab, d_spectra,
                           reinterpret_cast<const RirC*>(d_tw), N, Q, d_w, d_peaks, nullptr, nullptr);
    hipLaunchKernelGGL(rir_seg_tail_kernel, grid, dim3(256), 0, stream, d_tab, d_w, d_peaks, N, Q, d_out);
    return hipGetLastError();
}

hipError_t rir_mix_launch(const int16_t* d_arena, const nww_mix_item* d_tab, const nww_rir_item* d_rtab, const float* d_spectra, int M,
                          const float* d_tw, int B, int N, int16_t* d_out, hipStream_t stream, const nww_pitch_item* d_ptab, const float* d_y) {
    if (B <= 0) return hipSuccess;
    switch (M) {
    case 2048: return mix_m<2048>(d_arena, d_tab, d_rtab, d_spectra, d_tw, B, N, d_out, d_ptab, d_y, stream);
    case 8192: return mix_m<8192>(d_arena, d_tab, d_rtab, d_spectra, d_tw, B, N, d_out, d_ptab, d_y, stream);
    case 32768: return mix_m<32768>(d_arena, d_tab, d_rtab, d_spectra, d_tw, B, N, d_out, d_ptab, d_y, stream);
    }
    return hipErrorInvalidValue;
}
