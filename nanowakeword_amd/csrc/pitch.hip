// pitch.hip - clips shifted in pitch on the device (include/nww.h, nww_pitch_* / nww_mix_aug_*): three kernels, one
// workgroup of 256 threads per clip each; a clip whose pitch_id is -1 ends every one of them at once.
//   pitch_mix_f32_kernel    rir.hip's steps 1 and 2 - the integer statistics, the scale, y = mix_y(...) - into w [N] float32
//   pitch_vocoder_kernel    marches over the clip in tiles of PV_F output frames; per tile
//                             the input frames under it, windowed, into LDS and through the forward network and the split (tasks over
//                             the threads, frames side by side: a stage is one barrier for the whole tile);
//                             the recurrence, a thread per position over the tile's frames in order - u stays in its registers from
//                             tile to tile;
//                             the packing and the inverse network; the overlap-add, a thread per sample of the strip in ascending frame
//                             order; the strip's finished PV_F * 128 samples divided by the envelope and stored, its last 384 carried.
//                           The spectrogram is never materialised: LDS holds PV_NI input and PV_F output frames (40 KiB) and the tables.
//                           A tile's first one or two input frames were the previous tile's last: they are transformed again (2 of ~11)
//                           rather than kept, which saves the bookkeeping of a ring for a sixth of the forward work.
//   pitch_resample_kernel   a thread per output sample, 256 consecutive samples a trip: the stretched samples under a trip through LDS,
//                           the phase's taps as four 16-byte loads, PITCH_TAPS products in table order; with d_out the peak over the
//                           clip, the ratio and mix_out follow in the same workgroup, the float32 clip read back from L2
// Everything is pitch_plan.h's arithmetic, shared with the CPU check; reductions are integer adds and maxima: a clip's bits depend on
// its item and its ratio alone.  Built without SLP (build.py), as rir.hip.
#include "pitch.h"
#include "pitch_plan.h"

namespace {

constexpr int PV_THREADS = 256, PV_WAVES = PV_THREADS / 64, PV_F = 8, PV_NI = 12;
constexpr int PV_STRIP = (PV_F + 3) * PITCH_HOP, PV_DONE = PV_F * PITCH_HOP, PV_CARRY = 3 * PITCH_HOP, PV_PER = (PV_STRIP + PV_THREADS - 1) / PV_THREADS;
// the input frames under PV_F output frames: i(t0 + PV_F - 1) - i(t0) <= floor((PV_F - 1) q / p) + 1, q / p <= 2^(1/3) < 162 / 128, and
// frames i .. i + 1 of the last
static_assert((PV_F - 1) * 162 / 128 + 1 + 2 <= PV_NI, "a tile's input frames fit");
static_assert(PITCH_H == PV_THREADS, "a thread per position");
// the stretched samples under PV_THREADS consecutive outputs of the resampler: ceil((PV_THREADS - 1) p / q) + PITCH_TAPS, p / q < 162 / 128
constexpr int RS_SPAN = PV_THREADS * 162 / 128 + PITCH_TAPS + 2;

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

__global__ __launch_bounds__(PV_THREADS) void pitch_mix_f32_kernel(const int16_t* __restrict__ arena, const nww_mix_item* __restrict__ tab,
                                                                   const nww_pitch_item* __restrict__ ptab, int N, float* __restrict__ w_out) {
    constexpr int THREADS = PV_THREADS, WAVES = PV_WAVES;
    __shared__ unsigned long long red_sum[2][WAVES];
    __shared__ unsigned red_max[WAVES];
    const size_t clip = blockIdx.x;
    if (ptab[clip].pitch_id < 0) return;                               // the same in every lane of the workgroup
    float* w = w_out + (size_t)ptab[clip].reserved * (size_t)N;
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const nww_mix_item it = tab[clip];
    const int16_t* fg = arena + it.fg_off;
    const int16_t* bg = it.bg_len > 0 ? arena + it.bg_off : nullptr;
    const unsigned bg_len = (unsigned)it.bg_len;
    const unsigned p0 = bg ? ((unsigned)it.bg_start + tid) % bg_len : 0u, step = bg ? (unsigned)THREADS % bg_len : 0u;
    bool real = false;
    float s = 0.0f;
    if (bg) {                                                          // pass 1, as rir_mix_kernel's
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
        if (lane == 0) { red_sum[0][wave] = Sf; red_sum[1][wave] = Sb; red_max[wave] = P; }
        __syncthreads();
        Sf = Sb = 0; P = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) { Sf += red_sum[0][k]; Sb += red_sum[1][k]; P = red_max[k] > P ? red_max[k] : P; }
        real = mix_real_background(it.bg_len, (int32_t)P);
        if (real) s = mix_scale(Sf, Sb, it.fg_len, it.snr_linear);
    }
    const long long ws = real ? it.start : 0;
    unsigned p = p0;
#pragma unroll 4
    for (unsigned i = tid; i < (unsigned)N; i += THREADS) {
        const long long j = (long long)i - ws;
        const bool in_fg = j >= 0 && j < it.fg_len;
        int b = 0;
        if (real) { b = bg[p]; p += step; if (p >= bg_len) p -= bg_len; }
        w[i] = mix_y(in_fg ? fg[j] : 0, b, in_fg, real, s, it.gain);
    }
}

// rir_rev at four digits
__device__ inline uint32_t rev4(uint32_t k) {
    const uint32_t r = __brev(k) >> 24;
    return ((r & 0xaau) >> 1) | ((r & 0x55u) << 1);
}
// the positions and the bin of pair task u < 128 of a frame (rir_plan.h): task 0 works on the self-paired k = 128
__device__ inline void pair_task(uint32_t u, uint32_t& pk, uint32_t& pm, uint32_t& k) {
    pk = u ? rir_task_pos(u) : 2u;
    k = u ? rev4(pk) : (uint32_t)(PITCH_H / 2);
    pm = rev4((uint32_t)PITCH_H - k);
}

// one stage of either network over n frames lying side by side: 64 butterflies a frame, tasks over the threads
template <bool FWD> __device__ inline void frames_stage(RirC* z, int n, const RirC* Tw, int s) {
    const int tw = PITCH_NFFT / (4 * s);
    for (int e = (int)threadIdx.x; e < n * 64; e += PV_THREADS) {
        RirC* zf = z + (e >> 6) * PITCH_H;
        const int u = e & 63, j = u & (s - 1), g = ((u - j) << 2) + j;
        RirC a[4] = {zf[g], zf[g + s], zf[g + 2 * s], zf[g + 3 * s]};
        if (FWD) rir_bfly_fwd(a, Tw[j * tw], Tw[2 * j * tw], Tw[3 * j * tw]);
        else rir_bfly_inv(a, Tw[j * tw], Tw[2 * j * tw], Tw[3 * j * tw]);
#pragma unroll
        for (int m = 0; m < 4; ++m) zf[g + m * s] = a[m];
    }
    __syncthreads();
}

__global__ __launch_bounds__(PV_THREADS) void pitch_vocoder_kernel(const nww_pitch_item* __restrict__ ptab, const PitchRatio* __restrict__ ratios,
                                                                   const float* __restrict__ tables, const float* __restrict__ w_in, int N,
                                                                   float* __restrict__ s_out, int s_stride) {
    __shared__ __attribute__((aligned(16))) RirC Xin[PV_NI * PITCH_H];
    __shared__ __attribute__((aligned(16))) RirC Yo[PV_F * PITCH_H];
    __shared__ RirC Tw[PITCH_NFFT / 4 * 3];
    __shared__ float win[PITCH_NFFT];
    __shared__ float carry[PV_CARRY];
    const size_t clip = blockIdx.x;
    const int pid = ptab[clip].pitch_id;
    if (pid < 0) return;                                               // the same in every lane of the workgroup
    const size_t row = ptab[clip].reserved;
    const int tid = (int)threadIdx.x;
    const int p = ratios[pid].p, q = ratios[pid].q;
    const int T = pitch_frames(N), T_out = pitch_out_frames(T, p, q), S = pitch_stretched(T_out);
    const float* w = w_in + row * (size_t)N;
    float* sr = s_out + row * (size_t)s_stride;
    const float* env = tables + PITCH_TAB_ENV;
    for (int i = tid; i < PITCH_NFFT / 4 * 3; i += PV_THREADS) Tw[i] = reinterpret_cast<const RirC*>(tables + PITCH_TAB_TW)[i];
    for (int i = tid; i < PITCH_NFFT; i += PV_THREADS) win[i] = tables[PITCH_TAB_WIN + i];
    for (int i = tid; i < PV_CARRY; i += PV_THREADS) carry[i] = 0.0f;
    __syncthreads();
    RirC u = {1.0f, 0.0f}, uh = {1.0f, 0.0f};                          // this position's unit vector (thread 0: bins 0 and 256)
#pragma unroll 1
    for (int t0 = 0; t0 <= T_out; t0 += PV_F) {
        const int nf = T_out - t0 < PV_F ? T_out - t0 : PV_F;          // <= 0 behind the last frame: the strip is flushed all the same
        if (nf > 0) {
            const int ib = (int)((long long)t0 * q / p);
            int ni = (int)((long long)(t0 + nf - 1) * q / p) + 2 - ib;
            ni = ni < PV_NI ? ni : PV_NI;
            float* xf = reinterpret_cast<float*>(Xin);
            for (int e = tid; e < ni * PITCH_NFFT; e += PV_THREADS) {
                const int f = e >> 9, n = e & (PITCH_NFFT - 1), i = ib + f;
                float v = 0.0f;
                if (i < T) { MIX_NO_CONTRACT v = w[pitch_reflect(PITCH_HOP * i + n - PITCH_NFFT / 2, N)] * win[n]; }
                xf[e] = v;
            }
            __syncthreads();
#pragma unroll 1
            for (int s = PITCH_H / 4; s >= 1; s >>= 2) frames_stage<true>(Xin, ni, Tw, s);
            for (int e = tid; e < ni * (PITCH_H / 2); e += PV_THREADS) {
                RirC* z = Xin + (e >> 7) * PITCH_H;
                uint32_t pk, pm, k;
                pair_task((uint32_t)(e & 127), pk, pm, k);
                RirC xk, xm;
                rir_split(z[pk], z[pm], Tw[k], xk, xm);
                z[pm] = xm; z[pk] = xk;
                if ((e & 127) == 0) z[0] = rir_split0(z[0]);
            }
            __syncthreads();
#pragma unroll 1
            for (int f = 0; f < nf; ++f) {                             // the recurrence: this thread's position, frames in order
                const long long tq = (long long)(t0 + f) * q;
                const int i = (int)(tq / p), m = (int)(tq - (long long)i * p);
                const float alpha = pitch_alpha(m, p);
                const RirC x0 = Xin[(i - ib) * PITCH_H + tid], x1 = Xin[(i - ib + 1) * PITCH_H + tid];
                if (t0 + f == 0) {
                    if (tid) u = pitch_unit(x0);
                    else { u = pitch_unit({x0.re, 0.0f}); uh = pitch_unit({x0.im, 0.0f}); }
                }
                Yo[f * PITCH_H + tid] = tid ? pitch_bin(x0, x1, alpha, u) : pitch_bin0(x0, x1, alpha, u, uh);
            }
            __syncthreads();
            for (int e = tid; e < nf * (PITCH_H / 2); e += PV_THREADS) {
                RirC* y = Yo + (e >> 7) * PITCH_H;
                uint32_t pk, pm, k;
                pair_task((uint32_t)(e & 127), pk, pm, k);
                RirC zk, zm;
                rir_unsplit(y[pk], y[pm], Tw[k], zk, zm);
                y[pm] = zm; y[pk] = zk;
                if ((e & 127) == 0) y[0] = rir_unsplit0(y[0].re, y[0].im);
            }
            __syncthreads();
#pragma unroll 1
            for (int s = 1; s <= PITCH_H / 4; s <<= 2) frames_stage<false>(Yo, nf, Tw, s);
        }
        // the strip: padded positions 128 t0 + e, e < PV_STRIP; its first 384 carry the previous tiles' frames
        float acc[PV_PER];
        const float* yf = reinterpret_cast<const float*>(Yo);
#pragma unroll
        for (int j = 0; j < PV_PER; ++j) {
            const int e = tid + j * PV_THREADS;
            float a = 0.0f;
            if (e < PV_STRIP) {
                if (e < PV_CARRY) a = carry[e];
                for (int f = 0; f < nf; ++f) {
                    const int off = e - PITCH_HOP * f;
                    if (off >= 0 && off < PITCH_NFFT) a = pitch_ola(a, pitch_synth(yf[f * PITCH_NFFT + off], win[off]));
                }
            }
            acc[j] = a;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PV_PER; ++j) {
            const int e = tid + j * PV_THREADS;
            if (e < PV_DONE) {
                const int P = PITCH_HOP * t0 + e, jo = P - PITCH_NFFT / 2;
                if (jo >= 0 && jo < S) sr[jo] = acc[j] / env[pitch_env_mask(P / PITCH_HOP, T_out) * PITCH_HOP + (P & (PITCH_HOP - 1))];
            } else if (e < PV_STRIP) {
                carry[e - PV_DONE] = acc[j];
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PV_THREADS) void pitch_resample_kernel(const nww_mix_item* __restrict__ tab, const nww_pitch_item* __restrict__ ptab,
                                                                    const PitchRatio* __restrict__ ratios, const float* __restrict__ taps,
                                                                    const float* __restrict__ s_in, int s_stride, int N, float* __restrict__ y_out,
                                                                    int16_t* __restrict__ out) {
    __shared__ unsigned red_max[PV_WAVES];
    __shared__ float span[RS_SPAN];
    const size_t clip = blockIdx.x;
    const int pid = ptab[clip].pitch_id;
    if (pid < 0) return;                                               // the same in every lane of the workgroup
    const size_t row = ptab[clip].reserved;
    const unsigned tid = threadIdx.x;
    const PitchRatio r = ratios[pid];
    const int S = pitch_stretched(pitch_out_frames(pitch_frames(N), r.p, r.q)), Ly = pitch_resampled(S, r.p, r.q);
    const float* s = s_in + row * (size_t)s_stride;
    const float* g = taps + r.off;
    float* y = y_out + row * (size_t)N;
    unsigned m = 0;
    // a trip of the workgroup is PV_THREADS consecutive outputs; the stretched samples under them - k0(n) = floor(n p / q) + PITCH_TAP0
    // moves by at most ceil(255 p / q) <= 322 over a trip - go through LDS once instead of sixteen times through L1 (zeros outside [0, S):
    // those taps are left out below, as pitch_plan.h says)
#pragma unroll 1
    for (int n0 = 0; n0 < N; n0 += PV_THREADS) {
        int32_t ph, k_lo;
        pitch_phase(n0, r.p, r.q, ph, k_lo);
        __syncthreads();                                               // the trip before has read its span
        for (int e = (int)tid; e < RS_SPAN; e += PV_THREADS) {
            const int k = k_lo + e;
            span[e] = k >= 0 && k < S ? s[k] : 0.0f;
        }
        __syncthreads();
        const int n = n0 + (int)tid;
        if (n < N) {
            float acc = 0.0f;
            if (n < Ly) {
                int32_t k0;
                pitch_phase(n, r.p, r.q, ph, k0);
                const float4* gp = reinterpret_cast<const float4*>(g + ph * PITCH_TAPS);       // rows of 64 bytes, aligned
                float gj[PITCH_TAPS];
#pragma unroll
                for (int j = 0; j < PITCH_TAPS / 4; ++j) { const float4 v = gp[j]; gj[4 * j] = v.x; gj[4 * j + 1] = v.y; gj[4 * j + 2] = v.z; gj[4 * j + 3] = v.w; }
                const int at = k0 - k_lo;                              // in [0, RS_SPAN - PITCH_TAPS]
#pragma unroll
                for (int j = 0; j < PITCH_TAPS; ++j)
                    if (k0 + j >= 0 && k0 + j < S) acc = pitch_tap(acc, span[at + j], gj[j]);
            }
            y[n] = acc;
            const unsigned a = __float_as_uint(acc) & 0x7fffffffu;
            m = a > m ? a : m;
        }
    }
    if (!out) return;
    const nww_mix_item it = tab[clip];
    float pk = 0.0f;
    if (it.flags & NWW_MIX_PEAK_NORMALISE) {
        m = wave_max(m);
        if ((tid & 63) == 0) red_max[tid >> 6] = m;
        __syncthreads();
        m = red_max[0];
#pragma unroll
        for (int k = 1; k < PV_WAVES; ++k) m = red_max[k] > m ? red_max[k] : m;
        pk = __uint_as_float(m);
    }
    const float ratio = mix_ratio(it.level, it.flags, pk);
    int16_t* o = out + clip * (size_t)N;
    for (int n = (int)tid; n < N; n += PV_THREADS) o[n] = mix_out(y[n], ratio);      // a thread reads back what it wrote itself
}

}  // namespace

hipError_t pitch_launch(const int16_t* d_arena, const nww_mix_item* d_tab, const nww_pitch_item* d_ptab, const PitchRatio* d_ratios,
                        const float* d_taps, const float* d_tables, int B, int N, float* d_w, float* d_s, int s_stride, int16_t* d_out,
                        hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    if (!pitch_length_ok(N) || s_stride < pitch_stride(N)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)B), block(PV_THREADS);
    hipLaunchKernelGGL(pitch_mix_f32_kernel, grid, block, 0, stream, d_arena, d_tab, d_ptab, N, d_w);
    hipLaunchKernelGGL(pitch_vocoder_kernel, grid, block, 0, stream, d_ptab, d_ratios, d_tables, d_w, N, d_s, s_stride);
    hipLaunchKernelGGL(pitch_resample_kernel, grid, block, 0, stream, d_tab, d_ptab, d_ratios, d_taps, d_s, s_stride, N, d_w, d_out);
    return hipGetLastError();
}
