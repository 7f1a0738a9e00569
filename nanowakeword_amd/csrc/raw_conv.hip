// raw_conv.hip - conv1d_strided: one stage of the raw-PCM frontend per launch.  A workgroup takes TT output rows of one clip: the input
// window ((TT - 1) stride + k rows, zeros outside the clip) is staged in LDS once, then every thread owns one output channel of four
// consecutive rows and walks the taps with float32 fmaf in a fixed order - a clip's result does not depend on its batch or slot.  The
// weights are tap-major [k][Cin][Cout], so the lanes of a wave read consecutive floats; the LDS reads of a row are broadcasts.
// conv2d_strided (further down) is the same manner of kernel for the RawAudioBackbone's zero-padded 3x3 convs: the float32 route of the
// e2e_cnn head that is always there (conv2s_x3.h).
#include "raw_conv.h"
#include "conv2s_x3.h"

namespace {

constexpr int RAW_THREADS = 256;
constexpr int RAW_ROWS_PER_THREAD = 4;
constexpr size_t RAW_LDS_BYTES = 48 * 1024;

template <bool PCM>
__global__ void __launch_bounds__(RAW_THREADS)
conv1d_strided_kernel(const int16_t* __restrict__ pcm, size_t pcm_stride, const float* __restrict__ x, const float* __restrict__ w,
                      const float* __restrict__ bias, float* __restrict__ y, int L, int Lout, int Cin, int Cout, int k, int stride, int TT,
                      int tiles, int ct_out) {
    extern __shared__ float xs[];                       // [(TT - 1) stride + k][Cin]
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * TT;
    const int rows = (TT - 1) * stride + k, in0 = t0 * stride - k / 2;
    for (int e = threadIdx.x; e < rows * Cin; e += RAW_THREADS) {
        const int r = e / Cin, ci = e - r * Cin, gi = in0 + r;
        float v = 0.0f;
        if (gi >= 0 && gi < L) {
            if (PCM) v = (float)pcm[(size_t)b * pcm_stride + gi] * (1.0f / 32768.0f);
            else v = x[((size_t)b * L + gi) * Cin + ci];
        }
        xs[e] = v;
    }
    __syncthreads();
    const int items = (TT / RAW_ROWS_PER_THREAD) * Cout;
    for (int e = threadIdx.x; e < items; e += RAW_THREADS) {
        const int tg = e / Cout, co = e - tg * Cout;
        const float b0 = bias[co];
        float acc[RAW_ROWS_PER_THREAD];
#pragma unroll
        for (int q = 0; q < RAW_ROWS_PER_THREAD; ++q) acc[q] = b0;
        const float* xr = xs + (size_t)tg * RAW_ROWS_PER_THREAD * stride * Cin;
        for (int j = 0; j < k; ++j) {
            const float* wj = w + (size_t)j * Cin * Cout + co;
            const float* xj = xr + j * Cin;
            for (int ci = 0; ci < Cin; ++ci) {
                const float wv = wj[(size_t)ci * Cout];
#pragma unroll
                for (int q = 0; q < RAW_ROWS_PER_THREAD; ++q) acc[q] = fmaf(xj[q * stride * Cin + ci], wv, acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < RAW_ROWS_PER_THREAD; ++q) {
            const int t = t0 + tg * RAW_ROWS_PER_THREAD + q;
            if (t < Lout) {
                const float v = fmaxf(acc[q], 0.0f);
                if (ct_out) y[((size_t)b * Cout + co) * Lout + t] = v;
                else y[((size_t)b * Lout + t) * Cout + co] = v;
            }
        }
    }
}

// conv2d_strided: zero-padded 3x3 convolution, stride 1 or 2 per axis, on channels-last planes [A][Bd][C] (conv2s_x3.h).  A thread owns
// one output channel of four consecutive Bd positions: the bias in front, then the taps in a fixed order (A tap, Bd tap, input channel)
// with float32 fmaf, the activation behind.  A tap that falls into the padding is skipped (it would add an exact zero).  The lanes of a
// wave are consecutive output channels of the same pixels, so the weight reads ([3][3][Cin][Cout]) are consecutive floats and the input
// reads broadcasts.  No tile, no batch dependence: any extents >= 1.
__global__ void __launch_bounds__(RAW_THREADS)
conv2d_strided_kernel(Conv2sArgs a, int Ao, int Bo, int BoG, size_t total) {
    const size_t idx = (size_t)blockIdx.x * RAW_THREADS + threadIdx.x;      // idx = ((b Ao + ao) BoG + bg) Cout + co
    if (idx >= total) return;
    const int co = (int)(idx % a.Cout);
    size_t r = idx / a.Cout;
    const int bg = (int)(r % BoG); r /= BoG;
    const int ao = (int)(r % Ao);
    const size_t b = r / Ao;
    const float* xb = a.x + b * (size_t)a.A * a.Bd * a.Cin;
    const float b0 = a.bias[co];
    float acc[RAW_ROWS_PER_THREAD];
#pragma unroll
    for (int q = 0; q < RAW_ROWS_PER_THREAD; ++q) acc[q] = b0;
    for (int tA = 0; tA < 3; ++tA) {
        const int ga = ao * a.sA - 1 + tA;
        if (ga < 0 || ga >= a.A) continue;
        for (int tB = 0; tB < 3; ++tB) {
            const float* wp = a.w + (size_t)(tA * 3 + tB) * a.Cin * a.Cout + co;
            const float* xp[RAW_ROWS_PER_THREAD];
#pragma unroll
            for (int q = 0; q < RAW_ROWS_PER_THREAD; ++q) {
                const int gb = (RAW_ROWS_PER_THREAD * bg + q) * a.sB - 1 + tB;
                xp[q] = (gb >= 0 && gb < a.Bd && RAW_ROWS_PER_THREAD * bg + q < Bo) ? xb + ((size_t)ga * a.Bd + gb) * a.Cin : nullptr;
            }
            for (int ci = 0; ci < a.Cin; ++ci) {
                const float wv = wp[(size_t)ci * a.Cout];
#pragma unroll
                for (int q = 0; q < RAW_ROWS_PER_THREAD; ++q)
                    if (xp[q]) acc[q] = fmaf(xp[q][ci], wv, acc[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < RAW_ROWS_PER_THREAD; ++q) {
        const int bo = RAW_ROWS_PER_THREAD * bg + q;
        if (bo < Bo) {
            const float v = acc[q];
            a.y[((b * Ao + ao) * Bo + bo) * a.Cout + co] = conv2s_act(v, a.act);
        }
    }
}

// The same sums for ONE input channel (the backbone's conv1): a thread owns one output pixel and all COUT channels, so the nine inputs are
// read once, the weights and biases are wave-uniform (scalar loads), and a pixel's COUT outputs leave as consecutive float4 stores.  The
// fmaf order per output is conv2d_strided_kernel's (bias, then A tap, Bd tap), so the results are the same bits.
template <int COUT>
__global__ void __launch_bounds__(RAW_THREADS)
conv2d_strided_c1_kernel(Conv2sArgs a, int Ao, int Bo, size_t total) {
    const size_t idx = (size_t)blockIdx.x * RAW_THREADS + threadIdx.x;      // idx = (b Ao + ao) Bo + bo
    if (idx >= total) return;
    const int bo = (int)(idx % Bo);
    const size_t r = idx / Bo;
    const int ao = (int)(r % Ao);
    const size_t b = r / Ao;
    const float* xb = a.x + b * (size_t)a.A * a.Bd;
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = a.bias[co];
#pragma unroll
    for (int tA = 0; tA < 3; ++tA) {
        const int ga = ao * a.sA - 1 + tA;
#pragma unroll
        for (int tB = 0; tB < 3; ++tB) {
            const int gb = bo * a.sB - 1 + tB;
            if (ga >= 0 && ga < a.A && gb >= 0 && gb < a.Bd) {
                const float xv = xb[(size_t)ga * a.Bd + gb];
                const float* wp = a.w + (tA * 3 + tB) * COUT;
#pragma unroll
                for (int co = 0; co < COUT; ++co) acc[co] = fmaf(xv, wp[co], acc[co]);
            }
        }
    }
    float* yp = a.y + idx * COUT;
#pragma unroll
    for (int co = 0; co < COUT; co += 4) {
        float4 v;
        v.x = conv2s_act(acc[co], a.act); v.y = conv2s_act(acc[co + 1], a.act); v.z = conv2s_act(acc[co + 2], a.act); v.w = conv2s_act(acc[co + 3], a.act);
        *reinterpret_cast<float4*>(yp + co) = v;
    }
}

}  // namespace

hipError_t launch_conv2d_strided(const Conv2sArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (a.A < 1 || a.Bd < 1 || a.Cin < 1 || a.Cout < 1 || a.sA < 1 || a.sA > 2 || a.sB < 1 || a.sB > 2 || !a.x || !a.y || !a.w || !a.bias) return hipErrorInvalidValue;
    const int Ao = conv2s_out(a.A, a.sA), Bo = conv2s_out(a.Bd, a.sB), BoG = (Bo + RAW_ROWS_PER_THREAD - 1) / RAW_ROWS_PER_THREAD;
    if (a.Cin == 1 && a.Cout == 24) {
        const size_t px = (size_t)a.B * Ao * Bo, nb = (px + RAW_THREADS - 1) / RAW_THREADS;
        if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(conv2d_strided_c1_kernel<24>, dim3((unsigned)nb), dim3(RAW_THREADS), 0, s, a, Ao, Bo, px);
        return hipGetLastError();
    }
    const size_t total = (size_t)a.B * Ao * BoG * a.Cout, blocks = (total + RAW_THREADS - 1) / RAW_THREADS;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv2d_strided_kernel, dim3((unsigned)blocks), dim3(RAW_THREADS), 0, s, a, Ao, Bo, BoG, total);
    return hipGetLastError();
}

hipError_t launch_conv1d_strided(const RawConvArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (a.L < 1 || a.Cin < 1 || a.Cout < 1 || a.k < 1 || !(a.k & 1) || a.stride < 1 || !a.w || !a.bias || !a.y) return hipErrorInvalidValue;
    const bool pcm = a.pcm != nullptr;
    // (pcm_stride < L: clips that overlap - the windows of a recording a hop apart; the kernel only reads samples [0, L) of each)
    if (pcm ? (a.Cin != 1 || a.pcm_stride < 1) : !a.x) return hipErrorInvalidValue;
    const int Lout = raw_conv_rows(a.L, a.stride);
    // the largest tile of output rows whose input window fits the LDS budget, and no larger than the clip needs
    int TT = 64;
    while (TT > RAW_ROWS_PER_THREAD && (((size_t)(TT - 1) * a.stride + a.k) * a.Cin * sizeof(float) > RAW_LDS_BYTES || TT / 2 >= Lout)) TT /= 2;
    const size_t lds = ((size_t)(TT - 1) * a.stride + a.k) * a.Cin * sizeof(float);
    if (lds > RAW_LDS_BYTES) return hipErrorInvalidValue;
    const int tiles = (Lout + TT - 1) / TT;
    if ((size_t)tiles * a.B > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((size_t)tiles * a.B)), block(RAW_THREADS);
    if (pcm)
        hipLaunchKernelGGL(conv1d_strided_kernel<true>, grid, block, lds, s, a.pcm, a.pcm_stride, nullptr, a.w, a.bias, a.y, a.L, Lout, a.Cin, a.Cout, a.k,
                           a.stride, TT, tiles, a.ct_out);
    else
        hipLaunchKernelGGL(conv1d_strided_kernel<false>, grid, block, lds, s, nullptr, (size_t)0, a.x, a.w, a.bias, a.y, a.L, Lout, a.Cin, a.Cout, a.k,
                           a.stride, TT, tiles, a.ct_out);
    return hipGetLastError();
}
