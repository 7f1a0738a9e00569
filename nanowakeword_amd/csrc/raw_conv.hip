// raw_conv.hip - conv1d_strided: one stage of the raw-PCM frontend per launch.  A workgroup takes TT output rows of one clip: the input
// window ((TT - 1) stride + k rows, zeros outside the clip) is staged in LDS once, then every thread owns one output channel of four
// consecutive rows and walks the taps with float32 fmaf in a fixed order - a clip's result does not depend on its batch or slot.  The
// weights are tap-major [k][Cin][Cout], so the lanes of a wave read consecutive floats; the LDS reads of a row are broadcasts.
#include "raw_conv.h"

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

}  // namespace

hipError_t launch_conv1d_strided(const RawConvArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (a.L < 1 || a.Cin < 1 || a.Cout < 1 || a.k < 1 || !(a.k & 1) || a.stride < 1 || !a.w || !a.bias || !a.y) return hipErrorInvalidValue;
    const bool pcm = a.pcm != nullptr;
    if (pcm ? (a.Cin != 1 || a.pcm_stride < (size_t)a.L) : !a.x) return hipErrorInvalidValue;
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
