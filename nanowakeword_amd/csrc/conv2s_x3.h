// conv2s_x3.h - zero-padded 3x3 convolution, stride 1 or 2 per axis, on channels-last planes (RawAudioBackbone, architectures.py:739-776).
// A clip's plane is [A][Bd][C]: A the outer axis, Bd the middle one, the channels innermost.  The raw-PCM frontend writes its output
// time-major [rows][width], which is the reference's one-channel image [H = width][W = rows] transposed: A is the image's W (time), Bd its
// H, and the 3x3 weights are transposed once at nww_finalize instead of the data.  Output extent per axis: (n - 1) / stride + 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "layers.h"

// the backbone's activation behind the folded BatchNorm (nww_config.activation), shared by both routes
__device__ __forceinline__ float conv2s_act(float v, int act) {
    return act == ACT_RELU ? fmaxf(v, 0.0f) : act == ACT_GELU ? nww_gelu(v) : act == ACT_SILU ? nww_silu(v) : v;
}

inline int conv2s_out(int n, int stride) { return (n - 1) / stride + 1; }

// conv2d_strided (raw_conv.hip): float32 on the VALU, one launch per layer, any Cin / Cout / stride 1-2 / A / Bd >= 1.  w is tap-major
// [3 (A)][3 (Bd)][Cin][Cout] with the BatchNorm folded in, bias [Cout] its shift; y = act(bias + sum) in a fixed fmaf order.
struct Conv2sArgs {
    const float* x = nullptr; float* y = nullptr;
    const float *w = nullptr, *bias = nullptr;
    int B = 0, A = 0, Bd = 0, Cin = 0, Cout = 0, sA = 1, sB = 1, act = 0;
};
hipError_t launch_conv2d_strided(const Conv2sArgs& a, hipStream_t s);

// conv2s_x3 (conv2s_x3.hip): the same layer as an implicit GEMM on v_mfma_f32_32x32x16_f16 from two binary16 terms per operand.
// packed: launch_qn_x3_pack's fragment order of the folded [CoutP][9 Cp] weights (tap-major columns, Cin padded to Cp = a multiple of 16
// with zero columns, Cout padded to CoutP = a multiple of 32 with zero rows), every row already times its own power of two; w_un [CoutP]
// undoes it in the epilogue.  The input tile's power of two comes from the tile's own largest magnitude inside the kernel.
struct Conv2sX3Args {
    const float* x = nullptr; float* y = nullptr;
    const unsigned char* packed = nullptr;
    const float *w_un = nullptr, *bias = nullptr;
    int B = 0, A = 0, Bd = 0, Cin = 0, Cout = 0, stride = 1, act = 0;
};
bool conv2s_x3_supported(int Cin, int Cout, int sA, int sB);
inline int conv2s_x3_cp(int Cin) { return (Cin + 15) / 16 * 16; }
inline int conv2s_x3_coutp(int Cout) { return (Cout + 31) / 32 * 32; }
inline size_t conv2s_x3_packed_bytes(int Cin, int Cout) { return (size_t)(conv2s_x3_coutp(Cout) / 32) * (9 * conv2s_x3_cp(Cin) / 16) * 2048; }
size_t conv2s_x3_lds_bytes(int Cin, int stride);
hipError_t launch_conv2s_x3(const Conv2sX3Args& a, hipStream_t s);
