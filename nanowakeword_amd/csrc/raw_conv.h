// raw_conv.h - the learned raw-PCM frontend (RawAudioFrontend, architectures.py:692-710): zero-padded strided Conv1d stages with the
// BatchNorm folded into weights and bias and ReLU in the epilogue (raw_conv.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

struct RawConvArgs {
    const int16_t* pcm = nullptr;   // stage 0: int16 samples, pcm_stride samples between clips (clips may overlap: pcm_stride < L); the kernel reads sample / 32768 (exact in float32)
    size_t pcm_stride = 0;
    const float* x = nullptr;       // later stages: time-major rows [B][L][Cin]
    const float* w = nullptr;       // folded weights, tap-major [k][Cin][Cout]
    const float* bias = nullptr;    // folded bias [Cout]
    float* y = nullptr;             // [B][Lout][Cout], or [B][Cout][Lout] with ct_out
    int B = 0, L = 0, Cin = 1, Cout = 0, k = 0, stride = 1, ct_out = 0;
};
// rows a stage yields: (L - 1) / stride + 1 for the odd kernels padded by k / 2 zeros each side
inline int raw_conv_rows(int L, int stride) { return L < 1 ? 0 : (L - 1) / stride + 1; }
hipError_t launch_conv1d_strided(const RawConvArgs& a, hipStream_t s);
