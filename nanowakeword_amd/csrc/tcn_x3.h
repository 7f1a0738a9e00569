// tcn_x3.h - the TCN head's TemporalBlock stack (tcn_x3.hip): one clip-resident launch over the last step's receptive-field cone in the
// two-term binary16 arithmetic, and the pieces of the generic fallback (causal im2col, last-row gather)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#define TCN_MAX_LEVELS 4

struct TcnConv {
    const unsigned char* packed = nullptr;    // launch_tcn_x3_pack output; null: no such conv (identity residual)
    const float* bias = nullptr;              // [Cout]
    float w_un = 1.0f;                        // 1 / the weight's power-of-two scale
};

struct TcnArgs {
    const float* x = nullptr;                 // [B][T][F] features
    float* out = nullptr;                     // [B][ch[L - 1]]: the last block's output at t = T - 1
    int B = 0, T = 0, F = 0;
    int S = 0;                                // time steps kept per clip: the last S, S = min(T, receptive field)
    int NC = 0;                               // clips per workgroup (NC S <= 32 RT rows)
    int RT = 0;                               // 32-row tiles per workgroup (filled by tcn_x3_plan)
    int L = 0, k = 0;                         // levels, kernel size (level i: dilation 2^i)
    int cin0 = 0;                             // F rounded up to a multiple of 16
    int ch[TCN_MAX_LEVELS] = {0, 0, 0, 0};
    int ld = 0;                               // LDS row stride (floats)
    TcnConv c1[TCN_MAX_LEVELS], c2[TCN_MAX_LEVELS], ds[TCN_MAX_LEVELS];
};

// 1 + 2 (k - 1) (2^L - 1): the time steps of the input that the last step's output depends on
int tcn_receptive_field(int L, int k);
// fills S / NC / RT / cin0 / ld of a for the shape in a (T, F, L, k, ch); false: the fused kernel does not take this shape
bool tcn_x3_plan(TcnArgs& a);
size_t tcn_x3_packed_bytes(int Cin, int Cout, int taps);
// W [Cout][Cin][taps] float32 (nn.Conv1d) -> [Cout / 32][taps][ceil(Cin / 16)][2 terms][64 lanes] 16-byte fragments of W x ws
hipError_t launch_tcn_x3_pack(const float* W, void* out, int Cin, int Cout, int taps, float ws, hipStream_t s);
hipError_t launch_tcn_x3(const TcnArgs& a, hipStream_t s);

// fallback: col[(b T + t)][ci k + j] = x[b][t - (k - 1 - j) dil][ci], 0 before the clip (the layout of W [Cout][Cin][k] read as [Cout][Cin k])
hipError_t launch_tcn_im2col(const float* x, float* col, int B, int T, int C, int k, int dil, hipStream_t s);
// out[b][c] = y[b][T - 1][c]
hipError_t launch_tcn_last_row(const float* y, float* out, int B, int T, int C, hipStream_t s);
