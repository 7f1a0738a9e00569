// rnn.h - the recurrent layers (nn.GRU / nn.LSTM, one direction per launch): rnn_f32.hip, rnn_x3.hip, rnn_stream.hip.
#pragma once
#include <hip/hip_runtime.h>

// Recurrence for one direction. xg [B][T][gates H] = x W_ih^T + b_ih (precomputed by GEMM; gate order r, z, n / i, f, g, o).
// reverse=0: t = 0..T-1; reverse=1: t = T-1..0.  steps = number of steps to run (T, or 1 for the
// "last step of a reverse direction" shortcut).  seq_out (may be null) [B][T][ld_seq] receives h at
// column offset col_off for every visited t; last_out (may be null) [B][ld_last] at col_off gets the
// h after the final visited step... see rnn_f32.hip.
struct RnnArgs {
    const float* xg; const float* w_hh; const float* b_hh;
    float* seq_out; int ld_seq; float* last_out; int ld_last; int col_off;
    int B, T, H, reverse, steps;
    int products = 0;      // 6 / 9: recurrent product from split operands on the bf16 matrix cores (rnn_x3.hip), 0: float32 MFMA;
                           // 3: two binary16 terms per operand (h times 2^14 - |h| <= 1 - and W_hh times w_scale, a power of two)
    float w_scale = 1.0f;
    int gates;             // 3: GRU, 4: LSTM
    // rnn_x3 only: the FIRST step of the opposite direction (all that rnn_out[:, -1] needs of it; h = 0, so no recurrent product)
    // computed in the same launch from its gate pre-activations xg2 [B][xg2_bstride] and recurrent bias -> last_out[:, col_off2 + j]
    const float* xg2 = nullptr; size_t xg2_bstride = 0; const float* b_hh2 = nullptr; int col_off2 = 0;
    int ldw = 0;           // > 0: w_hh is the zero-padded [gates H][ldw] copy of launch_rnn_pad_weights -> the any-width kernel (H <= 512)
    // rnn_x3, products = 3, forward direction only: fin > 0 (GRU: 32 / 64; LSTM at H = 32 / 64: 32 / 64 / 96) fuses the INPUT projection
    // into the recurrence - xg is not read; the step's gate
    // pre-activations x_t W_ih^T + b_ih come from x_in [B][T][fin] (clamped to +-x_clamp, times x_scale) and w_ih [gates H][fin] (times
    // wi_scale) as two binary16 terms each, on the matrix pipe beside the recurrent product (the GRU head's 64 mel bins: no 635 MB
    // round trip of gate pre-activations through HBM)
    const float* x_in = nullptr; const float* w_ih = nullptr; const float* b_ih = nullptr;
    int fin = 0; float x_scale = 1.0f, x_clamp = 0.0f, wi_scale = 1.0f;
    // rnn_stream (128 < H <= 256, products = 3): W_hh x w_scale as two binary16 terms in MFMA fragment order (launch_rnn_stream_pack), read every step
    const void* w_packed = nullptr;
    int cu_count = 256;    // the device's compute units (rnn_stream: 16-clip tiles up to B = 16 x cu_count, 32-clip tiles beyond)
    int dbg = 0;           // NWW_ABLATION builds only (rnn_stream: phase-skipping for timing; results are garbage)
};
// picks the kernel: w_packed -> rnn_stream, ldw -> the any-width kernel, else rnn_x3 where usable, else the float32 kernels of rnn_f32.hip
hipError_t launch_rnn(const RnnArgs& a, hipStream_t s);
size_t rnn_wide_weight_bytes(int gates, int H);
hipError_t launch_rnn_pad_weights(const float* w_hh, float* out, int gates, int H, hipStream_t s);
// rnn_x3.hip: H in {32, 64, 128}
bool rnn_x3_usable(const RnnArgs& a);
hipError_t launch_rnn_x3(const RnnArgs& a, hipStream_t s);
// rnn_stream.hip: 128 < H <= 256 (H % 4 == 0), two-term form, W_hh streamed from L2 each step
bool rnn_stream_usable(const RnnArgs& a);
size_t rnn_stream_packed_bytes(int gates, int H);
hipError_t launch_rnn_stream_pack(const float* w_hh, void* packed, int gates, int H, float w_scale, hipStream_t s);
hipError_t launch_rnn_stream(const RnnArgs& a, hipStream_t s);
