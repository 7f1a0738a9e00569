// qn_x3.h - the QuartzNet block in one clip-resident launch (qn_x3.hip), and the two small launches its generic plan adds.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

constexpr int QN_CK = 64;            // input channels per LDS chunk
constexpr int QN_MAX_T = 128, QN_MAX_C = 512, QN_MAX_K = 39;

struct QnArgs {
    const float* x = nullptr;               // [B][T][Cin] time-major (the head input, or the previous block's output)
    float* out = nullptr;                   // [B][T][Cout]; mean: [B][Cout], the time mean of the block's output
    const unsigned char* packed = nullptr;  // launch_qn_x3_pack's image of the folded [pointwise | projection] matrix
    const float* dw = nullptr;              // depthwise taps, tap-major [k][Cp], zeros past Cin
    const float* bias = nullptr;            // [Cout]: every bias and BatchNorm shift of the block folded into one row
    int B = 0, T = 0, Cin = 0, Cp = 0, Cout = 0, k = 0;   // Cp: Cin rounded up to 32
    int proj = 0;                           // 1: projected residual inside the contraction (K = 2 Cp); 0: + x in the epilogue (Cin == Cout)
    int mean = 0;
    float amax = 0.0f;                      // max over channels of sum_j |tap j|: |depthwise(x)[t]| <= amax max |x| over the taps' rows
    float w_un = 1.0f;                      // 1 / the packed image's power-of-two scale
};

bool qn_x3_supported(int T, int Cin, int Cout, int k);
// columns of the folded matrix [Cout][qn_x3_ktot]: per 64-channel chunk the pointwise columns, then (proj) the projection's
inline int qn_x3_cp(int Cin) { return (Cin + 31) / 32 * 32; }
inline int qn_x3_ktot(int Cin, int proj) { return qn_x3_cp(Cin) * (proj ? 2 : 1); }
inline int qn_x3_col(int Cin, int proj, int part, int ci) {      // part 0: pointwise (depthwise output ci), 1: projection (input ci)
    const int Cp = qn_x3_cp(Cin), c0 = ci / QN_CK * QN_CK, cw = Cp - c0 < QN_CK ? Cp - c0 : QN_CK;
    return c0 * (proj ? 2 : 1) + part * cw + (ci - c0);
}
size_t qn_x3_packed_bytes(int Cin, int Cout, int proj);
hipError_t launch_qn_x3_pack(const float* wcat, void* packed, int Cout, int Ktot, float ws, hipStream_t s);
// one workgroup per clip and 256 output channels, at most as many as the CUs hold at once (cu_count: the handle's)
hipError_t launch_qn_x3(const QnArgs& a, int cu_count, hipStream_t s);

// generic plan: y[b][t][c] = sum_j w[j][c] x[b][t + j - (k - 1) / 2][c], zeros outside the clip (no bias, BatchNorm or activation)
hipError_t launch_dwconv1d_same(const float* x, const float* w_t /*[k][ldw]*/, float* y, int B, int T, int C, int k, int ldw, hipStream_t s);
// y = relu(a + b)
hipError_t launch_add_relu(const float* a, const float* b, float* y, size_t n, hipStream_t s);
