// layers.h - launchers of the classifier-head kernels (layers.hip).  All tensors float32, row-major,
// activations NCHW per clip like the reference's torch modules so flatten orders match the weights.
#pragma once
#include <hip/hip_runtime.h>
#include "rnn.h"

// Raise a kernel's dynamic-LDS limit once per (device, kernel).  The attribute is per device: a process that creates
// handles on several GPUs must set it on each of them, so the cache is keyed by the current device as well.
#include <map>
#include <mutex>
#include <utility>
inline hipError_t nww_allow_lds(const void* func, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    size_t& cur = done[std::make_pair(dev, func)];
    if (bytes > cur) {
        e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        cur = bytes;
    }
    return hipSuccess;
}

// SiLU of the fused conv epilogues: x / (1 + e^-x) on v_exp_f32 and v_rcp_f32 (5 instructions, ~3 ulp) instead of expf + an IEEE
// division (~20).  x = -inf .. -88: e^-x overflows to +inf, the reciprocal is +0, the result -0 (the true value is below 1e-36).
__device__ __forceinline__ float nww_silu(float v) {
    return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f));
}

// GELU of the fused epilogues, x Phi(x) with Phi(-t) = 2^P(t) for t = |x| (P = log2 of the normal tail: -1 + t R(t), R a degree-9
// polynomial fitted to 3e-8 in Phi over [0, 5.9]; below -126 the tail is zero like the reference's 1 + erf): 10 fma, v_exp_f32, a
// subtraction and a select - 15 instructions against 26 through a two-branch single-precision erf (and far fewer than the device library's erff, whose
// branches and temporaries cost the GELU instances of the trunk and the BcResNet front kernel 58-109 spilled registers: VERDICT r04 weak 11).  |error| <= 3.9e-7 up to |x| = 12 (the float32 form the
// reference evaluates, 0.5 x (1 + erf(x / sqrt 2)), is 4.5e-7 from exact on the same points: tools/erf_check.py).
__device__ __forceinline__ float nww_gelu(float x) {
    const float t = fabsf(x);
    float r = -1.7879411728927153e-08f;
    r = fmaf(r, t, 5.763639592260006e-07f);
    r = fmaf(r, t, -7.931240361358505e-06f);
    r = fmaf(r, t, 5.882469122298062e-05f);
    r = fmaf(r, t, -0.00021966989152133465f);
    r = fmaf(r, t, -0.00012137762678321451f);
    r = fmaf(r, t, 0.0070888083428144455f);
    r = fmaf(r, t, -0.05253036320209503f);
    r = fmaf(r, t, -0.45919492840766907f);
    r = fmaf(r, t, -1.151106595993042f);
    const float h = __builtin_amdgcn_exp2f(fmaxf(fmaf(r, t, -1.0f), -126.0f));
    return x * (x >= 0.0f ? 1.0f - h : h);
}

enum NwwAct { ACT_RELU = 0, ACT_GELU = 1, ACT_SILU = 2, ACT_NONE = 3, ACT_SIGMOID = 4, ACT_SWISH = 2 };

// C[M,N] = post( A[M,K] * W[N,K]^T ) with
//   v = acc + bias[n] (bias may be null); v = v*alpha[n] + beta[n] (alpha may be null: folded BatchNorm1d);
//   v = act(v); v = res[m*ldres+n] + rscale*v (res may be null).
// lda/ldc/ldres are row strides in floats (lda % 4 == 0 and A, W 16-byte aligned).
struct GemmArgs {
    const float* A; int lda;
    const float* W;            // [N][K], row stride K
    float* C; int ldc;
    int M, N, K;
    const float* bias; const float* alpha; const float* beta;
    int act;
    const float* res; int ldres; float rscale;
    // deterministic split-K: when splitk > 1, partial[z][M][N] go to splitk_ws and a second kernel adds them
    // in z order before the epilogue (bit-reproducible, unlike atomics). 0/1 = off.
    int splitk = 0; float* splitk_ws = nullptr;
    // split-K only: leave the partials in splitk_ws and skip the reduce launch - the consumer (the fused classifier tail)
    // sums them itself, in the same z order, and applies bias / BN / activation (nww_api.hip: Run::deferred)
    bool defer_reduce = false;
    // W pre-split into three bf16 terms ([N][ceil(K/16)][3][16], gemm_x3.hip); when set the contraction runs on the
    // bf16 matrix cores with exact operand splitting (float32-equivalent), else on v_mfma_f32_32x32x2_f32
    const void* Wx3 = nullptr;
    // h2 != 0: Wx3 holds TWO binary16 terms of W * (a power of two) ([N][ceil(K/16)][2][16], launch_split_weights_h2); A is
    // multiplied by a_scale (a power of two that keeps it inside the binary16 range) before it is split the same way, three
    // partial products per operand pair go to v_mfma_f32_32x32x16_f16 and the sums leave times c_scale = 1 / (a_scale x weight scale)
    // a_clamp > 0: A is clamped to +-a_clamp first (an ASSUMED bound - the head's input features; bounds derived from the weights hold by themselves)
    int h2 = 0; float a_scale = 1.0f, c_scale = 1.0f, a_clamp = 0.0f;
    // > 0 (split-operand kernel only): A is stored as [ceil(M/128)][a_blocked = K/32][128][32] tiles (written that way by
    // the fused conv trunk) instead of row-major - every tile load is one contiguous 16 KB block.  With row-major A
    // (row stride 51 KB for fc1) the same loads reach 2.5-2.9 TB/s (tools/ubench/strided_read.hip)
    int a_blocked = 0;
    // != 0 (NWW_GEMM_PP, the default): the bulk two-term split-K shape with blocked A and 128-column tiles (fc1 at M > 64) runs two row
    // tiles per 8-wave workgroup, each half staging under the other's MFMAs (gemm_x3.hip); 0: one row tile per 4-wave workgroup
    int pp = 0;
    // dual GEMM (BcResNet block): C = (A2 W2^T * alpha2 + beta2) + rscale * act((A W^T + bias) * alpha + beta), the second
    // product (shortcut branch) computed by the same workgroup instead of a separate GEMM + a residual round trip
    const float* A2 = nullptr; int lda2 = 0; const float* W2 = nullptr; int K2 = 0;
    const float* alpha2 = nullptr; const float* beta2 = nullptr;
};
size_t gemm_x3_weight_bytes(int N, int K);
// wave-specialised form (gemm_x3s.hip): producer waves stage + split, consumer waves multiply; same results bit for bit
hipError_t launch_split_weights_x3(const float* W, void* out, int N, int K, hipStream_t s);
hipError_t launch_split_weights_h2(const float* W, void* out, int N, int K, float scale, hipStream_t s);
bool gemm_x3_usable(const GemmArgs& g);
bool gemm_writes_partials(const GemmArgs& g);   // launch_gemm will take an MFMA kernel (split-K partials), not the VALU fallback
hipError_t launch_gemm_x3(const GemmArgs& g, hipStream_t s);
// rows(M) x N x K -> recommended split (1 = none); workspace floats needed = split*M*N
int gemm_recommended_splitk(long long M, int N, int K, int cu_count);
hipError_t launch_gemm(const GemmArgs& g, hipStream_t s);

// 3x3 conv, stride 1, pad 1 on NCHW + bias + (alpha,beta) + act, optionally followed by MaxPool2d(2) (floor).
// in [B][Cin][H][W] -> out [B][Cout][Ho][Wo], Ho = pool ? H/2 : H.
struct Conv3Args {
    const float* in; const float* w; const float* bias; const float* alpha; const float* beta;
    float* out; int B, Cin, Cout, H, W; int act; int pool;
    int nhwc_out = 0;     // 1: write [B][Ho][Wo][Cout] (channels last) instead of [B][Cout][Ho][Wo]
};
hipError_t launch_conv3x3(const Conv3Args& a, hipStream_t s);

// depthwise 3x3, pad 1, stride (sh, sw) on channels-last data: in [B][H][W][C], wt [9][C] (tap-major weights)
// -> d_out [B][Ho][Wo][C]; xs_out (may be null) receives in[b][oy*sh][ox*sw][c], the input of a strided 1x1 conv.
// act16 = 1 / 2 (nww_config.act_dtype): `in` and `d_out` are bf16 / scaled binary16 arrays, xs_out must be null; binary16: the sums
// are multiplied by out_mul = d_out's scale / in's scale before rounding
hipError_t launch_dwconv3x3_nhwc(const float* in, const float* wt, float* d_out, float* xs_out, int B, int C, int H,
                                 int W, int sh, int sw, hipStream_t s, int act16 = 0, float out_mul = 1.0f);
// rows [R][D]: y = act(LayerNorm(x)*w + b), eps 1e-5, biased variance; in place allowed (y == x)
// LayerNorm over x[row][i] = sum_z parts[z][row][i] + in_bias[i] (the split-K partials of the producing GEMM; D <= 256)
hipError_t launch_layernorm_parts(const float* parts, int nparts, size_t part_stride, const float* in_bias, float* y, const float* w,
                                  const float* b, int R, int D, int act, hipStream_t s);
hipError_t launch_layernorm(const float* x, float* y, const float* w, const float* b, int R, int D, int act,
                            hipStream_t s);
// mean over the middle axis: in [B][L][D] -> out [B][D]   (global average pools / mean over time)
// act16 = 1 / 2: `in` is a bf16 / scaled binary16 array (nww_config.act_dtype); binary16: the means are multiplied by unscale
hipError_t launch_mean_mid(const float* in, float* out, int B, int L, int D, hipStream_t s, int act16 = 0, float unscale = 1.0f);
// LayerNorm over D of every row of [B][L][D], then the mean over L -> out [B][D] (D <= 256)
hipError_t launch_ln_mean(const float* x, float* out, const float* w, const float* b, int B, int L, int D, hipStream_t s);
// AvgPool2d(kernel (kh,kw), stride (sh,sw)) on [B*C][H][W] -> [B*C][oh][ow]  (export form of AdaptiveAvgPool2d)
hipError_t launch_avgpool(const float* in, float* out, int BC, int H, int W, int kh, int kw, int sh, int sw, int oh,
                          int ow, hipStream_t s);
// y = act(x) elementwise (sigmoid for probabilities)
hipError_t launch_unary(const float* x, float* y, size_t n, int act, hipStream_t s);
// x [B][T][D] <- x * scale + pe[t][D] in place (the Transformer's input projection output, architectures.py:196-199; pe has >= T rows)
hipError_t launch_scale_add_pe(float* x, const float* pe, int B, int T, int D, float scale, hipStream_t s);
// GLU over the last axis: in [R][2D] -> out [R][D] = in[:, :D] * sigmoid(in[:, D:])
hipError_t launch_glu(const float* in, float* out, int R, int D, hipStream_t s);
// E-Branchformer merge + residual: x [n] += a g + c (1 - g), g = sigmoid(z) (the gate Linear's output); MergingModule, architectures.py:555-561
hipError_t launch_branch_merge(float* x, const float* a, const float* c, const float* z, size_t n, hipStream_t s);
// depthwise conv1d over time, 'same' padding, + bias, folded BN (alpha,beta), Swish: x [B][T][D] -> y [B][T][D]
hipError_t launch_dwconv1d_bn_swish(const float* x, const float* w /*[D][K]*/, const float* bias, const float* alpha,
                                    const float* beta, float* y, int B, int T, int D, int K, hipStream_t s);
// multi-head self-attention core: qkv [B][T][3D] (q|k|v) -> out [B][T][D]; softmax(q k^T / sqrt(dh)) v per head
hipError_t launch_mha_core(const float* qkv, float* out, int B, int T, int D, int n_head, hipStream_t s);
// the same on v_mfma_f32_32x32x2_f32 (mha_mfma.hip): T <= 128, head dim a multiple of 4 with a compiled instance
bool mha_mfma_supported(int T, int D, int n_head);
// head_major != 0: qkv is [q|k|v][B][n_head][T][D / n_head] (lin_x3's qkv store) instead of [B][T][3 D]; cus: the device's compute units
hipError_t launch_mha_mfma(const float* qkv, float* out, int B, int T, int D, int n_head, int cus, hipStream_t s, int head_major = 0);
bool mha_head_dim_supported(int head_dim);
// the same from two binary16 terms per operand on v_mfma_f32_32x32x16_f16 (mha_h2.hip; NWW_ARITH_F16X3): K, V scaled by the
// unit's own maxima, every query row by its own; the softmax subtracts the maximum from the raw scores before scaling them
bool mha_h2_supported(int T, int D, int n_head);
hipError_t launch_mha_h2(const float* qkv, float* out, int B, int T, int D, int n_head, int cus, hipStream_t s, int head_major = 0);
// [B][C][H][W] -> [B][W][C*H]  (CRNN: sequence over W, features C*H; architectures.py:272-276)
hipError_t launch_crnn_seq(const float* in, float* out, int B, int C, int H, int W, hipStream_t s);
// [B][R][C] -> [B][C][R]
hipError_t launch_transpose_planes(const float* in, float* out, int B, int R, int C, hipStream_t s);

// Tail of every head in ONE launch: emb = x We^T + be  (the head's last Linear, written to `emb`),
// hid = act(emb W0^T + b0), logit = hid . w3 + b3, prob = sigmoid(logit) when `probs` is set
// (Model.classifier, model.py:291-296; InferenceWrapper sigmoid, _export/onnx.py:164-172).  x [B][Kin], Kin <= 512, E <= 256.
struct TailArgs {
    const float* x; int Kin;
    const float *We, *be; int E;
    const float *W0, *b0, *w3, *b3;
    float *emb, *logits, *probs;
    int B, act;
    // x given as split-K partials of the producing GEMM: x[b][k] = in_act((sum_z parts[z][b][k] + in_bias[k]) * in_alpha[k] + in_beta[k]),
    // z ascending (gemm_splitk_reduce_kernel's order and epilogue, bit for bit)
    const float* parts = nullptr; int nparts = 0; size_t part_stride = 0;
    const float *in_bias = nullptr, *in_alpha = nullptr, *in_beta = nullptr; int in_act = 0;
    // completion word for the interpreter's small calls: when the launch is ONE workgroup (B <= 16), its last act is
    // *done_flag = done_seq (system scope, after the logits / probabilities) - the host polls it instead of paying the
    // runtime's stream synchronisation
    unsigned int* done_flag = nullptr; unsigned int done_seq = 0;
    // DNN head (Net, architectures.py:102-126) behind its first Linear, in the same launch: x <- act(LayerNorm(x; ln0_w, ln0_b)), then
    // n_mid times x <- act(LayerNorm(x mid_W[i]^T + mid_b[i]; mid_lnw[i], mid_lnb[i])) with [Kin][Kin] weights, then the tail above.
    // Used at EVERY batch size (a clip's logit must not depend on the batch it travels in); Kin <= 256, n_mid <= 4.
    const float *ln0_w = nullptr, *ln0_b = nullptr;
    int n_mid = 0;
    const float *mid_W[4] = {nullptr, nullptr, nullptr, nullptr}, *mid_b[4] = {nullptr, nullptr, nullptr, nullptr};
    const float *mid_lnw[4] = {nullptr, nullptr, nullptr, nullptr}, *mid_lnb[4] = {nullptr, nullptr, nullptr, nullptr};
    int cu_count = 256;    // the device's compute units: the grid of the large-batch kernel's persistent workgroups
};
bool tail_supported(int Kin, int E);
// true when launch_classifier_tail runs the large-batch kernel (persistent workgroups, weights in LDS) on this shape; nparts > 0: x arrives
// as that many split-K partials.  add_gemm defers its reduce to the tail by the SAME predicate.
bool tail_batch_runs(int B, int Kin, int E, bool dnn_body, int nparts);
hipError_t launch_classifier_tail(const TailArgs& a, hipStream_t s);
