// merge_x3.hip - the E-Branchformer block's merge of its two branches in one launch (EBranchformerBlock, architectures.py:564-594):
//     c = s Wc^T + bc            conv_branch.conv2 on the depthwise stage's output s = swish(BN(dw(...)))
//     g = sigmoid(c Wg^T + bg)   merger.gate, on the CONV branch's output
//     x <- LayerNorm(x + a g + c (1 - g); final_norm)
// row-local: a workgroup owns 64 rows (two 32-row tiles) and reads s, a, x once and writes x once; c and g never leave the chip.
//
// Both products are transposed as in lin_x3.hip / tcn_x3.hip: acc [32 outputs x 32 rows] += W[32 x 16] . X^T[16 x 32], three
// v_mfma_f32_32x32x16_f16 per product (hi.hi, hi.lo, lo.hi of two binary16 terms per operand), float32 accumulation.  Wave w owns
// output block w (32 channels; D = 144: five waves, the last block half empty) for BOTH row tiles, so a weight fragment read from
// global memory / L2 serves 64 rows; a lane holds 16 output channels of ONE row, so a row's arithmetic does not depend on where the row
// sits.  Neither s nor c has a plan-time bound: every row is multiplied by its own power of two (largest magnitude into [2^14, 2^15))
// before it is split into two binary16 terms, ONCE, into the LDS planes XH / XL that all waves read their B fragments from, and the
// accumulator is multiplied back per row.  c goes to an LDS float plane (the blend needs it), is re-scaled and re-split per row into the
// same planes for the second product; g then overwrites the planes (same size) and the last phase walks the rows wave by wave with
// coalesced reads of a and x: blend, residual, LayerNorm (layernorm_kernel's arithmetic: mean, then the centred squares), store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "layers.h"
#include "split_h2.h"
#include "merge_x3.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int MG_ROWS = 64;                                   // rows per workgroup: two 32-row tiles

__host__ __device__ constexpr int mg_nb(int D) { return (D + 31) / 32; }         // output blocks = waves
__host__ __device__ constexpr int mg_ldh(int D) { return D + 8; }                // XH / XL row pitch in halves = g's pitch in floats: 8 rows' 16-byte reads conflict-free
__host__ __device__ constexpr int mg_ldc(int D) { return D + 4; }                // c's row pitch in floats
__host__ __device__ constexpr size_t mg_lds_bytes(int D) { return (size_t)MG_ROWS * mg_ldh(D) * 4 + (size_t)MG_ROWS * mg_ldc(D) * 4 + 2 * MG_ROWS * 4; }

// fragment (cb, kb) of W [D][D] x ws: lane holds output 32 cb + (lane & 31), inputs 16 kb + 8 (lane >> 5) .. + 7; hi plane then lo plane
__global__ void __launch_bounds__(256) merge_pack_kernel(const float* __restrict__ W, unsigned char* __restrict__ out, int D, float ws) {
    const int K16 = D / 16;
    const size_t total = (size_t)mg_nb(D) * K16 * 64;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    const size_t f = idx >> 6;
    const int kb = (int)(f % K16), cb = (int)(f / K16);
    const int co = 32 * cb + (lane & 31), c0 = 16 * kb + 8 * (lane >> 5);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = co < D ? W[(size_t)co * D + c0 + e] * ws : 0.0f;
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) nww_split2h(v[2 * e], v[2 * e + 1], hi[e], lo[e]);
    unsigned char* dst = out + f * 2048 + (size_t)lane * 16;
    *reinterpret_cast<uint4*>(dst) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4*>(dst + 1024) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

__device__ __forceinline__ void mfma3h(uint4 wh, uint4 wl, uint4 xh, uint4 xl, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wl), __builtin_bit_cast(f16x8, xh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xh), acc, 0, 0, 0);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_add(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a row's four values of lane `lane` (columns 4 lane .. + 3; lanes past the row hold zeros) -> the row's exponent (largest magnitude's
// field, as lin_x3.hip / tcn_x3.hip), the values times the power of two that puts that magnitude in [2^14, 2^15) as two binary16 terms
template <int D>
__device__ __forceinline__ void split_row(float4 v, int lane, _Float16* xh_row, _Float16* xl_row, unsigned* eb_out) {
    const float m = wave_max(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    const uint32_t eb = min(max(__float_as_uint(m) >> 23, 16u), 254u);
    const float sc = __uint_as_float((268u - eb) << 23);
    if (4 * lane < D) {
        uint32_t h0, l0, h1, l1;
        nww_split2h(v.x * sc, v.y * sc, h0, l0);
        nww_split2h(v.z * sc, v.w * sc, h1, l1);
        *reinterpret_cast<uint2*>(xh_row + 4 * lane) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(xl_row + 4 * lane) = make_uint2(l0, l1);
    }
    if (lane == 0) *eb_out = eb;
}

// acc[rt] (output block `wave`, row tile rt) = W fragments of one matrix . the rows' split planes
template <int D>
__device__ __forceinline__ void product(const unsigned char* __restrict__ wfrag, const _Float16* XH, const _Float16* XL, int wave, int lane,
                                        f32x16 (&acc)[2]) {
    constexpr int K16 = D / 16, LDH = mg_ldh(D);
    const int n = lane & 31, h = lane >> 5;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[rt][e] = 0.0f;
    const unsigned char* wp = wfrag + (size_t)wave * K16 * 2048 + (size_t)lane * 16;
#pragma unroll
    for (int kb = 0; kb < K16; ++kb) {
        const uint4 wh = *reinterpret_cast<const uint4*>(wp + (size_t)kb * 2048), wl = *reinterpret_cast<const uint4*>(wp + (size_t)kb * 2048 + 1024);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const int off = (32 * rt + n) * LDH + 16 * kb + 8 * h;
            const uint4 xh = *reinterpret_cast<const uint4*>(XH + off), xl = *reinterpret_cast<const uint4*>(XL + off);
            mfma3h(wh, wl, xh, xl, acc[rt]);
        }
    }
}

template <int D>
__global__ void __launch_bounds__(64 * mg_nb(D)) merge_x3_kernel(MergeArgs a) {
    constexpr int NB = mg_nb(D), K16 = D / 16, LDH = mg_ldh(D), LDC = mg_ldc(D), D4 = D / 4;
    static_assert(D % 16 == 0 && D4 <= 64, "one float4 per lane and row");
    extern __shared__ __attribute__((aligned(16))) unsigned char mg_lds[];
    _Float16* XH = reinterpret_cast<_Float16*>(mg_lds);                        // [64][LDH] halves
    _Float16* XL = XH + MG_ROWS * LDH;
    float* G = reinterpret_cast<float*>(mg_lds);                               // [64][LDH] floats: the same bytes, after the second product
    float* C = reinterpret_cast<float*>(mg_lds + (size_t)MG_ROWS * LDH * 4);   // [64][LDC]
    unsigned* EBS = reinterpret_cast<unsigned*>(C + MG_ROWS * LDC);            // rows' exponents of s, then of c
    unsigned* EBC = EBS + MG_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const size_t row0 = (size_t)blockIdx.x * MG_ROWS;

    // ---- s rows -> scaled two-term planes (a wave per row, a float4 per lane; rows past M are zeros)
    // (eight rows requested before the first is reduced: one row at a time left a wave with a single load in flight)
    for (int rb = wave; rb < MG_ROWS; rb += 8 * NB) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = rb + j * NB;
            v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (lane < D4 && r < MG_ROWS && row0 + r < (size_t)a.M) v[j] = *reinterpret_cast<const float4*>(a.s + (row0 + r) * D + 4 * lane);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = rb + j * NB;
            if (r < MG_ROWS) split_row<D>(v[j], lane, XH + r * LDH, XL + r * LDH, EBS + r);
        }
    }
    __syncthreads();

    // ---- c = s Wc^T + bc -> C (float32)
    f32x16 acc[2];
    product<D>(a.packed, XH, XL, wave, lane, acc);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int lr = 32 * rt + n;
        const float un = __uint_as_float((EBS[lr] - 14u) << 23) * a.wc_un;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = 32 * wave + 8 * g + 4 * h;
            if (co < D) {
                const float4 b4 = *reinterpret_cast<const float4*>(a.bc + co);
                *reinterpret_cast<float4*>(C + lr * LDC + co) = make_float4(fmaf(acc[rt][4 * g], un, b4.x), fmaf(acc[rt][4 * g + 1], un, b4.y),
                                                                            fmaf(acc[rt][4 * g + 2], un, b4.z), fmaf(acc[rt][4 * g + 3], un, b4.w));
            }
        }
    }
    __syncthreads();                                                            // C complete; every wave is done with the planes of s

    // ---- c rows -> the planes, each row by its own power of two
    for (int r = wave; r < MG_ROWS; r += NB) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (lane < D4) v = *reinterpret_cast<const float4*>(C + r * LDC + 4 * lane);
        split_row<D>(v, lane, XH + r * LDH, XL + r * LDH, EBC + r);
    }
    __syncthreads();

    // ---- g = sigmoid(c Wg^T + bg) -> G, over the planes once every wave has read them
    product<D>(a.packed + (size_t)NB * K16 * 2048, XH, XL, wave, lane, acc);
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int lr = 32 * rt + n;
        const float un = __uint_as_float((EBC[lr] - 14u) << 23) * a.wg_un;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = 32 * wave + 8 * g + 4 * h;
            if (co < D) {
                const float4 b4 = *reinterpret_cast<const float4*>(a.bg + co);
                float z[4] = {fmaf(acc[rt][4 * g], un, b4.x), fmaf(acc[rt][4 * g + 1], un, b4.y), fmaf(acc[rt][4 * g + 2], un, b4.z), fmaf(acc[rt][4 * g + 3], un, b4.w)};
#pragma unroll
                for (int e = 0; e < 4; ++e) z[e] = 1.0f / (1.0f + expf(-z[e]));
                *reinterpret_cast<float4*>(G + lr * LDH + co) = make_float4(z[0], z[1], z[2], z[3]);
            }
        }
    }
    __syncthreads();

    // ---- x <- LayerNorm(x + a g + c (1 - g)), a wave per row
    float4 w4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), bb4 = w4;
    if (lane < D4) { w4 = *reinterpret_cast<const float4*>(a.ln_w + 4 * lane); bb4 = *reinterpret_cast<const float4*>(a.ln_b + 4 * lane); }
    for (int rb = wave; rb < MG_ROWS; rb += 4 * NB) {
        // four rows of x and a requested ahead of their arithmetic
        float4 xq[4], aq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = rb + j * NB;
            xq[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); aq[j] = xq[j];
            if (lane < D4 && r < MG_ROWS && row0 + r < (size_t)a.M) {
                xq[j] = *reinterpret_cast<const float4*>(a.x + (row0 + r) * D + 4 * lane);
                aq[j] = *reinterpret_cast<const float4*>(a.a + (row0 + r) * D + 4 * lane);
            }
        }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = rb + j * NB;
        if (r >= MG_ROWS || row0 + r >= (size_t)a.M) break;                     // wave-uniform
        float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float* xp = a.x + (row0 + r) * D + 4 * lane;
        if (lane < D4) {
            const float4 x4 = xq[j], a4 = aq[j];
            const float4 c4 = *reinterpret_cast<const float4*>(C + r * LDC + 4 * lane), g4 = *reinterpret_cast<const float4*>(G + r * LDH + 4 * lane);
            y[0] = x4.x + fmaf(a4.x, g4.x, c4.x * (1.0f - g4.x)); y[1] = x4.y + fmaf(a4.y, g4.y, c4.y * (1.0f - g4.y));
            y[2] = x4.z + fmaf(a4.z, g4.z, c4.z * (1.0f - g4.z)); y[3] = x4.w + fmaf(a4.w, g4.w, c4.w * (1.0f - g4.w));
        }
        const float mu = wave_add((y[0] + y[1]) + (y[2] + y[3])) / (float)D;
        float q = 0.0f;
        if (lane < D4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = y[e] - mu; q = fmaf(d, d, q); }
        }
        const float rstd = 1.0f / sqrtf(wave_add(q) / (float)D + 1e-5f);
        if (lane < D4)
            *reinterpret_cast<float4*>(xp) = make_float4((y[0] - mu) * rstd * w4.x + bb4.x, (y[1] - mu) * rstd * w4.y + bb4.y,
                                                         (y[2] - mu) * rstd * w4.z + bb4.z, (y[3] - mu) * rstd * w4.w + bb4.w);
      }
    }
}

template <int D>
hipError_t launch_instance(const MergeArgs& a, hipStream_t s) {
    constexpr size_t lds = mg_lds_bytes(D);
    static_assert(lds <= 160 * 1024, "the workgroup's planes exceed the LDS");
    const hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(&merge_x3_kernel<D>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(merge_x3_kernel<D>, dim3((unsigned)((a.M + MG_ROWS - 1) / MG_ROWS)), dim3(64 * mg_nb(D)), lds, s, a);
    return hipGetLastError();
}

}  // namespace

bool merge_x3_supported(int D) { return D == 32 || D == 64 || D == 96 || D == 128 || D == 144 || D == 192 || D == 256; }

size_t merge_x3_packed_bytes(int D) { return (size_t)2 * mg_nb(D) * (D / 16) * 2048; }

hipError_t launch_merge_x3_pack(const float* Wc, const float* Wg, void* packed, int D, float wsc, float wsg, hipStream_t s) {
    if (!merge_x3_supported(D)) return hipErrorInvalidValue;
    const size_t total = (size_t)mg_nb(D) * (D / 16) * 64;
    unsigned char* out = reinterpret_cast<unsigned char*>(packed);
    hipLaunchKernelGGL(merge_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, Wc, out, D, wsc);
    hipLaunchKernelGGL(merge_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, Wg, out + merge_x3_packed_bytes(D) / 2, D, wsg);
    return hipGetLastError();
}

hipError_t launch_merge_x3(const MergeArgs& a, int D, hipStream_t s) {
    if (a.M <= 0) return hipSuccess;
    switch (D) {
        case 32: return launch_instance<32>(a, s);
        case 64: return launch_instance<64>(a, s);
        case 96: return launch_instance<96>(a, s);
        case 128: return launch_instance<128>(a, s);
        case 144: return launch_instance<144>(a, s);
        case 192: return launch_instance<192>(a, s);
        case 256: return launch_instance<256>(a, s);
    }
    return hipErrorInvalidValue;
}
