// conv2s_x3.hip - one layer of the RawAudioBackbone (Conv2d 3x3, pad 1, stride 1 or 2 on both axes, folded BatchNorm, activation) per
// launch, as an implicit GEMM on v_mfma_f32_32x32x16_f16.  Planes are channels-last [A][Bd][C] per clip (conv2s_x3.h).
//
// A workgroup (4 waves) takes one clip's tile of TA (A) x 16 (Bd) output pixels and every output channel - TA = 8 at stride 1, 4 at
// stride 2, where the halo is four times the tile and a smaller tile lets two or three workgroups share a CU's LDS; the tiling depends on
// the plane's extents only, never on the batch or the device, so a clip's bits do not depend on its batch or slot.  The input halo tile -
// ((TA - 1) s + 3) x ((16 - 1) s + 3) pixels, zeros outside the image (that IS the padding) - is read from float32 twice: once for the
// tile's largest magnitude, once to stage it in LDS as two binary16 planes [pixel][Cp + 8] (hi, lo of value x 2^e, e the power of two
// that puts the tile's maximum in [2^14, 2^15); an all-zero tile takes 1).  Nothing is clamped and no bound is assumed: the scale is
// the data's own.  The second read hits the cache.
//
// The product is transposed as in qn_x3.hip: acc [32 outputs x 32 pixels] += W [32 x 16] . X^T [16 x 32], K = 9 taps x Cp channels
// tap-major, so a 16-wide K-chunk stays inside one tap and the B fragment of lane (n, h) is 16 bytes at pixel (n under the tap), channel
// 16 c16 + 8 h.  A wave owns one row tile of 32 pixels (two A positions x 16 Bd positions) and NCBW output blocks: at TA = 8 the four
// waves are the four row tiles and each takes ALL output blocks, at TA = 4 two waves share a row tile and split the two blocks.  The X
// fragments are read from LDS once per K-chunk and meet NCBW weight fragments, which come from the packed image in launch_qn_x3_pack's
// order (hi plane, lo plane; one coalesced 1 KB read each).  Three products per chunk, small terms first.  The weights carry one power
// of two per OUTPUT CHANNEL (folded at nww_finalize), which the epilogue's fma undoes together with the tile's, then bias, activation and
// a float32 store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "layers.h"
#include "split_h2.h"
#include "conv2s_x3.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int C2_TB = 16, C2_THREADS = 256;
__host__ __device__ constexpr int c2_ta(int s) { return s == 1 ? 8 : 4; }

__host__ __device__ constexpr int c2_halo(int tile, int s) { return (tile - 1) * s + 3; }
__host__ __device__ constexpr size_t c2_lds_bytes(int CP, int S) {
    return (size_t)c2_halo(c2_ta(S), S) * c2_halo(C2_TB, S) * (CP + 8) * 2 * 2 + 32;
}

__device__ __forceinline__ void mfma3h(uint4 wh, uint4 wl, uint4 xh, uint4 xl, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wl), __builtin_bit_cast(f16x8, xh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xh), acc, 0, 0, 0);
}

template <int CP, int NCB, int S>
__global__ void __launch_bounds__(C2_THREADS) conv2s_x3_kernel(Conv2sX3Args a, int Ao, int Bo, int tilesA, int tilesB) {
    constexpr int C2_TA = c2_ta(S), RT = C2_TA / 2, NCBW = NCB * RT / 4;      // row tiles of 32 pixels; output blocks per wave
    static_assert(4 % RT == 0 && (NCB * RT) % 4 == 0, "the waves must divide the row tiles and the output blocks");
    constexpr int HA = c2_halo(C2_TA, S), HB = c2_halo(C2_TB, S), NPIX = HA * HB, PITCH = CP + 8, C16 = CP / 16, K16 = 9 * C16, CG = CP / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char c2_lds[];
    _Float16* XH = reinterpret_cast<_Float16*>(c2_lds);                 // [NPIX][PITCH] each
    _Float16* XL = XH + NPIX * PITCH;
    float* RED = reinterpret_cast<float*>(XL + NPIX * PITCH);           // the waves' maxima
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const int tb = blockIdx.x % tilesB, ta = (blockIdx.x / tilesB) % tilesA, b = blockIdx.x / (tilesB * tilesA);
    const int a0 = ta * C2_TA, b0 = tb * C2_TB, inA0 = a0 * S - 1, inB0 = b0 * S - 1;
    const int A = a.A, Bd = a.Bd, Cin = a.Cin, Cout = a.Cout;
    const float* xb = a.x + (size_t)b * A * Bd * Cin;

    // ---- the tile's largest magnitude
    float mx = 0.0f;
    for (int idx = tid; idx < NPIX * CG; idx += C2_THREADS) {
        const int pix = idx / CG, c = 4 * (idx - pix * CG), la = pix / HB, ga = inA0 + la, gb = inB0 + (pix - la * HB);
        if (ga >= 0 && ga < A && gb >= 0 && gb < Bd && c < Cin) {
            const float4 v = *reinterpret_cast<const float4*>(xb + ((size_t)ga * Bd + gb) * Cin + c);
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) RED[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(RED[0], RED[1]), fmaxf(RED[2], RED[3]));
    // biased exponent of the maximum: x 2^(141 - eb) lands in [2^14, 2^15); zero -> 141 (scale 1)
    const unsigned eb = mx == 0.0f ? 141u : min(max(__float_as_uint(mx) >> 23, 16u), 254u);
    const float sc = __uint_as_float((268u - eb) << 23);

    // ---- stage the halo tile as two binary16 planes
    for (int idx = tid; idx < NPIX * CG; idx += C2_THREADS) {
        const int pix = idx / CG, c = 4 * (idx - pix * CG), la = pix / HB, ga = inA0 + la, gb = inB0 + (pix - la * HB);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ga >= 0 && ga < A && gb >= 0 && gb < Bd && c < Cin) v = *reinterpret_cast<const float4*>(xb + ((size_t)ga * Bd + gb) * Cin + c);
        uint32_t h0, l0, h1, l1;
        nww_split2h(v.x * sc, v.y * sc, h0, l0);
        nww_split2h(v.z * sc, v.w * sc, h1, l1);
        *reinterpret_cast<uint2*>(XH + pix * PITCH + c) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(XL + pix * PITCH + c) = make_uint2(l0, l1);
    }
    __syncthreads();

    // ---- the contraction: 9 taps x CP / 16 chunks, three products each
    const int al = 2 * (wave % RT) + (n >> 4), bl = n & 15, cb0 = (wave / RT) * NCBW;
    f32x16 acc[NCBW];
#pragma unroll
    for (int i = 0; i < NCBW; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;
    const unsigned char* wp = a.packed + (size_t)lane * 16;
    for (int t = 0; t < 9; ++t) {
        const int tA = t / 3, tB = t - 3 * tA;
        const int off = ((al * S + tA) * HB + bl * S + tB) * PITCH + 8 * h;
#pragma unroll
        for (int c16 = 0; c16 < C16; ++c16) {
            const uint4 xh = *reinterpret_cast<const uint4*>(XH + off + 16 * c16), xl = *reinterpret_cast<const uint4*>(XL + off + 16 * c16);
            const int kb = t * C16 + c16;
#pragma unroll
            for (int i = 0; i < NCBW; ++i) {
                const unsigned char* f = wp + ((size_t)(cb0 + i) * K16 + kb) * 2048;
                mfma3h(*reinterpret_cast<const uint4*>(f), *reinterpret_cast<const uint4*>(f + 1024), xh, xl, acc[i]);
            }
        }
    }

    // ---- epilogue: both powers of two back, bias, activation; a lane holds 16 output channels per block of ONE pixel
    const int ao = a0 + al, bo = b0 + bl;
    if (ao < Ao && bo < Bo) {
        const float un = __uint_as_float((eb - 14u) << 23);
        float* yp = a.y + (((size_t)b * Ao + ao) * Bo + bo) * Cout;
#pragma unroll
        for (int i = 0; i < NCBW; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = 32 * (cb0 + i) + 8 * g + 4 * h;
                if (co < Cout) {
                    const float4 u4 = *reinterpret_cast<const float4*>(a.w_un + co), b4 = *reinterpret_cast<const float4*>(a.bias + co);
                    float4 y;
                    y.x = conv2s_act(fmaf(acc[i][4 * g] * un, u4.x, b4.x), a.act);
                    y.y = conv2s_act(fmaf(acc[i][4 * g + 1] * un, u4.y, b4.y), a.act);
                    y.z = conv2s_act(fmaf(acc[i][4 * g + 2] * un, u4.z, b4.z), a.act);
                    y.w = conv2s_act(fmaf(acc[i][4 * g + 3] * un, u4.w, b4.w), a.act);
                    *reinterpret_cast<float4*>(yp + co) = y;
                }
            }
    }
}

template <int CP, int NCB, int S>
hipError_t launch_instance(const Conv2sX3Args& a, hipStream_t s) {
    constexpr size_t lds = c2_lds_bytes(CP, S);
    static_assert(lds <= 160 * 1024, "the halo tile exceeds the LDS");
    const hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(&conv2s_x3_kernel<CP, NCB, S>), lds);
    if (e != hipSuccess) return e;
    const int Ao = conv2s_out(a.A, S), Bo = conv2s_out(a.Bd, S);
    constexpr int C2_TA = c2_ta(S);
    const int tilesA = (Ao + C2_TA - 1) / C2_TA, tilesB = (Bo + C2_TB - 1) / C2_TB;
    const size_t grid = (size_t)a.B * tilesA * tilesB;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((conv2s_x3_kernel<CP, NCB, S>), dim3((unsigned)grid), dim3(C2_THREADS), lds, s, a, Ao, Bo, tilesA, tilesB);
    return hipGetLastError();
}

}  // namespace

// the backbone's three instances: (Cin, Cout, stride) = (24, 48, 2), (48, 64, 2), (64, 96, 1)
bool conv2s_x3_supported(int Cin, int Cout, int sA, int sB) {
    return sA == sB && ((Cin == 24 && Cout == 48 && sA == 2) || (Cin == 48 && Cout == 64 && sA == 2) || (Cin == 64 && Cout == 96 && sA == 1));
}

size_t conv2s_x3_lds_bytes(int Cin, int stride) { return c2_lds_bytes(conv2s_x3_cp(Cin), stride); }

hipError_t launch_conv2s_x3(const Conv2sX3Args& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (!conv2s_x3_supported(a.Cin, a.Cout, a.stride, a.stride) || a.A < 1 || a.Bd < 1 || !a.x || !a.y || !a.packed || !a.w_un || !a.bias) return hipErrorInvalidValue;
    if (a.Cin == 24) return launch_instance<32, 2, 2>(a, s);
    if (a.Cin == 48) return launch_instance<48, 2, 2>(a, s);
    return launch_instance<64, 3, 1>(a, s);
}
