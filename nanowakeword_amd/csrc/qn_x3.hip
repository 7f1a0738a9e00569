// qn_x3.hip - one QuartzNetBlock (architectures.py:370-407) per launch, a clip resident in a workgroup:
//     d = depthwise(x)  (k taps over time, zero padding 'same', bias folded away)      float32 on the VALU, from LDS
//     y = relu([d | x] . [W_pw' ; W_res']^T + b)     projected residual: one contraction over K = 2 Cin
//     y = relu(d . W_pw'^T + b + x)                  identity residual (Cin == Cout): K = Cin, x added in the float32 epilogue
// W_pw' / W_res' carry their BatchNorms and b every bias (folded in float64 at plan time, nww_plan.hip).  The last block writes the
// time mean of y instead of y.
//
// The product is transposed as in merge_x3.hip / lin_x3.hip: acc [32 outputs x 32 rows] += W[32 x 16] . X^T[16 x 32], three
// v_mfma_f32_32x32x16_f16 per step (hi.hi, hi.lo, lo.hi of two binary16 terms per operand), float32 accumulation; a lane holds 16 output
// channels of ONE row.  A workgroup (8 waves) takes one clip and up to 256 output channels (blockIdx.y: the second half of Cout = 512,
// which stages and filters the clip a second time - 6 % of its matrix work); wave w owns output block w for all row tiles (Cout >= 160),
// or shares a block's row tiles with other waves when there are fewer blocks than waves.
//
// Input channels go through LDS in chunks of 64: the chunk's rows as float32 with a zero halo of k - 1 rows (XF), its taps (WD), and four
// binary16 planes [rows][64 + 8] - the two terms of d and of x.  Every row t has ONE power of two for both operands, from a bound that
// needs no second pass over d:  |d[t][c]| <= amax max_{rows under the taps} max_c |x|,  bound[t] = max(max_c |x[t]|, that); the bound's
// exponent puts it in [2^14, 2^15) (no clamp anywhere; the row's accumulator is multiplied back in the epilogue).  The bound depends on
// the clip's own rows only, so a clip's result does not depend on its batch or slot.
//
// LDS lanes: XF's pitch is 64 dwords; a depthwise lane reads 16 bytes at (row, 4 (lane & 15)) and the four 16-lane
// quarters of a wave read rows 4 apart, so each ds_read_b128 lane group {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} covers banks 0-63 once.
// The planes' pitch is 36 dwords: the B fragment of lane (n, h) sits at row n, 16 bytes from column 16 kb + 8 h, and the 16 rows of a lane
// group start at 16 different multiples of 4 banks (merge_x3.hip's layout).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "layers.h"
#include "split_h2.h"
#include "qn_x3.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int QN_LDH = QN_CK + 8;     // plane row pitch in halves
constexpr int QN_DS = 4;              // steps a depthwise lane owns
constexpr int QN_HALO = 48;           // XF rows beyond the tile rows: k - 1 <= 38 halo rows and the QN_DS-row look-ahead of the filter's ring
constexpr int QN_WD_ROWS = 40;
constexpr int QN_THREADS = 512;

__host__ __device__ constexpr size_t qn_lds_bytes(int RT) {
    return (size_t)(32 * RT + QN_HALO) * QN_CK * 4 + (size_t)QN_WD_ROWS * QN_CK * 4 + (size_t)4 * 32 * RT * QN_LDH * 2 + (size_t)2 * 32 * RT * 4 +
           (size_t)RT * 256 * 4;
}

// fragment (cb, kb) of W [Cout][Ktot] x ws: lane holds output 32 cb + (lane & 31), inputs 16 kb + 8 (lane >> 5) .. + 7; hi plane then lo plane
__global__ void __launch_bounds__(256) qn_pack_kernel(const float* __restrict__ W, unsigned char* __restrict__ out, int Cout, int Ktot, float ws) {
    const int K16 = Ktot / 16;
    const size_t total = (size_t)(Cout / 32) * K16 * 64;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    const size_t f = idx >> 6;
    const int kb = (int)(f % K16), cb = (int)(f / K16);
    const int co = 32 * cb + (lane & 31), c0 = 16 * kb + 8 * (lane >> 5);
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) nww_split2h(W[(size_t)co * Ktot + c0 + 2 * e] * ws, W[(size_t)co * Ktot + c0 + 2 * e + 1] * ws, hi[e], lo[e]);
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

__device__ __forceinline__ float4 f4_fma(float4 w, float4 x, float4 a) {
    return make_float4(fmaf(w.x, x.x, a.x), fmaf(w.y, x.y, a.y), fmaf(w.z, x.z, a.z), fmaf(w.w, x.w, a.w));
}

// four values times sc -> two binary16 terms each, 8 bytes into each plane
__device__ __forceinline__ void split4(float4 v, float sc, _Float16* ph, _Float16* pl) {
    uint32_t h0, l0, h1, l1;
    nww_split2h(v.x * sc, v.y * sc, h0, l0);
    nww_split2h(v.z * sc, v.w * sc, h1, l1);
    *reinterpret_cast<uint2*>(ph) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(pl) = make_uint2(l0, l1);
}

template <int RT>
__global__ void __launch_bounds__(QN_THREADS) qn_x3_kernel(QnArgs a) {
    constexpr int TP = 32 * RT, XR = TP + QN_HALO;
    extern __shared__ __attribute__((aligned(16))) unsigned char qn_lds[];
    float* XF = reinterpret_cast<float*>(qn_lds);                                  // [XR][64]: row r is time r - padL
    float* WD = XF + XR * QN_CK;                                                   // [40][64]
    _Float16* DH = reinterpret_cast<_Float16*>(WD + QN_WD_ROWS * QN_CK);          // [TP][72] each
    _Float16* DL = DH + TP * QN_LDH;
    _Float16* XH = DL + TP * QN_LDH;
    _Float16* XL = XH + TP * QN_LDH;
    float* MX = reinterpret_cast<float*>(XL + TP * QN_LDH);                        // rows' largest |x|
    unsigned* EB = reinterpret_cast<unsigned*>(MX + TP);                           // rows' exponents
    float* PS = reinterpret_cast<float*>(EB + TP);                                 // [RT][256]: row tiles' sums over time (mean)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const int T = a.T, k = a.k, padL = (k - 1) / 2, Cin = a.Cin, Cp = a.Cp, Cout = a.Cout;
    const int m = a.proj ? 2 : 1, K16tot = Cp / 16 * m;
    const int cb0 = 8 * blockIdx.y, NCB = min(8, Cout / 32 - cb0);
    const int WPC = NCB >= 5 ? 1 : NCB >= 3 ? 2 : NCB == 2 ? 4 : 8;               // waves per output block
    const int cbl = wave / WPC, sub = wave % WPC;
    const bool mma = cbl < NCB;

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float* xb = a.x + (size_t)b * T * Cin;
        // ---- rows' largest magnitudes over ALL input channels, then each row's bound and exponent
        for (int t = wave; t < TP; t += QN_THREADS / 64) {
            float mx = 0.0f;
            if (t < T)
                for (int c = 4 * lane; c < Cin; c += 256) {
                    const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)t * Cin + c);
                    mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
                }
            mx = wave_max(mx);
            if (lane == 0) MX[t] = mx;
        }
        __syncthreads();
        if (tid < TP) {
            float bnd = 0.0f;
            if (tid < T) {
                float w = 0.0f;
                const int lo = max(0, tid - padL), hi = min(T - 1, tid + (k - 1 - padL));
                for (int t = lo; t <= hi; ++t) w = fmaxf(w, MX[t]);
                bnd = fmaxf(MX[tid], a.amax * w);
            }
            EB[tid] = min(max(__float_as_uint(bnd) >> 23, 16u), 254u);
        }
        __syncthreads();

        f32x16 acc[RT];
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;

        for (int c0 = 0; c0 < Cp; c0 += QN_CK) {
            const int cw = min(QN_CK, Cp - c0);
            // ---- stage the chunk: rows with their zero halo, the taps, and (projection) the scaled two-term planes of x
            for (int idx = tid; idx < XR * 16; idx += QN_THREADS) {
                const int r = idx >> 4, cg = idx & 15, t = r - padL, c = c0 + 4 * cg;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (t >= 0 && t < T && c < Cin) v = *reinterpret_cast<const float4*>(xb + (size_t)t * Cin + c);
                *reinterpret_cast<float4*>(XF + r * QN_CK + 4 * cg) = v;
            }
            for (int idx = tid; idx < k * 16; idx += QN_THREADS) {
                const int j = idx >> 4, cg = idx & 15, c = c0 + 4 * cg;
                float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (c < Cp) w = *reinterpret_cast<const float4*>(a.dw + (size_t)j * Cp + c);
                *reinterpret_cast<float4*>(WD + j * QN_CK + 4 * cg) = w;
            }
            if (a.proj)
                for (int idx = tid; idx < TP * 16; idx += QN_THREADS) {
                    const int t = idx >> 4, cg = idx & 15, c = c0 + 4 * cg;
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (t < T && c < Cin) v = *reinterpret_cast<const float4*>(xb + (size_t)t * Cin + c);
                    split4(v, __uint_as_float((268u - EB[t]) << 23), XH + t * QN_LDH + 4 * cg, XL + t * QN_LDH + 4 * cg);
                }
            __syncthreads();

            // ---- depthwise: a lane owns 4 channels of QN_DS consecutive steps; the rows under tap j sit in a register ring, so a tap costs one
            // row read and one tap read per 4 QN_DS multiply-adds.  TP / QN_DS * 16 items: all 512 threads at T > 64
            for (int item = tid; item < (TP / QN_DS) * 16; item += QN_THREADS) {
                const int cg = item & 15, t0 = QN_DS * (item >> 4);
                float4 o[QN_DS];
#pragma unroll
                for (int q = 0; q < QN_DS; ++q) o[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (t0 < T) {
                    const float* xp = XF + t0 * QN_CK + 4 * cg;
                    float4 ring[QN_DS];
#pragma unroll
                    for (int q = 0; q < QN_DS; ++q) ring[q] = *reinterpret_cast<const float4*>(xp + q * QN_CK);
                    for (int jb = 0; jb < k; jb += QN_DS) {
#pragma unroll
                        for (int jj = 0; jj < QN_DS; ++jj) {
                            const int j = jb + jj;
                            if (j < k) {
                                const float4 w = *reinterpret_cast<const float4*>(WD + j * QN_CK + 4 * cg);
#pragma unroll
                                for (int q = 0; q < QN_DS; ++q) o[q] = f4_fma(w, ring[(q + jj) % QN_DS], o[q]);
                                ring[jj] = *reinterpret_cast<const float4*>(xp + (j + QN_DS) * QN_CK);  // row t0 + j is done with: t0 + j + QN_DS takes its slot
                            }
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < QN_DS; ++q) {
                    const int t = t0 + q;
                    const float4 v = t < T ? o[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    split4(v, __uint_as_float((268u - EB[t]) << 23), DH + t * QN_LDH + 4 * cg, DL + t * QN_LDH + 4 * cg);
                }
            }
            __syncthreads();

            // ---- the chunk's steps of the contraction: the d columns, then (projection) the x columns
            if (mma) {
                const int nk = cw / 16;
                const unsigned char* wp = a.packed + ((size_t)(cb0 + cbl) * K16tot + (size_t)(c0 / 16) * m) * 2048 + (size_t)lane * 16;
                for (int kb = 0; kb < nk * m; ++kb) {
                    const uint4 wh = *reinterpret_cast<const uint4*>(wp + (size_t)kb * 2048), wl = *reinterpret_cast<const uint4*>(wp + (size_t)kb * 2048 + 1024);
                    const bool dpart = kb < nk;
                    const _Float16* PH = dpart ? DH : XH;
                    const _Float16* PL = dpart ? DL : XL;
                    const int col = 16 * (dpart ? kb : kb - nk) + 8 * h;
#pragma unroll
                    for (int i = 0; i < RT; ++i) {
                        const int rt = sub + i * WPC;
                        if (rt < RT) {
                            const int off = (32 * rt + n) * QN_LDH + col;
                            mfma3h(wh, wl, *reinterpret_cast<const uint4*>(PH + off), *reinterpret_cast<const uint4*>(PL + off), acc[i]);
                        }
                    }
                }
            }
            __syncthreads();                                                       // the planes are free for the next chunk
        }

        // ---- epilogue: scale back, bias, identity residual, ReLU; the rows, or their sum over time in a fixed order (lanes' butterfly
        // inside a row tile, then the tiles in order)
        if (mma) {
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                const int rt = sub + i * WPC;
                if (rt >= RT) continue;
                const int t = 32 * rt + n;
                const float un = __uint_as_float((EB[t] - 14u) << 23) * a.w_un;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int cl = 32 * cbl + 8 * g + 4 * h, co = 32 * cb0 + cl;
                    const float4 b4 = *reinterpret_cast<const float4*>(a.bias + co);
                    float y[4] = {fmaf(acc[i][4 * g], un, b4.x), fmaf(acc[i][4 * g + 1], un, b4.y), fmaf(acc[i][4 * g + 2], un, b4.z), fmaf(acc[i][4 * g + 3], un, b4.w)};
                    if (!a.proj && t < T) {
                        const float4 x4 = *reinterpret_cast<const float4*>(xb + (size_t)t * Cin + co);
                        y[0] += x4.x; y[1] += x4.y; y[2] += x4.z; y[3] += x4.w;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = t < T ? fmaxf(y[e], 0.0f) : 0.0f;
                    if (a.mean) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
#pragma unroll
                            for (int o = 1; o < 32; o <<= 1) y[e] += __shfl_xor(y[e], o, 64);
                        }
                        if (n == 0) *reinterpret_cast<float4*>(PS + rt * 256 + cl) = make_float4(y[0], y[1], y[2], y[3]);
                    } else if (t < T) {
                        *reinterpret_cast<float4*>(a.out + ((size_t)b * T + t) * Cout + co) = make_float4(y[0], y[1], y[2], y[3]);
                    }
                }
            }
        }
        if (a.mean) {
            __syncthreads();
            if (tid < 32 * NCB) {
                float s = 0.0f;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) s += PS[rt * 256 + tid];
                a.out[(size_t)b * Cout + 32 * cb0 + tid] = s / (float)T;
            }
        }
        __syncthreads();                                                           // EB, PS and the planes belong to the next clip
    }
}

template <int RT>
hipError_t launch_instance(const QnArgs& a, int cu_count, hipStream_t s) {
    constexpr size_t lds = qn_lds_bytes(RT);
    static_assert(lds <= 160 * 1024, "the clip's planes exceed the LDS");
    const hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(&qn_x3_kernel<RT>), lds);
    if (e != hipSuccess) return e;
    const int per_cu = (int)(160 * 1024 / lds) < 4 ? (int)(160 * 1024 / lds) : 4;      // 512 threads: at most 4 workgroups a CU
    const int ny = (a.Cout + 255) / 256;
    int gx = (cu_count > 0 ? cu_count : 256) * per_cu / ny;
    if (gx < 1) gx = 1;
    if (gx > a.B) gx = a.B;
    hipLaunchKernelGGL(qn_x3_kernel<RT>, dim3((unsigned)gx, (unsigned)ny), dim3(QN_THREADS), lds, s, a);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) dwconv1d_same_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int T, int C,
                                                            int k, int ldw, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // idx = (b T + t) C + c
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const size_t bt = idx / C;
    const int t = (int)(bt % T);
    const float* xb = x + (bt - t) * (size_t)C + c;
    const int left = (k - 1) / 2;                                    // padding='same': the odd row of an even kernel goes behind
    float acc = 0.0f;
    for (int j = 0; j < k; ++j) {
        const int tt = t - left + j;
        if (tt >= 0 && tt < T) acc = fmaf(xb[(size_t)tt * C], w[(size_t)j * ldw + c], acc);
    }
    y[idx] = acc;
}

__global__ void __launch_bounds__(256) add_relu_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, size_t n) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n) y[idx] = fmaxf(a[idx] + b[idx], 0.0f);
}

}  // namespace

bool qn_x3_supported(int T, int Cin, int Cout, int k) {
    return T >= 1 && T <= QN_MAX_T && Cin >= 4 && Cin % 4 == 0 && Cin <= QN_MAX_C && Cout % 32 == 0 && Cout >= 32 && Cout <= QN_MAX_C && (k & 1) && k >= 1 &&
           k <= QN_MAX_K;
}

size_t qn_x3_packed_bytes(int Cin, int Cout, int proj) { return (size_t)(Cout / 32) * (qn_x3_ktot(Cin, proj) / 16) * 2048; }

hipError_t launch_qn_x3_pack(const float* wcat, void* packed, int Cout, int Ktot, float ws, hipStream_t s) {
    if (Cout % 32 || Ktot % 16) return hipErrorInvalidValue;
    const size_t total = (size_t)(Cout / 32) * (Ktot / 16) * 64;
    hipLaunchKernelGGL(qn_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, wcat, reinterpret_cast<unsigned char*>(packed), Cout, Ktot, ws);
    return hipGetLastError();
}

hipError_t launch_qn_x3(const QnArgs& a, int cu_count, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (!qn_x3_supported(a.T, a.Cin, a.Cout, a.k) || a.Cp != qn_x3_cp(a.Cin) || (!a.proj && a.Cin != a.Cout)) return hipErrorInvalidValue;
    if (a.T <= 32) return launch_instance<1>(a, cu_count, s);
    if (a.T <= 64) return launch_instance<2>(a, cu_count, s);
    return launch_instance<4>(a, cu_count, s);
}

hipError_t launch_dwconv1d_same(const float* x, const float* w_t, float* y, int B, int T, int C, int k, int ldw, hipStream_t s) {
    const size_t total = (size_t)B * T * C;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(dwconv1d_same_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, w_t, y, T, C, k, ldw, total);
    return hipGetLastError();
}

hipError_t launch_add_relu(const float* a, const float* b, float* y, size_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(add_relu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, b, y, n);
    return hipGetLastError();
}
