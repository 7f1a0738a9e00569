// tcn_x3.hip - the TCN head (TCNModel, TemporalBlock: architectures.py:290-367) in one launch, over the last step's cone only.
//
// Level i (dilation d = 2^i) is relu( relu(conv2(relu(conv1(x)))) + res ), res = x or downsample(x) (a 1x1 conv, only when
// Cin != Cout); each conv is causal with zero history, y[t] = b + sum_j W[:, :, j] x[t - (k - 1 - j) d].  The head reads the last step
// only, and that step depends on the last R = 1 + 2 (k - 1) (2^L - 1) input steps (29 at the defaults).  The kernel keeps the last
// S = min(T, R) steps of every clip and runs EVERY level over those same S rows, with a row before the window read as zero.  A conv
// output at time t is then exact once t - (k - 1) d is inside the window (or below 0, the true zero history): each conv moves the
// exact region (k - 1) d to the right, and after the 2L convs it starts at T - S + R - 1 >= T - 1.  Rows of the input older than the
// window are never read.
//
// Organisation: NC clips x S rows per workgroup (<= 32 RT rows, RT = 1..3 tiles of 32), activations in LDS (float32, three buffers
// that rotate: block input, conv1 output, block output) with one power-of-two exponent per row (its largest magnitude).  Each conv is
// an implicit GEMM, transposed as in lin_x3.hip: acc [32 outputs x 32 rows] += W[32 x 16] . X^T[16 x 32] per tap and 16 input channels,
// three v_mfma_f32_32x32x16_f16 per product (hi.hi, hi.lo, lo.hi of two binary16 terms).  Wave w owns rows 32 (w % RT) .. + 31 and
// the output blocks w / RT, + 4, ...: a lane holds 16 output channels of ONE row, so the per-row arithmetic is the same wherever the
// row sits.  The B operand of tap j for row r is row r - (k - 1 - j) d, scaled by that row's own power of two and split into two
// binary16 terms; the tap's accumulator is multiplied back by that row's inverse scale before it joins the sum (no per-clip or
// per-tensor bound, no feature clamp).  Weights (two binary16 terms of W x a power of two, packed at finalize) are read from global
// memory / L2 fragment by fragment: each 2 KB fragment serves the workgroup's 32 RT rows.  Bias, ReLU, the residual (or the
// downsample's product, computed in the same pass) and the second ReLU are the conv2 epilogue; the last level writes only the last row
// of each clip, to out[B][C].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "layers.h"
#include "split_h2.h"
#include "tcn_x3.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TCN_G = 4;                   // output-block groups per 32-row tile (waves per tile)
constexpr int TCN_KC = 4;                  // 16-channel input blocks per step (B and A fragments held at once)
constexpr size_t TCN_LDS_MAX = 160 * 1024;

__global__ void __launch_bounds__(256) tcn_pack_kernel(const float* __restrict__ W, unsigned char* __restrict__ out, int Cin, int Cout,
                                                       int taps, float ws) {
    const int K16 = (Cin + 15) / 16;
    const size_t total = (size_t)(Cout / 32) * taps * K16 * 64;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    size_t r = idx >> 6;
    const int kb = (int)(r % K16); r /= K16;
    const int j = (int)(r % taps);
    const int cb = (int)(r / taps);
    const int co = 32 * cb + (lane & 31), c0 = 16 * kb + 8 * (lane >> 5);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = c0 + e < Cin ? W[((size_t)co * Cin + c0 + e) * taps + j] : 0.0f;
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) nww_split2h(v[2 * e] * ws, v[2 * e + 1] * ws, hi[e], lo[e]);
    unsigned char* dst = out + (idx >> 6) * 2048 + (size_t)lane * 16;
    *reinterpret_cast<uint4*>(dst) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4*>(dst + 1024) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

__device__ __forceinline__ void mfma3h(uint4 wh, uint4 wl, uint4 xh, uint4 xl, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wl), __builtin_bit_cast(f16x8, xh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xh), acc, 0, 0, 0);
}

// a row's exponent field of its largest magnitude -> the power of two that puts it in [2^14, 2^15) (as lin_x3.hip) and its inverse
__device__ __forceinline__ uint32_t tcn_eb(uint32_t maxbits) { return min(max(maxbits >> 23, 16u), 254u); }

// acc[i] (output block cg + 4 i) += conv tap j over the rows sr (one per lane) of src: B = the rows x their scale, two binary16 terms
template <int NBW>
__device__ __forceinline__ void tcn_tap(const float* src, int ld, int sr, bool ok, float sc, int K16, const unsigned char* packed, int taps,
                                        int j, int cg, int nCB, int lane, f32x16 (&acc)[NBW]) {
    const int h = lane >> 5;
    for (int k0 = 0; k0 < K16; k0 += TCN_KC) {
        const int nk = min(TCN_KC, K16 - k0);
        uint4 xh[TCN_KC], xl[TCN_KC];
#pragma unroll
        for (int q = 0; q < TCN_KC; ++q) {
            xh[q] = make_uint4(0u, 0u, 0u, 0u); xl[q] = xh[q];
            if (q < nk && ok) {
                const float* p = src + (size_t)sr * ld + 16 * (k0 + q) + 8 * h;
                const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
                uint32_t hi[4], lo[4];
                nww_split2h(a.x * sc, a.y * sc, hi[0], lo[0]);
                nww_split2h(a.z * sc, a.w * sc, hi[1], lo[1]);
                nww_split2h(b.x * sc, b.y * sc, hi[2], lo[2]);
                nww_split2h(b.z * sc, b.w * sc, hi[3], lo[3]);
                xh[q] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
                xl[q] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
            }
        }
#pragma unroll
        for (int i = 0; i < NBW; ++i) {
            const int cb = cg + TCN_G * i;
            if (cb >= nCB) break;
            const unsigned char* wp = packed + ((size_t)(cb * taps + j) * K16 + k0) * 2048 + (size_t)lane * 16;
            uint4 wh[TCN_KC], wl[TCN_KC];
#pragma unroll
            for (int q = 0; q < TCN_KC; ++q)
                if (q < nk) { wh[q] = *reinterpret_cast<const uint4*>(wp + q * 2048); wl[q] = *reinterpret_cast<const uint4*>(wp + q * 2048 + 1024); }
#pragma unroll
            for (int q = 0; q < TCN_KC; ++q)
                if (q < nk) mfma3h(wh[q], wl[q], xh[q], xl[q], acc[i]);
        }
    }
}

// NBW: output blocks per wave (4 NBW x 32 >= the widest level); NBW = 2 only with one row tile (RT = 1, four waves)
template <int NBW>
__global__ void __launch_bounds__(NBW == 1 ? 768 : 256) tcn_x3_kernel(TcnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tcn_lds[];
    const int R = 32 * a.RT, ld = a.ld, nthr = 256 * a.RT;
    // three activation buffers [32 RT][ld] and their rows' largest magnitudes (float bits), addressed arithmetically (no private arrays)
    auto buf = [&](int i) { return tcn_lds + (size_t)i * R * ld; };
    unsigned* emx_base = reinterpret_cast<unsigned*>(tcn_lds + (size_t)3 * R * ld);
    auto emx = [&](int i) { return emx_base + i * R; };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const int rt = wave % a.RT, cg = wave / a.RT;
    const int lr = 32 * rt + n;                               // the lane's row in the workgroup
    const int S = a.S, rows = a.NC * S;
    const int slot = lr % S;
    const int clip = (int)blockIdx.x * a.NC + lr / S;
    const bool out_row = lr < rows && slot == S - 1 && clip < a.B;

    // ---- the last S steps of NC clips -> buffer 0 (channels F .. cin0 and rows past the clips zero), each row's largest magnitude
    for (int i = tid; i < R; i += nthr) emx(0)[i] = 0u;
    __syncthreads();
    {
        const int c4 = a.cin0 / 4;
        for (int idx = tid; idx < R * c4; idx += nthr) {
            const int r = idx / c4, f = 4 * (idx - r * c4);
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const int b = (int)blockIdx.x * a.NC + r / S;
            if (r < rows && b < a.B) {
                const float* xp = a.x + ((size_t)b * a.T + (a.T - S + r % S)) * a.F;
#pragma unroll
                for (int e = 0; e < 4; ++e) if (f + e < a.F) v[e] = xp[f + e];
            }
            *reinterpret_cast<float4*>(buf(0) + (size_t)r * ld + f) = make_float4(v[0], v[1], v[2], v[3]);
            const float m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
            if (m > 0.0f) atomicMax(&emx(0)[r], __float_as_uint(m));
        }
    }

    // one conv over every row of the workgroup: mode 0 = relu(conv + b) (conv1); 1 = relu(relu(conv + b) + res) (conv2), res = the
    // block input's row or the downsample's product; last: write the last row of each clip to out instead of the LDS
    auto conv = [&](int si, int Cin, const TcnConv& cv, int dil, int di, int Cout, int mode, int pi, int Cres, const TcnConv* dsv, bool last) {
        const float* src = buf(si);
        for (int i = tid; i < R; i += nthr) emx(di)[i] = 0u;   // nobody reads emx(di) in this phase
        __syncthreads();
        const int nCB = Cout / 32, K16 = Cin / 16, taps = a.k;
        f32x16 tot[NBW], dsa[NBW];
#pragma unroll
        for (int i = 0; i < NBW; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) { tot[i][e] = 0.0f; dsa[i][e] = 0.0f; }
        float mx = 0.0f;
        if (cg < nCB) {
            for (int j = 0; j < taps; ++j) {
                const int off = (taps - 1 - j) * dil;
                const bool ok = slot >= off;
                const int sr = ok ? lr - off : lr;
                const uint32_t eb = tcn_eb(emx(si)[sr]);
                const float sc = __uint_as_float((268u - eb) << 23), un = ok ? __uint_as_float((eb - 14u) << 23) * cv.w_un : 0.0f;
                f32x16 acc[NBW];
#pragma unroll
                for (int i = 0; i < NBW; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;
                tcn_tap<NBW>(src, ld, sr, ok, sc, K16, cv.packed, taps, j, cg, nCB, lane, acc);
#pragma unroll
                for (int i = 0; i < NBW; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) tot[i][e] = fmaf(acc[i][e], un, tot[i][e]);
            }
            if (dsv) {                                          // downsample: 1x1 conv of the block input's own row
                const uint32_t eb = tcn_eb(emx(pi)[lr]);
                const float sc = __uint_as_float((268u - eb) << 23), un = __uint_as_float((eb - 14u) << 23) * dsv->w_un;
                f32x16 acc[NBW];
#pragma unroll
                for (int i = 0; i < NBW; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;
                tcn_tap<NBW>(buf(pi), ld, lr, true, sc, Cres / 16, dsv->packed, 1, 0, cg, nCB, lane, acc);
#pragma unroll
                for (int i = 0; i < NBW; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) dsa[i][e] = acc[i][e] * un;
            }
#pragma unroll
            for (int i = 0; i < NBW; ++i) {
                const int cb = cg + TCN_G * i;
                if (cb >= nCB) break;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = 32 * cb + 8 * g + 4 * h;
                    const float4 b4 = *reinterpret_cast<const float4*>(cv.bias + co);
                    float v[4] = {fmaxf(tot[i][4 * g] + b4.x, 0.0f), fmaxf(tot[i][4 * g + 1] + b4.y, 0.0f),
                                  fmaxf(tot[i][4 * g + 2] + b4.z, 0.0f), fmaxf(tot[i][4 * g + 3] + b4.w, 0.0f)};
                    if (mode == 1) {
                        float r[4];
                        if (dsv) {
                            const float4 d4 = *reinterpret_cast<const float4*>(dsv->bias + co);
                            r[0] = dsa[i][4 * g] + d4.x; r[1] = dsa[i][4 * g + 1] + d4.y; r[2] = dsa[i][4 * g + 2] + d4.z; r[3] = dsa[i][4 * g + 3] + d4.w;
                        } else {
                            const float4 x4 = *reinterpret_cast<const float4*>(buf(pi) + (size_t)lr * ld + co);
                            r[0] = x4.x; r[1] = x4.y; r[2] = x4.z; r[3] = x4.w;
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e] + r[e], 0.0f);
                    }
                    mx = fmaxf(mx, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
                    if (!last) *reinterpret_cast<float4*>(buf(di) + (size_t)lr * ld + co) = make_float4(v[0], v[1], v[2], v[3]);
                    else if (out_row) *reinterpret_cast<float4*>(a.out + (size_t)clip * Cout + co) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        if (h == 0 && mx > 0.0f) atomicMax(&emx(di)[lr], __float_as_uint(mx));
        __syncthreads();
    };

    int P = 0, Cin = a.cin0;
    for (int l = 0; l < a.L; ++l) {
        const int H = (P + 1) % 3, Q = (P + 2) % 3, Cout = a.ch[l], dil = 1 << l;
        conv(P, Cin, a.c1[l], dil, H, Cout, 0, P, Cin, nullptr, false);
        conv(H, Cout, a.c2[l], dil, Q, Cout, 1, P, Cin, a.ds[l].packed ? &a.ds[l] : nullptr, l == a.L - 1);
        P = Q; Cin = Cout;
    }
}

__global__ void __launch_bounds__(256) tcn_im2col_kernel(const float* __restrict__ x, float* __restrict__ col, int B, int T, int C, int k, int dil) {
    const size_t total = (size_t)B * T * C * k;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int j = (int)(idx % k);
        size_t r = idx / k;
        const int ci = (int)(r % C); r /= C;
        const int t = (int)(r % T);
        const size_t b = r / T;
        const int ts = t - (k - 1 - j) * dil;
        col[idx] = ts >= 0 ? x[(b * T + ts) * C + ci] : 0.0f;
    }
}

__global__ void __launch_bounds__(256) tcn_last_row_kernel(const float* __restrict__ y, float* __restrict__ out, int B, int T, int C) {
    const size_t total = (size_t)B * C;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t b = idx / C;
    out[idx] = y[(b * T + T - 1) * C + idx % C];
}

size_t tcn_lds_bytes(int RT, int ld) { return (size_t)3 * 32 * RT * ld * sizeof(float) + (size_t)3 * 32 * RT * sizeof(unsigned); }

}  // namespace

int tcn_receptive_field(int L, int k) { return 1 + 2 * (k - 1) * ((1 << L) - 1); }

bool tcn_x3_plan(TcnArgs& a) {
    if (a.L < 1 || a.L > TCN_MAX_LEVELS || a.k < 2 || a.T < 1 || a.F < 1) return false;
    a.cin0 = (a.F + 15) / 16 * 16;
    int cmax = a.cin0;
    for (int l = 0; l < a.L; ++l) {
        if (a.ch[l] <= 0 || a.ch[l] % 32 || a.ch[l] > 256) return false;
        cmax = cmax > a.ch[l] ? cmax : a.ch[l];
    }
    if (cmax > 256) return false;
    a.ld = cmax + 4;                                           // rows 4 banks apart: the 16-byte B-operand reads of 8 lanes are conflict-free
    a.S = a.T < tcn_receptive_field(a.L, a.k) ? a.T : tcn_receptive_field(a.L, a.k);
    // the widest level decides the instance: four output blocks per tile and wave group (up to 128 channels, 1..3 tiles, 4..12
    // waves) or eight (up to 256 channels, one tile of four waves).  With cmax <= 128 three tiles always fit (ld <= 132:
    // tcn_lds_bytes(3, 132) = 153216 <= TCN_LDS_MAX), so the loop below settles on RT = 3 for every S <= 96 and refuses a longer
    // cone: RT = 1 / 2 of instance <1> are kept by the kernel and the launcher but no plan reaches them
    const int max_rt = cmax <= 128 ? 3 : 1;
    a.RT = 0;
    for (int rt = max_rt; rt >= 1; --rt)
        if (32 * rt >= a.S && tcn_lds_bytes(rt, a.ld) <= TCN_LDS_MAX) { a.RT = rt; break; }
    if (!a.RT) return false;
    a.NC = 32 * a.RT / a.S;
    return true;
}

size_t tcn_x3_packed_bytes(int Cin, int Cout, int taps) { return (size_t)(Cout / 32) * taps * ((Cin + 15) / 16) * 2048; }

hipError_t launch_tcn_x3_pack(const float* W, void* out, int Cin, int Cout, int taps, float ws, hipStream_t s) {
    if (Cout % 32 || Cin < 1 || taps < 1) return hipErrorInvalidValue;
    const size_t total = (size_t)(Cout / 32) * taps * ((Cin + 15) / 16) * 64;
    hipLaunchKernelGGL(tcn_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, W, reinterpret_cast<unsigned char*>(out),
                       Cin, Cout, taps, ws);
    return hipGetLastError();
}

hipError_t launch_tcn_x3(const TcnArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (a.RT < 1 || a.RT > 3 || a.NC < 1 || a.NC * a.S > 32 * a.RT || a.S > a.T || a.ld % 4) return hipErrorInvalidValue;
    int cmax = a.cin0;
    for (int l = 0; l < a.L; ++l) cmax = cmax > a.ch[l] ? cmax : a.ch[l];
    if (cmax + 4 > a.ld || (cmax > 128 && a.RT != 1)) return hipErrorInvalidValue;
    const size_t lds = tcn_lds_bytes(a.RT, a.ld);
    if (lds > TCN_LDS_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.B + a.NC - 1) / a.NC));
    hipError_t e;
    if (cmax <= 128) {
        if ((e = nww_allow_lds(reinterpret_cast<const void*>(&tcn_x3_kernel<1>), lds)) != hipSuccess) return e;
        hipLaunchKernelGGL(tcn_x3_kernel<1>, grid, dim3(256 * a.RT), lds, s, a);
    } else {
        if ((e = nww_allow_lds(reinterpret_cast<const void*>(&tcn_x3_kernel<2>), lds)) != hipSuccess) return e;
        hipLaunchKernelGGL(tcn_x3_kernel<2>, grid, dim3(256), lds, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_tcn_im2col(const float* x, float* col, int B, int T, int C, int k, int dil, hipStream_t s) {
    const size_t total = (size_t)B * T * C * k;
    if (!total) return hipSuccess;
    size_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(tcn_im2col_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, col, B, T, C, k, dil);
    return hipGetLastError();
}

hipError_t launch_tcn_last_row(const float* y, float* out, int B, int T, int C, hipStream_t s) {
    const size_t total = (size_t)B * C;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(tcn_last_row_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, y, out, B, T, C);
    return hipGetLastError();
}
