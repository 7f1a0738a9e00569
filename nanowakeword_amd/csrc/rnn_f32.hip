// rnn_f32.hip - GRU / LSTM recurrences with the recurrent product h W_hh^T on the float32 matrix cores (gfx950), and launch_rnn.
//
// nn.GRU (gates r, z, n) / nn.LSTM (gates i, f, g, o in the G H rows of W_ih / W_hh; CRNNModel's default backend:
// nanowakeword/modules/architectures.py:247-254, model.py:214): with xg = x W_ih^T + b_ih precomputed for every frame, a kernel
// walks the steps of one direction; the cell update is rnn_cell (rnn_cell.h).  Every kernel is one template over G = 3 (GRU) / 4 (LSTM).
// conv_arith = "f32" runs these at every width; the split-operand arithmetics at the widths rnn_x3.hip / rnn_stream.hip do not take.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "layers.h"
#include "rnn_cell.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
// H % 4 == 0, H <= 256.  One workgroup = 32 clips x all H hidden units; wave w owns hidden units [32w, 32w+32) and computes, per
// step, the G 32x32 gate tiles (columns j, H+j, ...) of  hg = h W_hh^T  on v_mfma_f32_32x32x2_f32, with h as the
// A operand read from LDS ([32][H+4] floats) and W_hh rows streamed from L2.  Gate math runs in the MFMA C
// layout (lane = hidden unit j, 16 clips per lane), so xg loads and h stores are coalesced along j, and
// the carried state (h / c) stays in registers across steps.  Gate functions: expf / tanhf.
// k-loop: the G loads of an 8-k slice of W_hh sit under ONE branch, so that they are waited for one by one as the MFMAs consume them
// (a branch per load ends in one wait for all of them: + 8 % at H = 96).  Requesting the next slice a trip ahead gains nothing - the
// compiler waits for it before the current slice's third MFMA - and costs the LSTM 200 bytes of scratch.
template <int G>
__global__ void __launch_bounds__(512) rnn32_kernel(RnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* hs = reinterpret_cast<float*>(smem_raw);           // [32][H+4]
    const int H = a.H, ldh = H + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, hh = lane >> 5;
    const int b0 = blockIdx.x * 32;
    const int j = wave * 32 + i;                              // hidden unit of this lane (C-layout column)
    const bool jok = j < H;
    const int jc = jok ? j : H - 1;
    for (int idx = threadIdx.x; idx < 32 * ldh; idx += blockDim.x) hs[idx] = 0.0f;
    float state[16];                                          // what the cell carries (h / c) for the lane's 16 clips
#pragma unroll
    for (int r = 0; r < 16; ++r) state[r] = 0.0f;
    float bh[G];
    const float* wq[G];                                       // B operand rows (col = lane&31 -> same jc)
#pragma unroll
    for (int q = 0; q < G; ++q) {
        bh[q] = a.b_hh[q * H + jc];
        wq[q] = a.w_hh + (size_t)(q * H + jc) * H + 4 * hh;
    }
    const float* arow = hs + (size_t)i * ldh + 4 * hh;        // A operand row (clip i)
    __syncthreads();
    for (int step = 0; step < a.steps; ++step) {
        const int t = a.reverse ? a.T - 1 - step : step;
        // (opaque per step: the 16 gate-row and output addresses of the lane are not hoisted out of the step loop and spilled)
        int hh_o = lane >> 5;
        asm volatile("" : "+v"(hh_o));
        f32x16 acc[G];
#pragma unroll
        for (int q = 0; q < G; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
        // the input-side gate pre-activations of this step do not depend on h: fetch them (HBM, one row per clip)
        // before the recurrent product so their latency hides under the MFMA loop
        float xq[16][G];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int b = b0 + (r & 3) + 8 * (r >> 2) + 4 * hh_o;
#pragma unroll
            for (int q = 0; q < G; ++q) xq[r][q] = 0.0f;
            if (b < a.B && jok) {
                const float* xg = a.xg + ((size_t)b * a.T + t) * G * H;
#pragma unroll
                for (int q = 0; q < G; ++q) xq[r][q] = xg[q * H + j];
            }
        }
        if (step > 0) {                                       // h == 0 on the first step
            for (int k = 0; k < H; k += 8) {
                float4 av = make_float4(0, 0, 0, 0), bw[G];
#pragma unroll
                for (int q = 0; q < G; ++q) bw[q] = make_float4(0, 0, 0, 0);
                if (k + 4 * hh + 4 <= H) {                    // (one branch around the slice's loads: the MFMAs start as each arrives)
                    av = *reinterpret_cast<const float4*>(arow + k);
#pragma unroll
                    for (int q = 0; q < G; ++q) bw[q] = *reinterpret_cast<const float4*>(wq[q] + k);
                }
#pragma unroll
                for (int q = 0; q < G; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bw[q].x, acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < G; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bw[q].y, acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < G; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bw[q].z, acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < G; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bw[q].w, acc[q], 0, 0, 0);
            }
        }
        __syncthreads();                                      // every wave has finished reading hs
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = (r & 3) + 8 * (r >> 2) + 4 * hh_o;  // clip row within the block
            const int b = b0 + c;
            float hn = 0.0f;
            if (b < a.B && jok) {
                hn = rnn_cell<G, GatesLib>(xq[r], 1, acc_row(acc, r), bh, state[r]);
                if (a.seq_out) a.seq_out[((size_t)b * a.T + t) * a.ld_seq + a.col_off + j] = hn;
                if (a.last_out && step == a.steps - 1) a.last_out[(size_t)b * a.ld_last + a.col_off + j] = hn;
            }
            if (jok) hs[(size_t)c * ldh + j] = hn;
        }
        __syncthreads();
    }
}

// Register-resident variant for H in {32, 64, 128} (H = 256 would need 384 weight registers at two waves per SIMD): one workgroup =
// 16 clips, wave w owns 16 NB hidden units of every gate as NB 16-wide column blocks on v_mfma_f32_16x16x4_f32 - two for the GRU
// (H / 32 waves, one per SIMD at H = 128: the 512-register budget is there), one for the LSTM (H / 16 waves).  Lane (n = l&15, g = l>>4)
// feeds k = g*H/4 + s at MFMA step s, so its slice of every W_hh row it needs is H/4 CONTIGUOUS floats, loaded once and kept in
// G*NB*H/4 VGPRs for all steps - the 32-clip kernel above re-streams W_hh (G*H*H floats) from L2 on every step.  Half the clips per
// workgroup also means twice the workgroups (256 at B = 4096) and half the MFMA chain per step.  C layout: column = hidden unit,
// rows 4g..4g+3 = clips, so xg loads / h stores stay coalesced along the hidden dimension.  Gate functions: hardware exp2 / rcp.
constexpr int rnn16_blocks(int G) { return G == 3 ? 2 : 1; }     // NB
template <int G, int H>
__global__ void __launch_bounds__(64 * H / (16 * rnn16_blocks(G)), 1) rnn16_kernel(RnnArgs a) {
    constexpr int NB = rnn16_blocks(G);
    constexpr int KS = H / 4, LDH = H + 4;                    // MFMA steps per product, LDS row stride
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* hs = reinterpret_cast<float*>(smem_raw);           // [16][H+4]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int j0 = 16 * NB * wave + n;                        // hidden unit of column block 0
    for (int idx = threadIdx.x; idx < 16 * LDH; idx += blockDim.x) hs[idx] = 0.0f;
    // W_hh -> registers: gate q, column block bl, k slice g
    float wreg[G][NB][KS];
    float bh[NB][G];
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
        for (int bl = 0; bl < NB; ++bl) {
            const int j = j0 + 16 * bl;
            const float4* src = reinterpret_cast<const float4*>(a.w_hh + (size_t)(q * H + j) * H + g * KS);
#pragma unroll
            for (int s4 = 0; s4 < KS / 4; ++s4) {
                const float4 v = src[s4];
                wreg[q][bl][4 * s4] = v.x; wreg[q][bl][4 * s4 + 1] = v.y; wreg[q][bl][4 * s4 + 2] = v.z; wreg[q][bl][4 * s4 + 3] = v.w;
            }
            bh[bl][q] = a.b_hh[q * H + j];
        }
    float state[NB][4];
#pragma unroll
    for (int bl = 0; bl < NB; ++bl)
#pragma unroll
        for (int r = 0; r < 4; ++r) state[bl][r] = 0.0f;
    const float* arow = hs + n * LDH + g * KS;                // A operand: clip n, k slice g
    // input-side pre-activations (independent of h) are fetched ONE STEP AHEAD: a row per clip from HBM takes longer than a step's
    // recurrent product
    float xq[NB][4][G], xnext[NB][4][G];
    auto fetch = [&](int step, float (&x)[NB][4][G]) {
        const int t = a.reverse ? a.T - 1 - step : step;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + 4 * g + r;
            const float* xg = a.xg + ((size_t)min(b, a.B - 1) * a.T + t) * G * H + j0;
#pragma unroll
            for (int q = 0; q < G; ++q)
#pragma unroll
                for (int bl = 0; bl < NB; ++bl) x[bl][r][q] = xg[q * H + 16 * bl];
        }
    };
    fetch(0, xq);
    __syncthreads();
    for (int step = 0; step < a.steps; ++step) {
        const int t = a.reverse ? a.T - 1 - step : step;
        f32x4 acc[NB][G];
#pragma unroll
        for (int bl = 0; bl < NB; ++bl)
#pragma unroll
            for (int q = 0; q < G; ++q) acc[bl][q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (step + 1 < a.steps) fetch(step + 1, xnext);
        if (step > 0) {                                       // h == 0 on the first step
#pragma unroll
            for (int s4 = 0; s4 < KS / 4; ++s4) {
                const float4 av = *reinterpret_cast<const float4*>(arow + 4 * s4);
                const float ae[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int q = 0; q < G; ++q)
#pragma unroll
                        for (int bl = 0; bl < NB; ++bl)
                            acc[bl][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ae[e], wreg[q][bl][4 * s4 + e], acc[bl][q], 0, 0, 0);
            }
        }
        __syncthreads();                                      // every wave has finished reading hs
#pragma unroll
        for (int bl = 0; bl < NB; ++bl) {
            const int j = j0 + 16 * bl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 4 * g + r, b = b0 + c;
                float hn = 0.0f;
                if (b < a.B) {
                    hn = rnn_cell<G, GatesHw>(xq[bl][r], 1, acc_row(acc[bl], r), bh[bl], state[bl][r]);
                    if (a.seq_out) a.seq_out[((size_t)b * a.T + t) * a.ld_seq + a.col_off + j] = hn;
                    if (a.last_out && step == a.steps - 1) a.last_out[(size_t)b * a.ld_last + a.col_off + j] = hn;
                }
                hs[c * LDH + j] = hn;
            }
        }
#pragma unroll
        for (int bl = 0; bl < NB; ++bl)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < G; ++q) xq[bl][r][q] = xnext[bl][r][q];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ any-width recurrence
// nn.GRU / nn.LSTM take any hidden_size (architectures.py:132-145,238-254); the kernels above want H % 4 == 0 (16-byte weight rows)
// and H <= 256 (a wave per 32 hidden units).  This one takes any H <= 512: W_hh re-laid at plan time as [G H][ldw] rows padded with
// zeros to ldw = H rounded up to 8 (rnn_pad_rows_kernel), a wave walks tiles wave, wave + 8 (32 hidden units each) one after the
// other within a step, and h lives in TWO LDS buffers (read step t, write step t + 1: one barrier per step).  Gate functions on the
// hardware exp2 / rcp: the library expf / tanhf cost this kernel 22 (GRU) / 52 (LSTM) spilled registers under its 256-register budget.
__global__ void __launch_bounds__(256) rnn_pad_rows_kernel(const float* __restrict__ w, float* __restrict__ out, int rows, int H, int ldw) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)rows * ldw) return;
    const int r = (int)(idx / ldw), k = (int)(idx - (size_t)r * ldw);
    out[idx] = k < H ? w[(size_t)r * H + k] : 0.0f;
}
template <int G>
__global__ void __launch_bounds__(512) rnn_wide_kernel(RnnArgs a) {
    constexpr int TP = 2;                                     // tiles per wave: 8 waves x 2 x 32 = 512 hidden units
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int H = a.H, ldw = a.ldw, ldh = ldw + 4;
    float* hbuf[2] = {reinterpret_cast<float*>(smem_raw), reinterpret_cast<float*>(smem_raw) + (size_t)32 * ldh};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, hh = lane >> 5;
    const int b0 = blockIdx.x * 32;
    const int ntile = (H + 31) / 32;
    for (int idx = threadIdx.x; idx < 2 * 32 * ldh; idx += blockDim.x) hbuf[0][idx] = 0.0f;
    // the previous h of a (clip, unit) is read back from the LDS plane the products use (zero at step 0); only the LSTM's cell state lives in
    // registers (h in registers as well cost 20 / 50 spilled ones under the 256-register budget of sixteen... eight waves)
    float cprev[G == 4 ? TP : 1][16];
#pragma unroll
    for (int tp = 0; tp < (G == 4 ? TP : 1); ++tp)
#pragma unroll
        for (int r = 0; r < 16; ++r) cprev[tp][r] = 0.0f;
    __syncthreads();
    for (int step = 0; step < a.steps; ++step) {
        const int t = a.reverse ? a.T - 1 - step : step;
        const float* cur = hbuf[step & 1];
        float* nxt = hbuf[(step & 1) ^ 1];
        // lane coordinates re-derived from an opaque copy every step: from the plain ones the 16 output addresses per tile are loop-invariant,
        // get hoisted out of the step loop and spill (50 registers in the LSTM instance)
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
        const int i = lane_o & 31, hh = lane_o >> 5;
#pragma unroll
        for (int tp = 0; tp < TP; ++tp) {
            const int tile = wave + 8 * tp;
            if (tile >= ntile) continue;                      // (wave-uniform)
            const int j = tile * 32 + i;
            const bool jok = j < H;
            const int jc = jok ? j : H - 1;
            f32x16 acc[G];
#pragma unroll
            for (int q = 0; q < G; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
            if (step > 0) {
                const float* arow = cur + (size_t)i * ldh + 4 * hh;
                const float* wq[G];
#pragma unroll
                for (int q = 0; q < G; ++q) wq[q] = a.w_hh + (size_t)(q * H + jc) * ldw + 4 * hh;
                for (int k = 0; k < ldw; k += 8) {
                    const float4 av = *reinterpret_cast<const float4*>(arow + k);
                    float4 bw[G];
#pragma unroll
                    for (int q = 0; q < G; ++q) bw[q] = *reinterpret_cast<const float4*>(wq[q] + k);
#pragma unroll
                    for (int q = 0; q < G; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bw[q].x, acc[q], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < G; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bw[q].y, acc[q], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < G; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bw[q].z, acc[q], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < G; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bw[q].w, acc[q], 0, 0, 0);
                }
            }
            float bh[G];
#pragma unroll
            for (int q = 0; q < G; ++q) bh[q] = a.b_hh[q * H + jc];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = (r & 3) + 8 * (r >> 2) + 4 * hh;
                const int b = b0 + c;
                float hn = 0.0f, cn = 0.0f;
                if (b < a.B && jok) {
                    const float* xg = a.xg + ((size_t)b * a.T + t) * G * H + j;
                    float st = G == 3 ? cur[(size_t)c * ldh + j] : cprev[G == 4 ? tp : 0][r];      // the carried state: h / c
                    hn = rnn_cell<G, GatesHw>(xg, H, acc_row(acc, r), bh, st);
                    cn = st;
                    if (a.seq_out) a.seq_out[((size_t)b * a.T + t) * a.ld_seq + a.col_off + j] = hn;
                    if (a.last_out && step == a.steps - 1) a.last_out[(size_t)b * a.ld_last + a.col_off + j] = hn;
                }
                if (G == 4) cprev[G == 4 ? tp : 0][r] = cn;
                if (jok) nxt[(size_t)c * ldh + j] = hn;
            }
        }
        __syncthreads();
    }
}
}  // namespace

size_t rnn_wide_weight_bytes(int gates, int H) { return (size_t)gates * H * ((H + 7) & ~7) * sizeof(float); }
hipError_t launch_rnn_pad_weights(const float* w_hh, float* out, int gates, int H, hipStream_t s) {
    const int ldw = (H + 7) & ~7;
    const size_t total = (size_t)gates * H * ldw;
    hipLaunchKernelGGL(rnn_pad_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w_hh, out, gates * H, H, ldw);
    return hipGetLastError();
}

template <int G>
static hipError_t launch_rnn_wide(const RnnArgs& a, hipStream_t s) {
    if (a.H < 1 || a.H > 512 || a.ldw != ((a.H + 7) & ~7) || a.xg2) return hipErrorInvalidValue;
    const size_t lds = (size_t)2 * 32 * (a.ldw + 4) * sizeof(float);
    hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(rnn_wide_kernel<G>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rnn_wide_kernel<G>, dim3((a.B + 31) / 32), dim3(512), lds, s, a);
    return hipGetLastError();
}

// H % 4 == 0, H <= 256: the register-resident kernel at its widths, else 32 clips per workgroup with W_hh from L2
template <int G>
static hipError_t launch_rnn_f32(const RnnArgs& a, hipStream_t s) {
    if ((a.H == 32 || a.H == 64 || a.H == 128) && (reinterpret_cast<uintptr_t>(a.w_hh) & 15) == 0) {
        const size_t lds16 = (size_t)16 * (a.H + 4) * sizeof(float);
        const dim3 grid((a.B + 15) / 16), block(64 * a.H / (16 * rnn16_blocks(G)));
        switch (a.H) {
            case 32: hipLaunchKernelGGL((rnn16_kernel<G, 32>), grid, block, lds16, s, a); break;
            case 64: hipLaunchKernelGGL((rnn16_kernel<G, 64>), grid, block, lds16, s, a); break;
            default: hipLaunchKernelGGL((rnn16_kernel<G, 128>), grid, block, lds16, s, a); break;
        }
        return hipGetLastError();
    }
    const int waves = (a.H + 31) / 32;                        // a wave per 32 hidden units, 512 threads
    const size_t lds = (size_t)32 * (a.H + 4) * sizeof(float);
    hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(rnn32_kernel<G>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rnn32_kernel<G>, dim3((a.B + 31) / 32), dim3(waves * 64), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_rnn(const RnnArgs& a, hipStream_t s) {
    if (a.gates != 3 && a.gates != 4) return hipErrorInvalidValue;
    if (a.w_packed) return launch_rnn_stream(a, s);
    if (a.ldw) return a.gates == 3 ? launch_rnn_wide<3>(a, s) : launch_rnn_wide<4>(a, s);      // padded weights (planned for H % 4 != 0 or H > 256)
    if (a.H % 4 != 0 || a.H > 256) return hipErrorInvalidValue;
    if (rnn_x3_usable(a)) return launch_rnn_x3(a, s);
    if (a.xg2) return hipErrorInvalidValue;                           // only rnn_x3 folds the opposite direction's step
    return a.gates == 3 ? launch_rnn_f32<3>(a, s) : launch_rnn_f32<4>(a, s);
}
