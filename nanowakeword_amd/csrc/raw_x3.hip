// raw_x3.hip - the raw-PCM frontend in one launch.  A workgroup takes 32 rows of the LAST stage of one clip and recomputes the halo in
// front of them: 137 rows of the stage before (4 . 31 + 13) and, at depth 3, 557 rows of stage 0.  The intermediate rows never leave
// LDS: each is two binary16 planes (hi, lo of value x a plan-time power of two), time-major.
//   stage 0 (1 -> C1, k 41, stride 16): float32 fmaf on the VALU straight from the int16 samples in LDS, in conv1d_strided's order - a
//     thread keeps its channel's 41 taps (x 2^-15, exact) in registers and the lanes of a row read the same words (broadcast);
//   later stages (k 13, stride 4): implicit GEMMs, transposed as in qn_x3.hip: acc [32 outputs x 32 rows] += W[32 x 16] . X^T[16 x 32];
//     a K-chunk of 16 is 16 channels of ONE tap, so lane (n, h)'s B fragment is 16 bytes of row 4 r + j - read straight out of the plane.
//     Three v_mfma_f32_32x32x16_f16 per chunk (hi.hi, hi.lo, lo.hi), float32 accumulation, weight fragments packed at plan time.
// Scaling clamps nothing: |x| <= 1 bounds every stage's output through the folded weights' row 1-norms (plan time), the bound's power of
// two puts it in [2^14, 2^15).  No scale depends on the data, so a clip's rows do not depend on its batch or slot.
// Plane rows are stored by residue: local row i at position (i & 3) Q + (i >> 2), Q = ceil(R / 4), so that the 32 rows 4 r + j a tap
// reads are consecutive positions; with pitches of 12, 20 and 36 dwords sixteen consecutive positions start at sixteen different
// multiples of 4 banks.  Rows outside the clip are the next stage's zero padding and are stored as zeros.
#include <stdint.h>
#include <algorithm>
#include "layers.h"
#include "split_h2.h"
#include "raw_x3.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int RX_THREADS = 512;
constexpr int RX_ROWS = 32;                // rows of the last stage per workgroup
constexpr int RX_R1 = 4 * (RX_ROWS - 1) + 13;      // 137
constexpr int RX_R0 = 4 * (RX_R1 - 1) + 13;        // 557

__host__ __device__ constexpr int rx_plane_rows(int R) { return 4 * ((R + 3) / 4); }
__host__ __device__ constexpr int rx_pcm_halves(int R) { return ((R - 1) * 16 + 41 + 1 + 7) & ~7; }

__device__ __forceinline__ int rx_pos(int i, int Q) { return (i & 3) * Q + (i >> 2); }

__device__ __forceinline__ void rx_mfma3h(uint4 wh, uint4 wl, uint4 xh, uint4 xl, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wl), __builtin_bit_cast(f16x8, xh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wh), __builtin_bit_cast(f16x8, xh), acc, 0, 0, 0);
}

// One strided stage on the matrix pipe.  Reads plane (PH, PL) [Rin rows][pitch halves] of Cin channels; yields Rout local rows (local
// row r is row gout0 + r of the clip's Lst rows at this stage) of Cout channels: into the plane (OH, OL) times oscale, or to y.
// SUB (the row-subset instance): local row r is global row rowtab[r] of whichever clip its segment belongs to (negative: not a row
// of any), and a kept row of the last stage goes to y + off1[r] (and, in a ring, again to y + off2[r]).
template <bool SUB>
__device__ __forceinline__ void rx_stage(const _Float16* PH, const _Float16* PL, int pitch, int Rin, int Cin, int Cout, const unsigned char* packed,
                                         const float* __restrict__ bias, float un, int Rout, int gout0, int Lst, _Float16* OH, _Float16* OL, int opitch,
                                         float oscale, float* __restrict__ y, int ct_out, int wave, int lane, const int* rowtab = nullptr,
                                         const long long* off1 = nullptr, const long long* off2 = nullptr) {
    const int n = lane & 31, h = lane >> 5;
    const int ncb = Cout / 32, nrt = (Rout + 31) / 32, Qin = (Rin + 3) >> 2, Qout = (Rout + 3) >> 2, cpj = Cin / 16, K16 = 13 * cpj;
    for (int item = wave; item < ncb * nrt; item += RX_THREADS / 64) {
        const int cb = item % ncb, rt = item / ncb, r = 32 * rt + n;
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        const unsigned char* wp = packed + (size_t)cb * K16 * 2048 + (size_t)lane * 16;
        for (int j = 0; j < 13; ++j) {
            const int i = min(4 * r + j, Rin - 1);             // rows past the tile's last feed only rows that are not kept
            const int base = rx_pos(i, Qin) * pitch + 8 * h;
            for (int cc = 0; cc < cpj; ++cc) {
                const unsigned char* w = wp + (size_t)(j * cpj + cc) * 2048;
                rx_mfma3h(*reinterpret_cast<const uint4*>(w), *reinterpret_cast<const uint4*>(w + 1024),
                          *reinterpret_cast<const uint4*>(PH + base + 16 * cc), *reinterpret_cast<const uint4*>(PL + base + 16 * cc), acc);
            }
        }
        int tg;
        if constexpr (SUB) tg = r < Rout ? rowtab[r] : -1;
        else tg = gout0 + r;
        const bool live = r < Rout && tg >= 0 && tg < Lst;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = 32 * cb + 8 * g + 4 * h;
            const float4 b4 = *reinterpret_cast<const float4*>(bias + co);
            float v[4] = {fmaf(acc[4 * g], un, b4.x), fmaf(acc[4 * g + 1], un, b4.y), fmaf(acc[4 * g + 2], un, b4.z), fmaf(acc[4 * g + 3], un, b4.w)};
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = live ? fmaxf(v[e], 0.0f) : 0.0f;
            if (OH) {
                if (r < Rout) {
                    uint32_t h0, l0, h1, l1;
                    nww_split2h(v[0] * oscale, v[1] * oscale, h0, l0);
                    nww_split2h(v[2] * oscale, v[3] * oscale, h1, l1);
                    const int off = rx_pos(r, Qout) * opitch + co;
                    *reinterpret_cast<uint2*>(OH + off) = make_uint2(h0, h1);
                    *reinterpret_cast<uint2*>(OL + off) = make_uint2(l0, l1);
                }
            } else if (live) {
                if constexpr (SUB) {
                    const float4 o4 = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4*>(y + off1[r] + co) = o4;
                    if (off2[r] >= 0) *reinterpret_cast<float4*>(y + off2[r] + co) = o4;
                } else if (ct_out) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[(size_t)(co + e) * Lst + tg] = v[e];
                } else {
                    *reinterpret_cast<float4*>(y + (size_t)tg * Cout + co) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
    }
}

// Stage 0 on the VALU: thread = (channel, row lane); the channel's taps stay in registers.  Local row r is global row g0 + r of the clip
// (SUB: rowtab[r]).
template <bool SUB>
__device__ __forceinline__ void rx_stage0(const RawX3Args& a, const int16_t* PC, _Float16* P0H, _Float16* P0L, int R0, int p0pitch, int g0, int tid,
                                          const int* rowtab = nullptr) {
    const int C1 = a.C1;
    const int co = tid % C1, rl = tid / C1, rstep = RX_THREADS / C1, Q0 = (R0 + 3) >> 2;
    float w[41];
#pragma unroll
    for (int j = 0; j < 41; ++j) w[j] = a.w1[j * C1 + co] * (1.0f / 32768.0f);
    const float b0 = a.b1[co], sc = a.scale[0];
    for (int r = rl; r < R0; r += rstep) {
        const uint32_t* sp = reinterpret_cast<const uint32_t*>(PC + 16 * r);
        float acc = b0;
#pragma unroll
        for (int q = 0; q < 21; ++q) {
            const uint32_t u = sp[q];
            acc = fmaf((float)(int16_t)(u & 0xffffu), w[2 * q], acc);
            if (2 * q + 1 < 41) acc = fmaf((float)((int32_t)u >> 16), w[2 * q + 1], acc);
        }
        int tg;
        if constexpr (SUB) tg = rowtab[r];
        else tg = g0 + r;
        const float v = tg >= 0 && tg < a.L[0] ? fmaxf(acc, 0.0f) * sc : 0.0f;
        uint32_t hi, lo;
        nww_split2h(v, 0.0f, hi, lo);
        const int off = rx_pos(r, Q0) * p0pitch + co;
        reinterpret_cast<uint16_t*>(P0H)[off] = (uint16_t)(hi & 0xffffu);
        reinterpret_cast<uint16_t*>(P0L)[off] = (uint16_t)(lo & 0xffffu);
    }
}

__global__ void __launch_bounds__(RX_THREADS) raw_x3_kernel(RawX3Args a, int tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rx_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * RX_ROWS;
    const int C1 = a.C1, depth = a.depth;
    const int R0 = depth == 3 ? RX_R0 : RX_R1;                 // stage-0 rows this tile needs
    const int p0pitch = C1 + 8, p1pitch = 2 * C1 + 8;
    int16_t* PC = reinterpret_cast<int16_t*>(rx_lds);
    _Float16* P0H = reinterpret_cast<_Float16*>(PC + rx_pcm_halves(R0));
    _Float16* P0L = P0H + rx_plane_rows(R0) * p0pitch;
    _Float16* P1H = P0L + rx_plane_rows(R0) * p0pitch;        // depth 3 only
    _Float16* P1L = P1H + rx_plane_rows(RX_R1) * p1pitch;
    // global row of local row 0 at each level, from the last stage down; then the first sample
    const int gl = t0, gm = 4 * gl - 6, g0 = depth == 3 ? 4 * gm - 6 : gm, s0 = 16 * g0 - 20;
    const int nsamp = (R0 - 1) * 16 + 41 + 1;
    const int16_t* pb = a.pcm + (size_t)b * a.pcm_stride;
    for (int i = tid; i < nsamp; i += RX_THREADS) {
        const int gi = s0 + i;
        PC[i] = gi >= 0 && gi < a.N ? pb[gi] : (int16_t)0;
    }
    __syncthreads();

    rx_stage0<false>(a, PC, P0H, P0L, R0, p0pitch, g0, tid);
    __syncthreads();

    float* yb = a.y + (size_t)b * a.L[depth - 1] * (C1 << (depth - 1));
    if (depth == 3) {
        rx_stage<false>(P0H, P0L, p0pitch, RX_R0, C1, 2 * C1, a.packed[0], a.bias[0], a.un[0], RX_R1, gm, a.L[1], P1H, P1L, p1pitch, a.scale[1], nullptr, 0, wave, lane);
        __syncthreads();
        rx_stage<false>(P1H, P1L, p1pitch, RX_R1, 2 * C1, 4 * C1, a.packed[1], a.bias[1], a.un[1], RX_ROWS, gl, a.L[2], nullptr, nullptr, 0, 0.0f, yb, a.ct_out, wave, lane);
    } else {
        rx_stage<false>(P0H, P0L, p0pitch, RX_R1, C1, 2 * C1, a.packed[0], a.bias[0], a.un[0], RX_ROWS, gl, a.L[1], nullptr, nullptr, 0, 0.0f, yb, a.ct_out, wave, lane);
    }
}

// ---- the row-subset instance (streaming hops, the edge rows of a recording's windows): only rows of up to three ranges [t0, t1) of
// every clip's last stage are computed.  A range is cut into pieces of at most 32 rows; a workgroup packs G consecutive pieces - of
// whichever clips - into its 32-row tile as segments, segment s at local rows [o_s, o_s + n_s) with o_(s+1) = o_s + n_s + 3.  The
// three dead rows between two segments are what keeps their halos apart at every level: local row r of a stage reads local rows
// 4 r .. 4 r + 12 of the stage before, so segment s ends at 4 (o_s + n_s - 1) + 12 there and the next one starts at 4 (o_s + n_s + 3), and
// likewise 16 (o_s + n_s - 1) + 60 against 16 (o_s + n_s + 3) two stages down and in units of 16 samples below that.  The tile, its
// planes and every per-row instruction are the full kernel's (rx_stage0, rx_stage); only the map from a local row to (clip, global row)
// differs, and it is tabulated in LDS behind the planes.  Dead rows are computed from whatever their slot holds and never kept.
constexpr int RX_GAP = 3, RX_MAXSEG = 8;

struct RawX3SubDev {
    int nr = 0, P = 0, G = 0;              // ranges, pieces per clip, pieces per workgroup
    int t0[3] = {0, 0, 0}, t1[3] = {0, 0, 0}, cum[3] = {0, 0, 0};   // cum[i]: pieces of ranges 0..i
    long long total = 0;                   // B . P
    int ring_rows = 0, row0 = 0;
    long long out_clip_stride = 0;
};

__host__ __device__ constexpr size_t rx_sub_table_bytes(int R0) { return (size_t)2 * RX_ROWS * 8 + (size_t)(RX_ROWS + 4 * RX_MAXSEG + 4 + rx_plane_rows(RX_R1) + rx_plane_rows(R0)) * 4; }

__global__ void __launch_bounds__(RX_THREADS) raw_x3_sub_kernel(RawX3Args a, RawX3SubDev d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rx_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C1 = a.C1, depth = a.depth, Cl = C1 << (depth - 1);
    const int R0 = depth == 3 ? RX_R0 : RX_R1;
    const int p0pitch = C1 + 8, p1pitch = 2 * C1 + 8;
    int16_t* PC = reinterpret_cast<int16_t*>(rx_lds);
    _Float16* P0H = reinterpret_cast<_Float16*>(PC + rx_pcm_halves(R0));
    _Float16* P0L = P0H + rx_plane_rows(R0) * p0pitch;
    _Float16* P1H = P0L + rx_plane_rows(R0) * p0pitch;        // depth 3 only
    _Float16* P1L = P1H + rx_plane_rows(RX_R1) * p1pitch;
    long long* off1 = reinterpret_cast<long long*>(depth == 3 ? P1L + rx_plane_rows(RX_R1) * p1pitch : P1H);
    long long* off2 = off1 + RX_ROWS;
    int* tabL = reinterpret_cast<int*>(off2 + RX_ROWS);
    int *so = tabL + RX_ROWS, *sn = so + RX_MAXSEG, *sb = sn + RX_MAXSEG, *st = sb + RX_MAXSEG, *nsp = st + RX_MAXSEG;
    int* tab1 = nsp + 4;
    int* tab0 = tab1 + rx_plane_rows(RX_R1);

    if (tid == 0) {                         // this workgroup's segments
        int o = 0, ns = 0;
        for (int j = 0; j < d.G && ns < RX_MAXSEG; ++j) {
            const long long q = (long long)blockIdx.x * d.G + j;
            if (q >= d.total) break;
            const int b = (int)(q / d.P), pi = (int)(q - (long long)b * d.P);
            int rg = 0, prev = 0;
            while (rg < d.nr - 1 && pi >= d.cum[rg]) { prev = d.cum[rg]; ++rg; }
            const int t = d.t0[rg] + RX_ROWS * (pi - prev), n = min(RX_ROWS, d.t1[rg] - t);
            if (n < 1 || o + n > RX_ROWS) break;               // (the launcher chose G so that this never happens)
            so[ns] = o; sn[ns] = n; sb[ns] = b; st[ns] = t; ++ns;
            o += n + RX_GAP;
        }
        *nsp = ns;
    }
    __syncthreads();
    const int nseg = *nsp;
    if (nseg == 0) return;
    const int m0 = depth == 3 ? 16 : 4, c0 = depth == 3 ? 30 : 6;       // stage-0 rows per last-stage row; global stage-0 row of local row 0 = m0 t - c0
    // the segment whose slot holds position x of a level with m positions per last-stage row
    auto seg_of = [&](int x, int m) {
        int s = 0;
        for (int j = 1; j < nseg; ++j) s += so[j] * m <= x ? 1 : 0;
        return s;
    };
    for (int r = tid; r < R0; r += RX_THREADS) {
        const int s = seg_of(r, m0);
        tab0[r] = m0 * st[s] - c0 + (r - m0 * so[s]);
    }
    if (depth == 3)
        for (int r = tid; r < RX_R1; r += RX_THREADS) {
            const int s = seg_of(r, 4);
            tab1[r] = 4 * st[s] - 6 + (r - 4 * so[s]);
        }
    if (tid < RX_ROWS) {
        const int s = seg_of(tid, 1), rr = tid - so[s], tg = st[s] + rr;
        const bool kept = rr < sn[s];
        const long long base = (long long)sb[s] * d.out_clip_stride;
        tabL[tid] = kept ? tg : -1;
        if (d.ring_rows > 0) {             // a ring of 2 ring_rows rows: row x = row0 + t and again ring_rows rows away (Fe2Sub)
            const int x = d.row0 + tg;
            off1[tid] = base + (long long)x * Cl;
            off2[tid] = base + (long long)(x < d.ring_rows ? x + d.ring_rows : x - d.ring_rows) * Cl;
        } else {
            off1[tid] = base + (long long)tg * Cl;
            off2[tid] = -1;
        }
    }
    const int nsamp = (R0 - 1) * 16 + 41 + 1;
    for (int i = tid; i < nsamp; i += RX_THREADS) {
        const int s = seg_of(i, 16 * m0);
        const int gi = 16 * (m0 * st[s] - c0) - 20 + (i - 16 * m0 * so[s]);
        PC[i] = gi >= 0 && gi < a.N ? a.pcm[(size_t)sb[s] * a.pcm_stride + gi] : (int16_t)0;
    }
    __syncthreads();

    rx_stage0<true>(a, PC, P0H, P0L, R0, p0pitch, 0, tid, tab0);
    __syncthreads();

    if (depth == 3) {
        rx_stage<true>(P0H, P0L, p0pitch, RX_R0, C1, 2 * C1, a.packed[0], a.bias[0], a.un[0], RX_R1, 0, a.L[1], P1H, P1L, p1pitch, a.scale[1], nullptr, 0, wave, lane, tab1);
        __syncthreads();
        rx_stage<true>(P1H, P1L, p1pitch, RX_R1, 2 * C1, 4 * C1, a.packed[1], a.bias[1], a.un[1], RX_ROWS, 0, a.L[2], nullptr, nullptr, 0, 0.0f, a.y, 0, wave, lane, tabL, off1, off2);
    } else {
        rx_stage<true>(P0H, P0L, p0pitch, RX_R1, C1, 2 * C1, a.packed[0], a.bias[0], a.un[0], RX_ROWS, 0, a.L[1], nullptr, nullptr, 0, 0.0f, a.y, 0, wave, lane, tabL, off1, off2);
    }
}

}  // namespace

bool raw_x3_supported(int channels, int depth) { return (channels == 16 || channels == 32) && (depth == 2 || depth == 3); }

size_t raw_x3_lds_bytes(int channels, int depth) {
    const int R0 = depth == 3 ? RX_R0 : RX_R1;
    size_t bytes = (size_t)rx_pcm_halves(R0) * 2 + (size_t)2 * rx_plane_rows(R0) * (channels + 8) * 2;
    if (depth == 3) bytes += (size_t)2 * rx_plane_rows(RX_R1) * (2 * channels + 8) * 2;
    return bytes;
}

// (pcm_stride may be smaller than N: overlapping clips, the windows of a recording a hop apart - samples [0, N) of each are read only)
hipError_t launch_raw_x3(const RawX3Args& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (!raw_x3_supported(a.C1, a.depth) || a.N < 1 || a.pcm_stride < 1 || !a.pcm || !a.y || !a.w1 || !a.b1 || !a.packed[0] || !a.bias[0] ||
        (a.depth == 3 && (!a.packed[1] || !a.bias[1])) || a.L[a.depth - 1] < 1)
        return hipErrorInvalidValue;
    const size_t lds = raw_x3_lds_bytes(a.C1, a.depth);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(&raw_x3_kernel), lds);
    if (e != hipSuccess) return e;
    const int tiles = (a.L[a.depth - 1] + RX_ROWS - 1) / RX_ROWS;
    if ((size_t)tiles * a.B > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(raw_x3_kernel, dim3((unsigned)((size_t)tiles * a.B)), dim3(RX_THREADS), lds, s, a, tiles);
    return hipGetLastError();
}

hipError_t launch_raw_x3_sub(const RawX3Args& a, const RawX3Sub& sub, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (!raw_x3_supported(a.C1, a.depth) || a.N < 1 || a.pcm_stride < 1 || !a.pcm || !a.y || !a.w1 || !a.b1 || !a.packed[0] || !a.bias[0] ||
        (a.depth == 3 && (!a.packed[1] || !a.bias[1])) || a.L[a.depth - 1] < 1 || a.ct_out || sub.nr < 0 || sub.nr > 3)
        return hipErrorInvalidValue;
    const int T = a.L[a.depth - 1], Cl = a.C1 << (a.depth - 1);
    if (sub.ring_rows && (sub.ring_rows < T || sub.row0 < 0 || sub.row0 >= sub.ring_rows)) return hipErrorInvalidValue;
    RawX3SubDev d;
    d.ring_rows = sub.ring_rows; d.row0 = sub.row0;
    d.out_clip_stride = sub.out_clip_stride ? (long long)sub.out_clip_stride : (long long)T * Cl;
    if ((reinterpret_cast<uintptr_t>(a.y) & 15) || (d.out_clip_stride & 3)) return hipErrorInvalidValue;
    // the pieces of one clip, in order (nr = 0: every row)
    int pn[3 * 64], P = 0, nr = 0;
    for (int i = 0; i < (sub.nr ? sub.nr : 1); ++i) {
        const int t0 = sub.nr ? sub.t0[i] : 0, t1 = sub.nr ? sub.t1[i] : T;
        if (t0 < 0 || t1 <= t0 || t1 > T || (nr > 0 && t0 < d.t1[nr - 1])) return hipErrorInvalidValue;
        if (nr > 0 && t0 == d.t1[nr - 1]) d.t1[nr - 1] = t1;   // a range that continues the one before shares its halo
        else { d.t0[nr] = t0; d.t1[nr] = t1; ++nr; }
    }
    for (int i = 0; i < nr; ++i) {
        if ((d.t1[i] - d.t0[i] + RX_ROWS - 1) / RX_ROWS > 64) return hipErrorInvalidValue;
        for (int t = d.t0[i]; t < d.t1[i]; t += RX_ROWS) pn[P++] = std::min(RX_ROWS, d.t1[i] - t);
        d.cum[i] = P;
    }
    d.nr = nr; d.P = P; d.total = (long long)a.B * P;
    // G: the most consecutive pieces - from any piece of a clip on, into the next clips - whose segments and gaps fit the 32-row tile
    int G = 1;
    for (int g = 2; g <= RX_MAXSEG; ++g) {
        bool ok = true;
        for (int c = 0; c < P && ok; ++c) {
            int rows = RX_GAP * (g - 1);
            for (int j = 0; j < g; ++j) rows += pn[(c + j) % P];
            ok = rows <= RX_ROWS;
        }
        if (!ok) break;
        G = g;
    }
    d.G = G;
    const int R0 = a.depth == 3 ? RX_R0 : RX_R1;
    const size_t lds = raw_x3_lds_bytes(a.C1, a.depth) + rx_sub_table_bytes(R0);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const hipError_t e = nww_allow_lds(reinterpret_cast<const void*>(&raw_x3_sub_kernel), lds);
    if (e != hipSuccess) return e;
    const long long grid = (d.total + G - 1) / G;
    if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(raw_x3_sub_kernel, dim3((unsigned)grid), dim3(RX_THREADS), lds, s, a, d);
    return hipGetLastError();
}
