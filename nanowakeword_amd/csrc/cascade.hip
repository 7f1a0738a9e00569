// cascade.hip - select / gather / scatter of a gate + verifier cascade (cascade.h).  All three are small and memory-bound: a window costs
// the select 4 bytes read and 8 written, the gather moves a survivor's window once, the scatter 8 bytes per survivor.  The pool select
// is the same select over the table of a pool call (stream_pool.h): it also reads an entry's 24 bytes and writes two lists.
#include "cascade.h"
#include <cmath>

namespace {

// the reference's gate rule on float(np.float32): closed exactly when (double)p < thr, so a NaN probability is open
__device__ __forceinline__ bool cascade_is_open(float p, double thr) { return !((double)p < thr); }

// sum of v over the block's 256 threads (four waves), returned to every thread
__device__ __forceinline__ int block_sum(int v, int* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const int t = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return t;
}

// pass 1: counts[b] = open windows among block b's [b * per, min(n, (b + 1) * per))
__global__ void __launch_bounds__(256) cascade_count_kernel(const float* __restrict__ probs, long long n, double thr, long long per,
                                                            int32_t* __restrict__ counts) {
    __shared__ int red[4];
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    int c = 0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) c += cascade_is_open(probs[i], thr) ? 1 : 0;
    c = block_sum(c, red);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// pass 2: block b starts at the sum of the counts before it (every block adds them up itself: at most CASCADE_MAX_BLOCKS ints) and
// walks its windows again, 256 at a time; a window's place is that base + the open windows of the waves before its own + those of the
// lanes before its own (ballot + popcount).  Ascending and the same on every run: nothing depends on arrival order.
__global__ void __launch_bounds__(256) cascade_place_kernel(const float* __restrict__ probs, long long n, double thr, long long per,
                                                            int32_t* __restrict__ counts, int32_t* __restrict__ idx,
                                                            float* __restrict__ fill_logits, float* __restrict__ fill_probs) {
    __shared__ int red[4];
    __shared__ int wcnt[4];
    int part = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256) part += counts[j];
    int base = block_sum(part, red);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) counts[CASCADE_MAX_BLOCKS] = base + counts[blockIdx.x];
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long i0 = lo; i0 < hi; i0 += 256) {       // the same trip count for the whole block
        const long long i = i0 + threadIdx.x;
        const bool in = i < hi;
        const bool open = in && cascade_is_open(probs[i], thr);
        const unsigned long long m = __ballot(open);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; ++w) {
            const int c = wcnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (open) idx[base + before + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
        if (in) {
            if (fill_logits) fill_logits[i] = -INFINITY;
            if (fill_probs) fill_probs[i] = 0.0f;
        }
        base += total;
        __syncthreads();
    }
}

// ---- the same two passes over the table of a pool call (stream_pool.h): entry i is open when its stream holds a window and the rule
// above opens probs[i]
__device__ __forceinline__ bool pool_entry_open(int group, float p, double thr) { return group != POOL_NOT_FULL && cascade_is_open(p, thr); }

__global__ void __launch_bounds__(256) cascade_pool_count_kernel(const PoolEntry* __restrict__ tab, const float* __restrict__ probs, int n, double thr,
                                                                 int per, int32_t* __restrict__ counts) {
    __shared__ int red[4];
    const int lo = (int)blockIdx.x * per, hi = n - lo < per ? n : lo + per;
    int c = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) c += pool_entry_open(tab[i].group, probs[i], thr) ? 1 : 0;
    c = block_sum(c, red);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// the placement pass of cascade_place_kernel; an open entry leaves its window's ring offset (units of 8 samples) and its own index, and
// every entry its fill: 0 / 0 where the stream holds no window yet, -INFINITY / 0 where it is closed (or open: the scatter overwrites it)
__global__ void __launch_bounds__(256) cascade_pool_place_kernel(const PoolEntry* __restrict__ tab, const float* __restrict__ probs, int n, double thr,
                                                                 int per, int W, int32_t* __restrict__ counts, int32_t* __restrict__ ring8,
                                                                 int32_t* __restrict__ out, float* __restrict__ fill_logits,
                                                                 float* __restrict__ fill_probs) {
    __shared__ int red[4];
    __shared__ int wcnt[4];
    int part = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256) part += counts[j];
    int base = block_sum(part, red);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) counts[CASCADE_MAX_BLOCKS] = base + counts[blockIdx.x];
    const int lo = (int)blockIdx.x * per, hi = n - lo < per ? n : lo + per;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i0 = lo; i0 < hi; i0 += 256) {             // the same trip count for the whole block
        const int i = i0 + (int)threadIdx.x;
        const bool in = i < hi;
        PoolEntry e;
        e.group = POOL_NOT_FULL;
        if (in) e = tab[i];
        const bool open = in && pool_entry_open(e.group, probs[i], thr);
        const unsigned long long m = __ballot(open);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; ++w) {
            const int c = wcnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (open) {
            const int j = base + before + __popcll(m & ((1ull << lane) - 1ull));
            ring8[j] = pool_entry_win8(e, W);
            out[j] = (int32_t)i;
        }
        if (in) {
            if (fill_logits) fill_logits[i] = e.group == POOL_NOT_FULL ? 0.0f : -INFINITY;
            if (fill_probs) fill_probs[i] = 0.0f;
        }
        base += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) cascade_gather16_kernel(const int16_t* __restrict__ src, const int32_t* __restrict__ idx, size_t row_stride,
                                                               int n8, size_t total, uint4* __restrict__ dst) {
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t j = t / (size_t)n8, i = t - j * (size_t)n8;
        dst[t] = *reinterpret_cast<const uint4*>(src + (size_t)idx[j] * row_stride + i * 8);
    }
}

__global__ void __launch_bounds__(256) cascade_gather2_kernel(const int16_t* __restrict__ src, const int32_t* __restrict__ idx, size_t row_stride,
                                                              int N, size_t total, int16_t* __restrict__ dst) {
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t j = t / (size_t)N, i = t - j * (size_t)N;
        dst[t] = src[(size_t)idx[j] * row_stride + i];
    }
}

__global__ void __launch_bounds__(256) cascade_scatter_kernel(const int32_t* __restrict__ idx, int rows, const float* __restrict__ logits,
                                                              const float* __restrict__ probs, float* __restrict__ out_logits,
                                                              float* __restrict__ out_probs) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= rows) return;
    const size_t w = (size_t)idx[j];
    if (out_logits) out_logits[w] = logits[j];
    if (out_probs) out_probs[w] = probs[j];
}

unsigned capped_blocks(size_t total) {
    const size_t b = (total + 255) / 256;
    return (unsigned)(b < (size_t)1 << 20 ? b : (size_t)1 << 20);      // the gathers stride over the grid beyond 2^28 elements
}

}  // namespace

hipError_t launch_cascade_select(const float* d_probs, long long n, double thr, int32_t* d_idx, int32_t* d_counts, float* fill_logits,
                                 float* fill_probs, hipStream_t s) {
    if (n < 1 || n > 0x7fffffffll || !d_probs || !d_idx || !d_counts) return hipErrorInvalidValue;
    const CascadeGrid g = cascade_grid(n);
    hipLaunchKernelGGL(cascade_count_kernel, dim3((unsigned)g.blocks), dim3(256), 0, s, d_probs, n, thr, g.per, d_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cascade_place_kernel, dim3((unsigned)g.blocks), dim3(256), 0, s, d_probs, n, thr, g.per, d_counts, d_idx, fill_logits, fill_probs);
    return hipGetLastError();
}

hipError_t launch_cascade_pool_select(const PoolEntry* d_tab, const float* d_gate_probs, int n, double thr, int W, int32_t* d_ring8, int32_t* d_out,
                                      int32_t* d_counts, float* fill_logits, float* fill_probs, hipStream_t s) {
    if (n < 1 || W < 8 || !d_tab || !d_gate_probs || !d_ring8 || !d_out || !d_counts) return hipErrorInvalidValue;
    const CascadeGrid g = cascade_grid(n);
    hipLaunchKernelGGL(cascade_pool_count_kernel, dim3((unsigned)g.blocks), dim3(256), 0, s, d_tab, d_gate_probs, n, thr, (int)g.per, d_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cascade_pool_place_kernel, dim3((unsigned)g.blocks), dim3(256), 0, s, d_tab, d_gate_probs, n, thr, (int)g.per, W, d_counts, d_ring8,
                       d_out, fill_logits, fill_probs);
    return hipGetLastError();
}

hipError_t launch_cascade_gather(const int16_t* src, const int32_t* d_idx, size_t row_stride, int N, int rows, int16_t* dst, hipStream_t s) {
    if (N < 1 || rows < 1 || row_stride < 1 || !src || !d_idx || !dst) return hipErrorInvalidValue;
    const bool wide = ((uintptr_t)src | (uintptr_t)dst) % 16 == 0 && row_stride % 8 == 0 && N % 8 == 0;
    if (wide) {
        const size_t total = (size_t)rows * (N / 8);
        hipLaunchKernelGGL(cascade_gather16_kernel, dim3(capped_blocks(total)), dim3(256), 0, s, src, d_idx, row_stride, N / 8, total,
                           reinterpret_cast<uint4*>(dst));
    } else {
        const size_t total = (size_t)rows * N;
        hipLaunchKernelGGL(cascade_gather2_kernel, dim3(capped_blocks(total)), dim3(256), 0, s, src, d_idx, row_stride, N, total, dst);
    }
    return hipGetLastError();
}

hipError_t launch_cascade_scatter(const int32_t* d_idx, int rows, const float* logits, const float* probs, float* out_logits, float* out_probs,
                                  hipStream_t s) {
    if (rows < 1 || !d_idx || (out_logits && !logits) || (out_probs && !probs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cascade_scatter_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_idx, rows, logits, probs, out_logits, out_probs);
    return hipGetLastError();
}
