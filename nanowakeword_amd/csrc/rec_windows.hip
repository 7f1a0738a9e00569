// rec_windows.hip - recording scoring, shared-frame route: the dense head input of a pass from the pool of its interior frames.
#include "rec_windows.h"
#include <cstdint>

// blockIdx.y walks the windows, blockIdx.x the 16-byte pieces of a window's interior run: consecutive lanes take consecutive pieces of
// the run (which is contiguous on both sides), four pieces per lane in flight before the first store.  The window / row decomposition is
// the block index: no division per element.
constexpr int REC_BLOCK = 256, REC_UNROLL = 4;
static_assert(REC_UNROLL == 4, "the kernel's full blocks name their four pieces");

__global__ void __launch_bounds__(REC_BLOCK)
rec_assemble_kernel(const float4* __restrict__ pool, float4* __restrict__ dense, int B, int run4, size_t src_win4, size_t dst_win4) {
    const int i0 = (int)blockIdx.x * (REC_BLOCK * REC_UNROLL) + (int)threadIdx.x;
    for (int w = blockIdx.y; w < B; w += gridDim.y) {
        const float4* src = pool + (size_t)w * src_win4;
        float4* dst = dense + (size_t)w * dst_win4;
        if (i0 + (REC_UNROLL - 1) * REC_BLOCK < run4) {
            const float4 v0 = src[i0], v1 = src[i0 + REC_BLOCK], v2 = src[i0 + 2 * REC_BLOCK], v3 = src[i0 + 3 * REC_BLOCK];
            dst[i0] = v0; dst[i0 + REC_BLOCK] = v1; dst[i0 + 2 * REC_BLOCK] = v2; dst[i0 + 3 * REC_BLOCK] = v3;
        } else {                                             // the run's last block
#pragma unroll
            for (int u = 0; u < REC_UNROLL; ++u) {
                const int i = i0 + u * REC_BLOCK;
                if (i < run4) dst[i] = src[i];
            }
        }
    }
}

__global__ void __launch_bounds__(REC_BLOCK) rec_fill_kernel(float* __restrict__ p, size_t n, float v) {
    for (size_t i = (size_t)blockIdx.x * REC_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * REC_BLOCK) p[i] = v;
}

hipError_t launch_rec_fill(float* p, size_t n, float v, hipStream_t stream) {
    if (!p || n == 0) return hipSuccess;
    const size_t blocks = (n + REC_BLOCK - 1) / REC_BLOCK;
    hipLaunchKernelGGL(rec_fill_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(REC_BLOCK), 0, stream, p, n, v);
    return hipGetLastError();
}

hipError_t launch_rec_assemble(const float* d_pool, float* d_dense, int B, int T, int n_mels, int k, int el, int er, hipStream_t stream) {
    if (B <= 0 || T <= 0 || k <= 0 || el < 0 || er < 0 || el + er >= T || n_mels <= 0 || (n_mels & 3)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(d_pool) | reinterpret_cast<uintptr_t>(d_dense)) & 15) return hipErrorInvalidValue;
    const int row4 = n_mels / 4, run4 = (T - el - er) * row4;
    const unsigned gx = (unsigned)((run4 + REC_BLOCK * REC_UNROLL - 1) / (REC_BLOCK * REC_UNROLL)), gy = (unsigned)(B < 65535 ? B : 65535);
    // window w: pool rows [w k + el, w k + T - er) -> dense rows [w T + el, w T + T - er)
    hipLaunchKernelGGL(rec_assemble_kernel, dim3(gx, gy), dim3(REC_BLOCK), 0, stream, reinterpret_cast<const float4*>(d_pool) + (size_t)el * row4,
                       reinterpret_cast<float4*>(d_dense) + (size_t)el * row4, B, run4, (size_t)k * row4, (size_t)T * row4);
    return hipGetLastError();
}
