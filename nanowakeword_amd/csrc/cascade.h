// cascade.h - the three kernels of a gate + verifier cascade (cascade.hip) and the host-only arithmetic that sizes the select's grid.
//   cascade_select   probs[n], thr -> the ascending indices of the open windows, their count, and the closed fill of the dense outputs
//   cascade_gather   row j of a dense [rows][N] int16 <- src + idx[j] * row_stride (clips: N, recordings: hop, PCM rings: 2 W)
//   cascade_scatter  the verifier's logits / probabilities [rows] -> out[idx[j]]
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#define CASCADE_MAX_BLOCKS 1024      // blocks of the select: one int of d_counts each, summed by every block of the placement pass
#define CASCADE_COUNT_INTS (CASCADE_MAX_BLOCKS + 1)      // d_counts: the blocks' counts, then the total

// The select's grid for n windows (host-only arithmetic): block b owns the windows [b * per, min(n, (b + 1) * per)), `per` a multiple of
// the block's 256 threads, at most CASCADE_MAX_BLOCKS blocks, about 4096 windows per block before the blocks run out.  64-bit throughout:
// blocks * per reaches past n by up to one `per`, which at n = 2^31 - 1 no longer fits an int.
struct CascadeGrid { int blocks; long long per; };
inline CascadeGrid cascade_grid(long long n) {
    if (n < 1) return {0, 256};
    long long blocks = (n + 4095) / 4096;
    if (blocks > CASCADE_MAX_BLOCKS) blocks = CASCADE_MAX_BLOCKS;
    long long per = (n + blocks - 1) / blocks;
    per = (per + 255) / 256 * 256;
    blocks = (n + per - 1) / per;            // rounding `per` up can leave the last blocks without windows
    return {(int)blocks, per};
}

// d_idx [n], d_counts [CASCADE_COUNT_INTS] (the total lands in d_counts[CASCADE_MAX_BLOCKS]).  fill_logits / fill_probs [n] or null: every
// window's -INFINITY / 0.0f, which the scatter overwrites on the open ones.  1 <= n <= 2^31 - 1.
hipError_t launch_cascade_select(const float* d_probs, long long n, double thr, int32_t* d_idx, int32_t* d_counts, float* fill_logits,
                                 float* fill_probs, hipStream_t s);
// dst [rows][N] dense.  16-byte loads and stores when src, dst, row_stride and N allow, 2-byte ones otherwise (chosen here).
hipError_t launch_cascade_gather(const int16_t* src, const int32_t* d_idx, size_t row_stride, int N, int rows, int16_t* dst, hipStream_t s);
hipError_t launch_cascade_scatter(const int32_t* d_idx, int rows, const float* logits, const float* probs, float* out_logits, float* out_probs,
                                  hipStream_t s);
