// cascade.h - the three kernels of a gate + verifier cascade (cascade.hip) and the host-only arithmetic that sizes the select's grid.
//   cascade_select   probs[n], thr -> the ascending indices of the open windows, their count, and the closed fill of the dense outputs
//   cascade_gather   row j of a dense [rows][N] int16 <- src + idx[j] * row_stride (clips: N, recordings: hop, PCM rings: 2 W)
//   cascade_scatter  the verifier's logits / probabilities [rows] -> out[idx[j]]
//   cascade_pool_select  the select over the listed streams of a pool call: ring offsets for the gather, entries for the scatter
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "stream_pool.h"

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
// The select over the table of a pool call (stream_pool.h): the same count / prefix sum / placement, walking the call's n entries.  Entry i
// is a candidate unless its group is POOL_NOT_FULL, and open by the rule above on d_gate_probs[i] ([n], in list order).  The open
// entries, ascending, leave two lists: d_ring8[j], the start of the stream's window in the double-written PCM rings in units of 8
// samples (from the entry's own stream and pos: what launch_cascade_gather takes with row_stride 8), and d_out[j] = i (what
// launch_cascade_scatter takes).  fill_logits / fill_probs [n] or null: 0 / 0 for a stream that holds no window, -INFINITY / 0 for a
// closed one.  Both lists [n]; d_counts as above.  1 <= n <= 2^31 - 1; the rings hold at most 2^31 - 1 units (checked where they are made).
hipError_t launch_cascade_pool_select(const PoolEntry* d_tab, const float* d_gate_probs, int n, double thr, int W, int32_t* d_ring8, int32_t* d_out,
                                      int32_t* d_counts, float* fill_logits, float* fill_probs, hipStream_t s);
