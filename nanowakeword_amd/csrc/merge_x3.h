// merge_x3.h - the E-Branchformer block's branch merge in ONE row-local launch (merge_x3.hip; EBranchformerBlock / MergingModule,
// architectures.py:555-594):  x <- LayerNorm(x + a g + c (1 - g)),  c = s Wc^T + bc (conv_branch.conv2),  g = sigmoid(c Wg^T + bg)
// (merger.gate), from the depthwise stage's output s, the attention branch's output a and the residual stream x.  c and g stay on chip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct MergeArgs {
    const float* s;                  // [M][D] swish(BN(depthwise(...))): the conv module up to its last pointwise conv
    const float* a;                  // [M][D] attention branch output
    float* x;                        // [M][D] residual stream, updated in place (a workgroup reads and writes only its own 64 rows)
    const unsigned char* packed;     // launch_merge_x3_pack output: Wc fragments, then Wg fragments
    const float *bc, *bg;            // [D] biases of conv2 and of the gate
    const float *ln_w, *ln_b;        // [D] final_norm
    int M;
    float wc_un, wg_un;              // 1 / (scale of the packed conv2 / gate weights)
};

bool merge_x3_supported(int D);      // widths with a compiled instance
size_t merge_x3_packed_bytes(int D);
// Wc [D][D], Wg [D][D] float32 -> two binary16 terms of Wc wsc / Wg wsg in MFMA fragment order
hipError_t launch_merge_x3_pack(const float* Wc, const float* Wg, void* packed, int D, float wsc, float wsg, hipStream_t s);
hipError_t launch_merge_x3(const MergeArgs& a, int D, hipStream_t s);
