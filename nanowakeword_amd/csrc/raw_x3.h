// raw_x3.h - the whole raw-PCM frontend (RawAudioFrontend, architectures.py:692-710) in ONE launch under the two-term binary16
// arithmetic (raw_x3.hip): channels 16 or 32, depth 2 or 3.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

struct RawX3Args {
    const int16_t* pcm = nullptr; size_t pcm_stride = 0;
    float* y = nullptr;                    // [B][Lout][C], or [B][C][Lout] with ct_out
    int B = 0, N = 0, depth = 0, C1 = 0, ct_out = 0;
    int L[3] = {0, 0, 0};                  // rows each stage yields for N samples
    const float* w1 = nullptr;             // stage 0 folded, tap-major [41][C1]
    const float* b1 = nullptr;
    // the strided stages behind it (stage 1 and, at depth 3, stage 2): weight fragments packed at plan time (launch_qn_x3_pack on
    // [Cout][13 Cin], tap-major columns), folded bias, un = 1 / (weight scale x scale of the plane the stage reads)
    const unsigned char* packed[2] = {nullptr, nullptr};
    const float* bias[2] = {nullptr, nullptr};
    float un[2] = {0.0f, 0.0f};
    float scale[2] = {0.0f, 0.0f};         // power of two of the plane each of those stages reads, from the plan-time bounds
};
bool raw_x3_supported(int channels, int depth);
size_t raw_x3_lds_bytes(int channels, int depth);
hipError_t launch_raw_x3(const RawX3Args& a, hipStream_t s);
// The row-subset instance (streaming hops, recording scoring): only the rows of up to three ascending ranges [t0, t1) of every clip's
// last stage are computed (nr = 0: all of them), each with the clip's own zero padding and bit for bit as launch_raw_x3 computes it.
// Rows-major output only: row t of clip b at y + b * out_clip_stride + t * C (out_clip_stride = 0: dense clips), or with ring_rows > 0
// at row row0 + t of the clip's ring of 2 * ring_rows rows, and again ring_rows rows away (Fe2Sub, frontend.h).
struct RawX3Sub {
    int nr = 0;
    int t0[3] = {0, 0, 0}, t1[3] = {0, 0, 0};
    int ring_rows = 0, row0 = 0;
    size_t out_clip_stride = 0;
};
hipError_t launch_raw_x3_sub(const RawX3Args& a, const RawX3Sub& sub, hipStream_t s);
