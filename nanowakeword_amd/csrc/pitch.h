// pitch.h - launchers of pitch.hip: the clips of a table that name a ratio mixed to float32, stretched by the phase vocoder and resampled
// back to N samples (include/nww.h, nww_pitch_* / nww_mix_aug_*; the arithmetic is pitch_plan.h's)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/nww.h"

// a ratio on the device: p / q and where its q * PITCH_TAPS taps start in the taps buffer
struct PitchRatio { int32_t p, q, off, pad; };

// the constant tables of every call, back to back in one device buffer (floats): twiddles of the 512-point transform [384][2], the
// window [512], the envelope [16][128]
constexpr int PITCH_TAB_TW = 0, PITCH_TAB_WIN = 768, PITCH_TAB_ENV = 1280, PITCH_TAB_FLOATS = 1280 + 2048;

// d_ptab [B] is the pitch table AS UPLOADED: pitch_id (-1: the clip is left alone by every kernel here) and, in `reserved`, the clip's
// row in the scratch.  d_w [rows][N] receives mix_plan.h's y and then, in its place, the shifted clip; d_s [rows][s_stride] is the
// stretched signal.  With d_out the clips named are finished as well - peak, ratio, mix_out - into d_out [B][N]; without, d_w is left
// for rir.hip's instances that stage from it.  The tables were validated on the host: the kernels check nothing.
hipError_t pitch_launch(const int16_t* d_arena, const nww_mix_item* d_tab, const nww_pitch_item* d_ptab, const PitchRatio* d_ratios,
                        const float* d_taps, const float* d_tables, int B, int N, float* d_w, float* d_s, int s_stride, int16_t* d_out,
                        hipStream_t stream);
