// rir.h - launchers of rir.hip: response spectra prepared once, and B clips mixed out of an int16 arena and convolved with them
// (include/nww.h, nww_rir_* / nww_mix_rir_*)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/nww.h"

// M must be one of rir_plan.h's sizes, d_tw its twiddle table (rir_twiddles_host), and the tables validated on the host: the kernels
// check nothing.
// K responses at d_irs + d_off[k] of d_len[k] taps (the first min(len, N) are read) -> d_spectra [K][M / 2] complex
hipError_t rir_prepare_launch(const float* d_irs, const int64_t* d_off, const int32_t* d_len, int K, int N, int M, const float* d_tw,
                              float* d_spectra, hipStream_t stream);
// The segmented route (NWW_RIR_SEGMENTED; rir_plan.h): d_spectra holds rir_spectra_floats(K, N, longest, NWW_RIR_SEGMENTED) floats, P_max
// = rir_parts(N, longest); d_w [B][N] float32 and d_peaks [B][rir_segments(N)] are the caller's scratch
hipError_t rir_seg_prepare_launch(const float* d_irs, const int64_t* d_off, const int32_t* d_len, int K, int N, int P_max, const float* d_tw,
                                  float* d_spectra, hipStream_t stream);
hipError_t rir_seg_mix_launch(const int16_t* d_arena, const nww_mix_item* d_tab, const nww_rir_item* d_rtab, const float* d_spectra,
                              const float* d_tw, int B, int N, float* d_w, unsigned* d_peaks, int16_t* d_out, hipStream_t stream,
                              const nww_pitch_item* d_ptab = nullptr, const float* d_y = nullptr);
// d_rtab [B]: a clip's response (-1: none, the clip mix.hip gives)
// d_ptab / d_y (both routes; nww_mix_aug_*): the pitch table as pitch.h describes it and pitch.hip's shifted clips [rows][N] - a clip
// with pitch_id >= 0 is staged from its row instead of being mixed; null: the instances as they always were
hipError_t rir_mix_launch(const int16_t* d_arena, const nww_mix_item* d_tab, const nww_rir_item* d_rtab, const float* d_spectra, int M,
                          const float* d_tw, int B, int N, int16_t* d_out, hipStream_t stream, const nww_pitch_item* d_ptab = nullptr,
                          const float* d_y = nullptr);
