// mix.h - launcher of mix.hip: B clips mixed out of an int16 arena by a device table of validated items (include/nww.h, nww_mix_*)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/nww.h"

// d_tab [B] must have passed mix_first_bad_item (mix_plan.h) against the arena: the kernel checks nothing
hipError_t mix_launch(const int16_t* d_arena, const nww_mix_item* d_tab, int B, int N, int16_t* d_out, int cu_count, hipStream_t stream);
