// resample.h - launcher of resample.hip: the recordings of a table downmixed, brought to the target rate and converted (include/nww.h,
// nww_resample_*; the arithmetic is resample_plan.h's)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/nww.h"

struct ResampleRatio;

// d_tab [B] is the item table AS UPLOADED: `reserved` carries the item's first tile, a prefix over the table (strictly ascending:
// every item has at least one tile); `tiles` is their total.  span_floats: the largest resample_span of the ratios on the handle (0
// without any).  The formats are NWW_PCM_*.  The table was validated on the host: the kernel checks nothing.
hipError_t resample_launch(const void* d_src, int src_format, const nww_resample_item* d_tab, int B, unsigned tiles, const ResampleRatio* d_ratios,
                           const float* d_taps, int span_floats, void* d_dst, int dst_format, hipStream_t stream);
