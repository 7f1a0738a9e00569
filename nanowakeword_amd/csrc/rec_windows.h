#pragma once
#include <hip/hip_runtime.h>

// Recording scoring, shared-frame route (nww_recording.hip): the dense head input [B][T][n_mels] of a pass from the frames-major pool
// of its interior frames.  Pool row w * k + t is frame t of window w for every interior t in [el, T - er): a window's interior is ONE
// contiguous run of (T - el - er) * n_mels floats in the pool and in the dense tensor, so the assembly is a copy of B runs whose sources
// lie k rows apart.  n_mels % 4 == 0 and 16-byte aligned bases (checked by the launcher).
// (the raw-PCM heads: rows of the frontend's last stage, n_mels = its channels)
hipError_t launch_rec_assemble(const float* d_pool, float* d_dense, int B, int T, int n_mels, int k, int el, int er, hipStream_t stream);
// p[0, n) = v: the test instrument behind nww_recording_poison
hipError_t launch_rec_fill(float* p, size_t n, float v, hipStream_t stream);
