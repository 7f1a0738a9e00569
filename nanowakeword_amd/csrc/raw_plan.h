// raw_plan.h - what a (window, hop) pair shares between consecutive windows of a raw-PCM head: host-only integer arithmetic beside
// stream_plan.h (no HIP header; g++ compiles it for tests/test_raw_plan_host.py).  RawAudioFrontend is a stack of zero-padded strided
// convolutions: stage 0 has k 41, stride 16, pad 20, every later stage k 13, stride 4, pad 6.
#pragma once
#include "stream_plan.h"

// samples between consecutive rows of the last stage
inline int nww_raw_total_stride(int depth) { return 16 << (2 * (depth - 1)); }

// rows the last stage yields for W samples (the frame law of nww_pcm_rows)
inline int nww_raw_rows(int depth, int W) {
    if (W < 1 || depth < 1) return 0;
    int L = (W - 1) / 16 + 1;
    for (int i = 1; i < depth; ++i) L = (L - 1) / 4 + 1;
    return L;
}

// A row is interior when every tap reads real data: samples of [0, W) at stage 0, interior rows of the stage before at a later stage.
// The other rows of the last stage - they see the window's own zero padding, directly or through a padded row of an earlier stage -
// are its first el and last er rows (el = T, er = 0 when no row is interior).  Returns T.
inline int nww_raw_edge_rows(int depth, int W, int& el, int& er) {
    const int T = nww_raw_rows(depth, W);
    auto floor_div = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    // interior rows [lo, hi] stage by stage: row r reads samples 16 r - 20 .. 16 r + 20, later rows 4 r - 6 .. 4 r + 6 of the stage before
    int lo = 2, hi = floor_div(W - 21, 16);
    for (int i = 1; i < depth; ++i) { lo = (lo + 6 + 3) / 4; hi = floor_div(hi - 6, 4); }
    if (T < 1 || hi < lo) { el = T; er = 0; return T; }
    el = lo; er = T - 1 - hi;
    return T;
}

// A hop of k = hop / stride rows (stride = 16 . 4^(depth - 1)) turns interior row t of the old window into row t - k of the new one, bit
// for bit - the fused frontend's scales are plan-time constants and its sums run in a fixed order (raw_x3.hip) - so per hop only rows
// [0, el) and [T - er - k, T) are computed, and interior row t of window w of a recording is row w k + t of the frontend run over the
// whole span as one clip.  fused: the one-launch frontend is planned (its row-subset instance exists); level: NWW_STREAM_INC /
// NWW_REC_SHARED.  Only valid, T, k, el, er and shared are set: the raw heads keep no pooled rows.
inline HopPlan nww_plan_hop_raw(int depth, int W, int hop, int level, bool fused) {
    HopPlan p;
    int el = 0, er = 0;
    p.T = nww_raw_edge_rows(depth, W, el, er);
    p.valid = W > 0 && hop > 0 && hop <= W && (W % 8) == 0 && (hop % 8) == 0;
    const int stride = nww_raw_total_stride(depth);
    if (!p.valid || level <= 0 || !fused || hop % stride != 0) return p;
    const int k = hop / stride;
    if (p.T - er - k <= el) return p;                          // a hop replaces (nearly) the whole window: nothing to keep
    p.k = k; p.el = el; p.er = er; p.shared = true;
    return p;
}
