// stream_plan.h - what a (window, hop) pair shares between consecutive windows: host-only integer arithmetic (no HIP header; g++ compiles
// it for tests/test_stream_plan_host.py).  nww_stream_open keeps rings by it, the recording route shares a pass's interior frames by it.
#pragma once
#include "fe_tables.h"

// the first el and last er of a W-sample window's T frames read its reflect padding (centred frontends; 0 / 0 otherwise): every other frame is
// the same samples, hence the same log-mel bits, in whichever window of a stream or recording it falls
inline void nww_edge_frames(const FeParams& fe, int T, int W, int& el, int& er) {
    const int pad = fe.center ? fe.n_fft / 2 : 0;
    el = er = 0;
    while (el < T && el * fe.hop - pad < 0) ++el;
    while (er < T && (T - 1 - er) * fe.hop - pad + fe.n_fft > W) ++er;
}

// The frames a hop of k frames computes in a window of T: the leading edge [0, el), the k new interior frames [T - er - k, T - er) and the
// trailing edge [T - er, T) as a range of its own (the frontend groups frames range by range) - ascending, disjoint, none empty, so at
// most three.  k = 0: a window's edge frames alone (the recording route).  Needs el <= T - er - k, which a shared HopPlan guarantees.
// Sub: Fe2Sub (frontend.h), or anything with its nr, t0[4] and t1[4].
template <class Sub>
void nww_hop_ranges(int T, int k, int el, int er, Sub& sub) {
    sub.nr = 0;
    auto add = [&](int a, int b) {
        if (a < b) { sub.t0[sub.nr] = a; sub.t1[sub.nr] = b; ++sub.nr; }
    };
    add(0, el);
    add(T - er - k, T - er);
    add(T - er, T);
}

// A hop of k = hop / hop_length frames turns frame t of the old window into frame t - k of the new one, bit for bit, unless the frame
// touches the reflect padding of either window: per hop only frames [0, el) and [T - er - k, T) are computed (`shared`).
// Likewise pooled row j of the fused trunk (input rows 4j - 3 .. 4j + 6) equals row j + k / 4 of the previous window when those rows are
// shifted interior frames in both windows: rows [a2_lo, a2_hi] of the a2_rows are kept, the strips [sub_a, sub_b) recomputed (`conv`).
// And pooled row j of the third conv (input rows 8j - 7 .. 8j + 14) equals row j + k / 8 of the previous hop: rows [a3_lo, a3_hi] of
// its sequence output are carried over (`seq`).
struct HopPlan {
    bool valid = false;          // window and hop are positive multiples of 8 samples with hop <= window
    int T = 0, k = 0, el = 0, er = 0;
    bool shared = false, conv = false, seq = false;
    int a2_rows = 0, a2_lo = 0, a2_hi = -1, a2_shift = 0, nsub = 0, sub_a[4] = {0, 0, 0, 0}, sub_b[4] = {0, 0, 0, 0};
    int a3_lo = 0, a3_hi = -1, a3_shift = 0;
};

// level (NWW_STREAM_INC): 0 = nothing is shared, 1 = frames, 2 = + the fused trunk's rows, 3 = + the third conv's rows.  fe_subsets: the
// input is frames-major and the frame-subset frontend instances exist; trunk: a fused trunk -> third conv pair works on the T-row
// plane, seq: and that conv writes the sequence layout; fits(a, b): pooled rows [a, b) are a strip the fused trunk can hold in LDS.
template <class Fits>
HopPlan nww_plan_hop(const FeParams& fe, int T, int W, int hop, int level, bool fe_subsets, bool trunk, bool seq, Fits fits) {
    HopPlan p;
    p.T = T;
    p.valid = W > 0 && hop > 0 && hop <= W && (W % 8) == 0 && (hop % 8) == 0;
    if (!p.valid || level <= 0 || !fe_subsets || hop % fe.hop != 0) return p;
    const int k = hop / fe.hop;
    int el, er;
    nww_edge_frames(fe, T, W, el, er);
    if (T - er - k <= el) return p;                            // a hop replaces (nearly) the whole window: nothing to keep
    p.k = k; p.el = el; p.er = er; p.shared = true;
    if (level < 2 || !trunk || (k % 4) != 0) return p;
    const int H2 = T / 4, lo = (el + 3 + 3) / 4, hi = (T - 1 - er - k - 6) >= 0 ? (T - 1 - er - k - 6) / 4 : -1;
    // The rows a hop recomputes - [0, lo) and (hi, H2) - go to the fused trunk as explicit strips, and a strip must fit in LDS:
    // each range is cut into the fewest equal pieces that do (at most four strips in all, TrunkArgs::sub_a).  A window / hop pair
    // that would need more keeps the frontend ring only and re-scores the conv rows (hops of 68-84 frames at W = 16000
    // asked for a 165-198 KB strip and every hop after the first full window failed).
    bool ok = hi >= lo && hi < H2;
    auto cut = [&](int a, int b) {
        if (a >= b || !ok) return;
        for (int n = 1; n <= 4 && n <= b - a && p.nsub + n <= 4; ++n) {
            bool all = true;
            for (int q = 0; q < n && all; ++q) all = fits(a + (b - a) * q / n, a + (b - a) * (q + 1) / n);
            if (!all) continue;
            for (int q = 0; q < n; ++q) { p.sub_a[p.nsub] = a + (b - a) * q / n; p.sub_b[p.nsub] = a + (b - a) * (q + 1) / n; ++p.nsub; }
            return;
        }
        ok = false;
    };
    cut(0, lo);
    cut(hi + 1, H2);
    if (!ok) { p.nsub = 0; return p; }
    p.conv = true; p.a2_rows = H2; p.a2_lo = lo; p.a2_hi = hi; p.a2_shift = k / 4;
    const int H3 = H2 / 2, lo3 = (el + 7 + 7) / 8, hi3 = (T - 1 - er - k - 14) >= 0 ? (T - 1 - er - k - 14) / 8 : -1;
    if (level >= 3 && seq && (k % 8) == 0 && hi3 >= lo3 && hi3 < H3) { p.seq = true; p.a3_lo = lo3; p.a3_hi = hi3; p.a3_shift = k / 8; }
    return p;
}
