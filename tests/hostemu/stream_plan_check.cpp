// stream_plan_check.cpp - nww_plan_hop (csrc/stream_plan.h) against brute force over receptive fields (tests/test_stream_plan_host.py).
// Nothing here repeats the plan's closed forms: edge frames come from sample spans, kept rows from the frames each pooled row reads,
// and whether a strip cover exists from a search over all cuts.
#include <cstdio>
#include <vector>
#include "stream_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++g_fail <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                       \
    } while (0)

struct Brute {
    const FeParams& fe;
    int T, W, k;
    bool edge(int t) const {               // the frame's sample span leaves [0, W)
        const int a = t * fe.hop - (fe.center ? fe.n_fft / 2 : 0);
        return a < 0 || a + fe.n_fft > W;
    }
    // frame t of the new window is frame t + k of the previous one, an interior frame in both
    bool carried(int t) const { return t >= 0 && t < T && !edge(t) && t + k < T && !edge(t + k); }
    // pooled row j reads frames [stride j - before, stride j + after]
    bool kept(int j, int stride, int before, int after) const {
        if (k % stride) return false;
        for (int t = stride * j - before; t <= stride * j + after; ++t)
            if (!carried(t)) return false;
        return true;
    }
};

// fewest accepted strips that tile [a, b) (any cuts), or 99
template <class Fits>
static int min_cover(int a, int b, Fits fits) {
    std::vector<int> best(b - a + 1, 99);
    best[0] = 0;
    for (int e = a + 1; e <= b; ++e)
        for (int s = a; s < e; ++s)
            if (best[s - a] < 99 && fits(s, e) && best[s - a] + 1 < best[e - a]) best[e - a] = best[s - a] + 1;
    return best[b - a];
}

struct Counts { long plans = 0, shared = 0, conv = 0, seq = 0, cut = 0, gave_up = 0, ranges = 0, two = 0, three = 0; };

// nww_hop_ranges: ascending, disjoint, none empty, at most four; their union is exactly [0, el) and [T - er - k, T), and the trailing er
// frames are a range of their own
struct Ranges { int nr = -1, t0[4] = {0, 0, 0, 0}, t1[4] = {0, 0, 0, 0}; };
static void check_ranges(int T, int k, int el, int er, Counts& n) {
    Ranges r;
    nww_hop_ranges(T, k, el, er, r);
    ++n.ranges;
#define AT "T=%d k=%d el=%d er=%d", T, k, el, er
    CHECK(r.nr >= 0 && r.nr <= 4, AT);
    std::vector<int> hit(T, 0);
    bool trailing = er == 0;
    for (int q = 0; q < r.nr && q < 4; ++q) {
        CHECK(r.t0[q] >= 0 && r.t0[q] < r.t1[q] && r.t1[q] <= T && (q == 0 || r.t1[q - 1] <= r.t0[q]), AT);
        for (int t = r.t0[q]; t < r.t1[q] && t < T; ++t) ++hit[t < 0 ? 0 : t];
        if (r.t0[q] == T - er && r.t1[q] == T) trailing = true;
    }
    for (int t = 0; t < T; ++t) CHECK(hit[t] == ((t < el || t >= T - er - k) ? 1 : 0), AT);
    CHECK(trailing, AT);
    if (r.nr == 2) ++n.two;
    if (r.nr == 3) ++n.three;
#undef AT
}

template <class Fits>
static void check_pair(const FeParams& fe, int W, int hop, Fits fits, const char* pred, Counts& n) {
    const int T = fe_num_frames(fe, W);
    for (int level = 0; level <= 3; ++level) {
        const HopPlan p = nww_plan_hop(fe, T, W, hop, level, true, true, true, fits);
        ++n.plans;
#define AT "center=%d W=%d hop=%d level=%d pred=%s", fe.center, W, hop, level, pred
        CHECK(p.valid && p.T == T, AT);
        const int k = hop % fe.hop ? 0 : hop / fe.hop;
        const Brute b{fe, T, W, k};
        int el = 0, er = 0, n_carried = 0;
        for (int t = 0; t < T; ++t) {
            if (t * fe.hop - (fe.center ? fe.n_fft / 2 : 0) < 0) ++el;
            else if (b.edge(t)) ++er;
            if (k > 0 && b.carried(t)) ++n_carried;
        }
        const bool shared = level >= 1 && k > 0 && n_carried > 0;
        CHECK(p.shared == shared, AT);
        if (!p.shared) { CHECK(!p.conv && !p.seq && p.nsub == 0, AT); continue; }
        ++n.shared;
        CHECK(p.k == k && p.el == el && p.er == er, AT);
        check_ranges(T, k, el, er, n);                                                 // the frames a hop computes, and a recording window's edge frames
        check_ranges(T, 0, el, er, n);
        // the fused trunk's pooled rows
        const int H2 = T / 4;
        int lo = -1, hi = -1, kept = 0;
        for (int j = 0; j < H2; ++j)
            if (b.kept(j, 4, 3, 6)) { if (lo < 0) lo = j; hi = j; ++kept; }
        CHECK(kept == 0 || kept == hi - lo + 1, AT);                                   // one run
        const bool cover = kept > 0 && min_cover(0, lo, fits) + min_cover(hi + 1, H2, fits) <= 4;
        CHECK(p.conv == (level >= 2 && cover), AT);
        if (level >= 2 && kept > 0 && !cover) ++n.gave_up;                             // the frontend ring only
        if (!p.conv) { CHECK(!p.seq && p.nsub == 0, AT); continue; }
        ++n.conv;
        CHECK(k % 4 == 0 && p.a2_rows == H2 && p.a2_lo == lo && p.a2_hi == hi && p.a2_shift == k / 4, AT);
        CHECK(p.nsub >= 0 && p.nsub <= 4, AT);
        std::vector<int> hit(H2, 0);
        for (int q = 0; q < p.nsub; ++q) {
            CHECK(p.sub_a[q] >= 0 && p.sub_a[q] < p.sub_b[q] && p.sub_b[q] <= H2 && (q == 0 || p.sub_b[q - 1] <= p.sub_a[q]), AT);
            CHECK(fits(p.sub_a[q], p.sub_b[q]), AT);
            for (int j = p.sub_a[q]; j < p.sub_b[q] && j < H2; ++j) ++hit[j < 0 ? 0 : j];
        }
        for (int j = 0; j < H2; ++j) CHECK(hit[j] == ((j < lo || j > hi) ? 1 : 0), AT);
        if (p.nsub > (lo > 0) + (hi + 1 < H2)) ++n.cut;                                 // a range went out in more than one strip
        // the third conv's pooled rows
        const int H3 = H2 / 2;
        int lo3 = -1, hi3 = -1, kept3 = 0;
        for (int j = 0; j < H3; ++j)
            if (b.kept(j, 8, 7, 14)) { if (lo3 < 0) lo3 = j; hi3 = j; ++kept3; }
        CHECK(kept3 == 0 || kept3 == hi3 - lo3 + 1, AT);
        CHECK(p.seq == (level >= 3 && kept3 > 0), AT);
        if (p.seq) { ++n.seq; CHECK(k % 8 == 0 && p.a3_lo == lo3 && p.a3_hi == hi3 && p.a3_shift == k / 8, AT); }
    }
    // the recording route shares frames (level 1) exactly where a stream keeps a log-mel ring (any level >= 1)
    const bool rec = nww_plan_hop(fe, T, W, hop, 1, true, true, true, fits).shared;
    for (int level = 1; level <= 3; ++level) CHECK(nww_plan_hop(fe, T, W, hop, level, true, true, true, fits).shared == rec, AT);
    const int level = 3;
    CHECK(!nww_plan_hop(fe, T, W, hop, level, false, true, true, fits).shared, AT);   // no frame-subset frontend: nothing is kept
#undef AT
}

int main() {
    auto any = [](int, int) { return true; };
    auto five = [](int a, int b) { return b - a <= 5; };
    Counts all, small;
    for (int center = 0; center <= 1; ++center) {
        FeParams fe;
        fe.n_fft = 400; fe.hop = 160; fe.center = center;
        for (int W : {4800, 16000, 24000}) {
            for (int hop = 8; hop <= W; hop += 8) {
                check_pair(fe, W, hop, any, "any", all);
                check_pair(fe, W, hop, five, "five", small);
            }
            // the window / hop rule
            for (int bad : {0, -8, 4, 12, W + 8}) CHECK(!nww_plan_hop(fe, fe_num_frames(fe, W), W, bad, 3, true, true, true, any).valid, "hop=%d W=%d", bad, W);
            CHECK(!nww_plan_hop(fe, fe_num_frames(fe, W + 4), W + 4, 8, 3, true, true, true, any).valid, "W=%d", W + 4);
        }
    }
    for (const Counts* c : {&all, &small})
        std::printf("plans=%ld shared=%ld conv=%ld seq=%ld cut=%ld gave_up=%ld ranges=%ld two=%ld three=%ld\n", c->plans, c->shared, c->conv, c->seq, c->cut, c->gave_up,
                    c->ranges, c->two, c->three);
    // both paths of the strip cutter occur: a range that goes out in several strips, and a pair that keeps the frontend ring only
    CHECK(small.cut > 0 && small.gave_up > 0, "cut=%ld gave_up=%ld", small.cut, small.gave_up);
    CHECK(all.conv > 0 && all.seq > 0 && all.gave_up == 0, "conv=%ld seq=%ld", all.conv, all.seq);
    // a centred frontend's hop has three ranges, its recording window two
    CHECK(all.ranges > 0 && all.two > 0 && all.three > 0, "ranges=%ld two=%ld three=%ld", all.ranges, all.two, all.three);
    if (g_fail) std::printf("FAILED %d checks\n", g_fail);
    else std::printf("ok\n");
    return g_fail ? 1 : 0;
}
