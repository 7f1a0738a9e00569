// raw_plan_check.cpp - nww_raw_edge_rows / nww_plan_hop_raw (csrc/raw_plan.h) against a brute-force walk over receptive fields
// (tests/test_raw_plan_host.py).  Nothing here repeats the header's closed forms: a stage's rows are counted from the convolution's
// definition on the padded input, and a row is interior when every tap it reads is real data or an interior row of the stage before.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "raw_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++g_fail <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                       \
    } while (0)

// rows of Conv1d(k, stride, pad) on L inputs, by its definition: windows of k that fit into the padded input
static int conv_rows(int L, int k, int stride, int pad) {
    int n = 0;
    for (int r = 0; r * stride + k <= L + 2 * pad; ++r) ++n;
    return n;
}

// interior flags of the last stage's rows for a W-sample window
static std::vector<char> interior_rows(int depth, int W) {
    std::vector<char> prev(W, 1);                               // the samples themselves
    for (int i = 0; i < depth; ++i) {
        const int k = i == 0 ? 41 : 13, stride = i == 0 ? 16 : 4, pad = k / 2, L = (int)prev.size();
        std::vector<char> cur(conv_rows(L, k, stride, pad), 1);
        for (int r = 0; r < (int)cur.size(); ++r)
            for (int j = 0; j < k; ++j) {
                const int x = r * stride - pad + j;
                if (x < 0 || x >= L || !prev[x]) cur[r] = 0;
            }
        prev.swap(cur);
    }
    return prev;
}

struct Counts { long windows = 0, plans = 0, shared = 0; };

static void check_window(int depth, int W, Counts& n) {
    ++n.windows;
    const std::vector<char> in = interior_rows(depth, W);
    const int T = (int)in.size(), stride = nww_raw_total_stride(depth);
    int s = 16;
    for (int i = 1; i < depth; ++i) s *= 4;
    CHECK(stride == s, "depth=%d", depth);
    int el = 0, er = 0, mid = 0;
    while (el < T && !in[el]) ++el;
    while (er < T - el && !in[T - 1 - er]) ++er;
    for (int t = el; t < T - er; ++t) mid += in[t] ? 0 : 1;
    CHECK(mid == 0, "depth=%d W=%d: the edge rows are not a prefix and a suffix", depth, W);
    int pel = -1, per = -1;
    const int pT = nww_raw_edge_rows(depth, W, pel, per);
    CHECK(pT == T && nww_raw_rows(depth, W) == T, "depth=%d W=%d T=%d plan %d", depth, W, T, pT);
    CHECK(pel == el && per == er, "depth=%d W=%d el=%d er=%d plan %d %d", depth, W, el, er, pel, per);
    // hops: one row, five rows, the largest hop that leaves an interior row to share, the next one, and one that is no whole row
    const int kmax = T - er - el - 1;
    std::vector<int> hops = {stride, 5 * stride, stride + 8};
    if (kmax >= 1) { hops.push_back(kmax * stride); hops.push_back((kmax + 1) * stride); }
    for (int hop : hops)
        for (int level = 0; level <= 3; ++level)
            for (int fused = 0; fused <= 1; ++fused) {
                ++n.plans;
                const HopPlan p = nww_plan_hop_raw(depth, W, hop, level, fused != 0);
#define AT "depth=%d W=%d hop=%d level=%d fused=%d", depth, W, hop, level, fused
                const bool valid = W % 8 == 0 && hop % 8 == 0 && hop <= W;
                CHECK(p.valid == valid && p.T == T, AT);
                const int k = hop % stride ? 0 : hop / stride;
                int carried = 0;                                // rows of the new window that are interior rows of the previous one too
                for (int t = 0; k > 0 && t + k < T; ++t) carried += in[t] && in[t + k];
                const bool shared = valid && level >= 1 && fused && k > 0 && carried > 0;
                CHECK(p.shared == shared, AT);
                CHECK(!p.conv && !p.seq && p.nsub == 0, AT);
                if (!p.shared) continue;
                ++n.shared;
                CHECK(p.k == k && p.el == el && p.er == er && T - er - k > el, AT);
                // the pool: the span of B windows as one clip has exactly the rows the windows read, and window w's interior row t
                // reads the samples of the span's row w k + t
                for (int B : {1, 2, 7}) CHECK(nww_raw_rows(depth, (B - 1) * hop + W) == (B - 1) * k + T, AT);
#undef AT
            }
}

int main(int argc, char** argv) {
    if (argc == 4) {                        // depth W hop -> the plan (level 1, fused), for the test's float64 check of what it claims
        const HopPlan p = nww_plan_hop_raw(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), 1, true);
        std::printf("%d %d %d %d %d\n", p.T, p.k, p.el, p.er, p.shared ? 1 : 0);
        return 0;
    }
    Counts n;
    for (int depth = 1; depth <= 4; ++depth) {
        for (int W = 16; W <= 1100; ++W) check_window(depth, W, n);
        for (int W : {4000, 4096, 15999, 16000, 16001, 32000}) check_window(depth, W, n);
    }
    // the issue's examples
    struct { int depth, W, T, el, er; } ex[] = {{3, 16000, 63, 2, 2}, {3, 4096, 16, 2, 1}, {3, 4000, 16, 2, 2}, {2, 16000, 250, 2, 1}};
    for (const auto& e : ex) {
        int el, er;
        const int T = nww_raw_edge_rows(e.depth, e.W, el, er);
        CHECK(T == e.T && el == e.el && er == e.er, "depth=%d W=%d: T=%d el=%d er=%d", e.depth, e.W, T, el, er);
    }
    // the window / hop rule of nww_plan_hop
    for (int bad : {0, -16, 4, 12, 16008}) CHECK(!nww_plan_hop_raw(3, 16000, bad, 3, true).valid, "hop=%d", bad);
    std::printf("windows=%ld plans=%ld shared=%ld\n", n.windows, n.plans, n.shared);
    CHECK(n.shared > 0, "no plan shared anything");
    if (g_fail) std::printf("FAILED %d checks\n", g_fail);
    else std::printf("ok\n");
    return g_fail ? 1 : 0;
}
