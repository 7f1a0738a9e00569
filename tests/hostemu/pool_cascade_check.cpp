// pool_cascade_check.cpp - what the cascade's pool select (csrc/cascade.hip) takes from the table of a pool call, against brute force
// (tests/test_cascade_pool_host.py).  The PCM rings of all streams are emulated cell by cell as ONE array [S][2 W], each cell holding the
// number of the sample stored there, written from the call's table alone as pool_push_kernel writes them.  For every call of random join /
// skip / reset schedules: the offset pool_entry_win8 gives for each scored entry - from the entry's own stream and pos, walking the entries
// in LIST order - times 8 must be where the stream's last W samples lie contiguously; and the two compacted lists a select derives for
// a random open set (the threshold rule on random probabilities, a stream that holds no window never open) must be ascending in stream
// number, hold exactly the open entries, and lead the gather to each open stream's window and the scatter to its entry.  The table's own
// win8 list is in SLOT order: the run also counts the calls on which reading it by dense index would have led to another stream's window.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "stream_plan.h"
#include "stream_pool.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++g_fail <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                       \
    } while (0)

struct Totals { long pushes = 0, not_full = 0, whole = 0, primed = 0, mixed = 0, slot_order_differs = 0, opened = 0, closed = 0, none_open = 0, all_open = 0, nan_open = 0; };

// the gate rule of cascade.hip: closed exactly when (double)p < thr
static bool is_open(float p, double thr) { return !((double)p < thr); }

static void run(const FeParams& fe, int W, int hop, unsigned seed, Totals& tot) {
    const int S = 7, T = fe_num_frames(fe, W);
    const HopPlan hp = nww_plan_hop(fe, T, W, hop, 1, true, false, false, [](int, int) { return true; });
    StreamPool p;
    p.open(S, W, hop);
    if (hp.shared) {
        int head, tail;
        pool_primed_spans(fe, W, T, hp.k, hp.el, hp.er, head, tail);
        p.keep_frames((T + hp.k - 1) / hp.k * hp.k, T, hp.k, hp.el, hp.er, head, tail);
    }
#define AT "W=%d hop=%d op=%d", W, hop, op
    std::vector<int64_t> samples((size_t)S, 0);                      // pushed since the stream's last reset
    std::vector<int64_t> ring((size_t)S * 2 * W, -1);                // [S][2 W], flat: what launch_cascade_gather indexes in units of 8
    std::mt19937 rng(seed);
    const int late = (int)(rng() % S), skipper = (int)(rng() % S);   // one stream joins late, one skips every third push
    const int n_ops = 30 + 4 * ((W + hop - 1) / hop);
    for (int op = 0; op < n_ops; ++op) {
        if (rng() % 100 < 6) {                                       // a reset of a few streams
            std::vector<int32_t> idx;
            for (int s = 0; s < S; ++s)
                if (rng() % 4 == 0) idx.push_back(s);
            pool_reset(p, idx.data(), (int)idx.size());
            for (int s : idx) samples[(size_t)s] = 0;
            continue;
        }
        std::vector<int32_t> idx;
        for (int s = 0; s < S; ++s) {
            if (s == late && op < 5) continue;
            if (s == skipper && op % 3 == 2) continue;
            if (rng() % 100 < 85) idx.push_back(s);
        }
        const int n = (int)idx.size();
        PoolCall c;
        pool_plan_push(p, idx.data(), n, c);
        ++tot.pushes;
        // the chunk rows into the rings, as pool_push_kernel places them
        for (int i = 0; i < n; ++i) {
            const PoolEntry& e = c.entries[(size_t)i];
            const int s = e.stream, p0 = ((e.pos - hop) % W + W) % W;
            for (int j = 0; j < hop; ++j) {
                const int q = (p0 + j) % W;
                ring[(size_t)s * 2 * W + q] = ring[(size_t)s * 2 * W + q + W] = samples[(size_t)s] + j;
            }
            samples[(size_t)s] += hop;
        }
        // (1) every scored entry's own offset, in list order
        bool has[3] = {false, false, false}, by_dense_wrong = false;
        for (int i = 0; i < n; ++i) {
            const PoolEntry& e = c.entries[(size_t)i];
            const int s = e.stream;
            has[e.group] = true;
            const bool full = samples[(size_t)s] >= W;
            CHECK((e.group == POOL_NOT_FULL) == !full, AT);
            if (!full) { ++tot.not_full; continue; }
            (e.group == POOL_PRIMED ? tot.primed : tot.whole)++;
            const int64_t off = (int64_t)pool_entry_win8(e, W) * 8, a = samples[(size_t)s] - W;
            CHECK(off >= 0 && off + W <= (int64_t)ring.size() && off % 8 == 0, AT);
            bool ok = off >= 0 && off + W <= (int64_t)ring.size();
            for (int j = 0; j < W && ok; ++j) ok = ring[(size_t)(off + j)] == a + j;
            CHECK(ok, AT);
            CHECK(off / (2 * W) == s, AT);                           // inside the stream's own ring
            CHECK(c.win8[(size_t)e.slot] == pool_entry_win8(e, W), AT);     // the table's list holds the same offset, at the entry's SLOT
            if (c.win8[(size_t)e.dense] != pool_entry_win8(e, W)) by_dense_wrong = true;
        }
        if (has[POOL_NOT_FULL] && has[POOL_WHOLE] && has[POOL_PRIMED]) ++tot.mixed;
        if (by_dense_wrong) ++tot.slot_order_differs;
        // (2) the select's two lists for a random open set
        std::vector<float> probs((size_t)n);
        const unsigned mode = rng() % 8;
        const double thr = mode == 0 ? 0.0 : mode == 1 ? 2.0 : 0.5;
        for (int i = 0; i < n; ++i) {
            probs[(size_t)i] = (float)(rng() % 1000) / 1000.0f;
            if (rng() % 16 == 0) probs[(size_t)i] = 0.5f;               // equal to the threshold: open
            if (rng() % 16 == 0) probs[(size_t)i] = NAN;                // open
        }
        std::vector<int32_t> ring8, out;
        std::vector<int> want_open((size_t)n, 0);
        for (int i = 0; i < n; ++i) {                                   // the placement pass, serially: ascending entries
            const PoolEntry& e = c.entries[(size_t)i];
            const bool open = e.group != POOL_NOT_FULL && is_open(probs[(size_t)i], thr);
            // brute force: the stream holds a window, and its probability is not below the threshold
            want_open[(size_t)i] = samples[(size_t)e.stream] >= W && !(probs[(size_t)i] < thr);
            CHECK(open == (want_open[(size_t)i] != 0), AT);
            if (!open) { if (e.group != POOL_NOT_FULL) ++tot.closed; continue; }
            if (std::isnan(probs[(size_t)i])) ++tot.nan_open;
            ring8.push_back(pool_entry_win8(e, W));
            out.push_back(i);
        }
        const int n_open = (int)out.size();
        tot.opened += n_open;
        if (c.m() > 0 && n_open == 0) ++tot.none_open;
        if (c.m() > 0 && n_open == c.m()) ++tot.all_open;
        if (mode == 0) CHECK(n_open == c.m(), AT);                      // threshold 0 opens exactly the scored streams
        if (mode == 1) {                                                // a threshold above 1 closes all but a NaN, which no comparison closes
            int n_nan = 0;
            for (int i = 0; i < n; ++i) n_nan += c.entries[(size_t)i].group != POOL_NOT_FULL && std::isnan(probs[(size_t)i]);
            CHECK(n_open == n_nan, AT);
        }
        int n_want = 0;
        for (int i = 0; i < n; ++i) n_want += want_open[(size_t)i];
        CHECK(n_open == n_want, AT);
        for (int j = 0; j < n_open; ++j) {
            const int i = out[(size_t)j];
            CHECK(i >= 0 && i < n && want_open[(size_t)i], AT);
            const PoolEntry& e = c.entries[(size_t)i];
            if (j > 0) CHECK(e.stream > c.entries[(size_t)out[(size_t)(j - 1)]].stream, AT);      // ascending in stream number
            CHECK(e.stream == idx[(size_t)i], AT);                      // the scatter writes output i, which belongs to stream idx[i]
            const int64_t off = (int64_t)ring8[(size_t)j] * 8, a = samples[(size_t)e.stream] - W;
            bool ok = off >= 0 && off + W <= (int64_t)ring.size();
            for (int q = 0; q < W && ok; ++q) ok = ring[(size_t)(off + q)] == a + q;      // the gather reads this stream's last W samples
            CHECK(ok, AT);
        }
        pool_commit_push(p, c, true);
        for (int s = 0; s < S; ++s) CHECK(p.of(s).filled == samples[(size_t)s], AT);
    }
#undef AT
}

int main() {
    Totals tot;
    unsigned seed = 1;
    FeParams fe;
    fe.n_fft = 400; fe.hop = 160; fe.center = 1;
    for (int W : {3200, 4800})
        for (int hop : {320, 296})
            for (int rep = 0; rep < 8; ++rep) run(fe, W, hop, seed++, tot);
    std::printf("pushes=%ld not_full=%ld whole=%ld primed=%ld mixed=%ld slot_order_differs=%ld opened=%ld closed=%ld none_open=%ld all_open=%ld nan_open=%ld\n",
                tot.pushes, tot.not_full, tot.whole, tot.primed, tot.mixed, tot.slot_order_differs, tot.opened, tot.closed, tot.none_open, tot.all_open,
                tot.nan_open);
    CHECK(tot.not_full > 0 && tot.whole > 0 && tot.primed > 0 && tot.mixed > 0 && tot.slot_order_differs > 0 && tot.opened > 0 && tot.closed > 0 &&
              tot.none_open > 0 && tot.all_open > 0 && tot.nan_open > 0, "a path of the schedule never ran");
    if (g_fail) std::printf("FAILED %d checks\n", g_fail);
    else std::printf("ok\n");
    return g_fail ? 1 : 0;
}
