// stream_pool_check.cpp - the ring state arithmetic of csrc/stream_pool.h against brute force (tests/test_stream_pool_host.py), through the
// very functions nww_stream.hip calls: pool calls (pool_plan_push / pool_commit_push / pool_reset), lock-step pushes (pool_lock_ok /
// pool_lock_plan / pool_lock_commit) and whole-batch resets (pool_reset_all).
// The brute force keeps, per stream, ONE sample counter, the list of frame origins of its current window, how often its log-mel ring has
// been rotated and whether that ring holds its window; the rings are emulated cell by cell from what a call hands to the device alone
// (what the kernels of nww_stream.hip do with a pool call's table, and what the lock-step frontend does with the hop's frame ranges,
// nww_hop_ranges, written straight into the double-written ring), each PCM cell holding the number of the sample stored there and each
// log-mel row the identity of the frame stored there: its first sample, and for a frame that reads the window's own padding the window's
// first sample too.  After every push the window read at the reported offset must be the last W samples in order, and the T rows read at
// the reported row must be the current window's frames - through ring wrap-arounds, chunks split across the ring's end, joins, resets
// of single streams and of the whole batch, hand-overs between lock-step and pool calls in both directions, and failed lock-step hops
// (which leave garbage in the rows they would have written).  A lock-step push is a push of every stream; it must be permitted exactly
// when the brute force's streams have all been equal since the last whole reset.
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

struct FrameId {
    int64_t origin = -1, window = -1;          // window: -1 for a frame whose samples all lie inside the window
    bool operator==(const FrameId& o) const { return origin == o.origin && window == o.window; }
};

struct BruteStream {
    int64_t samples = 0;                       // pushed since its last reset
    int64_t rotated = 0;                       // hops that rotated its log-mel ring since its last reset
    bool valid = false;                        // its log-mel ring holds its current window
    std::vector<FrameId> frames;               // of the current window
    bool same(const BruteStream& o) const { return samples == o.samples && rotated == o.rotated && valid == o.valid; }
};

struct Ranges { int nr = 0, t0[4] = {0, 0, 0, 0}, t1[4] = {0, 0, 0, 0}; };

struct Totals {
    long pushes = 0, not_full = 0, whole = 0, primed = 0, pcm_wraps = 0, lm_wraps = 0, split_chunks = 0, unaligned = 0, realigned = 0, staged = 0, windows = 0;
    long lock = 0, lock_primed = 0, lock_primed_after_pool = 0, lock_refused = 0, lock_failed = 0, forced_whole = 0, lock_after_frameless_pool = 0;
};

// pool_frames: pool calls maintain the log-mel rings too (the mel heads); otherwise only the lock-step path does (a raw-PCM head)
static void run(const FeParams& fe, int W, int hop, bool pool_frames, unsigned seed, Totals& tot) {
    const int S = 5, T = fe_num_frames(fe, W), pad = fe.center ? fe.n_fft / 2 : 0;
    const HopPlan hp = nww_plan_hop(fe, T, W, hop, 1, true, false, false, [](int, int) { return true; });
    StreamPool p;
    p.open(S, W, hop);
    if (hp.shared && pool_frames) {
        int head, tail;
        pool_primed_spans(fe, W, T, hp.k, hp.el, hp.er, head, tail);
        p.keep_frames((T + hp.k - 1) / hp.k * hp.k, T, hp.k, hp.el, hp.er, head, tail);
    } else if (hp.shared) p.keep_ring((T + hp.k - 1) / hp.k * hp.k, hp.k);
    const bool ring_kept = p.lm_rows > 0;
#define AT "center=%d W=%d hop=%d frames=%d op=%d", fe.center, W, hop, (int)pool_frames, op
    std::vector<BruteStream> b((size_t)S);
    std::vector<std::vector<int64_t>> ring((size_t)S, std::vector<int64_t>((size_t)2 * W, -1));
    std::vector<std::vector<FrameId>> lm((size_t)S, std::vector<FrameId>((size_t)2 * (ring_kept ? p.lm_rows : 1)));
    std::mt19937 rng(seed);
    std::vector<int32_t> all;
    for (int s = 0; s < S; ++s) all.push_back(s);
    auto subset = [&](double prob) {
        std::vector<int32_t> idx;
        const unsigned mode = rng() % 10;
        for (int s = 0; s < S; ++s)
            if (mode == 0 || (mode == 1 ? s == (int)(rng() % S) : (rng() % 1000) < prob * 1000)) idx.push_back(s);
        return idx;
    };
    bool brute_aligned = true;
    auto brute_equal = [&] {
        for (int s = 1; s < S; ++s)
            if (!b[s].same(b[0])) return false;
        return true;
    };
    // the brute force's frames of the window that starts at sample a
    auto window_frames = [&](BruteStream& x, int64_t a) {
        x.frames.assign((size_t)T, FrameId());
        for (int t = 0; t < T; ++t) {
            const int64_t o = a + (int64_t)t * fe.hop - pad;
            x.frames[(size_t)t].origin = o;
            if (o < a || o + fe.n_fft > a + W) x.frames[(size_t)t].window = a;
        }
    };
    auto state_matches = [&](int op) {
        for (int s = 0; s < S; ++s) CHECK(p.of(s).filled == b[s].samples && p.of(s).pos == (int)(b[s].samples % W), AT);
    };
    const int fill = (W + hop - 1) / hop, wrap = ring_kept ? p.lm_rows / p.k : 0;
    const int n_ops = 40 + 6 * fill + 3 * wrap + 3 * (fill + wrap + 12);
    // an aligned phase draws lock-step pushes, pool pushes of every stream and whole resets only: long enough to fill a window, wrap
    // the log-mel ring and hand over between the two kinds of push many times
    int phase_left = 0;
    bool after_all_pool = false, after_frameless_pool = false, after_failed_lock = false;
    enum { RESET_ALL, RESET_SOME, PUSH_SOME, PUSH_ALL, LOCK };
    for (int op = 0; op < n_ops; ++op) {
        const unsigned r = rng() % 100;
        int kind;
        if (phase_left > 0) { --phase_left; kind = r < 3 ? RESET_ALL : r < 40 ? PUSH_ALL : LOCK; }
        else if (r < 3) kind = RESET_ALL;
        else if (r < 10) kind = RESET_SOME;
        else if (r < 14) kind = LOCK;
        else if (r < 17) { kind = RESET_ALL; phase_left = fill + wrap + 12; }
        else kind = PUSH_SOME;
        const bool was_all_pool = after_all_pool, was_frameless_pool = after_frameless_pool, was_failed_lock = after_failed_lock;
        after_all_pool = after_frameless_pool = after_failed_lock = false;
        if (kind == RESET_ALL) {                                 // the whole batch: aligned again
            pool_reset_all(p);
            for (auto& x : b) x = BruteStream();
            if (!brute_aligned) ++tot.realigned;
            brute_aligned = true;
            CHECK(pool_lock_ok(p), AT);
            state_matches(op);
            continue;
        }
        if (kind == RESET_SOME) {
            const std::vector<int32_t> idx = subset(0.3);
            CHECK(pool_idx_ok(idx.data(), (int)idx.size(), S), AT);
            pool_reset(p, idx.data(), (int)idx.size());
            for (int s : idx) b[s] = BruteStream();
            brute_aligned = brute_aligned && brute_equal();
            CHECK(p.aligned == brute_aligned, AT);
            for (int s : idx) CHECK(p.of(s).filled == 0 && p.of(s).pos == 0 && !p.of(s).primed, AT);
            state_matches(op);
            continue;
        }
        if (kind == LOCK) {                                      // a push of every stream, permitted while they are all equal
            CHECK(pool_lock_ok(p) == brute_aligned, AT);
            if (!pool_lock_ok(p)) { ++tot.lock_refused; continue; }
            const LockHop h = pool_lock_plan(p);
            ++tot.lock;
            CHECK(h.at >= 0 && h.at < W && h.at % 8 == 0 && h.pos == (h.at + hop) % W, AT);
            if (h.at + hop > W) ++tot.split_chunks;
            if (h.at + hop >= W) ++tot.pcm_wraps;
            const bool ok = rng() % 100 >= 6;                    // a hop whose launches fail leaves garbage where it would have written
            Ranges rg;
            if (h.primed) nww_hop_ranges(T, p.k, hp.el, hp.er, rg);
            else { rg.nr = 1; rg.t0[0] = 0; rg.t1[0] = T; }
            for (int s = 0; s < S; ++s) {
                BruteStream& x = b[s];
                for (int j = 0; j < hop; ++j) {
                    const int q = (h.at + j) % W;
                    ring[s][q] = ring[s][q + W] = x.samples + j;
                }
                x.samples += hop;
                CHECK(h.full == (x.samples >= W), AT);
                if (!h.full) { ++tot.not_full; continue; }
                const int64_t a = x.samples - W;
                bool window_ok = true;
                for (int i2 = 0; i2 < W && window_ok; ++i2) window_ok = ring[s][h.pos + i2] == a + i2;
                CHECK(window_ok, AT);
                window_frames(x, a);
                if (!ring_kept) { CHECK(!h.primed, AT); continue; }
                // primed exactly when the ring holds the previous window: after a lock-step hop or a pool call that maintains it
                CHECK(h.primed == x.valid, AT);
                CHECK(h.lm_row >= 0 && h.lm_row < p.lm_rows, AT);
                for (int q = 0; q < rg.nr; ++q)
                    for (int t = rg.t0[q]; t < rg.t1[q]; ++t) {
                        const int row = h.lm_row + t;
                        lm[s][(size_t)row] = lm[s][(size_t)(row < p.lm_rows ? row + p.lm_rows : row - p.lm_rows)] = ok ? x.frames[(size_t)t] : FrameId{-2, -2};
                    }
                bool rows_ok = true;
                for (int t = 0; t < T && rows_ok && ok; ++t) rows_ok = lm[s][(size_t)(h.lm_row + t)] == x.frames[(size_t)t];
                CHECK(rows_ok, AT);
                x.valid = ok;
                if (ok) ++x.rotated;
            }
            if (!ok) for (auto& x : b) x.valid = false;
            if (h.full && ring_kept) {
                if (h.primed) ++tot.lock_primed;
                if (h.primed && was_all_pool) ++tot.lock_primed_after_pool;
                if (!h.primed && was_frameless_pool) ++tot.lock_after_frameless_pool;
                if (!h.primed && was_failed_lock) ++tot.forced_whole;
                if (ok && h.lm_row + p.k >= p.lm_rows) ++tot.lm_wraps;
            }
            if (!ok) ++tot.lock_failed;
            after_failed_lock = !ok && h.full && ring_kept;
            pool_lock_commit(p, h, ok);
            CHECK(pool_lock_ok(p), AT);
            state_matches(op);
            continue;
        }
        const std::vector<int32_t> idx = kind == PUSH_ALL ? all : subset(0.7);
        const int n = (int)idx.size();
        PoolCall c;
        pool_plan_push(p, idx.data(), n, c);
        ++tot.pushes;
        CHECK((int)c.entries.size() == n && (int)c.win8.size() == c.m() && (int)c.out.size() == c.m(), AT);
        std::vector<int> slot_seen((size_t)c.m(), 0);
        std::vector<std::vector<FrameId>> scratch((size_t)c.m(), std::vector<FrameId>((size_t)T));
        int dense = 0;
        long frames_asked = 0, frames_want = 0;
        for (int i = 0; i < n; ++i) {
            const PoolEntry& e = c.entries[(size_t)i];
            const int s = idx[i];
            BruteStream& x = b[s];
            CHECK(e.stream == s && e.pos >= 0 && e.pos < W && e.pos % 8 == 0, AT);
            // (1) the chunk goes to pos - hop of the double-written ring
            const int p0 = ((e.pos - hop) % W + W) % W;
            if (p0 + hop > W) ++tot.split_chunks;
            if (p0 + hop >= W) ++tot.pcm_wraps;
            for (int j = 0; j < hop; ++j) {
                const int q = (p0 + j) % W;
                ring[s][q] = ring[s][q + W] = x.samples + j;
            }
            x.samples += hop;
            const bool full = x.samples >= W;
            CHECK((e.group == POOL_NOT_FULL) == !full, AT);
            const bool primed = p.frames && x.valid;
            if (!p.frames) x.valid = false;                      // a pool call that keeps no frames leaves the ring behind
            if (!full) { ++tot.not_full; CHECK(e.slot == -1 && e.dense == -1, AT); continue; }
            // (2) its window, read where the table says
            const int64_t a = x.samples - W;
            CHECK(e.slot >= 0 && e.slot < c.m() && e.dense == dense && c.out[(size_t)dense] == i, AT);
            ++dense;
            if (e.slot >= 0 && e.slot < c.m()) {
                CHECK(slot_seen[(size_t)e.slot]++ == 0, AT);
                CHECK((int64_t)c.win8[(size_t)e.slot] * 8 == (int64_t)s * 2 * W + e.pos, AT);
            }
            bool window_ok = true;
            for (int i2 = 0; i2 < W && window_ok; ++i2) window_ok = ring[s][e.pos + i2] == a + i2;
            CHECK(window_ok, AT);
            window_frames(x, a);
            CHECK(e.group == (primed ? POOL_PRIMED : POOL_WHOLE), AT);
            CHECK((e.group == POOL_WHOLE) == (e.slot < c.n_whole), AT);
            frames_asked += p.frames ? p.frames_of(e.group) : T;
            frames_want += primed ? hp.el + hp.k + hp.er : T;
            (primed ? tot.primed : tot.whole)++;
            if (!p.frames || e.slot < 0 || e.slot >= c.m()) continue;
            // (3) the frontend computes the group's frames of the staged window into the scratch; (4) they are placed in the ring
            // at lm_row + t, double-written; (5) the head's input is the T rows at lm_row
            CHECK(e.lm_row >= 0 && e.lm_row < p.lm_rows, AT);
            std::vector<int> ts;
            if (e.group == POOL_WHOLE) for (int t = 0; t < T; ++t) ts.push_back(t);
            else {
                for (int t = 0; t < p.el; ++t) ts.push_back(t);
                for (int t = T - p.er - p.k; t < T; ++t) ts.push_back(t);
            }
            // the PCM staging holds the whole window, or for a primed stream [0, head) and [tail, W) only: every sample a computed
            // frame reads (reflected at the window's ends) must be among them
            CHECK(p.head % 8 == 0 && p.tail % 8 == 0 && 0 <= p.head && p.head <= p.tail && p.tail <= W, AT);
            bool staged = true;
            for (int t : ts)
                for (int j = 0; j < fe.n_fft && staged && e.group == POOL_PRIMED; ++j) {
                    int q = t * fe.hop - pad + j;
                    if (q < 0) q = -q;
                    if (q >= W) q = 2 * (W - 1) - q;
                    staged = q < p.head || q >= p.tail;
                }
            CHECK(staged, AT);
            if (e.group == POOL_PRIMED) { tot.staged += p.head + W - p.tail; tot.windows += W; }
            for (int t : ts) scratch[(size_t)e.slot][(size_t)t] = x.frames[(size_t)t];
            for (int t : ts) {
                const int row = e.lm_row + t;
                lm[s][(size_t)row] = lm[s][(size_t)(row < p.lm_rows ? row + p.lm_rows : row - p.lm_rows)] = scratch[(size_t)e.slot][(size_t)t];
            }
            if (e.lm_row + p.k >= p.lm_rows) ++tot.lm_wraps;
            bool rows_ok = true;
            for (int t = 0; t < T && rows_ok; ++t) rows_ok = lm[s][(size_t)(e.lm_row + t)] == x.frames[(size_t)t];
            CHECK(rows_ok, AT);
            x.valid = true;
            ++x.rotated;
        }
        CHECK(dense == c.m() && frames_asked == frames_want, AT);
        pool_commit_push(p, c, true);
        brute_aligned = brute_aligned && brute_equal();
        CHECK(p.aligned == brute_aligned, AT);
        if (!p.aligned) ++tot.unaligned;
        after_all_pool = n == S && p.frames && c.m() == S;
        after_frameless_pool = n == S && !p.frames && ring_kept && c.m() == S;
        state_matches(op);
    }
#undef AT
}

int main() {
    Totals tot;
    unsigned seed = 1;
    for (int center = 0; center <= 1; ++center) {
        FeParams fe;
        fe.n_fft = 400; fe.hop = 160; fe.center = center;
        for (int W : {4800, 16000})
            for (int hop : {640, 1280, 296, W})
                for (int rep = 0; rep < 6; ++rep) run(fe, W, hop, rep != 5, seed++, tot);
    }
    // a failed call commits nothing but the loss of the kept frames
    {
        StreamPool p;
        p.open(3, 4800, 640);
        p.keep_frames(32, 31, 4, 2, 2, 360, 4120);
        const int32_t idx[2] = {0, 2};
        PoolCall c;
        for (int i = 0; i < 9; ++i) { pool_plan_push(p, idx, 2, c); pool_commit_push(p, c, true); }
        CHECK(p.of(0).primed && p.of(2).primed && !p.of(1).primed && !p.aligned, "primed after 9 hops");
        const int32_t pos = p.of(0).pos;
        pool_plan_push(p, idx, 2, c);
        CHECK(c.n_primed == 2 && c.n_whole == 0, "n_primed=%d", c.n_primed);
        pool_commit_push(p, c, false);
        CHECK(!p.of(0).primed && !p.of(2).primed && p.of(0).pos == pos && p.of(0).filled == 9 * 640, "failed call");
        const int32_t bad1[2] = {2, 0}, bad2[2] = {1, 1}, bad3[1] = {3}, bad4[1] = {-1};
        CHECK(pool_idx_ok(idx, 2, 3) && pool_idx_ok(nullptr, 0, 3), "idx");
        CHECK(!pool_idx_ok(bad1, 2, 3) && !pool_idx_ok(bad2, 2, 3) && !pool_idx_ok(bad3, 1, 3) && !pool_idx_ok(bad4, 1, 3) && !pool_idx_ok(nullptr, 1, 3) && !pool_idx_ok(idx, -1, 3), "bad idx");
    }
    // ... also on an aligned batch, which stays aligned when the call listed every stream and lost its frames as one
    {
        StreamPool p;
        p.open(2, 4800, 640);
        p.keep_frames(32, 31, 4, 2, 2, 360, 4120);
        const int32_t idx[2] = {0, 1};
        PoolCall c;
        for (int i = 0; i < 9; ++i) { pool_lock_commit(p, pool_lock_plan(p), true); }
        CHECK(pool_lock_plan(p).primed && p.all.filled == 9 * 640, "primed after 9 lock-step hops");
        pool_plan_push(p, idx, 2, c);
        CHECK(c.n_primed == 2, "n_primed=%d", c.n_primed);
        pool_commit_push(p, c, false);
        CHECK(pool_lock_ok(p) && !pool_lock_plan(p).primed && p.all.filled == 9 * 640, "failed call of every stream");
        pool_lock_commit(p, pool_lock_plan(p), true);
        pool_plan_push(p, idx, 1, c);
        pool_commit_push(p, c, false);                           // one stream of an aligned, primed batch loses its frames
        CHECK(!pool_lock_ok(p) && !p.of(0).primed && p.of(1).primed && p.of(0).filled == 10 * 640, "failed call of one stream");
        pool_reset_all(p);
        CHECK(pool_lock_ok(p) && p.of(1).filled == 0 && !p.of(1).primed, "whole reset");
    }
    CHECK(tot.staged * 2 < tot.windows, "a primed stream stages %ld of %ld samples", tot.staged, tot.windows);
    std::printf("pushes=%ld not_full=%ld whole=%ld primed=%ld pcm_wraps=%ld lm_wraps=%ld split_chunks=%ld unaligned=%ld realigned=%ld\n", tot.pushes,
                tot.not_full, tot.whole, tot.primed, tot.pcm_wraps, tot.lm_wraps, tot.split_chunks, tot.unaligned, tot.realigned);
    std::printf("lock=%ld lock_primed=%ld lock_primed_after_pool=%ld lock_refused=%ld lock_failed=%ld forced_whole=%ld lock_after_frameless_pool=%ld\n", tot.lock,
                tot.lock_primed, tot.lock_primed_after_pool, tot.lock_refused, tot.lock_failed, tot.forced_whole, tot.lock_after_frameless_pool);
    CHECK(tot.not_full > 0 && tot.whole > 0 && tot.primed > 0 && tot.pcm_wraps > 0 && tot.lm_wraps > 0 && tot.split_chunks > 0 && tot.unaligned > 0 &&
              tot.realigned > 0 && tot.lock > 0 && tot.lock_primed > 0 && tot.lock_primed_after_pool > 0 && tot.lock_refused > 0 && tot.forced_whole > 0 &&
              tot.lock_after_frameless_pool > 0, "a path of the schedule never ran");
    if (g_fail) std::printf("FAILED %d checks\n", g_fail);
    else std::printf("ok\n");
    return g_fail ? 1 : 0;
}
