// stream_pool.h - the ring state of a stream batch, and what one call asks of the device, as host-only integer arithmetic (no HIP header;
// g++ compiles it for tests/test_stream_pool_host.py).  Every push is commanded by the host, so the state lives here and nothing is read
// back.  There is ONE state, whichever entry point moves it: per stream the write position of its PCM ring, its fill count, the rotation
// of its log-mel ring and whether that ring holds the window before the next hop (primed).
//   lock-step calls (nww_stream_push*)   every stream pushes: pool_lock_plan / pool_lock_commit, O(1) on the common state
//   pool calls (nww_stream_push_some*, nww_stream_reset_some)   the listed streams push or reset on their own: a call turns its ascending
//                                        stream list into one small table (PoolCall) that the data-movement kernels of nww_stream.hip follow
//   nww_stream_reset                     pool_reset_all
// Alignment: while `aligned`, every stream has the state `all` and the lock-step calls may run.  A pool call gives each stream its own
// copy (`each`, O(S), made by the first such call) and works there; if it leaves them all equal - it listed every stream, or reset
// streams that were empty anyway - the batch stays aligned.  The first call that makes states differ ends alignment, and only
// pool_reset_all restores it.
// Primed: a pool that keeps frames maintains the log-mel rings, so lock-step and all-stream pool hops follow one another incrementally.
// A pool call that keeps none (raw-PCM head, route 0) clears the flag of the streams it lists: the next lock-step hop computes its window
// whole.  (The lock-step path's conv-row and sequence rings are its own, with a flag of their own: StreamState::rows_held.)
// A failed lock-step hop has stored its chunk: position and fill advance, primed is lost.  A failed pool call commits nothing but the
// loss of primed.
#pragma once
#include <cstdint>
#include <vector>
#include "fe_tables.h"

// what a call does with a listed stream
enum { POOL_NOT_FULL = 0,    // its ring holds no window yet: the chunk is stored, the score is 0
       POOL_WHOLE = 1,       // its window is computed whole (its first full window, or every window where no frames are kept)
       POOL_PRIMED = 2 };    // its log-mel ring holds the previous window: only the frames this hop invalidates are computed

// One listed stream; entry i belongs to row i of the chunk and to output i.  pos: where its window starts in its double-written PCM
// ring AFTER this push (the chunk itself goes to pos - hop, modulo W); lm_row: the row of its log-mel ring that frame 0 of that window
// takes; slot: its row in the PCM staging and the frontend's scratch (whole windows first, then the primed ones, each in list order);
// dense: its row in the head's input and output (list order).  slot and dense are -1 for POOL_NOT_FULL.
struct PoolEntry { int32_t stream, pos, lm_row, group, slot, dense; };

#ifdef __HIPCC__
#define POOL_HD __host__ __device__
#else
#define POOL_HD
#endif
// where an entry's window starts in the PCM rings [S][2 W], in units of 8 samples (16 bytes), from the entry alone: what win8 holds in
// slot order, and what a reader that walks the entries in list order (the cascade's pool select, cascade.hip) computes for itself
POOL_HD inline int32_t pool_entry_win8(const PoolEntry& e, int W) { return (int32_t)(((int64_t)e.stream * 2 * W + e.pos) / 8); }

struct PoolCall {
    std::vector<PoolEntry> entries;      // [n]
    std::vector<int32_t> win8;           // [m], slot order: the window's offset in the PCM rings, in units of 8 samples (16 bytes)
    std::vector<int32_t> out;            // [m], dense order: the entry (= output index) of each scored stream
    int n_whole = 0, n_primed = 0;
    int m() const { return n_whole + n_primed; }
};

// one stream's rings
struct RingState {
    int32_t pos = 0, lm_pos = 0;
    int64_t filled = 0;                  // samples since its last reset
    bool primed = false;
    bool operator==(const RingState& o) const { return pos == o.pos && lm_pos == o.lm_pos && filled == o.filled && primed == o.primed; }
};

struct StreamPool {
    int S = 0, W = 0, hop = 0;
    int lm_rows = 0, k = 0;              // a log-mel ring of lm_rows rows is kept (keep_ring); a hop shifts a window by k frames
    bool frames = false;                 // ... and pool calls maintain it too (route 1); a window has T frames, el / er of them edge frames
    int T = 0, el = 0, er = 0;
    int head = 0, tail = 0;              // a primed stream's hop reads samples [0, head) and [tail, W) of its window only (pool_primed_spans)
    bool aligned = true;
    RingState all;                       // every stream's state while aligned; afterwards what it was when alignment ended
    std::vector<RingState> each;         // [S] while not aligned

    void open(int S_, int W_, int hop_) { *this = StreamPool(); S = S_; W = W_; hop = hop_; }
    void keep_ring(int lm_rows_, int k_) { lm_rows = lm_rows_; k = k_; }
    void keep_frames(int lm_rows_, int T_, int k_, int el_, int er_, int head_, int tail_) {
        keep_ring(lm_rows_, k_);
        frames = true; T = T_; el = el_; er = er_; head = head_; tail = tail_;
    }
    const RingState& of(int s) const { return aligned ? all : each[(size_t)s]; }
    // a pool call's writes: f works on the streams' own states; an aligned batch stays aligned if f leaves them all equal
    template <class F>
    void edit(F f) {
        if (aligned) each.assign((size_t)S, all);
        f(each);
        for (int s = 1; s < S && aligned; ++s) aligned = each[(size_t)s] == each[0];
        if (aligned && S > 0) all = each[0];
    }
    // log-mel frames the frontend computes for one stream of a group
    int frames_of(int group) const { return group == POOL_NOT_FULL ? 0 : group == POOL_PRIMED ? el + k + er : T; }
};

// The samples of a W-sample window that the frames a hop invalidates - [0, el) and [T - er - k, T) - read, reflect padding included:
// [0, head) and [tail, W), both multiples of 8 samples (head == tail: the whole window).  Only these go into a primed stream's PCM staging.
inline void pool_primed_spans(const FeParams& fe, int W, int T, int k, int el, int er, int& head, int& tail) {
    const int pad = fe.center ? fe.n_fft / 2 : 0;
    // frame t reads samples [t hop - pad, t hop - pad + n_fft); a sample s < 0 is read at -s (up to pad), one >= W at 2 (W - 1) - s (down to W - 1 - pad)
    head = el > 0 ? (el - 1) * fe.hop - pad + fe.n_fft : 0;
    if (el > 0 && head < pad + 1) head = pad + 1;
    head = (head + 7) & ~7;
    if (head > W) head = W;
    tail = (T - er - k) * fe.hop - pad;
    if (er > 0 && tail > W - 1 - pad) tail = W - 1 - pad;
    if (tail < 0) tail = 0;
    tail &= ~7;
    if (tail < head) tail = head;
}

// n strictly ascending stream numbers in [0, S)
inline bool pool_idx_ok(const int32_t* idx, int n, int S) {
    if (n < 0 || (n > 0 && !idx)) return false;
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= S || (i > 0 && idx[i] <= idx[i - 1])) return false;
    return true;
}

// What a push of one hop for the listed streams does; nothing is committed (pool_commit_push), so a call that fails on the way leaves
// the state as it was.
inline void pool_plan_push(const StreamPool& p, const int32_t* idx, int n, PoolCall& c) {
    c.entries.assign((size_t)n, PoolEntry{});
    c.n_whole = c.n_primed = 0;
    for (int i = 0; i < n; ++i) {
        const RingState& r = p.of(idx[i]);
        PoolEntry& e = c.entries[(size_t)i];
        e.stream = idx[i];
        e.pos = (r.pos + p.hop) % p.W;
        e.lm_row = r.lm_pos;
        e.group = r.filled + p.hop < p.W ? POOL_NOT_FULL : (p.frames && r.primed) ? POOL_PRIMED : POOL_WHOLE;
        e.slot = e.dense = -1;
        if (e.group == POOL_WHOLE) ++c.n_whole;
        if (e.group == POOL_PRIMED) ++c.n_primed;
    }
    c.win8.assign((size_t)c.m(), 0);
    c.out.assign((size_t)c.m(), 0);
    int whole = 0, primed = 0, dense = 0;
    for (int i = 0; i < n; ++i) {
        PoolEntry& e = c.entries[(size_t)i];
        if (e.group == POOL_NOT_FULL) continue;
        e.slot = e.group == POOL_WHOLE ? whole++ : c.n_whole + primed++;
        e.dense = dense++;
        c.win8[(size_t)e.slot] = pool_entry_win8(e, p.W);
        c.out[(size_t)e.dense] = i;
    }
}

// ok: every launch of the call went out; otherwise the listed streams' log-mel rings may hold a half-written hop and their next window
// is computed whole
inline void pool_commit_push(StreamPool& p, const PoolCall& c, bool ok) {
    p.edit([&](std::vector<RingState>& each) {
        for (const PoolEntry& e : c.entries) {
            RingState& r = each[(size_t)e.stream];
            if (!ok || !p.frames) r.primed = false;
            if (!ok) continue;
            r.pos = e.pos;
            r.filled += p.hop;
            if (e.group != POOL_NOT_FULL && p.frames) { r.lm_pos = (r.lm_pos + p.k) % p.lm_rows; r.primed = true; }
        }
    });
}

// a new session for the listed streams
inline void pool_reset(StreamPool& p, const int32_t* idx, int n) {
    p.edit([&](std::vector<RingState>& each) {
        for (int i = 0; i < n; ++i) each[(size_t)idx[i]] = RingState();
    });
}

// ... and for the whole batch, which is aligned again
inline void pool_reset_all(StreamPool& p) { p.all = RingState(); p.aligned = true; }

// ---- the lock-step calls: every stream pushes one hop; they run only while the batch is aligned
inline bool pool_lock_ok(const StreamPool& p) { return p.aligned; }

// What a lock-step push reads.  at: where the chunk goes in every PCM ring; pos: where the window starts after the push (the last W
// samples are contiguous there in the double-written ring); full: the rings hold a window; lm_row: the row of the log-mel rings that
// frame 0 of that window takes; primed: those rings hold the previous window.
struct LockHop { int32_t at, pos, lm_row; bool full, primed; };
inline LockHop pool_lock_plan(const StreamPool& p) {
    const RingState& r = p.all;
    return {r.pos, (r.pos + p.hop) % p.W, r.lm_pos, r.filled + p.hop >= p.W, r.primed};
}

// The chunk is in the rings, so position and fill advance either way.  ok: the hop's launches went out - where a log-mel ring is kept and
// the window was full, the ring has been rotated to it; otherwise the rings may hold a half-finished hop.
inline void pool_lock_commit(StreamPool& p, const LockHop& hp, bool ok) {
    RingState& r = p.all;
    r.pos = hp.pos;
    r.filled += p.hop;
    if (!ok) r.primed = false;
    else if (hp.full && p.lm_rows > 0) { r.lm_pos = (r.lm_pos + p.k) % p.lm_rows; r.primed = true; }
}
