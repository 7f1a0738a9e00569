// stream_pool.h - a stream batch whose streams push, join and reset on their own (nww_stream_push_some / nww_stream_reset_some): the
// per-stream ring state and what one call asks of the device, as host-only integer arithmetic (no HIP header; g++ compiles it for
// tests/test_stream_pool_host.py).  Every push is commanded by the host, so the state lives here and nothing is read back: a call
// turns its ascending stream list into one small table (PoolCall) that the data-movement kernels of nww_stream.hip follow.
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

struct StreamPool {
    int S = 0, W = 0, hop = 0;
    bool frames = false;                 // log-mel rings are kept (route 1); lm_rows rows per ring, a hop shifts a window by k of T frames
    int lm_rows = 0, k = 0, T = 0, el = 0, er = 0;
    int head = 0, tail = 0;              // a primed stream's hop reads samples [0, head) and [tail, W) of its window only (pool_primed_spans)
    // every stream has the same state: the lock-step entry points may run.  Cleared by the first call that makes the states differ,
    // set again only by a reset of the whole batch.
    bool aligned = true;
    std::vector<int32_t> pos, lm_pos;
    std::vector<int64_t> filled;
    std::vector<uint8_t> primed;

    void open(int S_, int W_, int hop_) {
        S = S_; W = W_; hop = hop_;
        frames = false; lm_rows = k = T = el = er = head = tail = 0;
        aligned = true;
        set_all(0, 0, 0, false);
    }
    void keep_frames(int lm_rows_, int T_, int k_, int el_, int er_, int head_, int tail_) {
        frames = true; lm_rows = lm_rows_; T = T_; k = k_; el = el_; er = er_; head = head_; tail = tail_;
    }
    // every stream takes the lock-step batch's state
    void set_all(int pos_, long long filled_, int lm_pos_, bool primed_) {
        pos.assign((size_t)S, pos_); lm_pos.assign((size_t)S, lm_pos_); filled.assign((size_t)S, filled_); primed.assign((size_t)S, primed_ ? 1 : 0);
    }
    bool all_equal() const {
        for (int s = 1; s < S; ++s)
            if (pos[s] != pos[0] || lm_pos[s] != lm_pos[0] || filled[s] != filled[0] || primed[s] != primed[0]) return false;
        return true;
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
        const int s = idx[i];
        PoolEntry& e = c.entries[(size_t)i];
        e.stream = s;
        e.pos = (p.pos[s] + p.hop) % p.W;
        e.lm_row = p.lm_pos[s];
        e.group = p.filled[s] + p.hop < p.W ? POOL_NOT_FULL : (p.frames && p.primed[s]) ? POOL_PRIMED : POOL_WHOLE;
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
    for (const PoolEntry& e : c.entries) {
        const int s = e.stream;
        if (!ok) { p.primed[s] = 0; continue; }
        p.pos[s] = e.pos;
        p.filled[s] += p.hop;
        if (e.group != POOL_NOT_FULL && p.frames) {
            p.lm_pos[s] = (p.lm_pos[s] + p.k) % p.lm_rows;
            p.primed[s] = 1;
        }
    }
    if (p.aligned && !p.all_equal()) p.aligned = false;
}

// a new session for the listed streams
inline void pool_reset(StreamPool& p, const int32_t* idx, int n) {
    for (int i = 0; i < n; ++i) {
        const int s = idx[i];
        p.pos[s] = 0; p.lm_pos[s] = 0; p.filled[s] = 0; p.primed[s] = 0;
    }
    if (p.aligned && !p.all_equal()) p.aligned = false;
}
