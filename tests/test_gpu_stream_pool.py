"""Streams that push, join and reset on their own (nww_stream_push_some / nww_stream_reset_some) on the GPU (run with -m gpu).  The
oracle is the library itself: the test keeps each stream's last W samples on the host and, after every tick, runs forward_pcm on the full
windows stacked in idx order; equality is np.array_equal on logits and probabilities, and a stream that holds no window yet must read
exactly 0.  Shapes are small on purpose: W = 4800 (T = 31 at centre 1, edge frames el = er = 2), S = 6, 24 ticks.  With hop 640
the window is no multiple of the hop, so chunks are split across the PCM ring's end; the log-mel ring has 32 rows there and a hop
shifts it by k = 4."""
import ctypes as C

import numpy as np
import pytest

from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_pcm, synth_state_dict

pytestmark = pytest.mark.gpu

S, W, T, EL, ER, TICKS = 6, 4800, 31, 2, 2, 24


def _model(cfg, g=None):
    from nanowakeword_amd.session import HipModel
    kw = dict(window=g["window"], mel_fb=g["fb64"]) if g is not None else {}
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg), **kw)


def _audio(n_streams, n, seed):
    kinds = ("speechlike", "noise", "loud", "speechlike", "chirp", "noise")
    x = np.concatenate([synth_pcm(kinds[s % len(kinds)], 1, n, seed=seed + 3 * s) for s in range(n_streams)], 0)
    x[3, n // 3:n // 3 + 1500] = 0                         # a stretch of digital silence: -100 dB floor rows travel through the rings
    return x


def _schedule(seed, n_streams=S, ticks=TICKS):
    """[(streams reset before the tick, streams that push)]: a tick with all streams, one with a single stream, ticks where no listed
    stream is full yet (the first ones), stream 5 joining at tick 5, stream 2 reset at tick 12; otherwise each stream pushes with
    probability 0.9, so that the streams' ring positions drift apart"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(ticks):
        ids = [s for s in range(n_streams) if rng.random() < 0.9]
        if t in (0, 8, 15, ticks - 1):
            ids = list(range(n_streams))
        if t == 2:
            ids = [1]
        if t < 5:
            ids = [s for s in ids if s != 5]
        out.append(([2] if t == 12 else [], ids))
    return out


class Host:
    """what the test knows of every stream: its samples since its last reset, and whether it has been scored since"""

    def __init__(self, audio, window, hop):
        self.audio, self.W, self.hop = audio, window, hop
        n = len(audio)
        self.cursor = np.zeros(n, int)                       # next sample of the stream's audio
        self.hist = [np.zeros(0, np.int16) for _ in range(n)]
        self.scored = np.zeros(n, int)

    def reset(self, ids):
        for s in ids:
            self.hist[s] = np.zeros(0, np.int16)
            self.scored[s] = 0

    def chunk(self, ids):
        rows = []
        for s in ids:
            c = self.audio[s, self.cursor[s]:self.cursor[s] + self.hop]
            assert len(c) == self.hop
            self.cursor[s] += self.hop
            self.hist[s] = np.concatenate([self.hist[s], c])
            rows.append(c)
        return np.ascontiguousarray(np.stack(rows)) if rows else np.zeros((0, self.hop), np.int16)

    def full(self, ids):
        return [i for i, s in enumerate(ids) if len(self.hist[s]) >= self.W]

    def windows(self, ids, full):
        return np.ascontiguousarray(np.stack([self.hist[ids[i]][-self.W:] for i in full]))


def _walk(m, window, hop, rows, route, per_hop, schedule, seed=0, what=""):
    """the schedule against the oracle; rows: frames (rows) of a whole window, per_hop: frames of a primed stream's hop.  Returns which kinds
    of tick occurred (how often) and whether the rings wrapped."""
    n_streams = 1 + max(s for _, ids in schedule for s in ids)
    host = Host(_audio(n_streams, hop * (len(schedule) + 1), 50 + seed), window, hop)
    m.stream_open(n_streams, window, hop)
    seen = dict(primed_only=0, first_window=0, nothing=0, single=0, everybody=0, pcm_wrap=0, lm_wrap=0)
    for t, (resets, ids) in enumerate(schedule):
        if resets:
            m.stream_reset_some(resets)
            host.reset(resets)
            assert all(m.stream_filled(s) == 0 for s in resets)
        chunk = host.chunk(ids)
        lg, pr = m.stream_push_some(ids, chunk)
        assert lg.dtype == pr.dtype == np.float32 and lg.shape == pr.shape == (len(ids),)
        full = host.full(ids)
        want_l, want_p = np.zeros(len(ids), np.float32), np.zeros(len(ids), np.float32)
        if full:
            want_l[full], want_p[full] = m.forward_pcm(host.windows(ids, full))
        assert np.array_equal(lg, want_l), (what, t, ids, lg, want_l)
        assert np.array_equal(pr, want_p), (what, t, ids, pr, want_p)
        assert all(m.stream_filled(s) == len(host.hist[s]) for s in range(n_streams)), (what, t)
        frames = sum(per_hop if (route == 1 and host.scored[ids[i]]) else rows for i in full)
        n_primed = sum(1 for i in full if host.scored[ids[i]])
        assert m.stream_pool_stats() == (len(full), route, frames), (what, t, m.stream_pool_stats(), (len(full), route, frames))
        seen["primed_only"] += bool(full) and n_primed == len(full)
        seen["first_window"] += n_primed < len(full)
        seen["nothing"] += bool(ids) and not full
        seen["single"] += len(ids) == 1
        seen["everybody"] += len(ids) == n_streams
        for i in full:
            host.scored[ids[i]] += 1
    # every stream's PCM ring has wrapped since its last reset, and the log-mel ring (32 rows) of every stream that was there from the
    # first tick and never reset
    seen["pcm_wrap"] = min(len(h) for h in host.hist) > window
    seen["lm_wrap"] = route == 0 or min(host.scored[s] for s in (0, 1, 3, 4)) * (hop // 160) > 32
    m.stream_close()
    print(what, seen)
    return seen


# ---- route 1: shared frames
@pytest.mark.parametrize("head", ["cnn", "crnn"])
@pytest.mark.parametrize("hop", [640, 1280])
def test_shared_frames(golden_frontend, head, hop):
    cfg = HeadConfig(head, (T, 64))
    m = _model(cfg, golden_frontend)
    k = hop // 160
    seen = _walk(m, W, hop, T, 1, EL + k + ER, _schedule(hop), seed=hop, what=(head, hop))
    # every kind of tick the schedule is there for has occurred, and both rings have wrapped for every stream
    assert all(seen.values()), seen
    m.close()


# ---- route 0: whole windows
def test_whole_windows_hop_off_the_frame_grid(golden_frontend):
    m = _model(HeadConfig("cnn", (T, 64)), golden_frontend)
    seen = _walk(m, W, 296, T, 0, T, _schedule(296, ticks=2 * TICKS), seed=296, what=("cnn", 296))       # 16.2 hops fill a window
    assert all(seen.values()), seen
    m.close()


def test_whole_windows_raw_pcm_head():
    """e2e_cnn at its smallest golden shape: 1040 samples -> (17, 64).  Hop 320 is a whole number of its frontend's rows, so lock-step
    streaming would keep a ring of them; a pool re-scores whole windows."""
    m = _model(HeadConfig("e2e_cnn", (17, 64), e2e_frontend_channels=32))
    seen = _walk(m, 1040, 320, 17, 0, 17, _schedule(320), seed=320, what=("e2e_cnn", 320))
    assert all(seen.values()), seen
    m.close()


def test_stream_inc_0_takes_route_0():
    """(the knob is read once per process, so this runs in a fresh one)"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import numpy as np\n"
            "from nanowakeword_amd.config import FrontendConfig, HeadConfig\n"
            "from nanowakeword_amd.session import HipModel\n"
            "from nanowakeword_amd.synth import synth_pcm, synth_state_dict\n"
            "cfg = HeadConfig('cnn', (31, 64))\n"
            "m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))\n"
            "x = synth_pcm('speechlike', 3, 640 * 12, seed=3)\n"
            "m.stream_open(3, 4800, 640)\n"
            "for t in range(12):\n"
            "    ids = [0, 2] if t % 3 else [0, 1, 2]\n"
            "    lg, pr = m.stream_push_some(ids, np.ascontiguousarray(x[ids, t * 640:(t + 1) * 640]))\n"
            "assert m.stream_pool_stats() == (2, 0, 62), m.stream_pool_stats()\n"
            "want = m.forward_pcm(np.ascontiguousarray(x[[0, 2], 12 * 640 - 4800:]))\n"
            "assert np.array_equal(lg, want[0]) and np.array_equal(pr, want[1])\n"
            "print('route0 ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, NWW_STREAM_INC="0"))
    assert r.returncode == 0 and "route0 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- isolation
def test_reset_of_one_stream_leaves_the_others_alone(golden_frontend):
    """Stream 2 is filled with loud noise and then reset alone.  Every other stream scores, tick for tick, what it scores in a run in
    which stream 2 was never touched; stream 2 reads 0 until its own W samples have arrived and then what forward_pcm gives on its new
    audio alone."""
    hop, before, after = 640, 10, 12
    m = _model(HeadConfig("cnn", (T, 64)), golden_frontend)
    audio = _audio(S, hop * (before + after), 900)
    loud = synth_pcm("loud", 1, hop * before, seed=5)[0]
    fresh = synth_pcm("speechlike", 1, hop * after, seed=6)[0]
    others = [0, 1, 3, 4, 5]

    def run(touch):
        m.stream_open(S, W, hop)
        out = []
        for t in range(before + after):
            ids = sorted(others + [2]) if touch else others
            if touch and t == before:
                m.stream_reset_some([2])
                assert m.stream_filled(2) == 0 and m.stream_filled(1) == hop * before
            rows = audio[:, t * hop:(t + 1) * hop].copy()
            rows[2] = loud[t * hop:(t + 1) * hop] if t < before else fresh[(t - before) * hop:(t - before + 1) * hop]
            lg, pr = m.stream_push_some(ids, np.ascontiguousarray(rows[ids]))
            out.append((dict(zip(ids, lg)), dict(zip(ids, pr))))
        m.stream_close()
        return out

    touched, alone = run(True), run(False)
    for t in range(before + after):
        for s in others:
            assert touched[t][0][s] == alone[t][0][s] and touched[t][1][s] == alone[t][1][s], (t, s)
    assert any(alone[t][0][0] != 0 for t in range(before, before + after))
    assert touched[before - 1][0][2] != 0                                            # it did score its noise before the reset
    for j in range(after):
        lg, pr = touched[before + j][0][2], touched[before + j][1][2]
        n = (j + 1) * hop
        if n < W:
            assert lg == 0 and pr == 0, (j, lg, pr)                                   # nothing of the previous client's window
        else:
            want_l, want_p = m.forward_pcm(np.ascontiguousarray(fresh[None, n - W:n]))
            assert lg == want_l[0] and pr == want_p[0], (j, lg, want_l)
    m.close()


# ---- the lock-step entry points
def test_lock_step_unchanged(golden_frontend):
    """On a fresh batch nww_stream_push equals push_some with every stream listed, and the two interleave while every call lists every
    stream (CRNN: the lock-step path keeps conv-row and sequence rings that a pool call does not maintain).  After a diverging
    push_some the lock-step push is refused until nww_stream_reset; after it, it equals a fresh batch."""
    from nanowakeword_amd.session import NwwError
    hop, ticks = 640, 14
    cfg = HeadConfig("crnn", (T, 64))
    m = _model(cfg, golden_frontend)
    audio = _audio(S, hop * ticks, 77)
    every = list(range(S))
    chunks = [np.ascontiguousarray(audio[:, t * hop:(t + 1) * hop]) for t in range(ticks)]

    def run(kinds):
        out = []
        for t, kind in enumerate(kinds):
            out.append(m.stream_push(chunks[t]) if kind == "lock" else m.stream_push_some(every, chunks[t]))
        return np.stack([np.stack(o) for o in out])

    m.stream_open(S, W, hop)
    lock = run(["lock"] * ticks)
    assert lock[-1].all() and not lock[:7].any() and m.stream_filled() == hop * ticks
    m.stream_reset()
    some = run(["some"] * ticks)
    assert np.array_equal(some, lock)
    assert m.stream_filled() == hop * ticks == m.stream_filled(3)                    # still aligned: the lock-step count follows
    m.stream_reset()
    mixed = run((["lock", "some", "some", "lock", "lock"] * 3)[:ticks])
    assert np.array_equal(mixed, lock)
    # a push that leaves a stream out ends the lock-step
    m.stream_push_some([0, 1, 2, 4, 5], np.ascontiguousarray(chunks[0][[0, 1, 2, 4, 5]]))
    with pytest.raises(NwwError, match="no longer share one state"):
        m.stream_push(chunks[0])
    assert m.stream_filled(3) == hop * ticks and m.stream_filled(0) == hop * (ticks + 1)
    m.stream_reset()
    assert all(m.stream_filled(s) == 0 for s in every)
    again = run(["lock"] * ticks)
    assert np.array_equal(again, lock)
    # ... and so does the reset of one stream alone
    m.stream_reset_some([4])
    with pytest.raises(NwwError, match="no longer share one state"):
        m.stream_push(chunks[0])
    m.stream_close()
    m.stream_open(S, W, hop)                                                         # a fresh batch
    assert np.array_equal(run(["lock"] * ticks), lock)
    m.stream_close(); m.close()


@pytest.mark.parametrize("head,shape,kw,n_streams,window,hop,ticks", [
    ("cnn", (T, 64), {}, S, W, 640, 14),                                             # frames kept by both paths, no conv-row rings
    ("e2e_cnn", (17, 64), dict(e2e_frontend_channels=32), 3, 1040, 320, 12),         # the lock-step plan shares rows, the pool keeps none
])
def test_lock_step_and_pool_interleave(golden_frontend, head, shape, kw, n_streams, window, hop, ticks):
    """While every call lists every stream the two kinds of push describe one state: all lock-step, all push_some and a mix of the two
    score the same bits, and the batch's fill count is every stream's after every call."""
    m = _model(HeadConfig(head, shape, **kw), golden_frontend if head == "cnn" else None)
    kinds = ("speechlike", "noise", "loud", "chirp")
    audio = np.concatenate([synth_pcm(kinds[s % 4], 1, hop * ticks, seed=31 + 3 * s) for s in range(n_streams)], 0)
    every = list(range(n_streams))
    chunks = [np.ascontiguousarray(audio[:, t * hop:(t + 1) * hop]) for t in range(ticks)]

    def run(schedule):
        m.stream_open(n_streams, window, hop)
        out = []
        for t, kind in enumerate(schedule):
            out.append(np.stack(m.stream_push(chunks[t]) if kind == "lock" else m.stream_push_some(every, chunks[t])))
            assert all(m.stream_filled() == m.stream_filled(s) == hop * (t + 1) for s in every), (kind, t)
        m.stream_close()
        return np.stack(out)

    lock = run(["lock"] * ticks)
    assert lock[-1].all() and not lock[0].any()
    assert np.array_equal(run(["some"] * ticks), lock)
    assert np.array_equal(run((["lock", "some", "some", "lock", "lock"] * 3)[:ticks]), lock)
    m.close()


# ---- errors
def test_errors(golden_frontend):
    m = _model(HeadConfig("cnn", (T, 64)), golden_frontend)
    lib, hop = m.lib, 640
    chunk = synth_pcm("noise", 3, hop, seed=1)
    lg, pr = np.full(3, 7.0, np.float32), np.full(3, 7.0, np.float32)

    def push(ids, chunk_ptr=chunk.ctypes.data_as(C.c_void_p)):
        ids = np.asarray(ids, np.int32)
        return lib.nww_stream_push_some(m._h, ids.ctypes.data_as(C.c_void_p), len(ids), chunk_ptr, lg.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p))

    assert push([0, 1, 2]) == 5 and b"no open stream batch" in lib.nww_last_error(m._h)          # NWW_ERR_STATE
    one = np.zeros(1, np.int32)
    assert lib.nww_stream_reset_some(m._h, one.ctypes.data_as(C.c_void_p), 1) == 5
    assert lib.nww_stream_filled_of(m._h, 0) == 0
    m.stream_open(S, W, hop)
    for t in range(8):                                               # every stream holds a window: a call that went through would score
        m.stream_push_some(list(range(S)), np.ascontiguousarray(synth_pcm("noise", S, hop, seed=t)))
    filled = [m.stream_filled(s) for s in range(S)]
    for bad in ([2, 1, 0], [0, 2, 1], [1, 1, 3], [0, 1, S], [-1, 0, 1]):
        assert push(bad) == 1, bad                                   # NWW_ERR_INVALID
        assert b"strictly ascending" in lib.nww_last_error(m._h)
    assert push([0, 1, 2], None) == 1 and b"null chunk" in lib.nww_last_error(m._h)
    assert (lg == 7.0).all() and (pr == 7.0).all()                   # outputs untouched
    assert [m.stream_filled(s) for s in range(S)] == filled          # ... and nothing was pushed
    bad = np.asarray([3, 3], np.int32)
    assert lib.nww_stream_reset_some(m._h, bad.ctypes.data_as(C.c_void_p), 2) == 1
    assert m.stream_filled(3) == filled[3]
    with pytest.raises(ValueError, match="strictly ascending"):
        m.stream_push_some([1, 0], chunk[:2])
    with pytest.raises(ValueError, match="chunk must have shape"):
        m.stream_push_some([0, 1], chunk)
    # n == 0: NWW_OK, nothing is launched or written
    assert lib.nww_stream_push_some(m._h, None, 0, None, lg.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p)) == 0
    assert (lg == 7.0).all() and m.stream_pool_stats()[0] == 0
    e0, e1 = m.stream_push_some([], np.zeros((0, hop), np.int16))
    assert e0.shape == e1.shape == (0,)
    assert push([0, 1, 2]) == 0 and (lg != 7.0).all() and (pr != 7.0).all() and m.stream_pool_stats()[0] == 3
    m.stream_close(); m.close()
