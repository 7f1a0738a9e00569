"""interpreter.StreamPool on the CPU: every slot behaves exactly like a StreamBatch of ONE stream fed that slot's chunks.  The backend is
scripted - a session's score is a function of the session and of how many chunks it has been pushed, so the two sides agree without any
audio arithmetic - and the schedule is seeded: 6 slots, 60 ticks, each slot pushing or idle per tick, with an attach into a free slot, a
detach and re-attach (the slot's next client must inherit nothing) and a reset.  Scores are compared with ==, with patience, with
debounce and with neither; the ValueErrors of StreamBatch.push are raised in the same cases."""
import numpy as np
import pytest

from nanowakeword_amd.interpreter import StreamBatch, StreamPool

S, W, HOP, TICKS = 6, 4800, 640, 60


def _score(key: int, pushes: int, filled: int) -> np.float32:
    """what a session reports after its `pushes`-th chunk: 0 until its window is full, then a value that crosses 0.5 in runs"""
    if filled < W:
        return np.float32(0.0)
    x = np.sin(0.37 * pushes + 1.3 * key) * 0.5 + 0.5
    return np.float32(0.0 if (pushes + key) % 11 == 0 else x)          # exact zeros too: the filters skip them


class ScriptedPoolBackend:
    """stream_* of HipModel, scripted: `key[s]` names the session in slot s"""

    def stream_open(self, n, window, hop):
        self.S, self.W, self.hop = n, window, hop
        self.key = list(range(n))
        self.pushes, self.filled = np.zeros(n, int), np.zeros(n, int)

    def stream_reset(self):
        self.pushes[:] = 0; self.filled[:] = 0

    def stream_reset_some(self, ids):
        self.pushes[ids] = 0; self.filled[ids] = 0

    def stream_push_some(self, ids, chunk):
        assert chunk.shape == (len(ids), self.hop) and chunk.dtype == np.int16
        assert (np.diff(ids) > 0).all()
        self.pushes[ids] += 1; self.filled[ids] += self.hop
        p = np.array([_score(self.key[s], self.pushes[s], self.filled[s]) for s in ids], np.float32)
        return p.copy(), p

    def stream_push(self, chunk):                     # one lock-step stream: StreamBatch(S = 1)
        return self.stream_push_some(np.arange(self.S), chunk)

    def stream_close(self):
        pass


def _single(key):
    b = ScriptedPoolBackend()
    sb = StreamBatch(b, 1, W, HOP)
    b.key = [key]
    return sb


def _schedule(seed):
    """per tick: ("push", ids) | ("attach",) | ("detach", slot) | ("reset", ids)"""
    rng = np.random.default_rng(seed)
    ops, attached = [], set()
    for _ in range(4):
        ops.append(("attach",)); attached.add(len(attached))
    for t in range(TICKS):
        if t == 9:
            ops.append(("attach",)); attached.add(4)                     # a client joins a slot nobody has used
        if t == 25:
            ops.append(("detach", 1)); attached.discard(1)
        if t == 31:
            ops.append(("attach",)); attached.add(1)                     # ... and one the previous client left full of scores
        if t == 40:
            ops.append(("reset", [0, 3]))
        ids = sorted(s for s in attached if rng.random() < 0.8)
        if t % 13 == 5:
            ids = sorted(attached)                                       # everybody
        if t % 17 == 3:
            ids = ids[:1]                                                # one stream
        ops.append(("push", ids))
    return ops


@pytest.mark.parametrize("kw", [{}, {"patience": 3, "threshold": 0.5}, {"patience": 1, "threshold": 0.6}, {"debounce_time": 0.1, "threshold": 0.5}],
                         ids=["plain", "patience3", "patience1", "debounce"])
def test_pool_slot_equals_streambatch_of_one(kw):
    backend = ScriptedPoolBackend()
    pool = StreamPool(backend, S, W, HOP)
    singles, next_key, n_scores, n_kept = {}, 100, 0, 0
    chunk = np.zeros((S, HOP), np.int16)
    for op in _schedule(7):
        if op[0] == "attach":
            slot = pool.attach()
            backend.key[slot] = next_key
            singles[slot] = _single(next_key)
            next_key += 1
            assert pool.count[slot] == 0 and not pool.history[:, slot].any()
        elif op[0] == "detach":
            pool.detach(op[1])
            del singles[op[1]]
        elif op[0] == "reset":
            pool.reset(op[1])
            for s in op[1]:
                singles[s].reset()
        else:
            ids = op[1]
            got = pool.push(ids, chunk[:len(ids)], **kw)
            want = np.array([singles[s].push(chunk[:1], **kw)[0] for s in ids], np.float32)
            assert got.dtype == np.float32 and got.shape == (len(ids),)
            assert (got == want).all(), (ids, got, want)
            assert (pool.raw_scores[ids] == np.array([singles[s].raw_scores[0] for s in ids], np.float32)).all()
            assert (pool.post_processed_scores[ids] == want).all()
            n_scores += len(ids); n_kept += int((got != 0).sum())
    assert sorted(singles) == [0, 1, 2, 3, 4] and pool.attached.tolist() == [True] * 5 + [False]
    assert n_scores > 200 and n_kept < n_scores                # the warm-up and the filters zero scores ...
    # ... and pass others - but for a patience of 2 or more: the history holds post-filter scores, as the reference's does, so the
    # run of hits it asks for never builds up (StreamBatch and HipInterpreter.predict share that)
    assert (n_kept == 0) == (kw.get("patience", 0) >= 2), n_kept
    for s, sb in singles.items():                               # the histories themselves
        rows = sb.history.shape[0]
        assert pool.count[s] == rows and (pool.history[30 - rows:, s] == sb.history[:, 0]).all()


def test_pool_errors_match_streambatch():
    pool = StreamPool(ScriptedPoolBackend(), S, W, HOP)
    sb = _single(0)
    chunk = np.zeros((2, HOP), np.int16)
    for bad in ({"patience": 2}, {"debounce_time": 0.5}, {"patience": 2, "debounce_time": 0.5, "threshold": 0.5}):
        with pytest.raises(ValueError) as e1:
            pool.push([0, 1], chunk, **bad)
        with pytest.raises(ValueError) as e2:
            sb.push(chunk[:1], **bad)
        assert str(e1.value) == str(e2.value)
    with pytest.raises(ValueError, match="Numpy array"):
        pool.push([0], [[0] * HOP])
    with pytest.raises(ValueError, match="Numpy array"):
        sb.push([[0] * HOP])
    for ids in ([1, 0], [2, 2], [S], [-1]):
        with pytest.raises(ValueError, match="strictly ascending"):
            pool.push(ids, chunk[:len(ids)])
    for _ in range(S):
        pool.attach()
    with pytest.raises(RuntimeError, match="slots are taken"):
        pool.attach()
    pool.detach(2)
    with pytest.raises(ValueError, match="not attached"):
        pool.detach(2)
    assert pool.attach() == 2
    pool.reset()                                                 # every stream
    assert not pool.count.any() and pool.attached.all()
    pool.close()
