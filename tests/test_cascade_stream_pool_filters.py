"""interpreter.CascadeStreamPool on the CPU: every slot behaves exactly like a CascadeStreamBatch of ONE stream fed that slot's chunks.
The cascade is a duck-typed fake whose two models return scripted probabilities - a session's scores are a function of the session and of
how many chunks it has been pushed, so the two sides agree without any audio arithmetic - and which applies the device's rule itself:
0 / 0 / 0 until the stream's own window is full, the verifier 0 on a closed stream.  The schedule is seeded: 6 slots, 70 ticks, late joins,
skipped ticks, an attach into a slot nobody has used, a detach and re-attach (the slot's next client must inherit nothing) and a reset.
Scores are compared with np.array_equal, plain, with patience per model and with debounce."""
import numpy as np
import pytest

from nanowakeword_amd.config import cascade_pool_open
from nanowakeword_amd.interpreter import CascadeStreamBatch, CascadeStreamPool

S, W, HOP, TICKS, THR = 6, 4800, 640, 70, 0.45


def _scores(key: int, pushes: int):
    """(gate probability, verifier probability) a session reports for its `pushes`-th chunk once its window is full"""
    gate = np.float32(np.sin(0.29 * pushes + 0.9 * key) * 0.5 + 0.5)
    ver = np.float32(0.0 if (pushes + key) % 11 == 0 else np.cos(0.41 * pushes + 1.7 * key) * 0.5 + 0.5)      # exact zeros too
    return gate, ver


class ScriptedCascade:
    """stream_* of session.HipCascade, scripted: `key[s]` names the session in slot s"""

    gate_threshold = THR

    def stream_open(self, n, window, hop):
        self.S, self.W, self.hop = n, window, hop
        self.key = list(range(n))
        self.pushes, self.filled = np.zeros(n, int), np.zeros(n, int)

    def stream_reset(self):
        self.pushes[:] = 0; self.filled[:] = 0

    def stream_reset_some(self, ids):
        self.pushes[ids] = 0; self.filled[ids] = 0

    def stream_push_some(self, ids, chunk, gate_threshold=None):
        ids = np.asarray(ids, int)
        assert chunk.shape == (len(ids), self.hop) and chunk.dtype == np.int16 and (np.diff(ids) > 0).all()
        self.pushes[ids] += 1; self.filled[ids] += self.hop
        scored = self.filled[ids] >= self.W
        both = np.array([_scores(self.key[s], self.pushes[s]) for s in ids], np.float32).reshape(len(ids), 2)
        gp = np.where(scored, both[:, 0], np.float32(0)).astype(np.float32)
        open_ = cascade_pool_open(gp, scored, self.gate_threshold if gate_threshold is None else gate_threshold)
        probs = np.where(open_, both[:, 1], np.float32(0)).astype(np.float32)
        logits = np.where(open_, np.float32(1), np.where(scored, np.float32(-np.inf), np.float32(0))).astype(np.float32)
        return gp, logits, probs, int(open_.sum())

    def stream_push(self, chunk, gate_threshold=None):          # one lock-step stream: CascadeStreamBatch(S = 1)
        return self.stream_push_some(np.arange(self.S), chunk, gate_threshold)

    def stream_close(self):
        self.closed = True


def _single(key):
    c = ScriptedCascade()
    sb = CascadeStreamBatch(c, 1, W, HOP, gate_name="lite", name="kw")
    c.key = [key]
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
        if t == 30:
            ops.append(("detach", 1)); attached.discard(1)
        if t == 36:
            ops.append(("attach",)); attached.add(1)                     # ... and one the previous client left full of scores
        if t == 50:
            ops.append(("reset", [0, 3]))
        ids = sorted(s for s in attached if rng.random() < 0.8 and not (s == 2 and t < 4))      # slot 2's client is late; ticks are skipped
        if t % 13 == 5:
            ids = sorted(attached)                                       # everybody
        if t % 17 == 3:
            ids = ids[:1]                                                # one stream
        ops.append(("push", ids))
    return ops


FILTERS = [{}, {"patience": {"kw": 1}, "threshold": {"kw": 0.5}}, {"patience": {"kw": 3, "lite": 1}, "threshold": {"kw": 0.5, "lite": 0.6}},
           {"debounce_time": 0.1, "threshold": {"kw": 0.5}}, {"debounce_time": 0.2, "threshold": {"kw": 0.4, "lite": 0.5}}]


@pytest.mark.parametrize("kw", FILTERS, ids=["plain", "patience1", "patience3_and_gate", "debounce", "debounce_both"])
def test_pool_slot_equals_cascade_stream_batch_of_one(kw):
    cascade = ScriptedCascade()
    pool = CascadeStreamPool(cascade, S, W, HOP, gate_name="lite", name="kw")
    singles, next_key = {}, 100
    n_scores, kept = 0, {"lite": 0, "kw": 0}
    closed_behind_warmup = 0
    chunk = np.zeros((S, HOP), np.int16)
    for op in _schedule(7):
        if op[0] == "attach":
            slot = pool.attach()
            cascade.key[slot] = next_key
            singles[slot] = _single(next_key)
            next_key += 1
            assert pool.count[slot] == 0 and pool.filled[slot] == 0 and not any(pool.history[n][:, slot].any() for n in ("lite", "kw"))
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
            want = [singles[s].push(chunk[:1], **kw) for s in ids]
            assert sorted(got) == ["kw", "lite"]
            for name in ("lite", "kw"):
                w = np.array([x[name][0] for x in want], np.float32)
                assert got[name].dtype == np.float32 and got[name].shape == (len(ids),)
                assert np.array_equal(got[name], w), (name, ids, got[name], w)
                assert np.array_equal(pool.raw_scores[name][ids], np.array([singles[s].raw_scores[name][0] for s in ids], np.float32)), name
                assert np.array_equal(pool.post_processed_scores[name][ids], w)
                kept[name] += int((got[name] != 0).sum())
            n_scores += len(ids)
            closed_behind_warmup += int(((got["lite"] != 0) & (pool.raw_scores["kw"][ids] == 0)).sum())
            assert pool.n_open == sum(singles[s].n_open for s in ids)
    assert sorted(singles) == [0, 1, 2, 3, 4] and pool.attached.tolist() == [True] * 5 + [False]
    assert n_scores > 200 and 0 < kept["lite"] < n_scores              # the warm-up zeroes scores and passes others
    # the verifier passes scores too - but for a patience of 2 or more: the history holds post-filter scores, as the reference's does,
    # so the run of hits it asks for never builds up (CascadeStreamBatch and HipInterpreter.predict share that)
    assert (kept["kw"] == 0) == (kw.get("patience", {}).get("kw", 0) >= 2), kept
    assert closed_behind_warmup > 0                                     # streams the gate closed behind its warm-up
    for s, sb in singles.items():                                       # the histories themselves
        for name in ("lite", "kw"):
            rows = sb.history[name].shape[0]
            assert pool.count[s] == rows and np.array_equal(pool.history[name][30 - rows:, s], sb.history[name][:, 0])
    pool.close()
    assert cascade.closed


def test_pool_errors_match_cascade_stream_batch():
    pool = CascadeStreamPool(ScriptedCascade(), S, W, HOP, gate_name="lite", name="kw")
    sb = _single(0)
    chunk = np.zeros((2, HOP), np.int16)
    for bad in ({"patience": {"kw": 2}}, {"debounce_time": 0.5}, {"patience": {"kw": 2}, "debounce_time": 0.5, "threshold": {"kw": 0.5}}):
        with pytest.raises(ValueError) as e1:
            pool.push([0, 1], chunk, **bad)
        with pytest.raises(ValueError) as e2:
            sb.push(chunk[:1], **bad)
        assert str(e1.value) == str(e2.value)
    with pytest.raises(ValueError, match="Numpy array"):
        pool.push([0], [[0] * HOP])
    with pytest.raises(ValueError, match="two names"):
        CascadeStreamPool(ScriptedCascade(), S, W, HOP, gate_name="kw", name="kw")
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
    pool.push([0, 1], chunk)
    pool.reset()                                                 # every stream
    assert not pool.count.any() and not pool.filled.any() and pool.attached.all()
