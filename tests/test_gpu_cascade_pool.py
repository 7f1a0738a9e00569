"""Gate + verifier cascades on stream pools (nww_cascade_stream_push_some / _reset_some) on the GPU (run with -m gpu): the listed streams
of a batch push, join and reset on their own, the gate scores those whose own ring holds a window, and the verifier runs on the ones the
gate opens.  The oracle is the library itself: a second gate handle that receives the same stream_push_some calls for the gate's
probabilities, config.cascade_pool_open for the open set, verifier.forward_pcm on the open streams' windows - cut on the host from the
audio each stream was fed and stacked in ascending stream order - and 0 / 0 on streams that hold no window, -inf / 0 on closed ones;
equality is np.array_equal throughout.  Every threshold is taken from the second gate handle's probabilities, so every open set is known
exactly.  Shapes are small on purpose: W = 3200 (T = 21, edge frames el = er = 2), S = 6."""
import ctypes as C

import numpy as np
import pytest

from nanowakeword_amd.config import FrontendConfig, HeadConfig, cascade_pool_open
from nanowakeword_amd.synth import synth_pcm, synth_state_dict

pytestmark = pytest.mark.gpu

S, W, T, EL, ER, TICKS = 6, 3200, 21, 2, 2, 24
NEG_INF = np.float32(-np.inf)
GATE, VER = HeadConfig("cnn", (T, 64)), HeadConfig("gru", (T, 64))


def _model(cfg, g):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg), window=g["window"], mel_fb=g["fb64"])


def _cascade(g, gate_cfg=GATE, ver_cfg=VER, verifier=None):
    from nanowakeword_amd.session import HipCascade
    return HipCascade(_model(gate_cfg, g), verifier or _model(ver_cfg, g))


def _launches(m):
    return sum(c for _, _, c in m.get_profile())


def _audio(n_streams, n, seed):
    kinds = ("speechlike", "noise", "loud", "speechlike", "chirp", "noise")
    x = np.concatenate([synth_pcm(kinds[s % len(kinds)], 1, n, seed=seed + 3 * s) for s in range(n_streams)], 0)
    x[3, n // 3:n // 3 + 1500] = 0                         # a stretch of digital silence
    return x


class Host:
    """what the test knows of every stream: the samples it was fed since its last reset"""

    def __init__(self, audio, hop):
        self.audio, self.hop = audio, hop
        self.cursor = np.zeros(len(audio), int)
        self.hist = [np.zeros(0, np.int16) for _ in range(len(audio))]

    def reset(self, ids):
        for s in ids:
            self.hist[s] = np.zeros(0, np.int16)

    def chunk(self, ids):
        rows = []
        for s in ids:
            c = self.audio[s, self.cursor[s]:self.cursor[s] + self.hop]
            assert len(c) == self.hop
            self.cursor[s] += self.hop
            self.hist[s] = np.concatenate([self.hist[s], c])
            rows.append(c)
        return np.ascontiguousarray(np.stack(rows)) if rows else np.zeros((0, self.hop), np.int16)

    def filled(self, s):
        return len(self.hist[s])

    def scored(self, ids):
        return np.array([self.filled(s) >= W for s in ids], bool)

    def windows(self, streams):
        return np.ascontiguousarray(np.stack([self.hist[s][-W:] for s in streams]))


def _want(ver, host, ids, g_pr, thr):
    """the oracle of one call: (open mask, logits, probabilities) for the listed streams, after host.chunk(ids)"""
    ids = np.asarray(ids, int)
    scored = host.scored(ids)
    open_ = cascade_pool_open(g_pr, scored, thr)
    want_l, want_p = np.zeros(len(ids), np.float32), np.zeros(len(ids), np.float32)
    want_l[scored] = NEG_INF
    if open_.any():
        want_l[open_], want_p[open_] = ver.forward_pcm(host.windows(ids[open_]))
    return open_, want_l, want_p


def _kth(p, k):
    """the threshold that opens exactly the k largest of the probabilities p (when they are distinct)"""
    return float(np.sort(p)[-k])


def _schedule(hop):
    """[(streams reset before the tick, streams that push)] and the fill counts after every tick: stream 2 starts three ticks late,
    stream 4 skips every third tick, stream 5 is reset once its ring is full"""
    fill_ticks = -(-W // hop)
    filled, out, fills = np.zeros(S, int), [], []
    for t in range(TICKS):
        resets = [5] if t == fill_ticks + 1 else []
        ids = [s for s in range(S) if not (s == 2 and t < 3) and not (s == 4 and t % 3 == 2)]
        filled[resets] = 0
        filled[ids] += hop
        out.append((resets, ids))
        fills.append(filled.copy())
    return out, fills


# ---- 1. a schedule that makes the streams' states differ, on both routes of the gate
@pytest.mark.parametrize("hop,route", [(320, 1), (296, 0)], ids=["shared_frames", "whole_windows"])
def test_schedule(golden_frontend, hop, route):
    g = golden_frontend
    ver, ver_none = _model(VER, g), _model(VER, g)
    # three cascades receive every call, each with its own threshold rule: the k-th largest scored probability, 2.0 and 0.0
    cas = {"kth": _cascade(g, verifier=ver), "none": _cascade(g, verifier=ver_none), "all": _cascade(g, verifier=ver)}
    alone = _model(GATE, g)                                  # the gate alone: the same stream_push_some calls
    sched, fills = _schedule(hop)
    # the tick the schedule is there for: listed together a stream that holds no window yet, one that scores its first whole window and a
    # primed one (scored before) with a LOWER number, so that the slot order of the gate's table (whole windows first) is not list order
    special = [t for t, (_, ids) in enumerate(sched)
               if any(fills[t][s] < W for s in ids)
               and any(W <= fills[t][a] < W + hop and any(fills[t][b] >= W + hop for b in ids if b < a) for a in ids)]
    assert special, "the schedule has no tick with a not-full, a first-window and a lower-numbered primed stream"
    special = special[0]
    checked = [special, special + 3, TICKS - 1]
    host = Host(_audio(S, hop * (TICKS + 1), 300 + hop), hop)
    for c in cas.values():
        c.stream_open(S, W, hop)
    alone.stream_open(S, W, hop)
    ver_none.set_profiling(True)
    seen_open = {k: [] for k in cas}
    for t, (resets, ids) in enumerate(sched):
        if resets:
            assert all(host.filled(s) >= W for s in resets)           # its ring is full when it is reset
            for c in cas.values():
                c.stream_reset_some(resets)
            alone.stream_reset_some(resets)
            host.reset(resets)
            assert all(cas["kth"].stream_filled_of(s) == 0 for s in resets)
        chunk = host.chunk(ids)
        assert [host.filled(s) for s in range(S)] == fills[t].tolist()
        _, g_pr = alone.stream_push_some(ids, chunk)
        stats = alone.stream_pool_stats()
        scored = host.scored(ids)
        assert stats[:2] == (int(scored.sum()), route)
        n_sc = int(scored.sum())
        if t in checked:
            assert n_sc >= 3 and len(set(g_pr[scored].tolist())) == n_sc, (t, g_pr)    # distinct scores: the k-th largest opens exactly k
        thr = {"kth": _kth(g_pr[scored], max(1, n_sc // 2)) if n_sc else 0.5, "none": 2.0, "all": 0.0}
        if t == special:
            n_first = sum(W <= host.filled(s) < W + hop for s in ids)
            n_primed = n_sc - n_first
            assert n_sc < len(ids) and n_first >= 1 and n_primed >= 1
            if route == 1:                                     # the gate's frontend was asked for whole windows AND for hops
                assert stats[2] == n_first * T + n_primed * (EL + hop // 160 + ER), stats
        for name, c in cas.items():
            gp, lg, pr, n_open = c.stream_push_some(ids, chunk, gate_threshold=thr[name])
            open_, want_l, want_p = _want(c.verifier, host, ids, g_pr, thr[name])
            print("tick", t, name, "thr", thr[name], "listed", len(ids), "scored", n_sc, "open", n_open)
            assert gp.dtype == lg.dtype == pr.dtype == np.float32 and gp.shape == lg.shape == pr.shape == (len(ids),)
            assert np.array_equal(gp, g_pr), (t, name, gp, g_pr)
            assert not gp[~scored].any() and not lg[~scored].any() and not pr[~scored].any(), (t, name)
            assert n_open == int(open_.sum()), (t, name, n_open, open_)
            assert np.array_equal(lg, want_l), (t, name, lg, want_l)
            assert np.array_equal(pr, want_p), (t, name, pr, want_p)
            closed = scored & ~open_
            assert (lg[closed] == NEG_INF).all() and (pr[closed] == 0.0).all() and np.isfinite(lg[open_]).all()
            assert c.gate.stream_pool_stats() == stats, (t, name)
            assert all(c.stream_filled_of(s) == host.filled(s) for s in range(S)), (t, name)
            seen_open[name].append((n_open, n_sc))
    for t in checked:
        assert 0 < seen_open["kth"][t][0] < seen_open["kth"][t][1], (t, seen_open["kth"][t])
        assert seen_open["none"][t][0] == 0 and seen_open["all"][t] == (seen_open["all"][t][1],) * 2
    assert len(set(pr[open_].tolist())) > 1                                         # (the last tick, every scored stream open)
    assert _launches(ver_none) == 0                                                  # threshold 2.0: the verifier never ran
    ids = list(range(S))
    assert cas["none"].stream_push_some(ids, host.chunk(ids), gate_threshold=0.0)[3] == S
    assert _launches(ver_none) > 0                                                   # the profile does count a verifier run
    ver_none.set_profiling(False)
    for c in cas.values():
        c.stream_close()
        c.gate.close()
    alone.stream_close()
    for m in (alone, ver, ver_none):
        m.close()


# ---- 2. aligned batches
def test_aligned_batch_keeps_lock_step(golden_frontend):
    """calls that list every stream of a fresh batch equal the lock-step stream_push of a twin cascade and keep the batch aligned: a
    lock-step push afterwards still runs; after one partial call it is refused (existing behaviour, seen from the new path)"""
    from nanowakeword_amd.session import NwwError
    g, hop = golden_frontend, 320
    ver = _model(VER, g)
    cas, twin, alone = _cascade(g, verifier=ver), _cascade(g, verifier=ver), _model(GATE, g)
    for c in (cas, twin):
        c.stream_open(S, W, hop)
    alone.stream_open(S, W, hop)
    every, ticks = list(range(S)), W // hop + 3
    audio = _audio(S, hop * (ticks + 2), 77)
    chunks = [np.ascontiguousarray(audio[:, t * hop:(t + 1) * hop]) for t in range(ticks + 2)]
    opened = []
    for t in range(ticks):
        _, g_pr = alone.stream_push(chunks[t])
        thr = _kth(g_pr, S // 2) if g_pr.any() else 0.0
        want = twin.stream_push(chunks[t], gate_threshold=thr)
        got = cas.stream_push_some(every, chunks[t], gate_threshold=thr)
        for a, b in zip(got[:3], want[:3]):
            assert np.array_equal(a, b), (t, a, b)
        assert got[3] == want[3]
        assert np.array_equal(got[0], g_pr)
        opened.append(got[3])
        assert cas.stream_filled() == (t + 1) * hop == cas.stream_filled_of(3)
    assert opened[:W // hop - 1] == [0] * (W // hop - 1) and all(0 < n < S for n in opened[W // hop - 1:]), opened
    # a lock-step push on the cascade that was driven through push_some: still aligned
    _, g_pr = alone.stream_push(chunks[ticks])
    thr = _kth(g_pr, 2)
    got, want = cas.stream_push(chunks[ticks], gate_threshold=thr), twin.stream_push(chunks[ticks], gate_threshold=thr)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3] == 2
    # one partial call ends that
    part = [0, 1, 2, 4, 5]
    cas.stream_push_some(part, np.ascontiguousarray(chunks[ticks + 1][part]))
    with pytest.raises(NwwError, match="no longer share one state"):
        cas.stream_push(chunks[ticks + 1])
    assert cas.stream_filled_of(3) == (ticks + 1) * hop and cas.stream_filled_of(0) == (ticks + 2) * hop
    # the launch list of a pool call differs from the lock-step one in its select alone
    lock, pool = cas.describe().split("\n"), cas.describe(pool=True).split("\n")
    diff = [i for i, (a, b) in enumerate(zip(lock, pool)) if a != b]
    assert len(lock) == len(pool) and len(diff) == 1 and lock[diff[0]].startswith("cascade_select:") and pool[diff[0]].startswith("cascade_pool_select:")
    for c in (cas, twin):
        c.stream_close()
        c.gate.close()
    alone.stream_close(); alone.close(); ver.close()


# ---- 3. device pointers
def test_device_variant_equals_host_variant(golden_frontend):
    torch = pytest.importorskip("torch")
    g, hop = golden_frontend, 320
    ver = _model(VER, g)
    cas_h, cas_d, alone = _cascade(g, verifier=ver), _cascade(g, verifier=ver), _model(GATE, g)
    for c in (cas_h, cas_d):
        c.stream_open(S, W, hop)
    alone.stream_open(S, W, hop)
    ticks = W // hop + 5
    host = Host(_audio(S, hop * (ticks + 1), 21), hop)
    mixed = 0
    for t in range(ticks):
        ids = [s for s in range(S) if not (s == 2 and t < 3) and not (s == 4 and t % 3 == 2)]
        n = len(ids)
        chunk = host.chunk(ids)
        _, g_pr = alone.stream_push_some(ids, chunk)
        scored = host.scored(ids)
        thr = _kth(g_pr[scored], max(1, int(scored.sum()) // 2)) if scored.any() else 0.0
        gp, lg, pr, n_open = cas_h.stream_push_some(ids, chunk, gate_threshold=thr)
        d_chunk = torch.from_numpy(chunk).cuda()
        out = [torch.full((n + 1,), -7.0, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()                                          # the library enqueues on its own stream
        # (a d_gate_probs of 0 on every other tick: the gate's probabilities then stay inside the library)
        n_dev = cas_d.stream_push_some_dev(ids, d_chunk.data_ptr(), out[0].data_ptr() if t % 2 else 0, out[1].data_ptr(), out[2].data_ptr(),
                                           gate_threshold=thr)
        torch.cuda.synchronize()
        assert n_dev == n_open, (t, n_dev, n_open)
        for k, (o, want) in enumerate(zip(out, (gp, lg, pr))):
            got = o.cpu().numpy()
            assert got[n] == -7.0                                         # nothing written behind the last listed stream
            if k == 0 and not t % 2:
                assert (got == -7.0).all()
            else:
                assert np.array_equal(got[:n], want), (t, k, got, want)
        mixed += 0 < n_open < int(scored.sum()) and int((~scored).sum()) > 0
    assert mixed > 0                                 # ticks with not-full, closed and open streams listed together went through both
    for c in (cas_h, cas_d):
        c.stream_close()
        c.gate.close()
    alone.stream_close(); alone.close(); ver.close()


# ---- 4. the interpreter
@pytest.mark.parametrize("filt", [{}, {"patience": {"kw": 1}}], ids=["plain", "patience"])
def test_cascade_stream_pool_equals_interpreters(golden_frontend, filt):
    """every slot of a CascadeStreamPool against a HipInterpreter of its own with a cascade_config, predict() called only on the ticks
    the slot is listed, a fresh interpreter after attach"""
    from nanowakeword_amd.interpreter import CascadeStreamPool, HipInterpreter
    from nanowakeword_amd.session import HipSession
    g, hop, n_slots, ticks = golden_frontend, 320, 4, W // 320 + 14
    cas = _cascade(g)
    gate2, ver2 = _model(GATE, g), _model(VER, g)
    audio = _audio(n_slots + 1, hop * ticks, 70)                          # one track per client: slot 3 serves two of them
    wins = np.ascontiguousarray(np.concatenate([audio[s, a:a + W][None] for s in range(n_slots + 1) for a in range(0, hop * ticks - W + 1, 4 * hop)]))
    cas.gate_threshold = float(np.median(gate2.forward_pcm(wins)[1]))     # from the gate's own scores: some windows open, some closed
    kw = dict(filt)
    if filt:
        kw["threshold"] = {"kw": float(np.median(ver2.forward_pcm(wins)[1]))}

    def interpreter():
        it = HipInterpreter({"lite": HipSession(gate2, clip_samples=W, name="lite"), "kw": HipSession(ver2, clip_samples=W, name="kw")})
        it.cascade_config = {"gate": "lite", "verifier": "kw", "gate_threshold": cas.gate_threshold}
        return it

    pool = CascadeStreamPool(cas, n_slots, W, hop, gate_name="lite", name="kw")
    its, track, cursor = {}, {}, {}
    for s in range(n_slots):
        assert pool.attach() == s
        its[s], track[s], cursor[s] = interpreter(), s, 0
    seen = {"lite": [], "kw": []}
    for t in range(ticks):
        if t == W // hop + 3:                                             # the client of slot 3 leaves; another takes the slot
            pool.detach(3)
            assert pool.attach() == 3
            its[3], track[3], cursor[3] = interpreter(), n_slots, 0
        ids = [s for s in range(n_slots) if not (s == 2 and t < 3) and not (s == 1 and t % 4 == 2)]
        rows = []
        for s in ids:
            rows.append(audio[track[s], cursor[s]:cursor[s] + hop])
            cursor[s] += hop
        chunk = np.ascontiguousarray(np.stack(rows))
        got = pool.push(ids, chunk, **kw)
        want = [its[s].predict(chunk[i], **kw).scores for i, s in enumerate(ids)]
        for name in ("lite", "kw"):
            assert np.array_equal(got[name], np.array([w[name] for w in want], np.float32)), (t, name, got[name], want)
            assert np.array_equal(pool.raw_scores[name][ids], np.array([its[s].raw_scores[name] for s in ids], np.float32)), (t, name)
            seen[name].append(got[name])
    lite, kw_scores = np.concatenate(seen["lite"]), np.concatenate(seen["kw"])
    assert (lite != 0).any() and (kw_scores != 0).any()                   # non-zero scores behind the warm-up ...
    assert (kw_scores[lite != 0] == 0).any()                              # ... and streams the gate closed
    pool.close()
    gate2.close(); ver2.close()
    cas.gate.close(); cas.verifier.close()


# ---- 5. errors
def test_errors(golden_frontend):
    from nanowakeword_amd.session import HipCascade, NwwError
    g, hop = golden_frontend, 320
    cas = _cascade(g)
    gate, ver = cas.gate, cas.verifier
    lib = gate.lib
    chunk = synth_pcm("noise", S, hop, seed=1)
    out = [np.full(S, 7.0, np.float32) for _ in range(3)]
    n_open = C.c_int32(-5)

    def push(gate_h, ver_h, ids, chunk_ptr=chunk.ctypes.data_as(C.c_void_p)):
        ids = np.asarray(ids, np.int32)
        return lib.nww_cascade_stream_push_some(gate_h, ver_h, ids.ctypes.data_as(C.c_void_p), len(ids), chunk_ptr, 0.0,
                                                out[0].ctypes.data_as(C.c_void_p), out[1].ctypes.data_as(C.c_void_p),
                                                out[2].ctypes.data_as(C.c_void_p), C.byref(n_open))

    def untouched():
        return all((o == 7.0).all() for o in out)

    # no open batch
    assert push(gate._h, ver._h, [0, 1, 2]) == 5 and b"no open stream batch" in lib.nww_last_error(ver._h)           # NWW_ERR_STATE
    one = np.zeros(1, np.int32)
    assert lib.nww_cascade_stream_reset_some(gate._h, ver._h, one.ctypes.data_as(C.c_void_p), 1) == 5
    with pytest.raises(NwwError, match="gate: no open stream batch"):
        cas.stream_reset_some([0])
    cas.stream_open(S, W, hop)
    for t in range(W // hop + 1):                                        # every stream but 3 holds a window: a call that went through would score
        ids = [s for s in range(S) if s != 3 or t % 2]
        cas.stream_push_some(ids, np.ascontiguousarray(synth_pcm("noise", S, hop, seed=t)[ids]), gate_threshold=0.0)
    filled = [cas.stream_filled_of(s) for s in range(S)]
    assert filled[3] < W <= filled[0]
    # idx descending, repeated or out of range
    for bad in ([2, 1, 0], [0, 2, 1], [1, 1, 3], [0, 1, S], [-1, 0, 1]):
        assert push(gate._h, ver._h, bad) == 1, bad                      # NWW_ERR_INVALID
        assert b"strictly ascending" in lib.nww_last_error(ver._h)
        assert [cas.stream_filled_of(s) for s in range(S)] == filled and untouched()
    with pytest.raises(ValueError, match="strictly ascending"):
        cas.stream_push_some([1, 0], chunk[:2])
    with pytest.raises(ValueError, match="chunk must have shape"):
        cas.stream_push_some([0, 1], chunk)
    assert push(gate._h, ver._h, [0, 1, 2], None) == 1 and b"null chunk" in lib.nww_last_error(ver._h)
    bad = np.asarray([3, 3], np.int32)
    assert lib.nww_cascade_stream_reset_some(gate._h, ver._h, bad.ctypes.data_as(C.c_void_p), 2) == 1
    # the same handle twice
    assert push(gate._h, gate._h, [0, 1, 2]) == 1 and b"distinct" in lib.nww_last_error(gate._h)
    assert lib.nww_cascade_stream_reset_some(gate._h, gate._h, one.ctypes.data_as(C.c_void_p), 1) == 1
    assert [cas.stream_filled_of(s) for s in range(S)] == filled and untouched()
    # a verifier built for another window
    other = _model(HeadConfig("gru", (31, 64)), g)
    assert push(gate._h, other._h, [0, 1, 2]) == 3                       # NWW_ERR_SHAPE
    assert b"verifier: frontend yields (21,64) features for 3200 samples" in lib.nww_last_error(other._h)
    with pytest.raises(ValueError, match="verifier: frontend yields"):
        HipCascade(gate, other).stream_push_some([0, 1, 2], chunk[:3])
    assert [cas.stream_filled_of(s) for s in range(S)] == filled and untouched()
    # n == 0: NWW_OK, nothing is launched or written
    ver.set_profiling(True)
    assert lib.nww_cascade_stream_push_some(gate._h, ver._h, None, 0, None, 0.0, out[0].ctypes.data_as(C.c_void_p), out[1].ctypes.data_as(C.c_void_p),
                                            out[2].ctypes.data_as(C.c_void_p), C.byref(n_open)) == 0
    assert n_open.value == 0 and untouched() and gate.stream_pool_stats()[0] == 0 and _launches(ver) == 0
    e = cas.stream_push_some([], np.zeros((0, hop), np.int16))
    assert e[0].shape == e[1].shape == e[2].shape == (0,) and e[3] == 0 and _launches(ver) == 0
    ver.set_profiling(False)
    assert [cas.stream_filled_of(s) for s in range(S)] == filled
    # the pair still works: a good call goes through and scores
    assert push(gate._h, ver._h, [0, 1, 3]) == 0 and n_open.value == 2
    assert out[0][2] == 0 and out[1][2] == 0 and out[2][2] == 0 and np.isfinite(out[1][:2]).all() and out[0][:2].all()
    assert [cas.stream_filled_of(s) for s in (0, 1, 3)] == [filled[0] + hop, filled[1] + hop, filled[3] + hop]
    cas.stream_close()
    other.close(); gate.close(); ver.close()
