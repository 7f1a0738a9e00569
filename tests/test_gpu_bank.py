"""Model banks (nww_bank_*, session.HipBank) on the GPU (run with -m gpu): several heads score the same audio on ONE frontend pass -
the leader's - and every member's logits and probabilities are bit-identical to the single-handle call on that member alone, whichever
member leads.  The oracle is the library's own single-handle calls (forward_pcm, forward_recording, stream_push_some on a batch of its
own); equality is np.array_equal throughout.  Shapes are small on purpose: W = 3200 (T = 21, edge frames el = er = 2), 64 mel, S = 6."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_pcm, synth_state_dict

pytestmark = pytest.mark.gpu

S, W, T, TICKS = 6, 3200, 21, 24
CFGS = OrderedDict([("cnn", HeadConfig("cnn", (T, 64))), ("gru", HeadConfig("gru", (T, 64))), ("dnn", HeadConfig("dnn", (T, 64))),
                    ("crnn", HeadConfig("crnn", (T, 64), crnn_rnn_type="gru"))])
NAMES = list(CFGS)


def _model(cfg, g, fe=None, mel_fb=None, finalize=True, **kw):
    from nanowakeword_amd.session import HipModel
    m = HipModel(cfg, fe or FrontendConfig(), window=g["window"], mel_fb=g["fb64"] if mel_fb is None else mel_fb, **kw)
    m.load_state_dict(synth_state_dict(cfg))
    return m.finalize() if finalize else m


def _bank(models, order=None):
    from nanowakeword_amd.session import HipBank
    return HipBank(OrderedDict((n, models[n]) for n in (order or list(models))))


def _audio(n_rows, n, seed):
    kinds = ("speechlike", "noise", "loud", "speechlike", "chirp", "noise")
    x = np.concatenate([synth_pcm(kinds[s % len(kinds)], 1, n, seed=seed + 3 * s) for s in range(n_rows)], 0)
    if n_rows > 3:
        x[3, n // 3:n // 3 + 1500] = 0                     # a stretch of digital silence
    return x


@pytest.fixture(scope="module")
def members(golden_frontend):
    ms = OrderedDict((n, _model(c, golden_frontend)) for n, c in CFGS.items())
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def batches(members):
    """the clips of the batch tests and every member's own forward_pcm on them, computed once"""
    out = {}
    for B in (1, 7, 129):                                  # 129 crosses the 128-clip row block of the blocked trunk -> fc1 hand-over
        pcm = _audio(B, W, 500 + B)
        out[B] = (pcm, {n: m.forward_pcm(pcm) for n, m in members.items()})
    return out


def _same(got, want, what):
    assert set(got) == set(want), what
    for n in want:
        for a, b, kind in zip(got[n], want[n], ("logits", "probs")):
            assert a.dtype == np.float32 and a.shape == b.shape, (what, n, kind)
            assert np.array_equal(a, b), (what, n, kind, a, b)


# ---- 1. a batch of clips
@pytest.mark.parametrize("B", [1, 7, 129])
def test_batch_equals_every_member_alone(members, batches, B):
    pcm, want = batches[B]
    assert all(np.isfinite(l).all() and (B == 1 or len(set(l.tolist())) > 1) for l, _ in want.values())
    for lead in range(len(NAMES)):                         # each member leads in turn
        order = NAMES[lead:] + NAMES[:lead]
        bank = _bank(members, order)
        assert bank.names == order and bank.leader is members[order[0]]
        bank.check(W)
        _same(bank.forward_pcm(pcm), want, (B, order))
    for n in NAMES:                                        # k = 1 is the plain call
        _same(_bank({n: members[n]}).forward_pcm(pcm), {n: want[n]}, (B, "k=1", n))
    # two members, and a call without one of the outputs (either may be NULL)
    pair = _bank(members, ["dnn", "cnn"])
    _same(pair.forward_pcm(pcm), {n: want[n] for n in ("dnn", "cnn")}, (B, "pair"))
    probs = np.full((2, B), 7.0, np.float32)
    arr = pcm if pcm.flags["C_CONTIGUOUS"] else np.ascontiguousarray(pcm)
    assert pair.lib.nww_bank_forward_pcm(pair._members, 2, arr.ctypes.data_as(C.c_void_p), B, W, None, probs.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(probs[0], want["dnn"][1]) and np.array_equal(probs[1], want["cnn"][1])


# ---- 2. the frontend runs once
def test_frontend_runs_once(members, batches):
    pcm, want = batches[7]
    alone = {}
    for n, m in members.items():                           # what one single-handle call records, per plan entry
        m.set_profiling(True)
        m.forward_pcm(pcm)
        alone[n] = [c for _, _, c in m.get_profile()]
        assert alone[n][0] == 1 and sum(alone[n][1:]) >= 1, (n, alone[n])
        m.set_profiling(True)                              # (restarts the counts)
    bank = _bank(members)
    _same(bank.forward_pcm(pcm), want, "profiled")
    for j, (n, m) in enumerate(members.items()):
        prof = m.get_profile()
        got = [c for _, _, c in prof]
        print(n, prof)
        assert got[1:] == alone[n][1:], (n, got, alone[n])                 # one launch for every head entry of every member
        assert got[0] == (1 if j == 0 else 0), (n, got)                    # the frontend: once, on the leader
        assert j == 0 or prof[0][1:] == (0.0, 0), (n, prof[0])               # a follower's entry 0 records nothing
        m.set_profiling(False)


# ---- 3. followers read the leader's input
def test_followers_read_the_leaders_input(members, batches):
    pcm, want = batches[7]
    for n in NAMES[1:]:
        members[n].forward_pcm(pcm)                        # its own buffers exist ...
        members[n].poison_recording_workspace(float("nan"))      # ... and hold NaN: a follower that read its own head input scores NaN
    _same(_bank(members).forward_pcm(pcm), want, "poisoned followers")
    # (the instrument does poison: the dense head input of a model that runs its head alone on it)
    for n in NAMES[1:]:
        _same({n: members[n].forward_pcm(pcm)}, {n: want[n]}, "alone again")


# ---- 4. every window of a recording
@pytest.mark.parametrize("hop,route", [(320, 1), (296, 0)], ids=["shared_frames", "strided"])
def test_recording(members, hop, route):
    n = W + 37 * hop + 5                                   # 38 windows in passes of 16: several passes and a partial last one
    x = _audio(4, n, 40 + hop)
    pcm = np.ascontiguousarray(np.concatenate([x[2, :n // 3], x[3, n // 3:]]))      # loud, then digital silence, then speech-like
    want = {name: m.forward_recording(pcm, window=W, hop=hop, max_batch=16) for name, m in members.items()}
    assert all(len(l) == 38 and np.isfinite(l).all() and len(set(l.tolist())) > 1 for l, _ in want.values())
    for order in (NAMES, NAMES[2:] + NAMES[:2]):
        bank = _bank(members, order)
        assert bank.leader.recording_route(W, hop) == route
        _same(bank.forward_recording(pcm, window=W, hop=hop, max_batch=16), want, (hop, order))
    # an offset, and one pass that holds every window
    want = {name: m.forward_recording(pcm, window=W, hop=hop, offset=8, max_batch=64) for name, m in members.items()}
    _same(_bank(members).forward_recording(pcm, window=W, hop=hop, offset=8, max_batch=64), want, (hop, "offset"))
    _same(_bank({"gru": members["gru"]}).forward_recording(pcm, window=W, hop=hop, max_batch=16),
          {"gru": members["gru"].forward_recording(pcm, window=W, hop=hop, max_batch=16)}, (hop, "k=1"))
    # shorter than one window: no windows, no error
    empty = _bank(members).forward_recording(pcm[:W - 8], window=W, hop=hop)
    assert all(l.shape == p.shape == (0,) for l, p in empty.values())


# ---- 5. stream pools
def _schedule(hop):
    """[(streams reset before the tick, streams that push)]: stream 2 starts three ticks late, stream 4 skips every third tick, stream 5
    is reset once its ring is full"""
    fill_ticks = -(-W // hop)
    return [([5] if t == fill_ticks + 1 else [], [s for s in range(S) if not (s == 2 and t < 3) and not (s == 4 and t % 3 == 2)])
            for t in range(TICKS)]


@pytest.mark.parametrize("hop,route", [(320, 1), (296, 0)], ids=["shared_frames", "whole_windows"])
def test_stream_pool(golden_frontend, members, hop, route):
    from nanowakeword_amd.session import NwwError
    twins = OrderedDict((n, _model(c, golden_frontend)) for n, c in CFGS.items())       # K separate models, each with a batch of its own
    bank = _bank(members)
    bank.stream_open(S, W, hop)
    for m in twins.values():
        m.stream_open(S, W, hop)
    audio = _audio(S, hop * (TICKS + 1), 300 + hop)
    cursor = np.zeros(S, int)
    filled = np.zeros(S, int)
    seen = {"not_full": 0, "scored": 0, "mixed": 0}
    for t, (resets, ids) in enumerate(_schedule(hop)):
        if resets:
            assert all(filled[s] >= W for s in resets)
            bank.stream_reset_some(resets)
            for m in twins.values():
                m.stream_reset_some(resets)
            filled[resets] = 0
            assert all(bank.stream_filled_of(s) == 0 for s in resets)
        chunk = np.ascontiguousarray(np.stack([audio[s, cursor[s]:cursor[s] + hop] for s in ids]))
        cursor[ids] += hop
        filled[ids] += hop
        want = {n: m.stream_push_some(ids, chunk) for n, m in twins.items()}
        got = bank.stream_push_some(ids, chunk)
        _same(got, want, (hop, t))
        scored = filled[ids] >= W
        for n in NAMES:                                    # a listed stream that holds no window: 0 / 0 for every member
            assert not got[n][0][~scored].any() and not got[n][1][~scored].any(), (t, n)
            assert got[n][1][scored].all(), (t, n)
        assert bank.stream_pool_stats() == twins[NAMES[0]].stream_pool_stats(), t       # scored, route, frames: the leader's twin's
        assert bank.stream_pool_stats()[:2] == (int(scored.sum()), route)
        assert [bank.stream_filled_of(s) for s in range(S)] == filled.tolist()
        seen["not_full"] += int((~scored).sum()); seen["scored"] += int(scored.sum()); seen["mixed"] += bool(scored.any() and (~scored).any())
    assert all(seen.values()), seen
    for n in NAMES[1:]:                                    # a follower has no stream batch
        with pytest.raises(NwwError, match="no open stream batch"):
            members[n].stream_filled_of(0)
    bank.stream_close()
    for m in twins.values():
        m.stream_close()
        m.close()


def test_aligned_batch_keeps_lock_step(golden_frontend, members):
    """calls that list every stream keep the leader's batch aligned: the lock-step stream_push on the leader alone runs afterwards and
    equals its twin's, which was driven in lock-step throughout"""
    hop, every = 320, list(range(S))
    order = ["crnn", "dnn", "cnn"]                         # a leader whose lock-step path keeps conv rows
    bank = _bank(members, order)
    twin = _model(CFGS["crnn"], golden_frontend)
    bank.stream_open(S, W, hop)
    twin.stream_open(S, W, hop)
    ticks = W // hop + 3
    audio = _audio(S, hop * (ticks + 2), 77)
    chunks = [np.ascontiguousarray(audio[:, t * hop:(t + 1) * hop]) for t in range(ticks + 2)]
    for t in range(ticks):
        want = twin.stream_push(chunks[t])
        got = bank.stream_push_some(every, chunks[t])
        _same({"crnn": got["crnn"]}, {"crnn": want}, t)
        if (t + 1) * hop >= W:
            windows = np.ascontiguousarray(audio[:, (t + 1) * hop - W:(t + 1) * hop])
            _same({n: got[n] for n in ("dnn", "cnn")}, {n: members[n].forward_pcm(windows) for n in ("dnn", "cnn")}, t)
        assert members["crnn"].stream_filled() == (t + 1) * hop == bank.stream_filled_of(3)
    for t in (ticks, ticks + 1):                           # lock-step on the leader alone: the first computes its window whole, the next a hop
        lg, pr = members["crnn"].stream_push(chunks[t])
        wl, wp = twin.stream_push(chunks[t])
        assert np.array_equal(lg, wl) and np.array_equal(pr, wp) and pr.all(), t
    bank.stream_close()
    twin.stream_close(); twin.close()


def test_stream_device_variant_equals_host_variant(golden_frontend, members):
    torch = pytest.importorskip("torch")
    hop = 320
    bank = _bank(members)
    twin_models = OrderedDict((n, _model(c, golden_frontend)) for n, c in CFGS.items())
    host = _bank(twin_models)
    bank.stream_open(S, W, hop)
    host.stream_open(S, W, hop)
    ticks = W // hop + 4
    audio = _audio(S, hop * ticks, 21)
    cursor = np.zeros(S, int)
    k = len(NAMES)
    for t in range(ticks):
        ids = [s for s in range(S) if not (s == 2 and t < 3) and not (s == 4 and t % 3 == 2)]
        n = len(ids)
        chunk = np.ascontiguousarray(np.stack([audio[s, cursor[s]:cursor[s] + hop] for s in ids]))
        cursor[ids] += hop
        want = host.stream_push_some(ids, chunk)
        d_chunk = torch.from_numpy(chunk).cuda()
        out = [torch.full((k * n + 1,), -7.0, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()                           # the library enqueues on its own stream
        bank.stream_push_some_dev(ids, d_chunk.data_ptr(), out[0].data_ptr(), out[1].data_ptr() if t % 2 else 0)
        torch.cuda.synchronize()
        lg, pr = out[0].cpu().numpy(), out[1].cpu().numpy()
        assert lg[k * n] == -7.0 and pr[k * n] == -7.0     # nothing written behind the last member's row
        for j, name in enumerate(NAMES):
            assert np.array_equal(lg[j * n:(j + 1) * n], want[name][0]), (t, name)
            if t % 2:
                assert np.array_equal(pr[j * n:(j + 1) * n], want[name][1]), (t, name)
        if not t % 2:
            assert (pr == -7.0).all()
    # the batch entry point on device pointers
    pcm = _audio(7, W, 9)
    want = {n: m.forward_pcm(pcm) for n, m in members.items()}
    d_pcm = torch.from_numpy(pcm).cuda()
    out = [torch.full((k * 7 + 1,), -7.0, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    bank.forward_pcm_dev(d_pcm.data_ptr(), 7, W, out[0].data_ptr(), out[1].data_ptr())
    torch.cuda.synchronize()
    lg, pr = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert lg[k * 7] == -7.0 and pr[k * 7] == -7.0
    for j, name in enumerate(NAMES):
        assert np.array_equal(lg[j * 7:(j + 1) * 7], want[name][0]) and np.array_equal(pr[j * 7:(j + 1) * 7], want[name][1]), name
    bank.stream_close(); host.stream_close()
    for m in twin_models.values():
        m.close()


# ---- 6. e2e_dnn as a member
def test_e2e_dnn_member(golden_frontend):
    g, N = golden_frontend, 16000
    cnn = _model(HeadConfig("cnn", (101, 64)), g)
    e2e = _model(HeadConfig("e2e_dnn", (64, 101)), g)
    pcm = _audio(3, N, 61)
    want = {"cnn": cnn.forward_pcm(pcm), "e2e": e2e.forward_pcm(pcm)}
    assert len(set(want["e2e"][0].tolist())) == 3
    _same(_bank({"cnn": cnn, "e2e": e2e}).forward_pcm(pcm), want, "cnn leads")
    _same(_bank({"e2e": e2e, "cnn": cnn}).forward_pcm(pcm), want, "e2e_dnn leads")
    # planned in the reference's orientation it reads mel-major log-mel, which no bank provides
    f32 = _model(HeadConfig("e2e_dnn", (64, 101)), g, conv_arith="f32")
    assert np.isfinite(f32.forward_pcm(pcm)[0]).all()
    with pytest.raises(NotImplementedError, match="member 1 reads mel-major"):
        _bank({"cnn": cnn, "f32": f32}).forward_pcm(pcm)
    _same(_bank({"f32": f32}).forward_pcm(pcm), {"f32": f32.forward_pcm(pcm)}, "k=1 has no such rule")
    for m in (cnn, e2e, f32):
        m.close()


# ---- 7. errors
def test_errors(golden_frontend, members):
    from nanowakeword_amd.config import raw_frontend_frames
    g, hop = golden_frontend, 320
    lib = members["cnn"].lib
    pcm = np.ascontiguousarray(_audio(S, W, 5))
    chunk = np.ascontiguousarray(pcm[:, :hop])
    out = [np.full(4 * 64, 7.0, np.float32) for _ in range(2)]
    ids = np.arange(3, dtype=np.int32)

    def arr(ms):
        return (C.c_void_p * max(1, len(ms)))(*[m._h if m is not None else None for m in ms])

    def calls(ms, k=None):
        """the return codes of the three host-pointer entry points and of nww_bank_check on these members"""
        a, k = arr(ms), len(ms) if k is None else k
        o = [x.ctypes.data_as(C.c_void_p) for x in out]
        return [lib.nww_bank_check(a, k, W),
                lib.nww_bank_forward_pcm(a, k, pcm.ctypes.data_as(C.c_void_p), S, W, o[0], o[1]),
                lib.nww_bank_forward_recording(a, k, pcm.ctypes.data_as(C.c_void_p), pcm.size, W, hop, 16, o[0], o[1], None),
                lib.nww_bank_stream_push_some(a, k, ids.ctypes.data_as(C.c_void_p), len(ids), chunk.ctypes.data_as(C.c_void_p), o[0], o[1])]

    def untouched():
        return all((o == 7.0).all() for o in out)

    lead = members["cnn"]
    lead.stream_open(S, W, hop)
    for t in range(W // hop + 1):
        lead.stream_push_some(list(range(S)), np.ascontiguousarray(_audio(S, hop, t)))
    filled = [lead.stream_filled_of(s) for s in range(S)]
    assert min(filled) >= W                                # a call that went through would score

    def refused(ms, code, text, k=None, err_of=lead):
        rcs = calls(ms, k)
        assert rcs == [code] * 4, (text, rcs)
        msg = lib.nww_last_error(err_of._h if err_of is not None else None).decode()
        assert text in msg, (text, msg)
        assert untouched() and [lead.stream_filled_of(s) for s in range(S)] == filled, text

    # another n_mels (and so another head shape): the frontend rule comes first
    fe40 = FrontendConfig(n_mels=40)
    mel40 = _model(HeadConfig("dnn", (T, 40)), g, fe=fe40, mel_fb=g["fb40"])
    refused([lead, members["gru"], mel40], 1, "member 2: its frontend differs from member 0's in n_mels")
    # one entry of the filterbank changed by one ulp
    fb = g["fb64"].copy()
    i = np.flatnonzero(fb.ravel())[7]
    fb.ravel()[i] = np.nextafter(fb.ravel()[i], np.float32(2.0))
    ulp = _model(CFGS["gru"], g, mel_fb=fb)
    refused([lead, ulp], 1, "member 1: its frontend differs from member 0's in frontend.mel_fb")
    # built-in tables against loaded ones (they differ by up to 1e-5 per coefficient)
    from nanowakeword_amd.session import HipModel
    builtin = HipModel(CFGS["gru"], FrontendConfig(), state_dict=synth_state_dict(CFGS["gru"]), tables="builtin")
    refused([lead, builtin], 1, "member 1: its frontend differs from member 0's in frontend.")
    # a raw-PCM head
    probe = HeadConfig("e2e_quartznet", (1, 128))
    raw = _model(HeadConfig("e2e_quartznet", (raw_frontend_frames(probe, W), 128)), g)
    refused([lead, raw], 1, "member 1 is a raw-PCM head")
    # the same handle twice, a NULL member, an unfinalized member, no members
    refused([lead, members["gru"], lead], 1, "member 2 is the same handle as member 0")
    refused([lead, None], 1, "member 1 is NULL")
    loose = _model(CFGS["dnn"], g, finalize=False)
    refused([lead, loose], 1, "member 1: model not finalized")
    refused([lead], 1, "a bank needs k >= 1 members", k=0, err_of=None)
    assert lib.nww_bank_check(None, 2, W) == 1
    # a window that fits the leader but not member 2
    other = _model(HeadConfig("gru", (31, 64)), g)
    refused([lead, members["dnn"], other], 3, "member 2: frontend yields (21,64) features for 3200 samples")
    with pytest.raises(ValueError, match="member 2: frontend yields"):
        _bank(OrderedDict([("a", lead), ("b", members["dnn"]), ("c", other)])).forward_pcm(pcm)
    # the stream call alone: a leader without a batch, a bad index list
    a = arr([members["gru"], members["dnn"]])
    o = [x.ctypes.data_as(C.c_void_p) for x in out]
    assert lib.nww_bank_stream_push_some(a, 2, ids.ctypes.data_as(C.c_void_p), 3, chunk.ctypes.data_as(C.c_void_p), o[0], o[1]) == 5
    assert b"member 0: no open stream batch" in lib.nww_last_error(members["gru"]._h)
    a = arr([lead, members["dnn"]])
    for bad in ([2, 1, 0], [1, 1, 3], [0, 1, S], [-1, 0, 1]):
        b = np.asarray(bad, np.int32)
        assert lib.nww_bank_stream_push_some(a, 2, b.ctypes.data_as(C.c_void_p), 3, chunk.ctypes.data_as(C.c_void_p), o[0], o[1]) == 1, bad
        assert b"strictly ascending" in lib.nww_last_error(lead._h)
        assert untouched() and [lead.stream_filled_of(s) for s in range(S)] == filled
    # n == 0: NWW_OK, nothing written; then a good call goes through and scores
    assert lib.nww_bank_stream_push_some(a, 2, None, 0, None, o[0], o[1]) == 0 and untouched()
    assert lib.nww_bank_stream_push_some(a, 2, ids.ctypes.data_as(C.c_void_p), 3, chunk.ctypes.data_as(C.c_void_p), o[0], o[1]) == 0
    assert out[1][:6].all() and (out[1][6:] == 7.0).all()
    assert [lead.stream_filled_of(s) for s in range(S)] == [f + hop * (s < 3) for s, f in enumerate(filled)]
    lead.stream_close()
    for m in (mel40, ulp, builtin, raw, loose, other):
        m.close()


# ---- 8. the Python layers above the bank, on real models
def test_interpreter_through_a_bank(golden_frontend, members):
    """load_model(bank=True) on HipSessions against bank=False on sessions of the same models: equal predict() traces, equal
    score_recording() output and state; a session with another frontend sends the interpreter back to the loop"""
    from nanowakeword_amd.interpreter import HipInterpreter
    from nanowakeword_amd.session import HipSession
    names, chunk = ["dnn", "cnn", "gru"], 320

    def sessions():
        return OrderedDict((n, HipSession(members[n], clip_samples=W, name=n)) for n in names)

    it, ref = HipInterpreter.load_model(sessions(), bank=True), HipInterpreter.load_model(sessions())
    assert [s.name for s in it.bank] == names and not ref.bank
    lead = it.models["dnn"]
    assert lead.bank_accepts(it.models["cnn"]) and not lead.bank_accepts(lead) and not lead.bank_accepts(HipSession(members["dnn"], clip_samples=W))
    x = _audio(4, W + 30 * chunk + 100, 88)
    pcm = np.ascontiguousarray(np.concatenate([x[2, :W], x[3, W:]]))
    thr = float(np.median(members["cnn"].forward_recording(pcm, window=W, hop=chunk)[1]))
    for kw in ({}, {"patience": {"cnn": 1}, "threshold": {"cnn": thr}}):
        it.reset(); ref.reset()
        for i in range(0, W + 12 * chunk, chunk):
            a, b = it.predict(pcm[i:i + chunk], **kw), ref.predict(pcm[i:i + chunk], **kw)
            assert a.scores == b.scores and it.raw_scores == ref.raw_scores, (i, a.scores, b.scores)
        assert all(v != 0 for v in it.raw_scores.values())
        got, want = it.score_recording(pcm, chunk_size=chunk, **kw), ref.score_recording(pcm, chunk_size=chunk, **kw)
        assert all(np.array_equal(got[n], want[n]) and (want[n] != 0).any() for n in names), kw
        assert {n: list(v) for n, v in it.prediction_buffer.items()} == {n: list(v) for n, v in ref.prediction_buffer.items()}
        assert it.raw_scores == ref.raw_scores and it.e2e_buffer_samples == ref.e2e_buffer_samples
    # a session with 40 mel bins: not accepted, and the interpreter scores model by model as before
    m40 = _model(HeadConfig("dnn", (T, 40)), golden_frontend, fe=FrontendConfig(n_mels=40), mel_fb=golden_frontend["fb40"])
    mixed = sessions()
    mixed["m40"] = HipSession(m40, clip_samples=W, name="m40")
    assert not lead.bank_accepts(mixed["m40"])
    loop = HipInterpreter.load_model(mixed, bank=True)
    assert not loop.bank
    got = loop.score_recording(pcm, chunk_size=chunk)
    plain = HipInterpreter.load_model(sessions()).score_recording(pcm, chunk_size=chunk)
    assert all(np.array_equal(got[n], plain[n]) for n in names) and (got["m40"] != 0).any()
    m40.close()


def test_bank_stream_pool_on_the_device(golden_frontend, members):
    """BankStreamPool on a real bank against one StreamPool per model on a twin with a batch of its own"""
    from nanowakeword_amd.interpreter import BankStreamPool, StreamPool
    hop, names, n_slots = 320, ["dnn", "cnn"], 4
    pool = BankStreamPool(_bank(members, names), n_slots, W, hop)
    twins = OrderedDict((n, _model(CFGS[n], golden_frontend)) for n in names)
    alone = {n: StreamPool(m, n_slots, W, hop, name=n) for n, m in twins.items()}
    ticks = W // hop + 9
    audio = _audio(n_slots, hop * ticks, 70)
    thr = {n: float(np.median(m.forward_pcm(np.ascontiguousarray(audio[:, -W:]))[1])) for n, m in twins.items()}
    cursor = np.zeros(n_slots, int)
    for s in range(n_slots):
        assert pool.attach() == s and all(p.attach() == s for p in alone.values())
    seen = {n: [] for n in names}
    for t in range(ticks):
        ids = [s for s in range(n_slots) if not (s == 2 and t < 3) and not (s == 1 and t % 4 == 2)]
        chunk = np.ascontiguousarray(np.stack([audio[s, cursor[s]:cursor[s] + hop] for s in ids]))
        cursor[ids] += hop
        got = pool.push(ids, chunk, patience={"cnn": 1}, threshold={"cnn": thr["cnn"]})
        for n, p in alone.items():
            want = p.push(ids, chunk, **({"patience": 1, "threshold": thr["cnn"]} if n == "cnn" else {}))
            assert np.array_equal(got[n], want), (t, n, got[n], want)
            assert np.array_equal(pool.raw_scores[n], p.raw_scores) and np.array_equal(pool.history[n], p.history) and np.array_equal(pool.count[n], p.count)
            seen[n].append(want)
    assert all((np.concatenate(v) != 0).any() for v in seen.values())
    pool.close()
    for p in alone.values():
        p.close()
    for m in twins.values():
        m.close()
