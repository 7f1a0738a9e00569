"""Gate + verifier cascades on the GPU (run with -m gpu): the verifier runs on the windows the gate opens, for a batch of clips, every
window of a recording and S lock-step streams.  The oracle is the library itself: the gate handle alone for the gate's probabilities,
config.cascade_open for the open set, verifier.forward_pcm on the open windows stacked in ascending order (in chunks of max_batch), and
0.0 / -inf elsewhere; equality is np.array_equal throughout.  Every threshold is taken from the gate's own probabilities on the test's
input (the gate scored alone first), so every open set is known exactly.  Shapes are small on purpose: W = 3200 (T = 21), hop = 320."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from nanowakeword_amd.config import FrontendConfig, HeadConfig, cascade_open, raw_frontend_frames, recording_windows
from nanowakeword_amd.synth import synth_pcm, synth_state_dict

pytestmark = pytest.mark.gpu

W, HOP = 3200, 320
NEG_INF = np.float32(-np.inf)


def _model(cfg, fe=None, g=None, **kw):
    from nanowakeword_amd.session import HipModel
    fe = fe or FrontendConfig()
    if g is not None:
        kw.update(window=g["window"], mel_fb=g["fb64"] if fe.n_mels == 64 else g["fb40"])
    return HipModel(cfg, fe, state_dict=synth_state_dict(cfg), **kw)


def _cascade(gate_cfg, ver_cfg, g=None, ver_fe=None):
    from nanowakeword_amd.session import HipCascade
    return HipCascade(_model(gate_cfg, g=g), _model(ver_cfg, ver_fe, g=g))


def _close(cas):
    cas.gate.close()
    cas.verifier.close()


def _recording(n, seed=0):
    """speech-like audio with a stretch of noise and one of digital silence, so that neighbouring windows differ"""
    x = synth_pcm("speechlike", 1, n, seed=40 + seed)[0].copy()
    a = n // 3
    x[a:a + min(700, n - a)] = synth_pcm("loud", 1, 700, seed=seed)[0][:min(700, n - a)]
    x[n // 2:n // 2 + 900] = 0
    return x


def _launches(m):
    return sum(c for _, _, c in m.get_profile())


def _kth_largest(p, k):
    """the threshold that opens exactly the k largest probabilities (when they are distinct)"""
    return float(np.sort(p)[-k])


def _above(p):
    """the smallest double above every probability: nothing opens"""
    return float(np.nextafter(np.float64(p.max()), np.inf))


def _check_recording(cas, pcm, window, hop, thr, gate_probs, offset=0, max_batch=4096, what=""):
    """one cascade call against the oracle; gate_probs: the gate handle alone on the same input and pass sizes"""
    wins = sliding_window_view(pcm, window)[offset::hop]
    n = len(wins)
    assert n == recording_windows(len(pcm), window, hop, offset) == len(gate_probs) > 0
    idx = np.flatnonzero(cascade_open(gate_probs, thr))
    want_l, want_p = np.full(n, NEG_INF, np.float32), np.zeros(n, np.float32)
    for i in range(0, len(idx), max_batch):
        part = idx[i:i + max_batch]
        want_l[part], want_p[part] = cas.verifier.forward_pcm(np.ascontiguousarray(wins[part]))
    gp, lg, pr, n_open = cas.forward_recording(pcm, window=window, hop=hop, offset=offset, max_batch=max_batch, gate_threshold=thr)
    print(what, "thr", thr, "open", n_open, "of", n)
    assert gp.dtype == lg.dtype == pr.dtype == np.float32 and gp.shape == lg.shape == pr.shape == (n,)
    assert np.array_equal(gp, gate_probs), what
    assert n_open == len(idx), (what, n_open, len(idx))
    assert np.array_equal(lg, want_l), (what, lg, want_l)
    assert np.array_equal(pr, want_p), (what, pr, want_p)
    closed = np.ones(n, bool); closed[idx] = False
    assert (lg[closed] == NEG_INF).all() and (pr[closed] == 0.0).all() and np.isfinite(lg[idx]).all()
    return idx, pr


def _gate_probs(cas, pcm, window, hop, offset=0, max_batch=4096):
    return cas.gate.forward_recording(pcm, window=window, hop=hop, offset=offset, max_batch=max_batch)[1]


# ---- the select alone
def _patterns(n, rng):
    closed, open_ = np.float32(0.25), np.float32(0.75)
    none, every = np.full(n, closed), np.full(n, open_)
    other = none.copy(); other[::2] = open_
    first = none.copy(); first[0] = open_
    last = none.copy(); last[-1] = open_
    rand = rng.random(n).astype(np.float32) * np.float32(0.5)
    rand[rng.random(n) < 0.05] = open_
    nans = rand.copy(); nans[[0, n // 2]] = np.nan
    return dict(none=none, all=every, every_other=other, first=first, last=last, random=rand, nans=nans)


@pytest.fixture(scope="module")
def small_cascade():
    cas = _cascade(HeadConfig("dnn", (21, 64), layer_dim=32), HeadConfig("dnn", (21, 64), layer_dim=32), None)
    yield cas
    _close(cas)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1025, 100003])
def test_select_alone(small_cascade, n):
    cas = small_cascade
    rng = np.random.default_rng(n)
    for name, p in _patterns(n, rng).items():
        want = np.flatnonzero(cascade_open(p, 0.5)).astype(np.int32)
        got = cas.select(p, 0.5)
        assert got.dtype == np.int32 and len(got) == len(want), (n, name, len(got), len(want))
        assert np.array_equal(got, want), (n, name)
    p = rng.random(n).astype(np.float32)
    thr = float(p[n // 2])                                      # equal to one score: that one is open
    got = cas.select(p, thr)
    assert np.array_equal(got, np.flatnonzero(cascade_open(p, thr))) and n // 2 in got
    assert len(cas.select(p, 0.0)) == n and len(cas.select(p, 2.0)) == 0 and len(cas.select(p)) == int((p.astype(np.float64) >= 0.3).sum())


# ---- recordings
def _verifiers():
    return {"cnn": (HeadConfig("cnn", (21, 64)), None), "gru": (HeadConfig("gru", (21, 64)), None),
            "dnn40": (HeadConfig("dnn", (21, 40)), FrontendConfig(n_mels=40))}


@pytest.mark.parametrize("ver", ["cnn", "gru", "dnn40"])
def test_recording(golden_frontend, ver):
    cfg, fe = _verifiers()[ver]
    cas = _cascade(HeadConfig("dnn", (21, 64), layer_dim=32), cfg, golden_frontend, fe)
    assert cas.clip_samples == W
    mixed = []
    for nW in (1, 2, 33):
        pcm = _recording(W + (nW - 1) * HOP + 37, seed=nW)              # + a trailing partial hop
        gp = _gate_probs(cas, pcm, W, HOP)
        assert len(gp) == nW
        idx, _ = _check_recording(cas, pcm, W, HOP, _above(gp), gp, what=(ver, nW, "none"))
        assert len(idx) == 0
        idx, _ = _check_recording(cas, pcm, W, HOP, float(gp.min()), gp, what=(ver, nW, "all"))
        assert len(idx) == nW
        idx, _ = _check_recording(cas, pcm, W, HOP, float(gp[nW // 2]), gp, what=(ver, nW, "equal"))
        assert nW // 2 in idx                                            # a threshold equal to a window's own probability opens it
        if nW == 33:
            assert len(set(gp.tolist())) == nW                          # distinct scores: the thresholds below open exactly what they say
            idx, pr = _check_recording(cas, pcm, W, HOP, _kth_largest(gp, 11), gp, what=(ver, nW, "a third"))
            assert len(idx) == 11 and len(set(pr[idx].tolist())) > 1
            mixed.append(idx)
            # exactly one window open: the gate's best one, as the first, the last and a middle window of a recording cut around it
            m = int(np.argmax(gp))
            lo, hi = max(m - 4, 0), min(m + 4, nW - 1)
            for what, a, b in (("first", m, hi), ("last", lo, m), ("middle", lo, hi)):
                cut = pcm[a * HOP:b * HOP + W]
                g = _gate_probs(cas, cut, W, HOP)
                assert int(np.argmax(g)) == m - a and len(g) == b - a + 1
                idx, _ = _check_recording(cas, cut, W, HOP, float(g.max()), g, what=(ver, "one open", what))
                assert idx.tolist() == [m - a]
    assert len(mixed) == 1 and 0 < len(mixed[0]) < 33
    # passes and chunks of three over eight windows, 4 to 7 of them open: survivors straddle the gate's passes and the verifier's chunks
    pcm = _recording(W + 7 * HOP, seed=9)
    gp = _gate_probs(cas, pcm, W, HOP, max_batch=3)
    assert len(set(gp.tolist())) == 8
    for k in (4, 5, 6, 7):
        idx, pr = _check_recording(cas, pcm, W, HOP, _kth_largest(gp, k), gp, max_batch=3, what=(ver, "max_batch 3", k))
        assert len(idx) == k and len(set(pr[idx].tolist())) > 1
    # an offset moves the grid
    gp = _gate_probs(cas, pcm, W, HOP, offset=8)
    idx, _ = _check_recording(cas, pcm, W, HOP, _kth_largest(gp, 3), gp, offset=8, what=(ver, "offset 8"))
    assert len(gp) == 7 and 0 < len(idx) < 7
    # shorter than a window: nothing to score
    out = cas.forward_recording(pcm[:W - 1], hop=HOP)
    assert out[0].shape == out[1].shape == out[2].shape == (0,) and out[3] == 0
    text = cas.describe().strip().split("\n")
    g, v = cas.gate.describe_plan().strip().split("\n"), cas.verifier.describe_plan().strip().split("\n")
    assert text[:len(g)] == g and text[len(g)].startswith("cascade_select:") and text[len(g) + 1].startswith("cascade_gather:")
    assert text[len(g) + 2:-1] == v and text[-1].startswith("cascade_scatter:")
    _close(cas)


def test_no_verifier_launch_when_nothing_opens(golden_frontend):
    cas = _cascade(HeadConfig("dnn", (21, 64), layer_dim=32), HeadConfig("gru", (21, 64)), golden_frontend)
    pcm = _recording(W + 8 * HOP, seed=2)
    gp = _gate_probs(cas, pcm, W, HOP)
    cas.verifier.set_profiling(True)
    _, lg, pr, n_open = cas.forward_recording(pcm, hop=HOP, gate_threshold=_above(gp))
    assert n_open == 0 and (lg == NEG_INF).all() and not pr.any()
    _, lg, pr, n_open = cas.forward_pcm(np.ascontiguousarray(sliding_window_view(pcm, W)[::HOP]), gate_threshold=2.0)
    assert n_open == 0 and (lg == NEG_INF).all() and not pr.any()
    assert _launches(cas.verifier) == 0
    assert cas.forward_recording(pcm, hop=HOP, gate_threshold=float(gp.max()))[3] == 1
    assert _launches(cas.verifier) > 0                                   # the profile does count a verifier run
    cas.verifier.set_profiling(False)
    _close(cas)


def test_recording_raw_pcm_verifier_behind_a_mel_gate(golden_frontend):
    """e2e_quartznet at a 4000-sample window, hop 1000: a raw-PCM verifier, and a hop that is no whole number of frames"""
    n, hop = 4000, 1000
    probe = HeadConfig("e2e_quartznet", (1, 128))
    ver = HeadConfig("e2e_quartznet", (raw_frontend_frames(probe, n), 128))
    cas = _cascade(HeadConfig("dnn", (26, 64), layer_dim=32), ver, golden_frontend)
    pcm = _recording(n + 8 * hop + 5, seed=n)
    gp = _gate_probs(cas, pcm, n, hop, max_batch=4)
    assert len(set(gp.tolist())) == 9
    for k, what in ((9, "all"), (4, "mixed"), (1, "one")):
        idx, pr = _check_recording(cas, pcm, n, hop, _kth_largest(gp, k), gp, max_batch=4, what=("e2e_quartznet", what))
        assert len(idx) == k
    assert len(_check_recording(cas, pcm, n, hop, _above(gp), gp, max_batch=4, what=("e2e_quartznet", "none"))[0]) == 0
    _close(cas)


def test_recording_at_the_real_shape(golden_frontend):
    cas = _cascade(HeadConfig("e2e_dnn", (64, 101)), HeadConfig("cnn", (101, 64)), golden_frontend)
    assert cas.clip_samples == 16000
    pcm = _recording(640 + 16000 + 19 * 1280, seed=3)
    gp = _gate_probs(cas, pcm, 16000, 1280, offset=640)
    assert len(gp) == 20 and len(set(gp.tolist())) == 20
    idx, pr = _check_recording(cas, pcm, 16000, 1280, _kth_largest(gp, 10), gp, offset=640, what="real shape")
    assert len(idx) == 10 and len(set(pr[idx].tolist())) > 1
    _close(cas)


# ---- a batch of clips
@pytest.mark.parametrize("N", [3200, 3201])
def test_batch_entry(golden_frontend, N):
    """N = 3201: every clip but the first starts at an odd 2-byte offset - the gather's 2-byte path (T is still 21)"""
    cas = _cascade(HeadConfig("dnn", (21, 64), layer_dim=32), HeadConfig("gru", (21, 64)), golden_frontend)
    pcm = _recording(N + 32 * 330, seed=N)
    for B in (1, 17, 33):
        clips = np.ascontiguousarray(sliding_window_view(pcm, N)[::330][:B])
        assert clips.shape == (B, N)
        gate_p = cas.gate.forward_pcm(clips)[1]
        for what, thr in (("none", _above(gate_p)), ("all", float(gate_p.min())), ("mixed", float(np.sort(gate_p)[B // 2]))):
            idx = np.flatnonzero(cascade_open(gate_p, thr))
            want_l, want_p = np.full(B, NEG_INF, np.float32), np.zeros(B, np.float32)
            if len(idx):
                want_l[idx], want_p[idx] = cas.verifier.forward_pcm(np.ascontiguousarray(clips[idx]))
            gp, lg, pr, n_open = cas.forward_pcm(clips, gate_threshold=thr)
            print(N, B, what, "open", n_open)
            assert np.array_equal(gp, gate_p) and n_open == len(idx), (N, B, what)
            assert np.array_equal(lg, want_l) and np.array_equal(pr, want_p), (N, B, what)
            if what == "mixed" and B > 1:
                assert 0 < n_open < B and len(set(pr[idx].tolist())) > 1
    _close(cas)


# ---- S lock-step streams
def test_streams(golden_frontend):
    from nanowakeword_amd.session import HipCascade
    S = 5
    gate_cfg, ver_cfg = HeadConfig("cnn", (21, 64)), HeadConfig("gru", (21, 64))
    cas = _cascade(gate_cfg, ver_cfg, golden_frontend)
    alone = _model(gate_cfg, g=golden_frontend)                           # a second gate handle: the gate's own stream_push
    cas.stream_open(S, hop_samples=HOP)
    alone.stream_open(S, W, HOP)
    audio = np.stack([_recording(W + 6 * HOP, seed=60 + s) for s in range(S)])

    def run(first_thr):
        cas.verifier.set_profiling(True)
        for t in range(W // HOP + 2):
            chunk = np.ascontiguousarray(audio[:, t * HOP:(t + 1) * HOP])
            _, g_pr = alone.stream_push(chunk)
            full = (t + 1) * HOP >= W
            thr = ([first_thr(g_pr), 2.0, 0.0][t - (W // HOP - 1)]) if full else 0.0
            gp, lg, pr, n_open = cas.stream_push(chunk, gate_threshold=thr)
            assert np.array_equal(gp, g_pr), t
            if not full:                                                   # the ring holds no window yet: zeros, the verifier not run
                assert not gp.any() and not lg.any() and not pr.any() and n_open == 0
                if t == W // HOP - 2:
                    assert _launches(cas.verifier) == 0
                    cas.verifier.set_profiling(False)
                continue
            wins = np.ascontiguousarray(audio[:, (t + 1) * HOP - W:(t + 1) * HOP])
            idx = np.flatnonzero(cascade_open(g_pr, thr))
            want_l, want_p = np.full(S, NEG_INF, np.float32), np.zeros(S, np.float32)
            if len(idx):
                want_l[idx], want_p[idx] = cas.verifier.forward_pcm(wins[idx])
            print("push", t, "thr", thr, "open", n_open)
            assert n_open == len(idx) and np.array_equal(lg, want_l) and np.array_equal(pr, want_p), t
            if t == W // HOP - 1:
                assert 0 < n_open < S
        assert cas.stream_filled() == W + 2 * HOP

    run(lambda p: float(np.sort(p)[S // 2]))
    cas.stream_reset(); alone.stream_reset()                              # starts over
    run(lambda p: float(np.sort(p)[1]))
    cas.stream_close(); alone.stream_close()
    alone.close()
    _close(cas)


@pytest.mark.parametrize("filt", [{}, {"patience": {"kw": 1}}], ids=["plain", "patience"])
def test_cascade_stream_batch_equals_interpreters(golden_frontend, filt):
    from nanowakeword_amd.interpreter import CascadeStreamBatch, HipInterpreter
    from nanowakeword_amd.session import HipSession
    S, pushes = 4, W // HOP + 6
    cas = _cascade(HeadConfig("cnn", (21, 64)), HeadConfig("gru", (21, 64)), golden_frontend)
    gate2, ver2 = _model(HeadConfig("cnn", (21, 64)), g=golden_frontend), _model(HeadConfig("gru", (21, 64)), g=golden_frontend)
    audio = np.stack([_recording(pushes * HOP, seed=70 + s) for s in range(S)])
    last = np.ascontiguousarray(audio[:, -W:])
    cas.gate_threshold = float(np.median(gate2.forward_pcm(last)[1]))     # from the gate's own scores: some streams open, some closed
    kw = dict(filt)
    if filt:
        kw["threshold"] = {"kw": float(np.median(ver2.forward_pcm(last)[1]))}
    its = []
    for s in range(S):
        it = HipInterpreter({"lite": HipSession(gate2, clip_samples=W, name="lite"), "kw": HipSession(ver2, clip_samples=W, name="kw")})
        it.cascade_config = {"gate": "lite", "verifier": "kw", "gate_threshold": cas.gate_threshold}
        its.append(it)
    sb = CascadeStreamBatch(cas, S, W, HOP, gate_name="lite", name="kw")
    seen = {"lite": [], "kw": []}
    for t in range(pushes):
        chunk = np.ascontiguousarray(audio[:, t * HOP:(t + 1) * HOP])
        got = sb.push(chunk, **kw)
        want = [its[s].predict(chunk[s], **kw).scores for s in range(S)]            # one predict() per stream scores both models
        for name in ("lite", "kw"):
            assert np.array_equal(got[name], np.array([w[name] for w in want], np.float32)), (t, name)
            assert np.array_equal(sb.raw_scores[name], np.array([its[s].raw_scores[name] for s in range(S)], np.float32)), (t, name)
            seen[name].append(got[name])
    assert np.stack(seen["lite"])[W // HOP - 1:].all() and np.stack(seen["kw"]).any()
    closed = np.stack(seen["kw"])[W // HOP - 1:] == 0
    assert closed.any() and not closed.all()                              # the gate closed some and opened some
    sb.close()
    gate2.close(); ver2.close()
    _close(cas)


# ---- device pointers
def test_device_variant_equals_host_variant(golden_frontend):
    torch = pytest.importorskip("torch")
    cas = _cascade(HeadConfig("dnn", (21, 64), layer_dim=32), HeadConfig("cnn", (21, 64)), golden_frontend)
    pcm = _recording(8 + W + 12 * HOP, seed=21)
    gate_p = _gate_probs(cas, pcm, W, HOP, offset=8, max_batch=5)
    thr = _kth_largest(gate_p, 6)
    gp, lg, pr, n_open = cas.forward_recording(pcm, hop=HOP, offset=8, max_batch=5, gate_threshold=thr)
    assert len(gp) == 13 and n_open == 6
    d = torch.from_numpy(pcm).cuda()
    out = [torch.full((14,), -7.0, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()                                              # the library enqueues on its own stream
    nw, n_dev = cas.forward_recording_dev(d.data_ptr() + 2 * 8, len(pcm) - 8, W, HOP, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                          max_batch=5, gate_threshold=thr)
    torch.cuda.synchronize()
    assert (nw, n_dev) == (13, 6)
    for t, want in zip(out, (gp, lg, pr)):
        assert np.array_equal(t.cpu().numpy()[:13], want) and t[13].item() == -7.0     # nothing written behind the last window
    # a batch of clips through device pointers
    clips = torch.from_numpy(np.ascontiguousarray(sliding_window_view(pcm, W)[8::HOP])).cuda()
    out = [torch.full((14,), -7.0, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    assert cas.forward_pcm_dev(clips.data_ptr(), 13, W, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), gate_threshold=thr) == 6
    torch.cuda.synchronize()
    want = cas.forward_pcm(clips.cpu().numpy(), gate_threshold=thr)
    for t, w in zip(out, want[:3]):
        assert np.array_equal(t.cpu().numpy()[:13], w) and t[13].item() == -7.0
    assert cas.forward_recording_dev(d.data_ptr(), W - 8, W, HOP, out[0].data_ptr(), out[1].data_ptr()) == (0, 0)
    _close(cas)


# ---- the interpreter
def test_interpreter_score_recording_of_a_cascade(tmp_path):
    from nanowakeword_amd.interpreter import HipInterpreter
    from nanowakeword_amd.weights import save_bundle
    main, lite = HeadConfig("cnn", (101, 64)), HeadConfig("dnn", (101, 64), layer_dim=32)
    path, gate_path = str(tmp_path / "kw.nww.npz"), str(tmp_path / "kw_lite.nww.npz")
    save_bundle(path, main, synth_state_dict(main), mode="e2e", clip_samples=16000)
    save_bundle(gate_path, lite, synth_state_dict(lite), mode="e2e", clip_samples=16000)
    pcm = _recording(48000, seed=5)
    gate_scores = HipInterpreter.load_model(gate_path).score_recording(pcm)["kw_lite"]
    thr = float(np.median(gate_scores[12:]))
    ref = HipInterpreter.load_model(path, cascade=True, gate_threshold=thr)
    assert ref.is_cascade and list(ref.models) == ["kw_lite", "kw"]

    def loop(**kw):
        ref.reset()
        out = [ref.predict(pcm[i:i + 1280], **kw).scores for i in range(0, len(pcm), 1280)]
        return {n: np.array([d[n] for d in out], np.float32) for n in ref.models}

    want = loop()
    it = HipInterpreter.load_model(path, cascade=True, gate_threshold=thr)
    got = it.score_recording(pcm)
    for name in ("kw_lite", "kw"):
        assert np.array_equal(got[name], want[name]), (name, int((got[name] != want[name]).sum()))
        assert list(it.prediction_buffer[name]) == list(ref.prediction_buffer[name])
    assert np.array_equal(want["kw_lite"], gate_scores) and len(want["kw"]) == 38
    open_ = want["kw"][12:] != 0
    assert open_.any() and not open_.all() and np.array_equal(open_, cascade_open(want["kw_lite"][12:], thr))
    # the verifier was asked for fewer windows than there are
    windows, n_open = it.models["kw"].last_cascade                       # 37 full chunks, the 13th fills the window; the 38th is short
    assert windows == 25 and n_open == int(open_[:25].sum()) < windows
    kw = dict(patience={"kw": 1}, threshold={"kw": float(np.median(want["kw"][12:][open_]))})
    want_f = loop(**kw)
    got_f = it.score_recording(pcm, **kw)
    assert all(np.array_equal(got_f[n], want_f[n]) for n in ("kw_lite", "kw")) and (want_f["kw"] != 0).any()


# ---- errors
def test_errors(golden_frontend):
    from nanowakeword_amd.session import HipCascade
    cas = _cascade(HeadConfig("dnn", (21, 64), layer_dim=32), HeadConfig("gru", (31, 64)), golden_frontend)
    gate, ver = cas.gate, cas.verifier
    pcm = _recording(8000)
    with pytest.raises(ValueError, match="distinct"):
        HipCascade(gate, gate)
    lib, n_open = gate.lib, np.zeros(1, np.int32)
    out = np.zeros(3 * 64, np.float32)
    rc = lib.nww_cascade_forward_pcm(gate._h, gate._h, pcm.ctypes.data, 1, W, 0.5, out.ctypes.data, out.ctypes.data, out.ctypes.data, None)
    assert rc == 1 and "distinct" in lib.nww_last_error(gate._h).decode()          # NWW_ERR_INVALID
    with pytest.raises(ValueError, match="pass `window`"):
        cas.clip_samples
    # a window that fits the gate but not the verifier, and the other way round
    with pytest.raises(ValueError, match=r"verifier: a 3200-sample window gives \(21,64\) features but the head expects \(31,64\)"):
        cas.forward_recording(pcm, window=W, hop=HOP)
    with pytest.raises(ValueError, match=r"gate: a 4800-sample window gives \(31,64\) features but the head expects \(21,64\)"):
        cas.forward_recording(pcm, window=4800, hop=HOP)
    with pytest.raises(ValueError, match=r"verifier: frontend yields \(21,64\) features for 3200 samples"):
        cas.forward_pcm(pcm[None, :W])
    cas.stream_open(2, W, HOP)
    with pytest.raises(ValueError, match="verifier: frontend yields"):
        cas.stream_push(np.zeros((2, HOP), np.int16))
    cas.stream_close()
    with pytest.raises(RuntimeError, match="no open stream batch"):
        cas.stream_push_dev(1, 0, 0)
    with pytest.raises(ValueError, match="multiples of 8"):
        cas.forward_recording(pcm, window=W, hop=12)
    with pytest.raises(ValueError):
        cas.forward_recording(pcm.astype(np.float32), window=W, hop=HOP)
    with pytest.raises(ValueError):
        cas.forward_recording(pcm, window=W, hop=HOP, offset=-8)
    # both handles still work afterwards
    wins = np.ascontiguousarray(sliding_window_view(pcm, W)[::HOP])
    assert np.array_equal(gate.forward_recording(pcm, hop=HOP)[1], gate.forward_pcm(wins)[1])
    wins = np.ascontiguousarray(sliding_window_view(pcm, 4800)[::HOP])
    assert np.array_equal(ver.forward_recording(pcm, hop=HOP)[0], ver.forward_pcm(wins)[0])
    _close(cas)
