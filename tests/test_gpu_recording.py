"""Recording scoring on the GPU (run with -m gpu): every window of one recording in a call, on the shared-frame route and on the strided
route.  The oracle is the library's own forward_pcm on sliding_window_view(pcm, W)[off::hop], scored in batches of the passes' sizes;
equality is np.array_equal on logits and probabilities.  Shapes are small on purpose: W = 3200 (T = 21), hop = 320 (k = 2 frames per
hop, el = er = 2 edge frames)."""
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from nanowakeword_amd.config import FrontendConfig, HeadConfig, raw_frontend_frames, recording_windows
from nanowakeword_amd.synth import synth_pcm, synth_state_dict

pytestmark = pytest.mark.gpu

W, HOP = 3200, 320


def _model(cfg, fe=None, g=None, **kw):
    from nanowakeword_amd.session import HipModel
    fe = fe or FrontendConfig()
    if g is not None:
        kw.update(window=g["window"], mel_fb=g["fb64"] if fe.n_mels == 64 else g["fb40"])
    return HipModel(cfg, fe, state_dict=synth_state_dict(cfg), **kw)


def _recording(n, seed=0):
    """speech-like audio with a stretch of noise and one of digital silence (-100 dB floor rows), so that neighbouring windows differ"""
    x = synth_pcm("speechlike", 1, n, seed=40 + seed)[0].copy()
    a = n // 3
    x[a:a + min(700, n - a)] = synth_pcm("loud", 1, 700, seed=seed)[0][:min(700, n - a)]
    x[n // 2:n // 2 + 900] = 0
    return x


def _oracle(m, pcm, window, hop, offset=0, max_batch=4096):
    """forward_pcm on the materialised windows, in batches of the passes' sizes"""
    wins = sliding_window_view(pcm, window)[offset::hop]
    lg, pr = [], []
    for i in range(0, len(wins), max_batch):
        a, b = m.forward_pcm(np.ascontiguousarray(wins[i:i + max_batch]))
        lg.append(a); pr.append(b)
    return np.concatenate(lg), np.concatenate(pr)


def _check(m, pcm, window, hop, route, offset=0, max_batch=4096, what=""):
    assert m.recording_route(window, hop) == route, (what, m.recording_route(window, hop))
    want, want_p = _oracle(m, pcm, window, hop, offset, max_batch)
    assert len(want) == recording_windows(len(pcm), window, hop, offset) > 0
    lg, pr = m.forward_recording(pcm, window=window, hop=hop, offset=offset, max_batch=max_batch)
    assert lg.shape == want.shape and np.isfinite(lg).all()
    assert np.array_equal(lg, want), (what, int((lg != want).sum()), float(np.abs(lg - want).max()))
    assert np.array_equal(pr, want_p), what
    return lg


# ---- the shared-frame route
@pytest.mark.parametrize("head", ["cnn", "dnn", "gru"])
def test_shared_route_window_counts_and_passes(golden_frontend, head):
    m = _model(HeadConfig(head, (21, 64)), g=golden_frontend)
    assert m.clip_samples == W and m.recording_route(hop=HOP) == 1
    seen = []
    for nW in (1, 2, 5, 33):
        pcm = _recording(W + (nW - 1) * HOP + 37, seed=nW)          # + a trailing partial hop
        seen.append(_check(m, pcm, W, HOP, 1, what=(head, nW)))
    assert len(set(np.concatenate(seen).tolist())) > 30              # the windows really score differently
    # passes of three windows over eight: two pass boundaries and a short last pass
    pcm = _recording(W + 7 * HOP, seed=9)
    a = _check(m, pcm, W, HOP, 1, max_batch=3, what=(head, "max_batch 3"))
    assert len(a) == 8
    # window defaults to the head's clip length; an offset moves the grid
    lg, _ = m.forward_recording(pcm, hop=HOP, offset=8)
    assert np.array_equal(lg, _oracle(m, pcm, W, HOP, 8)[0]) and len(lg) == 7
    # shorter than a window: nothing to score
    lg, pr = m.forward_recording(pcm[:W - 1], hop=HOP)
    assert lg.shape == pr.shape == (0,)
    # describe_recording names the route that ran, in front of the head's own launches
    text, plan = m.describe_recording(hop=HOP), m.describe_plan()
    assert "rec_assemble:" in text and "frontend:pool" in text and "frontend:edge frames" in text and "strided" not in text, text
    assert text.strip().split("\n")[3:] == [l for l in plan.strip().split("\n") if not l.startswith("frontend:")]
    other = m.describe_recording(hop=1000)
    assert "strided route" in other and "rec_assemble" not in other and other.count("frontend:") == plan.count("frontend:") >= 1, other
    m.close()


@pytest.mark.parametrize("hop,k", [(160, 1), (2560, 16)])
def test_shared_route_smallest_and_largest_hop(golden_frontend, hop, k):
    """k = 1: maximum overlap; k = 16: the largest hop that leaves an interior frame to share (T - er - k = 3 > el = 2)"""
    m = _model(HeadConfig("dnn", (21, 64)), g=golden_frontend)
    assert hop == k * 160 and m.recording_route(W, hop + 160) == (1 if k == 1 else 0)
    _check(m, _recording(W + 6 * hop, seed=k), W, hop, 1, what=hop)
    _check(m, _recording(W + 6 * hop, seed=k + 1), W, hop, 1, max_batch=2, what=(hop, "max_batch 2"))
    m.close()


def test_shared_route_at_the_real_shape(golden_frontend):
    m = _model(HeadConfig("cnn", (101, 64)), g=golden_frontend)
    pcm = _recording(640 + 16000 + 19 * 1280, seed=3)
    lg = _check(m, pcm, 16000, 1280, 1, offset=640, what="real shape")
    assert len(lg) == 20
    m.close()


@pytest.mark.parametrize("n_mels,center,rows", [(40, True, 21), (40, False, 18), (64, False, 18)])
def test_shared_route_other_frontends(golden_frontend, n_mels, center, rows):
    """a 40-mel filterbank; center=False has no reflect padding, so no window has edge frames at all"""
    fe = FrontendConfig(n_mels=n_mels, center=center)
    assert fe.n_frames(W) == rows
    m = _model(HeadConfig("dnn", (rows, n_mels)), fe, g=golden_frontend)
    _check(m, _recording(W + 9 * HOP, seed=n_mels + center), W, HOP, 1, what=(n_mels, center))
    _check(m, _recording(W + 9 * HOP, seed=n_mels), W, HOP, 1, max_batch=4, what=(n_mels, center, "max_batch 4"))
    m.close()


def test_e2e_dnn_is_bit_identical_on_its_route(golden_frontend):
    """the mel-major head: the shared route when its plan reads the frames-major plane, the strided route otherwise"""
    m = _model(HeadConfig("e2e_dnn", (64, 33)), g=golden_frontend)
    assert m.clip_samples == 5120
    route = m.recording_route(5120, HOP)
    assert route in (0, 1)
    print("e2e_dnn (64, 33): recording route", route)
    _check(m, _recording(5120 + 6 * HOP, seed=6), 5120, HOP, route, what="e2e_dnn")
    _check(m, _recording(5120 + 6 * HOP, seed=7), 5120, HOP, route, max_batch=4, what="e2e_dnn max_batch 4")
    m.close()


# ---- the strided route
@pytest.mark.parametrize("hop", [1000, W])
def test_strided_route_hops(golden_frontend, hop):
    """a hop that is no whole number of frames; hop == window (nothing overlaps)"""
    m = _model(HeadConfig("gru", (21, 64)), g=golden_frontend)
    _check(m, _recording(W + 4 * hop + 5, seed=hop), W, hop, 0, what=hop)
    _check(m, _recording(W + 4 * hop, seed=hop + 1), W, hop, 0, max_batch=2, what=(hop, "max_batch 2"))
    m.close()


def test_strided_route_raw_pcm_head():
    """e2e_quartznet at its smallest clip - 16 samples, one row - and at 4000 samples"""
    for n, hop in ((16, 8), (4000, 1000)):
        probe = HeadConfig("e2e_quartznet", (1, 128))
        cfg = HeadConfig("e2e_quartznet", (raw_frontend_frames(probe, n), 128))
        m = _model(cfg)
        pcm = _recording(n + 6 * hop, seed=n)
        _check(m, pcm, n, hop, 0, what=("e2e_quartznet", n))
        _check(m, pcm, n, hop, 0, max_batch=3, what=("e2e_quartznet", n, "max_batch 3"))
        m.close()


def test_knob_off_takes_the_strided_route(tmp_path):
    """NWW_REC_SHARED=0 (read once per process: a fresh interpreter): the strided route, the same bits as the shared one"""
    out = str(tmp_path / "strided.npz")
    pcm = _recording(W + 11 * HOP, seed=12)
    np.save(str(tmp_path / "pcm.npy"), pcm)
    code = ("import sys, numpy as np\n"
            "from nanowakeword_amd.config import FrontendConfig, HeadConfig\n"
            "from nanowakeword_amd.session import HipModel\n"
            "from nanowakeword_amd.synth import synth_state_dict\n"
            "cfg = HeadConfig('gru', (21, 64)); m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg), tables='builtin')\n"
            "lg, pr = m.forward_recording(np.load(sys.argv[2]), window=3200, hop=320, max_batch=5)\n"
            "np.savez(sys.argv[1], route=np.array(m.recording_route(3200, 320)), logits=lg, probs=pr)\n"
            "m.close()\n")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]), NWW_REC_SHARED="0")
    r = subprocess.run([sys.executable, "-c", code, out, str(tmp_path / "pcm.npy")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    un = dict(np.load(out, allow_pickle=False))
    assert int(un["route"]) == 0
    cfg = HeadConfig("gru", (21, 64))
    m = _model(cfg, tables="builtin")
    lg = _check(m, pcm, W, HOP, 1, max_batch=5, what="knob on")
    assert np.array_equal(un["logits"], lg) and np.array_equal(un["probs"], m.forward_recording(pcm, W, HOP, max_batch=5)[1])
    m.close()


# ---- errors
def test_errors(golden_frontend):
    m = _model(HeadConfig("dnn", (21, 64)), g=golden_frontend)
    pcm = _recording(8000)
    with pytest.raises(ValueError, match="multiples of 8"):
        m.forward_recording(pcm, window=W, hop=12)
    with pytest.raises(ValueError, match="multiples of 8"):
        m.recording_route(W, W + 8)                                  # hop > window
    with pytest.raises(ValueError, match=r"a 4800-sample window gives \(31,64\) features but the head expects \(21,64\)"):
        m.forward_recording(pcm, window=4800, hop=HOP)
    with pytest.raises(ValueError, match="features but the head expects"):
        m.recording_route(4800, HOP)
    with pytest.raises(ValueError):
        m.forward_recording(pcm.astype(np.float32), hop=HOP)
    with pytest.raises(ValueError):
        m.forward_recording(pcm[None], hop=HOP)
    with pytest.raises(ValueError):
        m.forward_recording(pcm, hop=HOP, offset=-8)
    lg, _ = m.forward_recording(pcm, hop=HOP)                        # the handle still works after the refusals
    assert np.array_equal(lg, _oracle(m, pcm, W, HOP)[0])
    m.close()


# ---- several recordings in one call
def test_recordings_in_a_batch(golden_frontend):
    m = _model(HeadConfig("gru", (21, 64)), g=golden_frontend)
    recs = [_recording(n, seed=n) for n in (W + 5 * HOP + 11, W, 2 * W + 3 * HOP + 300)] + [_recording(W - 1, seed=2)]
    got = m.forward_recordings(recs, hop=HOP)
    assert [len(a) for a, _ in got] == [6, 1, 14, 0]
    for r, (lg, pr) in zip(recs, got):
        alone, alone_p = m.forward_recording(r, hop=HOP)
        assert np.array_equal(lg, alone) and np.array_equal(pr, alone_p), len(r)
    m.close()


# ---- the interpreter
def test_interpreter_score_recording(tmp_path):
    from nanowakeword_amd.interpreter import HipInterpreter
    from nanowakeword_amd.weights import save_bundle
    cfg = HeadConfig("cnn", (101, 64))
    path = str(tmp_path / "kw.nww.npz")
    save_bundle(path, cfg, synth_state_dict(cfg), mode="e2e", clip_samples=16000)
    pcm = _recording(48000, seed=5)
    ref = HipInterpreter.load_model(path)
    want = np.array([ref.predict(pcm[i:i + 1280]).scores["kw"] for i in range(0, len(pcm), 1280)], np.float32)
    it = HipInterpreter.load_model(path)
    assert it.models["kw"].model.recording_route(16000, 1280) == 1
    got = it.score_recording(pcm)["kw"]
    assert not want[:12].any() and want[12:].all() and len(want) == 38
    assert np.array_equal(got, want), (int((got != want).sum()), float(np.abs(got - want).max()))
    assert list(it.prediction_buffer["kw"]) == list(ref.prediction_buffer["kw"])
    kw = dict(patience={"kw": 1}, threshold={"kw": float(np.median(want[12:]))})
    ref.reset()
    want_f = np.array([ref.predict(pcm[i:i + 1280], **kw).scores["kw"] for i in range(0, len(pcm), 1280)], np.float32)
    assert np.array_equal(it.score_recording(pcm, **kw)["kw"], want_f) and (want_f != 0).any()


# ---- device pointers
def test_device_variant_equals_host_variant(golden_frontend):
    torch = pytest.importorskip("torch")
    m = _model(HeadConfig("cnn", (21, 64)), g=golden_frontend)
    pcm = _recording(8 + W + 12 * HOP, seed=21)
    want, want_p = m.forward_recording(pcm, hop=HOP, offset=8, max_batch=5)
    d = torch.from_numpy(pcm).cuda()
    lg = torch.full((len(want) + 1,), -7.0, device="cuda"); pr = torch.full((len(want) + 1,), -7.0, device="cuda")
    torch.cuda.synchronize()                                              # the library enqueues on its own stream
    n = m.forward_recording_dev(d.data_ptr() + 2 * 8, len(pcm) - 8, W, HOP, lg.data_ptr(), pr.data_ptr(), max_batch=5)
    torch.cuda.synchronize()
    assert n == len(want) == 13
    assert np.array_equal(lg.cpu().numpy()[:n], want) and np.array_equal(pr.cpu().numpy()[:n], want_p)
    assert lg[n].item() == -7.0 and pr[n].item() == -7.0                  # nothing written behind the last window
    assert m.forward_recording_dev(d.data_ptr(), W - 8, W, HOP, lg.data_ptr()) == 0
    with pytest.raises(ValueError):
        m.forward_recording_dev(d.data_ptr(), len(pcm), W, 12, lg.data_ptr())
    m.close()
