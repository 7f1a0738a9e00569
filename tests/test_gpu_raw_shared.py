"""The raw-PCM heads on the shared route (run with -m gpu): recordings whose windows share the rows of the learned frontend's last
stage, and streams that keep them in a ring.  The oracle is the library's own forward_pcm on the materialised windows,
through test_gpu_recording's _check; equality is np.array_equal on logits and probabilities.  Shapes are small on purpose: e2e_quartznet
(depth 3, total stride 256) at W = 4096 has T = 16 rows, el = 2, er = 1; at W = 4000 er = 2; e2e_cnn (depth 2, stride 64) at W = 4096 has
T = 64.  A hop shares rows when it is a multiple k of the stride with T - er - k > el."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nanowakeword_amd.config import HeadConfig, cascade_open, raw_frontend_frames
from nanowakeword_amd.synth import synth_state_dict
from test_gpu_recording import _check, _model, _oracle, _recording

pytestmark = pytest.mark.gpu

W = 4096


def _cfg(head, n, channels=32):
    depth = 3 if head == "e2e_quartznet" else 2
    cols = channels << (depth - 1)
    probe = HeadConfig(head, (1, cols), e2e_frontend_channels=channels)
    return HeadConfig(head, (raw_frontend_frames(probe, n), cols), e2e_frontend_channels=channels)


# ---- recordings
@pytest.mark.parametrize("channels", [16, 32])
def test_quartznet_hops_counts_and_passes(channels):
    m = _model(_cfg("e2e_quartznet", W, channels))
    assert m.clip_samples == W and "frontend:raw_x3:" in m.describe_plan()
    # k = 1 (maximum overlap), k = 5, and the largest hop that leaves an interior row to share: T - er - k = 16 - 1 - 12 = 3 > el = 2
    for hop in (256, 1280, 3072):
        _check(m, _recording(W + 6 * hop + 5, seed=hop), W, hop, 1, what=(channels, hop))
    assert m.recording_route(W, 3072 + 256) == 0
    _check(m, _recording(W + 3 * 3328, seed=1), W, 3328, 0, what=(channels, "one row too many"))
    seen = []
    for nW in (1, 2, 5, 33):
        pcm = _recording(W + (nW - 1) * 256 + 37, seed=nW)              # + a trailing partial hop
        seen.append(_check(m, pcm, W, 256, 1, what=(channels, nW)))
    assert len(set(np.concatenate(seen).tolist())) > 30                  # the windows really score differently
    pcm = _recording(W + 7 * 1280, seed=9)
    assert len(_check(m, pcm, W, 1280, 1, max_batch=3, what=(channels, "max_batch 3"))) == 8
    lg, _ = m.forward_recording(pcm, hop=1280, offset=8)                 # a PCM pointer that is 16 bytes off a 32-byte line
    assert np.array_equal(lg, _oracle(m, pcm, W, 1280, 8)[0]) and len(lg) == 7
    m.close()


def test_describe_and_poison():
    m = _model(_cfg("e2e_quartznet", W))
    text, plan = m.describe_recording(hop=1280), m.describe_plan()
    assert "raw_x3:pool" in text and "raw_x3:edge rows" in text and "rec_assemble:" in text and "strided" not in text, text
    assert text.strip().split("\n")[3:] == [l for l in plan.strip().split("\n") if not l.startswith("frontend:")]
    other = m.describe_recording(hop=1000)
    assert "strided route" in other and "rec_assemble" not in other and other.count("frontend:") == plan.count("frontend:") == 1, other
    # every row of the pool and of the dense head input is written by every pass: poison both, score again
    for hop, max_batch in ((1280, 4096), (256, 4)):
        pcm = _recording(W + 9 * hop, seed=hop + 1)
        first = _check(m, pcm, W, hop, 1, max_batch=max_batch, what=("before poison", hop))
        m.poison_recording_workspace(1e30)
        lg, pr = m.forward_recording(pcm, window=W, hop=hop, max_batch=max_batch)
        assert np.array_equal(lg, first) and np.isfinite(pr).all(), hop
    m.close()


def test_quartznet_window_4000():
    """W = 4000: 16 rows as at 4096, but the last TWO see the zero padding (er depends on W mod 256)"""
    m = _model(_cfg("e2e_quartznet", 4000))
    for hop in (256, 1280):
        _check(m, _recording(4000 + 8 * hop + 3, seed=hop), 4000, hop, 1, what=(4000, hop))
    _check(m, _recording(4000 + 8 * 256, seed=4), 4000, 256, 1, max_batch=4, what=(4000, "max_batch 4"))
    assert m.recording_route(4000, 11 * 256) == 1 and m.recording_route(4000, 12 * 256) == 0    # T - er - k > el: 16 - 2 - 11 = 3
    _check(m, _recording(4000 + 4 * 2816, seed=5), 4000, 2816, 1, what=(4000, "largest hop"))
    m.close()


def test_quartznet_at_the_real_shape():
    m = _model(_cfg("e2e_quartznet", 16000))
    assert m.head.input_shape == (63, 128)
    lg = _check(m, _recording(640 + 16000 + 19 * 1280, seed=3), 16000, 1280, 1, offset=640, what="real shape")
    assert len(lg) == 20
    m.close()


def test_cnn_head():
    m = _model(_cfg("e2e_cnn", W))
    assert m.head.input_shape == (64, 64) and "frontend:raw_x3:" in m.describe_plan()
    for hop in (64, 1280):
        _check(m, _recording(W + 9 * hop + 11, seed=hop), W, hop, 1, what=("e2e_cnn", hop))
        _check(m, _recording(W + 9 * hop, seed=hop + 1), W, hop, 1, max_batch=4, what=("e2e_cnn", hop, "max_batch 4"))
    _check(m, _recording(W + 4 * 1000, seed=2), W, 1000, 0, what=("e2e_cnn", "strided"))
    m.close()


def test_cnn_head_at_the_real_shape():
    m = _model(_cfg("e2e_cnn", 16000))
    assert m.head.input_shape == (250, 64)
    assert len(_check(m, _recording(16000 + 5 * 1280, seed=8), 16000, 1280, 1, what="e2e_cnn real shape")) == 6
    m.close()


def test_silence_and_full_scale_noise():
    """a recording that is digital silence for a stretch and full-scale noise for another, hop after hop"""
    m = _model(_cfg("e2e_quartznet", W))
    pcm = _recording(W + 20 * 256, seed=11)
    pcm[1000:1000 + 2 * W] = 0
    pcm[-W - 700:-300] = np.random.default_rng(3).integers(-32768, 32768, W + 400).astype(np.int16)
    lg = _check(m, pcm, W, 256, 1, what="silence and noise")
    assert len(set(lg.tolist())) > 10
    m.close()


CHILD = ("import sys, numpy as np\n"
         "from nanowakeword_amd.config import HeadConfig\n"
         "from nanowakeword_amd.config import FrontendConfig\n"
         "from nanowakeword_amd.session import HipModel\n"
         "from nanowakeword_amd.synth import synth_state_dict\n"
         "cfg = HeadConfig('e2e_quartznet', (16, 128)); m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))\n"
         "pcm = np.load(sys.argv[2])\n"
         "lg, pr = m.forward_recording(pcm[0], window=4096, hop=1280, max_batch=5)\n"
         "m.stream_open(pcm.shape[0], 4096, 1280)\n"
         "st = np.stack([m.stream_push(np.ascontiguousarray(pcm[:, t * 1280:(t + 1) * 1280]))[0] for t in range(8)])\n"
         "np.savez(sys.argv[1], route=np.array(m.recording_route(4096, 1280)), logits=lg, probs=pr, stream=st)\n"
         "m.close()\n")


def _child(tmp_path, pcm, **env):
    out = str(tmp_path / "child.npz")
    np.save(str(tmp_path / "pcm.npy"), pcm)
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]), **env)
    r = subprocess.run([sys.executable, "-c", CHILD, out, str(tmp_path / "pcm.npy")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(out, allow_pickle=False))


def _stream_run(m, audio, Wn, hop, pushes, reset_at=None):
    """push `pushes` hops of every stream; every full window's logits against forward_pcm on that stream's last Wn samples"""
    S = audio.shape[0]
    m.stream_open(S, Wn, hop)
    rows, t0 = [], 0
    for t in range(pushes):
        if t == reset_at:
            m.stream_reset()
            t0 = t
        lg, pr = m.stream_push(np.ascontiguousarray(audio[:, t * hop:(t + 1) * hop]))
        have = (t + 1 - t0) * hop
        if have < Wn:
            assert not lg.any() and not pr.any(), t
        else:
            want, want_p = m.forward_pcm(np.ascontiguousarray(audio[:, (t + 1) * hop - Wn:(t + 1) * hop]))
            assert np.array_equal(lg, want) and np.array_equal(pr, want_p), (t, lg, want)
        rows.append(lg)
    m.stream_close()
    return np.stack(rows)


def test_streams(tmp_path):
    S, hop = 3, 1280
    m = _model(_cfg("e2e_quartznet", W))
    audio = np.stack([_recording(12 * hop, seed=80 + s) for s in range(S)])
    got = _stream_run(m, audio, W, hop, 8)
    assert not got[:3].any() and len(set(got[3:].ravel().tolist())) > 2 * S          # a window after four hops; the scores differ
    _stream_run(m, audio, W, hop, 12, reset_at=6)                      # a reset mid-way: the next full window is computed whole
    _stream_run(m, audio, W, 256, 20)                                  # k = 1
    assert m.recording_route(W, 1000) == 0
    _stream_run(m, audio[:, :11000], W, 1000, 8)                       # no whole number of rows: every hop re-scores its window
    # the knobs off, in a fresh process: the strided route and whole-window hops, the same bits
    un = _child(tmp_path, audio[:, :8 * hop], NWW_REC_SHARED="0", NWW_STREAM_INC="0")
    assert int(un["route"]) == 0
    lg = _check(m, audio[0, :8 * hop], W, hop, 1, max_batch=5, what="knobs on")
    assert np.array_equal(un["logits"], lg) and np.array_equal(un["stream"], got)
    m.close()


def test_cnn_head_streams():
    m = _model(_cfg("e2e_cnn", W))
    audio = np.stack([_recording(9 * 1280, seed=90 + s) for s in range(2)])
    _stream_run(m, audio, W, 1280, 9)
    m.close()


# ---- a cascade whose gate is a raw-PCM head
def test_cascade_with_a_raw_gate():
    from nanowakeword_amd.session import HipCascade
    hop = 1280
    gate_cfg, ver_cfg = _cfg("e2e_cnn", W), _cfg("e2e_quartznet", W)
    cas = HipCascade(_model(gate_cfg), _model(ver_cfg))
    gate, ver = _model(gate_cfg), _model(ver_cfg)                       # the two models by hand
    assert cas.gate.recording_route(W, hop) == 1
    pcm = _recording(W + 10 * hop + 9, seed=17)
    wins = np.lib.stride_tricks.sliding_window_view(pcm, W)[::hop]
    gp = gate.forward_pcm(np.ascontiguousarray(wins))[1]
    thr = float(np.sort(gp)[-4])
    idx = np.flatnonzero(cascade_open(gp, thr))
    assert 0 < len(idx) < len(wins)
    want_l, want_p = np.full(len(wins), -np.inf, np.float32), np.zeros(len(wins), np.float32)
    want_l[idx], want_p[idx] = ver.forward_pcm(np.ascontiguousarray(wins[idx]))
    g, lg, pr, n_open = cas.forward_recording(pcm, window=W, hop=hop, gate_threshold=thr)
    assert n_open == len(idx) and np.array_equal(g, gp) and np.array_equal(lg, want_l) and np.array_equal(pr, want_p)
    # and as streams: the gate keeps its ring, the verifier sees the gathered windows
    S = 3
    audio = np.stack([_recording(7 * hop, seed=30 + s) for s in range(S)])
    cas.stream_open(S, W, hop)
    for t in range(7):
        out = cas.stream_push(np.ascontiguousarray(audio[:, t * hop:(t + 1) * hop]), gate_threshold=0.0)
        if (t + 1) * hop >= W:
            last = np.ascontiguousarray(audio[:, (t + 1) * hop - W:(t + 1) * hop])
            assert np.array_equal(out[0], gate.forward_pcm(last)[1]) and np.array_equal(out[1], ver.forward_pcm(last)[0]), t
    cas.stream_close()
    for m in (cas.gate, cas.verifier, gate, ver):
        m.close()
