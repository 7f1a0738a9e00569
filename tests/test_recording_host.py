"""Recording scoring, host side (no GPU): the window count law, the four C-ABI symbols in the header and the binding, the bookkeeping of
several recordings scored as one (a stub model that hashes each window), and HipInterpreter.score_recording against the predict() chunk
loop on a stub session."""
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT
from nanowakeword_amd import _lib
from nanowakeword_amd.config import FrontendConfig, HeadConfig, clip_samples, recording_windows
from nanowakeword_amd.interpreter import HipInterpreter
from nanowakeword_amd.session import score_recordings
from nanowakeword_amd.synth import synth_pcm

REC_SYMBOLS = ["nww_recording_windows", "nww_recording_route", "nww_forward_recording_dev", "nww_forward_recording"]


def test_recording_windows_law():
    W, hop = 16000, 1280
    assert recording_windows(W - 1, W, hop) == 0 and recording_windows(0, W, hop) == 0
    assert recording_windows(W, W, hop) == 1
    assert recording_windows(W + hop - 1, W, hop) == 1          # a trailing partial hop is ignored
    assert recording_windows(W + hop, W, hop) == 2
    assert recording_windows(48000, W, hop) == 26 and recording_windows(48000, W, hop, offset=640) == 25
    assert recording_windows(W + 640, W, hop, offset=640) == 1 and recording_windows(W + 639, W, hop, offset=640) == 0
    assert recording_windows(100, W, hop, offset=200) == 0      # an offset behind the end
    for n, w, h, off in ((5000, 3200, 320, 0), (5000, 3200, 320, 8), (3200, 3200, 3200, 0), (9999, 3200, 1000, 3)):
        want = len(range(off, n - w + 1, h))
        assert recording_windows(n, w, h, off) == want, (n, w, h, off)
    with pytest.raises(ValueError):
        recording_windows(100, 0, 8)
    with pytest.raises(ValueError):
        recording_windows(100, 8, 8, offset=-1)


def test_clip_samples_of_a_head():
    assert clip_samples(HeadConfig("cnn", (101, 64)), FrontendConfig()) == 16000
    assert clip_samples(HeadConfig("gru", (21, 64)), FrontendConfig()) == 3200
    assert clip_samples(HeadConfig("dnn", (98, 40)), FrontendConfig(n_mels=40, center=False)) == 15920
    assert FrontendConfig(n_mels=40, center=False).n_frames(15920) == 98
    assert clip_samples(HeadConfig("e2e_dnn", (64, 33)), FrontendConfig()) == 5120


def test_header_and_binding_hold_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    declared = set(re.findall(r"\b(nww_[a-z_0-9]+)\s*\(", hdr))
    for sym in REC_SYMBOLS:
        assert re.search(r"^extern int %s\(nww_handle\* h, " % sym, hdr, re.M), sym
        assert sym in declared and sym in _lib.SYMBOLS, sym
    assert len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)


def _hash_score(window: np.ndarray) -> np.float32:
    """a window's samples -> a score in [0, 1): any sample that belongs to another window or recording changes it"""
    return np.float32((zlib.crc32(np.ascontiguousarray(window, np.int16).tobytes()) % 100003) / 100003.0)


class HashModel:
    """forward_recording of a model whose logit is a hash of the window's samples"""

    def __init__(self):
        self.calls = 0

    def forward_recording(self, pcm, window, hop, offset=0, max_batch=4096):
        self.calls += 1
        n = recording_windows(len(pcm), window, hop, offset)
        lg = np.array([_hash_score(pcm[offset + i * hop:offset + i * hop + window]) for i in range(n)], np.float32)
        return lg, (lg * np.float32(0.5)).astype(np.float32)


@pytest.mark.parametrize("window,hop", [(3200, 320), (3200, 1000), (1600, 1600)])
def test_forward_recordings_boundaries(window, hop):
    rng = np.random.default_rng(3)
    lens = [5000, window, 100, window + hop, window + hop - 1, 0, 7777, 3 * hop]      # shorter than a window, exact, ragged, empty
    recs = [rng.integers(-3000, 3000, n).astype(np.int16) for n in lens]
    m = HashModel()
    got = score_recordings(m.forward_recording, recs, window, hop)
    assert m.calls == 1 and len(got) == len(recs)
    for r, (lg, pr) in zip(recs, got):
        want, want_p = HashModel().forward_recording(r, window, hop)
        assert lg.shape == want.shape and np.array_equal(lg, want) and np.array_equal(pr, want_p), len(r)
    assert score_recordings(m.forward_recording, [], window, hop) == []
    with pytest.raises(ValueError):
        score_recordings(m.forward_recording, [np.zeros((2, 4000), np.int16)], window, hop)


class HashSession:
    """E2E session stub (int16 in): run() hashes the clip; run_recording() hashes every window - the two agree by construction only if
    the interpreter asks for the right windows."""
    accepts_int16 = True

    def __init__(self, clip_samples=16000, batch=True):
        self.clip_samples = clip_samples
        self.metadata = {"mode": "e2e"}
        self.runs = self.rec_calls = 0
        if batch:
            self.run_recording = self._run_recording

    def get_inputs(self):
        class In:
            name, shape = "input", [None, 1, self.clip_samples]
        return [In()]

    def run(self, _, feed):
        self.runs += 1
        x = feed["input"]
        assert x.dtype == np.int16 and x.shape == (1, 1, self.clip_samples)
        return [np.array([[[_hash_score(x.reshape(-1))]]], np.float32)]

    def _run_recording(self, pcm, hop=1280, offset=0, max_batch=4096):
        self.rec_calls += 1
        assert pcm.dtype == np.int16 and offset % 8 == 0 and hop % 8 == 0
        return HashModel().forward_recording(pcm, self.clip_samples, hop, offset)[0]


def _predict_loop(pcm, chunk, clip=16000, **kw):
    it = HipInterpreter({"kw": HashSession(clip, batch=False)})
    out = [it.predict(pcm[i:i + chunk], **kw).scores["kw"] for i in range(0, len(pcm), chunk)]
    return np.array(out, np.float32), it


FILTERS = [{}, {"patience": {"kw": 2}, "threshold": {"kw": 0.4}}, {"patience": {"kw": 1}, "threshold": {"kw": 0.5}},
           {"debounce_time": 0.3, "threshold": {"kw": 0.4}}]


@pytest.mark.parametrize("kw", FILTERS, ids=["plain", "patience2", "patience1", "debounce"])
@pytest.mark.parametrize("chunk", [1280, 1600])
@pytest.mark.parametrize("n", [8000, 16000, 48000, 48000 + 700])
def test_score_recording_equals_predict_loop(n, chunk, kw):
    pcm = synth_pcm("speechlike", 1, n, seed=n + chunk)[0]
    want, ref = _predict_loop(pcm, chunk, **kw)
    s = HashSession()
    it = HipInterpreter({"kw": s})
    got = it.score_recording(pcm, chunk_size=chunk, **kw)["kw"]
    assert got.dtype == np.float32 and np.array_equal(got, want), (got, want)
    if n >= 16000:
        assert (want != 0).any() or kw                          # the loop really scores something
        assert s.rec_calls == 1 and s.runs == (1 if n % chunk else 0)      # one batch call (+ the last, shorter chunk)
    # the state a predict() loop leaves behind, and the next chunk scores alike
    assert list(it.prediction_buffer["kw"]) == list(ref.prediction_buffer["kw"]) and it.raw_scores == ref.raw_scores
    assert it.e2e_buffer_samples == ref.e2e_buffer_samples
    nxt = synth_pcm("noise", 1, chunk, seed=5)[0]
    assert it.predict(nxt, **kw).scores == ref.predict(nxt, **kw).scores
    # a second recording is a new stream
    assert np.array_equal(it.score_recording(pcm, chunk_size=chunk, **kw)["kw"], want)


def test_first_window_offset_of_the_defaults():
    """16000 / 1280 is not whole: the window first holds a clip after 13 chunks, and then starts 640 samples in"""
    pcm = synth_pcm("noise", 1, 32000)[0]
    seen = {}

    class S(HashSession):
        def _run_recording(self, pcm, hop=1280, offset=0, max_batch=4096):
            seen["offset"], seen["hop"] = offset, hop
            return super()._run_recording(pcm, hop, offset)

    got = HipInterpreter({"kw": S()}).score_recording(pcm)["kw"]
    assert seen == {"offset": 640, "hop": 1280} and len(got) == 25
    # twelve chunks of zeros (they fill the five warm-up predictions too), then window i starts at 640 + i * 1280
    assert not got[:12].any() and all(got[12 + i] == _hash_score(pcm[640 + i * 1280:640 + i * 1280 + 16000]) for i in range(13))


@pytest.mark.parametrize("chunk", [1004, 1284, 20000])
def test_score_recording_keeps_the_loop_off_the_grid(chunk):
    """chunks that are no multiple of 8 samples (window starts would not be 16-byte aligned) or longer than the clip"""
    pcm = synth_pcm("speechlike", 1, 40000, seed=2)[0]
    want, _ = _predict_loop(pcm, chunk)
    s = HashSession()
    got = HipInterpreter({"kw": s}).score_recording(pcm, chunk_size=chunk)["kw"]
    assert np.array_equal(got, want) and s.rec_calls == 0 and s.runs > 0


def test_score_recording_cascade_and_sessions_without_a_batch_path():
    pcm = synth_pcm("speechlike", 1, 40000, seed=4)[0]
    # a session without run_recording: the loop
    s = HashSession(batch=False)
    want, _ = _predict_loop(pcm, 1280)
    assert np.array_equal(HipInterpreter({"kw": s}).score_recording(pcm)["kw"], want) and s.runs > 0
    # a cascade: the gate decides chunk by chunk whether the verifier runs
    def cascade():
        it = HipInterpreter({"gate": HashSession(), "kw": HashSession()})
        it.cascade_config = {"gate": "gate", "verifier": "kw", "gate_threshold": 0.5}
        return it
    ref = cascade()
    loop = [ref.predict(pcm[i:i + 1280]).scores for i in range(0, len(pcm), 1280)]
    it = cascade()
    got = it.score_recording(pcm)
    for name in ("gate", "kw"):
        assert np.array_equal(got[name], np.array([d[name] for d in loop], np.float32))
        assert it.models[name].rec_calls == 0
