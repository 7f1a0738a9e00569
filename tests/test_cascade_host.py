"""Gate + verifier cascades, host side (no GPU): the seven C-ABI symbols in the header and the binding, the one rule that decides which
windows a gate opens (config.cascade_open), and HipInterpreter.score_recording's batch path for a cascade against the predict() chunk loop,
on stub sessions whose scores hash each window's samples."""
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT
from nanowakeword_amd import _lib
from nanowakeword_amd.config import cascade_open, recording_windows
from nanowakeword_amd.interpreter import HipInterpreter
from nanowakeword_amd.synth import synth_pcm

CASCADE_SYMBOLS = ["nww_cascade_select", "nww_cascade_forward_pcm_dev", "nww_cascade_forward_pcm", "nww_cascade_forward_recording_dev",
                   "nww_cascade_forward_recording", "nww_cascade_stream_push", "nww_cascade_stream_push_dev"]


def test_header_and_binding_hold_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    for sym in CASCADE_SYMBOLS:
        assert re.search(r"^extern int %s\(nww_handle\* (gate|verifier), " % sym, hdr, re.M), sym
        assert sym in _lib.SYMBOLS, sym
    # the count two existing tests pin: declarations that start a line with their return type
    assert len(re.findall(r"^(?:int|int32_t|int64_t|void|float|const char\*)\s+nww_\w+\(", hdr, re.M)) == 48
    assert len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    assert "double gate_threshold" in hdr


def test_cascade_open_is_the_reference_rule():
    p = np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)
    assert cascade_open(p, 0.5).tolist() == [False, False, True, True, True]          # equal to the threshold: open
    assert cascade_open(p, 0.0).all() and cascade_open(p, -1.0).all()                 # a threshold <= 0 opens everything
    assert not cascade_open(p, 2.0).any() and not cascade_open(p, 1.0 + 1e-12).any()  # one > 1 closes everything
    assert cascade_open(p, 1.0).tolist() == [False, False, False, False, True]
    q = np.array([np.nan, 0.1, np.nan], np.float32)
    assert cascade_open(q, 0.5).tolist() == [True, False, True]                       # NaN < thr is false: open
    assert cascade_open(q, 2.0).tolist() == [True, False, True]
    # the comparison is float(np.float32) against the double: 0.3f is above 0.3, 0.1f is above 0.1, 0.7f is below 0.7
    for v in (0.3, 0.1, 0.7, 0.2999999):
        f = np.float32(v)
        assert bool(cascade_open([f], v)[0]) == (not float(f) < v)
        assert bool(cascade_open([f], float(f))[0])                                   # a float32 probability equal to the threshold
    assert cascade_open(np.float32(0.7), 0.7).shape == () and not cascade_open(np.float32(0.7), 0.7)
    out = cascade_open(np.zeros((2, 3), np.float32), 0.5)
    assert out.dtype == bool and out.shape == (2, 3)
    # what the interpreter's own gate test says, value for value
    it = HipInterpreter({"gate": CasSession(0), "kw": CasSession(1)})
    it.cascade_config = {"gate": "gate", "verifier": "kw", "gate_threshold": 0.3}
    for v in (np.float32(0.3), np.float32(0.29999998), np.float32(np.nan), np.float32(0.0)):
        assert it._gate_closed("kw", {"gate": float(v)}) == (not cascade_open(v, 0.3))


def _score(window: np.ndarray, salt: int) -> np.float32:
    """a window's samples -> a score in [0, 1) that differs between the two models"""
    return np.float32((zlib.crc32(np.ascontiguousarray(window, np.int16).tobytes(), salt) % 100003) / 100003.0)


class CasSession:
    """E2E session stub (int16 in): run() hashes the clip; run_recording_cascade() hashes every window with the gate's salt and the
    open ones with its own - it agrees with the predict() loop only if the interpreter asks for the right windows and keeps the gate
    rule.  `asked` counts the windows the verifier was run on."""
    accepts_int16 = True

    def __init__(self, salt, clip_samples=16000, cascade=True):
        self.salt, self.clip_samples = salt, clip_samples
        self.metadata = {"mode": "e2e"}
        self.runs = self.cascade_calls = self.asked = self.windows = 0
        if cascade:
            self.run_recording_cascade = self._run_recording_cascade
            self.cascade_accepts = lambda gate: getattr(gate, "clip_samples", None) == self.clip_samples

    def get_inputs(self):
        class In:
            name, shape = "input", [None, 1, self.clip_samples]
        return [In()]

    def run(self, _, feed):
        self.runs += 1
        x = feed["input"]
        assert x.dtype == np.int16 and x.shape == (1, 1, self.clip_samples)
        return [np.array([[[_score(x.reshape(-1), self.salt)]]], np.float32)]

    def _run_recording_cascade(self, gate, pcm, hop=1280, offset=0, gate_threshold=0.3, max_batch=4096):
        self.cascade_calls += 1
        assert pcm.dtype == np.int16 and offset % 8 == 0 and hop % 8 == 0
        W = self.clip_samples
        n = recording_windows(len(pcm), W, hop, offset)
        win = lambda i: pcm[offset + i * hop:offset + i * hop + W]
        gp = np.array([_score(win(i), gate.salt) for i in range(n)], np.float32)
        open_ = cascade_open(gp, gate_threshold)
        vp = np.zeros(n, np.float32)
        for i in np.flatnonzero(open_):
            vp[i] = _score(win(i), self.salt)
        self.asked += int(open_.sum())
        self.windows += n
        return gp, vp


def _cascade(thr, gate=None, ver=None, extra=None):
    sessions = {"gate": gate or CasSession(0), "kw": ver or CasSession(1)}
    if extra is not None:
        sessions["third"] = extra
    it = HipInterpreter(sessions)
    it.cascade_config = {"gate": "gate", "verifier": "kw", "gate_threshold": thr}
    return it


def _loop(it, pcm, chunk, **kw):
    out = [it.predict(pcm[i:i + chunk], **kw).scores for i in range(0, len(pcm), chunk)]
    return {n: np.array([d[n] for d in out], np.float32) for n in it.models}


FILTERS = [{}, {"patience": {"kw": 2}, "threshold": {"kw": 0.4}}, {"patience": {"kw": 1}, "threshold": {"kw": 0.5}},
           {"debounce_time": 0.3, "threshold": {"kw": 0.4, "gate": 0.4}}]


@pytest.mark.parametrize("kw", FILTERS, ids=["plain", "patience2", "patience1", "debounce"])
@pytest.mark.parametrize("chunk", [1280, 1600])
@pytest.mark.parametrize("n", [8000, 16000, 48700])
@pytest.mark.parametrize("thr", [0.0, 0.5, 2.0])
def test_cascade_batch_path_equals_predict_loop(thr, n, chunk, kw):
    pcm = synth_pcm("speechlike", 1, n, seed=n + chunk)[0]
    ref = _cascade(thr, CasSession(0, cascade=False), CasSession(1, cascade=False))
    want = _loop(ref, pcm, chunk, **kw)
    it = _cascade(thr)
    got = it.score_recording(pcm, chunk_size=chunk, **kw)
    for name in ("gate", "kw"):
        assert got[name].dtype == np.float32 and np.array_equal(got[name], want[name]), (name, got[name], want[name])
    ver, gate = it.models["kw"], it.models["gate"]
    n_full = n // chunk
    assert ver.cascade_calls == 1 and gate.cascade_calls == 0
    last = 1 if n % chunk and n >= 16000 else 0                           # only a last, shorter chunk goes through predict()
    assert gate.runs == last and ver.runs <= last                         # ... where the gate may keep the verifier from running
    assert ver.windows == max(0, n_full - (-(-16000 // chunk) - 1))
    if thr == 2.0:
        assert ver.asked == 0
    elif thr == 0.0:
        assert ver.asked == ver.windows
    elif n == 48700:
        assert 0 < ver.asked < ver.windows                                # the mixed case is not vacuous
        assert (want["kw"] != 0).any() or kw
    # the state a predict() loop leaves behind, and the next chunk scores alike
    for name in ("gate", "kw"):
        assert list(it.prediction_buffer[name]) == list(ref.prediction_buffer[name]), name
    assert it.raw_scores == ref.raw_scores and it.e2e_buffer_samples == ref.e2e_buffer_samples
    nxt = synth_pcm("noise", 1, chunk, seed=5)[0]
    assert it.predict(nxt, **kw).scores == ref.predict(nxt, **kw).scores
    # a second recording is a new stream
    again = it.score_recording(pcm, chunk_size=chunk, **kw)
    assert all(np.array_equal(again[name], want[name]) for name in ("gate", "kw"))


def test_gating_is_on_the_post_warm_up_score():
    """the gate's first five predictions are zeroed, and the verifier is gated on that zero: with a positive threshold it reports 0 there
    although the raw gate probability opens the window on the device"""
    pcm = synth_pcm("speechlike", 1, 16000 * 8, seed=11)[0]               # chunks of a whole clip: the first chunk fills the window
    it = _cascade(1e-6)
    got = it.score_recording(pcm, chunk_size=16000)
    ver = it.models["kw"]
    assert ver.asked == ver.windows == 8                                    # every raw gate probability reaches 1e-6
    assert not got["kw"][:5].any() and got["kw"][5:].all() and not got["gate"][:5].any() and got["gate"][5:].all()
    ref = _cascade(1e-6, CasSession(0, cascade=False), CasSession(1, cascade=False))
    assert np.array_equal(_loop(ref, pcm, 16000)["kw"], got["kw"]) and ref.models["kw"].runs == 3


def test_the_loop_is_kept():
    pcm = synth_pcm("speechlike", 1, 40000, seed=4)[0]

    def check(it, chunk=1280):
        ref = HipInterpreter({n: CasSession(s.salt, s.clip_samples, cascade=False) for n, s in it.models.items()})
        ref.cascade_config = dict(it.cascade_config)
        want = _loop(ref, pcm, chunk)
        got = it.score_recording(pcm, chunk_size=chunk)
        for name in it.models:
            assert np.array_equal(got[name], want[name]), name
            assert it.models[name].cascade_calls == 0 and it.models[name].runs == ref.models[name].runs
        assert it.models["gate"].runs > 0

    check(_cascade(0.5, ver=CasSession(1, cascade=False)))                 # the verifier lacks the method
    check(_cascade(0.5, gate=CasSession(0, clip_samples=8000)))            # cascade_accepts is false: the clip lengths differ
    check(_cascade(0.5), chunk=1284)                                       # off the 8-sample grid
    check(_cascade(0.5, extra=CasSession(2)))                              # a third model
