"""Model banks (nww_bank_*) on the CPU: the seven declarations of include/nww.h and their ctypes symbols; the rules of csrc/bank.h -
the frontend comparison and the member validation - in tests/hostemu/bank_check.cpp, a stand-alone g++ program with its own main,
built with -fsanitize=address,undefined; interpreter.BankStreamPool against K independent StreamPools on fake backends; and
HipInterpreter.load_model(bank=True) against bank=False on fake sessions that offer bank_accepts / run_bank / run_recording_bank.
No GPU, and no library is loaded into Python."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from nanowakeword_amd.config import recording_windows
from nanowakeword_amd.interpreter import BankStreamPool, HipInterpreter, StreamPool
from nanowakeword_amd.synth import synth_pcm

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")
BANK = ("nww_bank_check", "nww_bank_forward_pcm_dev", "nww_bank_forward_pcm", "nww_bank_forward_recording_dev", "nww_bank_forward_recording",
        "nww_bank_stream_push_some_dev", "nww_bank_stream_push_some")


def test_header_declares_the_bank_entry_points():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    for name in BANK:
        assert len(re.findall(r"^extern int %s\(nww_handle\* const\* members, int32_t k[,)]" % name, hdr, re.M)) == 1, name
    # declared `extern`: the pinned count of declarations that start a line with their return type has not moved
    assert len(re.findall(r"^(?:int|int32_t|int64_t|void|float|const char\*)\s+nww_\w+\(", hdr, re.M)) == 48
    from nanowakeword_amd import _lib
    assert set(BANK) <= set(_lib.SYMBOLS) and len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    # every bank entry point has a definition, in its own translation unit, which the build compiles
    src = open(os.path.join(CSRC, "nww_bank.hip")).read()
    for name in BANK:
        assert len(re.findall(r'^extern "C" int %s\(' % name, src, re.M)) == 1, name
    from nanowakeword_amd import build
    assert "nww_bank.hip" in build.HIP_SOURCES
    # the rules live in a header that needs no HIP
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(CSRC, "bank.h")).read()).lower()


def test_bank_rules_host_program(tmp_path):
    exe = str(tmp_path / "bank_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "hostemu", "bank_check.cpp"), os.path.join(CSRC, "fe_tables.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]


# ---- BankStreamPool against K independent StreamPools
def _score(window: np.ndarray, salt: int) -> np.float32:
    """a window's samples and the model's salt -> a score in (0, 1): any sample of another stream or window changes it"""
    return np.float32((zlib.crc32(np.ascontiguousarray(window, np.int16).tobytes() + bytes([salt])) % 99991 + 1) / 100003.0)


class FakeStreams:
    """CPU stand-in for HipModel's pool calls: every stream keeps its own samples since its last reset; the score of a full window is
    a hash of it and of the model's salt"""

    def __init__(self, salt):
        self.salt, self.pushes = salt, 0

    def stream_open(self, S, W, hop):
        self.S, self.W, self.hop = S, W, hop
        self.stream_reset()

    def stream_reset(self):
        self.buf = [np.zeros(0, np.int16) for _ in range(self.S)]

    def stream_reset_some(self, ids):
        for s in ids:
            self.buf[int(s)] = np.zeros(0, np.int16)

    def feed(self, ids, chunk):
        assert chunk.shape == (len(ids), self.hop)
        for i, s in enumerate(ids):
            self.buf[int(s)] = np.concatenate([self.buf[int(s)], chunk[i]])[-self.W:]

    def scores(self, ids, salt):
        p = np.array([_score(self.buf[int(s)], salt) if len(self.buf[int(s)]) >= self.W else 0.0 for s in ids], np.float32)
        return p.copy(), p

    def stream_push_some(self, ids, chunk):
        self.pushes += 1
        self.feed(ids, chunk)
        return self.scores(ids, self.salt)

    def stream_close(self):
        self.closed = True


class FakeBank(FakeStreams):
    """... and for session.HipBank: one set of rings, K scores per listed stream"""

    def __init__(self, salts):
        super().__init__(None)
        self.names, self.salts = list(salts), dict(salts)

    def stream_push_some(self, ids, chunk):
        self.pushes += 1
        self.feed(ids, chunk)
        return {n: self.scores(ids, self.salts[n]) for n in self.names}


SALTS = {"hey": 1, "stop": 2, "lights": 3}
BANK_FILTERS = [({}, {}),
                (dict(patience={"hey": 1, "stop": 3}, threshold={"hey": 0.3, "stop": 0.6}), {"hey": dict(patience=1, threshold=0.3), "stop": dict(patience=3, threshold=0.6)}),
                (dict(debounce_time=0.1, threshold={"hey": 0.4, "lights": 0.7}), {"hey": dict(debounce_time=0.1, threshold=0.4), "lights": dict(debounce_time=0.1, threshold=0.7)})]


@pytest.mark.parametrize("kw,per_model", BANK_FILTERS, ids=["plain", "patience", "debounce"])
def test_bank_stream_pool_equals_independent_pools(kw, per_model):
    S, W, hop, ticks = 5, 1600, 320, 40
    fake = FakeBank(SALTS)
    pool = BankStreamPool(fake, S, W, hop)
    alone = {n: StreamPool(FakeStreams(s), S, W, hop, name=n) for n, s in SALTS.items()}
    audio = np.stack([synth_pcm("noise", 1, hop * ticks, seed=s)[0] for s in range(S)])
    cursor = np.zeros(S, int)
    nonzero = {n: 0 for n in SALTS}
    for s in range(S):
        assert pool.attach() == s and all(p.attach() == s for p in alone.values())
    for t in range(ticks):
        if t == 12:                                              # a client leaves, another takes its slot; one stream is reset in place
            pool.detach(3)
            assert pool.attach() == 3
            pool.reset([1])
            for p in alone.values():
                p.detach(3)
                assert p.attach() == 3
                p.reset([1])
        if t == 30:                                              # every stream at once
            pool.reset()
            for p in alone.values():
                p.reset()
        ids = [s for s in range(S) if not (s == 2 and t < 3) and not (s == 4 and t % 3 == 2)]      # a late joiner, one that skips ticks
        chunk = np.ascontiguousarray(np.stack([audio[s, cursor[s]:cursor[s] + hop] for s in ids]))
        cursor[ids] += hop
        got = pool.push(ids, chunk, **kw)
        assert list(got) == list(SALTS)
        for n, p in alone.items():
            want = p.push(ids, chunk, **per_model.get(n, {}))
            assert got[n].dtype == np.float32 and np.array_equal(got[n], want), (t, n, got[n], want)
            assert np.array_equal(pool.history[n], p.history) and np.array_equal(pool.count[n], p.count), (t, n)
            assert np.array_equal(pool.raw_scores[n], p.raw_scores) and np.array_equal(pool.post_processed_scores[n], p.post_processed_scores), (t, n)
            nonzero[n] += int((want != 0).sum())
        assert np.array_equal(pool.attached, alone["hey"].attached)
    # (a patience of two or more never lets a first score through: the history it counts holds filtered scores, as in the reference)
    assert all(v for n, v in nonzero.items() if per_model.get(n, {}).get("patience", 0) < 2), nonzero
    assert fake.pushes == ticks and all(p.backend.pushes == ticks for p in alone.values())      # one device call per tick for all models
    if kw:                                                       # the filters did zero scores the plain run reports
        plain = BankStreamPool(FakeBank(SALTS), 1, W, hop)
        raw = [plain.push([0], audio[:1, t * hop:(t + 1) * hop]) for t in range(12)]
        filt = BankStreamPool(FakeBank(SALTS), 1, W, hop)
        out = [filt.push([0], audio[:1, t * hop:(t + 1) * hop], **kw) for t in range(12)]
        assert any(a[n][0] != 0 and b[n][0] == 0 for a, b in zip(raw, out) for n in per_model)
    with pytest.raises(ValueError, match="threshold"):
        pool.push([0], audio[:1, :hop], patience={"hey": 2})
    with pytest.raises(ValueError, match="cannot be used together"):
        pool.push([0], audio[:1, :hop], patience={"hey": 2}, threshold={"hey": 0.5}, debounce_time=0.5)
    with pytest.raises(ValueError, match="strictly ascending"):
        pool.push([1, 0], audio[:2, :hop])
    pool.close()
    assert fake.closed


# ---- HipInterpreter(bank=True) against bank=False
class PlainSession:
    """E2E session stub (int16 in) whose score is a hash of the clip and of its salt"""
    accepts_int16 = True

    def __init__(self, salt, clip_samples=16000, family="a"):
        self.salt, self.clip_samples, self.family = salt, clip_samples, family
        self.metadata = {"mode": "e2e"}
        self.runs = self.rec_calls = self.bank_runs = self.bank_rec_calls = 0

    def get_inputs(self):
        class In:
            name, shape = "input", [None, 1, self.clip_samples]
        return [In()]

    def run(self, _, feed):
        self.runs += 1
        x = feed["input"]
        assert x.dtype == np.int16 and x.shape == (1, 1, self.clip_samples)
        return [np.array([[[_score(x.reshape(-1), self.salt)]]], np.float32)]

    def run_recording(self, pcm, hop=1280, offset=0, max_batch=4096):
        self.rec_calls += 1
        assert pcm.dtype == np.int16 and offset % 8 == 0 and hop % 8 == 0
        n = recording_windows(len(pcm), self.clip_samples, hop, offset)
        return np.array([_score(pcm[offset + i * hop:offset + i * hop + self.clip_samples], self.salt) for i in range(n)], np.float32)


class BankSession(PlainSession):
    """... with the bank protocol of session.HipSession: bank_accepts, and run_bank / run_recording_bank, which score for every session
    of the list in one call"""

    def bank_accepts(self, other):
        return isinstance(other, BankSession) and other is not self and other.clip_samples == self.clip_samples and other.family == self.family

    def run_bank(self, sessions, x):
        assert sessions[0] is self and x.dtype == np.int16 and x.shape == (1, self.clip_samples)
        self.bank_runs += 1
        return [np.array([[[_score(x.reshape(-1), s.salt)]]], np.float32) for s in sessions]

    def run_recording_bank(self, sessions, pcm, hop=1280, offset=0, max_batch=4096):
        assert sessions[0] is self
        self.bank_rec_calls += 1
        out = []
        for s in sessions:
            out.append(s.run_recording(pcm, hop, offset))
            s.rec_calls -= 1                                     # (the stub's own arithmetic, not a call of the interpreter's)
        return out


def _sessions(cls=BankSession):
    return {"hey": cls(1), "stop": cls(2), "lights": cls(3)}


FILTERS = [{}, {"patience": {"hey": 2, "lights": 1}, "threshold": {"hey": 0.4, "lights": 0.5}}, {"debounce_time": 0.3, "threshold": {"hey": 0.4, "stop": 0.6}}]


@pytest.mark.parametrize("kw", FILTERS, ids=["plain", "patience", "debounce"])
@pytest.mark.parametrize("chunk", [1280, 1600, 1004])
def test_interpreter_bank_equals_the_loop(kw, chunk):
    pcm = synth_pcm("speechlike", 1, 48000 + 700, seed=chunk)[0]
    ref = HipInterpreter.load_model(_sessions())
    it = HipInterpreter.load_model(_sessions(), bank=True)
    assert not ref.bank and len(it.bank) == 3 and it.bank[0] is it.models["hey"]
    # predict(): equal traces, one bank call per chunk that holds a clip, no single-session call
    n_chunks, full_from = 0, None
    for i in range(0, len(pcm), chunk):
        a, b = it.predict(pcm[i:i + chunk], **kw), ref.predict(pcm[i:i + chunk], **kw)
        assert a.scores == b.scores and list(a.scores) == list(b.scores), (i, a.scores, b.scores)
        assert (a.score, a.detected, a.model_name) == (b.score, b.detected, b.model_name)
        assert it.raw_scores == ref.raw_scores and it.post_processed_scores == ref.post_processed_scores
        n_chunks += 1
        if full_from is None and i + min(chunk, len(pcm) - i) >= 16000:
            full_from = n_chunks - 1
    assert {n: list(v) for n, v in it.prediction_buffer.items()} == {n: list(v) for n, v in ref.prediction_buffer.items()}
    assert it.e2e_buffer_samples == ref.e2e_buffer_samples
    assert any(v != 0 for v in it.raw_scores.values())
    lead = it.models["hey"]
    assert lead.bank_runs == n_chunks - full_from and all(s.runs == 0 and s.bank_runs == 0 for n, s in it.models.items() if n != "hey") and lead.runs == 0
    assert all(s.runs == n_chunks - full_from for s in ref.models.values())
    # score_recording(): equal output and state; on the grid one bank call for the recording (+ the last, shorter chunk through predict)
    runs0 = lead.bank_runs
    got, want = it.score_recording(pcm, chunk_size=chunk, **kw), ref.score_recording(pcm, chunk_size=chunk, **kw)
    assert list(got) == list(want) and all(np.array_equal(got[n], want[n]) for n in want), (got, want)
    assert all((want[n] != 0).any() for n in want) or kw
    assert {n: list(v) for n, v in it.prediction_buffer.items()} == {n: list(v) for n, v in ref.prediction_buffer.items()}
    assert it.raw_scores == ref.raw_scores and it.e2e_buffer_samples == ref.e2e_buffer_samples
    if chunk % 8 == 0:
        assert lead.bank_rec_calls == 1 and lead.bank_runs - runs0 == (1 if len(pcm) % chunk else 0)
        assert all(s.rec_calls == 0 for s in it.models.values()) and all(s.rec_calls == 1 for s in ref.models.values())
    else:                                                        # off the grid: the predict() loop, which is the bank's too
        assert lead.bank_rec_calls == 0 and lead.bank_runs - runs0 == n_chunks - full_from
    nxt = synth_pcm("noise", 1, chunk, seed=5)[0]
    assert it.predict(nxt, **kw).scores == ref.predict(nxt, **kw).scores
    it.reset()
    assert it.e2e_buffer_samples == {n: 0 for n in it.models} and not any(it.raw_scores.values())


def test_interpreter_bank_falls_back_to_the_loop():
    pcm = synth_pcm("speechlike", 1, 40000, seed=4)[0]

    def same_as_loop(it, sessions):
        ref = HipInterpreter.load_model({n: BankSession(s.salt, s.clip_samples) for n, s in sessions.items()})
        assert not it.bank
        got, want = it.score_recording(pcm), ref.score_recording(pcm)
        assert all(np.array_equal(got[n], want[n]) for n in want)
        for i in range(0, 20000, 1280):
            assert it.predict(pcm[i:i + 1280]).scores == ref.predict(pcm[i:i + 1280]).scores
        assert all(s.bank_runs == 0 and s.bank_rec_calls == 0 for s in sessions.values())
        assert all(s.rec_calls == 1 and s.runs > 0 for s in sessions.values())

    # a session of another family (another frontend): the first one's bank_accepts says no
    ss = _sessions()
    ss["stop"].family = "b"
    same_as_loop(HipInterpreter.load_model(ss, bank=True), ss)
    # another clip length
    ss = {"hey": BankSession(1), "stop": BankSession(2, clip_samples=24000)}
    same_as_loop(HipInterpreter.load_model(ss, bank=True), ss)
    # sessions without the bank protocol
    ss = _sessions(PlainSession)
    assert not hasattr(ss["hey"], "bank_accepts")
    same_as_loop(HipInterpreter.load_model(ss, bank=True), ss)
    # one model: nothing to share
    ss = {"hey": BankSession(1)}
    same_as_loop(HipInterpreter.load_model(ss, bank=True), ss)
    # a cascade stays a cascade
    ss = {"hey": BankSession(1)}
    it = HipInterpreter.load_model(ss, gate_model=BankSession(9), gate_threshold=0.5, bank=True)
    assert it.is_cascade and not it.bank
    # bank defaults to False
    assert not HipInterpreter.load_model(_sessions()).bank
