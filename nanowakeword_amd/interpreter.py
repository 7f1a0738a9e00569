"""Host-side mirror of the reference's inference API for the hot path.

``HipInterpreter`` keeps the public surface of ``nanowakeword.interpreter.NanoInterpreter``
(reference: nanowakeword/interpreter/nanointerpreter.py): ``load_model`` / ``predict`` /
``predict_clip`` / ``reset`` / ``detected`` and the ``score`` / ``gate_score`` / ``verifier_score`` /
``model_name`` / ``gate_name`` / ``is_cascade`` / ``info`` / ``raw_scores`` accessors, plus
``DetectionResult`` (:45-115).  Scores come from any object that follows the session protocol
(``get_inputs()``, ``run(None, {"input": x})``) - normally a ``HipSession`` on an MI355X.

Kept on the host, per stream: the raw-audio window, the first-5-predictions
zeroing (:689-691,789-790), cascade gating (:660-669,758-769) and the patience / debounce filters
(:1034-1064).  Not mirrored (out of scope): VAD, noise reduction, the WebSocket
remote verifier, the microphone loop.
"""
from __future__ import annotations

import math
import os
import wave
from collections import deque
from typing import Dict, List, Mapping, Optional, Union

import numpy as np

from .config import cascade_open, cascade_pool_open

N_WARMUP_PREDICTIONS = 5        # nanointerpreter.py:690,789
PREDICTION_HISTORY = 30         # nanointerpreter.py:1002
HOP_SAMPLES = 1280              # 80 ms @ 16 kHz (AudioFeatures.py:414)


class DetectionResult:
    """Attribute + dict-style view of one predict() call (nanointerpreter.py:45-115)."""

    __slots__ = ("scores", "model_name", "gate_name", "threshold")

    def __init__(self, scores: dict, model_name: str, gate_name: Optional[str], threshold: float = 0.0):
        self.scores, self.model_name, self.gate_name, self.threshold = scores, model_name, gate_name, threshold

    @property
    def score(self) -> float:
        return self.scores.get(self.model_name, 0.0)

    @property
    def gate_score(self) -> float:
        return self.scores.get(self.gate_name, 0.0) if self.gate_name else 0.0

    @property
    def detected(self) -> bool:
        return self.score >= self.threshold if self.threshold > 0 else False

    def get(self, model_name: str, default: float = 0.0) -> float:
        return self.scores.get(model_name, default)

    def __getitem__(self, key: str) -> float:
        return self.scores[key]

    def __contains__(self, key: str) -> bool:
        return key in self.scores

    def __repr__(self) -> str:
        out = [f"score={self.score:.4f}"]
        if self.gate_name:
            out.append(f"gate={self.gate_score:.4f}")
        if self.threshold > 0:
            out.append(f"detected={self.detected}")
        return "DetectionResult(" + ", ".join(out) + ")"


class _AudioWindow:
    """Last `size` int16 samples of a stream (the reference keeps a deque(maxlen) of floats, :181,751-756)."""

    def __init__(self, size: int):
        self.size = int(size)
        self.data = np.zeros(self.size, np.int16)
        self.filled = 0          # total samples seen (saturating semantics only matter vs size)

    def push(self, x: np.ndarray):
        n = len(x)
        if n >= self.size:
            self.data[:] = x[n - self.size:]
        elif n:
            self.data[:-n] = self.data[n:]
            self.data[-n:] = x
        self.filled += n

    def clear(self):
        self.data[:] = 0
        self.filled = 0


def _is_e2e_session(session) -> bool:
    """Mode detection (nanointerpreter.py:968-992): explicit metadata first, then the rank heuristic."""
    meta = getattr(session, "metadata", None)
    if isinstance(meta, Mapping) and "mode" in meta:
        return meta["mode"] == "e2e"
    shape = session.get_inputs()[0].shape
    if len(shape) <= 2:
        return True
    return len(shape) == 3 and shape[-1] not in (32, 64, 96)


class HipInterpreter:
    """Stateful wake-word scoring over a stream of int16 chunks (one instance per stream; not thread-safe,
    like the reference)."""

    def __init__(self, sessions: Mapping[str, object], preprocessor=None, vad_threshold: float = 0,
                 enable_noise_reduction: bool = False):
        if not sessions:
            raise ValueError("at least one model session is required")
        if vad_threshold and vad_threshold > 0:
            raise NotImplementedError("VAD post-filter is outside the accelerated path (SURVEY.md §2 #9)")
        if enable_noise_reduction:
            raise NotImplementedError("noise reduction is outside the accelerated path")
        self.models: Dict[str, object] = dict(sessions)
        self.model_input_names = {n: [i.name for i in s.get_inputs()] for n, s in self.models.items()}
        self.model_feature_length = {n: s.get_inputs()[0].shape[1] for n, s in self.models.items()}
        self.class_mapping = {n: {"0": n} for n in self.models}
        self.raw_scores = {n: 0.0 for n in self.models}
        self.post_processed_scores = {n: 0.0 for n in self.models}
        self.is_e2e = {n: _is_e2e_session(s) for n, s in self.models.items()}
        self.e2e_clip_samples, self.e2e_input_ndim, self._windows = {}, {}, {}
        for n, s in self.models.items():
            if self.is_e2e[n]:
                shape = s.get_inputs()[0].shape
                self.e2e_clip_samples[n] = int(shape[-1])
                self.e2e_input_ndim[n] = len(shape)
                self._windows[n] = _AudioWindow(shape[-1])
        self.prediction_buffer: Dict[str, deque] = {}
        all_e2e = all(self.is_e2e.values())
        if not all_e2e and preprocessor is None:
            raise ValueError("feature-input models need a preprocessor object (AudioFeatures protocol: "
                             "__call__, feature_buffer, get_features, reset)")
        self.preprocessor = None if all_e2e else preprocessor
        self.cascade_config: dict = {}
        self.vad_threshold = 0
        self.bank: list = []          # load_model(bank=True): the sessions that share one frontend pass, the leader first (else empty)

    # ------------------------------------------------------------------ construction
    @classmethod
    def load_model(cls, model: Union[str, List[str], Mapping[str, object], object, None] = None, cascade: bool = False,
                   gate_model=None, gate_threshold: float = 0.3, device: int = 0, bank: bool = False, **kwargs) -> "HipInterpreter":
        """Same calling convention as NanoInterpreter.load_model (:310-325).  ``model`` may be a path (or
        list of paths) to the reference's own exported ``*.onnx`` files (weights recovered by
        ``weights.state_dict_from_onnx``), to bundles written by ``weights.save_bundle`` (``*.nww.npz``),
        or ready session objects / a {name: session} mapping.  ``cascade=True`` looks for ``<name>_lite``
        next to the main bundle; ``gate_model`` names the gate explicitly (implies cascade).  ``bank=True`` scores several wake words
        on ONE frontend pass (session.HipBank): it applies when the interpreter is not a cascade, holds at least two e2e sessions and the
        first one's ``bank_accepts`` takes every other - one device, one clip length, identical mel frontends; ``predict`` then keeps one
        audio window and ``score_recording`` uploads the recording once.  Sessions that do not qualify are scored one after the other,
        as without it; scores, histories and results are the same either way."""
        from .weights import load_session
        if model is None:
            raise ValueError("`model` is required (remote verifier mode is not part of the accelerated path)")
        sessions: Dict[str, object] = {}
        paths: List[str] = []
        if isinstance(model, Mapping):
            sessions.update(model)
        elif isinstance(model, str):
            paths = [model]
        elif isinstance(model, list) and all(isinstance(m, str) for m in model):
            paths = list(model)
        elif isinstance(model, (list, tuple)):
            for i, s in enumerate(model):
                sessions[getattr(s, "name", f"model{i}")] = s
        elif hasattr(model, "run") and hasattr(model, "get_inputs"):
            sessions[getattr(model, "name", "model")] = model
        else:
            raise TypeError("`model` must be a string, list of strings, a session or a mapping of sessions.")
        for p in paths:
            if not os.path.exists(p):
                raise FileNotFoundError(f"Model file not found: {p}")

        def stem(p):
            b = os.path.basename(p)
            for ext in (".nww.npz", ".npz", ".onnx", ".pt"):
                if b.endswith(ext):
                    return b[:-len(ext)]
            return os.path.splitext(b)[0]

        cascade_cfg: dict = {}
        gate_session = None
        if gate_model is not None and not isinstance(gate_model, str):
            gate_session, gate_name = gate_model, getattr(gate_model, "name", "gate")
        if (cascade or gate_model is not None) and (len(paths) == 1 or (len(sessions) == 1 and gate_session is not None)):
            main_name = stem(paths[0]) if paths else next(iter(sessions))
            if gate_session is not None:
                pass
            elif gate_model is not None:
                if not os.path.exists(gate_model):
                    raise FileNotFoundError(f"The specified gate model does not exist: {gate_model}")
                gate_name, gate_session = stem(gate_model), load_session(gate_model, device=device)
            else:
                d = os.path.dirname(os.path.abspath(paths[0]))
                gate_name = main_name + "_lite"
                cand = [os.path.join(d, gate_name + ext) for ext in (".nww.npz", ".npz", ".onnx")]
                hit = next((c for c in cand if os.path.exists(c)), None)
                gate_session = load_session(hit, device=device) if hit else None    # else: single-model mode (:481-487)
            if gate_session is not None:
                ordered = {gate_name: gate_session}              # the gate is evaluated first
                for p in paths:
                    ordered[stem(p)] = load_session(p, device=device)
                ordered.update(sessions)
                sessions, paths = ordered, []
                cascade_cfg = {"gate": gate_name, "verifier": main_name, "gate_threshold": gate_threshold}
        for p in paths:
            name = stem(p)
            if name not in sessions:
                sessions[name] = load_session(p, device=device)
        inst = cls(sessions, **kwargs)
        inst.cascade_config = cascade_cfg
        if bank:
            inst._enable_bank()
        return inst

    def _enable_bank(self):
        """the sessions as a bank, when they qualify (load_model(bank=True)); otherwise nothing changes"""
        ss = list(self.models.values())
        lead = ss[0]
        if (self.is_cascade or self.preprocessor is not None or len(ss) < 2 or not all(self.is_e2e.values())
                or not all(hasattr(lead, a) for a in ("bank_accepts", "run_bank", "run_recording_bank"))
                or len(set(self.e2e_clip_samples.values())) != 1 or not all(lead.bank_accepts(s) for s in ss[1:])):
            return
        self.bank = ss
        shared = self._windows[next(iter(self.models))]            # one audio window for all models
        self._windows = {n: shared for n in self.models}

    # ------------------------------------------------------------------ accessors (:196-295)
    @property
    def is_cascade(self) -> bool:
        return bool(self.cascade_config)

    @property
    def model_name(self) -> str:
        return self.cascade_config["verifier"] if self.is_cascade else next(iter(self.models))

    @property
    def gate_name(self) -> Optional[str]:
        return self.cascade_config.get("gate")

    @property
    def gate_score(self) -> float:
        return self.post_processed_scores.get(self.gate_name, 0.0) if self.gate_name else 0.0

    @property
    def verifier_score(self) -> float:
        return self.post_processed_scores.get(self.model_name, 0.0)

    @property
    def score(self) -> float:
        return self.verifier_score

    @property
    def info(self) -> dict:
        return {"model_name": self.model_name, "is_cascade": self.is_cascade, "is_remote": False,
                "gate_name": self.gate_name, "gate_threshold": self.cascade_config.get("gate_threshold"),
                "loaded_models": list(self.models), "score": self.score, "gate_score": self.gate_score,
                "raw_scores": dict(self.raw_scores)}

    def detected(self, threshold: float, model: Optional[str] = None) -> bool:
        return self.post_processed_scores.get(model or self.model_name, 0.0) >= threshold

    def __repr__(self) -> str:
        if self.is_cascade:
            return (f"HipInterpreter(model='{self.model_name}', gate='{self.gate_name}', "
                    f"gate_threshold={self.cascade_config.get('gate_threshold', 0.3)})")
        names = list(self.models)
        return f"HipInterpreter(model='{names[0]}')" if len(names) == 1 else f"HipInterpreter(models={names})"

    # ------------------------------------------------------------------ scoring
    def _history(self, name) -> deque:
        buf = self.prediction_buffer.get(name)
        if buf is None:
            buf = self.prediction_buffer[name] = deque(maxlen=PREDICTION_HISTORY)
        return buf

    def _gate_closed(self, name, current) -> bool:
        c = self.cascade_config
        return bool(c) and name == c["verifier"] and current.get(c["gate"], 0.0) < c["gate_threshold"]

    def _run_e2e(self, name, session) -> float:
        win = self._windows[name]
        clip = win.data
        if getattr(session, "accepts_int16", False):
            x = clip.reshape(1, 1, -1) if self.e2e_input_ndim[name] == 3 else clip.reshape(1, -1)
        else:   # the reference's float path: x/32768.0, (1,1,N) or (1,N)  (:750,771-775)
            f = clip.astype(np.float32) / np.float32(32768.0)
            x = f.reshape(1, 1, -1) if self.e2e_input_ndim[name] == 3 else f.reshape(1, -1)
        return float(session.run(None, {"input": x})[0].item())

    def predict(self, x: np.ndarray, patience: dict = {}, threshold: dict = {}, debounce_time: float = 0.0) -> DetectionResult:
        """One chunk of 16-bit PCM in, per-model scores out (nanointerpreter.py:606-717, 735-814)."""
        if not isinstance(x, np.ndarray):
            raise ValueError("Input audio `x` must be a Numpy array.")
        current: Dict[str, float] = {}
        if self.preprocessor is None:                       # ---- E2E: raw audio windows per model
            xi = x if x.dtype == np.int16 else x.astype(np.int16)
            if self.bank:                                    # one window, one upload, one frontend pass for all models
                win = self._windows[next(iter(self.models))]
                win.push(xi)
                scores = ([float(p.item()) for p in self.bank[0].run_bank(self.bank, win.data.reshape(1, -1))]
                          if win.filled >= win.size else [0.0] * len(self.models))
                for name, score in zip(self.models, scores):
                    self.raw_scores[name] = score
                    if len(self.prediction_buffer.get(name, ())) < N_WARMUP_PREDICTIONS:
                        score = 0.0
                    current[name] = score
            for name, session in () if self.bank else self.models.items():
                win = self._windows[name]
                win.push(xi)
                if win.filled >= win.size:
                    if self._gate_closed(name, current):
                        current[name] = 0.0
                        self.raw_scores[name] = 0.0
                        continue
                    score = self._run_e2e(name, session)
                else:
                    score = 0.0
                self.raw_scores[name] = score
                if len(self.prediction_buffer.get(name, ())) < N_WARMUP_PREDICTIONS:
                    score = 0.0
                current[name] = score
            n_samples = len(x)
        else:                                               # ---- feature mode: preprocessor protocol
            n_samples = self.preprocessor(x)
            if n_samples < HOP_SAMPLES:
                return DetectionResult(dict(self.post_processed_scores), self.model_name, self.gate_name)
            for name, session in self.models.items():
                frames = self.model_feature_length[name]
                if self.preprocessor.feature_buffer.shape[0] < frames or self._gate_closed(name, current):
                    current[name] = 0.0
                    continue
                score = float(session.run(None, {"input": self.preprocessor.get_features(frames)})[0].item())
                self.raw_scores[name] = score
                if len(self.prediction_buffer.get(name, ())) < N_WARMUP_PREDICTIONS:
                    score = 0.0
                current[name] = score
        final = dict(current)
        self._post_filters(final, patience, threshold, debounce_time, n_samples)
        for name, s in final.items():
            self._history(name).append(s)
            self.post_processed_scores[name] = s
        return DetectionResult(dict(final), self.model_name, self.gate_name)

    def _post_filters(self, preds, patience, threshold, debounce_time, n_samples):
        """Patience (N consecutive frames >= threshold) or debounce (suppress repeats), :1034-1064."""
        if not patience and debounce_time <= 0:
            return
        if not threshold:
            raise ValueError("`threshold` must be provided when using `patience` or `debounce_time`.")
        if patience and debounce_time > 0:
            raise ValueError("`patience` and `debounce_time` cannot be used together.")
        for name, s in list(preds.items()):
            if s == 0.0:
                continue
            hist = list(self._history(name))
            if name in patience:
                need = patience[name]
                if len(hist) < need:
                    preds[name] = 0.0
                    continue
                tail = hist[-(need - 1):] if need > 1 else hist      # reference slices buffer[-(need-1):]; need==1 -> [-0:] = all
                hits = sum(1 for v in tail + [s] if v >= threshold[name])
                if hits < need:
                    preds[name] = 0.0
            elif debounce_time > 0 and name in threshold:
                dur = n_samples / 16000.0
                if dur <= 0:
                    continue
                k = int(math.ceil(debounce_time / dur))
                if s >= threshold[name] and any(v >= threshold[name] for v in hist[-k:]):
                    preds[name] = 0.0

    def predict_clip(self, clip: Union[str, np.ndarray], chunk_size: int = HOP_SAMPLES, **kwargs) -> list:
        """Whole clip (path or array) -> list of DetectionResult (:816-833). E2E mode: one prediction."""
        if isinstance(clip, str):
            with wave.open(clip, mode="rb") as f:
                if f.getframerate() != 16000 or f.getsampwidth() != 2 or f.getnchannels() != 1:
                    raise ValueError("Audio clip must be a 16kHz, 16-bit, single-channel WAV file.")
                data = np.frombuffer(f.readframes(f.getnframes()), dtype=np.int16)
        elif isinstance(clip, np.ndarray):
            data = clip
        else:
            raise TypeError("`clip` must be a file path (string) or a numpy array.")
        if self.preprocessor is None:
            return [self.predict(data, **kwargs)]
        return [self.predict(data[i:i + chunk_size], **kwargs) for i in range(0, len(data), chunk_size)]

    def score_recording(self, pcm: Union[str, np.ndarray], chunk_size: int = HOP_SAMPLES, patience: dict = {}, threshold: dict = {},
                        debounce_time: float = 0.0) -> Dict[str, np.ndarray]:
        """A whole recording as a NEW stream: {model: float32 scores, one per chunk} - exactly what reset() followed by predict() on
        pcm[0:chunk_size], pcm[chunk_size:2 * chunk_size], ... returns as DetectionResult.scores, and the same state left behind (zeros
        until the window holds a clip, first five predictions zeroed, patience / debounce).  E2E sessions that offer run_recording
        (HipSession) score every full chunk's window in batches, the recording uploaded once: the first window starts at
        (-clip_samples) % chunk_size.  A cascade takes the batch path when it is exactly a gate and a verifier whose session offers
        run_recording_cascade and accepts the gate's session (two HipSessions on one device with the same clip length): the verifier
        then runs only on the windows the gate opens.  Other cascades, embedding-mode interpreters (a preprocessor) and chunk sizes or
        first offsets that are not multiples of 8 samples take the predict() loop."""
        if isinstance(pcm, str):
            with wave.open(pcm, mode="rb") as f:
                if f.getframerate() != 16000 or f.getsampwidth() != 2 or f.getnchannels() != 1:
                    raise ValueError("Audio clip must be a 16kHz, 16-bit, single-channel WAV file.")
                pcm = np.frombuffer(f.readframes(f.getnframes()), dtype=np.int16)
        if not isinstance(pcm, np.ndarray) or pcm.ndim != 1:
            raise ValueError("a recording must be a one-dimensional Numpy array (or a WAV path)")
        chunk_size = int(chunk_size)
        if chunk_size <= 0:
            raise ValueError("chunk_size must be positive")
        kw = dict(patience=patience, threshold=threshold, debounce_time=debounce_time)
        self.reset()
        n_chunks = -(-len(pcm) // chunk_size)
        out = {n: np.zeros(n_chunks, np.float32) for n in self.models}

        def keep(t, res):
            for n in out:
                out[n][t] = res.scores.get(n, 0.0)

        n_full = len(pcm) // chunk_size
        grid = (self.preprocessor is None and chunk_size % 8 == 0 and n_full > 0
                and all(chunk_size <= self.e2e_clip_samples[n] and (-self.e2e_clip_samples[n]) % chunk_size % 8 == 0 for n in self.models))
        if self.is_cascade:
            # a gate + verifier pair whose verifier session scores only the windows the gate opens (HipSession.run_recording_cascade)
            gate_s, ver_s = self.models.get(self.gate_name), self.models.get(self.model_name)
            batch = bool(grid and len(self.models) == 2 and gate_s is not None and ver_s is not None
                         and hasattr(ver_s, "run_recording_cascade") and hasattr(ver_s, "cascade_accepts") and ver_s.cascade_accepts(gate_s))
        else:
            batch = grid and all(hasattr(s, "run_recording") for s in self.models.values())
        if not batch:
            for t in range(n_chunks):
                keep(t, self.predict(pcm[t * chunk_size:(t + 1) * chunk_size], **kw))
            return out
        xi = pcm if pcm.dtype == np.int16 else pcm.astype(np.int16)
        full = np.ascontiguousarray(xi[:n_full * chunk_size])
        raw, first = {}, {}
        if self.bank:                                             # one call: the recording uploaded once, each pass's frontend run once
            clip = self.e2e_clip_samples[self.model_name]
            got = dict(zip(self.models, self.bank[0].run_recording_bank(self.bank, full, hop=chunk_size, offset=(-clip) % chunk_size)))
        if self.is_cascade:
            # the device opens a superset of what predict() would: every window whose RAW gate probability reaches the threshold.  The
            # loop below still gates on the gate's post-warm-up score (_gate_closed) and zeroes the verifier wherever that says closed.
            clip = self.e2e_clip_samples[self.model_name]
            pair = ver_s.run_recording_cascade(gate_s, full, hop=chunk_size, offset=(-clip) % chunk_size,
                                               gate_threshold=self.cascade_config["gate_threshold"])
            got = dict(zip((self.gate_name, self.model_name), pair))
        for n, s in self.models.items():
            clip = self.e2e_clip_samples[n]
            first[n] = -(-clip // chunk_size) - 1                 # the chunk that fills the window
            if self.is_cascade or self.bank:
                raw[n] = np.asarray(got[n], np.float32).reshape(-1)
            else:
                raw[n] = np.asarray(s.run_recording(full, hop=chunk_size, offset=(-clip) % chunk_size), np.float32).reshape(-1)
            assert len(raw[n]) == max(0, n_full - first[n]), (len(raw[n]), n_full, first[n])
        for t in range(n_full):                                   # predict()'s bookkeeping, the scores looked up
            current = {}
            for n in self.models:
                if t >= first[n] and self._gate_closed(n, current):
                    current[n] = 0.0
                    self.raw_scores[n] = 0.0
                    continue
                score = float(raw[n][t - first[n]]) if t >= first[n] else 0.0
                self.raw_scores[n] = score
                if len(self.prediction_buffer.get(n, ())) < N_WARMUP_PREDICTIONS:
                    score = 0.0
                current[n] = score
            self._post_filters(current, patience, threshold, debounce_time, chunk_size)
            for n, v in current.items():
                self._history(n).append(v)
                self.post_processed_scores[n] = v
                out[n][t] = v
        for w in {id(w): w for w in self._windows.values()}.values():      # (a bank's models share one window)
            w.push(full)
        if n_full < n_chunks:                                     # a last, shorter chunk: its window starts off the grid
            keep(n_full, self.predict(pcm[n_full * chunk_size:], **kw))
        return out

    def reset(self):
        """New stream: clear histories, windows and scores (:719-733)."""
        self.prediction_buffer.clear()
        if self.preprocessor is not None:
            self.preprocessor.reset()
        for name in self.raw_scores:
            self.raw_scores[name] = 0.0
            self.post_processed_scores[name] = 0.0
        for w in self._windows.values():
            w.clear()

    # reference-compatible view of the e2e buffers
    @property
    def e2e_buffer_samples(self) -> Dict[str, int]:
        return {n: w.filled for n, w in self._windows.items()}


def _filter_streams(score: np.ndarray, history: np.ndarray, patience: int, threshold: float, debounce_time: float, hop: int):
    """Patience or debounce (:1034-1064) on one model's scores [S] in place, against its history [rows][S] (most recent last)."""
    nz = score != 0.0
    if patience:
        if history.shape[0] < patience:
            score[nz] = 0.0
        else:
            tail = history[-(patience - 1):] if patience > 1 else history
            hits = (tail >= threshold).sum(axis=0) + (score >= threshold)
            score[nz & (hits < patience)] = 0.0
    else:
        k = int(math.ceil(debounce_time / (hop / 16000.0)))
        recent = (history[-k:] >= threshold).any(axis=0) if history.shape[0] else np.zeros(len(score), bool)
        score[nz & (score >= threshold) & recent] = 0.0


def _filter_by_count(score: np.ndarray, history: np.ndarray, cnt: np.ndarray, ids: np.ndarray, patience: int, threshold: float,
                     debounce_time: float, hop: int):
    """_filter_streams for streams that each hold their own number of scores: score [n] in place for the streams ids [n], whose latest
    cnt[i] scores are the last rows of history [PREDICTION_HISTORY][S].  Streams that hold equally many share one call of the filter."""
    for c in np.unique(cnt):
        g = np.flatnonzero(cnt == c)
        part = score[g]
        _filter_streams(part, history[PREDICTION_HISTORY - int(c):, ids[g]], patience, threshold, debounce_time, hop)
        score[g] = part


class StreamBatch:
    """S lock-step audio streams scored together on one GPU: the batched form of the E2E branch of
    ``NanoInterpreter.predict`` (nanointerpreter.py:735-814).  The raw-audio windows live in device rings
    (``nww_stream_*``); per-stream filter state stays here on the host, vectorised over streams:
    raw score 0 until a stream has a full window (:785-786), first five predictions zeroed (:789-790),
    patience / debounce (:1034-1064), 30-entry prediction history (:1002).  Every stream receives exactly
    ``hop`` new samples per push (streams never migrate)."""

    def __init__(self, backend, n_streams: int, window_samples: int = 16000, hop_samples: int = HOP_SAMPLES,
                 name: str = "model"):
        self.backend, self.S, self.window, self.hop, self.name = backend, int(n_streams), int(window_samples), int(hop_samples), name
        backend.stream_open(self.S, self.window, self.hop)
        self.reset(_device=False)

    def reset(self, _device: bool = True):
        if _device:
            self.backend.stream_reset()
        self.history = np.zeros((0, self.S), np.float32)          # most recent last, at most PREDICTION_HISTORY rows
        self.raw_scores = np.zeros(self.S, np.float32)
        self.post_processed_scores = np.zeros(self.S, np.float32)

    def push(self, chunk: np.ndarray, patience: int = 0, threshold: float = 0.0, debounce_time: float = 0.0) -> np.ndarray:
        """chunk int16 [S, hop] -> post-processed scores [S] (what DetectionResult.score is per stream)."""
        if not isinstance(chunk, np.ndarray):
            raise ValueError("Input audio `x` must be a Numpy array.")
        _, probs = self.backend.stream_push(chunk)
        raw = probs.astype(np.float32)
        self.raw_scores = raw
        score = raw.copy()
        if self.history.shape[0] < N_WARMUP_PREDICTIONS:
            score[:] = 0.0
        if patience or debounce_time > 0:
            if not threshold:
                raise ValueError("`threshold` must be provided when using `patience` or `debounce_time`.")
            if patience and debounce_time > 0:
                raise ValueError("`patience` and `debounce_time` cannot be used together.")
            _filter_streams(score, self.history, patience, threshold, debounce_time, self.hop)
        self.history = np.vstack([self.history, score[None]])[-PREDICTION_HISTORY:]
        self.post_processed_scores = score
        return score

    def close(self):
        self.backend.stream_close()


class StreamPool:
    """S audio streams on one GPU that push, join and leave on their own: what a server scoring many clients needs of ``StreamBatch``.
    A push names the streams that have a chunk this tick (``nww_stream_push_some``); a client that connects takes a free slot through
    ``attach`` and inherits nothing of the slot's previous client - neither audio nor filter state; one whose packet is late is left out
    of the tick.  Every slot behaves exactly like a ``StreamBatch`` of one stream fed that slot's chunks: raw score 0 until the slot's own
    window is full, its first five predictions zeroed, patience / debounce against its own 30-entry history."""

    def __init__(self, backend, n_streams: int, window_samples: int = 16000, hop_samples: int = HOP_SAMPLES, name: str = "model"):
        self.backend, self.S, self.window, self.hop, self.name = backend, int(n_streams), int(window_samples), int(hop_samples), name
        backend.stream_open(self.S, self.window, self.hop)
        self.attached = np.zeros(self.S, bool)
        self.history = np.zeros((PREDICTION_HISTORY, self.S), np.float32)      # per stream: its latest `count` scores in the last rows
        self.count = np.zeros(self.S, np.int64)
        self.raw_scores = np.zeros(self.S, np.float32)
        self.post_processed_scores = np.zeros(self.S, np.float32)

    def _ids(self, ids) -> np.ndarray:
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if len(ids) and (ids[0] < 0 or ids[-1] >= self.S or (np.diff(ids) <= 0).any()):
            raise ValueError(f"stream ids must be strictly ascending numbers in [0, {self.S})")
        return ids

    def attach(self) -> int:
        """A new client: the lowest free slot, reset (device ring and filter state)."""
        free = np.flatnonzero(~self.attached)
        if not len(free):
            raise RuntimeError(f"all {self.S} stream slots are taken")
        slot = int(free[0])
        self.reset([slot])
        self.attached[slot] = True
        return slot

    def detach(self, slot: int):
        if not 0 <= int(slot) < self.S or not self.attached[int(slot)]:
            raise ValueError(f"slot {slot} is not attached")
        self.attached[int(slot)] = False

    def reset(self, ids=None):
        """New session for the listed streams (None: every stream, which also puts the batch back in lock-step)."""
        if ids is None:
            self.backend.stream_reset()
            ids = np.arange(self.S)
        else:
            ids = self._ids(ids)
            self.backend.stream_reset_some(ids)
        self.history[:, ids] = 0.0
        self.count[ids] = 0
        self.raw_scores[ids] = 0.0
        self.post_processed_scores[ids] = 0.0

    def push(self, ids, chunk: np.ndarray, patience: int = 0, threshold: float = 0.0, debounce_time: float = 0.0) -> np.ndarray:
        """ids: strictly ascending stream numbers [n]; chunk int16 [n, hop], row i for stream ids[i] -> post-processed scores [n]."""
        if not isinstance(chunk, np.ndarray):
            raise ValueError("Input audio `x` must be a Numpy array.")
        ids = self._ids(ids)
        _, probs = self.backend.stream_push_some(ids, chunk)
        raw = probs.astype(np.float32)
        self.raw_scores[ids] = raw
        score = raw.copy()
        cnt = self.count[ids]
        score[cnt < N_WARMUP_PREDICTIONS] = 0.0
        if patience or debounce_time > 0:
            if not threshold:
                raise ValueError("`threshold` must be provided when using `patience` or `debounce_time`.")
            if patience and debounce_time > 0:
                raise ValueError("`patience` and `debounce_time` cannot be used together.")
            _filter_by_count(score, self.history, cnt, ids, patience, threshold, debounce_time, self.hop)
        self.history[:-1, ids] = self.history[1:, ids]
        self.history[-1, ids] = score
        self.count[ids] = np.minimum(cnt + 1, PREDICTION_HISTORY)
        self.post_processed_scores[ids] = score
        return score

    def close(self):
        self.backend.stream_close()


class CascadeStreamBatch:
    """S lock-step streams through a gate + verifier pair (session.HipCascade): StreamBatch's filter state once per model, and the
    cascade rule of ``HipInterpreter.predict`` vectorised over streams.  Only the gate keeps a device ring; the verifier scores the
    windows of the streams whose RAW gate probability reaches the threshold (the device's select), and the host zeroes it wherever the
    gate's post-warm-up score is below the threshold (:660-669, 758-769) - so during the gate's first five predictions the verifier
    reports 0 for any positive threshold, as it does in the reference.  ``push`` returns {gate_name: scores [S], name: scores [S]},
    per stream what ``DetectionResult.scores`` holds."""

    def __init__(self, cascade, n_streams: int, window_samples: int = 16000, hop_samples: int = HOP_SAMPLES, gate_name: str = "gate",
                 name: str = "model"):
        if gate_name == name:
            raise ValueError("the gate and the verifier need two names")
        self.cascade, self.S, self.window, self.hop = cascade, int(n_streams), int(window_samples), int(hop_samples)
        self.gate_name, self.name = gate_name, name
        cascade.stream_open(self.S, self.window, self.hop)
        self.reset(_device=False)

    def reset(self, _device: bool = True):
        if _device:
            self.cascade.stream_reset()
        self.filled = 0
        self.history = {n: np.zeros((0, self.S), np.float32) for n in (self.gate_name, self.name)}
        self.raw_scores = {n: np.zeros(self.S, np.float32) for n in (self.gate_name, self.name)}
        self.post_processed_scores = {n: np.zeros(self.S, np.float32) for n in (self.gate_name, self.name)}
        self.n_open = 0

    def push(self, chunk: np.ndarray, patience: dict = {}, threshold: dict = {}, debounce_time: float = 0.0) -> Dict[str, np.ndarray]:
        """chunk int16 [S, hop] -> {name: post-processed scores [S]}; patience / threshold are keyed by model name, as in predict()"""
        if not isinstance(chunk, np.ndarray):
            raise ValueError("Input audio `x` must be a Numpy array.")
        if (patience or debounce_time > 0) and not threshold:
            raise ValueError("`threshold` must be provided when using `patience` or `debounce_time`.")
        if patience and debounce_time > 0:
            raise ValueError("`patience` and `debounce_time` cannot be used together.")
        gate_probs, _, probs, self.n_open = self.cascade.stream_push(chunk)
        self.filled += self.hop
        full = self.filled >= self.window
        out = {}
        for n, raw in ((self.gate_name, gate_probs), (self.name, probs)):
            raw = raw.astype(np.float32)
            if n == self.name and full:
                raw[~cascade_open(out[self.gate_name], self.cascade.gate_threshold)] = 0.0     # the gate's post-warm-up score decides
            self.raw_scores[n] = raw
            score = raw.copy()
            if self.history[n].shape[0] < N_WARMUP_PREDICTIONS:
                score[:] = 0.0
            out[n] = score
        final = {n: v.copy() for n, v in out.items()}
        for n, score in final.items():
            if n in patience:
                _filter_streams(score, self.history[n], int(patience[n]), threshold[n], 0.0, self.hop)
            elif debounce_time > 0 and n in threshold:
                _filter_streams(score, self.history[n], 0, threshold[n], debounce_time, self.hop)
            self.history[n] = np.vstack([self.history[n], score[None]])[-PREDICTION_HISTORY:]
            self.post_processed_scores[n] = score
        return final

    def close(self):
        self.cascade.stream_close()


class CascadeStreamPool(StreamPool):
    """StreamPool through a gate + verifier pair (session.HipCascade.stream_push_some): S streams that push, join and leave on their own,
    the verifier scoring only the listed streams the gate opens.  Every slot behaves exactly like a ``CascadeStreamBatch`` of one stream
    fed that slot's chunks: raw score 0 until the slot's own window is full, each model's first five predictions zeroed, the verifier
    zeroed wherever the gate's post-warm-up score is below the threshold, patience / debounce per model against the slot's own 30-entry
    history.  ``attach`` / ``detach`` are StreamPool's: a slot handed out inherits neither audio nor filter state.  ``push`` returns
    {gate_name: scores [n], name: scores [n]}."""

    def __init__(self, cascade, n_streams: int, window_samples: int = 16000, hop_samples: int = HOP_SAMPLES, gate_name: str = "gate",
                 name: str = "model"):
        if gate_name == name:
            raise ValueError("the gate and the verifier need two names")
        self.cascade, self.S, self.window, self.hop = cascade, int(n_streams), int(window_samples), int(hop_samples)
        self.gate_name, self.name = gate_name, name
        cascade.stream_open(self.S, self.window, self.hop)
        self.attached = np.zeros(self.S, bool)
        names = (gate_name, name)
        self.history = {n: np.zeros((PREDICTION_HISTORY, self.S), np.float32) for n in names}   # per stream: its latest `count` scores in the last rows
        self.count = np.zeros(self.S, np.int64)                 # one count for both models: every push scores both
        self.filled = np.zeros(self.S, np.int64)
        self.raw_scores = {n: np.zeros(self.S, np.float32) for n in names}
        self.post_processed_scores = {n: np.zeros(self.S, np.float32) for n in names}
        self.n_open = 0

    def reset(self, ids=None):
        """New session for the listed streams (None: every stream, which also puts the gate's batch back in lock-step)."""
        if ids is None:
            self.cascade.stream_reset()
            ids = np.arange(self.S)
        else:
            ids = self._ids(ids)
            self.cascade.stream_reset_some(ids)
        self.count[ids] = 0
        self.filled[ids] = 0
        for n in (self.gate_name, self.name):
            self.history[n][:, ids] = 0.0
            self.raw_scores[n][ids] = 0.0
            self.post_processed_scores[n][ids] = 0.0

    def push(self, ids, chunk: np.ndarray, patience: dict = {}, threshold: dict = {}, debounce_time: float = 0.0) -> Dict[str, np.ndarray]:
        """ids: strictly ascending stream numbers [n]; chunk int16 [n, hop], row i for stream ids[i] -> {name: post-processed scores [n]};
        patience / threshold are keyed by model name, as in predict()"""
        if not isinstance(chunk, np.ndarray):
            raise ValueError("Input audio `x` must be a Numpy array.")
        if (patience or debounce_time > 0) and not threshold:
            raise ValueError("`threshold` must be provided when using `patience` or `debounce_time`.")
        if patience and debounce_time > 0:
            raise ValueError("`patience` and `debounce_time` cannot be used together.")
        ids = self._ids(ids)
        gate_probs, _, probs, self.n_open = self.cascade.stream_push_some(ids, chunk)
        self.filled[ids] += self.hop
        full = self.filled[ids] >= self.window
        cnt = self.count[ids]
        out = {}
        for n, raw in ((self.gate_name, gate_probs), (self.name, probs)):
            raw = raw.astype(np.float32)
            if n == self.name:
                raw[~cascade_pool_open(out[self.gate_name], full, self.cascade.gate_threshold)] = 0.0   # the gate's post-warm-up score decides
            self.raw_scores[n][ids] = raw
            score = raw.copy()
            score[cnt < N_WARMUP_PREDICTIONS] = 0.0
            out[n] = score
        final = {n: v.copy() for n, v in out.items()}
        for n, score in final.items():
            if n in patience:
                _filter_by_count(score, self.history[n], cnt, ids, int(patience[n]), threshold[n], 0.0, self.hop)
            elif debounce_time > 0 and n in threshold:
                _filter_by_count(score, self.history[n], cnt, ids, 0, threshold[n], debounce_time, self.hop)
            self.history[n][:-1, ids] = self.history[n][1:, ids]
            self.history[n][-1, ids] = score
            self.post_processed_scores[n][ids] = score
        self.count[ids] = np.minimum(cnt + 1, PREDICTION_HISTORY)
        return final

    def close(self):
        self.cascade.stream_close()


class BankStreamPool(StreamPool):
    """StreamPool through a bank (session.HipBank.stream_push_some): S streams that push, join and leave on their own, every listed
    stream scored by all of the bank's models on one frontend pass.  Filter state is kept once per model - history, count, raw and
    post-processed scores, ``[model][stream]`` - and every (model, slot) behaves exactly like a ``StreamPool`` of that model alone fed
    that slot's chunks.  ``attach`` / ``detach`` are StreamPool's.  ``push`` returns {name: scores [n]}."""

    def __init__(self, bank, n_streams: int, window_samples: int = 16000, hop_samples: int = HOP_SAMPLES):
        self.bank, self.S, self.window, self.hop = bank, int(n_streams), int(window_samples), int(hop_samples)
        self.names = list(bank.names)
        bank.stream_open(self.S, self.window, self.hop)
        self.attached = np.zeros(self.S, bool)
        self.history = {n: np.zeros((PREDICTION_HISTORY, self.S), np.float32) for n in self.names}
        self.count = {n: np.zeros(self.S, np.int64) for n in self.names}
        self.raw_scores = {n: np.zeros(self.S, np.float32) for n in self.names}
        self.post_processed_scores = {n: np.zeros(self.S, np.float32) for n in self.names}

    def reset(self, ids=None):
        """New session for the listed streams (None: every stream, which also puts the leader's batch back in lock-step)."""
        if ids is None:
            self.bank.stream_reset()
            ids = np.arange(self.S)
        else:
            ids = self._ids(ids)
            self.bank.stream_reset_some(ids)
        for n in self.names:
            self.history[n][:, ids] = 0.0
            self.count[n][ids] = 0
            self.raw_scores[n][ids] = 0.0
            self.post_processed_scores[n][ids] = 0.0

    def push(self, ids, chunk: np.ndarray, patience: dict = {}, threshold: dict = {}, debounce_time: float = 0.0) -> Dict[str, np.ndarray]:
        """ids: strictly ascending stream numbers [n]; chunk int16 [n, hop], row i for stream ids[i] -> {name: post-processed scores [n]};
        patience / threshold are keyed by model name, as in predict()"""
        if not isinstance(chunk, np.ndarray):
            raise ValueError("Input audio `x` must be a Numpy array.")
        if (patience or debounce_time > 0) and not threshold:
            raise ValueError("`threshold` must be provided when using `patience` or `debounce_time`.")
        if patience and debounce_time > 0:
            raise ValueError("`patience` and `debounce_time` cannot be used together.")
        ids = self._ids(ids)
        got = self.bank.stream_push_some(ids, chunk)
        final = {}
        for n in self.names:
            raw = got[n][1].astype(np.float32)
            self.raw_scores[n][ids] = raw
            score = raw.copy()
            cnt = self.count[n][ids]
            score[cnt < N_WARMUP_PREDICTIONS] = 0.0
            if n in patience:
                _filter_by_count(score, self.history[n], cnt, ids, int(patience[n]), threshold[n], 0.0, self.hop)
            elif debounce_time > 0 and n in threshold:
                _filter_by_count(score, self.history[n], cnt, ids, 0, threshold[n], debounce_time, self.hop)
            self.history[n][:-1, ids] = self.history[n][1:, ids]
            self.history[n][-1, ids] = score
            self.count[n][ids] = np.minimum(cnt + 1, PREDICTION_HISTORY)
            self.post_processed_scores[n][ids] = score
            final[n] = score
        return final

    def close(self):
        self.bank.stream_close()
