"""Host-side mirror of the reference's session boundary, on top of the libnwwhip C-ABI.

``HipModel``   : create / load_state_dict / finalize / forward - one handle on one GPU.
``HipCascade`` : a gate and a verifier HipModel as a pair - the verifier runs on the windows the gate opens (nww_cascade_*).
``HipBank``    : several HipModels with identical mel frontends on ONE frontend pass - the first leads, the others run their heads (nww_bank_*).
``HipSession`` : duck-types ``onnxruntime.InferenceSession`` exactly as the reference uses it
                 (``get_inputs()[0].name/.shape`` and ``run(None, {"input": x}) -> [probs (B,1,1)]``;
                 reference: nanowakeword/interpreter/nanointerpreter.py:165-167,177-178,677,681,783;
                 in-tree precedent of a substitute backend: remote_verifier.py:490-648 ``_RemoteSession``).

Error behaviour follows the reference's conventions: ValueError for bad inputs,
KeyError/ValueError for state_dict problems, RuntimeError for device failures.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Optional

import numpy as np

from . import _lib
from .config import FrontendConfig, HeadConfig, RAW_HEADS, clip_samples, param_spec, recording_windows


class NwwError(RuntimeError):
    pass


_EXC = {1: ValueError, 2: KeyError, 3: ValueError, 4: NwwError, 5: NwwError, 6: NotImplementedError}


def _as_f32(a) -> np.ndarray:
    if hasattr(a, "detach"):           # torch tensor
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def torchaudio_tables(fe: FrontendConfig):
    """Hann window and mel filterbank exactly as torchaudio builds them (float32 torch ops):
    torch.hann_window(win_length) and torchaudio.functional.melscale_fbanks(norm=None,
    mel_scale="htk") - the tables T.MelSpectrogram carries at architectures.py:830-836.
    The C library's built-in tables evaluate the same formulas in double precision, which
    differs from this float32 evaluation by up to 1e-5 per coefficient (up to ~4e-3 dB on narrow low-frequency filters); use these
    (or the exported model's own buffers) when bit-level agreement with the reference matters."""
    import math
    import torch
    window = torch.hann_window(fe.win_length)
    n_freqs = fe.n_fft // 2 + 1
    all_freqs = torch.linspace(0, fe.sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + (fe.f_min / 700.0))
    m_max = 2595.0 * math.log10(1.0 + (fe.f_max / 700.0))
    m_pts = torch.linspace(m_min, m_max, fe.n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.max(torch.zeros(1), torch.min(down, up))
    return window.numpy().astype(np.float32), fb.numpy().astype(np.float32)


def score_recordings(forward_recording, recordings, window: int, hop: int = 1280, max_batch: int = 4096):
    """Several recordings through ONE forward_recording(pcm, window=, hop=, max_batch=) call: each is padded with zeros to a multiple of
    `hop`, so that every recording starts on the window grid of the concatenation; the windows that lie in one recording's own samples are
    kept, those that reach into the padding or the next recording dropped.  Returns [(logits, probs)] per recording, each what the
    recording scores alone."""
    recs = [HipModel._pcm1(r) for r in recordings]
    window, hop = int(window), int(hop)
    if not recs:
        return []
    starts, parts, at = [], [], 0
    for r in recs:
        pad = -len(r) % hop
        starts.append(at // hop)
        parts.append(r)
        if pad:
            parts.append(np.zeros(pad, np.int16))
        at += len(r) + pad
    logits, probs = forward_recording(np.concatenate(parts), window=window, hop=hop, max_batch=max_batch)
    out = []
    for r, i0 in zip(recs, starts):
        n = recording_windows(len(r), window, hop)
        out.append((logits[i0:i0 + n].copy(), probs[i0:i0 + n].copy()))
    return out


class HipModel:
    """One finalized head (+ frontend) on one GPU behind the C-ABI."""

    def __init__(self, head: HeadConfig, frontend: Optional[FrontendConfig] = None, device: int = 0,
                 state_dict: Optional[Mapping] = None, window=None, mel_fb=None, tables: str = "torchaudio",
                 conv_arith: Optional[str] = None, act_dtype: Optional[str] = None):
        """act_dtype="bf16": the BcResNet head stores the activations between its kernels as bf16 (BASELINE config 3 as written;
        float32 products and accumulation; logits then agree with the float32 reference to ~1e-2 instead of 1e-4 - 0.2 on all-zero
        PCM).  act_dtype="f16": the same tensors as scaled binary16 (same bytes, 11 significant bits: ~5e-3 on every test clip)."""
        self.lib = _lib.load_library()      # ImportError if the HIP extension is missing - no fallback
        self.head = head
        self.fe = frontend or FrontendConfig()
        self.device = device
        self.act_dtype = act_dtype
        self._h = C.c_void_p()
        cfg = _lib.make_config(head, self.fe, device, conv_arith=conv_arith, act_dtype=act_dtype)      # None: library defaults
        rc = self.lib.nww_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = self.lib.nww_last_error(None).decode()
            self._h = C.c_void_p()
            raise _EXC.get(rc, NwwError)(msg)
        self.finalized = False
        self._pitch_bank = None            # the augment.PitchBank whose ratios the handle holds (PitchBank.prepare)
        if window is None and mel_fb is None and tables == "torchaudio":
            try:
                window, mel_fb = torchaudio_tables(self.fe)
            except ImportError:       # no torch on this host: the C library's double-precision tables (<= 1e-5 per coefficient away)
                window = mel_fb = None
        if window is not None:
            self._load("frontend.window", _as_f32(window))
        if mel_fb is not None:
            self._load("frontend.mel_fb", _as_f32(mel_fb))
        if state_dict is not None:
            self.load_state_dict(state_dict)
            self.finalize()

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int):
        if rc != 0:
            raise _EXC.get(rc, NwwError)(self.lib.nww_last_error(self._h).decode())

    def _load(self, key: str, arr: np.ndarray):
        shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
        self._check(self.lib.nww_load_tensor(self._h, key.encode(), arr.ctypes.data_as(C.c_void_p), shape, arr.ndim, 0))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.nww_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def required_tensors(self):
        out = {}
        key, nd = C.c_char_p(), C.c_int32()
        shape = (C.c_int64 * 4)()
        for i in range(self.lib.nww_num_tensors(self._h)):
            self._check(self.lib.nww_tensor_info(self._h, i, C.byref(key), shape, C.byref(nd)))
            out[key.value.decode()] = tuple(int(shape[d]) for d in range(nd.value))
        return out

    def load_state_dict(self, sd: Mapping, strict: bool = True):
        """Accepts Model.state_dict() of the reference (torch tensors or numpy arrays)."""
        spec = param_spec(self.head)
        for k, v in sd.items():
            if k.endswith("num_batches_tracked") or k.startswith("model.mel_spec."):
                continue
            if k not in spec:
                if strict:
                    raise KeyError(f"Unexpected key(s) in state_dict: '{k}'")
                continue
            self._load(k, _as_f32(v))
        # exported E2E models carry their own frontend tables (ONNXSafeMelSpectrogram buffers)
        if "model.mel_spec.mel_fb" in sd:
            self._load("frontend.mel_fb", _as_f32(sd["model.mel_spec.mel_fb"]))
        if "model.mel_spec.real_basis" in sd:
            rb = _as_f32(sd["model.mel_spec.real_basis"])          # [201,1,400]; row k=0 is the padded window
            n_fft, wl = self.fe.n_fft, self.fe.win_length
            pad = (n_fft - wl) // 2
            self._load("frontend.window", np.ascontiguousarray(rb.reshape(rb.shape[0], -1)[0, pad:pad + wl]))
        return self

    def finalize(self):
        self._check(self.lib.nww_finalize(self._h))
        self.finalized = True
        return self

    # ------------------------------------------------------------------ host-array entry points
    def num_frames(self, n_samples: int) -> int:
        return int(self.lib.nww_num_frames(self._h, int(n_samples)))

    @staticmethod
    def _pcm(pcm) -> np.ndarray:
        if not isinstance(pcm, np.ndarray):
            raise ValueError("Input audio `x` must be a Numpy array.")     # nanointerpreter.py:628-629
        if pcm.dtype != np.int16:
            raise ValueError("PCM must be int16")
        if pcm.ndim == 1:
            pcm = pcm[None]
        if pcm.ndim != 2:
            raise ValueError("PCM must have shape (B, N) or (N,)")
        return np.ascontiguousarray(pcm)

    def frontend(self, pcm, return_power: bool = False):
        """int16 [B,N] -> log-mel dB float32 [B, n_mels, frames] (+ mel power); for the raw-PCM heads (e2e_quartznet, e2e_cnn) the learned raw-PCM
        frontend's output [B, channels, rows] (no mel power there)."""
        pcm = self._pcm(pcm)
        B, N = pcm.shape
        T = self.num_frames(N)
        raw = self.head.model_type in RAW_HEADS
        if T <= 0 and raw:
            raise ValueError(f"a clip needs at least one sample (got {N})")
        if T <= 0:
            raise ValueError(f"Input clip of {N} samples is too short (n_fft={self.fe.n_fft}, center={self.fe.center})")
        if raw and return_power:
            raise ValueError("the raw-PCM frontend has no mel power")
        out = np.empty((B, self.head.input_shape[1] if raw else self.fe.n_mels, T), np.float32)
        pw = np.empty_like(out) if return_power else None
        fr = C.c_int32()
        self._check(self.lib.nww_frontend_ex(self._h, pcm.ctypes.data_as(C.c_void_p), B, N, out.ctypes.data_as(C.c_void_p),
                                             pw.ctypes.data_as(C.c_void_p) if return_power else None, C.byref(fr)))
        assert fr.value == T
        return (out, pw) if return_power else out

    def forward_pcm(self, pcm):
        """int16 [B,N] -> (logits [B], probs [B])."""
        pcm = self._pcm(pcm)
        B, N = pcm.shape
        logits, probs = np.empty(B, np.float32), np.empty(B, np.float32)
        self._check(self.lib.nww_forward_pcm(self._h, pcm.ctypes.data_as(C.c_void_p), B, N,
                                             logits.ctypes.data_as(C.c_void_p), probs.ctypes.data_as(C.c_void_p)))
        return logits, probs

    # ------------------------------------------------------------------ recording scoring (nww_recording_*, nww_forward_recording*)
    @staticmethod
    def _pcm1(pcm) -> np.ndarray:
        if not isinstance(pcm, np.ndarray):
            raise ValueError("Input audio `x` must be a Numpy array.")
        if pcm.dtype != np.int16 or pcm.ndim != 1:
            raise ValueError("a recording must be a one-dimensional int16 array")
        if pcm.size >= 2 ** 31:
            raise ValueError("a recording holds at most 2**31 - 1 samples per call")
        return np.ascontiguousarray(pcm)

    @property
    def clip_samples(self) -> int:
        """the clip length the head was built for (config.clip_samples)"""
        return clip_samples(self.head, self.fe)

    def _rec_count(self, n: int, window: int, hop: int) -> int:
        nw = int(self.lib.nww_recording_windows(self._h, int(n), int(window), int(hop)))
        if nw < 0:
            self._check(-nw)
        return nw

    def recording_route(self, window: Optional[int] = None, hop: int = 1280) -> int:
        """1: the shared-frame route scores this (window, hop), 0: the strided route (nww_recording_route)"""
        r = int(self.lib.nww_recording_route(self._h, int(self.clip_samples if window is None else window), int(hop)))
        if r < 0:
            self._check(-r)
        return r

    def describe_recording(self, window: Optional[int] = None, hop: int = 1280) -> str:
        """The launches of one pass of forward_recording at this (window, hop), one per line: the route's frontend launches, then the
        head's lines of describe_plan()."""
        window = int(self.clip_samples if window is None else window)
        raw = self.head.model_type in RAW_HEADS
        if self.recording_route(window, hop) and raw:
            fe = ["raw_x3:pool - the pass's span of (B - 1) * %d + %d samples as one clip, rows-major" % (hop, window),
                  "raw_x3:edge rows - the rows of every window's last frontend stage that see its own zero padding",
                  "rec_assemble:pool -> [B][rows][channels] (shared-frame route)"]
        elif self.recording_route(window, hop):
            fe = ["frontend:pool - the pass's span of (B - 1) * %d + %d samples as one clip, frames-major" % (hop, window),
                  "frontend:edge frames - the frames of every window that touch its own reflect padding (none without centring)",
                  "rec_assemble:pool -> [B][frames][n_mels] (shared-frame route)"]
        else:
            fe = ["%s - every frame of every window, row_stride = %d (strided route)" % (l, hop)
                  for l in self.describe_plan().strip().split("\n") if l.startswith("frontend:")]
        return "\n".join(fe + [l for l in self.describe_plan().strip().split("\n") if not l.startswith("frontend:")]) + "\n"

    def forward_recording(self, pcm, window: Optional[int] = None, hop: int = 1280, offset: int = 0, max_batch: int = 4096):
        """int16 [N] -> (logits [nW], probs [nW]) of every window pcm[offset + i * hop : offset + i * hop + window]; each bit-identical to
        forward_pcm on that window (in batches of the passes' sizes).  The recording goes to the device once, never as windows."""
        pcm = self._pcm1(pcm)
        window = int(self.clip_samples if window is None else window)
        if offset < 0:
            raise ValueError("offset must not be negative")
        x = pcm[min(int(offset), len(pcm)):]
        nw = self._rec_count(len(x), window, hop)
        assert nw == recording_windows(len(pcm), window, hop, min(int(offset), len(pcm)))
        logits, probs = np.empty(nw, np.float32), np.empty(nw, np.float32)
        if nw:
            n_out = C.c_int32()
            self._check(self.lib.nww_forward_recording(self._h, x.ctypes.data_as(C.c_void_p), len(x), window, int(hop), int(max_batch),
                                                       logits.ctypes.data_as(C.c_void_p), probs.ctypes.data_as(C.c_void_p), C.byref(n_out)))
            assert n_out.value == nw
        return logits, probs

    def poison_recording_workspace(self, value: float = 1e30) -> None:
        """Test instrument (nww_recording_poison): the shared route's pool and the dense head input hold `value` everywhere."""
        self._check(self.lib.nww_recording_poison(self._h, float(value)))

    def forward_recordings(self, recordings, window: Optional[int] = None, hop: int = 1280, max_batch: int = 4096):
        """list of int16 [N_i] -> [(logits, probs)] per recording, scored together (score_recordings): windows never mix two recordings"""
        return score_recordings(self.forward_recording, recordings, int(self.clip_samples if window is None else window), hop, max_batch)

    def forward_recording_dev(self, pcm_ptr: int, n_samples: int, window: int, hop: int, logits_ptr: int, probs_ptr: int = 0,
                              max_batch: int = 4096, stream: int = 0) -> int:
        """Raw device pointers; enqueues on `stream`, does not synchronise.  Returns the number of windows written."""
        nw = self._rec_count(n_samples, window, hop)
        if nw:
            self._check(self.lib.nww_forward_recording_dev(self._h, C.c_void_p(pcm_ptr), int(n_samples), int(window), int(hop), int(max_batch),
                                                           C.c_void_p(logits_ptr) if logits_ptr else None,
                                                           C.c_void_p(probs_ptr) if probs_ptr else None,
                                                           C.c_void_p(stream) if stream else None))
        return nw

    @property
    def feature_clamp(self) -> float:
        """+-bound the plan assumes on (and clamps) the head's input features; 0.0 when nothing is clamped (nww_feature_clamp)"""
        return float(self.lib.nww_feature_clamp(self._h))

    def forward_features(self, feats, return_embedding: bool = False):
        """float32 [B,T,F] -> (logits [B], probs [B][, embedding [B,E]])."""
        feats = np.ascontiguousarray(np.asarray(feats), dtype=np.float32)
        if feats.ndim == 2:
            feats = feats[None]
        if feats.ndim != 3 or tuple(feats.shape[1:]) != tuple(self.head.input_shape):
            raise ValueError(f"features must have shape (B, {self.head.input_shape[0]}, {self.head.input_shape[1]}), got {feats.shape}")
        B = feats.shape[0]
        clamp = self.feature_clamp
        if clamp > 0.0 and feats.size and float(np.abs(feats).max()) > clamp:
            import warnings
            why = "16-bit activation storage (act_dtype)" if self.act_dtype not in (None, "f32") else "the default arithmetic (conv_arith='f16x3')"
            warnings.warn(f"features reach {float(np.abs(feats).max()):.4g}: {why} clamps the head input to "
                          f"+-{clamp:g} (log-mel dB never gets there; the reference does not clamp) - pass conv_arith='bf16x6' and act_dtype=None for unbounded features",
                          RuntimeWarning, stacklevel=2)
        logits, probs = np.empty(B, np.float32), np.empty(B, np.float32)
        emb = np.empty((B, self.head.embedding_dim), np.float32) if return_embedding else None
        self._check(self.lib.nww_forward_features_ex(self._h, feats.ctypes.data_as(C.c_void_p), B,
                                                     logits.ctypes.data_as(C.c_void_p), probs.ctypes.data_as(C.c_void_p),
                                                     emb.ctypes.data_as(C.c_void_p) if return_embedding else None))
        return (logits, probs, emb) if return_embedding else (logits, probs)

    # ------------------------------------------------------------------ device-pointer entry points (torch tensors as plumbing)
    def reserve(self, B: int, N: int = 0):
        self._check(self.lib.nww_reserve(self._h, int(B), int(N)))

    def forward_pcm_dev(self, pcm_ptr: int, B: int, N: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0):
        """Raw device pointers (e.g. torch.Tensor.data_ptr()); enqueues on `stream`, does not synchronise."""
        self._check(self.lib.nww_forward_pcm_dev(self._h, C.c_void_p(pcm_ptr), B, N, C.c_void_p(logits_ptr),
                                                 C.c_void_p(probs_ptr) if probs_ptr else None,
                                                 C.c_void_p(stream) if stream else None))

    def frontend_dev(self, pcm_ptr: int, B: int, N: int, out_ptr: int, frames_major: bool = False, stream: int = 0):
        self._check(self.lib.nww_frontend_dev(self._h, C.c_void_p(pcm_ptr), B, N, C.c_void_p(out_ptr), int(frames_major),
                                              C.c_void_p(stream) if stream else None))

    def forward_features_dev(self, feats_ptr: int, B: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0):
        self._check(self.lib.nww_forward_features_dev(self._h, C.c_void_p(feats_ptr), B, C.c_void_p(logits_ptr),
                                                      C.c_void_p(probs_ptr) if probs_ptr else None,
                                                      C.c_void_p(stream) if stream else None))

    # ------------------------------------------------------------------ clips mixed on the device (nww_mix_*, augment.py)
    def rir_prepare_dev(self, irs_ptr: int, ir_off, ir_len, N: int, M: int, spectra_ptr: int, stream: int = 0):
        """nww_rir_prepare_dev: float32 responses back to back at irs_ptr (host tables ir_off int64 / ir_len int32, samples) -> their
        spectra float32 [K, M] at spectra_ptr, for clips of N samples at transform size M - or, with M = augment.RIR_SEGMENTED, the
        augment.rir_spectra_floats(...) values of the segmented route.  Synchronises `stream`."""
        off, ln = np.ascontiguousarray(ir_off, np.int64), np.ascontiguousarray(ir_len, np.int32)
        if off.ndim != 1 or off.shape != ln.shape:
            raise ValueError("ir_off and ir_len must be one-dimensional and of one length")
        self._check(self.lib.nww_rir_prepare_dev(self._h, C.c_void_p(irs_ptr), off.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), len(off),
                                                 int(N), int(M), C.c_void_p(spectra_ptr), C.c_void_p(stream) if stream else None))

    def _rir_args(self, irs, ir_ids, B: int, N: int):
        """(spectra pointer, n_irs, M, the RIR_ITEM table) of a call's irs / ir_ids, or None without them (augment.IrArena, prepared here)"""
        if irs is None and ir_ids is None:
            return None
        if irs is None or ir_ids is None:
            raise ValueError("irs (an augment.IrArena) and ir_ids (one response id per item, -1: none) go together")
        from .augment import as_rir_items
        if int(N) != irs.N:
            raise ValueError(f"the IrArena was prepared for clips of {irs.N} samples, not {int(N)}")
        rt = as_rir_items(ir_ids, B)
        irs.prepare(self)
        return C.c_void_p(irs.spectra_ptr), irs.n, irs.M, rt

    def pitch_set_ratios(self, num, den):
        """nww_pitch_set_ratios: the ratios num[k] / den[k] a call's pitch ids name (augment.PitchBank does this); waits for the device"""
        num, den = np.ascontiguousarray(num, np.int32), np.ascontiguousarray(den, np.int32)
        if num.ndim != 1 or num.shape != den.shape:
            raise ValueError("num and den must be one-dimensional and of one length")
        self._check(self.lib.nww_pitch_set_ratios(self._h, num.ctypes.data_as(C.c_void_p), den.ctypes.data_as(C.c_void_p), len(num)))
        self._pitch_bank = None

    def _pitch_args(self, pitch, pitch_ids, B: int):
        """the PITCH_ITEM table of a call's pitch / pitch_ids, or None without them (augment.PitchBank, set on this model here)"""
        if pitch is None and pitch_ids is None:
            return None
        if pitch is None or pitch_ids is None:
            raise ValueError("pitch (an augment.PitchBank) and pitch_ids (one ratio id per item, -1: none) go together")
        from .augment import as_pitch_items
        pt = as_pitch_items(pitch_ids, B)
        pitch.prepare(self)
        return pt

    def _mix_call(self, form: str, arena, arena_samples: int, items, N: int, rest, rir, pt):
        """nww_mix<form>, nww_mix_rir<form> or nww_mix_aug<form> - the first that takes the tables given; `rest` are the call's arguments
        behind N"""
        head = [self._h, arena, int(arena_samples)]
        tabs = [items.ctypes.data_as(C.c_void_p)]
        if rir is not None or pt is not None:
            head += list(rir[:3]) if rir is not None else [None, 0, 0]
            tabs.append(rir[3].ctypes.data_as(C.c_void_p) if rir is not None else None)
        if pt is not None:
            tabs.append(pt.ctypes.data_as(C.c_void_p))
        fn = getattr(self.lib, "nww_mix" + ("_aug" if pt is not None else "_rir" if rir is not None else "") + form)
        self._check(fn(*head, *tabs, len(items), int(N), *rest))

    def mix_dev(self, arena_ptr: int, arena_samples: int, items, N: int, out_ptr: int, stream: int = 0, irs=None, ir_ids=None, pitch=None,
                pitch_ids=None):
        """Raw device pointers; `items` is a host table of augment.MIX_ITEM.  int16 out [B, N]; enqueues on `stream`, does not synchronise.
        With `irs` (an augment.IrArena) and `ir_ids` every clip with an id >= 0 is convolved with that response (nww_mix_rir_dev); with
        `pitch` (an augment.PitchBank) and `pitch_ids` every clip with an id >= 0 is shifted by that ratio first (nww_mix_aug_dev)."""
        from .augment import as_items
        items = as_items(items)
        st = C.c_void_p(stream) if stream else None
        rir, pt = self._rir_args(irs, ir_ids, len(items), N), self._pitch_args(pitch, pitch_ids, len(items))
        self._mix_call("_dev", C.c_void_p(arena_ptr), arena_samples, items, N, [C.c_void_p(out_ptr), st], rir, pt)

    def forward_mixed_dev(self, arena_ptr: int, arena_samples: int, items, N: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0, irs=None,
                          ir_ids=None, pitch=None, pitch_ids=None):
        """mix_dev into the handle's PCM staging, then forward_pcm_dev's path on it; does not synchronise."""
        from .augment import as_items
        items = as_items(items)
        st, pp = C.c_void_p(stream) if stream else None, C.c_void_p(probs_ptr) if probs_ptr else None
        rir, pt = self._rir_args(irs, ir_ids, len(items), N), self._pitch_args(pitch, pitch_ids, len(items))
        self._mix_call("_forward_pcm_dev", C.c_void_p(arena_ptr), arena_samples, items, N, [C.c_void_p(logits_ptr), pp, st], rir, pt)

    def frontend_mixed_dev(self, arena_ptr: int, arena_samples: int, items, N: int, out_ptr: int, frames_major: bool = False, stream: int = 0,
                           irs=None, ir_ids=None, pitch=None, pitch_ids=None):
        """mix_dev into the handle's PCM staging, then frontend_dev's path on it; does not synchronise."""
        from .augment import as_items
        items = as_items(items)
        st = C.c_void_p(stream) if stream else None
        rir, pt = self._rir_args(irs, ir_ids, len(items), N), self._pitch_args(pitch, pitch_ids, len(items))
        self._mix_call("_frontend_dev", C.c_void_p(arena_ptr), arena_samples, items, N, [C.c_void_p(out_ptr), int(frames_major), st], rir, pt)

    def mix(self, arena, items, N: int, irs=None, ir_ids=None, pitch=None, pitch_ids=None) -> np.ndarray:
        """The clips of `items` (augment.mix_items / draw_mix_items) mixed out of `arena` -> int16 [B, N].  A device-resident
        augment.ClipArena is read where it lies; a host arena (ClipArena(device=None) or an int16 array) is uploaded by the call.
        `irs` (an augment.IrArena) and `ir_ids` (augment.draw_rir_ids; -1: none) send clips through impulse responses; `pitch` (an
        augment.PitchBank) and `pitch_ids` (augment.draw_pitch_ids; -1: none) shift them in pitch before that."""
        from .augment import as_items
        items = as_items(items)
        B, N = len(items), int(N)
        rir, pt = self._rir_args(irs, ir_ids, B, N), self._pitch_args(pitch, pitch_ids, B)
        host = arena if isinstance(arena, np.ndarray) else arena.host
        if host is not None:
            if host.dtype != np.int16 or host.ndim != 1:
                raise ValueError("a host arena must be a one-dimensional int16 array")
            host = np.ascontiguousarray(host)
            out = np.empty((B, max(N, 0)), np.int16)
            self._mix_call("", host.ctypes.data_as(C.c_void_p), host.size, items, N, [out.ctypes.data_as(C.c_void_p)], rir, pt)
            return out
        import torch
        out = torch.empty((B, max(N, 0)), dtype=torch.int16, device=f"cuda:{self.device}")
        self.mix_dev(arena.ptr, arena.samples, items, N, out.data_ptr(), irs=irs, ir_ids=ir_ids, pitch=pitch, pitch_ids=pitch_ids)
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy()

    def forward_mixed(self, arena, items, N: int, irs=None, ir_ids=None, pitch=None, pitch_ids=None):
        """(logits [B], probs [B]) of the clips mix() gives, bit-identical to forward_pcm(mix(arena, items, N)); the clips stay on the device."""
        import torch
        from .augment import as_items
        items = as_items(items)
        out = torch.zeros((2, len(items)), dtype=torch.float32, device=f"cuda:{self.device}")
        self.forward_mixed_dev(arena.ptr, arena.samples, items, N, out[0].data_ptr(), out[1].data_ptr(), irs=irs, ir_ids=ir_ids, pitch=pitch,
                               pitch_ids=pitch_ids)
        torch.cuda.synchronize(self.device)
        res = out.cpu().numpy()
        return res[0].copy(), res[1].copy()

    # ------------------------------------------------------------------ recordings at their own sample rate (nww_resample_*, augment.py)
    def resample_set_ratios(self, num, den):
        """nww_resample_set_ratios: the ratios num[k] / den[k] (source rate over target rate) a table's rate_id names, at most 16;
        waits for the device"""
        num, den = np.ascontiguousarray(num, np.int32), np.ascontiguousarray(den, np.int32)
        if num.ndim != 1 or num.shape != den.shape:
            raise ValueError("num and den must be one-dimensional and of one length")
        self._check(self.lib.nww_resample_set_ratios(self._h, num.ctypes.data_as(C.c_void_p), den.ctypes.data_as(C.c_void_p), len(num)))

    def resample_dev(self, src_ptr: int, src_values: int, src_format: int, items, dst_ptr: int, dst_values: int, dst_format: int, stream: int = 0):
        """Raw device pointers; `items` is a host table of augment.RESAMPLE_ITEM, the formats are augment.PCM_S16 / PCM_F32.  Enqueues on
        `stream`, does not synchronise."""
        from .augment import as_resample_items
        items = as_resample_items(items)
        self._check(self.lib.nww_resample_dev(self._h, C.c_void_p(src_ptr), int(src_values), int(src_format), items.ctypes.data_as(C.c_void_p),
                                              len(items), C.c_void_p(dst_ptr), int(dst_values), int(dst_format), C.c_void_p(stream) if stream else None))

    def resample(self, recordings, rates, dst_hz: int = 16000, dtype=np.int16, chunk_bytes: int = 64 << 20):
        """Recordings - arrays [frames] or [frames, channels], int16 or float32 in units of full scale, each with its sample rate in
        `rates` - downmixed and brought to dst_hz on the device -> one host array per recording, int16 or (dtype=np.float32, what an
        augment.IrArena takes) float32 in units of full scale.  A recording at dst_hz is downmixed and converted only."""
        from .augment import PCM_F32, PCM_S16, resample_plan
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.int16), np.dtype(np.float32)):
            raise ValueError("dtype must be int16 or float32")
        recs, lengths, chunks = resample_plan(recordings, rates, dst_hz, chunk_bytes)
        out = []
        for ch in chunks:
            src = np.concatenate([r.ravel() for r in recs[ch["lo"]:ch["hi"]]])
            dst = np.empty(int(lengths[ch["lo"]:ch["hi"]].sum()), dtype)
            if ch["ratios"]:
                self.resample_set_ratios([a for a, _ in ch["ratios"]], [b for _, b in ch["ratios"]])
            self._check(self.lib.nww_resample(self._h, src.ctypes.data_as(C.c_void_p), src.size, ch["format"], ch["items"].ctypes.data_as(C.c_void_p),
                                              len(ch["items"]), dst.ctypes.data_as(C.c_void_p), dst.size, PCM_F32 if dtype == np.float32 else PCM_S16))
            out += [dst[o:o + n].copy() for o, n in zip(ch["items"]["dst_off"].tolist(), lengths[ch["lo"]:ch["hi"]].tolist())]
        return out

    # ------------------------------------------------------------------ batched streaming (rings on the device)
    def stream_open(self, n_streams: int, window_samples: int = 16000, hop_samples: int = 1280):
        self._check(self.lib.nww_stream_open(self._h, int(n_streams), int(window_samples), int(hop_samples)))
        self._stream = (int(n_streams), int(window_samples), int(hop_samples))

    def stream_push(self, chunk):
        """chunk int16 [S, hop] -> (logits [S], probs [S]); zeros until every stream has a full window."""
        S, W, hop = self._stream
        chunk = self._pcm(chunk)
        if chunk.shape != (S, hop):
            raise ValueError(f"chunk must have shape ({S}, {hop}), got {chunk.shape}")
        logits, probs = np.empty(S, np.float32), np.empty(S, np.float32)
        self._check(self.lib.nww_stream_push(self._h, chunk.ctypes.data_as(C.c_void_p), logits.ctypes.data_as(C.c_void_p),
                                             probs.ctypes.data_as(C.c_void_p)))
        return logits, probs

    def stream_push_dev(self, chunk_ptr: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0):
        self._check(self.lib.nww_stream_push_dev(self._h, C.c_void_p(chunk_ptr), C.c_void_p(logits_ptr),
                                                 C.c_void_p(probs_ptr) if probs_ptr else None,
                                                 C.c_void_p(stream) if stream else None))

    def stream_reset(self):
        self._check(self.lib.nww_stream_reset(self._h))

    def stream_filled(self, s: Optional[int] = None) -> int:
        """samples seen since open / reset: of the batch (streams in lock-step), or of stream `s` alone"""
        if s is None:
            return int(self.lib.nww_stream_filled(self._h))
        return int(self.lib.nww_stream_filled_of(self._h, int(s)))

    def stream_filled_of(self, s: int) -> int:
        """samples stream `s` has seen since open / its last reset; NwwError on a handle that has no open stream batch (a bank's follower)"""
        self.stream_pool_stats()
        return int(self.lib.nww_stream_filled_of(self._h, int(s)))

    def stream_close(self):
        self._check(self.lib.nww_stream_close(self._h))

    # streams that push, join and reset on their own (nww_stream_push_some / nww_stream_reset_some)
    @staticmethod
    def _stream_ids(ids) -> np.ndarray:
        return np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int32)

    def stream_push_some(self, ids, chunk):
        """ids: strictly ascending stream numbers [n]; chunk int16 [n, hop], row i for stream ids[i] -> (logits [n], probs [n]), 0 for a
        stream whose own ring does not hold a window yet"""
        S, W, hop = self._stream
        ids = self._stream_ids(ids)
        n = len(ids)
        chunk = self._pcm(chunk) if n else np.zeros((0, hop), np.int16)
        if chunk.shape != (n, hop):
            raise ValueError(f"chunk must have shape ({n}, {hop}), got {chunk.shape}")
        logits, probs = np.empty(n, np.float32), np.empty(n, np.float32)
        self._check(self.lib.nww_stream_push_some(self._h, ids.ctypes.data_as(C.c_void_p), n, chunk.ctypes.data_as(C.c_void_p),
                                                  logits.ctypes.data_as(C.c_void_p), probs.ctypes.data_as(C.c_void_p)))
        return logits, probs

    def stream_push_some_dev(self, ids, chunk_ptr: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0):
        ids = self._stream_ids(ids)
        self._check(self.lib.nww_stream_push_some_dev(self._h, ids.ctypes.data_as(C.c_void_p), len(ids), C.c_void_p(chunk_ptr),
                                                      C.c_void_p(logits_ptr), C.c_void_p(probs_ptr) if probs_ptr else None,
                                                      C.c_void_p(stream) if stream else None))

    def stream_reset_some(self, ids):
        """a new session for the listed streams only"""
        ids = self._stream_ids(ids)
        self._check(self.lib.nww_stream_reset_some(self._h, ids.ctypes.data_as(C.c_void_p), len(ids)))

    def stream_pool_stats(self):
        """the latest stream_push_some: (streams scored, route: 1 shared frames / 0 whole windows, frames the frontend was asked for)"""
        n, route, frames = C.c_int32(), C.c_int32(), C.c_int64()
        if self.lib.nww_stream_pool_stats(self._h, C.byref(n), C.byref(route), C.byref(frames)) != 0:
            raise NwwError("no open stream batch (nww_stream_open)")
        return n.value, route.value, frames.value

    # ------------------------------------------------------------------ embedding-mode preprocessor state (nww_emb_*)
    def emb_open(self, n_streams: int = 1, mel_bins: int = 32, emb_dim: int = 96, mel_cap: int = 970, feat_cap: int = 120):
        self._check(self.lib.nww_emb_open(self._h, int(n_streams), int(mel_bins), int(emb_dim), int(mel_cap), int(feat_cap)))
        self._emb = (int(n_streams), int(mel_bins), int(emb_dim))

    def emb_reset(self):
        self._check(self.lib.nww_emb_reset(self._h))

    def emb_close(self):
        self._check(self.lib.nww_emb_close(self._h))

    def emb_state(self):
        a, b = C.c_int32(), C.c_int32()
        self._check(self.lib.nww_emb_state(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def emb_push_mel(self, mel, raw: bool = True):
        """mel float32 [S, n_frames, bins]: the mel model's output for the newest audio; raw applies x/10 + 2."""
        S, bins, _ = self._emb
        mel = _as_f32(mel)
        if mel.ndim != 3 or mel.shape[0] != S or mel.shape[2] != bins:
            raise ValueError(f"mel must have shape ({S}, n_frames, {bins}), got {mel.shape}")
        self._check(self.lib.nww_emb_push_mel(self._h, mel.ctypes.data_as(C.c_void_p), mel.shape[1], 0, int(bool(raw))))

    def emb_windows(self, n_chunks: int) -> np.ndarray:
        S, bins, _ = self._emb
        out = np.empty((S, int(n_chunks), 76, bins), np.float32)
        nv = C.c_int32()
        self._check(self.lib.nww_emb_windows(self._h, int(n_chunks), out.ctypes.data_as(C.c_void_p), 0, C.byref(nv)))
        return np.ascontiguousarray(out.reshape(-1)[:S * nv.value * 76 * bins].reshape(S, nv.value, 76, bins))

    def emb_push_features(self, emb):
        S, _, D = self._emb
        emb = _as_f32(emb)
        if emb.ndim != 3 or emb.shape[0] != S or emb.shape[2] != D:
            raise ValueError(f"embeddings must have shape ({S}, k, {D}), got {emb.shape}")
        if emb.shape[1]:
            self._check(self.lib.nww_emb_push_features(self._h, emb.ctypes.data_as(C.c_void_p), emb.shape[1], 0))

    def emb_get_features(self, n_frames: int) -> np.ndarray:
        S, _, D = self._emb
        out = np.empty((S, int(n_frames), D), np.float32)
        n = C.c_int32()
        self._check(self.lib.nww_emb_get_features(self._h, int(n_frames), out.ctypes.data_as(C.c_void_p), 0, C.byref(n)))
        return np.ascontiguousarray(out.reshape(-1)[:S * n.value * D].reshape(S, n.value, D))

    def emb_forward(self):
        """(logits [S], probs [S]) of the head on get_features(T) of every stream; features stay on the device."""
        S = self._emb[0]
        logits, probs = np.empty(S, np.float32), np.empty(S, np.float32)
        self._check(self.lib.nww_emb_forward(self._h, logits.ctypes.data_as(C.c_void_p), probs.ctypes.data_as(C.c_void_p)))
        return logits, probs

    def emb_window_batch(self, mel) -> np.ndarray:
        """mel float32 [B, F, bins] -> windows [B, (F-76)//8+1, 76, bins] (AudioFeatures._get_embeddings_batch windowing)."""
        mel = _as_f32(mel)
        B, F, bins = mel.shape
        if F < 76:
            raise ValueError("Embedding model requires the input melspectrograms to have at least 76 frames")
        W = (F - 76) // 8 + 1
        out = np.empty((B, W, 76, bins), np.float32)
        nw = C.c_int32()
        self._check(self.lib.nww_emb_window_batch(self._h, mel.ctypes.data_as(C.c_void_p), B, F, bins, out.ctypes.data_as(C.c_void_p), 0, C.byref(nw)))
        assert nw.value == W
        return out

    def emb_pad_batch(self, specs, pad: float = -80.0, raw: bool = False) -> np.ndarray:
        """list of float32 [frames_i, bins] -> [B, max frames, bins] padded with `pad` (AudioFeatures.py:213-225)."""
        specs = [_as_f32(s) for s in specs]
        bins = specs[0].shape[1]
        frames = np.array([s.shape[0] for s in specs], np.int32)
        Fmax = int(frames.max())
        packed = np.ascontiguousarray(np.concatenate(specs, axis=0))
        out = np.empty((len(specs), Fmax, bins), np.float32)
        self._check(self.lib.nww_emb_pad_batch(self._h, packed.ctypes.data_as(C.c_void_p), frames.ctypes.data_as(C.POINTER(C.c_int32)),
                                               len(specs), bins, Fmax, float(pad), int(bool(raw)), out.ctypes.data_as(C.c_void_p)))
        return out

    # ------------------------------------------------------------------ multi-GPU gather through the C-ABI (RCCL)
    @staticmethod
    def comm_unique_id() -> bytes:
        """128-byte RCCL id; rank 0 creates it and hands it to the other ranks (any transport)."""
        lib = _lib.load_library()
        buf = C.create_string_buffer(128)
        rc = lib.nww_comm_unique_id(buf)
        if rc != 0:
            raise NwwError(lib.nww_last_error(None).decode())
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        self._check(self.lib.nww_comm_init(self._h, int(rank), int(world), C.create_string_buffer(unique_id, 128)))
        self._comm = (int(rank), int(world))

    def comm_destroy(self):
        self._check(self.lib.nww_comm_destroy(self._h))

    def all_gather_logits_dev(self, send_ptr: int, recv_ptr: int, count: int, stream: int = 0):
        self._check(self.lib.nww_all_gather_logits(self._h, C.c_void_p(send_ptr), C.c_void_p(recv_ptr), int(count),
                                                   C.c_void_p(stream) if stream else None))

    def forward_pcm_gather_dev(self, pcm_ptr: int, B: int, N: int, all_logits_ptr: int, stream: int = 0):
        """this rank's B clips -> all ranks' logits [world, B] at all_logits_ptr; kernels + RCCL all-gather on one stream"""
        self._check(self.lib.nww_forward_pcm_gather_dev(self._h, C.c_void_p(pcm_ptr), int(B), int(N), C.c_void_p(all_logits_ptr),
                                                        C.c_void_p(stream) if stream else None))

    def forward_pcm_gather_async_dev(self, pcm_ptr: int, B: int, N: int, all_logits_ptr: int, stream: int = 0):
        """the same step with the all-gather on the handle's own stream behind an event (the next step's kernels do not wait for it);
        alternate two all_logits buffers, gather_fence(stream) before reading them"""
        self._check(self.lib.nww_forward_pcm_gather_async_dev(self._h, C.c_void_p(pcm_ptr), int(B), int(N), C.c_void_p(all_logits_ptr),
                                                              C.c_void_p(stream) if stream else None))

    def gather_fence(self, stream: int = 0):
        self._check(self.lib.nww_gather_fence(self._h, C.c_void_p(stream) if stream else None))

    def gather_overlap_ms(self) -> float:
        """ms from the latest asynchronous step's start to the end of the previous step's gather (> 0: they overlapped)"""
        ms = C.c_float(0.0)
        self._check(self.lib.nww_gather_overlap_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def set_profiling(self, enable=True):
        """True/1: HIP events around every launch of every forward; n > 1: of every n-th forward only; False: off."""
        self._check(self.lib.nww_set_profiling(self._h, int(enable)))

    def get_profile(self):
        """[(launch name, total ms, launches)] accumulated since set_profiling(True); HIP events on the launch stream."""
        names = self.describe_plan().strip().split("\n")
        # interval 0 is the whole frontend: the raw-PCM heads list one line per frontend launch, which share it
        n_fe = sum(l.startswith("frontend:") for l in names)
        if n_fe > 1:
            names = [" + ".join(names[:n_fe])] + names[n_fe:]
        n = C.c_int32(len(names) + 8)
        ms = (C.c_float * n.value)()
        cnt = (C.c_int32 * n.value)()
        self._check(self.lib.nww_get_profile(self._h, ms, cnt, C.byref(n)))
        return [(names[i] if i < len(names) else f"#{i}", float(ms[i]), int(cnt[i])) for i in range(n.value)]

    def describe_plan(self) -> str:
        buf = C.create_string_buffer(16384)
        self._check(self.lib.nww_describe_plan(self._h, buf, len(buf)))
        return buf.value.decode()


class HipCascade:
    """A gate and a verifier as a pair on one GPU (nww_cascade_*): the gate scores every window, the verifier only those the gate opens
    (config.cascade_open: closed exactly where float(gate_prob) < gate_threshold), selected, gathered and scattered on the device.
    Every entry point returns dense per-window outputs: the gate's probabilities as the gate alone gives them, the verifier's logits /
    probabilities as verifier.forward_pcm gives them on the open windows stacked in ascending order (in chunks of max_batch), and
    -inf / 0.0 on closed windows.  With no window open the verifier is not launched."""

    def __init__(self, gate: HipModel, verifier: HipModel, gate_threshold: float = 0.3):
        if not isinstance(gate, HipModel) or not isinstance(verifier, HipModel):
            raise TypeError("HipCascade needs two HipModel objects: the gate and the verifier")
        if gate is verifier:
            raise ValueError("a cascade needs two distinct models: the gate and the verifier are the same one")
        if not gate.finalized or not verifier.finalized:
            raise NwwError("HipCascade needs finalized HipModels")
        self.gate, self.verifier, self.gate_threshold = gate, verifier, float(gate_threshold)
        self.lib = verifier.lib

    def _check(self, rc: int):
        self.verifier._check(rc)              # a cascade's errors go to the verifier's handle

    @property
    def clip_samples(self) -> int:
        a, b = self.gate.clip_samples, self.verifier.clip_samples
        if a != b:
            raise ValueError(f"the gate was built for clips of {a} samples and the verifier for {b}: pass `window`")
        return a

    def _thr(self, thr) -> float:
        return self.gate_threshold if thr is None else float(thr)

    def select(self, probs, thr: Optional[float] = None) -> np.ndarray:
        """float32 [n] scores -> the ascending int32 indices of the open ones (nww_cascade_select: the device's select alone)"""
        p = np.ascontiguousarray(np.asarray(probs), dtype=np.float32).reshape(-1)
        if p.size == 0:
            return np.empty(0, np.int32)
        if p.size >= 2 ** 31:
            raise ValueError("at most 2**31 - 1 scores per call")
        idx, n_open = np.empty(p.size, np.int32), C.c_int32()
        self._check(self.lib.nww_cascade_select(self.verifier._h, p.ctypes.data_as(C.c_void_p), p.size, self._thr(thr),
                                                idx.ctypes.data_as(C.c_void_p), C.byref(n_open)))
        return idx[:n_open.value].copy()

    def forward_pcm(self, pcm, gate_threshold: Optional[float] = None):
        """int16 [B,N] -> (gate_probs [B], logits [B], probs [B], n_open); the verifier runs the open clips as one batch"""
        pcm = HipModel._pcm(pcm)
        B, N = pcm.shape
        gp, logits, probs = np.empty(B, np.float32), np.empty(B, np.float32), np.empty(B, np.float32)
        n_open = C.c_int32()
        self._check(self.lib.nww_cascade_forward_pcm(self.gate._h, self.verifier._h, pcm.ctypes.data_as(C.c_void_p), B, N, self._thr(gate_threshold),
                                                     gp.ctypes.data_as(C.c_void_p), logits.ctypes.data_as(C.c_void_p),
                                                     probs.ctypes.data_as(C.c_void_p), C.byref(n_open)))
        return gp, logits, probs, int(n_open.value)

    def forward_pcm_dev(self, pcm_ptr: int, B: int, N: int, gate_probs_ptr: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0,
                        gate_threshold: Optional[float] = None) -> int:
        """Raw device pointers; enqueues on `stream`, which it synchronises once (the count of open clips).  Returns n_open."""
        n_open = C.c_int32()
        self._check(self.lib.nww_cascade_forward_pcm_dev(self.gate._h, self.verifier._h, C.c_void_p(pcm_ptr), int(B), int(N), self._thr(gate_threshold),
                                                         C.c_void_p(gate_probs_ptr) if gate_probs_ptr else None,
                                                         C.c_void_p(logits_ptr) if logits_ptr else None,
                                                         C.c_void_p(probs_ptr) if probs_ptr else None, C.byref(n_open),
                                                         C.c_void_p(stream) if stream else None))
        return int(n_open.value)

    def forward_recording(self, pcm, window: Optional[int] = None, hop: int = 1280, offset: int = 0, max_batch: int = 4096,
                          gate_threshold: Optional[float] = None):
        """int16 [N] -> (gate_probs [nW], logits [nW], probs [nW], n_open) over the windows pcm[offset + i * hop : offset + i * hop + window]:
        the gate scores all passes, one select, then the verifier in chunks of at most max_batch open windows.  The recording goes up once."""
        pcm = HipModel._pcm1(pcm)
        window = int(self.clip_samples if window is None else window)
        if offset < 0:
            raise ValueError("offset must not be negative")
        x = pcm[min(int(offset), len(pcm)):]
        gp = np.empty(max(0, recording_windows(len(x), window, hop)) if window > 0 and hop > 0 else 0, np.float32)
        logits, probs = np.empty_like(gp), np.empty_like(gp)
        nw, n_open = C.c_int32(), C.c_int32()
        keep = x if len(x) else np.zeros(1, np.int16)               # a valid pointer for an empty recording
        self._check(self.lib.nww_cascade_forward_recording(self.gate._h, self.verifier._h, keep.ctypes.data_as(C.c_void_p), len(x), window, int(hop),
                                                           int(max_batch), self._thr(gate_threshold), gp.ctypes.data_as(C.c_void_p),
                                                           logits.ctypes.data_as(C.c_void_p), probs.ctypes.data_as(C.c_void_p),
                                                           C.byref(nw), C.byref(n_open)))
        assert nw.value == len(gp), (nw.value, len(gp))
        return gp, logits, probs, int(n_open.value)

    def forward_recording_dev(self, pcm_ptr: int, n_samples: int, window: int, hop: int, gate_probs_ptr: int, logits_ptr: int, probs_ptr: int = 0,
                              max_batch: int = 4096, stream: int = 0, gate_threshold: Optional[float] = None):
        """Raw device pointers; enqueues on `stream`, which it synchronises once.  Returns (windows written, n_open)."""
        nw = self.gate._rec_count(n_samples, window, hop)
        n_open = C.c_int32()
        self._check(self.lib.nww_cascade_forward_recording_dev(self.gate._h, self.verifier._h, C.c_void_p(pcm_ptr), int(n_samples), int(window), int(hop),
                                                               int(max_batch), self._thr(gate_threshold),
                                                               C.c_void_p(gate_probs_ptr) if gate_probs_ptr else None,
                                                               C.c_void_p(logits_ptr) if logits_ptr else None,
                                                               C.c_void_p(probs_ptr) if probs_ptr else None, C.byref(n_open),
                                                               C.c_void_p(stream) if stream else None))
        return nw, int(n_open.value)

    # ------------------------------------------------------------------ S lock-step streams: the ring is the gate's
    def stream_open(self, n_streams: int, window_samples: Optional[int] = None, hop_samples: int = 1280):
        self.gate.stream_open(n_streams, int(self.clip_samples if window_samples is None else window_samples), hop_samples)

    def stream_push(self, chunk, gate_threshold: Optional[float] = None):
        """chunk int16 [S, hop] -> (gate_probs [S], logits [S], probs [S], n_open); zeros until every stream has a full window"""
        S, W, hop = self.gate._stream
        chunk = HipModel._pcm(chunk)
        if chunk.shape != (S, hop):
            raise ValueError(f"chunk must have shape ({S}, {hop}), got {chunk.shape}")
        gp, logits, probs = np.empty(S, np.float32), np.empty(S, np.float32), np.empty(S, np.float32)
        n_open = C.c_int32()
        self._check(self.lib.nww_cascade_stream_push(self.gate._h, self.verifier._h, chunk.ctypes.data_as(C.c_void_p), self._thr(gate_threshold),
                                                     gp.ctypes.data_as(C.c_void_p), logits.ctypes.data_as(C.c_void_p),
                                                     probs.ctypes.data_as(C.c_void_p), C.byref(n_open)))
        return gp, logits, probs, int(n_open.value)

    def stream_push_dev(self, chunk_ptr: int, gate_probs_ptr: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0,
                        gate_threshold: Optional[float] = None) -> int:
        n_open = C.c_int32()
        self._check(self.lib.nww_cascade_stream_push_dev(self.gate._h, self.verifier._h, C.c_void_p(chunk_ptr), self._thr(gate_threshold),
                                                         C.c_void_p(gate_probs_ptr) if gate_probs_ptr else None,
                                                         C.c_void_p(logits_ptr) if logits_ptr else None,
                                                         C.c_void_p(probs_ptr) if probs_ptr else None, C.byref(n_open),
                                                         C.c_void_p(stream) if stream else None))
        return int(n_open.value)

    def stream_reset(self):
        self.gate.stream_reset()

    def stream_filled(self) -> int:
        return self.gate.stream_filled()

    def stream_close(self):
        self.gate.stream_close()

    # streams that push, join and reset on their own (nww_cascade_stream_push_some): the gate's batch in any state, aligned or not
    def stream_push_some(self, ids, chunk, gate_threshold: Optional[float] = None):
        """ids: strictly ascending stream numbers [n]; chunk int16 [n, hop], row i for stream ids[i] -> (gate_probs [n], logits [n],
        probs [n], n_open).  A stream whose own ring holds no window yet reads 0 / 0 / 0 and is never open; a scored one that the gate
        closes reads -inf / 0.0 (config.cascade_pool_open); the verifier runs the open streams' windows as one batch."""
        S, W, hop = self.gate._stream
        ids = HipModel._stream_ids(ids)
        n = len(ids)
        chunk = HipModel._pcm(chunk) if n else np.zeros((0, hop), np.int16)
        if chunk.shape != (n, hop):
            raise ValueError(f"chunk must have shape ({n}, {hop}), got {chunk.shape}")
        gp, logits, probs = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
        n_open = C.c_int32()
        self._check(self.lib.nww_cascade_stream_push_some(self.gate._h, self.verifier._h, ids.ctypes.data_as(C.c_void_p), n,
                                                          chunk.ctypes.data_as(C.c_void_p), self._thr(gate_threshold),
                                                          gp.ctypes.data_as(C.c_void_p), logits.ctypes.data_as(C.c_void_p),
                                                          probs.ctypes.data_as(C.c_void_p), C.byref(n_open)))
        return gp, logits, probs, int(n_open.value)

    def stream_push_some_dev(self, ids, chunk_ptr: int, gate_probs_ptr: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0,
                             gate_threshold: Optional[float] = None) -> int:
        """Raw device pointers (ids stays on the host); enqueues on `stream`, which it synchronises once.  Returns n_open."""
        ids = HipModel._stream_ids(ids)
        n_open = C.c_int32()
        self._check(self.lib.nww_cascade_stream_push_some_dev(self.gate._h, self.verifier._h, ids.ctypes.data_as(C.c_void_p), len(ids),
                                                              C.c_void_p(chunk_ptr), self._thr(gate_threshold),
                                                              C.c_void_p(gate_probs_ptr) if gate_probs_ptr else None,
                                                              C.c_void_p(logits_ptr) if logits_ptr else None,
                                                              C.c_void_p(probs_ptr) if probs_ptr else None, C.byref(n_open),
                                                              C.c_void_p(stream) if stream else None))
        return int(n_open.value)

    def stream_reset_some(self, ids):
        """a new session for the listed streams only (the ring is the gate's)"""
        ids = HipModel._stream_ids(ids)
        self._check(self.lib.nww_cascade_stream_reset_some(self.gate._h, self.verifier._h, ids.ctypes.data_as(C.c_void_p), len(ids)))

    def stream_filled_of(self, i: int) -> int:
        """samples stream i has seen since open / its last reset"""
        return self.gate.stream_filled(int(i))

    def describe(self, pool: bool = False) -> str:
        """The launches of one cascade call, one per line: the gate's plan, the select, the gather, the verifier's plan, the scatter.
        pool: of a stream_push_some call, whose select walks the table of the gate's pool call (the gate's own data movement around its
        plan is the pool's: DESIGN.md 4.8d)"""
        g = self.gate.describe_plan().strip().split("\n")
        v = self.verifier.describe_plan().strip().split("\n")
        select = ("cascade_pool_select:count + place over the call's table - ring offsets and entries of the scored streams with "
                  "float(gate_prob) >= threshold, ascending; 0 fill without a window, closed fill" if pool else
                  "cascade_select:count + place - ascending indices of the windows with float(gate_prob) >= threshold, closed fill")
        return "\n".join(g + [select,
                              "cascade_gather:open windows -> the verifier's PCM staging"] + v +
                         ["cascade_scatter:the verifier's logits / probabilities -> their windows"]) + "\n"


class HipBank:
    """Several wake words on one frontend pass (nww_bank_*): finalized HipModels on one GPU whose mel frontends are identical, in
    insertion order.  The first is the LEADER: it owns the PCM staging, the frontend's launches, the dense head input, the stream
    batch and the recording pool; the others run only their head plans, on the leader's head input.  Every entry point returns
    {name: (logits, probs)}, each pair bit-identical to the same call on that model alone, whichever model leads."""

    def __init__(self, models: Mapping[str, HipModel]):
        if not isinstance(models, Mapping) or not models:
            raise ValueError("HipBank needs a non-empty {name: HipModel} mapping")
        for m in models.values():
            if not isinstance(m, HipModel):
                raise TypeError("HipBank needs HipModel objects")
            if not m.finalized:
                raise NwwError("HipBank needs finalized HipModels")
        self.models = dict(models)
        self.names = list(self.models)
        self.leader = self.models[self.names[0]]
        self.lib = self.leader.lib
        self.k = len(self.names)
        self._members = (C.c_void_p * self.k)(*[m._h for m in self.models.values()])

    def _check(self, rc: int):
        self.leader._check(rc)                # a bank's errors go to the leader's handle

    def check(self, window: Optional[int] = None):
        """the bank's rules alone for clips or windows of `window` samples (nww_bank_check): raises what a call would raise"""
        self._check(self.lib.nww_bank_check(self._members, self.k, int(self.clip_samples if window is None else window)))

    @property
    def clip_samples(self) -> int:
        n = {name: m.clip_samples for name, m in self.models.items()}
        if len(set(n.values())) != 1:
            raise ValueError(f"the bank's models were built for clips of different lengths {n}: pass `window`")
        return next(iter(n.values()))

    def _split(self, logits: np.ndarray, probs: np.ndarray):
        return {name: (logits[j].copy(), probs[j].copy()) for j, name in enumerate(self.names)}

    def forward_pcm(self, pcm):
        """int16 [B,N] -> {name: (logits [B], probs [B])}; the clips are uploaded once and the frontend runs once"""
        pcm = HipModel._pcm(pcm)
        B, N = pcm.shape
        logits, probs = np.empty((self.k, B), np.float32), np.empty((self.k, B), np.float32)
        self._check(self.lib.nww_bank_forward_pcm(self._members, self.k, pcm.ctypes.data_as(C.c_void_p), B, N,
                                                  logits.ctypes.data_as(C.c_void_p), probs.ctypes.data_as(C.c_void_p)))
        return self._split(logits, probs)

    def forward_pcm_dev(self, pcm_ptr: int, B: int, N: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0):
        """Raw device pointers, outputs [k][B] member-major; enqueues on `stream`, does not synchronise."""
        self._check(self.lib.nww_bank_forward_pcm_dev(self._members, self.k, C.c_void_p(pcm_ptr), int(B), int(N),
                                                      C.c_void_p(logits_ptr) if logits_ptr else None,
                                                      C.c_void_p(probs_ptr) if probs_ptr else None, C.c_void_p(stream) if stream else None))

    def forward_recording(self, pcm, window: Optional[int] = None, hop: int = 1280, offset: int = 0, max_batch: int = 4096):
        """int16 [N] -> {name: (logits [nW], probs [nW])} over the windows pcm[offset + i * hop : offset + i * hop + window]; the recording
        goes up once and every pass runs the leader's frontend launches once"""
        pcm = HipModel._pcm1(pcm)
        window = int(self.clip_samples if window is None else window)
        if offset < 0:
            raise ValueError("offset must not be negative")
        x = pcm[min(int(offset), len(pcm)):]
        self.check(window)
        nw = self.leader._rec_count(len(x), window, hop)
        logits, probs = np.empty((self.k, nw), np.float32), np.empty((self.k, nw), np.float32)
        if nw:
            n_out = C.c_int32()
            self._check(self.lib.nww_bank_forward_recording(self._members, self.k, x.ctypes.data_as(C.c_void_p), len(x), window, int(hop),
                                                            int(max_batch), logits.ctypes.data_as(C.c_void_p),
                                                            probs.ctypes.data_as(C.c_void_p), C.byref(n_out)))
            assert n_out.value == nw
        return self._split(logits, probs)

    def forward_recording_dev(self, pcm_ptr: int, n_samples: int, window: int, hop: int, logits_ptr: int, probs_ptr: int = 0,
                              max_batch: int = 4096, stream: int = 0) -> int:
        """Raw device pointers, outputs [k][nW] member-major; enqueues on `stream`, does not synchronise.  Returns nW."""
        nw = self.leader._rec_count(n_samples, window, hop)
        self._check(self.lib.nww_bank_forward_recording_dev(self._members, self.k, C.c_void_p(pcm_ptr), int(n_samples), int(window), int(hop),
                                                            int(max_batch), C.c_void_p(logits_ptr) if logits_ptr else None,
                                                            C.c_void_p(probs_ptr) if probs_ptr else None,
                                                            C.c_void_p(stream) if stream else None))
        return nw

    # ------------------------------------------------------------------ streams: the batch, its rings and its state are the leader's
    def stream_open(self, n_streams: int, window_samples: Optional[int] = None, hop_samples: int = 1280):
        window = int(self.clip_samples if window_samples is None else window_samples)
        self.check(window)
        self.leader.stream_open(n_streams, window, hop_samples)

    def stream_reset(self):
        self.leader.stream_reset()

    def stream_reset_some(self, ids):
        self.leader.stream_reset_some(ids)

    def stream_close(self):
        self.leader.stream_close()

    def stream_filled_of(self, i: int) -> int:
        return self.leader.stream_filled_of(i)

    def stream_pool_stats(self):
        return self.leader.stream_pool_stats()

    def stream_push_some(self, ids, chunk):
        """ids: strictly ascending stream numbers [n]; chunk int16 [n, hop], row i for stream ids[i] -> {name: (logits [n], probs [n])},
        0 / 0 for every model on a stream whose own ring does not hold a window yet"""
        if not hasattr(self.leader, "_stream"):
            raise NwwError("member 0: no open stream batch (nww_stream_open): the leader holds a bank's streams")
        S, W, hop = self.leader._stream
        ids = HipModel._stream_ids(ids)
        n = len(ids)
        chunk = HipModel._pcm(chunk) if n else np.zeros((0, hop), np.int16)
        if chunk.shape != (n, hop):
            raise ValueError(f"chunk must have shape ({n}, {hop}), got {chunk.shape}")
        logits, probs = np.empty((self.k, n), np.float32), np.empty((self.k, n), np.float32)
        self._check(self.lib.nww_bank_stream_push_some(self._members, self.k, ids.ctypes.data_as(C.c_void_p), n, chunk.ctypes.data_as(C.c_void_p),
                                                       logits.ctypes.data_as(C.c_void_p), probs.ctypes.data_as(C.c_void_p)))
        return self._split(logits, probs)

    def stream_push_some_dev(self, ids, chunk_ptr: int, logits_ptr: int, probs_ptr: int = 0, stream: int = 0):
        """Raw device pointers (ids stays on the host), outputs [k][n] member-major; enqueues on `stream`, does not synchronise."""
        ids = HipModel._stream_ids(ids)
        self._check(self.lib.nww_bank_stream_push_some_dev(self._members, self.k, ids.ctypes.data_as(C.c_void_p), len(ids), C.c_void_p(chunk_ptr),
                                                           C.c_void_p(logits_ptr) if logits_ptr else None,
                                                           C.c_void_p(probs_ptr) if probs_ptr else None,
                                                           C.c_void_p(stream) if stream else None))

    def describe(self) -> str:
        """The launches of one bank call on a batch of clips, one per line: the leader's frontend, then every member's head plan under
        its name (a recording's shared route and a pool call run the leader's own launches around the frontend instead)."""
        lines = []
        for j, (name, m) in enumerate(self.models.items()):
            for l in m.describe_plan().strip().split("\n"):
                if l.startswith("frontend:"):
                    if j == 0:
                        lines.append(l + " - once, by the leader '%s'" % name)
                else:
                    lines.append("%s/%s" % (name, l))
        return "\n".join(lines) + "\n"


class _Input:
    """Stand-in for onnxruntime NodeArg (cf. _FakeInput, remote_verifier.py:595-603)."""

    def __init__(self, name, shape):
        self.name, self.shape, self.type = name, shape, "tensor(float)"


class HipSession:
    """Drop-in for the ONNX session the reference interpreter holds per model.

    mode="e2e":       input (B,1,N) or (B,N) float32 PCM/32768 (nanointerpreter.py:750,771-775) or int16.
    mode="features":  input (B,T,F) float32.
    run() returns [probabilities (B,1,1) float32] like the exported InferenceWrapper
    (_export/onnx.py:164-172); run_logits() returns the pre-sigmoid logits.
    """

    def __init__(self, model: HipModel, mode: str = "e2e", clip_samples: int = 16000, input_ndim: int = 3,
                 name: str = "hip_model"):
        if mode not in ("e2e", "features"):
            raise ValueError("mode must be 'e2e' or 'features'")
        if not model.finalized:
            raise NwwError("HipSession needs a finalized HipModel")
        self.model, self.mode, self.clip_samples, self.input_ndim = model, mode, int(clip_samples), int(input_ndim)
        self._model_filename = name + ".hip"
        self.name = name
        self.metadata = {"mode": mode}
        self.accepts_int16 = True       # HipInterpreter then skips the float32 round trip of nanointerpreter.py:750
        if mode == "e2e":
            T = model.num_frames(self.clip_samples)
            if model.head.model_type in RAW_HEADS:      # learned filters on raw PCM: num_frames is the raw frontend's frame law
                rows, cols = T, model.head.input_shape[1]
            else:
                rows, cols = (model.fe.n_mels, T) if model.head.model_type == "e2e_dnn" else (T, model.fe.n_mels)
            if (rows, cols) != tuple(model.head.input_shape):
                raise ValueError(f"clip_samples={clip_samples} gives ({rows},{cols}) features, head expects {model.head.input_shape}")

    def get_inputs(self):
        if self.mode == "e2e":
            shape = [None, 1, self.clip_samples] if self.input_ndim == 3 else [None, self.clip_samples]
        else:
            shape = [None, self.model.head.input_shape[0], self.model.head.input_shape[1]]
        return [_Input("input", shape)]

    def get_outputs(self):
        return [_Input("output", [None, 1, 1])]

    def _to_pcm(self, x: np.ndarray) -> np.ndarray:
        if x.ndim == 3:
            if x.shape[1] != 1:
                raise ValueError("e2e input must have shape (B,1,N) or (B,N)")
            x = x[:, 0, :]
        if x.ndim != 2:
            raise ValueError("e2e input must have shape (B,1,N) or (B,N)")
        if x.dtype == np.int16:
            return np.ascontiguousarray(x)
        xf = np.asarray(x, dtype=np.float32) * np.float32(32768.0)
        xi = np.rint(xf)
        if not np.array_equal(xi, xf) or xi.min(initial=0) < -32768 or xi.max(initial=0) > 32767:
            raise ValueError("float PCM must be int16/32768.0 exactly (as NanoInterpreter builds it); "
                             "pass the int16 samples for anything else")
        return np.ascontiguousarray(xi.astype(np.int16))

    def _forward(self, input_feed):
        if not isinstance(input_feed, dict) or "input" not in input_feed:
            raise ValueError("input_feed must be {'input': ndarray}")
        x = input_feed["input"]
        if not isinstance(x, np.ndarray):
            raise ValueError("Input must be a Numpy array.")
        if self.mode == "e2e":
            return self.model.forward_pcm(self._to_pcm(x))
        return self.model.forward_features(x)

    def run(self, output_names, input_feed):
        _, probs = self._forward(input_feed)
        return [probs.reshape(-1, 1, 1)]

    def run_recording(self, pcm: np.ndarray, hop: int = 1280, offset: int = 0, max_batch: int = 4096) -> np.ndarray:
        """int16 [N] -> probabilities [nW] of the windows pcm[offset + i * hop : offset + i * hop + clip_samples] (what run() returns for
        each of them), the recording uploaded once: HipInterpreter.score_recording's batch path."""
        if self.mode != "e2e":
            raise ValueError("run_recording needs an e2e session (raw PCM in)")
        return self.model.forward_recording(pcm, window=self.clip_samples, hop=hop, offset=offset, max_batch=max_batch)[1]

    def cascade_accepts(self, gate_session) -> bool:
        """Whether run_recording_cascade can take `gate_session` as this session's gate: both e2e HipSessions on two models of one
        device, built for the same clip length (cheap: no device call)."""
        return (isinstance(gate_session, HipSession) and gate_session is not self and self.mode == "e2e" and gate_session.mode == "e2e"
                and gate_session.model is not self.model and gate_session.model.device == self.model.device
                and gate_session.clip_samples == self.clip_samples)

    def run_recording_cascade(self, gate_session, pcm: np.ndarray, hop: int = 1280, offset: int = 0, gate_threshold: float = 0.3,
                              max_batch: int = 4096):
        """int16 [N] -> (gate probabilities [nW], this session's probabilities [nW]) over the windows of run_recording, this session's model
        run only on the windows whose raw gate probability reaches gate_threshold (0.0 elsewhere): HipInterpreter.score_recording's batch
        path for a cascade.  last_cascade keeps (windows, open windows) of the latest call."""
        if not self.cascade_accepts(gate_session):
            raise ValueError("run_recording_cascade needs two e2e HipSessions on one device with the same clip_samples")
        cas = getattr(self, "_cascade", None)
        if cas is None or cas.gate is not gate_session.model:
            cas = self._cascade = HipCascade(gate_session.model, self.model, gate_threshold)
        gp, _, probs, n_open = cas.forward_recording(pcm, window=self.clip_samples, hop=hop, offset=offset, max_batch=max_batch,
                                                     gate_threshold=gate_threshold)
        self.last_cascade = (len(gp), n_open)
        return gp, probs

    def bank_accepts(self, other_session) -> bool:
        """Whether `other_session` can share this session's frontend pass (run_recording_bank, HipBank): both e2e HipSessions on two
        models of one device, built for the same clip length, and the bank's rules hold for the pair led by this one (nww_bank_check)."""
        if not (isinstance(other_session, HipSession) and other_session is not self and self.mode == "e2e" and other_session.mode == "e2e"
                and other_session.model is not self.model and other_session.model.device == self.model.device
                and other_session.clip_samples == self.clip_samples):
            return False
        pair = (C.c_void_p * 2)(self.model._h, other_session.model._h)
        return self.model.lib.nww_bank_check(pair, 2, self.clip_samples) == 0

    def _bank(self, sessions) -> "HipBank":
        sessions = list(sessions)
        if not sessions or sessions[0] is not self or not all(self.bank_accepts(s) for s in sessions[1:]):
            raise ValueError("a bank needs e2e HipSessions on one device with the same clip_samples and identical frontends, led by this one")
        key = tuple(id(s.model) for s in sessions)
        bank = getattr(self, "_bank_cache", None)
        if bank is None or bank[0] != key:
            bank = self._bank_cache = (key, HipBank({str(j): s.model for j, s in enumerate(sessions)}))
        return bank[1]

    def run_bank(self, sessions, pcm: np.ndarray):
        """int16 (B,N) / (B,1,N) or float PCM as run() takes it -> [probabilities (B,1,1)] per session of `sessions` (this one first),
        scored on ONE upload and ONE frontend pass: HipInterpreter.predict's path for a bank."""
        out = self._bank(sessions).forward_pcm(self._to_pcm(pcm))
        return [out[str(j)][1].reshape(-1, 1, 1) for j in range(len(out))]

    def run_recording_bank(self, sessions, pcm: np.ndarray, hop: int = 1280, offset: int = 0, max_batch: int = 4096):
        """int16 [N] -> [probabilities [nW]] per session of `sessions` (this one first, the leader), over the windows of run_recording:
        the recording uploaded once and each pass's frontend run once.  HipInterpreter.score_recording's batch path for a bank."""
        out = self._bank(sessions).forward_recording(pcm, window=self.clip_samples, hop=hop, offset=offset, max_batch=max_batch)
        return [out[str(j)][1] for j in range(len(out))]

    def run_logits(self, input_feed):
        logits, _ = self._forward(input_feed)
        return logits.reshape(-1, 1)

    # clips mixed on the device out of an augment.ClipArena (HipModel.mix / forward_mixed): clips of clip_samples
    def mix(self, arena, items, irs=None, ir_ids=None, pitch=None, pitch_ids=None) -> np.ndarray:
        """int16 [B, clip_samples]: the clips of `items` mixed out of `arena` (irs / ir_ids: through impulse responses, pitch / pitch_ids:
        shifted in pitch; HipModel.mix)"""
        return self.model.mix(arena, items, self.clip_samples, irs=irs, ir_ids=ir_ids, pitch=pitch, pitch_ids=pitch_ids)

    def forward_mixed(self, arena, items, irs=None, ir_ids=None, pitch=None, pitch_ids=None):
        """[probabilities (B,1,1)] as run() returns them for mix(arena, items), the clips never leaving the device"""
        if self.mode != "e2e":
            raise ValueError("forward_mixed needs an e2e session (raw PCM in)")
        return [self.model.forward_mixed(arena, items, self.clip_samples, irs=irs, ir_ids=ir_ids, pitch=pitch,
                                         pitch_ids=pitch_ids)[1].reshape(-1, 1, 1)]

    # a pool of streams on the session's model (interpreter.StreamPool takes a session as its backend): windows of clip_samples
    def stream_open(self, n_streams: int, window_samples: Optional[int] = None, hop_samples: int = 1280):
        if self.mode != "e2e":
            raise ValueError("streams need an e2e session (raw PCM in)")
        self.model.stream_open(n_streams, self.clip_samples if window_samples is None else window_samples, hop_samples)

    def stream_push_some(self, ids, chunk):
        return self.model.stream_push_some(ids, chunk)

    def stream_reset_some(self, ids):
        self.model.stream_reset_some(ids)

    def stream_reset(self):
        self.model.stream_reset()

    def stream_filled(self, s: Optional[int] = None) -> int:
        return self.model.stream_filled(s)

    def stream_close(self):
        self.model.stream_close()
