"""Clips mixed on the device (nww_mix_*, include/nww.h): the caller side.

The reference mixes every foreground into a random background at a random SNR on the host, levels the batch and quantises it to int16
(``augment_clips``, nanowakeword/data/augment_clips.py:170-261; ``_mix_snr``, :45-79).  What is random there is the draw of the
parameters; here the host draws them (``draw_mix_items``) or lays them out as a grid (``mix_items``), ONE table per batch goes to the
device, and the recordings - uploaded once as a ``ClipArena`` - are gathered, measured and mixed there (``HipModel.mix`` /
``forward_mixed``, ``HipFeatures.embed_mixed``).  A robustness sweep of 1 000 positives x 20 noises x 6 SNRs is 120 000 table rows over
1 020 recordings.

Impulse responses (``ApplyImpulseResponse(p=rir_prob)``, augment_clips.py:150-157) ride on the same calls: the responses
go up once as an ``IrArena``, whose spectra are prepared once, ``draw_rir_ids`` draws a response or none per clip, and every call above
takes ``irs=..., ir_ids=...``.  ``gain`` is the reference's Gain step, ``level`` its volume step (:246-255).

Pitch shift (``PitchShift(+-2 semitones, p=0.5)`` between Gain and ApplyImpulseResponse, :150-157) rides on them as well:
``pitch_ratios`` lists rational ratios, a ``PitchBank`` sets them on a model, ``draw_pitch_ids`` draws a ratio or none per clip, and
every call takes ``pitch=..., pitch_ids=...``.  What is restated is a DEFINITION of the library's construction - a phase vocoder without
phase scaling, then a windowed-sinc resampler, at rational ratios - not ``torch_audiomentations``' samples: the transform length (512),
hop (128) and window (periodic Hann) are this project's own (include/nww.h).

Recordings that are not 16 kHz mono yet (``torchaudio.transforms.Resample(clip_sr, 16000)`` and the mean over the channels on every path
into the reference's clips, augment_clips.py:31-43) are downmixed and resampled on the device as well:
``ClipArena.from_recordings`` builds the arena out of arrays at their own rates, ``HipModel.resample`` returns them to the host -
float32 for an ``IrArena`` - and ``resample_ratio`` / ``resampled_length`` say what a rate pair comes to.
"""
from __future__ import annotations

from typing import Iterable, Iterator, Mapping, Optional, Sequence

import numpy as np

# struct nww_mix_item (include/nww.h), field for field: 48 bytes
MIX_ITEM = np.dtype([("fg_off", "<i8"), ("bg_off", "<i8"), ("fg_len", "<i4"), ("bg_len", "<i4"), ("bg_start", "<i4"), ("start", "<i4"),
                     ("snr_linear", "<f4"), ("gain", "<f4"), ("level", "<f4"), ("flags", "<u4")])
PEAK_NORMALISE = 1            # NWW_MIX_PEAK_NORMALISE

# augment_clips' defaults for what is restated here (augment_clips.py:139-145)
DEFAULT_SETTINGS = {"gain_prob": 1.0, "max_snr_in_db": 30.0, "min_snr_in_db": 5.0, "min_gain_in_db": -3.0, "max_gain_in_db": 3.0,
                    "min_volume_augmentation": 0.5, "max_volume_augmentation": 1.0}


class ClipArena:
    """Recordings back to back in one int16 buffer: ``offsets[i]`` / ``lengths[i]`` of clip i, ``samples`` in all.  With a device
    (the default, 0) the buffer is uploaded ONCE and ``ptr`` is its device address (a torch tensor holds it); ``device=None`` keeps
    it on the host as ``host`` (``ptr`` is 0) for the calls that upload the arena themselves."""

    def __init__(self, clips: Sequence[np.ndarray], device: Optional[int] = 0):
        arrs = []
        for i, c in enumerate(clips):
            if not isinstance(c, np.ndarray) or c.dtype != np.int16 or c.ndim != 1 or c.size == 0:
                raise ValueError(f"clip {i} must be a non-empty one-dimensional int16 array")
            arrs.append(c)
        if not arrs:
            raise ValueError("an arena needs at least one clip")
        self.lengths = np.array([a.size for a in arrs], np.int64)
        self.offsets = np.concatenate(([0], np.cumsum(self.lengths)[:-1])).astype(np.int64)
        self.samples = int(self.lengths.sum())
        self.device = device
        host = np.concatenate(arrs)
        if device is None:
            self.host, self._dev, self.ptr = host, None, 0
        else:
            import torch
            self.host = None
            self._dev = torch.from_numpy(host).to(f"cuda:{int(device)}")
            self.ptr = int(self._dev.data_ptr())

    def __len__(self) -> int:
        return len(self.lengths)

    @classmethod
    def from_recordings(cls, model, recordings: Sequence[np.ndarray], rates: Sequence[int], dst_hz: int = 16000, device: int = 0,
                        chunk_bytes: int = 64 << 20) -> "ClipArena":
        """An arena on the device out of recordings at their own sample rates: arrays [frames] or [frames, channels], int16 or float32
        (units of full scale), each with its rate in `rates`.  The sources go up in chunks of at most `chunk_bytes` and `model` (a
        HipModel on `device`) downmixes and resamples them straight into the arena's buffer (nww_resample_dev): offsets
        and lengths come from ``resampled_length``, and the host never sees the resampled audio.  A recording at `dst_hz` is downmixed
        and converted only."""
        import torch
        if device is None or int(device) != int(model.device):
            raise ValueError("from_recordings resamples on the device: `device` must be the model's")
        recs, lengths, chunks = resample_plan(recordings, rates, dst_hz, chunk_bytes)
        self = cls.__new__(cls)
        self.lengths = lengths
        self.offsets = np.concatenate(([0], np.cumsum(lengths)[:-1])).astype(np.int64)
        self.samples = int(lengths.sum())
        self.device, self.host = device, None
        dev = f"cuda:{int(device)}"
        self._dev = torch.empty((self.samples,), dtype=torch.int16, device=dev)
        self.ptr = int(self._dev.data_ptr())
        for ch in chunks:
            src = np.concatenate([r.ravel() for r in recs[ch["lo"]:ch["hi"]]])
            d_src = torch.from_numpy(src).to(dev)
            items = ch["items"].copy()
            items["dst_off"] = self.offsets[ch["lo"]:ch["hi"]]
            if ch["ratios"]:
                model.resample_set_ratios([a for a, _ in ch["ratios"]], [b for _, b in ch["ratios"]])
            torch.cuda.synchronize(int(device))                     # the upload has landed: the call runs on the model's own stream
            model.resample_dev(d_src.data_ptr(), src.size, ch["format"], items, self.ptr, self.samples, PCM_S16)
            torch.cuda.synchronize(int(device))                     # the chunk's source is released below
            del d_src
        return self


def as_items(items) -> np.ndarray:
    """a contiguous one-dimensional MIX_ITEM table"""
    if not isinstance(items, np.ndarray) or items.dtype != MIX_ITEM or items.ndim != 1:
        raise ValueError("items must be a one-dimensional array of augment.MIX_ITEM (mix_items / draw_mix_items build it)")
    return np.ascontiguousarray(items)


def mix_items(arena: ClipArena, fg_ids, bg_ids, N: int, *, snr_db=20.0, gain_db=0.0, level=1.0, start=0, bg_start=0, fg_crop=0,
              peak_normalise=True) -> np.ndarray:
    """The item table of clips of N samples from arrays that broadcast against each other (scalars included); the table is the
    broadcast shape flattened in C order, so a sweep is one call:
    ``mix_items(arena, fg[:, None, None], bg[None, :, None], N, snr_db=snrs[None, None, :])``.
    fg_ids / bg_ids index the arena's clips; bg_ids < 0 is no background.  A foreground longer than N - fg_crop is cut to it."""
    N = int(N)
    fg, bg, snr, gdb, lvl, st, bs, crop, pn = np.broadcast_arrays(
        np.asarray(fg_ids, np.int64), np.asarray(bg_ids, np.int64), np.asarray(snr_db, np.float64), np.asarray(gain_db, np.float64),
        np.asarray(level, np.float64), np.asarray(start, np.int64), np.asarray(bg_start, np.int64), np.asarray(fg_crop, np.int64),
        np.asarray(peak_normalise, bool))
    fg, bg, snr, gdb, lvl, st, bs, crop, pn = (a.ravel() for a in (fg, bg, snr, gdb, lvl, st, bs, crop, pn))
    if fg.size and (fg.min() < 0 or fg.max() >= len(arena) or bg.max() >= len(arena)):
        raise ValueError("fg_ids / bg_ids must index the arena's clips")
    if fg.size and (crop.min() < 0 or (crop >= arena.lengths[fg]).any()):
        raise ValueError("fg_crop must lie inside its foreground")
    t = np.zeros(fg.size, MIX_ITEM)
    has_bg = bg >= 0
    bgc = np.where(has_bg, bg, 0)
    t["fg_off"] = arena.offsets[fg] + crop
    t["fg_len"] = np.minimum(arena.lengths[fg] - crop, N)
    t["bg_off"] = np.where(has_bg, arena.offsets[bgc], 0)
    t["bg_len"] = np.where(has_bg, arena.lengths[bgc], 0)
    t["bg_start"] = np.where(has_bg, bs, 0)
    t["start"] = st
    t["snr_linear"] = 10.0 ** (snr / 20.0)
    t["gain"] = 10.0 ** (gdb / 20.0)
    t["level"] = lvl
    t["flags"] = np.where(pn, PEAK_NORMALISE, 0)
    return t


def draw_mix_items(rng: np.random.Generator, arena: ClipArena, fg_ids, bg_ids, N: int, settings: Optional[Mapping] = None) -> np.ndarray:
    """What augment_clips draws for each foreground of fg_ids (augment_clips.py:176,201-223,246-248), from `rng`: a background of
    bg_ids (none when it is empty), the crop of a background longer than N (a shorter one is tiled from its start), the crop of a
    foreground longer than N, the position, the SNR and gain in dB and the target level, with the reference's default ranges unless
    `settings` overrides them.  Peak-normalised, like the reference's batches.  The stream of random numbers is this function's own."""
    cfg = dict(DEFAULT_SETTINGS)
    if settings:
        cfg.update({k: v for k, v in settings.items() if k in cfg})
    N = int(N)
    fg = np.asarray(fg_ids, np.int64).ravel()
    bgs = np.asarray(bg_ids, np.int64).ravel()
    n = fg.size
    bg = rng.choice(bgs, size=n) if bgs.size else np.full(n, -1, np.int64)
    bg_len = np.where(bg >= 0, arena.lengths[np.maximum(bg, 0)], 0)
    bg_start = rng.integers(0, np.maximum(bg_len - N, 0) + 1)
    fg_crop = rng.integers(0, np.maximum(arena.lengths[fg] - N, 0) + 1)
    fg_len = np.minimum(arena.lengths[fg] - fg_crop, N)
    start = rng.integers(0, N - fg_len + 1)
    snr_db = rng.uniform(cfg["min_snr_in_db"], cfg["max_snr_in_db"], n)
    gain_db = np.where(rng.random(n) < cfg["gain_prob"], rng.uniform(cfg["min_gain_in_db"], cfg["max_gain_in_db"], n), 0.0)
    level = rng.uniform(cfg["min_volume_augmentation"], cfg["max_volume_augmentation"], n)
    return mix_items(arena, fg, bg, N, snr_db=snr_db, gain_db=gain_db, level=level, start=start, bg_start=bg_start, fg_crop=fg_crop)


# ---- room impulse responses (nww_rir_* / nww_mix_rir_*)
RIR_FFT_SIZES = (2048, 8192, 32768)


def rir_fft_size(N: int, max_ir_len: int) -> int:
    """nww_rir_fft_size: the smallest transform size with N + min(L, N) - 1 <= M, or 0 where none fits"""
    N, L = int(N), int(max_ir_len)
    if N < 1 or L < 1:
        return 0
    need = N + min(L, N) - 1
    return next((M for M in RIR_FFT_SIZES if need <= M), 0)


RIR_SEGMENTED = -1            # NWW_RIR_SEGMENTED: as M, the segmented route (clips and responses of any length)
RIR_SEG_TAPS = 16384          # taps of a partition, and outputs of a segment (csrc/rir_plan.h)


def rir_parts(N: int, max_ir_len: int) -> int:
    """nww_rir_parts: the partitions of a response of L taps against clips of N, ceil(min(L, N) / 16384); 0 for arguments below 1"""
    N, L = int(N), int(max_ir_len)
    if N < 1 or L < 1:
        return 0
    return -(-min(L, N) // RIR_SEG_TAPS)


def rir_spectra_floats(K: int, N: int, max_ir_len: int, M: int) -> int:
    """nww_rir_spectra_floats: the float32 values of a spectra buffer of K responses at M; 0 for bad arguments"""
    K, N, L, M = int(K), int(N), int(max_ir_len), int(M)
    if K < 1 or N < 1 or L < 1:
        return 0
    if M == RIR_SEGMENTED:
        return ((K + 2 + 3) & ~3) + K * rir_parts(N, L) * 32768
    return K * M if M in RIR_FFT_SIZES else 0


class IrArena:
    """Impulse responses for clips of N samples: float32 responses back to back (``offsets`` / ``lengths``, ``n`` of them), normalised
    on the host in float64 - ``"energy"``: sum h^2 = 1, ``"peak"``: max |h| = 1, None: as given (under peak normalisation of the clip the
    response's scale cancels) - and ``M``, the transform size that holds the longest.  With a device (the default, 0) the responses are
    uploaded ONCE and their spectra prepared ONCE, by the first model that uses the arena (``prepare(model)``); ``spectra_ptr`` is their
    device address.  ``device=None`` keeps the host side only.

    ``segmented=True`` lifts the limit of N + min(L, N) - 1 <= 32768: where no transform size fits, ``M`` is ``RIR_SEGMENTED`` and
    ``parts`` the partitions of the longest response (``rir_parts``); where one fits, ``M`` is that size, as without the argument
    (short clips keep the one-workgroup route and its bits) - unless ``M=RIR_SEGMENTED`` asks for the segmented route all the same."""

    def __init__(self, irs: Sequence[np.ndarray], N: int, device: Optional[int] = 0, normalize: Optional[str] = None, M: Optional[int] = None,
                 segmented: bool = False):
        """``M``: a transform size larger than the smallest that fits (the default), for a caller that wants one size for several arenas"""
        if normalize not in (None, "energy", "peak"):
            raise ValueError('normalize must be None, "energy" or "peak"')
        self.N = int(N)
        if segmented and self.N < 1:
            raise ValueError("a clip needs at least one sample")
        arrs = []
        for i, h in enumerate(irs):
            h = np.asarray(h)
            if h.ndim != 1 or h.size == 0 or h.dtype.kind != "f" or not np.isfinite(h).all():
                raise ValueError(f"response {i} must be a non-empty one-dimensional finite floating-point array")
            h64 = h.astype(np.float64)
            if normalize is not None:
                norm = float(np.sqrt((h64 * h64).sum())) if normalize == "energy" else float(np.abs(h64).max())
                if norm == 0.0:
                    raise ValueError(f"response {i} is all zeros and cannot be normalised")
                h64 = h64 / norm
            if not segmented and rir_fft_size(self.N, h.size) == 0:
                raise ValueError(f"response {i}: {h.size} taps against clips of {self.N} samples need more than 32768 points: "
                                 "overlap-save not built")
            arrs.append(h64.astype(np.float32))
        if not arrs:
            raise ValueError("an IrArena needs at least one response")
        self.lengths = np.array([a.size for a in arrs], np.int32)
        self.offsets = np.concatenate(([0], np.cumsum(self.lengths.astype(np.int64))[:-1])).astype(np.int64)
        self.n = len(arrs)
        self.M = rir_fft_size(self.N, int(self.lengths.max()))
        self.parts = 0
        if segmented and (self.M == 0 or (M is not None and int(M) == RIR_SEGMENTED)):
            # no transform size holds the longest response, or the caller wants this route for clips that one would hold
            if M is not None and int(M) != RIR_SEGMENTED:
                raise ValueError("these responses need the segmented route: M can only be RIR_SEGMENTED")
            self.M, self.parts = RIR_SEGMENTED, rir_parts(self.N, int(self.lengths.max()))
        elif M is not None:
            if int(M) not in RIR_FFT_SIZES or int(M) < self.M:
                raise ValueError(f"M must be one of {RIR_FFT_SIZES} and at least {self.M} for these responses")
            self.M = int(M)
        self.device = device
        self.host = np.concatenate(arrs)
        self._irs = self._spectra = None

    def __len__(self) -> int:
        return self.n

    def prepare(self, model) -> "IrArena":
        """upload and nww_rir_prepare_dev through `model` (a HipModel), once"""
        if self._spectra is None:
            if self.device is None:
                raise ValueError("an IrArena with device=None holds the host side only")
            import torch
            dev = f"cuda:{int(self.device)}"
            self._irs = torch.from_numpy(self.host).to(dev)
            if self.M == RIR_SEGMENTED:
                floats = int(model.lib.nww_rir_spectra_floats(self.n, self.N, int(self.lengths.max()), self.M))
                if floats != rir_spectra_floats(self.n, self.N, int(self.lengths.max()), self.M):
                    raise RuntimeError("nww_rir_spectra_floats disagrees with augment.rir_spectra_floats")
                spectra = torch.empty((floats,), dtype=torch.float32, device=dev)
            else:
                spectra = torch.empty((self.n, self.M), dtype=torch.float32, device=dev)
            model.rir_prepare_dev(self._irs.data_ptr(), self.offsets, self.lengths, self.N, self.M, spectra.data_ptr())
            self._spectra = spectra
        return self

    @property
    def spectra_ptr(self) -> int:
        if self._spectra is None:
            raise ValueError("the spectra are prepared by the first model that uses the arena: call prepare(model)")
        return int(self._spectra.data_ptr())


# struct nww_rir_item (include/nww.h): 8 bytes
RIR_ITEM = np.dtype([("ir_id", "<i4"), ("reserved", "<u4")])


def as_rir_items(ir_ids, B: int) -> np.ndarray:
    """a contiguous RIR_ITEM table of B rows from response ids (-1: none) or a RIR_ITEM table"""
    if isinstance(ir_ids, np.ndarray) and ir_ids.dtype == RIR_ITEM:
        t = np.ascontiguousarray(ir_ids)
    else:
        ids = np.asarray(ir_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("ir_ids must be a one-dimensional integer array (draw_rir_ids builds it) or a table of augment.RIR_ITEM")
        if ids.size and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):
            raise ValueError("ir_ids out of the int32 range")
        t = np.zeros(ids.size, RIR_ITEM)
        t["ir_id"] = ids
    if t.ndim != 1 or len(t) != B:
        raise ValueError(f"ir_ids must have one entry per item ({B}), got {t.shape}")
    return t


def draw_rir_ids(rng: np.random.Generator, n_irs: int, B: int, rir_prob: float = 0.5) -> np.ndarray:
    """What ApplyImpulseResponse(p=rir_prob) draws for B clips (augment_clips.py:150-157, rir_prob = 0.5): with that probability one of
    n_irs responses, uniformly, otherwise -1 (none) -> int32 [B].  The stream of random numbers is this function's own."""
    B = int(B)
    if int(n_irs) < 1:
        return np.full(B, -1, np.int32)
    on = rng.random(B) < float(rir_prob)
    return np.where(on, rng.integers(0, int(n_irs), B), -1).astype(np.int32)


# ---- pitch shift (nww_pitch_set_ratios / nww_mix_aug_*)
PITCH_MAX_TERM = 256          # a ratio's numerator and denominator
PITCH_MAX_RATIOS = 64         # the ratios a model holds at a time
PITCH_MIN_SAMPLES = 257       # clips of at most 256 samples cannot be reflect-padded


def pitch_ratio_ok(num: int, den: int) -> bool:
    """what nww_pitch_set_ratios accepts: terms in [1, 256] and 2^(-4/12) <= num / den <= 2^(4/12), decided in integers"""
    num, den = int(num), int(den)
    return 1 <= num <= PITCH_MAX_TERM and 1 <= den <= PITCH_MAX_TERM and num ** 3 <= 2 * den ** 3 and den ** 3 <= 2 * num ** 3


def pitch_ratios(min_semitones: float = -2.0, max_semitones: float = 2.0, max_den: int = 32):
    """The reduced fractions num / den with den <= max_den and 2^(min_semitones / 12) <= num / den <= 2^(max_semitones / 12), without 1,
    in ascending order -> [(num, den)].  The reference draws +-2 semitones (augment_clips.py:150-157); a call can name at most
    PITCH_MAX_RATIOS of them (the defaults list far more: pick, or lower max_den)."""
    from math import gcd
    lo, hi = 2.0 ** (float(min_semitones) / 12.0), 2.0 ** (float(max_semitones) / 12.0)
    out = []
    for den in range(1, int(max_den) + 1):
        for num in range(max(int(lo * den), 1), min(int(hi * den) + 1, PITCH_MAX_TERM) + 1):
            if num != den and gcd(num, den) == 1 and lo <= num / den <= hi and pitch_ratio_ok(num, den):
                out.append((num, den))
    return sorted(out, key=lambda r: (r[0] / r[1], r[1]))


class PitchBank:
    """The ratios (num, den) a call's pitch ids name, at most 64.  ``prepare(model)`` sets them on the model (nww_pitch_set_ratios builds
    the resampler tables and uploads them); a model holds one bank at a time, and a call with another bank sets that one."""

    def __init__(self, ratios: Sequence):
        r = [(int(a), int(b)) for a, b in ratios]
        if not r or len(r) > PITCH_MAX_RATIOS:
            raise ValueError(f"a PitchBank holds between 1 and {PITCH_MAX_RATIOS} ratios, got {len(r)}")
        for k, (a, b) in enumerate(r):
            if not pitch_ratio_ok(a, b):
                raise ValueError(f"ratio {k}: {a} / {b} out of range (terms in [1, 256], within +-4 semitones)")
        self.ratios = r
        self.num, self.den = np.array([a for a, _ in r], np.int32), np.array([b for _, b in r], np.int32)
        self.n = len(r)

    def __len__(self) -> int:
        return self.n

    def prepare(self, model) -> "PitchBank":
        if getattr(model, "_pitch_bank", None) is not self:
            model.pitch_set_ratios(self.num, self.den)
            model._pitch_bank = self
        return self


# struct nww_pitch_item (include/nww.h): 8 bytes
PITCH_ITEM = np.dtype([("pitch_id", "<i4"), ("reserved", "<u4")])


def as_pitch_items(pitch_ids, B: int) -> np.ndarray:
    """a contiguous PITCH_ITEM table of B rows from ratio ids (-1: none) or a PITCH_ITEM table"""
    if isinstance(pitch_ids, np.ndarray) and pitch_ids.dtype == PITCH_ITEM:
        t = np.ascontiguousarray(pitch_ids)
    else:
        ids = np.asarray(pitch_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("pitch_ids must be a one-dimensional integer array (draw_pitch_ids builds it) or a table of augment.PITCH_ITEM")
        if ids.size and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):
            raise ValueError("pitch_ids out of the int32 range")
        t = np.zeros(ids.size, PITCH_ITEM)
        t["pitch_id"] = ids
    if t.ndim != 1 or len(t) != B:
        raise ValueError(f"pitch_ids must have one entry per item ({B}), got {t.shape}")
    return t


def draw_pitch_ids(rng: np.random.Generator, n_ratios: int, B: int, pitch_prob: float = 0.5) -> np.ndarray:
    """What PitchShift(p=pitch_prob) draws for B clips (augment_clips.py:150-157, p = 0.5): with that probability one of n_ratios ratios,
    uniformly, otherwise -1 (none) -> int32 [B].  The stream of random numbers is this function's own."""
    B = int(B)
    if int(n_ratios) < 1:
        return np.full(B, -1, np.int32)
    on = rng.random(B) < float(pitch_prob)
    return np.where(on, rng.integers(0, int(n_ratios), B), -1).astype(np.int32)


# ---- recordings at their own sample rate (nww_resample_*)
# struct nww_resample_item (include/nww.h), field for field: 32 bytes
RESAMPLE_ITEM = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("src_frames", "<i4"), ("channels", "<i4"), ("rate_id", "<i4"), ("reserved", "<u4")])
RESAMPLE_TILE = 1024          # outputs a workgroup produces per tile (csrc/resample_plan.h)
RESAMPLE_MAX_TERM = 1024      # a ratio's numerator and denominator
RESAMPLE_MAX_RATIOS = 16      # the ratios a model holds at a time
RESAMPLE_MAX_FRAMES = 1 << 30
RESAMPLE_MAX_CHANNELS = 8
PCM_S16, PCM_F32 = 0, 1       # NWW_PCM_S16, NWW_PCM_F32


def resample_ratio_ok(num: int, den: int) -> bool:
    """what nww_resample_set_ratios accepts: terms in [1, 1024] and 1/4 <= num / den <= 12, decided in integers"""
    num, den = int(num), int(den)
    return 1 <= num <= RESAMPLE_MAX_TERM and 1 <= den <= RESAMPLE_MAX_TERM and den <= 4 * num and num <= 12 * den


def resample_ratio(src_hz: int, dst_hz: int = 16000):
    """(p, q) = (src_hz, dst_hz) / gcd - 48000 -> (3, 1), 44100 -> (441, 160), 22050 -> (441, 320) - or None when the rates are equal"""
    from math import gcd
    s, d = int(src_hz), int(dst_hz)
    if s != src_hz or d != dst_hz or s < 1 or d < 1:
        raise ValueError("sample rates must be positive integers")
    if s == d:
        return None
    g = gcd(s, d)
    p, q = s // g, d // g
    if not resample_ratio_ok(p, q):
        raise ValueError(f"{s} Hz -> {d} Hz is {p} / {q}: out of range (terms in [1, {RESAMPLE_MAX_TERM}], 1/4 <= ratio <= 12)")
    return p, q


def resampled_length(frames: int, src_hz: int, dst_hz: int = 16000) -> int:
    """the frames a recording has at dst_hz: ceil(frames q / p), as nww_resample_length; `frames` itself when the rates are equal"""
    r = resample_ratio(src_hz, dst_hz)
    frames = int(frames)
    if frames < 1 or frames > RESAMPLE_MAX_FRAMES:
        raise ValueError(f"a recording has between 1 and 2^30 frames (got {frames})")
    return frames if r is None else -(-frames * r[1] // r[0])


def as_resample_items(items) -> np.ndarray:
    """a contiguous one-dimensional RESAMPLE_ITEM table"""
    if not isinstance(items, np.ndarray) or items.dtype != RESAMPLE_ITEM or items.ndim != 1:
        raise ValueError("items must be a one-dimensional array of augment.RESAMPLE_ITEM")
    return np.ascontiguousarray(items)


def resample_plan(recordings: Sequence[np.ndarray], rates: Sequence[int], dst_hz: int = 16000, chunk_bytes: int = 64 << 20):
    """What HipModel.resample and ClipArena.from_recordings send: (the recordings as contiguous [frames, channels] arrays, their lengths
    at dst_hz as int64, the chunks).  A chunk is a run of consecutive recordings [lo, hi) of one sample format, of at most chunk_bytes
    of source (a longer recording goes alone) and at most RESAMPLE_MAX_RATIOS different ratios: a dict of lo, hi, format, ratios
    [(p, q)] and items - a RESAMPLE_ITEM table whose src_off count from the chunk's first value and whose dst_off pack the chunk's
    outputs back to back from 0."""
    if len(recordings) != len(rates):
        raise ValueError("one rate per recording")
    if len(recordings) == 0:
        raise ValueError("at least one recording is needed")
    recs, lens, ratios = [], [], []
    for i, (x, hz) in enumerate(zip(recordings, rates)):
        if not isinstance(x, np.ndarray) or x.dtype not in (np.int16, np.float32) or x.ndim not in (1, 2) or x.shape[0] == 0:
            raise ValueError(f"recording {i} must be a non-empty int16 or float32 array of shape [frames] or [frames, channels]")
        x = np.ascontiguousarray(x.reshape(x.shape[0], -1))
        if not 1 <= x.shape[1] <= RESAMPLE_MAX_CHANNELS:
            raise ValueError(f"recording {i} has {x.shape[1]} channels: between 1 and {RESAMPLE_MAX_CHANNELS} are taken")
        recs.append(x)
        lens.append(resampled_length(x.shape[0], hz, dst_hz))
        ratios.append(resample_ratio(hz, dst_hz))
    chunks, lo = [], 0
    while lo < len(recs):
        hi, size, rs = lo, 0, []
        while hi < len(recs) and recs[hi].dtype == recs[lo].dtype and (hi == lo or size + recs[hi].nbytes <= int(chunk_bytes)):
            if ratios[hi] is not None and ratios[hi] not in rs:
                if len(rs) == RESAMPLE_MAX_RATIOS:
                    break
                rs.append(ratios[hi])
            size += recs[hi].nbytes
            hi += 1
        t = np.zeros(hi - lo, RESAMPLE_ITEM)
        t["src_frames"] = [r.shape[0] for r in recs[lo:hi]]
        t["channels"] = [r.shape[1] for r in recs[lo:hi]]
        t["src_off"] = np.concatenate(([0], np.cumsum([r.size for r in recs[lo:hi]])[:-1]))
        t["dst_off"] = np.concatenate(([0], np.cumsum(lens[lo:hi])[:-1]))
        t["rate_id"] = [-1 if r is None else rs.index(r) for r in ratios[lo:hi]]
        chunks.append({"lo": lo, "hi": hi, "format": PCM_F32 if recs[lo].dtype == np.float32 else PCM_S16, "ratios": rs, "items": t})
        lo = hi
    return recs, np.array(lens, np.int64), chunks


class MixedClips:
    """The extractor generate_features runs over the tables of mixed_feature_batches: ``embed_clips(items)`` is
    ``features.embed_mixed(arena, items, N)`` - the mixed clips never exist on the host.  With ``irs`` (an IrArena) the batches are
    (items, ir_ids) pairs, with ``pitch`` (a PitchBank) (items, pitch_ids) pairs, with both (items, ir_ids, pitch_ids) triples, as
    mixed_feature_batches yields them when it is given the ids."""

    def __init__(self, features, arena: ClipArena, N: int, irs: Optional[IrArena] = None, pitch: Optional[PitchBank] = None):
        self.features, self.arena, self.N, self.irs, self.pitch = features, arena, int(N), irs, pitch

    def get_embedding_shape(self, audio_length_sec: float, sr: int = 16000):
        return self.features.get_embedding_shape(audio_length_sec, sr)

    def embed_clips(self, x, batch_size: int = 128, ncpu: int = 1) -> np.ndarray:
        if self.irs is None and self.pitch is None:
            return self.features.embed_mixed(self.arena, x, self.N)
        rest = list(x[1:])
        ir_ids = rest.pop(0) if self.irs is not None else None
        pitch_ids = rest.pop(0) if self.pitch is not None else None
        return self.features.embed_mixed(self.arena, x[0], self.N, irs=self.irs, ir_ids=ir_ids, pitch=self.pitch, pitch_ids=pitch_ids)


def mixed_feature_batches(items: np.ndarray, batch_size: int = 4096, irs: Optional[IrArena] = None, ir_ids=None,
                          pitch: Optional[PitchBank] = None, pitch_ids=None) -> Iterator:
    """`items` in tables of batch_size rows: what features.generate_features takes as its audio_batches when its extractor is a
    MixedClips - ``generate_features(mixed_feature_batches(items), len(items), path, MixedClips(feats, arena, N), N / 16000)``.
    With ``irs`` and ``ir_ids`` (one id per item) every batch is an (items, ir_ids) pair for ``MixedClips(..., irs=irs)``; with ``pitch``
    and ``pitch_ids`` the pitch ids follow, for ``MixedClips(..., pitch=pitch)``."""
    items = as_items(items)
    if (irs is None) != (ir_ids is None):
        raise ValueError("irs and ir_ids go together")
    if (pitch is None) != (pitch_ids is None):
        raise ValueError("pitch and pitch_ids go together")
    rt = None if ir_ids is None else as_rir_items(ir_ids, len(items))
    pt = None if pitch_ids is None else as_pitch_items(pitch_ids, len(items))
    step = max(int(batch_size), 1)
    for i in range(0, len(items), step):
        parts = [t[i:i + step] for t in (items, rt, pt) if t is not None]
        yield parts[0] if len(parts) == 1 else tuple(parts)
