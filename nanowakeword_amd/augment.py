"""Clips mixed on the device (nww_mix_*, include/nww.h): the caller side.

The reference mixes every foreground into a random background at a random SNR on the host, levels the batch and quantises it to int16
(``augment_clips``, nanowakeword/data/augment_clips.py:170-261; ``_mix_snr``, :45-79).  What is random there is the draw of the
parameters; here the host draws them (``draw_mix_items``) or lays them out as a grid (``mix_items``), ONE table per batch goes to the
device, and the recordings - uploaded once as a ``ClipArena`` - are gathered, measured and mixed there (``HipModel.mix`` /
``forward_mixed``, ``HipFeatures.embed_mixed``).  A robustness sweep of 1 000 positives x 20 noises x 6 SNRs is 120 000 table rows over
1 020 recordings.

Not restated: pitch shift and impulse responses (``torch_audiomentations``' PitchShift / ApplyImpulseResponse, augment_clips.py:150-157);
``gain`` is the reference's Gain step, ``level`` its volume step (:246-255).
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


class MixedClips:
    """The extractor generate_features runs over the tables of mixed_feature_batches: ``embed_clips(items)`` is
    ``features.embed_mixed(arena, items, N)`` - the mixed clips never exist on the host."""

    def __init__(self, features, arena: ClipArena, N: int):
        self.features, self.arena, self.N = features, arena, int(N)

    def get_embedding_shape(self, audio_length_sec: float, sr: int = 16000):
        return self.features.get_embedding_shape(audio_length_sec, sr)

    def embed_clips(self, x: np.ndarray, batch_size: int = 128, ncpu: int = 1) -> np.ndarray:
        return self.features.embed_mixed(self.arena, x, self.N)


def mixed_feature_batches(items: np.ndarray, batch_size: int = 4096) -> Iterator[np.ndarray]:
    """`items` in tables of batch_size rows: what features.generate_features takes as its audio_batches when its extractor is a
    MixedClips - ``generate_features(mixed_feature_batches(items), len(items), path, MixedClips(feats, arena, N), N / 16000)``."""
    items = as_items(items)
    step = max(int(batch_size), 1)
    for i in range(0, len(items), step):
        yield items[i:i + step]
