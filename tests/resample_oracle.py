"""Recordings brought to the target rate (nww_resample_*, include/nww.h) in numpy: (i) the float64 DEFINITION - the
mean over the channels, torchaudio's default Resample restated as its construction (sinc_interp_hann, lowpass_filter_width 6, rolloff
0.99; output length ceil(L q / p)), the tail - and (ii) csrc/resample_plan.h in float32 with the same operation order, which the CPU
walk (tests/hostemu/resample_check.cpp) and the kernels (csrc/resample.hip) must equal bit for bit.  Shared by tests/test_resample_host.py,
tests/test_gpu_resample.py and tools/make_resample_golden.py."""
import json
import os

import numpy as np

F32, F64 = np.float32, np.float64
RESAMPLE_ITEM = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("src_frames", "<i4"), ("channels", "<i4"), ("rate_id", "<i4"), ("reserved", "<u4")])
TILE = 1024
MAX_TERM = 1024
MAX_RATIOS = 16
MAX_FRAMES = 1 << 30
S16, PCM_F32 = 0, 1                     # NWW_PCM_S16, NWW_PCM_F32

# 48 k, 32 k, 24 k, 44.1 k, 22.05 k, 8 k, 11.025 k and 96 k to 16 k
RATIOS = [(3, 1), (2, 1), (3, 2), (441, 160), (441, 320), (1, 2), (441, 640), (6, 1)]
RATIOS_AT_THE_BOUNDS = [(1, 4), (12, 1), (1024, 1023), (256, 1024)]
BAD_RATIOS = [(0, 1), (1, 0), (-3, 1), (1025, 1024), (1024, 1025), (1, 5), (255, 1024), (13, 1), (1024, 85)]
TAPS_MEASURED = {(3, 1): 38, (441, 160): 34, (441, 320): 18, (1, 2): 14, (441, 640): 14, (6, 1): 74, (12, 1): 146}


def ratio_ok(p: int, q: int) -> bool:
    return 1 <= p <= MAX_TERM and 1 <= q <= MAX_TERM and q <= 4 * p and p <= 12 * q


def half_width(p: int, q: int) -> int:
    """ceil(6 / c), c = 0.99 min(1, q / p), in integers"""
    return -(-200 * p // (33 * q)) if p > q else 7


def taps(p: int, q: int) -> int:
    return 2 * half_width(p, q)


def j0(p: int, q: int) -> int:
    return 1 - half_width(p, q)


def length(L: int, p: int, q: int) -> int:
    return -(-int(L) * q // p)


def frames_for(M: int, p: int, q: int) -> int:
    """the fewest frames that give at least M outputs (exactly M wherever some length does)"""
    return (M - 1) * p // q + 1


def table64(p: int, q: int) -> np.ndarray:
    """g [q, taps] in float64"""
    c = 0.99 * (q / p if q < p else 1.0)
    ph = np.arange(q, dtype=np.int64)
    frac = ((ph * p) % q).astype(F64) / float(q)
    x = frac[:, None] - (j0(p, q) + np.arange(taps(p, q), dtype=F64))[None, :]
    cx = c * x
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(cx == 0.0, 1.0, np.sin(np.pi * cx) / (np.pi * cx))
    h = np.cos(np.pi * cx / 12.0)
    return np.where(np.abs(cx) < 6.0, c * sinc * h * h, 0.0)


def table(p: int, q: int) -> np.ndarray:
    return table64(p, q).astype(F32)


def _frames(x) -> np.ndarray:
    x = np.asarray(x)
    assert x.dtype in (np.int16, np.float32) and x.ndim in (1, 2) and x.shape[0] >= 1
    return x.reshape(x.shape[0], -1)


def _gather(m, g, p, q, dtype):
    """v [M] = sum over ascending j of m[k0 + j] g[phase, j], taps outside the recording left out; every operation in `dtype`"""
    L = m.shape[0]
    n = np.arange(length(L, p, q), dtype=np.int64)
    phase = n % q
    k0 = (n // q) * p + (phase * p) // q + j0(p, q)
    acc = np.zeros(n.size, dtype)
    for j in range(g.shape[1]):
        k = k0 + j
        ok = (k >= 0) & (k < L)
        prod = m[np.clip(k, 0, L - 1)] * g[phase, j]
        acc = np.where(ok, acc + prod, acc)
    return acc


# ---- (ii) resample_plan.h in float32
def downmix(x) -> np.ndarray:
    x = _frames(x)
    if x.shape[1] == 1:
        return x[:, 0].astype(F32)
    a = np.zeros(x.shape[0], F32)
    for c in range(x.shape[1]):
        a = a + x[:, c].astype(F32)
    return a / F32(x.shape[1])


def out_f32(v, src_f32: bool) -> np.ndarray:
    return v.astype(F32) if src_f32 else (v * F32(2.0 ** -15)).astype(F32)


def out_s16(v, src_f32: bool) -> np.ndarray:
    u = v * F32(32768.0) if src_f32 else v
    u = np.where(u > F32(-32768.0), u, F32(-32768.0))
    u = np.where(u < F32(32767.0), u, F32(32767.0))
    return np.rint(u).astype(np.int16)


def restatement_v(x, ratio) -> np.ndarray:
    """the float32 samples before the tail; ratio None: a row with rate_id == -1"""
    m = downmix(x)
    return m if ratio is None else _gather(m, table(*ratio), ratio[0], ratio[1], F32)


def restatement(x, ratio, dst_dtype) -> np.ndarray:
    src_f32 = np.asarray(x).dtype == np.float32
    v = restatement_v(x, ratio)
    return out_f32(v, src_f32) if np.dtype(dst_dtype) == np.float32 else out_s16(v, src_f32)


# ---- (i) the definition in float64
def definition_v(x, ratio) -> np.ndarray:
    x = _frames(x).astype(F64)
    m = x.sum(axis=1) / x.shape[1]
    return m if ratio is None else _gather(m, table64(*ratio), ratio[0], ratio[1], F64)


def definition(x, ratio, dst_dtype) -> np.ndarray:
    src_f32 = np.asarray(x).dtype == np.float32
    v = definition_v(x, ratio)
    if np.dtype(dst_dtype) == np.float32:
        return (v if src_f32 else v / 32768.0).astype(F32)
    u = v * 32768.0 if src_f32 else v
    return np.rint(np.clip(u, -32768.0, 32767.0)).astype(np.int16)


# ---- signals
def speech_like(rng, L: int, C: int, fs: float, dtype, amp: float = 9000.0) -> np.ndarray:
    """two tones plus noise, a different mix per channel -> [L] (C == 1) or [L, C] of dtype (float32 in units of full scale)"""
    t = np.arange(L, dtype=F64)[:, None] / fs
    f1, f2 = rng.uniform(150.0, 400.0, C), rng.uniform(900.0, 2800.0, C)
    x = amp * (0.6 * np.sin(2 * np.pi * f1 * t + rng.uniform(0, 6, C)) + 0.3 * np.sin(2 * np.pi * f2 * t) + 0.1 * rng.standard_normal((L, C)))
    x = np.rint(x).astype(np.int16) if np.dtype(dtype) == np.int16 else (x / 32768.0).astype(F32)
    return x[:, 0].copy() if C == 1 else x


def square_wave(fs: int = 48000, hz: int = 500, L: int = 4800) -> np.ndarray:
    """full scale: +32767 / -32768"""
    half = fs // (2 * hz)
    return np.where((np.arange(L) // half) % 2 == 0, 32767, -32768).astype(np.int16)


def lengths(p: int, q: int):
    """the source lengths at which the walk and the kernel take another path: below the tap count, and both sides of a tile boundary"""
    return sorted({1, 2, taps(p, q) - 1, frames_for(TILE - 1, p, q), frames_for(TILE, p, q), frames_for(TILE + 1, p, q), frames_for(3 * TILE + 5, p, q)})


def pack(recordings, rate_ids, ratios, gap_every: int = 5, gap: int = 3):
    """(src [values], items, dst_values): the recordings back to back, destinations ascending with `gap` unwritten values behind every
    gap_every-th item"""
    items = np.zeros(len(recordings), RESAMPLE_ITEM)
    parts, so, do = [], 0, 0
    for i, (x, rid) in enumerate(zip(recordings, rate_ids)):
        fr = _frames(x)
        n = fr.shape[0] if rid < 0 else length(fr.shape[0], *ratios[rid])
        items[i] = (so, do, fr.shape[0], fr.shape[1], rid, 0)
        parts.append(fr.ravel())
        so += fr.size
        do += n + (gap if (i + 1) % gap_every == 0 else 0)
    return np.concatenate(parts), items, do


def item_lengths(items, ratios) -> np.ndarray:
    return np.array([int(it["src_frames"]) if it["rate_id"] < 0 else length(int(it["src_frames"]), *ratios[int(it["rate_id"])]) for it in items], np.int64)


ALL_RATIOS = RATIOS + RATIOS_AT_THE_BOUNDS
_CASES = {}


def shape_cases(src_dtype):
    """(recordings, rate_ids): every ratio of ALL_RATIOS x C in {1, 2, 3} x lengths(p, q), and rows without a ratio; computed once"""
    key = np.dtype(src_dtype).name
    if key not in _CASES:
        rng = np.random.default_rng(11 if key == "int16" else 12)
        recs, ids = [], []
        for rid, (p, q) in enumerate(ALL_RATIOS):
            for C in (1, 2, 3):
                for L in lengths(p, q):
                    recs.append(speech_like(rng, L, C, 16000.0 * p / q, src_dtype)); ids.append(rid)
        for C in (1, 2, 3):
            for L in (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
                recs.append(speech_like(rng, L, C, 16000.0, src_dtype)); ids.append(-1)
        _CASES[key] = (recs, ids)
    return _CASES[key]


_WANT = {}


def shape_want(src_dtype, dst_dtype):
    """the restatement's output for every recording of shape_cases(src_dtype); computed once"""
    key = (np.dtype(src_dtype).name, np.dtype(dst_dtype).name)
    if key not in _WANT:
        recs, ids = shape_cases(src_dtype)
        _WANT[key] = [restatement(x, None if r < 0 else ALL_RATIOS[r], dst_dtype) for x, r in zip(recs, ids)]
    return _WANT[key]


def bad_items(src_values: int, dst_values: int, K: int, good):
    """[(item, field)]: `good` (an item of a valid table, not its first) with one rule broken each"""
    out = []

    def bad(field, **kw):
        it = good.copy()
        for k, v in kw.items():
            it[k] = v
        out.append((it, field))
    bad("src_frames", src_frames=0); bad("src_frames", src_frames=-5); bad("src_frames", src_frames=MAX_FRAMES + 1)
    bad("channels", channels=0); bad("channels", channels=9)
    bad("src_off", src_off=-1); bad("src_off", src_off=src_values - int(good["src_frames"]) * int(good["channels"]) + 1)
    bad("rate_id", rate_id=-2); bad("rate_id", rate_id=K)
    bad("reserved", reserved=1)
    bad("dst_off", dst_off=int(good["dst_off"]) - 1); bad("dst_off", dst_off=dst_values)
    return out


# ---- the golden
GOLDEN_PAIRS = [(48000, 2), (44100, 1), (22050, 1), (8000, 1), (32000, 2), (24000, 1), (11025, 1), (96000, 1)]     # (source rate, channels)


def rate_ratio(fs: int, ft: int = 16000):
    g = int(np.gcd(fs, ft))
    return fs // g, ft // g


def golden_recordings():
    """speech-like clips of half a second at eight rates"""
    rng = np.random.default_rng(2026)
    return [speech_like(rng, fs // 2, C, float(fs), np.int16) for fs, C in GOLDEN_PAIRS]


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample.npz")


def load_golden():
    """(recordings, ratios, ref [list of int16 arrays], meta) of tests/golden/resample.npz"""
    z = np.load(golden_path(), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    recs = golden_recordings()
    assert [int(_frames(x).astype(np.int64).sum()) for x in recs] == meta["recording_sums"]
    ratios = [tuple(r) for r in z["ratios"].tolist()]
    ref, at = [], 0
    for n in z["lengths"].tolist():
        ref.append(z["ref"][at:at + n]); at += n
    return recs, ratios, ref, meta
