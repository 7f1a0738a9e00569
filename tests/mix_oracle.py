"""The arithmetic of a mixed clip (include/nww.h, nww_mix_*) restated in numpy, independent of csrc/mix_plan.h: int64 sums, float64
parameters, float32 samples with every product and sum rounded on its own (numpy contracts nothing).  Checker only.

Also the edge table the CPU check (tests/hostemu/mix_check.cpp) and the GPU tests share, and the bad items both must refuse."""
import json
import math
import os

import numpy as np

MIX_ITEM = np.dtype([("fg_off", "<i8"), ("bg_off", "<i8"), ("fg_len", "<i4"), ("bg_len", "<i4"), ("bg_start", "<i4"), ("start", "<i4"),
                     ("snr_linear", "<f4"), ("gain", "<f4"), ("level", "<f4"), ("flags", "<u4")])
F32 = np.float32


def scale_f32(Sf: int, Sb: int, fg_len: int, snr_linear) -> np.float32:
    eps = 2.0 ** -23
    den = float(fg_len) * 2.0 ** 30
    msf, msb = float(Sf) / den, float(Sb) / den
    fr = math.sqrt(msf + eps)
    br = max(math.sqrt(msb + eps), 0.005)
    scale = float(F32(snr_linear)) * br / fr
    srms = math.sqrt(scale * scale * msf + eps)
    if srms < 0.01:
        scale = scale * (0.01 / srms)
    return F32(scale)


def mix_clip(arena: np.ndarray, it, N: int) -> np.ndarray:
    fg_off, fg_len, bg_off, bg_len = int(it["fg_off"]), int(it["fg_len"]), int(it["bg_off"]), int(it["bg_len"])
    start, bg_start = int(it["start"]), int(it["bg_start"])
    fg = arena[fg_off:fg_off + fg_len].astype(np.int64)
    f = fg.astype(F32) / F32(32768)
    real = False
    if bg_len > 0:
        bgN = arena[bg_off + (bg_start + np.arange(N, dtype=np.int64)) % bg_len].astype(np.int64)
        real = int(np.abs(bgN).max()) >= 4
    x = np.zeros(N, F32)
    if real:
        seg = bgN[start:start + fg_len]
        s = scale_f32(int((fg * fg).sum()), int((seg * seg).sum()), fg_len, it["snr_linear"])
        b = bgN.astype(F32) / F32(32768)
        x[:] = b
        fs = f * s
        x[start:start + fg_len] = b[start:start + fg_len] + fs
    else:
        x[:fg_len] = f
    y = x * F32(it["gain"])
    if int(it["flags"]) & 1:
        pk = F32(np.abs(y).max())
        if pk < F32(1e-8):
            pk = F32(1.0)
        r = F32(it["level"]) / pk
    else:
        r = F32(it["level"])
    z = y * r
    assert y.dtype == F32 and z.dtype == F32 and isinstance(r, np.float32)
    return (np.clip(z, F32(-1.0), F32(1.0)) * F32(32767)).astype(np.int16)


def mix(arena: np.ndarray, items: np.ndarray, N: int) -> np.ndarray:
    out = np.empty((len(items), N), np.int16)
    for i, it in enumerate(items):
        out[i] = mix_clip(arena, it, N)
    return out


def bad_field(it, arena_samples: int, N: int):
    """the first rule of include/nww.h the item breaks, by field name, or None"""
    fg_len, bg_len = int(it["fg_len"]), int(it["bg_len"])
    if not 1 <= fg_len <= N:
        return "fg_len"
    if not 0 <= int(it["fg_off"]) <= arena_samples - fg_len:
        return "fg_off"
    if bg_len < 0:
        return "bg_len"
    if bg_len > 0:
        if not 0 <= int(it["bg_off"]) <= arena_samples - bg_len:
            return "bg_off"
        if not 0 <= int(it["bg_start"]) < bg_len:
            return "bg_start"
    if not 0 <= int(it["start"]) <= N - fg_len:
        return "start"
    for k in ("snr_linear", "gain", "level"):
        if not (np.isfinite(it[k]) and it[k] > 0):
            return k
    if int(it["flags"]) & ~1:
        return "flags"
    return None


def item(fg_off, fg_len, bg_off=0, bg_len=0, bg_start=0, start=0, snr=1.0, gain=1.0, level=1.0, flags=1):
    t = np.zeros(1, MIX_ITEM)
    t[0] = (fg_off, bg_off, fg_len, bg_len, bg_start, start, snr, gain, level, flags)
    return t


def edge_table(N: int, seed: int = 5):
    """(arena, items): every edge the kernel has at clip length N.  The arena starts with a one-sample pad and its clips have lengths
    of either parity, so that foreground and background offsets are odd and even in every combination; foregrounds of 1 and N samples at
    both ends of the clip and a middling one inside; no background and backgrounds of 7, N - 1, N and 3 N + 5 samples entered so that the
    read wraps inside the clip; peaks of 3 (no real background: the foreground alone at index 0) and 4; a background under the 0.005
    floor; an SNR under the 0.01 floor; an all-zero foreground; full-scale inputs; bit 0 clear with a gain * level that clips."""
    rng = np.random.default_rng(seed + N)
    clips, off = {}, {}
    parts = [np.array([1234], np.int16)]
    at = 1

    def add(name, a):
        nonlocal at
        a = np.asarray(a, np.int16)
        clips[name], off[name] = a, at
        parts.append(a)
        at += a.size

    noise = lambda n, amp: np.clip(np.rint(rng.standard_normal(n) * amp), -32768, 32767).astype(np.int16)
    add("fg", noise(N, 3000.0))
    add("bg7", noise(7, 5000.0))
    add("zero", np.zeros(N, np.int16))
    if N > 1:
        add("bgNm1", noise(N - 1, 2500.0))
    add("bgN", noise(N, 2500.0))
    add("full", np.where(np.arange(N) % 3 == 0, -32768, 32767))
    add("bg3N5", noise(3 * N + 5, 4000.0))
    p3 = rng.integers(-3, 4, N + 2); p3[0] = 3; p3[-1] = -3
    add("bgP3", p3)
    p4 = rng.integers(-3, 4, N + 3); p4[N // 2] = -4
    add("bgP4", p4)
    add("quiet", np.clip(noise(N + 1, 30.0), -100, 100) + np.where(np.arange(N + 1) == 0, 8, 0).astype(np.int16))
    add("fullbg", np.where(np.arange(N + 4) % 2 == 0, 32767, -32768))
    arena = np.concatenate(parts)

    def wrap_start(L):                 # enter the background so that its end falls inside the clip where it can
        return max(L - 1 - (N // 2) % L, 0)

    rows = []
    bgs = [None, "bg7", "bgNm1", "bgN", "bg3N5"]
    k = 0
    for fg_len in sorted({1, N}):
        for start in sorted({0, N - fg_len}):
            for bg in bgs:
                if bg is not None and bg not in clips:
                    continue
                k += 1
                fo = off["fg"] + (k % max(N - fg_len + 1, 1))
                kw = dict(start=start, snr=10.0 ** ((5 + 5 * (k % 6)) / 20.0), gain=10.0 ** (((k % 7) - 3) / 20.0), level=0.5 + (k % 6) * 0.1, flags=1)
                if bg is not None:
                    L = clips[bg].size
                    kw.update(bg_off=off[bg], bg_len=L, bg_start=wrap_start(L))
                rows.append(item(fo, fg_len, **kw))
                if k % 3 == 0:                                                           # the same without peak normalisation
                    rows.append(item(fo, fg_len, **dict(kw, flags=0, level=0.9)))
    m = max(N // 3, 1)
    rows.append(item(off["fg"] + min(1, N - m), m, off["bg3N5"] + 1, 2 * N + 3, 2 * N + 3 - max(N // 4, 1), (N - m) // 2, snr=3.0, gain=0.8, level=0.7))
    full = lambda name, **kw: item(off[name], N, **kw)
    rows += [
        full("fg", bg_off=off["bgP3"], bg_len=N + 2, bg_start=0, start=0, snr=2.0, level=0.6),             # P = 3: passthrough
        item(off["fg"], max(N // 2, 1), off["bgP3"], N + 2, 1, N - max(N // 2, 1), snr=2.0, level=0.6),    # ... start ignored
        full("fg", bg_off=off["bgP4"], bg_len=N + 3, bg_start=0, start=0, snr=2.0, level=0.6),             # P = 4: mixed
        full("fg", bg_off=off["quiet"], bg_len=N + 1, bg_start=0, snr=4.0, level=0.8),                     # 0.005 floor
        full("fg", bg_off=off["bgN"], bg_len=N, bg_start=N // 2, snr=1e-4, level=0.8),                     # 0.01 floor
        full("zero", bg_off=off["bgN"], bg_len=N, bg_start=0, snr=3.0, level=0.5),                         # silent foreground
        full("zero", level=0.5),                                                                          # ... alone: peak 0 counts as 1
        full("full", bg_off=off["fullbg"], bg_len=N + 4, bg_start=1, snr=1.0, gain=1.5, level=1.0),        # full scale, normalised
        full("full", bg_off=off["fullbg"], bg_len=N + 4, bg_start=N + 3, snr=1.0, gain=2.0, level=1.5, flags=0),   # clips
        full("full", gain=1.4, level=1.3, flags=0),                                                        # clips without a background
        full("fg", bg_off=off["bgN"], bg_len=N, bg_start=N - 1, snr=10.0, gain=1.2, level=0.9, flags=0),
    ]
    return arena, np.concatenate(rows)


def table_of(items: np.ndarray, B: int) -> np.ndarray:
    """B rows: the table's own, then its rows again at other SNRs and levels"""
    reps = -(-B // len(items))
    t = np.concatenate([items] * reps)[:B].copy()
    j = np.arange(B) // len(items)
    t["snr_linear"] *= (1.0 + 0.37 * j).astype(F32)
    t["level"] *= (1.0 - 0.11 * np.minimum(j, 5)).astype(F32)
    return t


def bad_items(arena_samples: int, N: int):
    """[(item, field)]: each kind of bad item; every field but the named one is valid"""
    g = dict(fg_off=1, fg_len=max(N // 2, 1), bg_off=2, bg_len=min(7, arena_samples - 2), bg_start=3 % min(7, arena_samples - 2), start=0,
             snr=2.0, gain=1.0, level=0.7, flags=1)
    out = []
    for field, kw in [("fg_len", dict(fg_len=0)), ("fg_len", dict(fg_len=N + 1)), ("fg_off", dict(fg_off=-1)),
                      ("fg_off", dict(fg_off=arena_samples - g["fg_len"] + 1)), ("bg_len", dict(bg_len=-1)), ("bg_off", dict(bg_off=-2)),
                      ("bg_off", dict(bg_off=arena_samples - g["bg_len"] + 1)), ("bg_start", dict(bg_start=g["bg_len"])),
                      ("bg_start", dict(bg_start=-1)), ("start", dict(start=N - g["fg_len"] + 1)), ("start", dict(start=-1)),
                      ("snr_linear", dict(snr=0.0)), ("snr_linear", dict(snr=float("nan"))), ("gain", dict(gain=float("inf"))),
                      ("gain", dict(gain=-1.0)), ("level", dict(level=0.0)), ("level", dict(level=float("nan"))), ("flags", dict(flags=2))]:
        out.append((item(**dict(g, **kw))[0], field))
    return out


# ---- the inputs of tests/golden/mix.npz (tools/make_mix_goldens.py): from integer arithmetic alone, the same on any numpy
def _hash_u64(n: int, key: int) -> np.ndarray:
    x = np.arange(n, dtype=np.uint64) + np.uint64((int(key) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)          # wraps mod 2^64
    x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def golden_clip(n: int, key: int, amp: int) -> np.ndarray:
    """n int16 samples: the sum of four 14-bit fields of a splitmix64 hash, centred (bell-shaped, |x| < 2^15), scaled by amp / 32768
    in integers, under an integer triangular envelope of period 4001 so that the level moves along the clip"""
    h = _hash_u64(n, key)
    s = sum(((h >> np.uint64(14 * k)) & np.uint64(0x3FFF)).astype(np.int64) for k in range(4)) - 2 * 0x3FFF
    tri = np.abs((np.arange(n, dtype=np.int64) + 37 * key) % 4001 - 2000) + 400          # 400 .. 2400
    return (s * amp * tri // (32768 * 2400)).astype(np.int16)


GOLDEN_FG = [(800, 9000), (1600, 20000), (3100, 2500), (5001, 30000), (8000, 12000), (12345, 700), (16000, 25000), (20011, 16000)]
GOLDEN_BG = [(53, 6000), (1000, 15000), (3777, 300), (16000, 9000), (30001, 20000), (48000, 4000)]


def golden_arena():
    """(arena, offsets, lengths): GOLDEN_FG's foregrounds then GOLDEN_BG's backgrounds, back to back behind a one-sample pad"""
    parts, offs, lens, at = [np.array([-7], np.int16)], [], [], 1
    for key, (n, amp) in enumerate(GOLDEN_FG + GOLDEN_BG):
        parts.append(golden_clip(n, key + 1, amp)); offs.append(at); lens.append(n); at += n
    return np.concatenate(parts), np.array(offs, np.int64), np.array(lens, np.int64)


def load_golden():
    """(arena, items, ref, meta) of tests/golden/mix.npz; the arena is rebuilt and checked against the sums the file was made from"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mix.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    arena, _, _ = golden_arena()
    assert arena.size == meta["arena_samples"] and int(arena.astype(np.int64).sum()) == meta["arena_sum"]
    items = z["items"]
    assert items.dtype == MIX_ITEM and len(items) == meta["items"] == 40
    return arena, items, z["ref"], meta


def golden_conditions(out: np.ndarray, ref: np.ndarray) -> float:
    """the two conditions on clips against the reference's: no sample off by more than 1 LSB, and at most 0.5 % of them off at all (the
    reference sums its 16 000 squares in float32: its scale is a few ulps off, which moves a sample by ~0.01 LSB and flips few
    truncations - the cap keeps the 1-LSB allowance from hiding a wrong scale) -> the share"""
    d = np.abs(out.astype(np.int32) - ref.astype(np.int32))
    share = float((d > 0).mean())
    print(f"max |d| = {int(d.max())} LSB, differing samples {int((d > 0).sum())} of {d.size} ({100 * share:.4f} %)")
    assert int(d.max()) <= 1
    assert share <= 0.005
    return share
