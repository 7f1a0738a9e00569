"""Clips shifted in pitch (include/nww.h, nww_pitch_* / nww_mix_aug_*), for the checks - three things, all independent of
csrc/pitch_plan.h:

(i)   THE DEFINITION in float64 (`definition_y`): torch.stft / torch.istft in float64, the textbook phase vocoder - np.angle, the expected
      advance subtracted, the wrap to (-pi, pi], the advance added back, cumsum, polar - and the resampler as the direct sum.
(ii)  the same definition in float32 torch ops (`yardstick_y`): what the restatement's error is measured against.
(iii) a float32 RESTATEMENT of pitch_plan.h (`shift`): frames, the packed radix-4 network, the recurrence on unit vectors, the overlap-add
      and the tap sums, every product and sum a numpy float32 operation of its own.  It is the bridge for the bit-for-bit checks of the
      CPU walk and the kernels, as rir_oracle is for rir.hip.

Also the test clips, the bad items both sides must refuse, and the loader of tests/golden/pitch.npz (tools/make_pitch_goldens.py).
Checker only."""
import json
import os
from fractions import Fraction

import numpy as np

import mix_oracle
import rir_oracle
from mix_oracle import F32

F64 = np.float64
PITCH_ITEM = np.dtype([("pitch_id", "<i4"), ("reserved", "<u4")])
NFFT, HOP, H, D, TAPS, TAP0 = 512, 128, 256, 4, 16, -7
RATIOS = [(9, 8), (8, 9), (16, 15), (24, 25), (128, 125), (255, 256)]


def ratio_ok(p: int, q: int) -> bool:
    return 1 <= p <= 256 and 1 <= q <= 256 and p ** 3 <= 2 * q ** 3 and q ** 3 <= 2 * p ** 3


def frames(N): return 1 + N // HOP
def out_frames(T, p, q): return -(-T * p // q)
def stretched(T_out): return HOP * (T_out - 1)
def resampled(S, p, q): return -(-S * q // p)


# ---- (i) the definition, float64, and (ii) the yardstick, the same in float32
def _g(x, c):
    cx = c * x
    return np.where(np.abs(cx) < 6.0, c * np.sinc(cx) * np.cos(np.pi * cx / 12.0) ** 2, 0.0)


def _definition(w: np.ndarray, p: int, q: int, dt):
    import torch
    tdt = torch.float64 if dt == F64 else torch.float32
    N = w.size
    win = torch.hann_window(NFFT, periodic=True, dtype=tdt)
    X = torch.stft(torch.from_numpy(w.astype(dt)), NFFT, HOP, window=win, center=True, pad_mode="reflect", return_complex=True).numpy()   # [257, T]
    T = X.shape[1]
    assert T == frames(N) and X.shape[0] == 257
    T_out = out_frames(T, p, q)
    t = np.arange(T_out, dtype=np.int64)
    i, alpha = (t * q) // p, (((t * q) % p).astype(dt) / dt(p))
    Xz = np.concatenate([X, np.zeros((257, 2), X.dtype)], axis=1)
    X0, X1 = Xz[:, i], Xz[:, i + 1]
    mag = alpha * np.abs(X1) + (dt(1) - alpha) * np.abs(X0)
    adv = (np.linspace(0, np.pi * HOP, 257).astype(dt))[:, None]
    dphi = np.angle(X1) - np.angle(X0) - adv
    dphi = dphi - dt(2 * np.pi) * np.round(dphi / dt(2 * np.pi))                    # wrapped to [-pi, pi]
    dphi = (dphi + adv).astype(dt)
    phase = np.concatenate([np.angle(X[:, :1]).astype(dt), dphi[:, :-1]], axis=1)
    phase = np.cumsum(phase, axis=1, dtype=dt)
    Y = (mag * np.cos(phase) + 1j * (mag * np.sin(phase))).astype(np.complex128 if dt == F64 else np.complex64)
    s = torch.istft(torch.from_numpy(Y), NFFT, HOP, window=win, center=True).numpy()
    S = stretched(T_out)
    assert s.size == S and s.dtype == dt
    Ly = resampled(S, p, q)
    c = dt(0.99 * min(1.0, q / p))
    n = np.arange(min(Ly, N), dtype=np.int64)
    y = np.zeros(N, dt)
    pos = (n * p).astype(F64) / q
    k0 = np.floor(pos).astype(np.int64)
    acc = np.zeros(n.size, dt)
    for d in range(-9, 11):
        k = k0 + d
        ok = (k >= 0) & (k < S)
        acc = acc + np.where(ok, s[np.clip(k, 0, S - 1)], 0) * _g((pos - k).astype(dt), c).astype(dt)
    y[:n.size] = acc
    assert y.dtype == dt
    return y


def definition_y(w, p, q) -> np.ndarray:
    return _definition(w, p, q, F64)


def yardstick_y(w, p, q) -> np.ndarray:
    return _definition(w, p, q, F32)


def definition(arena, items, pitch_ids, ratios, N: int) -> np.ndarray:
    """the int16 clips of the definition: the float64 tail behind the float64 shift; clips without a ratio are mix_oracle's"""
    out = np.empty((len(items), N), np.int16)
    for i, it in enumerate(items):
        y = rir_oracle.mix_y(arena, it, N)
        k = int(pitch_ids[i])
        out[i] = rir_oracle.tail64(definition_y(y, *ratios[k]), it) if k >= 0 else rir_oracle.tail(y, it)
    return out


# ---- (iii) pitch_plan.h in float32
def window():
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT, dtype=F64) / NFFT)).astype(F32)


def env_table(win):
    e = np.zeros((16, HOP), F64)
    w2 = win.astype(F64) ** 2
    for m in range(16):
        for c in (3, 2, 1, 0):
            if m >> c & 1:
                e[m] = e[m] + w2[HOP * c:HOP * c + HOP]
    return e.astype(F32)


def resample_table(p: int, q: int):
    c = 0.99 * (q / p if q < p else 1.0)
    ph = np.arange(q, dtype=np.int64)
    frac = ((ph * p) % q).astype(F64) / float(q)
    x = frac[:, None] - (TAP0 + np.arange(TAPS, dtype=F64))[None, :]
    cx = c * x
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(cx == 0.0, 1.0, np.sin(np.pi * cx) / (np.pi * cx))
    h = np.cos(np.pi * cx / 12.0)
    return np.where(np.abs(cx) < 6.0, c * sinc * h * h, 0.0).astype(F32)


_TAB = {}


def tables():
    if not _TAB:
        win = window()
        pos = np.arange(1, H // 2)
        pk = ((pos >> 1) << 2) | (pos & 1)
        k = rir_oracle.rev(pk, D)
        pk, k = np.append(pk, 2), np.append(k, H // 2)
        _TAB.update(T=rir_oracle.twiddles(NFFT), win=win, env=env_table(win), pk=pk, pm=rir_oracle.rev(H - k, D), k=k)
    return _TAB


def _views(zr, zi, s):
    return zr.reshape(-1, H // (4 * s), 4, s), zi.reshape(-1, H // (4 * s), 4, s)


def _forward(zr, zi, T):
    """rir_oracle.forward over rows [F, 256]"""
    s = H // 4
    while s >= 1:
        vr, vi = _views(zr, zi, s)
        j = np.arange(s) * (NFFT // (4 * s))
        a = [(vr[:, :, m, :].copy(), vi[:, :, m, :].copy()) for m in range(4)]
        b0 = (a[0][0] + a[2][0], a[0][1] + a[2][1]); b1 = (a[0][0] - a[2][0], a[0][1] - a[2][1])
        b2 = (a[1][0] + a[3][0], a[1][1] + a[3][1]); b3 = (a[1][0] - a[3][0], a[1][1] - a[3][1])
        ib3 = (-b3[1], b3[0])
        vr[:, :, 0, :], vi[:, :, 0, :] = b0[0] + b2[0], b0[1] + b2[1]
        vr[:, :, 1, :], vi[:, :, 1, :] = rir_oracle._mulc(b1[0] - ib3[0], b1[1] - ib3[1], T[0][j], T[1][j])
        vr[:, :, 2, :], vi[:, :, 2, :] = rir_oracle._mulc(b0[0] - b2[0], b0[1] - b2[1], T[0][2 * j], T[1][2 * j])
        vr[:, :, 3, :], vi[:, :, 3, :] = rir_oracle._mulc(b1[0] + ib3[0], b1[1] + ib3[1], T[0][3 * j], T[1][3 * j])
        s //= 4


def _inverse(zr, zi, T):
    s = 1
    while s <= H // 4:
        vr, vi = _views(zr, zi, s)
        j = np.arange(s) * (NFFT // (4 * s))
        a0 = (vr[:, :, 0, :].copy(), vi[:, :, 0, :].copy())
        a1 = rir_oracle._mul(vr[:, :, 1, :], vi[:, :, 1, :], T[0][j], T[1][j])
        a2 = rir_oracle._mul(vr[:, :, 2, :], vi[:, :, 2, :], T[0][2 * j], T[1][2 * j])
        a3 = rir_oracle._mul(vr[:, :, 3, :], vi[:, :, 3, :], T[0][3 * j], T[1][3 * j])
        b0 = (a0[0] + a2[0], a0[1] + a2[1]); b1 = (a0[0] - a2[0], a0[1] - a2[1])
        b2 = (a1[0] + a3[0], a1[1] + a3[1]); b3 = (a1[0] - a3[0], a1[1] - a3[1])
        ib3 = (-b3[1], b3[0])
        vr[:, :, 0, :], vi[:, :, 0, :] = b0[0] + b2[0], b0[1] + b2[1]
        vr[:, :, 1, :], vi[:, :, 1, :] = b1[0] + ib3[0], b1[1] + ib3[1]
        vr[:, :, 2, :], vi[:, :, 2, :] = b0[0] - b2[0], b0[1] - b2[1]
        vr[:, :, 3, :], vi[:, :, 3, :] = b1[0] - ib3[0], b1[1] - ib3[1]
        s *= 4


def stft(w: np.ndarray):
    """(re, im) [T + 1, 256] by position, 2 X; position 0 holds (2 X[0], 2 X[256]); the last frame is zero"""
    tb = tables()
    N, T = w.size, frames(w.size)
    idx = HOP * np.arange(T)[:, None] + np.arange(NFFT)[None, :] - NFFT // 2
    idx = np.where(idx < 0, -idx, np.where(idx >= N, 2 * (N - 1) - idx, idx))
    f = np.zeros((T + 1, NFFT), F32)
    f[:T] = w[idx] * tb["win"][None, :]
    zr, zi = f[:, 0::2].copy(), f[:, 1::2].copy()
    _forward(zr, zi, tb["T"])
    pk, pm, k = tb["pk"], tb["pm"], tb["k"]
    z0r, z0i = zr[:, 0].copy(), zi[:, 0].copy()
    (xkr, xki), (xmr, xmi) = rir_oracle._split(zr[:, pk], zi[:, pk], zr[:, pm], zi[:, pm], tb["T"][0][k], tb["T"][1][k])
    zr[:, pm], zi[:, pm] = xmr, xmi
    zr[:, pk], zi[:, pk] = xkr, xki
    s0, d0 = z0r + z0i, z0r - z0i
    zr[:, 0], zi[:, 0] = s0 + s0, d0 + d0
    assert zr.dtype == F32
    return zr, zi


def _polar(re, im):
    s = re * re + im * im
    zero = s == 0
    r = np.sqrt(np.where(zero, F32(1), s))
    assert r.dtype == F32
    return np.where(zero, F32(1), re / r), np.where(zero, F32(0), im / r), np.where(zero, F32(0), r)


def _bin(x0r, x0i, x1r, x1i, alpha, ur, ui):
    e0r, e0i, m0 = _polar(x0r, x0i)
    e1r, e1i, m1 = _polar(x1r, x1i)
    om = F32(1) - alpha
    mag = alpha * m1 + om * m0
    yr, yi = mag * ur, mag * ui
    ar, ai = rir_oracle._mul(ur, ui, e1r, e1i)
    br, bi = rir_oracle._mulc(ar, ai, e0r, e0i)
    nr, ni, _ = _polar(br, bi)
    return yr, yi, nr, ni


def vocoder(Xr, Xi, p: int, q: int):
    """output frames by position (re, im) [T_out, 256]"""
    T = Xr.shape[0] - 1
    T_out = out_frames(T, p, q)
    Yr, Yi = np.zeros((T_out, H), F32), np.zeros((T_out, H), F32)
    z = np.zeros(1, F32)
    ur, ui, _ = _polar(Xr[0], Xi[0])
    u0r, u0i, _ = _polar(Xr[0, :1], z)
    uhr, uhi, _ = _polar(Xi[0, :1], z)
    for t in range(T_out):
        i, m = divmod(t * q, p)
        alpha = F32(m) / F32(p)
        yr, yi, ur, ui = _bin(Xr[i], Xi[i], Xr[i + 1], Xi[i + 1], alpha, ur, ui)
        y0, _, u0r, u0i = _bin(Xr[i, :1], z, Xr[i + 1, :1], z, alpha, u0r, u0i)
        yh, _, uhr, uhi = _bin(Xi[i, :1], z, Xi[i + 1, :1], z, alpha, uhr, uhi)
        Yr[t], Yi[t] = yr, yi
        Yr[t, 0], Yi[t, 0] = y0[0], yh[0]
    return Yr, Yi


def istft(Yr, Yi):
    """[T_out, 256] by position -> s [128 (T_out - 1)]"""
    tb = tables()
    T_out = Yr.shape[0]
    zr, zi = Yr.copy(), Yi.copy()
    pk, pm, k = tb["pk"], tb["pm"], tb["k"]
    wr, wi = tb["T"][0][k], tb["T"][1][k]
    ykr, yki, ymr, ymi = zr[:, pk], zi[:, pk], zr[:, pm], zi[:, pm]
    y0, yh = zr[:, 0].copy(), zi[:, 0].copy()
    ar, ai = ykr + ymr, yki - ymi
    br, bi = ykr - ymr, yki - (-ymi)
    orr, oi = rir_oracle._mul(br, bi, wr, wi)
    zr[:, pm], zi[:, pm] = ar + oi, orr - ai
    zr[:, pk], zi[:, pk] = ar - oi, ai + orr
    zr[:, 0], zi[:, 0] = y0 + yh, y0 - yh
    _inverse(zr, zi, tb["T"])
    v = np.empty((T_out, NFFT), F32)
    v[:, 0::2], v[:, 1::2] = zr, zi
    o = (v * F32(2.0 ** -10)) * tb["win"][None, :]
    acc = np.zeros(HOP * (T_out + 3), F32)
    for t in range(T_out):
        acc[HOP * t:HOP * t + NFFT] = acc[HOP * t:HOP * t + NFFT] + o[t]
    S = stretched(T_out)
    P = np.arange(S) + NFFT // 2
    fl = P // HOP
    mask = np.zeros(S, np.int64)
    for c in range(4):
        mask |= (((fl - c) >= 0) & ((fl - c) < T_out)).astype(np.int64) << c
    s = acc[P] / tb["env"][mask, P % HOP]
    assert s.dtype == F32
    return s


def resample(s: np.ndarray, p: int, q: int, N: int) -> np.ndarray:
    S = s.size
    g = resample_table(p, q)
    Ly = resampled(S, p, q)
    n = np.arange(min(N, Ly), dtype=np.int64)
    ph = n % q
    k0 = (n // q) * p + (ph * p) // q + TAP0
    acc = np.zeros(n.size, F32)
    for j in range(TAPS):
        k = k0 + j
        ok = (k >= 0) & (k < S)
        acc = np.where(ok, acc + s[np.clip(k, 0, S - 1)] * g[ph, j], acc)
    assert acc.dtype == F32
    y = np.zeros(N, F32)
    y[:n.size] = acc
    return y


def shift(w: np.ndarray, p: int, q: int) -> np.ndarray:
    """w [N] float32 -> y [N] float32: the restatement of pitch_clip_host"""
    assert w.dtype == F32 and w.size > 256
    Xr, Xi = stft(w)
    return resample(istft(*vocoder(Xr, Xi, p, q)), p, q, w.size)


def mix_aug_y(arena, it, pitch_id, ratios, N):
    y = rir_oracle.mix_y(arena, it, N)
    return shift(y, *ratios[int(pitch_id)]) if int(pitch_id) >= 0 else y


def mix_aug(arena, items, pitch_ids, ratios, N: int, ir_ids=None, irs=None, M: int = 0, after=None) -> np.ndarray:
    """the clips of nww_mix_aug: mix_y, the shift (pitch_id >= 0), the response (ir_id >= 0; `after(w, k)` if given, else rir_oracle's
    network at M), the tail"""
    T = rir_oracle.twiddles(M) if M in rir_oracle.SIZES else None
    specs = {}
    out = np.empty((len(items), N), np.int16)
    for i, it in enumerate(items):
        w = mix_aug_y(arena, it, pitch_ids[i], ratios, N)
        k = -1 if ir_ids is None else int(ir_ids[i])
        if k >= 0:
            if after is not None:
                w = after(w, k)
            else:
                if k not in specs:
                    specs[k] = rir_oracle.prepare(irs[k], N, M, T)
                w = rir_oracle.convolve(w, specs[k], M, T)
        out[i] = rir_oracle.tail(w, it)
    return out


def pitch_items(ids) -> np.ndarray:
    t = np.zeros(len(ids), PITCH_ITEM)
    t["pitch_id"] = ids
    return t


def bad_pitch_items(K: int):
    out = []
    for pid, reserved, field in [(-2, 0, "pitch_id"), (K, 0, "pitch_id"), (2 ** 31 - 1, 0, "pitch_id"), (0, 1, "reserved"), (-1, 9, "reserved")]:
        t = np.zeros(1, PITCH_ITEM)
        t[0] = (pid, reserved)
        out.append((t[0], field))
    return out


# 2^(1/3) = 1.259921..: 34/27 = 1.259259 lies inside, 63/50 = 1.26 outside
BAD_RATIOS = [(0, 1), (1, 0), (257, 256), (256, 257), (-9, -8), (4, 3), (3, 4), (63, 50), (50, 63), (100, 126), (127, 100)]
GOOD_RATIOS_AT_THE_BOUNDS = [(1, 1), (256, 256), (5, 4), (4, 5), (34, 27), (27, 34)]


# ---- inputs
def golden_inputs():
    """mix.npz's arena and its items with a background (broadband: no bin sits at the rounding floor while its neighbours are loud)"""
    arena, items, _, meta = mix_oracle.load_golden()
    return arena, items[items["bg_len"] > 0], meta["N"] if "N" in meta else None


def clip_table(N: int):
    """(arena, items): the rows the GPU and CPU checks share, seven of them - three of mix_oracle.edge_table(N) with a background, one
    without; an ISLAND, a recording appended to the arena that is exact zeros over its first 40 % and its last 30 % and noise between,
    taken whole without a background, so that whole frames of exact zeros (the unit(0) path) lead into loud ones and follow them; a
    foreground shorter than N without a background (mix_plan.h ignores its start: exact zeros behind it only); and a short foreground
    inside a background.  Exact zeros AHEAD of a foreground come from the island alone: a background of zeros is not a real one."""
    arena, items = mix_oracle.edge_table(N)
    rng = np.random.default_rng(1000 + N)
    island = np.zeros(N, np.int16)
    lo, hi = (2 * N) // 5, N - (3 * N) // 10
    island[lo:hi] = np.clip(np.rint(rng.standard_normal(hi - lo) * 6000.0), -32768, 32767).astype(np.int16)
    island_row = mix_oracle.item(arena.size, N, gain=0.9, level=0.85)
    arena = np.concatenate([arena, island])
    with_bg = items[(items["bg_len"] > 7) & (items["fg_len"] == N)][:3]
    no_bg = items[(items["bg_len"] == 0) & (items["fg_len"] == N)][:1]
    short = mix_oracle.item(int(no_bg[0]["fg_off"]), max(N // 3, 1), gain=1.1, level=0.8)
    mid = items[(items["bg_len"] > 7) & (items["fg_len"] < N) & (items["fg_len"] > 1)][:1]
    return arena, np.concatenate([with_bg, no_bg, island_row, short, mid])


def load_golden():
    """(arena, items, pitch_ids, ratios, ref, meta) of tests/golden/pitch.npz"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pitch.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    arena, _, _ = mix_oracle.golden_arena()
    assert arena.size == meta["arena_samples"] and int(arena.astype(np.int64).sum()) == meta["arena_sum"]
    return arena, z["items"], z["pitch_ids"], [tuple(r) for r in z["ratios"].tolist()], z["ref"], meta


def reduced_ratios(min_semitones=-2.0, max_semitones=2.0, max_den=32):
    """what augment.pitch_ratios lists, from Fractions"""
    lo, hi = 2.0 ** (min_semitones / 12.0), 2.0 ** (max_semitones / 12.0)
    out = set()
    for q in range(1, max_den + 1):
        for p in range(1, 257):
            f = Fraction(p, q)
            if f != 1 and lo <= p / q <= hi and f.denominator == q and f.numerator <= 256:
                out.add((f.numerator, f.denominator))
    return sorted(out, key=lambda r: (r[0] / r[1], r[1]))


# ---- the restatement against the definition, with the float32 torch route as the yardstick
def accuracy_clips():
    """(arena, items, N, ratio per clip): every item of tests/golden/mix.npz that has a background, each at one of RATIOS in turn"""
    arena, items, _, meta = mix_oracle.load_golden()
    sel = items[items["bg_len"] > 0]
    return arena, sel, int(meta["N"]), [RATIOS[i % len(RATIOS)] for i in range(len(sel))]


def accuracy(arena, items, N, ratios):
    """per clip (max-abs ratio, rms ratio, share of int16 samples that differ from the definition's, largest difference in LSB): the
    restatement's error against the float64 definition over the yardstick's"""
    rows = []
    for it, (p, q) in zip(items, ratios):
        w = rir_oracle.mix_y(arena, it, N)
        d, y, ys = definition_y(w, p, q), shift(w, p, q), yardstick_y(w, p, q)
        e, ey = y.astype(F64) - d, ys.astype(F64) - d
        di = np.abs(rir_oracle.tail(y, it).astype(np.int32) - rir_oracle.tail64(d, it).astype(np.int32))
        rows.append((float(np.abs(e).max() / np.abs(ey).max()), float(np.sqrt((e ** 2).mean()) / np.sqrt((ey ** 2).mean())),
                     float((di > 0).mean()), int(di.max())))
    return rows


# ---- tests/golden/pitch.npz (tools/make_pitch_goldens.py): four items at N = 4000 out of mix_oracle's golden arena
GOLDEN_N = 4000
GOLDEN_RATIOS = [(9, 8), (15, 16), (128, 125)]
GOLDEN_IDS = [0, 1, 2, -1]


def golden_items():
    _, offs, lens = mix_oracle.golden_arena()
    nfg = len(mix_oracle.GOLDEN_FG)
    rows = [mix_oracle.item(int(offs[2]), 3100, int(offs[nfg + 3]), int(lens[nfg + 3]), 5000, 450, snr=3.0, gain=1.2, level=0.9),
            mix_oracle.item(int(offs[1]), 1600, int(offs[nfg + 1]), int(lens[nfg + 1]), 777, 2400, snr=6.0, gain=0.8, level=0.7),
            mix_oracle.item(int(offs[4]) + 100, 4000, int(offs[nfg + 4]), int(lens[nfg + 4]), 29000, 0, snr=1.5, gain=1.0, level=1.0),
            mix_oracle.item(int(offs[0]), 800, int(offs[nfg + 5]), int(lens[nfg + 5]), 123, 3200, snr=10.0, gain=1.4, level=0.5)]
    return np.concatenate(rows)
