"""Clips through a room impulse response (include/nww.h, nww_mix_rir_* / nww_rir_*), for the checks - two things, both independent of
csrc/rir_plan.h:

(i)  THE DEFINITION in float64: np.convolve of mix_oracle's float32 y with h, cut to N, then the tail in float64 (`definition`).
(ii) a float32 RESTATEMENT of the network of rir_plan.h (`mix_rir`): the packed radix-4 transform, the pair stage and the inverse, each
     stage vectorised over its butterflies, every product and sum a numpy float32 operation of its own (numpy contracts nothing).  It is
     the bridge for the bit-for-bit checks of the CPU walk and the kernel, as mix_oracle is for mix.hip.

Also the edge cases the CPU check (tests/hostemu/rir_check.cpp) and the GPU tests share, the bad items both must refuse, and the loader
of tests/golden/rir.npz (tools/make_rir_goldens.py).  Checker only."""
import json
import os

import numpy as np

import mix_oracle
from mix_oracle import F32, scale_f32

RIR_ITEM = np.dtype([("ir_id", "<i4"), ("reserved", "<u4")])
SIZES = (2048, 8192, 32768)
F64 = np.float64


def fft_size(N: int, L: int) -> int:
    need = N + min(L, N) - 1
    for M in SIZES:
        if need <= M:
            return M
    return 0


def digits(M: int) -> int:
    return {2048: 5, 8192: 6, 32768: 7}[M]


def rev(k, D: int):
    k = np.asarray(k, np.int64).copy()
    r = np.zeros_like(k)
    for _ in range(D):
        r = (r << 2) | (k & 3)
        k >>= 2
    return r


def twiddles(M: int):
    """(cos, sin)(2 pi t / M), t < 3M/4: float64, rounded once"""
    a = 2.0 * np.pi * np.arange(3 * M // 4, dtype=F64) / float(M)
    return np.cos(a).astype(F32), np.sin(a).astype(F32)


# ---- the float32 clip before the level: mix_oracle.mix_clip's first half
def mix_y(arena: np.ndarray, it, N: int) -> np.ndarray:
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
        x[start:start + fg_len] = b[start:start + fg_len] + f * s
    else:
        x[:fg_len] = f
    y = x * F32(it["gain"])
    assert y.dtype == F32
    return y


def tail(w: np.ndarray, it) -> np.ndarray:
    """float32, as mix_oracle.mix_clip ends"""
    assert w.dtype == F32
    if int(it["flags"]) & 1:
        pk = F32(np.abs(w).max())
        if pk < F32(1e-8):
            pk = F32(1.0)
        r = F32(it["level"]) / pk
    else:
        r = F32(it["level"])
    z = w * r
    assert z.dtype == F32 and isinstance(r, np.float32)
    return (np.clip(z, F32(-1.0), F32(1.0)) * F32(32767)).astype(np.int16)


def tail64(w: np.ndarray, it) -> np.ndarray:
    w = w.astype(F64)
    r = float(it["level"])
    if int(it["flags"]) & 1:
        pk = float(np.abs(w).max())
        r = r / (pk if pk >= 1e-8 else 1.0)
    return np.trunc(np.clip(w * r, -1.0, 1.0) * 32767.0).astype(np.int16)


# ---- (i) the definition
def w64(y: np.ndarray, h: np.ndarray) -> np.ndarray:
    N = y.size
    return np.convolve(y.astype(F64), h.astype(F64)[:N])[:N]


def definition(arena, items, ir_ids, irs, N: int) -> np.ndarray:
    out = np.empty((len(items), N), np.int16)
    for i, it in enumerate(items):
        y = mix_y(arena, it, N)
        out[i] = tail64(w64(y, irs[int(ir_ids[i])]), it) if int(ir_ids[i]) >= 0 else tail(y, it)
    return out


# ---- (ii) the network of rir_plan.h in float32
def _mul(ar, ai, wr, wi):
    p0, p1, p2, p3 = ar * wr, ai * wi, ar * wi, ai * wr
    return p0 - p1, p2 + p3


def _mulc(ar, ai, wr, wi):
    p0, p1, p2, p3 = ar * wr, ai * wi, ar * wi, ai * wr
    return p0 + p1, p3 - p2


def _stage_views(zr, zi, s):
    H = zr.size
    return zr.reshape(H // (4 * s), 4, s), zi.reshape(H // (4 * s), 4, s)


def forward(zr, zi, M, T):
    H = M // 2
    s = H // 4
    while s >= 1:
        vr, vi = _stage_views(zr, zi, s)
        j = np.arange(s) * (M // (4 * s))
        a = [(vr[:, m, :].copy(), vi[:, m, :].copy()) for m in range(4)]
        b0 = (a[0][0] + a[2][0], a[0][1] + a[2][1]); b1 = (a[0][0] - a[2][0], a[0][1] - a[2][1])
        b2 = (a[1][0] + a[3][0], a[1][1] + a[3][1]); b3 = (a[1][0] - a[3][0], a[1][1] - a[3][1])
        ib3 = (-b3[1], b3[0])
        vr[:, 0, :], vi[:, 0, :] = b0[0] + b2[0], b0[1] + b2[1]
        vr[:, 1, :], vi[:, 1, :] = _mulc(b1[0] - ib3[0], b1[1] - ib3[1], T[0][j], T[1][j])
        vr[:, 2, :], vi[:, 2, :] = _mulc(b0[0] - b2[0], b0[1] - b2[1], T[0][2 * j], T[1][2 * j])
        vr[:, 3, :], vi[:, 3, :] = _mulc(b1[0] + ib3[0], b1[1] + ib3[1], T[0][3 * j], T[1][3 * j])
        s //= 4


def inverse(zr, zi, M, T):
    H = M // 2
    s = 1
    while s <= H // 4:
        vr, vi = _stage_views(zr, zi, s)
        j = np.arange(s) * (M // (4 * s))
        a0 = (vr[:, 0, :].copy(), vi[:, 0, :].copy())
        a1 = _mul(vr[:, 1, :], vi[:, 1, :], T[0][j], T[1][j])
        a2 = _mul(vr[:, 2, :], vi[:, 2, :], T[0][2 * j], T[1][2 * j])
        a3 = _mul(vr[:, 3, :], vi[:, 3, :], T[0][3 * j], T[1][3 * j])
        b0 = (a0[0] + a2[0], a0[1] + a2[1]); b1 = (a0[0] - a2[0], a0[1] - a2[1])
        b2 = (a1[0] + a3[0], a1[1] + a3[1]); b3 = (a1[0] - a3[0], a1[1] - a3[1])
        ib3 = (-b3[1], b3[0])
        vr[:, 0, :], vi[:, 0, :] = b0[0] + b2[0], b0[1] + b2[1]
        vr[:, 1, :], vi[:, 1, :] = b1[0] + ib3[0], b1[1] + ib3[1]
        vr[:, 2, :], vi[:, 2, :] = b0[0] - b2[0], b0[1] - b2[1]
        vr[:, 3, :], vi[:, 3, :] = b1[0] - ib3[0], b1[1] - ib3[1]
        s *= 4


def pair_tasks(M):
    """(pk, pm, k) of the pair stage: positions whose bin lies in (0, H/2), their partners at H - k, and last the self-paired H/2"""
    H, D = M // 2, digits(M)
    u = np.arange(1, H // 2)
    pk = ((u >> 1) << 2) | (u & 1)
    k = rev(pk, D)
    pk, k = np.append(pk, 2), np.append(k, H // 2)
    assert k[:-1].min() >= 1 and k[:-1].max() < H // 2 and rev(H // 2, D) == 2
    return pk, rev(H - k, D), k


def _split(zkr, zki, zmr, zmi, wr, wi):
    ar, ai = zkr + zmr, zki - zmi                       # zk + conj(zm)
    br, bi = zkr - zmr, zki - (-zmi)                    # zk - conj(zm)
    tr, ti = _mulc(br, bi, wr, wi)
    dr, di = ti, -tr
    return (ar + dr, ai + di), (ar - dr, -(ai - di))


def _pack(M):
    H = M // 2
    return F32(1.0) / F32(8 * H)


def prepare(h: np.ndarray, N: int, M: int, T=None):
    """a response's spectrum (re, im) [M/2] as nww_rir_prepare_dev writes it"""
    T = T or twiddles(M)
    n = min(h.size, N)
    y = np.zeros(M, F32)
    y[:n] = h[:n].astype(F32)
    zr, zi = y[0::2].copy(), y[1::2].copy()
    forward(zr, zi, M, T)
    pk, pm, k = pair_tasks(M)
    sc = _pack(M)
    (xkr, xki), (xmr, xmi) = _split(zr[pk], zi[pk], zr[pm], zi[pm], T[0][k], T[1][k])
    sr, si = np.zeros(M // 2, F32), np.zeros(M // 2, F32)
    sr[pm], si[pm] = xmr * sc, xmi * sc
    sr[pk], si[pk] = xkr * sc, xki * sc
    s0, d0 = zr[0] + zi[0], zr[0] - zi[0]
    sr[0], si[0] = (s0 + s0) * sc, (d0 + d0) * sc
    assert sr.dtype == F32 and isinstance(s0, np.float32)
    return sr, si


def convolve(y: np.ndarray, spec, M: int, T=None) -> np.ndarray:
    """y [N] float32 -> w [N] float32 through the network, against a prepared spectrum"""
    T = T or twiddles(M)
    N = y.size
    buf = np.zeros(M, F32)
    buf[:N] = y
    zr, zi = buf[0::2].copy(), buf[1::2].copy()
    forward(zr, zi, M, T)
    pk, pm, k = pair_tasks(M)
    sr, si = spec
    wr, wi = T[0][k], T[1][k]
    z0r, z0i = zr[0], zi[0]
    (xkr, xki), (xmr, xmi) = _split(zr[pk], zi[pk], zr[pm], zi[pm], wr, wi)
    ykr, yki = _mul(xkr, xki, sr[pk], si[pk])
    ymr, ymi = _mul(xmr, xmi, sr[pm], si[pm])
    ar, ai = ykr + ymr, yki - ymi
    br, bi = ykr - ymr, yki - (-ymi)
    orr, oi = _mul(br, bi, wr, wi)
    zr[pm], zi[pm] = ar + oi, orr - ai
    zr[pk], zi[pk] = ar - oi, ai + orr
    s0, d0 = z0r + z0i, z0r - z0i
    y0, yh = (s0 + s0) * sr[0], (d0 + d0) * si[0]
    zr[0], zi[0] = y0 + yh, y0 - yh
    inverse(zr, zi, M, T)
    assert zr.dtype == F32
    w = np.empty(M, F32)
    w[0::2], w[1::2] = zr, zi
    return w[:N]


def mix_rir(arena, items, ir_ids, irs, N: int, M: int, specs=None) -> np.ndarray:
    T = twiddles(M)
    specs = {} if specs is None else specs
    out = np.empty((len(items), N), np.int16)
    for i, it in enumerate(items):
        w = mix_y(arena, it, N)
        k = int(ir_ids[i])
        if k >= 0:
            if k not in specs:
                specs[k] = prepare(irs[k], N, M, T)
            w = convolve(w, specs[k], M, T)
        out[i] = tail(w, it)
    return out


def rir_items(ir_ids) -> np.ndarray:
    t = np.zeros(len(ir_ids), RIR_ITEM)
    t["ir_id"] = ir_ids
    return t


def bad_rir_items(n_irs: int):
    """[(item, field)]"""
    out = []
    for ir_id, reserved, field in [(-2, 0, "ir_id"), (n_irs, 0, "ir_id"), (2 ** 31 - 1, 0, "ir_id"), (0, 1, "reserved"), (-1, 7, "reserved")]:
        t = np.zeros(1, RIR_ITEM)
        t[0] = (ir_id, reserved)
        out.append((t[0], field))
    return out


# ---- inputs
def decaying(rng, L: int, amp: float = 1.0) -> np.ndarray:
    """a Gaussian response under an exponential decay (to e^-5 over its length)"""
    return (rng.standard_normal(L) * np.exp(-5.0 * np.arange(L) / max(L, 1)) * amp).astype(F32)


def edge_cases(M: int, seed: int = 9):
    """[(name, N, irs, arena, items, ir_ids)] for transform size M: the clip lengths and responses at which this instance can go wrong.
    N + min(L, N) - 1 == M exactly and one sample less; the first need that selects this M; L = 1 (a scaled delta) and a delta at tap
    L - 1; L > N with large taps beyond N (ignored); a response whose energy sits in its last tap; N odd and N = 1.  Items are rows of
    mix_oracle.edge_table(N) - its first rows (fg_len = 1, the 7-sample background) and its special last rows - and every table mixes
    ir_id = -1 with ids >= 0."""
    rng = np.random.default_rng(seed + M)
    prev = {2048: 0, 8192: 2048, 32768: 8192}[M]
    cases = []

    def add(name, N, irs):
        arena, items = mix_oracle.edge_table(N)
        pick = np.r_[0:min(4, len(items)), max(len(items) - 5, 0):len(items)]
        t = items[np.unique(pick)].copy()
        ids = np.arange(len(t)) % (len(irs) + 1) - 1                    # -1, 0, 1, .. in turn
        ids[-1] = len(irs) - 1
        for h in irs:
            assert fft_size(N, h.size) != 0 and fft_size(N, h.size) <= M
        cases.append((name, N, [np.ascontiguousarray(h, F32) for h in irs], arena, t, ids.astype(np.int32)))

    Na = M // 2 + 8
    delta_last = np.zeros(33, F32); delta_last[-1] = 0.75
    heavy_last = decaying(rng, 100, 0.01); heavy_last[-1] = 1.5
    add("exact", Na, [decaying(rng, M // 2 - 7), decaying(rng, M // 2 - 8), np.array([0.5], F32), delta_last, heavy_last])
    assert fft_size(Na, M // 2 - 7) == M and Na + (M // 2 - 7) - 1 == M
    No = M // 4 + 1                                                     # odd: the packing's last pair is half empty
    long_ = decaying(rng, 2 * No); long_[No:] = -30.0
    add("odd", No, [decaying(rng, No // 2), long_, np.array([-2.0], F32)])
    if prev:
        Nf = prev // 2 + 80
        add("first", Nf, [decaying(rng, prev + 2 - Nf)])
        assert fft_size(Nf, prev + 2 - Nf) == M and fft_size(Nf, prev + 1 - Nf) == prev
    add("one", 1, [np.array([0.25], F32), np.array([2.0, 9.0, 9.0], F32)])
    return cases


def accuracy_inputs(N: int = 16000, seed: int = 3):
    """Gaussian clips under a slow envelope (int16, no background) against exponentially decaying Gaussian responses of 800 / 4000 /
    16 000 taps: (arena, items, irs)"""
    rng = np.random.default_rng(seed)
    clips = []
    for k in range(3):
        env = 0.35 + 0.3 * np.sin(2 * np.pi * (np.arange(N) / N * (1.5 + k) + 0.1 * k))
        clips.append(np.clip(np.rint(rng.standard_normal(N) * env * 9000.0), -32768, 32767).astype(np.int16))
    arena = np.concatenate(clips)
    items = np.concatenate([mix_oracle.item(k * N, N, gain=1.0 + 0.1 * k, level=0.9 - 0.1 * k) for k in range(3)])
    irs = [decaying(rng, L) for L in (800, 4000, 16000)]
    return arena, items, irs


# ---- tests/golden/rir.npz (tools/make_rir_goldens.py)
GOLDEN_IR_LEN = (1, 301, 1600, 4000, 8000, 12001, 16000, 20000)


def golden_irs():
    """the golden's eight responses from integer arithmetic alone (mix_oracle's hash), under an integer-built decay: the same on any numpy"""
    out = []
    for key, L in enumerate(GOLDEN_IR_LEN):
        g = mix_oracle.golden_clip(L, 100 + key, 32767).astype(np.int64)
        t = np.arange(L, dtype=np.int64)
        dec = (4096 * (L - t) // L) ** 2                                 # quadratic decay, 2^24 .. 0
        out.append(((g * dec) // 4096).astype(F32) / F32(2.0 ** 27))
    return out


def load_golden():
    """(arena, items, ir_ids, irs, ref, meta)"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rir.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    arena, _, _ = mix_oracle.golden_arena()
    irs = golden_irs()
    assert arena.size == meta["arena_samples"] and int(arena.astype(np.int64).sum()) == meta["arena_sum"]
    assert [float(np.abs(h.astype(F64)).sum()) for h in irs] == meta["ir_abs_sums"]
    return arena, z["items"], z["ir_ids"], irs, z["ref"], meta


def conditions(out: np.ndarray, ref: np.ndarray, what: str = "") -> float:
    """per clip: no sample off by more than 1 LSB, and at most 0.5 % of the clip's samples off at all -> the largest share"""
    worst = 0.0
    for i in range(len(out)):
        d = np.abs(out[i].astype(np.int32) - ref[i].astype(np.int32))
        share = float((d > 0).mean())
        print(f"{what} clip {i}: max |d| = {int(d.max())} LSB, differing {int((d > 0).sum())} of {d.size} ({100 * share:.4f} %)")
        assert int(d.max()) <= 1, (what, i, int(d.max()))
        assert share <= 0.005, (what, i, share)
        worst = max(worst, share)
    return worst
