"""The segmented route of nww_mix_rir_* (M = NWW_RIR_SEGMENTED: clips and responses of any length) restated in numpy on top of
rir_oracle's float32 network - `prepare`, `convolve`, `mix_y` and `tail` are that module's, unchanged: uniformly partitioned overlap-save
on the 32768-point transform, independent of csrc/rir_plan.h's rir_seg_* walk.

  Le = min(L, N) taps count, P = ceil(Le / LP) partitions, Q = ceil(N / V) segments, V = LP = 16384, M = 32768.
  Partition p is taps [p LP, min((p + 1) LP, Le)), prepared as a response of a V-sample clip is.
  Segment q is ((c_0 + c_1) + c_2) + .. over p <= min(P - 1, q), c_p the upper half of the window y[(q - p - 1) V .. (q - p + 1) V)
  (zeros outside the clip) convolved with partition p; the peak runs over all N samples, then rir_oracle.tail.

Also the edge cases the CPU check (tests/hostemu/rir_seg_check.cpp) and the GPU tests share, and the loader of tests/golden/rir_seg.npz
(tools/make_rir_seg_goldens.py).  The float64 definition is rir_oracle.definition.  Checker only."""
import json
import os

import numpy as np

import mix_oracle
import rir_oracle
from mix_oracle import F32

SEGMENTED = -1
M = 32768
V = LP = 16384


def parts(N: int, L: int) -> int:
    return -(-min(L, N) // LP) if N >= 1 and L >= 1 else 0


def segments(N: int) -> int:
    return -(-N // V)


def spectra_floats(K: int, N: int, L: int, m: int) -> int:
    if K < 1 or N < 1 or L < 1:
        return 0
    if m == SEGMENTED:
        return ((K + 2 + 3) & ~3) + K * parts(N, L) * M
    return K * m if m in rir_oracle.SIZES else 0


def prepare(h: np.ndarray, N: int, T=None):
    """the spectra of a response's partitions: a list of P (re, im) pairs"""
    T = T or rir_oracle.twiddles(M)
    Le = min(h.size, N)
    return [rir_oracle.prepare(h[p * LP:min((p + 1) * LP, Le)], V, M, T) for p in range(parts(N, h.size))]


def convolve(y: np.ndarray, specs, T=None) -> np.ndarray:
    """y [N] float32 -> w [N] float32, segment by segment"""
    T = T or rir_oracle.twiddles(M)
    N = y.size
    Q = segments(N)
    pad = np.zeros((Q + 2) * V, F32)                                    # pad[V + i] = y[i]: zeros before and behind the clip
    pad[V:V + N] = y
    w = np.empty(Q * V, F32)
    for q in range(Q):
        acc = None
        for p in range(min(len(specs) - 1, q) + 1):
            lo = (q - p - 1) * V + V
            c = rir_oracle.convolve(pad[lo:lo + M], specs[p], M, T)[V:]
            acc = c if acc is None else acc + c
            assert acc.dtype == F32
        w[q * V:(q + 1) * V] = acc
    return w[:N]


def mix_rir(arena, items, ir_ids, irs, N: int, specs=None, with_w: bool = False):
    T = rir_oracle.twiddles(M)
    specs = {} if specs is None else specs
    out = np.empty((len(items), N), np.int16)
    ws = np.empty((len(items), N), F32)
    for i, it in enumerate(items):
        w = rir_oracle.mix_y(arena, it, N)
        k = int(ir_ids[i])
        if k >= 0:
            if k not in specs:
                specs[k] = prepare(irs[k], N, T)
            w = convolve(w, specs[k], T)
        ws[i] = w
        out[i] = rir_oracle.tail(w, it)
    return (out, ws) if with_w else out


# ---- inputs
def edge_cases_seg(seed: int = 21):
    """[(name, N, irs, arena, items, ir_ids)]: the clip lengths and responses at which the segmentation can go wrong.  N = 1; N = 16384
    (Q = 1) and 16385 (a last segment of one sample); N = 32768 and 32769 (Q = 2 and 3); N = 20000 with 12770 taps, the pair the
    one-workgroup route refuses; L = 1; L = 16384 and 16385 (a last partition of one tap); a delta at tap 16384 (a pure delay across the
    partition boundary - at N = 32768, where it moves half a clip: at N = 16385 its output would be ONE sample, whose float32 rounding
    alone exceeds a bound stated in the rms over the clip); L > N with loud taps beyond N (ignored); N = 40000 with 40000 taps (all
    six (q, p) pairs).  Items are rows of mix_oracle.edge_table(N) - first rows (fg_len = 1, the 7-sample background) and special last
    rows - and every table mixes ir_id = -1 with ids >= 0."""
    rng = np.random.default_rng(seed)
    dec = rir_oracle.decaying
    cases = []

    def add(name, N, irs, rows):
        arena, items = mix_oracle.edge_table(N)
        rows = [r % len(items) for r in rows]
        t = items[rows].copy()
        ids = np.arange(len(t)) % (len(irs) + 1) - 1                    # -1, 0, 1, .. in turn
        ids[-1] = len(irs) - 1
        assert (ids < 0).any() and set(range(len(irs))) <= set(ids.tolist())
        cases.append((name, N, [np.ascontiguousarray(h, F32) for h in irs], arena, t, ids.astype(np.int32)))

    delay = np.zeros(LP + 1, F32); delay[LP] = 0.5
    loud = dec(rng, 40000); loud[20000:] = -30.0
    add("one", 1, [np.array([0.25], F32), np.array([2.0, 9.0, 9.0], F32)], [0, 1, -1])
    add("q1", 16384, [dec(rng, 16384), np.array([-2.0], F32)], [0, 1, -11])
    add("q1+1", 16385, [dec(rng, 16385), dec(rng, 16384)], [0, 1, 2, -1])
    add("q2", 32768, [dec(rng, 20000), delay], [1, -3, -4])
    add("q3", 32769, [dec(rng, 16385)], [-1, 3])
    add("refused", 20000, [dec(rng, 12770), loud, np.array([0.5], F32)], [0, 1, 2, -2, -9])
    add("six", 40000, [dec(rng, 40000)], [1, -11])
    return cases


# ---- tests/golden/rir_seg.npz (tools/make_rir_seg_goldens.py)
GOLDEN_IRS = (4, 5, 6, 7)                                               # of rir_oracle.golden_irs(): 8000 / 12001 / 16000 / 20000 taps


def load_golden():
    """(arena, items, ir_ids, irs, ref, meta); ir_ids index the returned irs"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rir_seg.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    arena, _, _ = mix_oracle.golden_arena()
    irs = [rir_oracle.golden_irs()[k] for k in GOLDEN_IRS]
    assert arena.size == meta["arena_samples"] and int(arena.astype(np.int64).sum()) == meta["arena_sum"]
    assert [int(h.size) for h in irs] == meta["ir_lengths"] == [8000, 12001, 16000, 20000]
    assert [float(np.abs(h.astype(np.float64)).sum()) for h in irs] == meta["ir_abs_sums"]
    return arena, z["items"], z["ir_ids"], irs, z["ref"], meta
