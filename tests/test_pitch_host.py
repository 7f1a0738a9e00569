"""Clips shifted in pitch (nww_pitch_set_ratios / nww_mix_aug_*), on the CPU: the declarations of include/nww.h; csrc/pitch_plan.h - the
tables, the validation and the walk of a whole clip - through tests/hostemu/pitch_check.cpp, a stand-alone g++ program built with
-ffp-contract=off -fsanitize=address,undefined, against the float32 restatement of tests/pitch_oracle.py bit for bit; the restatement
against the float64 definition with the same definition in float32 torch ops as the yardstick; the properties of a pitch shift; the
definition's golden (tests/golden/pitch.npz); and augment.py's host side.

Restatement against definition, on the 36 items of tests/golden/mix.npz that have a background (N = 16000, pitch_oracle.RATIOS in turn):
the restatement's max-abs error is 0.0001 .. 0.035 of the yardstick's and its rms error 0.0001 .. 0.044 (the bound is 2): the unit-vector
recurrence adds a rounding of 2^-24 per frame to a bin's phase where the float32 angle route adds one of 2^-24 times the phase itself,
which grows with the bin's frequency and the frame.  After the int16 tail 0 .. 9.2 % of a clip's samples differ from the definition's
(median 0.2 %), by 1 LSB except one clip's 3 (its first: a quiet foreground in a loud background normalised up)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mix_oracle
import pitch_oracle
import rir_oracle
from conftest import ROOT

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")
AUG = ["nww_pitch_set_ratios", "nww_mix_aug_dev", "nww_mix_aug", "nww_mix_aug_forward_pcm_dev", "nww_mix_aug_frontend_dev"]
RATIOS = pitch_oracle.RATIOS


def test_declarations_and_item_layout():
    from nanowakeword_amd import _lib, augment
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    for sym in AUG:
        assert re.search(rf"^extern int {sym}\(", hdr, re.M), sym
        assert sym in _lib.SYMBOLS
    assert len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    assert "typedef struct nww_pitch_item { int32_t pitch_id; uint32_t reserved; } nww_pitch_item;" in hdr
    for dt in (augment.PITCH_ITEM, pitch_oracle.PITCH_ITEM):
        assert dt.names == ("pitch_id", "reserved") and [dt[n].str for n in dt.names] == ["<i4", "<u4"] and dt.itemsize == 8
    # the aug calls are the rir calls plus one table: the declared argument lists say so
    src = open(os.path.join(ROOT, "nanowakeword_amd", "_lib.py")).read()
    for form in ("_dev", "", "_forward_pcm_dev", "_frontend_dev"):
        rir = re.search(rf"lib\.nww_mix_rir{form}\.argtypes = \[(.*?)\]", src).group(1).split(", ")
        aug = re.search(rf"lib\.nww_mix_aug{form}\.argtypes = \[(.*?)\]", src).group(1).split(", ")
        assert aug == rir[:8] + ["vp"] + rir[8:], form
        decl = re.search(rf"^extern int nww_mix_aug{form}\((.*?)\);", hdr, re.M | re.S).group(1)
        assert decl.count(",") + 1 == len(aug) and "const nww_pitch_item* pitch_items, int32_t B, int32_t N" in " ".join(decl.split())
    # the existing items are as they were
    assert augment.MIX_ITEM == mix_oracle.MIX_ITEM and augment.MIX_ITEM.itemsize == 48 and augment.RIR_ITEM.itemsize == 8


@pytest.fixture(scope="module")
def pitch_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pitch_check") / "pitch_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostemu", "pitch_check.cpp")], check=True)

    def run(tables, tmp_path):
        """[(arena, items, pitch_items, ratios, N)] -> [dict(bad, bad_pitch, bad_ratio, length_ok, clips, y)]"""
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<q", len(tables)))
            for arena, items, pt, ratios, N in tables:
                assert len(pt) == len(items) and pt.dtype == pitch_oracle.PITCH_ITEM
                f.write(struct.pack("<qqqq", arena.size, len(items), N, len(ratios)))
                f.write(np.ascontiguousarray(arena, np.int16).tobytes())
                f.write(np.ascontiguousarray(items).tobytes())
                f.write(np.ascontiguousarray(pt).tobytes())
                f.write(np.array([r[0] for r in ratios], np.int32).tobytes())
                f.write(np.array([r[1] for r in ratios], np.int32).tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(dst, "rb").read()
        out, at = [], 0
        for arena, items, pt, ratios, N in tables:
            res = {}
            for key in ("bad", "bad_pitch"):
                idx, = struct.unpack_from("<q", raw, at)
                res[key] = (idx, raw[at + 8:at + 24].split(b"\0")[0].decode())
                at += 24
            res["bad_ratio"], res["length_ok"] = struct.unpack_from("<qq", raw, at)
            at += 16
            res["clips"] = res["y"] = None
            if res["bad"][0] < 0 and res["bad_pitch"][0] < 0 and res["bad_ratio"] < 0 and res["length_ok"]:
                n = len(items) * N
                res["clips"] = np.frombuffer(raw, np.int16, n, at).reshape(len(items), N)
                at += 2 * n
                res["y"] = np.frombuffer(raw, np.float32, n, at).reshape(len(items), N)
                at += 4 * n
            out.append(res)
        assert at == len(raw)
        return out
    run.exe = exe
    return run


def test_tables_are_numpys(pitch_check, tmp_path):
    """twiddles, window, envelope and taps: float64, rounded once.  A failure here means this platform's libm and numpy disagree on a
    float64 cos / sin by enough to move a float32 rounding - the bit-for-bit tests below would then fail for that reason and no other."""
    dst = str(tmp_path / "tb.bin")
    subprocess.run([pitch_check.exe, "--tables", dst], check=True)
    raw = np.fromfile(dst, np.float32)
    tb = pitch_oracle.tables()
    assert raw.size == 768 + 512 + 2048
    T = raw[:768].reshape(-1, 2)
    assert np.array_equal(T[:, 0], tb["T"][0]) and np.array_equal(T[:, 1], tb["T"][1])
    assert np.array_equal(raw[768:1280], tb["win"]) and np.array_equal(raw[1280:], tb["env"].ravel())
    assert tb["win"][0] == 0.0 and tb["win"][256] == 1.0 and abs(float(tb["env"][15].min()) - 1.5) < 1e-6 and abs(float(tb["env"][15].max()) - 1.5) < 1e-6
    for p, q in RATIOS + pitch_oracle.GOOD_RATIOS_AT_THE_BOUNDS:
        subprocess.run([pitch_check.exe, "--taps", str(p), str(q), dst], check=True)
        g = np.fromfile(dst, np.float32).reshape(q, pitch_oracle.TAPS)
        assert np.array_equal(g, pitch_oracle.resample_table(p, q)), (p, q)
        # the window of six zero crossings a side fits the sixteen taps: the outermost ones are zero somewhere, and a phase sums to ~1
        # (0.99 of the band kept)
        c = 0.99 * min(1.0, q / p)
        assert 6.0 / c < 8.0 and np.abs(g.sum(axis=1) - 1.0).max() < 2e-3, (p, q)


@pytest.mark.parametrize("N", [257, 384, 2000, 4000, 16000])
def test_walk_on_cpu_equals_restatement(pitch_check, tmp_path, N):
    """pitch_clip_host under the sanitizers against pitch_oracle: the same bits, before the tail and after; rows without a ratio are
    mix_oracle's.  The clips and ratios are those of the GPU test at every N (two clips and one row without a ratio at 16000)."""
    arena, items = pitch_oracle.clip_table(N)
    if N == 16000:
        items, ids = items[[0, 3, 4]].copy(), np.array([0, 5, -1], np.int32)
    else:
        items = mix_oracle.table_of(items, 8)
        ids = np.array([0, 1, 2, 3, 4, 5, -1, 1], np.int32)
    res, = pitch_check([(arena, items, pitch_oracle.pitch_items(ids), RATIOS, N)], tmp_path)
    assert res["clips"] is not None, res
    for i in range(len(items)):
        y = pitch_oracle.mix_aug_y(arena, items[i], ids[i], RATIOS, N)
        assert np.array_equal(y.view(np.uint32), res["y"][i].view(np.uint32)), (N, i, np.abs(y - res["y"][i]).max())
    want = pitch_oracle.mix_aug(arena, items, ids, RATIOS, N)
    assert np.array_equal(res["clips"], want)
    assert np.array_equal(res["clips"][ids < 0], mix_oracle.mix(arena, items[ids < 0], N))


def test_restatement_against_definition_with_the_float32_route_as_yardstick():
    """every item of mix.npz that has a background: the restatement's max-abs and rms error against the float64 definition is at most
    twice that of the same definition in float32 torch ops; after the int16 tail the share of differing samples and the largest
    difference are printed, and are what the golden's metadata recorded"""
    arena, items, N, ratios = pitch_oracle.accuracy_clips()
    assert len(items) == 36
    rows = pitch_oracle.accuracy(arena, items, N, ratios)
    for i, (rmax, rrms, share, dmax) in enumerate(rows):
        print(f"clip {i} at {ratios[i][0]}/{ratios[i][1]}: max-abs ratio {rmax:.4f}, rms ratio {rrms:.4f}, int16 differing {100 * share:.3f} %, max {dmax} LSB")
    for i, (rmax, rrms, share, dmax) in enumerate(rows):
        assert rmax <= 2.0 and rrms <= 2.0, (i, rmax, rrms)
    meta = pitch_oracle.load_golden()[5]
    assert len(meta["accuracy_max_abs_ratio"]) == 36 and max(meta["accuracy_max_abs_ratio"]) <= 2.0 and max(meta["accuracy_rms_ratio"]) <= 2.0


def _peak_hz(y):
    spec = np.abs(np.fft.rfft(y.astype(np.float64) * np.hanning(y.size)))
    return float(np.argmax(spec)) * 16000.0 / y.size


def test_a_sine_moves_by_the_ratio_and_silence_stays_silent():
    N = 16000
    w = (0.5 * np.sin(2.0 * np.pi * 1000.0 * np.arange(N) / 16000.0)).astype(np.float32)
    for (p, q), hz in (((9, 8), 1125.0), ((8, 9), 889.0)):
        for y in (pitch_oracle.shift(w, p, q), pitch_oracle.definition_y(w, p, q)):
            assert abs(_peak_hz(y) - hz) <= 31.25, (p, q, _peak_hz(y))
            assert np.isfinite(y).all() and 0.25 < float(np.abs(y).max()) < 1.0      # a tone: bins off it hold rounding noise, no more is asked
    z = np.zeros(4000, np.float32)
    for p, q in RATIOS:
        y = pitch_oracle.shift(z, p, q)
        assert y.dtype == np.float32 and not y.any() and np.isfinite(y).all()                   # unit(0) = (1, 0), times |X| = 0


def test_rate_one_returns_the_input_frames(pitch_check, tmp_path):
    """p = q, which only the walk can be asked for: u_t telescopes to unit(X_t), so the vocoder's frames are its input's within
    rounding - a few ulps of the frame's largest bin per frame passed - and the stretched signal is the clip"""
    N = 4000
    arena, items = pitch_oracle.clip_table(N)
    w = rir_oracle.mix_y(arena, items[0], N)
    for p in (1, 7):
        src, dst = str(tmp_path / "s.bin"), str(tmp_path / "o.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<qqq", N, p, p))
            f.write(w.tobytes())
        subprocess.run([pitch_check.exe, "--spec", src, dst], check=True)
        raw = np.fromfile(dst, np.float32)
        T = pitch_oracle.frames(N)
        X = raw[:(T + 1) * 512].reshape(T + 1, 256, 2)
        Y = raw[(T + 1) * 512:(2 * T + 1) * 512].reshape(T, 256, 2)
        s = raw[(2 * T + 1) * 512:]
        assert s.size == 128 * (T - 1)
        Xr, Xi = pitch_oracle.stft(w)
        assert np.array_equal(X[..., 0], Xr) and np.array_equal(X[..., 1], Xi)
        scale = np.abs(X[:T, 1:]).max()
        err = np.abs(Y[:, 1:] - X[:T, 1:]).max(axis=(1, 2))
        assert (err <= 2.0 ** -23 * scale * (4 + 2 * np.arange(T))).all(), (err / scale).max()
        assert np.abs(np.abs(Y[:, 0]) - np.abs(X[:T, 0])).max() <= 2.0 ** -22 * scale          # the two real bins
        n = min(s.size, N)
        assert np.abs(s[:n] - w[:n]).max() <= 1e-4 * np.abs(w).max()
        # the restatement takes the same route
        Yr, Yi = pitch_oracle.vocoder(Xr, Xi, p, p)
        assert np.array_equal(Y[..., 0], Yr) and np.array_equal(Y[..., 1], Yi)
        assert np.array_equal(s, pitch_oracle.istft(Yr, Yi))


def test_definition_and_restatement_against_the_golden(pitch_check, tmp_path):
    arena, items, ids, ratios, ref, meta = pitch_oracle.load_golden()
    N = meta["N"]
    assert N == 4000 and ratios == [(9, 8), (15, 16), (128, 125)] and ids.tolist() == [0, 1, 2, -1] and ref.shape == (4, N) and ref.dtype == np.int16
    assert np.array_equal(items, pitch_oracle.golden_items())
    now = pitch_oracle.definition(arena, items, ids, ratios, N)
    d = np.abs(now.astype(np.int32) - ref.astype(np.int32))
    print("definition today against the golden: differing", (d > 0).sum(axis=1), "max", int(d.max()))
    assert int(d.max()) <= 1 and (d > 0).mean() <= 1e-3                     # float64 throughout: another torch may flip a truncation
    res, = pitch_check([(arena, items, pitch_oracle.pitch_items(ids), ratios, N)], tmp_path)
    ours = pitch_oracle.mix_aug(arena, items, ids, ratios, N)
    assert np.array_equal(res["clips"], ours)
    d = np.abs(ours.astype(np.int32) - ref.astype(np.int32))
    assert [int(x) for x in (d > 0).sum(axis=1)] == meta["restatement_differing_per_clip"] and int(d.max()) == meta["restatement_max_abs_diff"] <= 1
    assert np.array_equal(ours[3], ref[3])
    # the allowance is not what lets a wrong ratio through: 9/8 against 8/9 moves nearly every sample
    wrong = pitch_oracle.definition(arena, items[:1], ids[:1], [(8, 9)], N)
    assert (wrong != ref[:1]).mean() > 0.5


def test_refusals(pitch_check, tmp_path):
    N = 2000
    arena, items = pitch_oracle.clip_table(N)
    ids = np.array([0, 1, -1, 2, 3, 5, 4], np.int32)
    assert len(items) == len(ids)
    good = pitch_oracle.pitch_items(ids)
    tables, expect = [], []
    for k, (bad, field) in enumerate(pitch_oracle.bad_pitch_items(len(RATIOS))):
        t = good.copy()
        t[(2 * k) % len(t)] = bad
        tables.append((arena, items, t, RATIOS, N)); expect.append(("bad_pitch", ((2 * k) % len(t), field)))
    t = good.copy(); t[4] = pitch_oracle.bad_pitch_items(len(RATIOS))[0][0]; t[1] = pitch_oracle.bad_pitch_items(len(RATIOS))[3][0]
    tables.append((arena, items, t, RATIOS, N)); expect.append(("bad_pitch", (1, "reserved")))              # the first is reported
    tables.append((arena, items, good, [], N)); expect.append(("bad_pitch", (0, "pitch_id")))               # no ratios: no id is valid
    bad_mix = items.copy(); bad_mix[3] = mix_oracle.bad_items(arena.size, N)[0][0]
    tables.append((arena, bad_mix, good, RATIOS, N)); expect.append(("bad", (3, "fg_len")))
    for r in pitch_oracle.BAD_RATIOS:
        tables.append((arena, items, good, RATIOS[:5] + [r], N)); expect.append(("bad_ratio", 5))
    tables.append((arena, items, good, RATIOS + [(9, 8)] * 59, N)); expect.append(("bad_ratio", 65))        # K <= 64
    tables.append((arena, items, good, RATIOS + [(9, 8)] * 57 + [(27, 34)], N)); expect.append(("bad_ratio", -1))
    tables.append((arena, items, good, RATIOS + pitch_oracle.GOOD_RATIOS_AT_THE_BOUNDS, N)); expect.append(("bad_ratio", -1))
    a256, i256 = pitch_oracle.clip_table(256)
    tables.append((a256, i256, pitch_oracle.pitch_items(np.full(len(i256), -1)), RATIOS, 256)); expect.append(("length_ok", 0))
    a257, i257 = pitch_oracle.clip_table(257)
    tables.append((a257, i257, pitch_oracle.pitch_items(np.zeros(len(i257), np.int32)), RATIOS, 257)); expect.append(("length_ok", 1))
    for (key, want), res in zip(expect, pitch_check(tables, tmp_path)):
        assert res[key] == want, (key, want, res[key])
        assert (res["clips"] is not None) == (want in (-1, 1))


def test_pitch_ratios_bank_and_draws():
    from nanowakeword_amd.augment import (PITCH_ITEM, MixedClips, PitchBank, as_pitch_items, draw_pitch_ids, mixed_feature_batches, pitch_ratio_ok,
                                          pitch_ratios)
    r = pitch_ratios()
    assert r == pitch_oracle.reduced_ratios() and (1, 1) not in r and len(r) == 72
    lo, hi = 2.0 ** (-2 / 12), 2.0 ** (2 / 12)
    assert all(lo <= p / q <= hi and np.gcd(p, q) == 1 and q <= 32 and pitch_ratio_ok(p, q) for p, q in r)
    assert [p / q for p, q in r] == sorted(p / q for p, q in r) and len(set(r)) == len(r)
    assert len(pitch_ratios(max_den=30)) == 62 and len(pitch_ratios(max_den=31)) == 68            # INTEGRATION.md's example fits a bank of 64
    assert pitch_ratios(max_den=8) == [] and pitch_ratios(max_den=10) == [(9, 10), (11, 10), (10, 9)]      # 8/9 and 9/8 lie just outside +-2
    assert pitch_ratios(-4, 4, 6) == pitch_oracle.reduced_ratios(-4, 4, 6) == [(4, 5), (5, 6), (7, 6), (6, 5), (5, 4)]
    assert (4, 5) in pitch_ratios(-4, 4, 5) and (5, 4) in pitch_ratios(-4, 4, 4) and (4, 3) not in pitch_ratios(-6, 6, 4)
    for p, q in pitch_oracle.BAD_RATIOS:
        assert not pitch_ratio_ok(p, q) and not pitch_oracle.ratio_ok(p, q), (p, q)
        with pytest.raises(ValueError, match="ratio 1"):
            PitchBank([(9, 8), (p, q)])
    for p, q in pitch_oracle.GOOD_RATIOS_AT_THE_BOUNDS + RATIOS:
        assert pitch_ratio_ok(p, q) and pitch_oracle.ratio_ok(p, q)
    b = PitchBank(r[:64])
    assert len(b) == b.n == 64 and b.num.dtype == np.int32 and b.den.dtype == np.int32 and list(zip(b.num.tolist(), b.den.tolist())) == r[:64]
    for bad in ([], r[:65]):
        with pytest.raises(ValueError, match="between 1 and 64"):
            PitchBank(bad)

    class Model:
        calls = 0

        def pitch_set_ratios(self, num, den):
            self.calls += 1
    m = Model()
    assert b.prepare(m) is b and b.prepare(m) is b and m.calls == 1                              # once per model
    PitchBank(RATIOS).prepare(m)
    assert b.prepare(m) is b and m.calls == 3                                                    # a model holds one bank at a time
    ids = draw_pitch_ids(np.random.default_rng(2), 64, 4000)
    assert ids.dtype == np.int32 and ids.shape == (4000,) and ids.min() == -1 and ids.max() == 63
    assert np.array_equal(ids, draw_pitch_ids(np.random.default_rng(2), 64, 4000))
    assert 0.46 < (ids >= 0).mean() < 0.54 and len(np.unique(ids)) == 65                         # p = 0.5 (augment_clips.py:150-157)
    assert (draw_pitch_ids(np.random.default_rng(2), 3, 50, 1.0) >= 0).all() and (draw_pitch_ids(np.random.default_rng(2), 3, 50, 0.0) == -1).all()
    assert (draw_pitch_ids(np.random.default_rng(2), 0, 7) == -1).all()
    t = as_pitch_items(ids[:9], 9)
    assert t.dtype == PITCH_ITEM and np.array_equal(t["pitch_id"], ids[:9]) and (t["reserved"] == 0).all() and as_pitch_items(t, 9) is not None
    for bad in (ids[:8], np.zeros(9, np.float32), np.zeros((3, 3), np.int32)):
        with pytest.raises(ValueError):
            as_pitch_items(bad, 9)
    # the batches carry the ids, behind the response ids where there are both
    items = np.concatenate([mix_oracle.item(k, 5) for k in range(7)])
    pid, rid = np.arange(7) % 3 - 1, np.arange(7) - 1
    got = list(mixed_feature_batches(items, 3, pitch=b, pitch_ids=pid))
    assert [len(x[0]) for x in got] == [3, 3, 1] and np.array_equal(np.concatenate([x[1]["pitch_id"] for x in got]), pid)
    got = list(mixed_feature_batches(items, 3, irs=object(), ir_ids=rid, pitch=b, pitch_ids=pid))
    assert all(len(x) == 3 for x in got) and np.array_equal(np.concatenate([x[1]["ir_id"] for x in got]), rid)
    assert np.array_equal(np.concatenate([x[2]["pitch_id"] for x in got]), pid)
    assert all(np.array_equal(x, items[3 * i:3 * i + 3]) for i, x in enumerate(mixed_feature_batches(items, 3)))      # as before without
    with pytest.raises(ValueError):
        list(mixed_feature_batches(items, 3, pitch_ids=pid))

    class Feats:
        def embed_mixed(self, arena, items, N, **kw):
            return kw
    kw = MixedClips(Feats(), None, 5, irs="I", pitch=b).embed_clips(got[0])
    assert kw["irs"] == "I" and kw["pitch"] is b and np.array_equal(kw["ir_ids"]["ir_id"], rid[:3]) and np.array_equal(kw["pitch_ids"]["pitch_id"], pid[:3])
    kw = MixedClips(Feats(), None, 5, pitch=b).embed_clips((items[:3], as_pitch_items(pid[:3], 3)))
    assert kw["irs"] is None and kw["ir_ids"] is None and np.array_equal(kw["pitch_ids"]["pitch_id"], pid[:3])
