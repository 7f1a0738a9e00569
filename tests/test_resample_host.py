"""Recordings brought to the target rate (nww_resample_*), on the CPU: the declarations of include/nww.h; csrc/resample_plan.h - the tap
tables, the validation and the walk of whole items, tile by tile - through tests/hostemu/resample_check.cpp, a stand-alone g++ program
built with -ffp-contract=off -fsanitize=address,undefined, against the float32 restatement of tests/resample_oracle.py bit for bit; the
restatement against the float64 definition after the int16 tail; the properties of the definition; its golden
(tests/golden/resample.npz); and augment.py's host side.

Restatement against definition on the golden's eight speech-like clips of half a second (48 k stereo, 44.1 k, 22.05 k, 8 k, 32 k stereo,
24 k, 11.025 k and 96 k to 16 k): 0.025 .. 0.075 % of the int16 samples differ, by 1 LSB, with a float32 error before the tail of at most
0.0040 LSB (the condition is 0.5 % and 1 LSB)."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import resample_oracle as ro
from conftest import ROOT

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")
SYMS = ["nww_resample_set_ratios", "nww_resample_length", "nww_resample_dev", "nww_resample"]
PAIRS = [(np.int16, np.int16), (np.int16, np.float32), (np.float32, np.int16), (np.float32, np.float32)]


def test_declarations_and_item_layout():
    from nanowakeword_amd import _lib, augment
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    for sym in SYMS:
        assert re.search(rf"^extern (int|int64_t) {sym}\(", hdr, re.M), sym
        assert sym in _lib.SYMBOLS
    assert len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    body = re.search(r"typedef struct nww_resample_item \{(.*?)\} nww_resample_item;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(int64_t|int32_t|uint32_t) (\w+);", body, re.M)
    assert fields == [("int64_t", "src_off"), ("int64_t", "dst_off"), ("int32_t", "src_frames"), ("int32_t", "channels"), ("int32_t", "rate_id"),
                      ("uint32_t", "reserved")]
    for dt in (augment.RESAMPLE_ITEM, ro.RESAMPLE_ITEM):
        assert dt.names == tuple(n for _, n in fields) and dt.itemsize == 32
        assert [dt[n].str for n in dt.names] == ["<i8", "<i8", "<i4", "<i4", "<i4", "<u4"] and [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 20, 24, 28]
    assert int(re.search(r"#define NWW_PCM_S16 (\d+)", hdr).group(1)) == augment.PCM_S16 == ro.S16 == 0
    assert int(re.search(r"#define NWW_PCM_F32 (\d+)", hdr).group(1)) == augment.PCM_F32 == ro.PCM_F32 == 1
    plan = open(os.path.join(CSRC, "resample_plan.h")).read()
    for name, val in (("RESAMPLE_TILE", augment.RESAMPLE_TILE), ("RESAMPLE_MAX_TERM", augment.RESAMPLE_MAX_TERM), ("RESAMPLE_MAX_RATIOS", augment.RESAMPLE_MAX_RATIOS),
                      ("RESAMPLE_MAX_CHANNELS", augment.RESAMPLE_MAX_CHANNELS)):
        assert int(re.search(rf"#define {name} (\d+)", plan).group(1)) == val, name
    assert augment.RESAMPLE_TILE == ro.TILE and augment.RESAMPLE_MAX_TERM == ro.MAX_TERM and augment.RESAMPLE_MAX_RATIOS == ro.MAX_RATIOS
    assert augment.RESAMPLE_MAX_FRAMES == ro.MAX_FRAMES == 1 << 30 and "#define RESAMPLE_MAX_FRAMES (1 << 30)" in plan
    src = open(os.path.join(ROOT, "nanowakeword_amd", "_lib.py")).read()
    for sym in SYMS:
        args = re.search(rf"lib\.{sym}\.argtypes = \[(.*?)\]", src).group(1).split(", ")
        decl = re.search(rf"^extern \w+ {sym}\((.*?)\);", hdr, re.M | re.S).group(1)
        assert decl.count(",") + 1 == len(args), sym
    assert "lib.nww_resample_length.restype = i64" in src


def test_rate_pairs_and_lengths():
    from nanowakeword_amd.augment import resample_ratio, resample_ratio_ok, resampled_length
    assert resample_ratio(48000) == (3, 1) and resample_ratio(44100) == (441, 160) and resample_ratio(22050) == (441, 320)
    assert resample_ratio(16000) is None and resample_ratio(8000) == (1, 2) and resample_ratio(16000, 48000) == (1, 3)
    for p, q in ro.ALL_RATIOS:
        assert resample_ratio_ok(p, q) and ro.ratio_ok(p, q), (p, q)
    for p, q in ro.BAD_RATIOS:
        assert not resample_ratio_ok(p, q) and not ro.ratio_ok(p, q), (p, q)
    for bad in (3999, 192001, 16001):                                  # below 1/4, above 12, a term above 1024
        with pytest.raises(ValueError, match="out of range"):
            resample_ratio(bad)
    for bad in (0, -8000, 22050.5):
        with pytest.raises(ValueError):
            resample_ratio(bad)
    assert resampled_length(48000, 48000) == 16000 and resampled_length(48001, 48000) == 16001 and resampled_length(1, 48000) == 1
    assert resampled_length(22050, 22050) == 16000 and resampled_length(22051, 22050) == 16001 and resampled_length(777, 16000) == 777
    for L in (1, 2, 37, 3070, 1 << 30):
        for p, q in ro.ALL_RATIOS:
            assert ro.length(L, p, q) == math.ceil(L * q / p) == -(-L * q // p)
    for bad in (0, (1 << 30) + 1):
        with pytest.raises(ValueError):
            resampled_length(bad, 48000)


@pytest.fixture(scope="module")
def resample_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resample_check") / "resample_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostemu", "resample_check.cpp")], check=True)

    def run(tables, tmp_path):
        """[(src, items, ratios, dst_values, dst_dtype or format code)] -> [dict(bad_ratio, formats_ok, bad, dst)]"""
        fsrc, fdst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fsrc, "wb") as f:
            f.write(struct.pack("<q", len(tables)))
            for src, items, ratios, dst_values, dst in tables:
                assert items.dtype == ro.RESAMPLE_ITEM
                sf = ro.PCM_F32 if src.dtype == np.float32 else ro.S16
                df = dst if isinstance(dst, int) else ro.PCM_F32 if np.dtype(dst) == np.float32 else ro.S16
                f.write(struct.pack("<qqqqqq", src.size, len(items), len(ratios), sf, df, dst_values))
                f.write(np.ascontiguousarray(src).tobytes())
                f.write(np.ascontiguousarray(items).tobytes())
                f.write(np.array([r[0] for r in ratios], np.int32).tobytes())
                f.write(np.array([r[1] for r in ratios], np.int32).tobytes())
        r = subprocess.run([exe, fsrc, fdst], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fdst, "rb").read()
        out, at = [], 0
        for src, items, ratios, dst_values, dst in tables:
            res = {}
            res["bad_ratio"], res["formats_ok"], idx = struct.unpack_from("<qqq", raw, at)
            res["bad"] = (idx, raw[at + 24:at + 40].split(b"\0")[0].decode())
            at += 40
            res["dst"] = None
            if res["bad_ratio"] < 0 and res["formats_ok"] and idx < 0:
                res["dst"] = np.frombuffer(raw, np.dtype(dst), dst_values, at)
                at += dst_values * np.dtype(dst).itemsize
            out.append(res)
        assert at == len(raw)
        return out
    run.exe = exe
    return run


def test_tables_are_numpys(resample_check, tmp_path):
    """float64, rounded once.  A failure here means this platform's libm and numpy disagree on a float64 cos / sin by enough to move a
    float32 rounding - the bit-for-bit tests below would then fail for that reason and no other."""
    dst = str(tmp_path / "taps.bin")
    for p, q in ro.ALL_RATIOS:
        subprocess.run([resample_check.exe, "--taps", str(p), str(q), dst], check=True)
        taps, j0, span = np.fromfile(dst, np.int32, 3).tolist()
        g = np.fromfile(dst, np.float32, offset=12).reshape(q, taps)
        c = 0.99 * min(1.0, q / p)
        assert taps == ro.taps(p, q) == 2 * math.ceil(6.0 / c) and j0 == ro.j0(p, q) == 1 - math.ceil(6.0 / c), (p, q)
        assert span == -(-(ro.TILE - 1) * p // q) + taps
        assert np.array_equal(g.view(np.uint32), ro.table(p, q).view(np.uint32)), (p, q)
        assert np.abs(g.astype(np.float64).sum(axis=1) - 1.0).max() < 2e-3, (p, q)
        x = ((np.arange(q) * p) % q / q)[:, None] - (j0 + np.arange(taps))[None, :]
        assert (g[np.abs(c * x) >= 6.0] == 0.0).all() and (g[np.abs(c * x) < 5.99] != 0.0).all()       # exact zeros outside the window, only there
    for (p, q), n in ro.TAPS_MEASURED.items():
        assert ro.taps(p, q) == n, (p, q)
    assert max(ro.taps(p, q) for p in range(1, 1025) for q in (1, 2, 85, 86, 341, 1024) if ro.ratio_ok(p, q)) == 146
    for p, q in ro.BAD_RATIOS:
        assert subprocess.run([resample_check.exe, "--taps", str(p), str(q), dst]).returncode == 2


@pytest.mark.parametrize("src_dtype,dst_dtype", PAIRS, ids=["s16-s16", "s16-f32", "f32-s16", "f32-f32"])
def test_walk_on_cpu_equals_restatement(resample_check, tmp_path, src_dtype, dst_dtype):
    """resample_item_host under the sanitizers against the restatement: the same bits for every ratio, C in {1, 2, 3}, the lengths on
    both sides of a tile boundary and below the tap count, and rows with rate_id == -1; what lies between the items is left alone"""
    recs, ids = ro.shape_cases(src_dtype)
    want = ro.shape_want(src_dtype, dst_dtype)
    src, items, dst_values = ro.pack(recs, ids, ro.ALL_RATIOS)
    res, = resample_check([(src, items, ro.ALL_RATIOS, dst_values, dst_dtype)], tmp_path)
    assert res["dst"] is not None, res
    raw = res["dst"].view(np.uint8)
    written = np.zeros(dst_values, bool)
    lens = ro.item_lengths(items, ro.ALL_RATIOS)
    bits = np.uint16 if np.dtype(dst_dtype) == np.int16 else np.uint32
    for i, it in enumerate(items):
        o = int(it["dst_off"])
        got = res["dst"][o:o + lens[i]]
        assert want[i].dtype == np.dtype(dst_dtype) and len(want[i]) == lens[i]
        assert np.array_equal(got.view(bits), want[i].view(bits)), (i, int(it["rate_id"]), int(it["src_frames"]), int(it["channels"]),
                                                                   np.argwhere(got != want[i])[:5].ravel())
        written[o:o + lens[i]] = True
    assert (~written).sum() == 3 * (len(items) // 5) and (raw.reshape(dst_values, -1)[~written] == 0x5a).all()
    assert max(float(np.abs(w.astype(np.float64)).max()) for w in want) > (1000 if np.dtype(dst_dtype) == np.int16 else 0.03)


def test_restatement_against_definition_after_the_int16_tail():
    recs, ratios, ref, meta = ro.load_golden()
    assert len(recs) == 8 and ratios == [ro.rate_ratio(fs) for fs, _ in ro.GOLDEN_PAIRS]
    for i, (x, r) in enumerate(zip(recs, ratios)):
        a, b = ro.restatement(x, r, np.int16).astype(np.int32), ro.definition(x, r, np.int16).astype(np.int32)
        share, dmax = float((a != b).mean()), int(np.abs(a - b).max())
        err = float(np.abs(ro.restatement_v(x, r).astype(np.float64) - ro.definition_v(x, r)).max())
        print(f"{ro.GOLDEN_PAIRS[i]} at {r[0]}/{r[1]}: int16 differing {100 * share:.3f} %, max {dmax} LSB, float32 error {err:.4f} LSB")
        assert share <= 0.005 and dmax <= 1, (i, share, dmax)
        assert abs(share - meta["restatement_differing_share"][i]) <= 1e-3 and dmax <= max(meta["restatement_max_abs_diff"][i], 1)
    assert max(meta["restatement_differing_share"]) <= 0.005 and max(meta["restatement_max_abs_diff"]) <= 1


def _tone(hz, fs, L, amp=0.5):
    return (amp * np.sin(2.0 * np.pi * hz * np.arange(L) / fs)).astype(np.float32)


EDGE = 20          # outputs left out at either end of a tone: a tone switched on is wide-band there, which is no matter of the filter's stop band


def _db(a, b):
    return 20.0 * np.log10(np.sqrt(np.mean(np.square(a.astype(np.float64)))) / np.sqrt(np.mean(np.square(b.astype(np.float64)))))


def test_properties_of_the_definition():
    x = _tone(1000.0, 48000.0, 24000)
    y = ro.definition(x, (3, 1), np.float32)
    assert y.size == 8000
    spec = np.abs(np.fft.rfft(y.astype(np.float64) * np.hanning(y.size)))
    assert abs(float(np.argmax(spec)) * 16000.0 / y.size - 1000.0) <= 2.0
    print("1 kHz at 48 k -> 16 k: rms", _db(y[EDGE:-EDGE], x), "dB; with the edges", _db(y, x))
    assert abs(_db(y[EDGE:-EDGE], x)) <= 0.05 and abs(_db(y, x)) <= 0.05
    y = ro.definition(_tone(12000.0, 48000.0, 24000), (3, 1), np.float32)
    print("12 kHz at 48 k -> 16 k:", _db(y[EDGE:-EDGE], x), "dB; with the edges", _db(y, x))
    assert _db(y[EDGE:-EDGE], x) <= -50.0
    x = _tone(10000.0, 44100.0, 22050)
    y = ro.definition(x, (441, 160), np.float32)
    print("10 kHz at 44.1 k -> 16 k:", _db(y[EDGE:-EDGE], x), "dB; with the edges", _db(y, x))
    assert y.size == 8000 and _db(y[EDGE:-EDGE], x) <= -40.0
    # the full-scale square wave overshoots and saturates: never wrapped
    sq = ro.square_wave()
    v = ro.definition_v(sq, (3, 1))
    print("square wave: overshoot", float(v.max()), float(v.min()))
    assert 37000.0 < v.max() < 38500.0 and v.min() < -37000.0
    for f in (ro.definition, ro.restatement):
        y = f(sq, (3, 1), np.int16)
        assert y.dtype == np.int16 and y.max() == 32767 and y.min() == -32768 and (y == 32767).sum() > 10 and (y == -32768).sum() > 10
        # wrapped samples would sit near the other rail inside a half-period: every sample has the sign of its half-period's middle
        mid = np.sign(y[8::16].astype(np.int32))
        assert (np.sign(y.astype(np.int32)).reshape(-1, 16)[:, 3:13] == mid[:, None]).all()
        yf = f((sq.astype(np.float32) / np.float32(32768.0)), (3, 1), np.int16)
        assert yf.max() == 32767 and yf.min() == -32768
    for p, q in ro.ALL_RATIOS:
        for dt in (np.int16, np.float32):
            z = np.zeros((300, 2), dt)
            for out in (np.int16, np.float32):
                y = ro.restatement(z, (p, q), out)
                assert y.size == ro.length(300, p, q) and not y.any() and not np.signbit(y.astype(np.float32)).any()
                assert not ro.definition(z, (p, q), out).any()
    # rounding to nearest even in the tail, and a row without a ratio is the downmix alone
    half = np.array([[1, 2], [3, 4], [-1, -2], [32767, 32767], [-32768, -32768]], np.int16)
    assert ro.restatement(half, None, np.int16).tolist() == [2, 4, -2, 32767, -32768]
    assert ro.restatement(half, None, np.float32).tolist() == [1.5 / 32768, 3.5 / 32768, -1.5 / 32768, 32767 / 32768, -1.0]
    f = np.array([0.25, -1.0, 1.0, 1.5e-5 * 3], np.float32)
    assert ro.restatement(f, None, np.int16).tolist() == [8192, -32768, 32767, 1] and np.array_equal(ro.restatement(f, None, np.float32), f)


def test_definition_and_restatement_against_the_golden(resample_check, tmp_path):
    recs, ratios, ref, meta = ro.load_golden()
    diff = []
    for i, (x, r) in enumerate(zip(recs, ratios)):
        assert ref[i].dtype == np.int16 and ref[i].size == ro.length(x.shape[0], *r) == 8000
        d = np.abs(ro.definition(x, r, np.int16).astype(np.int32) - ref[i].astype(np.int32))
        assert int(d.max()) <= 1 and (d > 0).mean() <= 1e-3, i                # float64 throughout: another libm may flip a rounding
        d = np.abs(ro.restatement(x, r, np.int16).astype(np.int32) - ref[i].astype(np.int32))
        diff.append(float((d > 0).mean()))
        assert int(d.max()) <= 1 and diff[-1] <= 0.005, (i, diff[-1])
    print("restatement against the golden, differing shares:", diff)
    # the walk gives the restatement on the golden's clips too
    uniq = sorted(set(ratios))
    ids = [uniq.index(r) for r in ratios]
    src, items, dst_values = ro.pack(recs, ids, uniq)
    res, = resample_check([(src, items, uniq, dst_values, np.int16)], tmp_path)
    for i, it in enumerate(items):
        o = int(it["dst_off"])
        assert np.array_equal(res["dst"][o:o + 8000], ro.restatement(recs[i], ratios[i], np.int16)), i
    # the allowance is not what lets a wrong ratio through
    wrong = ro.definition(recs[0], (2, 1), np.int16)[:8000]
    assert (wrong != ref[0]).mean() > 0.5


def test_refusals(resample_check, tmp_path):
    rng = np.random.default_rng(3)
    recs = [ro.speech_like(rng, L, C, 48000.0, np.int16) for L, C in ((500, 1), (300, 2), (40, 3), (700, 1))]
    ratios = [(3, 1), (441, 160)]
    ids = [0, 1, -1, 0]
    src, items, dst_values = ro.pack(recs, ids, ratios)
    tables, expect = [(src, items, ratios, dst_values, np.int16)], [("bad", (-1, ""))]
    for at in (1, 2, 3):
        for bad, field in ro.bad_items(src.size, dst_values, len(ratios), items[at]):
            t = items.copy()
            t[at] = bad
            tables.append((src, t, ratios, dst_values, np.int16)); expect.append(("bad", (at, field)))
    t = items.copy(); t[3]["channels"] = 0; t[1]["reserved"] = 7
    tables.append((src, t, ratios, dst_values, np.int16)); expect.append(("bad", (1, "reserved")))                 # the first is reported
    t = items.copy(); t[2]["dst_off"] = int(items[2]["dst_off"]) - 1
    tables.append((src, t, ratios, dst_values, np.int16)); expect.append(("bad", (2, "dst_off")))                  # overlaps the item before
    t = items.copy(); t[[1, 2]] = t[[2, 1]]
    tables.append((src, t, ratios, dst_values, np.int16)); expect.append(("bad", (2, "dst_off")))                  # not ascending
    tables.append((src, items, ratios, dst_values - 1, np.int16)); expect.append(("bad", (3, "dst_off")))          # the last item's end
    tables.append((src[:-1], items, ratios, dst_values, np.int16)); expect.append(("bad", (3, "src_off")))
    tables.append((src, items, [], dst_values, np.int16)); expect.append(("bad", (0, "rate_id")))                  # no ratios: no id is valid
    s2, i2, d2 = ro.pack(recs, [-1] * 4, [])
    tables.append((s2, i2, [], d2, np.int16)); expect.append(("bad", (-1, "")))                                    # ... but none is needed
    first = items.copy(); first[0]["dst_off"] = -1
    tables.append((src, first, ratios, dst_values, np.int16)); expect.append(("bad", (0, "dst_off")))
    for r in ro.BAD_RATIOS:
        tables.append((src, items, ratios + [r], dst_values, np.int16)); expect.append(("bad_ratio", 2))
    tables.append((src, items, ratios + [(2, 1)] * 15, dst_values, np.int16)); expect.append(("bad_ratio", 17))    # K <= 16
    tables.append((src, items, ratios + [(2, 1)] * 14, dst_values, np.int16)); expect.append(("bad_ratio", -1))
    tables.append((src, items, ratios + ro.RATIOS_AT_THE_BOUNDS, dst_values, np.int16)); expect.append(("bad_ratio", -1))
    tables.append((src, items, ratios, dst_values, 2)); expect.append(("formats_ok", 0))
    tables.append((src, items, ratios, dst_values, -1)); expect.append(("formats_ok", 0))
    for (key, want), res in zip(expect, resample_check(tables, tmp_path)):
        assert res[key] == want, (key, want, res)
        clean = res["bad_ratio"] < 0 and res["formats_ok"] and res["bad"][0] < 0
        assert (res["dst"] is not None) == bool(clean)


def test_plan_chunks_and_items():
    from nanowakeword_amd.augment import PCM_F32, PCM_S16, RESAMPLE_ITEM, ClipArena, as_resample_items, resample_plan, resampled_length
    rng = np.random.default_rng(4)
    recs = [ro.speech_like(rng, 2205, 1, 22050.0, np.int16), ro.speech_like(rng, 4800, 2, 48000.0, np.int16), ro.speech_like(rng, 1600, 1, 16000.0, np.int16),
            ro.speech_like(rng, 4410, 2, 44100.0, np.float32), ro.speech_like(rng, 800, 1, 8000.0, np.int16)]
    rates = [22050, 48000, 16000, 44100, 8000]
    out, lens, chunks = resample_plan(recs, rates)
    assert lens.dtype == np.int64 and lens.tolist() == [resampled_length(r.shape[0], hz) for r, hz in zip(recs, rates)] == [1600, 1600, 1600, 1600, 1600]
    assert [o.shape for o in out] == [(2205, 1), (4800, 2), (1600, 1), (4410, 2), (800, 1)] and all(o.flags.c_contiguous for o in out)
    assert [(c["lo"], c["hi"], c["format"], c["ratios"]) for c in chunks] == [(0, 3, PCM_S16, [(441, 320), (3, 1)]), (3, 4, PCM_F32, [(441, 160)]),
                                                                            (4, 5, PCM_S16, [(1, 2)])]
    t = chunks[0]["items"]
    assert t.dtype == RESAMPLE_ITEM and t["src_off"].tolist() == [0, 2205, 2205 + 9600] and t["dst_off"].tolist() == [0, 1600, 3200]
    assert t["rate_id"].tolist() == [0, 1, -1] and t["channels"].tolist() == [1, 2, 1] and (t["reserved"] == 0).all() and as_resample_items(t) is not None
    # bounded chunks: a recording larger than the bound goes alone, and a chunk names at most sixteen ratios
    _, _, small = resample_plan(recs[:3], rates[:3], chunk_bytes=5000)
    assert [(c["lo"], c["hi"]) for c in small] == [(0, 1), (1, 2), (2, 3)]
    many = [np.zeros(10, np.int16)] * 20
    _, _, ch = resample_plan(many, [16000 + 100 * k for k in range(1, 21)])
    assert [(c["lo"], c["hi"], len(c["ratios"])) for c in ch] == [(0, 16, 16), (16, 20, 4)]
    for bad in ([np.zeros((4, 9), np.int16)], [np.zeros(0, np.int16)], [np.zeros(4, np.float64)], [np.zeros((2, 2, 2), np.int16)], []):
        with pytest.raises(ValueError):
            resample_plan(bad, [48000] * len(bad))
    with pytest.raises(ValueError):
        resample_plan(recs, rates[:-1])
    with pytest.raises(ValueError):
        as_resample_items(np.zeros(3, np.int32))
    # the constructor and its attributes are as they were
    a = ClipArena([np.arange(5, dtype=np.int16), np.arange(3, dtype=np.int16)], device=None)
    assert a.lengths.tolist() == [5, 3] and a.offsets.tolist() == [0, 5] and a.samples == 8 and a.ptr == 0 and a.host.size == 8 and len(a) == 2
    assert isinstance(ClipArena.__dict__["from_recordings"], classmethod)
