"""Clips through room impulse responses (nww_rir_* / nww_mix_rir_*), on the CPU: the declarations of include/nww.h; csrc/rir_plan.h - the
twiddle table, the validation and the walk of a whole clip, rir_clip_host - through tests/hostemu/rir_check.cpp, a stand-alone g++
program built with -ffp-contract=off -fsanitize=address,undefined, against the float32 restatement of tests/rir_oracle.py bit for bit at
every transform size; the accuracy of the walk against the float64 definition, with the float32 library transform (scipy.fft) on the
same inputs as the yardstick; the reference route's golden (tests/golden/rir.npz); and augment.py's host side.

Accuracy of w before the tail, max |w - w64| / rms(w64) per clip, on Gaussian clips under a slow envelope against exponentially decaying
Gaussian responses of 800 / 4000 / 16 000 taps (rir_oracle.accuracy_inputs): the walk 8.5e-7 .. 9.5e-7, scipy.fft's float32 rfft / irfft
at n = N + L - 1 1.3e-6 .. 1.9e-6: the walk is at 0.44 .. 0.75 of the yardstick (the bound is 4)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mix_oracle
import rir_oracle
from conftest import ROOT

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")
RIR = ["nww_rir_fft_size", "nww_rir_prepare_dev", "nww_mix_rir_dev", "nww_mix_rir", "nww_mix_rir_forward_pcm_dev", "nww_mix_rir_frontend_dev"]


def test_declarations_and_item_layout():
    from nanowakeword_amd import _lib, augment
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    for sym in RIR:
        assert re.search(rf"^extern (int|int32_t) {sym}\(", hdr, re.M), sym
        assert sym in _lib.SYMBOLS
    assert len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    assert "typedef struct nww_rir_item { int32_t ir_id; uint32_t reserved; } nww_rir_item;" in hdr
    for dt in (augment.RIR_ITEM, rir_oracle.RIR_ITEM):
        assert dt.names == ("ir_id", "reserved") and [dt[n].str for n in dt.names] == ["<i4", "<u4"] and dt.itemsize == 8
    # the existing item and calls are as they were
    assert augment.MIX_ITEM == mix_oracle.MIX_ITEM and augment.MIX_ITEM.itemsize == 48
    assert "overlap-save not built" in hdr


@pytest.fixture(scope="module")
def rir_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rir_check") / "rir_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostemu", "rir_check.cpp")], check=True)

    def run(tables, tmp_path):
        """[(arena, items, rir_items, irs, N, M)] -> [dict(bad, bad_rir, bad_ir, size_ok, clips, w)]"""
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<q", len(tables)))
            for arena, items, rt, irs, N, M in tables:
                assert len(rt) == len(items) and rt.dtype == rir_oracle.RIR_ITEM
                f.write(struct.pack("<qqqqq", arena.size, len(items), N, M, len(irs)))
                f.write(np.ascontiguousarray(arena, np.int16).tobytes())
                f.write(np.ascontiguousarray(items).tobytes())
                f.write(np.ascontiguousarray(rt).tobytes())
                for h in irs:
                    f.write(struct.pack("<q", h.size))
                    f.write(np.ascontiguousarray(h, np.float32).tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(dst, "rb").read()
        out, at = [], 0

        def name(width):
            nonlocal at
            idx, = struct.unpack_from("<q", raw, at)
            s = raw[at + 8:at + 8 + width].split(b"\0")[0].decode()
            at += 8 + width
            return idx, s
        for arena, items, rt, irs, N, M in tables:
            res = dict(bad=name(16), bad_rir=name(16), bad_ir=name(32))
            res["size_ok"], = struct.unpack_from("<q", raw, at)
            at += 8
            res["clips"] = res["w"] = None
            if res["bad"][0] < 0 and res["bad_rir"][0] < 0 and res["bad_ir"][0] < 0 and res["size_ok"]:
                n = len(items) * N
                res["clips"] = np.frombuffer(raw, np.int16, n, at).reshape(len(items), N)
                at += 2 * n
                res["w"] = np.frombuffer(raw, np.float32, n, at).reshape(len(items), N)
                at += 4 * n
            out.append(res)
        assert at == len(raw)
        return out
    run.exe = exe
    return run


@pytest.mark.parametrize("M", rir_oracle.SIZES)
def test_twiddle_table_is_numpys(rir_check, tmp_path, M):
    """ONE table per M, float64 cos / sin rounded once.  A failure here means this platform's libm and numpy disagree on a float64
    cos / sin by enough to move a float32 rounding - the bit-for-bit tests below would then fail for that reason and no other."""
    dst = str(tmp_path / "tw.bin")
    subprocess.run([rir_check.exe, "--twiddles", str(M), dst], check=True)
    T = np.fromfile(dst, np.float32).reshape(-1, 2)
    c, s = rir_oracle.twiddles(M)
    assert T.shape == (3 * M // 4, 2)
    assert np.array_equal(T[:, 0], c) and np.array_equal(T[:, 1], s), "libm and numpy disagree on the twiddle table"
    assert T[0, 0] == 1.0 and T[0, 1] == 0.0


def test_restatement_is_a_convolution():
    """the network itself against the definition, before anything is compared with it: a delta, a delay, and the split's symmetry"""
    for M in rir_oracle.SIZES:
        rng = np.random.default_rng(M)
        N = M // 2 + 8
        y = rng.standard_normal(N).astype(np.float32)
        for h in (np.array([1.0], np.float32), np.r_[np.zeros(9, np.float32), np.float32(-0.5)], rir_oracle.decaying(rng, M // 2 - 7)):
            w = rir_oracle.convolve(y, rir_oracle.prepare(h, N, M), M)
            want = rir_oracle.w64(y, h)
            assert np.abs(w - want).max() <= 4e-6 * np.sqrt((want ** 2).mean()), (M, h.size)


def near_definition(res, arena, items, ids, irs, N, what):
    """The edge tables against the float64 definition.  Their clips include full-scale square patterns whose exact samples lie ON the
    truncation's integers, where any rounding flips a sample by 1 LSB - so the 0.5 % cap of the accuracy test, made for noise-like
    clips, does not apply; what keeps a wrong scale or a misplaced tap out here is w itself: within 4e-6 of rms(w64) - four times the
    float32 library transform's worst figure (9.0e-7 .. 1.0e-6 measured at these sizes), the margin the accuracy test grants - and then
    every int16 sample within 1 LSB plus what that bound on w is worth in LSBs behind the clip's ratio r (nothing under peak
    normalisation, where r rms <= 1; several LSBs for a row without it whose loud response lifts w far above full scale)."""
    ref = rir_oracle.definition(arena, items, ids, irs, N)
    for i in range(len(items)):
        tol = 0
        if ids[i] >= 0:
            want = rir_oracle.w64(rir_oracle.mix_y(arena, items[i], N), irs[ids[i]])
            rms = float(np.sqrt((want ** 2).mean()))
            err = float(np.abs(res["w"][i] - want).max())
            assert err <= 4e-6 * rms, (what, i, err, rms)
            pk = float(np.abs(want).max())
            r = float(items[i]["level"]) / (pk if pk >= 1e-8 else 1.0) if int(items[i]["flags"]) & 1 else float(items[i]["level"])
            tol = 1 + int(4e-6 * rms * r * 32767.0)
            assert tol == 1 or not int(items[i]["flags"]) & 1
        d = np.abs(res["clips"][i].astype(np.int32) - ref[i])
        assert int(d.max()) <= tol, (what, i, int(d.max()), tol)


@pytest.mark.parametrize("M", rir_oracle.SIZES)
def test_walk_on_cpu_equals_restatement(rir_check, tmp_path, M):
    """rir_clip_host over the edge cases of every transform size, under the sanitizers, against rir_oracle: the same bits; rows without
    a response are mix_clip_host's (mix_oracle's) bits"""
    cases = rir_oracle.edge_cases(M)
    tables = [(arena, items, rir_oracle.rir_items(ids), irs, N, M) for _, N, irs, arena, items, ids in cases]
    for (name, N, irs, arena, items, ids), res in zip(cases, rir_check(tables, tmp_path)):
        assert res["clips"] is not None, (name, res)
        want = rir_oracle.mix_rir(arena, items, ids, irs, N, M)
        assert np.array_equal(res["clips"], want), (M, name, np.argwhere(res["clips"] != want)[:5])
        none = ids < 0
        assert none.any() and (~none).any()
        assert np.array_equal(res["clips"][none], mix_oracle.mix(arena, items[none], N)), (M, name)
        near_definition(res, arena, items, ids, irs, N, f"M={M} {name}")


def test_small_clips_at_larger_sizes(rir_check, tmp_path):
    """a caller may take a larger M than the smallest: the same clip at every size that holds it, each against the restatement"""
    _, N, irs, arena, items, ids = rir_oracle.edge_cases(2048)[1]
    tables = [(arena, items, rir_oracle.rir_items(ids), irs, N, M) for M in rir_oracle.SIZES]
    for M, res in zip(rir_oracle.SIZES, rir_check(tables, tmp_path)):
        assert np.array_equal(res["clips"], rir_oracle.mix_rir(arena, items, ids, irs, N, M)), M
        near_definition(res, arena, items, ids, irs, N, f"M={M}")


def test_accuracy_against_definition_and_library_transform(rir_check, tmp_path):
    """w before the tail: the walk's error may be at most 4 times that of the float32 library transform on the same inputs; after the
    tail every sample within 1 LSB of the float64 definition and at most 0.5 % of a clip's samples different at all"""
    import scipy.fft as sf
    N, M = 16000, 32768
    arena, items, irs = rir_oracle.accuracy_inputs(N)
    ids = np.arange(3, dtype=np.int32)
    res, = rir_check([(arena, items, rir_oracle.rir_items(ids), irs, N, M)], tmp_path)
    for i in range(3):
        y = rir_oracle.mix_y(arena, items[i], N)
        want = rir_oracle.w64(y, irs[i])
        rms = float(np.sqrt((want ** 2).mean()))
        n = N + irs[i].size - 1
        lib = sf.irfft(sf.rfft(y, n) * sf.rfft(irs[i], n), n)[:N]
        assert lib.dtype == np.float32
        e_walk, e_lib = float(np.abs(res["w"][i] - want).max()) / rms, float(np.abs(lib - want).max()) / rms
        print(f"L = {irs[i].size}: walk {e_walk:.3e}, scipy.fft float32 {e_lib:.3e}, ratio {e_walk / e_lib:.2f}")
        assert e_walk <= 4.0 * e_lib
    rir_oracle.conditions(res["clips"], rir_oracle.definition(arena, items, ids, irs, N), "accuracy")
    assert np.array_equal(res["clips"], rir_oracle.mix_rir(arena, items, ids, irs, N, M))


def test_restatement_and_walk_against_reference_golden(rir_check, tmp_path):
    arena, items, ids, irs, ref, meta = rir_oracle.load_golden()
    N = meta["N"]
    assert ref.shape == (8, N) and ref.dtype == np.int16 and len(items) == 8 and (ids >= 0).all()
    res, = rir_check([(arena, items, rir_oracle.rir_items(ids), irs, N, 32768)], tmp_path)
    assert np.array_equal(res["clips"], rir_oracle.mix_rir(arena, items, ids, irs, N, 32768))
    rir_oracle.conditions(res["clips"], ref, "golden")
    rir_oracle.conditions(rir_oracle.definition(arena, items, ids, irs, N), ref, "definition against golden")
    # the cap is not what lets a misplaced tap through: the response one sample late moves far more than 0.5 % of the samples
    late = [np.r_[np.float32(0), h] for h in irs]
    d = rir_oracle.definition(arena, items[1:3], ids[1:3], late, N).astype(np.int32) - ref[1:3]
    assert (d != 0).mean() > 0.05


def test_bad_items_and_oversized_responses_are_rejected_with_their_index(rir_check, tmp_path):
    _, N, irs, arena, items, ids = rir_oracle.edge_cases(2048)[0]
    good = rir_oracle.rir_items(ids)
    tables, expect = [], []
    for k, (bad, field) in enumerate(rir_oracle.bad_rir_items(len(irs))):
        t = good.copy()
        t[(3 * k) % len(t)] = bad
        tables.append((arena, items, t, irs, N, 2048)); expect.append(("bad_rir", ((3 * k) % len(t), field)))
    t = good.copy(); t[5] = rir_oracle.bad_rir_items(len(irs))[0][0]; t[2] = rir_oracle.bad_rir_items(len(irs))[3][0]
    tables.append((arena, items, t, irs, N, 2048)); expect.append(("bad_rir", (2, "reserved")))           # the first is reported
    bad_mix = items.copy(); bad_mix[4] = mix_oracle.bad_items(arena.size, N)[0][0]
    tables.append((arena, bad_mix, good, irs, N, 2048)); expect.append(("bad", (4, "fg_len")))
    for M in (0, 1024, 4096, 65536):                                                                      # none of the three sizes
        tables.append((arena, items, good, irs, N, M)); expect.append(("size_ok", 0))
    # oversized: N + min(L, N) - 1 > 32768 - response 1 of three; N <= 16384 fits with any response; a response of no taps
    one = mix_oracle.item(0, 1)
    z = np.zeros(1, np.float32)
    big = np.zeros(40000, np.float32)
    a20 = np.zeros(20000, np.int16)
    rt1 = rir_oracle.rir_items([-1])
    tables.append((a20, one, rt1, [z, np.zeros(12770, np.float32), z], 20000, 32768)); expect.append(("bad_ir", (1, "overlap-save not built")))
    tables.append((a20, one, rt1, [z, np.zeros(12769, np.float32)], 20000, 32768)); expect.append(("bad_ir", (-1, "")))
    tables.append((a20, one, rt1, [big], 16384, 32768)); expect.append(("bad_ir", (-1, "")))
    tables.append((a20, one, rt1, [big], 16385, 32768)); expect.append(("bad_ir", (0, "overlap-save not built")))
    tables.append((a20, one, rt1, [z, z, np.zeros(0, np.float32)], 100, 2048)); expect.append(("bad_ir", (2, "ir_len")))
    tables.append((a20, one, rt1, [z, np.zeros(1950, np.float32)], 100, 2048)); expect.append(("bad_ir", (-1, "")))   # min(L, N) counts
    tables.append((a20, one, rt1, [z, np.zeros(100, np.float32)], 2000, 2048)); expect.append(("bad_ir", (1, "M")))   # fits 8192, not this M
    tables.append((a20, one, rt1, [z], 2049, 2048)); expect.append(("size_ok", 0))                                    # N > M
    for (key, want), res in zip(expect, rir_check(tables, tmp_path)):
        assert res[key] == want, (key, want, res[key])
        if key != "bad_ir" or want[0] >= 0:
            assert res["clips"] is None
    assert [rir_oracle.fft_size(n, l) for n, l in ((1, 1), (1025, 1024), (1025, 1025), (16384, 10 ** 6), (16385, 16385), (16385, 16384))] == \
        [2048, 2048, 8192, 32768, 0, 32768]


def test_ir_arena_on_the_host():
    from nanowakeword_amd.augment import IrArena, RIR_ITEM, as_rir_items, draw_rir_ids, rir_fft_size
    for n, l in ((1, 1), (1025, 1024), (1025, 1025), (4097, 4097), (16000, 16000), (16384, 10 ** 6), (16385, 16384), (0, 5), (5, 0)):
        assert rir_fft_size(n, l) == (rir_oracle.fft_size(n, l) if n >= 1 and l >= 1 else 0), (n, l)
    rng = np.random.default_rng(4)
    irs = [rir_oracle.decaying(rng, L, 3.0) for L in (5, 800, 301)]
    a = IrArena(irs, 1000, device=None)
    assert a.n == len(a) == 3 and a.M == 2048 and a.N == 1000
    assert a.offsets.tolist() == [0, 5, 805] and a.lengths.tolist() == [5, 800, 301] and a.lengths.dtype == np.int32 and a.offsets.dtype == np.int64
    assert a.host.dtype == np.float32 and np.array_equal(a.host, np.concatenate(irs))
    with pytest.raises(ValueError, match="prepare"):
        a.spectra_ptr
    assert IrArena(irs + [np.ones(1000, np.float32)], 1100, device=None).M == 8192        # the longest decides: 1100 + 1000 - 1 = 2099
    assert IrArena([np.ones(5000, np.float64)], 1000, device=None).M == 2048              # taps beyond N do not count
    e = IrArena(irs, 1000, device=None, normalize="energy")
    p = IrArena(irs, 1000, device=None, normalize="peak")
    for k, h in enumerate(irs):
        he, hp = e.host[e.offsets[k]:][:e.lengths[k]], p.host[p.offsets[k]:][:p.lengths[k]]
        h64 = h.astype(np.float64)
        assert np.array_equal(he, (h64 / np.sqrt((h64 ** 2).sum())).astype(np.float32)) and abs(float((he.astype(np.float64) ** 2).sum()) - 1) < 1e-6
        assert np.array_equal(hp, (h64 / np.abs(h64).max()).astype(np.float32)) and float(np.abs(hp).max()) == 1.0
    for bad in ([], [np.zeros(0, np.float32)], [np.zeros((2, 2), np.float32)], [np.array([1, 2])], [np.array([np.nan], np.float32)]):
        with pytest.raises(ValueError):
            IrArena(bad, 1000, device=None)
    with pytest.raises(ValueError, match="cannot be normalised"):
        IrArena([np.zeros(4, np.float32)], 1000, device=None, normalize="peak")
    with pytest.raises(ValueError, match="normalize"):
        IrArena(irs, 1000, device=None, normalize="rms")
    with pytest.raises(ValueError, match="overlap-save not built"):
        IrArena([np.ones(12770, np.float32)], 20000, device=None)
    # ids
    ids = draw_rir_ids(np.random.default_rng(2), 64, 4000)
    assert ids.dtype == np.int32 and ids.shape == (4000,) and ids.min() == -1 and ids.max() == 63
    assert np.array_equal(ids, draw_rir_ids(np.random.default_rng(2), 64, 4000))
    assert 0.46 < (ids >= 0).mean() < 0.54 and len(np.unique(ids)) == 65                   # rir_prob = 0.5 (augment_clips.py:150-157)
    assert (draw_rir_ids(np.random.default_rng(2), 3, 50, 1.0) >= 0).all() and (draw_rir_ids(np.random.default_rng(2), 3, 50, 0.0) == -1).all()
    assert (draw_rir_ids(np.random.default_rng(2), 0, 7) == -1).all()
    t = as_rir_items(ids[:9], 9)
    assert t.dtype == RIR_ITEM and np.array_equal(t["ir_id"], ids[:9]) and (t["reserved"] == 0).all() and as_rir_items(t, 9) is not None
    for bad in (ids[:8], np.zeros(9, np.float32), np.zeros((3, 3), np.int32)):
        with pytest.raises(ValueError):
            as_rir_items(bad, 9)


def test_mixed_feature_batches_carry_the_ids():
    from nanowakeword_amd.augment import mixed_feature_batches
    items = np.concatenate([mix_oracle.item(k, 5) for k in range(7)])
    ids = np.arange(7) - 1
    got = list(mixed_feature_batches(items, 3, irs=object(), ir_ids=ids))
    assert [len(b[0]) for b in got] == [3, 3, 1] and np.array_equal(np.concatenate([b[1]["ir_id"] for b in got]), ids)
    assert all(np.array_equal(b, items[3 * i:3 * i + 3]) for i, b in enumerate(mixed_feature_batches(items, 3)))      # as before without
    with pytest.raises(ValueError):
        list(mixed_feature_batches(items, 3, ir_ids=ids))
