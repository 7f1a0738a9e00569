"""The segmented route of nww_mix_rir_* (M = NWW_RIR_SEGMENTED: uniformly partitioned overlap-save on the 32768-point transform, for
clips and responses of any length), on the CPU: csrc/rir_plan.h's rir_seg_prepare_host / rir_seg_clip_host through
tests/hostemu/rir_seg_check.cpp, a stand-alone g++ program built with -ffp-contract=off -fsanitize=address,undefined, against the numpy
restatement of tests/rir_seg_oracle.py bit for bit; its accuracy against the float64 definition with the float32 library transform
(scipy.fft) as the yardstick; the reference route's golden at clips of 2 s (tests/golden/rir_seg.npz); the declarations, the sizes and
augment.py's host side.  The bounds are tests/test_rir_host.py's: 4 x the library transform, 4e-6 rms, 1 LSB, the 0.5 % cap.

Accuracy of w before the tail, max |w - w64| / rms(w64) per clip, at N = 32000 against decaying Gaussian responses of 800 / 16 000 /
32 000 taps: the walk 1.02e-6 / 1.09e-6 / 1.13e-6, scipy.fft's float32 rfft / irfft at n = N + L - 1 1.11e-6 / 1.67e-6 / 1.82e-6: the
walk is at 0.62 .. 0.91 of the yardstick (the bound is 4).  After the tail 0.08 .. 0.10 % of a clip's samples differ from the float64
definition, each by 1 LSB (the cap is 0.5 %)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mix_oracle
import rir_oracle
import rir_seg_oracle as seg
from conftest import ROOT
from test_rir_host import near_definition

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")
# (N, L): both sides of every boundary of ceil(min(L, N) / 16384) and of ceil(N / 16384), and arguments below 1
SIZE_TABLE = [(1, 1), (16384, 16384), (16385, 16384), (16385, 16385), (16384, 10 ** 6), (20000, 12770), (32000, 800), (32000, 16000), (32000, 32000),
              (32768, 32768), (32769, 32769), (32769, 32768), (40000, 40000), (100000, 49153), (2 ** 31 - 1, 2 ** 31 - 1), (0, 5), (5, 0), (-3, 7)]


@pytest.fixture(scope="module")
def seg_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rir_seg_check") / "rir_seg_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostemu", "rir_seg_check.cpp")], check=True)

    def run(tables, tmp_path):
        """[(arena, items, rir_items, irs, N)] -> [dict(bad, bad_rir, bad_ir, clips, w)]"""
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<q", len(tables)))
            for arena, items, rt, irs, N in tables:
                assert len(rt) == len(items) and rt.dtype == rir_oracle.RIR_ITEM
                f.write(struct.pack("<qqqq", arena.size, len(items), N, len(irs)))
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
        for arena, items, rt, irs, N in tables:
            res = dict(bad=name(16), bad_rir=name(16))
            res["bad_ir"], = struct.unpack_from("<q", raw, at)
            at += 8
            res["clips"] = res["w"] = None
            if res["bad"][0] < 0 and res["bad_rir"][0] < 0 and res["bad_ir"] < 0:
                n = len(items) * N
                res["clips"] = np.frombuffer(raw, np.int16, n, at).reshape(len(items), N)
                at += 2 * n
                res["w"] = np.frombuffer(raw, np.float32, n, at).reshape(len(items), N)
                at += 4 * n
            out.append(res)
        assert at == len(raw)
        return out

    def sizes(rows, tmp_path):
        """[(K, N, L, M)] -> int64 [n, 4]: rir_parts, rir_segments, rir_spectra_floats, rir_fft_size"""
        src, dst = str(tmp_path / "sizes_in.bin"), str(tmp_path / "sizes_out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<q", len(rows)))
            f.write(np.asarray(rows, np.int64).tobytes())
        subprocess.run([exe, "--sizes", src, dst], check=True)
        return np.fromfile(dst, np.int64).reshape(len(rows), 4)
    run.sizes = sizes
    return run


@pytest.fixture(scope="module")
def edge():
    """edge_cases_seg() with their clips and w by the restatement: computed once"""
    return [(name, N, irs, arena, items, ids) + seg.mix_rir(arena, items, ids, irs, N, with_w=True)
            for name, N, irs, arena, items, ids in seg.edge_cases_seg()]


def test_restatement_is_a_convolution():
    """the segmentation itself against the definition, before anything is compared with it: a delay across the partition boundary, a
    response of one tap, and a long decaying response over three segments"""
    rng = np.random.default_rng(1)
    N = 40000
    y = rng.standard_normal(N).astype(np.float32)
    delay = np.zeros(16385, np.float32); delay[-1] = -0.5
    for h in (np.array([1.0], np.float32), delay, rir_oracle.decaying(rng, 36000)):
        w = seg.convolve(y, seg.prepare(h, N))
        want = rir_oracle.w64(y, h)
        assert np.abs(w - want).max() <= 4e-6 * np.sqrt((want ** 2).mean()), h.size


def test_walk_on_cpu_equals_restatement(seg_check, tmp_path, edge):
    """rir_seg_clip_host over the edge cases, under the sanitizers, against rir_seg_oracle: the same bits, clips and w alike; rows
    without a response are mix_clip_host's (mix_oracle's) bits; and all of it near the float64 definition (test_rir_host's bounds)"""
    assert [c[1] for c in edge] == [1, 16384, 16385, 32768, 32769, 20000, 40000]
    tables = [(arena, items, rir_oracle.rir_items(ids), irs, N) for _, N, irs, arena, items, ids, _, _ in edge]
    for (name, N, irs, arena, items, ids, want, want_w), res in zip(edge, seg_check(tables, tmp_path)):
        assert res["clips"] is not None, (name, res)
        assert np.array_equal(res["clips"], want), (name, np.argwhere(res["clips"] != want)[:5])
        assert np.array_equal(res["w"].view(np.uint32), want_w.view(np.uint32)), name
        none = ids < 0
        assert none.any() and (~none).any()
        assert np.array_equal(res["clips"][none], mix_oracle.mix(arena, items[none], N)), name
        near_definition(res, arena, items, ids, irs, N, name)
    # what the cases were made for
    by = {c[0]: c for c in edge}
    assert rir_oracle.fft_size(20000, 12770) == 0 and by["refused"][2][0].size == 12770
    assert [seg.parts(16385, h.size) for h in by["q1+1"][2]] == [2, 1] and seg.segments(16385) == 2
    delay = by["q2"][2][1]
    assert delay.size == 16385 and np.flatnonzero(delay).tolist() == [16384] and seg.parts(32768, delay.size) == 2
    assert seg.parts(40000, 40000) == 3 and seg.segments(40000) == 3
    loud = by["refused"][2][1]
    assert loud.size > 20000 and np.abs(loud[20000:]).min() == 30.0          # taps beyond N are loud, and ignored


def test_routes_agree_with_the_definition_where_both_accept(seg_check, tmp_path):
    """N = 16000 with 4000 taps is accepted by both routes: each is within the bounds of the float64 definition.  They need NOT agree bit
    for bit - the one-workgroup route transforms the whole clip at once, the segmented one a window whose lower half is empty, and the
    roundings differ - so the share of differing int16 samples is printed, and bounded only through the definition (twice the 0.5 % cap)."""
    N = 16000
    arena, items, irs = rir_oracle.accuracy_inputs(N)
    ids = np.array([1, 1, 1], np.int32)
    assert rir_oracle.fft_size(N, irs[1].size) == 32768 and irs[1].size == 4000
    ref = rir_oracle.definition(arena, items, ids, irs, N)
    res, = seg_check([(arena, items, rir_oracle.rir_items(ids), irs, N)], tmp_path)
    one = rir_oracle.mix_rir(arena, items, ids, irs, N, 32768)
    assert np.array_equal(res["clips"], seg.mix_rir(arena, items, ids, irs, N))
    rir_oracle.conditions(res["clips"], ref, "segmented")
    rir_oracle.conditions(one, ref, "one workgroup")
    near_definition(res, arena, items, ids, irs, N, "segmented")
    d = res["clips"].astype(np.int32) - one
    print(f"segmented against one workgroup: {int((d != 0).sum())} of {d.size} samples differ ({100 * (d != 0).mean():.4f} %), max {int(np.abs(d).max())} LSB")
    assert np.abs(d).max() <= 2 and (d != 0).mean() <= 0.01


def test_accuracy_against_definition_and_library_transform(seg_check, tmp_path):
    """w before the tail at the reference's clip length: the walk's error may be at most 4 times that of the float32 library transform on
    the same inputs; after the tail every sample within 1 LSB of the float64 definition and at most 0.5 % of a clip's samples different"""
    import scipy.fft as sf
    N = 32000
    arena, items, _ = rir_oracle.accuracy_inputs(N)
    rng = np.random.default_rng(12)
    irs = [rir_oracle.decaying(rng, L) for L in (800, 16000, 32000)]
    ids = np.arange(3, dtype=np.int32)
    res, = seg_check([(arena, items, rir_oracle.rir_items(ids), irs, N)], tmp_path)
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
    assert np.array_equal(res["clips"], seg.mix_rir(arena, items, ids, irs, N))


def test_restatement_and_walk_against_reference_golden(seg_check, tmp_path):
    arena, items, ids, irs, ref, meta = seg.load_golden()
    N = meta["N"]
    assert N == 32000 and ref.shape == (4, N) and ref.dtype == np.int16 and len(items) == 4 and ids.tolist() == [0, 1, 2, 3]
    assert items.dtype == mix_oracle.MIX_ITEM and int(items[0]["bg_len"]) == 0 and int(items[1]["bg_len"]) == 53      # none; tiled
    assert all(rir_oracle.fft_size(N, h.size) == 0 for h in irs)                                  # none of them fits the other route
    res, = seg_check([(arena, items, rir_oracle.rir_items(ids), irs, N)], tmp_path)
    assert np.array_equal(res["clips"], seg.mix_rir(arena, items, ids, irs, N))
    rir_oracle.conditions(res["clips"], ref, "golden")
    rir_oracle.conditions(rir_oracle.definition(arena, items, ids, irs, N), ref, "definition against golden")
    # the cap is not what lets a misplaced tap through: the response one sample late moves far more than 0.5 % of the samples
    late = [np.r_[np.float32(0), h] for h in irs]
    d = rir_oracle.definition(arena, items[1:3], ids[1:3], late, N).astype(np.int32) - ref[1:3]
    assert (d != 0).mean() > 0.05


def test_declarations_and_sizes(seg_check, tmp_path):
    from nanowakeword_amd import _lib, augment
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    assert re.search(r"^#define NWW_RIR_SEGMENTED \(-1\)", hdr, re.M) and augment.RIR_SEGMENTED == seg.SEGMENTED == -1
    assert re.search(r"^extern int32_t nww_rir_parts\(int32_t N, int32_t max_ir_len\);", hdr, re.M)
    assert re.search(r"^extern int64_t nww_rir_spectra_floats\(int32_t K, int32_t N, int32_t max_ir_len, int32_t M\);", hdr, re.M)
    assert {"nww_rir_parts", "nww_rir_spectra_floats"} <= set(_lib.SYMBOLS) and len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    assert "overlap-save not built" in hdr and "pass NWW_RIR_SEGMENTED" in hdr
    rows = [(K, N, L, M) for N, L in SIZE_TABLE for K in (1, 3, 64) for M in (-1, 2048, 32768, 0, 4096)]
    got = seg_check.sizes(rows, tmp_path)
    for (K, N, L, M), (parts, segs, floats, fft) in zip(rows, got.tolist()):
        ok = N >= 1 and L >= 1
        want_parts = -(-min(L, N) // 16384) if ok else 0
        assert parts == want_parts == augment.rir_parts(N, L) == seg.parts(N, L), (N, L)
        assert segs == (-(-N // 16384) if N >= 1 else 0)
        assert fft == augment.rir_fft_size(N, L)
        want = 0
        if ok and M == -1:
            want = ((K + 2 + 3) & ~3) + K * want_parts * 32768                   # the counts' header, then [K][P][32768 / 2] complex
        elif ok and M in (2048, 32768):
            want = K * M                                                         # a transform size: today's rule
        assert floats == want == augment.rir_spectra_floats(K, N, L, M) == seg.spectra_floats(K, N, L, M), (K, N, L, M)
    assert augment.rir_parts(32000, 12000) == 1 and augment.rir_parts(32000, 32000) == 2 and augment.rir_parts(16385, 10 ** 6) == 2


def test_bad_items_and_responses_are_rejected_with_their_index(seg_check, tmp_path):
    """the rules that stay: mix items, rir items; a response without taps.  What the other route refuses for its length passes here"""
    _, N, irs, arena, items, ids = seg.edge_cases_seg()[0]
    good = rir_oracle.rir_items(ids)
    tables, expect = [], []
    for k, (bad, field) in enumerate(rir_oracle.bad_rir_items(len(irs))):
        t = good.copy()
        t[k % len(t)] = bad
        tables.append((arena, items, t, irs, N)); expect.append(("bad_rir", (k % len(t), field)))
    bad_mix = items.copy(); bad_mix[1] = mix_oracle.bad_items(arena.size, N)[0][0]
    tables.append((arena, bad_mix, good, irs, N)); expect.append(("bad", (1, "fg_len")))
    tables.append((arena, items, good, irs + [np.zeros(0, np.float32)], N)); expect.append(("bad_ir", len(irs)))
    a20 = np.zeros(20000, np.int16)
    tables.append((a20, mix_oracle.item(0, 1), rir_oracle.rir_items([0]), [np.zeros(12770, np.float32)], 20000)); expect.append(("bad_ir", -1))
    for (key, want), res in zip(expect, seg_check(tables, tmp_path)):
        assert res[key] == want, (key, want, res[key])
        assert (res["clips"] is None) == (want != -1)


def test_ir_arena_segmented_on_the_host():
    from nanowakeword_amd.augment import IrArena, RIR_SEGMENTED
    rng = np.random.default_rng(4)
    short = [rir_oracle.decaying(rng, L) for L in (800, 4000)]
    a = IrArena(short, 16000, device=None, segmented=True)
    assert a.M == 32768 and a.parts == 0                                      # a transform size fits: the one-workgroup route and its bits
    assert IrArena(short, 1000, device=None, segmented=True).M == IrArena(short, 1000, device=None).M == 2048
    b = IrArena([np.ones(12770, np.float32)], 20000, device=None, segmented=True)
    assert b.M == RIR_SEGMENTED and b.parts == 1 and b.n == 1 and b.N == 20000
    c = IrArena(short + [rir_oracle.decaying(rng, 40000)], 32000, device=None, segmented=True, normalize="peak")
    assert c.M == RIR_SEGMENTED and c.parts == 2 and c.lengths.tolist() == [800, 4000, 40000] and float(np.abs(c.host).max()) == 1.0
    with pytest.raises(ValueError, match="overlap-save not built"):           # without the argument: as before
        IrArena([np.ones(12770, np.float32)], 20000, device=None)
    with pytest.raises(ValueError, match="overlap-save not built"):
        IrArena([np.ones(12770, np.float32)], 20000, device=None, segmented=False)
    with pytest.raises(ValueError):
        IrArena([np.ones(12770, np.float32)], 20000, device=None, segmented=True, M=32768)
    with pytest.raises(ValueError, match="prepare"):
        b.spectra_ptr
    # the segmented route by name, for clips a transform size would hold - and only together with segmented=True
    f = IrArena(short, 16000, device=None, segmented=True, M=RIR_SEGMENTED)
    assert f.M == RIR_SEGMENTED and f.parts == 1
    with pytest.raises(ValueError, match="M must be one of"):
        IrArena(short, 16000, device=None, M=RIR_SEGMENTED)
