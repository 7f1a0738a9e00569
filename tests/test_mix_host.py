"""Clips mixed on the device (nww_mix_*), on the CPU: the four declarations of include/nww.h and the item's layout; the numpy
restatement tests/mix_oracle.py against the reference's own chain (tests/golden/mix.npz, tools/make_mix_goldens.py); csrc/mix_plan.h -
the validation and the per-sample arithmetic the kernel runs - through tests/hostemu/mix_check.cpp, a stand-alone g++ program built with
-ffp-contract=off -fsanitize=address,undefined, against the restatement bit for bit; and augment.py's table builders."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mix_oracle
from conftest import ROOT
from mix_oracle import golden_conditions, load_golden

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")
MIX = ["nww_mix_dev", "nww_mix", "nww_mix_forward_pcm_dev", "nww_mix_frontend_dev"]
EDGE_N = (1, 8, 250, 1001, 16000)


def test_declarations_and_item_layout():
    from nanowakeword_amd import _lib, augment
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    for sym in MIX:
        assert re.search(rf"^extern int {sym}\(", hdr, re.M), sym
        assert sym in _lib.SYMBOLS
    assert len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    body = hdr[hdr.index("typedef struct nww_mix_item {") + len("typedef struct nww_mix_item {"):hdr.index("} nww_mix_item;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, kinds = [], []
    for decl in body.split(";"):
        m = re.match(r"\s*(int64_t|int32_t|uint32_t|float)\s+(.*)", decl.strip(), flags=re.S)
        if m:
            for n in m.group(2).split(","):
                names.append(n.strip()); kinds.append({"int64_t": "<i8", "int32_t": "<i4", "uint32_t": "<u4", "float": "<f4"}[m.group(1)])
    for dt in (augment.MIX_ITEM, mix_oracle.MIX_ITEM):
        assert list(dt.names) == names and [dt[n].str for n in names] == kinds
        assert dt.itemsize == 48 == sum(np.dtype(k).itemsize for k in kinds)            # no implicit padding
    assert int(re.search(r"#define NWW_MIX_PEAK_NORMALISE (\d+)u", hdr).group(1)) == augment.PEAK_NORMALISE


def test_restatement_against_reference_golden():
    arena, items, ref, meta = load_golden()
    N = meta["N"]
    assert ref.shape == (40, N) and ref.dtype == np.int16
    share = golden_conditions(mix_oracle.mix(arena, items, N), ref)
    assert share == pytest.approx(meta["differing_share"]) and meta["max_abs_diff"] <= 1
    # the cap is not what lets a wrong scale through: 1 % more foreground moves far more than 0.5 % of the samples
    off = items.copy()
    off["snr_linear"] *= np.float32(1.01)
    d = mix_oracle.mix(arena, off[:4], N).astype(np.int32) - ref[:4]
    assert (d != 0).mean() > 0.05


@pytest.fixture(scope="module")
def mix_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mix_check") / "mix_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostemu", "mix_check.cpp")], check=True)

    def run(tables, tmp_path):
        """[(arena, items, N)] -> [(bad index, field, clips or None)]"""
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<q", len(tables)))
            for arena, items, N in tables:
                f.write(struct.pack("<qqq", arena.size, len(items), N))
                f.write(np.ascontiguousarray(arena, np.int16).tobytes())
                f.write(np.ascontiguousarray(items).tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(dst, "rb").read()
        out, at = [], 0
        for arena, items, N in tables:
            bad, = struct.unpack_from("<q", raw, at)
            field = raw[at + 8:at + 24].split(b"\0")[0].decode()
            at += 24
            clips = None
            if bad < 0:
                clips = np.frombuffer(raw, np.int16, len(items) * N, at).reshape(len(items), N)
                at += 2 * len(items) * N
            out.append((bad, field, clips))
        assert at == len(raw)
        return out
    return run


def test_mix_plan_on_cpu_equals_restatement(mix_check, tmp_path):
    """csrc/mix_plan.h over the edge table at every N, under the sanitizers, against mix_oracle: the same bits"""
    tables = []
    for N in EDGE_N:
        arena, items = mix_oracle.edge_table(N)
        assert all(mix_oracle.bad_field(it, arena.size, N) is None for it in items)
        tables.append((arena, mix_oracle.table_of(items, 65 if N <= 1001 else len(items)), N))
    for (arena, items, N), (bad, field, clips) in zip(tables, mix_check(tables, tmp_path)):
        assert bad == -1 and field == "", (N, bad, field)
        assert np.array_equal(clips, mix_oracle.mix(arena, items, N)), N


def test_mix_plan_on_cpu_equals_reference_golden(mix_check, tmp_path):
    arena, items, ref, meta = load_golden()
    (bad, _, clips), = mix_check([(arena, items, meta["N"])], tmp_path)
    assert bad == -1
    golden_conditions(clips, ref)
    assert np.array_equal(clips, mix_oracle.mix(arena, items, meta["N"]))


def test_bad_items_are_rejected_with_their_index(mix_check, tmp_path):
    N = 250
    arena, items = mix_oracle.edge_table(N)
    bads = mix_oracle.bad_items(arena.size, N)
    assert {f for _, f in bads} == {"fg_len", "fg_off", "bg_len", "bg_off", "bg_start", "start", "snr_linear", "gain", "level", "flags"}
    tables = []
    for k, (bad, field) in enumerate(bads):
        assert mix_oracle.bad_field(bad, arena.size, N) == field
        t = items[:12].copy()
        t[(5 * k) % 12] = bad
        tables.append((arena, t, N))
    # two bad items: the first is reported; a background that is not read (bg_len == 0) may hold anything
    t = items[:12].copy(); t[7] = bads[0][0]; t[3] = bads[-1][0]
    tables.append((arena, t, N))
    free = mix_oracle.item(1, 5, bg_off=-9, bg_len=0, bg_start=77)
    tables.append((arena, free, N))
    res = mix_check(tables, tmp_path)
    for k, (bad, field) in enumerate(bads):
        assert res[k][0] == (5 * k) % 12 and res[k][1] == field and res[k][2] is None, (k, field, res[k][:2])
    assert res[-2][:2] == (3, "flags")
    assert res[-1][0] == -1 and np.array_equal(res[-1][2], mix_oracle.mix(arena, free, N))


class _Arena:                                    # what the table builders read of an augment.ClipArena
    def __init__(self, lengths):
        self.lengths = np.asarray(lengths, np.int64)
        self.offsets = np.concatenate(([0], np.cumsum(self.lengths)[:-1]))
        self.samples = int(self.lengths.sum())

    def __len__(self):
        return len(self.lengths)


def test_clip_arena_on_the_host():
    from nanowakeword_amd.augment import ClipArena
    clips = [np.arange(5, dtype=np.int16), np.arange(3, dtype=np.int16) - 7, np.ones(4, np.int16)]
    a = ClipArena(clips, device=None)
    assert a.ptr == 0 and a.samples == 12 and len(a) == 3
    assert a.offsets.tolist() == [0, 5, 8] and a.lengths.tolist() == [5, 3, 4]
    assert np.array_equal(a.host, np.concatenate(clips))
    for bad in ([], [np.zeros(3, np.float32)], [np.zeros((2, 2), np.int16)], [np.zeros(0, np.int16)]):
        with pytest.raises(ValueError):
            ClipArena(bad, device=None)


def test_mix_items_broadcasts():
    from nanowakeword_amd.augment import MIX_ITEM, mix_items
    arena = _Arena([9000, 20000, 16000, 700, 48000])
    N = 16000
    fg, bg, snrs = np.array([0, 1]), np.array([3, 4, -1]), np.array([0.0, 6.0, 12.0, 20.0])
    t = mix_items(arena, fg[:, None, None], bg[None, :, None], N, snr_db=snrs[None, None, :], level=0.8, bg_start=[[[5], [100], [0]]])
    assert t.dtype == MIX_ITEM and t.shape == (24,)
    g = t.reshape(2, 3, 4)
    assert (g["fg_off"][0] == 0).all() and (g["fg_off"][1] == 9000).all()
    assert (g["fg_len"][0] == 9000).all() and (g["fg_len"][1] == 16000).all()           # cut to the clip
    assert (g["bg_off"][:, 0] == 45000).all() and (g["bg_len"][:, 0] == 700).all() and (g["bg_start"][:, 0] == 5).all()
    assert (g["bg_len"][:, 1] == 48000).all() and (g["bg_start"][:, 1] == 100).all()
    assert (g["bg_len"][:, 2] == 0).all() and (g["bg_off"][:, 2] == 0).all() and (g["bg_start"][:, 2] == 0).all()
    assert np.array_equal(g["snr_linear"][1, 2], (10.0 ** (snrs / 20.0)).astype(np.float32))
    assert (t["gain"] == 1.0).all() and (t["level"] == np.float32(0.8)).all() and (t["flags"] == 1).all() and (t["start"] == 0).all()
    assert all(mix_oracle.bad_field(it, arena.samples, N) is None for it in t)
    t2 = mix_items(arena, 1, 2, N, fg_crop=4000, gain_db=-6.0, peak_normalise=False, start=0)
    assert t2.shape == (1,) and t2["fg_off"][0] == 13000 and t2["fg_len"][0] == 16000 and t2["flags"][0] == 0
    assert t2["gain"][0] == np.float32(10.0 ** -0.3)
    with pytest.raises(ValueError):
        mix_items(arena, 5, 0, N)
    with pytest.raises(ValueError):
        mix_items(arena, 3, 0, N, fg_crop=700)


def test_draw_mix_items_stays_in_its_ranges():
    from nanowakeword_amd.augment import DEFAULT_SETTINGS, draw_mix_items
    arena = _Arena([9000, 20000, 16000, 700, 48000, 53, 16001])
    N = 16000
    fg = np.tile([0, 1, 2], 400)
    t = draw_mix_items(np.random.default_rng(11), arena, fg, [3, 4, 5, 6], N)
    assert len(t) == 1200 and all(mix_oracle.bad_field(it, arena.samples, N) is None for it in t)
    assert np.array_equal(t, draw_mix_items(np.random.default_rng(11), arena, fg, [3, 4, 5, 6], N))         # the generator alone decides
    assert set(np.unique(t["bg_len"])) == {700, 48000, 53, 16001}
    long_bg = t["bg_len"] > N
    assert (t["bg_start"][long_bg] <= t["bg_len"][long_bg] - N).all() and t["bg_start"][t["bg_len"] == 48000].max() > 16000     # a crop
    assert (t["bg_start"][~long_bg] == 0).all()                                                                              # tiled from its start
    assert (t["fg_len"] == np.minimum(arena.lengths[fg], N)).all()
    crop = t["fg_off"] - arena.offsets[fg]
    assert (crop[fg != 1] == 0).all() and crop[fg == 1].min() >= 0 and crop[fg == 1].max() <= 4000 and crop[fg == 1].max() > 2000
    assert (t["start"] >= 0).all() and (t["start"] <= N - t["fg_len"]).all() and t["start"][fg == 0].max() > 3500
    d = DEFAULT_SETTINGS
    assert (d["min_snr_in_db"], d["max_snr_in_db"], d["min_gain_in_db"], d["max_gain_in_db"]) == (5.0, 30.0, -3.0, 3.0)      # augment_clips.py:139-145
    assert (d["min_volume_augmentation"], d["max_volume_augmentation"], d["gain_prob"]) == (0.5, 1.0, 1.0)
    snr_db, gain_db = 20 * np.log10(t["snr_linear"].astype(np.float64)), 20 * np.log10(t["gain"].astype(np.float64))
    assert 5.0 - 1e-5 <= snr_db.min() < 6.0 and 29.0 < snr_db.max() <= 30.0 + 1e-5
    assert -3.0 - 1e-5 <= gain_db.min() < -2.7 and 2.7 < gain_db.max() <= 3.0 + 1e-5
    assert 0.5 <= t["level"].min() < 0.52 and 0.98 < t["level"].max() <= 1.0 and (t["flags"] == 1).all()
    # settings override the ranges; no backgrounds at all: none drawn
    t = draw_mix_items(np.random.default_rng(3), arena, fg[:50], [], N, {"min_snr_in_db": 0.0, "max_snr_in_db": 0.0, "gain_prob": 0.0})
    assert (t["bg_len"] == 0).all() and (t["snr_linear"] == 1.0).all() and (t["gain"] == 1.0).all()
