"""Recordings brought to the target rate (nww_resample_*, csrc/resample.hip) on the GPU: the kernel against the float32 restatement of
tests/resample_oracle.py bit for bit - every ratio, channel count and the lengths on both sides of a tile boundary and below the tap
count in ONE table per format pair - batch invariance beside a recording of many tiles, saturation, the host-pointer form, an arena
built by ClipArena.from_recordings under nww_mix, the validation, and the definition's golden (tests/golden/resample.npz)."""
import numpy as np
import pytest

import mix_oracle
import resample_oracle as ro
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

PAIRS = [(np.int16, np.int16), (np.int16, np.float32), (np.float32, np.int16), (np.float32, np.float32)]
FILL = 0x5a


def _model():
    from nanowakeword_amd.session import HipModel
    cfg = HeadConfig("cnn", (101, 64))
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))


@pytest.fixture(scope="module")
def model():
    m = _model()
    yield m
    m.close()


def all_ratios(m):
    """the ratios the shape cases name (HipModel.resample and ClipArena.from_recordings set their own)"""
    m.resample_set_ratios(*zip(*ro.ALL_RATIOS))


def fmt(dtype):
    return ro.PCM_F32 if np.dtype(dtype) == np.float32 else ro.S16


def run_dev(m, src, items, dst_values, dst_dtype):
    """nww_resample_dev on a destination whose every byte is FILL -> the destination"""
    import torch
    dev = f"cuda:{m.device}"
    d_src = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
    d_dst = torch.full((dst_values * np.dtype(dst_dtype).itemsize,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(m.device)                                   # the call runs on the handle's own stream
    m.resample_dev(d_src.data_ptr(), src.size, fmt(src.dtype), items, d_dst.data_ptr(), dst_values, fmt(dst_dtype))
    torch.cuda.synchronize(m.device)
    return d_dst.cpu().numpy().view(dst_dtype)


def check_items(got, items, want, dst_dtype, ratios=ro.ALL_RATIOS):
    """every item's range equals want[i] bit for bit; every byte outside the ranges is FILL"""
    bits = np.uint16 if np.dtype(dst_dtype) == np.int16 else np.uint32
    lens = ro.item_lengths(items, ratios)
    written = np.zeros(got.size, bool)
    for i, it in enumerate(items):
        o = int(it["dst_off"])
        assert len(want[i]) == lens[i] and want[i].dtype == np.dtype(dst_dtype)
        g = got[o:o + lens[i]]
        assert np.array_equal(g.view(bits), want[i].view(bits)), (i, int(it["rate_id"]), int(it["src_frames"]), int(it["channels"]),
                                                                 np.argwhere(g != want[i])[:5].ravel(), g[:4], want[i][:4])
        written[o:o + lens[i]] = True
    assert (got.view(np.uint8).reshape(got.size, -1)[~written] == FILL).all()
    return written


@pytest.mark.parametrize("src_dtype,dst_dtype", PAIRS, ids=["s16-s16", "s16-f32", "f32-s16", "f32-f32"])
def test_kernel_equals_restatement(model, src_dtype, dst_dtype):
    """the CPU walk's shapes: every ratio of ALL_RATIOS x C in {1, 2, 3} x {1, 2, taps - 1, the frames that give RESAMPLE_TILE - 1,
    RESAMPLE_TILE, RESAMPLE_TILE + 1 and 3 RESAMPLE_TILE + 5 outputs}, and rows with rate_id == -1"""
    all_ratios(model)
    recs, ids = ro.shape_cases(src_dtype)
    want = ro.shape_want(src_dtype, dst_dtype)
    src, items, dst_values = ro.pack(recs, ids, ro.ALL_RATIOS)
    got = run_dev(model, src, items, dst_values, dst_dtype)
    written = check_items(got, items, want, dst_dtype)
    assert (~written).sum() == 3 * (len(items) // 5)
    assert len(items) == 3 * sum(len(ro.lengths(p, q)) for p, q in ro.ALL_RATIOS) + 15


def test_batch_invariance(model):
    """an item's bits are the same alone, at another place of the table, and beside a stereo recording of 200 000 frames whose tiles lie
    before and behind theirs"""
    all_ratios(model)
    recs, ids = ro.shape_cases(np.int16)
    want = ro.shape_want(np.int16, np.int16)
    pick = [i for i, (x, r) in enumerate(zip(recs, ids)) if r in (0, 3, 5, -1) and x.shape[0] > 40][::3]
    assert len(pick) >= 8 and {ids[i] for i in pick} == {0, 3, 5, -1}
    for i in pick[:4]:
        src, items, dv = ro.pack([recs[i]], [ids[i]], ro.ALL_RATIOS)
        check_items(run_dev(model, src, items, dv, np.int16), items, [want[i]], np.int16)
    order = pick[::-1]
    src, items, dv = ro.pack([recs[i] for i in order], [ids[i] for i in order], ro.ALL_RATIOS, gap_every=2, gap=7)
    check_items(run_dev(model, src, items, dv, np.int16), items, [want[i] for i in order], np.int16)
    big = ro.speech_like(np.random.default_rng(21), 200000, 2, 48000.0, np.int16)
    big_want = ro.restatement(big, (3, 1), np.int16)
    assert big_want.size == 66667
    h = len(pick) // 2
    table = [recs[i] for i in pick[:h]] + [big] + [recs[i] for i in pick[h:]] + [big]
    tids = [ids[i] for i in pick[:h]] + [0] + [ids[i] for i in pick[h:]] + [0]
    twant = [want[i] for i in pick[:h]] + [big_want] + [want[i] for i in pick[h:]] + [big_want]
    src, items, dv = ro.pack(table, tids, ro.ALL_RATIOS)
    check_items(run_dev(model, src, items, dv, np.int16), items, twant, np.int16)


def test_saturation(model):
    sq = ro.square_wave()
    want = ro.restatement(sq, (3, 1), np.int16)
    assert want.max() == 32767 and want.min() == -32768 and (want == 32767).sum() > 10 and (want == -32768).sum() > 10
    got, = model.resample([sq], [48000])
    assert got.dtype == np.int16 and np.array_equal(got, want)
    sqf = sq.astype(np.float32) / np.float32(32768.0)
    got, = model.resample([sqf], [48000])
    assert np.array_equal(got, ro.restatement(sqf, (3, 1), np.int16)) and got.max() == 32767 and got.min() == -32768
    got, = model.resample([sq], [48000], dtype=np.float32)                                  # float32 keeps the overshoot
    assert np.array_equal(got, ro.restatement(sq, (3, 1), np.float32)) and 1.14 < got.max() < 1.18


def test_host_form_equals_device_form(model):
    import ctypes as C
    all_ratios(model)
    for src_dtype, dst_dtype in PAIRS:
        recs, ids = ro.shape_cases(src_dtype)
        sel = list(range(0, len(recs), 7))
        src, items, dv = ro.pack([recs[i] for i in sel], [ids[i] for i in sel], ro.ALL_RATIOS, gap_every=3, gap=5)
        dev = run_dev(model, src, items, dv, dst_dtype)
        host = np.full(dv * np.dtype(dst_dtype).itemsize, FILL, np.uint8).view(dst_dtype)
        model._check(model.lib.nww_resample(model._h, src.ctypes.data_as(C.c_void_p), src.size, fmt(src_dtype), items.ctypes.data_as(C.c_void_p), len(items),
                                            host.ctypes.data_as(C.c_void_p), dv, fmt(dst_dtype)))
        assert np.array_equal(host.view(np.uint8), dev.view(np.uint8)), (src_dtype, dst_dtype)     # what lies between the items included
        check_items(host, items, [ro.shape_want(src_dtype, dst_dtype)[i] for i in sel], dst_dtype)
    # HipModel.resample: one array per recording, any mix of formats and rates
    rng = np.random.default_rng(8)
    recs = [ro.speech_like(rng, 2205, 1, 22050.0, np.int16), ro.speech_like(rng, 4800, 2, 48000.0, np.float32), ro.speech_like(rng, 1600, 3, 16000.0, np.int16)]
    rates = [22050, 48000, 16000]
    for dt in (np.int16, np.float32):
        got = model.resample(recs, rates, dtype=dt)
        for g, x, hz in zip(got, recs, rates):
            r = None if hz == 16000 else ro.rate_ratio(hz)
            assert g.dtype == np.dtype(dt) and np.array_equal(g, ro.restatement(x, r, dt))


def test_an_arena_from_recordings_mixes_as_the_restatements_clips(model):
    from nanowakeword_amd.augment import ClipArena, mix_items, resampled_length
    rng = np.random.default_rng(9)
    recs = [ro.speech_like(rng, 11025, 1, 22050.0, np.int16), ro.speech_like(rng, 30000, 2, 48000.0, np.int16, amp=4000.0),
            ro.speech_like(rng, 7000, 1, 16000.0, np.int16)]
    rates = [22050, 48000, 16000]
    a = ClipArena.from_recordings(model, recs, rates)
    clips = [ro.restatement(x, None if hz == 16000 else ro.rate_ratio(hz), np.int16) for x, hz in zip(recs, rates)]
    b = ClipArena(clips)
    assert a.lengths.tolist() == b.lengths.tolist() == [resampled_length(x.shape[0], hz) for x, hz in zip(recs, rates)] == [8000, 10000, 7000]
    assert a.offsets.tolist() == b.offsets.tolist() and a.samples == b.samples == 25000 and a.host is None and a.ptr and len(a) == 3 and a.device == 0
    assert np.array_equal(a._dev.cpu().numpy(), np.concatenate(clips))
    N = 8000
    items = mix_items(a, np.array([0, 2, 0, 2]), np.array([1, 1, -1, 1]), N, snr_db=np.array([5.0, 15.0, 20.0, 0.0]), start=np.array([0, 300, 0, 1000]),
                      bg_start=np.array([0, 17, 0, 2500]))
    assert np.array_equal(items, mix_items(b, np.array([0, 2, 0, 2]), np.array([1, 1, -1, 1]), N, snr_db=np.array([5.0, 15.0, 20.0, 0.0]),
                                          start=np.array([0, 300, 0, 1000]), bg_start=np.array([0, 17, 0, 2500])))
    got = model.mix(a, items, N)
    assert np.array_equal(got, model.mix(b, items, N)) and np.array_equal(got, mix_oracle.mix(np.concatenate(clips), items, N))
    assert np.abs(got.astype(np.int32)).max() > 1000
    # bounded chunks give the same arena; float32 sources too
    c = ClipArena.from_recordings(model, recs, rates, chunk_bytes=1000)
    assert np.array_equal(c._dev.cpu().numpy(), np.concatenate(clips))
    f = [(x.astype(np.float32) / np.float32(32768.0)) for x in recs]
    d = ClipArena.from_recordings(model, [f[0], recs[1], f[2]], rates)
    assert np.array_equal(d._dev.cpu().numpy(), np.concatenate([ro.restatement(f[0], (441, 320), np.int16), clips[1], ro.restatement(f[2], None, np.int16)]))
    with pytest.raises(ValueError):
        ClipArena.from_recordings(model, recs, rates, device=None)


def test_refusals_leave_the_next_call_alone():
    import ctypes as C
    m = _model()
    rng = np.random.default_rng(3)
    recs = [ro.speech_like(rng, L, Cn, 48000.0, np.int16) for L, Cn in ((5000, 1), (3100, 2), (40, 3), (7000, 1))]
    ratios = [(3, 1), (441, 160)]
    ids = [0, 1, -1, 0]
    src, items, dv = ro.pack(recs, ids, ratios)
    want = [ro.restatement(x, None if r < 0 else ratios[r], np.int16) for x, r in zip(recs, ids)]

    def host_form(t, src=src, dv=dv, sf=ro.S16, df=ro.S16):
        out = np.full(dv, 0x5a5a, np.int16)
        m._check(m.lib.nww_resample(m._h, src.ctypes.data_as(C.c_void_p), src.size, sf, t.ctypes.data_as(C.c_void_p), len(t), out.ctypes.data_as(C.c_void_p),
                                    dv, df))
        return out
    with pytest.raises(ValueError, match="no resample ratios set"):                              # before any ratios
        run_dev(m, src, items, dv, np.int16)
    s1, i1, d1 = ro.pack(recs, [-1] * 4, [])                                                     # ... rows that name none need none
    check_items(run_dev(m, s1, i1, d1, np.int16), i1, [ro.restatement(x, None, np.int16) for x in recs], np.int16, [])
    for p, q in ro.BAD_RATIOS:
        with pytest.raises(ValueError, match=r"resample ratio 1: "):
            m.resample_set_ratios([3, p], [1, q])
    with pytest.raises(ValueError, match="number of resample ratios"):
        m.resample_set_ratios([3] * 17, [1] * 17)
    with pytest.raises(ValueError, match="no resample ratios set"):                              # a refused set changed nothing
        run_dev(m, src, items, dv, np.int16)
    m.resample_set_ratios(*zip(*ratios))
    check_items(run_dev(m, src, items, dv, np.int16), items, want, np.int16, ratios)
    for at in (1, 2, 3):
        for bad, field in ro.bad_items(src.size, dv, len(ratios), items[at]):
            t = items.copy()
            t[at] = bad
            with pytest.raises(ValueError, match=rf"resample item {at}: {field}\b"):
                run_dev(m, src, t, dv, np.int16)
            with pytest.raises(ValueError, match=rf"resample item {at}: {field}\b"):
                host_form(t)
    t = items.copy(); t[[1, 2]] = t[[2, 1]]
    with pytest.raises(ValueError, match=r"resample item 2: dst_off\b"):                          # destinations must ascend
        run_dev(m, src, t, dv, np.int16)
    with pytest.raises(ValueError, match=r"resample item 3: dst_off\b"):
        run_dev(m, src, items, dv - 1, np.int16)
    for sf, df, name in ((2, 0, "src_format"), (0, 2, "dst_format"), (-1, 1, "src_format")):
        with pytest.raises(ValueError, match=name):
            host_form(items, sf=sf, df=df)
    with pytest.raises(ValueError):
        m.resample_dev(0, src.size, 0, items, 0, dv, 0)                                          # null pointers
    m.resample_dev(0, 0, 0, items[:0], 0, 0, 0)                                                  # B == 0: nothing to do, nothing is read
    assert np.array_equal(host_form(items), run_dev(m, src, items, dv, np.int16))
    check_items(run_dev(m, src, items, dv, np.int16), items, want, np.int16, ratios)
    with pytest.raises(ValueError, match=r"resample ratio 0: "):                                  # a refused set keeps the ratios that were
        m.resample_set_ratios([13], [1])
    check_items(run_dev(m, src, items, dv, np.int16), items, want, np.int16, ratios)
    assert int(m.lib.nww_resample_length(48000, 3, 1)) == 16000 and int(m.lib.nww_resample_length(48001, 3, 1)) == 16001
    assert int(m.lib.nww_resample_length(22050, 441, 320)) == 16000 and int(m.lib.nww_resample_length(1 << 30, 1, 4)) == 1 << 32
    assert [int(m.lib.nww_resample_length(*a)) for a in ((0, 3, 1), ((1 << 30) + 1, 3, 1), (100, 13, 1), (100, 1, 5), (100, 0, 1))] == [0] * 5
    m.resample_set_ratios([], [])                                                                # K = 0 clears them
    with pytest.raises(ValueError, match="no resample ratios set"):
        run_dev(m, src, items, dv, np.int16)
    m.close()


def test_against_the_definitions_golden(model):
    recs, ratios, ref, meta = ro.load_golden()
    got = model.resample(recs, [fs for fs, _ in ro.GOLDEN_PAIRS])
    for i, (g, x, r) in enumerate(zip(got, recs, ratios)):
        assert np.array_equal(g, ro.restatement(x, r, np.int16)), i
        d = np.abs(g.astype(np.int32) - ref[i].astype(np.int32))
        print(ro.GOLDEN_PAIRS[i], "differing", float((d > 0).mean()), "max", int(d.max()))
        assert int(d.max()) <= 1 and (d > 0).mean() <= 0.005, i
