"""Clips shifted in pitch (nww_pitch_set_ratios / nww_mix_aug_*, csrc/pitch.hip) on the GPU: the kernels against the float32 restatement
of tests/pitch_oracle.py bit for bit at every clip length at which they take another path, batch invariance at B = 1, 3 and 65, rows
without a ratio against nww_mix, ratios with responses on both of rir.hip's routes, the forward / frontend / host-pointer forms against
the calls they compose, the validation, and the definition's golden (tests/golden/pitch.npz) through the C-ABI."""
import numpy as np
import pytest

import mix_oracle
import pitch_oracle
import rir_oracle
import rir_seg_oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

RATIOS = pitch_oracle.RATIOS
_CASES = {}


def case(N):
    """(arena, items, ids, the restatement's clips) at clip length N, computed once: pitch_oracle.clip_table's rows - with a background,
    without, the island between exact zeros, a short foreground with exact zeros behind it - every ratio of RATIOS and a row without
    one; two clips at N = 16000"""
    if N not in _CASES:
        arena, items = pitch_oracle.clip_table(N)
        if N == 16000:
            items, ids = items[[0, 3]].copy(), np.array([0, 5], np.int32)
        else:
            items = mix_oracle.table_of(items, 8)
            ids = np.array([0, 1, 2, 3, 4, 5, -1, 1], np.int32)
        _CASES[N] = (arena, items, ids, pitch_oracle.mix_aug(arena, items, ids, RATIOS, N))
    return _CASES[N]


@pytest.fixture(scope="module")
def model():
    from nanowakeword_amd.session import HipModel
    cfg = HeadConfig("cnn", (101, 64))
    m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))
    yield m
    m.close()


@pytest.fixture(scope="module")
def bank():
    from nanowakeword_amd.augment import PitchBank
    return PitchBank(RATIOS)


def dev_arena(arena):
    from nanowakeword_amd.augment import ClipArena
    return ClipArena([arena])


# 257: the smallest allowed (T = 3); 384: T_out small, one tile; 2000 / 4000: several tiles, a partial last one; 16000: clips of a second
@pytest.mark.parametrize("N", [257, 384, 2000, 4000, 16000])
def test_kernels_equal_restatement(model, bank, N):
    arena, items, ids, want = case(N)
    got = model.mix(dev_arena(arena), items, N, pitch=bank, pitch_ids=ids)
    assert got.shape == want.shape and got.dtype == np.int16
    for i in range(len(items)):
        assert np.array_equal(got[i], want[i]), (N, i, int(ids[i]), np.argwhere(got[i] != want[i])[:5].ravel(), got[i][:4], want[i][:4])
    assert np.abs(want.astype(np.int32)).max() > 1000


def test_batch_invariance(model, bank):
    """B = 1, 3 and 65: a clip's bits are the same alone, in a small table, and at any place of a table larger than 64, among clips with
    and without a ratio"""
    N = 2000
    arena, items, ids, want = case(N)
    a = dev_arena(arena)
    for i in (0, 3, 6):
        assert np.array_equal(model.mix(a, items[i:i + 1], N, pitch=bank, pitch_ids=ids[i:i + 1]), want[i:i + 1]), i
    for lo in (0, 5):
        assert np.array_equal(model.mix(a, items[lo:lo + 3], N, pitch=bank, pitch_ids=ids[lo:lo + 3]), want[lo:lo + 3]), lo
    order = (np.arange(65) * 5) % 8
    got = model.mix(a, items[order].copy(), N, pitch=bank, pitch_ids=ids[order].copy())
    assert np.array_equal(got, want[order])


def test_rows_without_a_ratio_are_nww_mix(model, bank):
    N = 2000
    arena, items, ids, want = case(N)
    a = dev_arena(arena)
    plain = model.mix(a, items, N)
    assert np.array_equal(plain, mix_oracle.mix(arena, items, N))
    assert np.array_equal(model.mix(a, items, N, pitch=bank, pitch_ids=np.full(len(items), -1)), plain)
    none = ids < 0
    assert none.any() and np.array_equal(want[none], plain[none])
    assert not np.array_equal(want[~none], plain[~none])                     # the shift is heard


def test_with_responses_at_a_transform_size(model, bank):
    from nanowakeword_amd.augment import IrArena
    N, M = 2000, 2048
    arena, items, ids, _ = case(N)
    rng = np.random.default_rng(5)
    irs = [rir_oracle.decaying(rng, L) for L in (49, 7)]
    ir_ids = np.array([0, -1, 1, 0, -1, 1, 0, -1], np.int32)
    ia = IrArena(irs, N)
    assert ia.M == M
    a = dev_arena(arena)
    want = pitch_oracle.mix_aug(arena, items, ids, RATIOS, N, ir_ids=ir_ids, irs=irs, M=M)
    got = model.mix(a, items, N, irs=ia, ir_ids=ir_ids, pitch=bank, pitch_ids=ids)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=1)).ravel()
    only_ir = model.mix(a, items, N, irs=ia, ir_ids=ir_ids)                  # nww_mix_rir_dev
    none = ids < 0
    assert np.array_equal(got[none], only_ir[none])
    assert np.array_equal(model.mix(a, items, N, irs=ia, ir_ids=ir_ids, pitch=bank, pitch_ids=np.full(8, -1)), only_ir)
    both = (ids >= 0) & (ir_ids >= 0)
    assert both.any() and not np.array_equal(got[both], only_ir[both])


def test_with_responses_on_the_segmented_route(model, bank):
    from nanowakeword_amd.augment import IrArena, RIR_SEGMENTED
    N = 4000
    arena, items, ids, _ = case(N)
    rng = np.random.default_rng(6)
    irs = [rir_oracle.decaying(rng, L) for L in (300, 4000)]
    ir_ids = np.array([1, -1, 0, 1, -1, 0, 1, -1], np.int32)
    ia = IrArena(irs, N, segmented=True, M=RIR_SEGMENTED)
    assert ia.M == RIR_SEGMENTED
    specs = {k: rir_seg_oracle.prepare(h, N) for k, h in enumerate(irs)}
    want = pitch_oracle.mix_aug(arena, items, ids, RATIOS, N, ir_ids=ir_ids, after=lambda w, k: rir_seg_oracle.convolve(w, specs[k]))
    a = dev_arena(arena)
    got = model.mix(a, items, N, irs=ia, ir_ids=ir_ids, pitch=bank, pitch_ids=ids)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=1)).ravel()
    only_ir = model.mix(a, items, N, irs=ia, ir_ids=ir_ids)
    assert np.array_equal(got[ids < 0], only_ir[ids < 0])


def test_composite_and_host_forms(model, bank):
    from nanowakeword_amd.augment import IrArena, MixedClips, mixed_feature_batches
    from nanowakeword_amd.features import HipFeatures
    from nanowakeword_amd.session import HipSession
    N = 16000
    arena, items = pitch_oracle.clip_table(N)
    items = mix_oracle.table_of(items, 7)
    ids = np.array([0, -1, 3, 5, -1, 1, 4], np.int32)
    a = dev_arena(arena)
    clips = model.mix(a, items, N, pitch=bank, pitch_ids=ids)
    assert np.array_equal(model.mix(arena, items, N, pitch=bank, pitch_ids=ids), clips)          # the host-pointer form
    lg, pr = model.forward_mixed(a, items, N, pitch=bank, pitch_ids=ids)
    lg0, pr0 = model.forward_pcm(clips)
    assert np.isfinite(lg).all() and np.array_equal(lg, lg0) and np.array_equal(pr, pr0)
    assert not np.array_equal(lg, model.forward_mixed(a, items, N)[0])
    s = HipSession(model, mode="e2e", clip_samples=N)
    assert np.array_equal(s.mix(a, items, pitch=bank, pitch_ids=ids), clips)
    assert np.array_equal(s.forward_mixed(a, items, pitch=bank, pitch_ids=ids)[0], pr0.reshape(-1, 1, 1))
    # with responses as well, host-pointer form against the device form
    ia = IrArena([rir_oracle.decaying(np.random.default_rng(1), 800)], N)
    ir_ids = np.array([0, 0, -1, 0, -1, -1, 0], np.int32)
    both = model.mix(a, items, N, irs=ia, ir_ids=ir_ids, pitch=bank, pitch_ids=ids)
    assert np.array_equal(model.mix(arena, items, N, irs=ia, ir_ids=ir_ids, pitch=bank, pitch_ids=ids), both)
    f = HipFeatures()
    fb = type(bank)(RATIOS)
    got = f.embed_mixed(a, items, N, pitch=fb, pitch_ids=ids)
    assert got.shape == (7, 101, 64) and np.array_equal(got, f.embed_clips(clips, batch_size=7))
    rows = [MixedClips(f, a, N, pitch=fb).embed_clips(b) for b in mixed_feature_batches(items, 4, pitch=fb, pitch_ids=ids)]
    assert np.array_equal(np.concatenate(rows), got)
    f.close()


class _NoBank:
    """a bank that sets nothing: the call reaches the C-ABI with whatever ratios the model holds"""
    def prepare(self, model):
        return self


def test_refusals_leave_the_next_call_alone(bank):
    from nanowakeword_amd.augment import PitchBank
    from nanowakeword_amd.session import HipModel
    cfg = HeadConfig("cnn", (101, 64))
    m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))
    N = 2000
    arena, items, ids, want = case(N)
    a = dev_arena(arena)
    good = pitch_oracle.pitch_items(ids)
    with pytest.raises(ValueError, match="no pitch ratios set"):                                  # before any ratios
        m.mix(a, items, N, pitch=_NoBank(), pitch_ids=good)
    for num, den in pitch_oracle.BAD_RATIOS:
        with pytest.raises(ValueError, match=r"pitch ratio 1: "):
            m.pitch_set_ratios([9, num], [8, den])
    with pytest.raises(ValueError, match=r"number of pitch ratios"):
        m.pitch_set_ratios([9] * 65, [8] * 65)
    with pytest.raises(ValueError, match="no pitch ratios set"):                                  # a refused set changed nothing
        m.mix(a, items, N, pitch=_NoBank(), pitch_ids=good)
    m.pitch_set_ratios(*zip(*pitch_oracle.GOOD_RATIOS_AT_THE_BOUNDS))
    b = PitchBank(RATIOS)
    assert np.array_equal(m.mix(a, items, N, pitch=b, pitch_ids=ids), want)
    for k, (bad, field) in enumerate(pitch_oracle.bad_pitch_items(len(RATIOS))):
        t = good.copy()
        t[(3 * k) % len(t)] = bad
        for ar in (a, arena):
            with pytest.raises(ValueError, match=rf"pitch item {(3 * k) % len(t)}: {field}\b"):
                m.mix(ar, items, N, pitch=b, pitch_ids=t)
        with pytest.raises(ValueError, match=rf"pitch item {(3 * k) % len(t)}: {field}\b"):
            m.forward_mixed(a, items, N, pitch=b, pitch_ids=t)
    bad_mix = items.copy(); bad_mix[4] = mix_oracle.bad_items(arena.size, N)[0][0]
    with pytest.raises(ValueError, match="mix item 4: fg_len"):
        m.mix(a, bad_mix, N, pitch=b, pitch_ids=ids)
    arena256, items256 = pitch_oracle.clip_table(256)                                             # N <= 256, by name
    with pytest.raises(ValueError, match="N = 256: .*more than 256 samples"):
        m.mix(dev_arena(arena256), items256, 256, pitch=b, pitch_ids=np.zeros(len(items256), np.int32))
    with pytest.raises(ValueError, match="N = 256: "):                                            # ... whatever the ids say
        m.mix(dev_arena(arena256), items256, 256, pitch=b, pitch_ids=np.full(len(items256), -1))
    with pytest.raises(ValueError):                                                               # one without the other; another length
        m.mix(a, items, N, pitch=b)
    with pytest.raises(ValueError):
        m.mix(a, items, N, pitch_ids=ids)
    with pytest.raises(ValueError):
        m.mix(a, items, N, pitch=b, pitch_ids=ids[:-1])
    assert m.mix(a, items[:0], N, pitch=b, pitch_ids=ids[:0]).shape == (0, N)                     # B == 0: nothing to do
    assert np.array_equal(m.mix(a, items, N, pitch=b, pitch_ids=ids), want)
    m.pitch_set_ratios([], [])                                                                    # K = 0 clears them
    with pytest.raises(ValueError, match="no pitch ratios set"):
        m.mix(a, items, N, pitch=_NoBank(), pitch_ids=good)
    assert np.array_equal(m.mix(a, items, N, pitch=b, pitch_ids=ids), want)                       # the bank sets them again
    m.close()


def test_against_the_definitions_golden(model):
    from nanowakeword_amd.augment import PitchBank
    arena, items, ids, ratios, ref, meta = pitch_oracle.load_golden()
    N = meta["N"]
    got = model.mix(dev_arena(arena), items, N, pitch=PitchBank(ratios), pitch_ids=ids)
    assert np.array_equal(got, pitch_oracle.mix_aug(arena, items, ids, ratios, N))
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    print("differing per clip", (d > 0).sum(axis=1), "max", int(d.max()))
    assert [int(x) for x in (d > 0).sum(axis=1)] == meta["restatement_differing_per_clip"] and int(d.max()) == meta["restatement_max_abs_diff"]
    assert np.array_equal(got[ids < 0], ref[ids < 0])
