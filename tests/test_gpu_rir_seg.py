"""The segmented route of nww_mix_rir_* (M = NWW_RIR_SEGMENTED; csrc/rir.hip's rir_seg_* kernels) on the GPU: the edge cases of
tests/rir_seg_oracle.py against its float32 restatement bit for bit, with device and host arenas; rows without a response against
nww_mix; batch invariance; the forward / frontend forms against the calls they compose at clips of 2 s; the reference route's golden
(tests/golden/rir_seg.npz); and the validation."""
import numpy as np
import pytest

import mix_oracle
import rir_oracle
import rir_seg_oracle as seg
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

_CASES = []
_SPEECH = {}


def cases():
    """seg.edge_cases_seg() with their clips by the restatement: computed once"""
    if not _CASES:
        _CASES.extend((name, N, irs, arena, items, ids, seg.mix_rir(arena, items, ids, irs, N))
                      for name, N, irs, arena, items, ids in seg.edge_cases_seg())
    return _CASES


def speech(N=32000):
    """(arena, 12 items, ids, irs, their clips by the restatement) at clips of two seconds: rows of mix's edge table against decaying
    responses of 800 / 16 000 / 32 000 taps (one and two partitions), every fourth row without one"""
    if N not in _SPEECH:
        arena, items = mix_oracle.edge_table(N)
        t = mix_oracle.table_of(items, 65)[-12:].copy()
        rng = np.random.default_rng(78)
        irs = [rir_oracle.decaying(rng, L) for L in (800, 16000, 32000)]
        ids = (np.arange(12) % 4 - 1).astype(np.int32)
        _SPEECH[N] = (arena, t, ids, irs, seg.mix_rir(arena, t, ids, irs, N))
    return _SPEECH[N]


@pytest.fixture(scope="module")
def model():
    from nanowakeword_amd.session import HipModel
    cfg = HeadConfig("cnn", (201, 64), embedding_dim=16)
    m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))
    yield m
    m.close()


def dev_arena(arena):
    from nanowakeword_amd.augment import ClipArena
    return ClipArena([arena])


def seg_arena(irs, N):
    """an IrArena on the segmented route - asked for by name where a transform size would hold the clips (N <= 16384)"""
    from nanowakeword_amd.augment import RIR_SEGMENTED, IrArena
    ia = IrArena(irs, N, segmented=True, M=RIR_SEGMENTED)
    assert ia.M == RIR_SEGMENTED and ia.parts == seg.parts(N, max(h.size for h in irs))
    return ia


def test_edge_cases_equal_restatement(model):
    from nanowakeword_amd.augment import RIR_SEGMENTED, IrArena
    for name, N, irs, arena, items, ids, want in cases():
        a, ia = dev_arena(arena), seg_arena(irs, N)
        auto = IrArena(irs, N, segmented=True)                             # the route is chosen by the lengths alone
        assert (auto.M == RIR_SEGMENTED) == (rir_oracle.fft_size(N, max(h.size for h in irs)) == 0), name
        got = model.mix(a, items, N, irs=ia, ir_ids=ids)
        assert got.shape == (len(items), N) and got.dtype == np.int16
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        assert np.array_equal(model.mix(arena, items, N, irs=ia, ir_ids=ids), want), name                  # the host-pointer call
        assert np.array_equal(model.mix(a, items[-1:], N, irs=ia, ir_ids=ids[-1:]), want[-1:]), name       # B = 1
        if auto.M == RIR_SEGMENTED:
            assert np.array_equal(model.mix(a, items, N, irs=auto, ir_ids=ids), want), name
        else:                                                              # short clips keep the one-workgroup route and its bits
            assert np.array_equal(model.mix(a, items, N, irs=auto, ir_ids=ids), rir_oracle.mix_rir(arena, items, ids, irs, N, auto.M)), name


def test_rows_without_a_response_are_nww_mix(model):
    name, N, irs, arena, items, ids, want = cases()[5]
    assert name == "refused" and N == 20000
    a, ia = dev_arena(arena), seg_arena(irs, N)
    plain = model.mix(a, items, N)
    none = ids < 0
    assert none.any() and np.array_equal(want[none], plain[none])
    assert np.array_equal(model.mix(a, items, N, irs=ia, ir_ids=np.full(len(items), -1)), plain)
    assert np.array_equal(plain, mix_oracle.mix(arena, items, N))
    full_arena, full_items = mix_oracle.edge_table(N)                       # every row of the edge table, none with a response
    fa = dev_arena(full_arena)
    assert np.array_equal(model.mix(fa, full_items, N, irs=ia, ir_ids=np.full(len(full_items), -1)), model.mix(fa, full_items, N))


def test_batch_invariance(model):
    """twelve clips at B = 12, one by one, in reverse, and scattered through a table of 300: the same bits"""
    N = 32000
    arena, t, ids, irs, want = speech(N)
    a, ia = dev_arena(arena), seg_arena(irs, N)
    assert np.array_equal(model.mix(a, t, N, irs=ia, ir_ids=ids), want)
    for i in range(12):
        assert np.array_equal(model.mix(a, t[i:i + 1], N, irs=ia, ir_ids=ids[i:i + 1]), want[i:i + 1]), i
    assert np.array_equal(model.mix(a, t[::-1].copy(), N, irs=ia, ir_ids=ids[::-1].copy()), want[::-1])
    _, items = mix_oracle.edge_table(N)
    big = mix_oracle.table_of(items, 300)
    big_ids = ((np.arange(300) * 7) % 4 - 1).astype(np.int32)
    where = np.array([0, 3, 31, 64, 65, 127, 128, 199, 255, 256, 298, 299])
    big[where], big_ids[where] = t, ids
    got = model.mix(a, big, N, irs=ia, ir_ids=big_ids)
    assert np.array_equal(got[where], want)


def test_forward_mixed_is_forward_pcm_of_mix(model):
    N = 32000
    arena, t, ids, irs, want = speech(N)
    a, ia = dev_arena(arena), seg_arena(irs, N)
    clips = model.mix(a, t, N, irs=ia, ir_ids=ids)
    assert np.array_equal(clips, want)
    lg, pr = model.forward_mixed(a, t, N, irs=ia, ir_ids=ids)
    lg0, pr0 = model.forward_pcm(clips)
    assert np.isfinite(lg).all() and np.array_equal(lg, lg0) and np.array_equal(pr, pr0)
    assert np.unique(lg).size > 1
    assert not np.array_equal(lg, model.forward_mixed(a, t, N)[0])           # the responses are heard


def test_embed_mixed_is_embed_clips_of_mix(tmp_path):
    from nanowakeword_amd.augment import MixedClips, mixed_feature_batches
    from nanowakeword_amd.features import HipFeatures, generate_features
    N = 32000
    arena, t, ids, irs, want = speech(N)
    a, ia = dev_arena(arena), seg_arena(irs, N)
    f = HipFeatures()
    clips = f.mix(a, t, N, irs=ia, ir_ids=ids)
    assert np.array_equal(clips, want)
    got = f.embed_mixed(a, t, N, irs=ia, ir_ids=ids)
    assert got.shape == (12, 201, 64) and np.array_equal(got, f.embed_clips(clips, batch_size=12))
    path = str(tmp_path / "feats.npy")
    rows = generate_features(mixed_feature_batches(t, 5, irs=ia, ir_ids=ids), 12, path, MixedClips(f, a, N, irs=ia), 2.0)
    assert rows == 12 and np.array_equal(np.load(path), got)
    f.close()


def test_against_reference_golden(model):
    from nanowakeword_amd.augment import RIR_SEGMENTED, IrArena
    arena, items, ids, irs, ref, meta = seg.load_golden()
    N = meta["N"]
    ia = IrArena(irs, N, segmented=True)
    assert ia.M == RIR_SEGMENTED and ia.parts == 2
    got = model.mix(dev_arena(arena), items, N, irs=ia, ir_ids=ids)
    rir_oracle.conditions(got, ref, "golden")
    assert np.array_equal(got, seg.mix_rir(arena, items, ids, irs, N))


def test_bad_items_raise_and_leave_the_next_call_alone(model):
    from nanowakeword_amd.augment import RIR_SEGMENTED
    name, N, irs, arena, items, ids, want = cases()[5]
    a, ia = dev_arena(arena), seg_arena(irs, N)
    good = rir_oracle.rir_items(ids)
    for k, (bad, field) in enumerate(rir_oracle.bad_rir_items(len(irs))):
        t = good.copy()
        t[(3 * k) % len(t)] = bad
        for ar in (a, arena):
            with pytest.raises(ValueError, match=rf"rir item {(3 * k) % len(t)}: {field}\b"):
                model.mix(ar, items, N, irs=ia, ir_ids=t)
        with pytest.raises(ValueError, match=rf"rir item {(3 * k) % len(t)}: {field}\b"):
            model.forward_mixed(a, items, N, irs=ia, ir_ids=t)
    for k, (bad, field) in enumerate(mix_oracle.bad_items(arena.size, N)):
        bad_mix = items.copy(); bad_mix[k % len(items)] = bad
        with pytest.raises(ValueError, match=rf"mix item {k % len(items)}: {field}\b"):
            model.mix(a, bad_mix, N, irs=ia, ir_ids=ids)
    with pytest.raises(ValueError, match="prepared for clips"):
        model.mix(a, items, N - 1, irs=ia, ir_ids=ids)
    with pytest.raises(ValueError, match="response 1: ir_len out of range"):          # the C-ABI's own checks on this route
        model.rir_prepare_dev(a.ptr, np.zeros(2, np.int64), np.array([5, 0], np.int32), N, RIR_SEGMENTED, a.ptr)
    with pytest.raises(ValueError, match="response 0: ir_off out of range"):
        model.rir_prepare_dev(a.ptr, np.array([-1], np.int64), np.array([5], np.int32), N, RIR_SEGMENTED, a.ptr)
    with pytest.raises(ValueError, match="not a transform size"):                      # no other negative M is a route
        model.rir_prepare_dev(a.ptr, np.zeros(1, np.int64), np.array([5], np.int32), N, -2, a.ptr)
    with pytest.raises(ValueError, match="response 0: .*overlap-save not built"):     # the other route refuses as before
        model.rir_prepare_dev(a.ptr, np.zeros(1, np.int64), np.array([12770], np.int32), N, 32768, a.ptr)
    assert model.lib.nww_rir_parts(N, 12770) == 1 and model.lib.nww_rir_parts(32000, 32000) == 2 and model.lib.nww_rir_parts(0, 5) == 0
    assert model.lib.nww_rir_spectra_floats(3, N, 40000, RIR_SEGMENTED) == seg.spectra_floats(3, N, 40000, -1)
    assert model.lib.nww_rir_spectra_floats(3, N, 5, 8192) == 3 * 8192 and model.lib.nww_rir_spectra_floats(3, N, 5, 4096) == 0
    assert model.mix(a, items[:0], N, irs=ia, ir_ids=ids[:0]).shape == (0, N)         # B == 0: nothing to do
    assert np.array_equal(model.mix(a, items, N, irs=ia, ir_ids=ids), want)
