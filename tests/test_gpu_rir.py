"""Clips through room impulse responses (nww_mix_rir_*, csrc/rir.hip) on the GPU: the edge cases of every transform size against the
float32 restatement of tests/rir_oracle.py bit for bit at B = 1 and 3, batch invariance, rows without a response against nww_mix, the
reference route's golden (tests/golden/rir.npz), the forward / frontend forms against the calls they compose, nww_rir_prepare_dev on
several responses against one at a time (and against the restatement), the table slots on a stream of the caller's, and the validation."""
import numpy as np
import pytest

import mix_oracle
import rir_oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig, raw_frontend_frames
from nanowakeword_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

_CASES = {}
_SPEECH = {}


def cases(M):
    """rir_oracle.edge_cases(M) with their clips by the restatement: computed once per transform size"""
    if M not in _CASES:
        _CASES[M] = [(name, N, irs, arena, items, ids, rir_oracle.mix_rir(arena, items, ids, irs, N, M))
                     for name, N, irs, arena, items, ids in rir_oracle.edge_cases(M)]
    return _CASES[M]


def speech(N=16000):
    """(arena, 12 items, ids, irs, their clips by the restatement) at clips of one second, M = 32768: rows of mix's edge table against
    decaying responses of 800 / 4000 / 16 000 taps, every third row without one"""
    if N not in _SPEECH:
        arena, items = mix_oracle.edge_table(N)
        t = mix_oracle.table_of(items, 65)[-12:].copy()
        rng = np.random.default_rng(77)
        irs = [rir_oracle.decaying(rng, L) for L in (800, 4000, 16000)]
        ids = (np.arange(12) % 4 - 1).astype(np.int32)
        _SPEECH[N] = (arena, t, ids, irs, rir_oracle.mix_rir(arena, t, ids, irs, N, 32768))
    return _SPEECH[N]


@pytest.fixture(scope="module")
def model():
    from nanowakeword_amd.session import HipModel
    cfg = HeadConfig("cnn", (101, 64))
    m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))
    yield m
    m.close()


def dev_arena(arena):
    from nanowakeword_amd.augment import ClipArena
    return ClipArena([arena])


def ir_arena(irs, N, M=None):
    from nanowakeword_amd.augment import IrArena
    return IrArena(irs, N, M=M)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("M", rir_oracle.SIZES)
def test_edge_cases_equal_restatement(model, M, B):
    for name, N, irs, arena, items, ids, want in cases(M):
        a, ia = dev_arena(arena), ir_arena(irs, N, M)
        assert ia.M == M
        if name != "one":
            assert ir_arena(irs, N).M == M, name                           # the case was made for this instance
        for lo in range(0, len(items) - B + 1, B):
            got = model.mix(a, items[lo:lo + B], N, irs=ia, ir_ids=ids[lo:lo + B])
            assert got.shape == (B, N) and got.dtype == np.int16
            assert np.array_equal(got, want[lo:lo + B]), (name, lo, np.argwhere(got != want[lo:lo + B])[:5])
        if B == 3:                                                          # the table's last rows, and the host-pointer call
            assert np.array_equal(model.mix(a, items[-3:], N, irs=ia, ir_ids=ids[-3:]), want[-3:]), name
            assert np.array_equal(model.mix(arena, items[-3:], N, irs=ia, ir_ids=ids[-3:]), want[-3:]), name


def test_batch_invariance_and_rows_without_a_response(model):
    M = 8192
    name, N, irs, arena, items, ids, want = cases(M)[1]
    a, ia = dev_arena(arena), ir_arena(irs, N)
    assert np.array_equal(model.mix(a, items, N, irs=ia, ir_ids=ids), want)
    assert np.array_equal(model.mix(a, items[::-1].copy(), N, irs=ia, ir_ids=ids[::-1].copy()), want[::-1])
    rep = np.concatenate([items] * 5)
    assert np.array_equal(model.mix(a, rep, N, irs=ia, ir_ids=np.tile(ids, 5)), np.concatenate([want] * 5))
    # ir_id == -1 is nww_mix's clip, and a call without ids is nww_mix itself
    none = ids < 0
    plain = model.mix(a, items, N)
    assert none.any() and np.array_equal(want[none], plain[none])
    assert np.array_equal(model.mix(a, items, N, irs=ia, ir_ids=np.full(len(items), -1)), plain)
    assert np.array_equal(plain, mix_oracle.mix(arena, items, N))


def test_against_reference_golden(model):
    arena, items, ids, irs, ref, meta = rir_oracle.load_golden()
    N = meta["N"]
    ia = ir_arena(irs, N)
    assert ia.M == 32768
    got = model.mix(dev_arena(arena), items, N, irs=ia, ir_ids=ids)
    rir_oracle.conditions(got, ref, "golden")
    assert np.array_equal(got, rir_oracle.mix_rir(arena, items, ids, irs, N, 32768))


def test_forward_mixed_is_forward_pcm_of_mix(model):
    N = 16000
    arena, t, ids, irs, want = speech(N)
    a, ia = dev_arena(arena), ir_arena(irs, N)
    clips = model.mix(a, t, N, irs=ia, ir_ids=ids)
    assert np.array_equal(clips, want)
    lg, pr = model.forward_mixed(a, t, N, irs=ia, ir_ids=ids)
    lg0, pr0 = model.forward_pcm(clips)
    assert np.isfinite(lg).all() and np.array_equal(lg, lg0) and np.array_equal(pr, pr0)
    assert np.unique(lg).size > 1
    assert not np.array_equal(lg, model.forward_mixed(a, t, N)[0])           # the responses are heard
    from nanowakeword_amd.session import HipSession
    s = HipSession(model, mode="e2e", clip_samples=N)
    assert np.array_equal(s.mix(a, t, irs=ia, ir_ids=ids), clips)
    assert np.array_equal(s.forward_mixed(a, t, irs=ia, ir_ids=ids)[0], pr0.reshape(-1, 1, 1))


@pytest.mark.parametrize("n", [16, 17])
def test_forward_mixed_raw_pcm_head(n):
    from nanowakeword_amd.session import HipModel
    probe = HeadConfig("e2e_quartznet", (1, 128), e2e_frontend_channels=32)
    cfg = HeadConfig("e2e_quartznet", (raw_frontend_frames(probe, n), 128), e2e_frontend_channels=32)
    m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))
    arena, items = mix_oracle.edge_table(n)
    t = mix_oracle.table_of(items, 33)
    rng = np.random.default_rng(n)
    irs = [rir_oracle.decaying(rng, 9), np.array([0.0, 0.0, 0.7], np.float32)]
    ids = (np.arange(33) % 3 - 1).astype(np.int32)
    a, ia = dev_arena(arena), ir_arena(irs, n)
    clips = m.mix(a, t, n, irs=ia, ir_ids=ids)
    assert np.array_equal(clips, rir_oracle.mix_rir(arena, t, ids, irs, n, 2048))
    lg, pr = m.forward_mixed(a, t, n, irs=ia, ir_ids=ids)
    lg0, pr0 = m.forward_pcm(clips)
    assert np.isfinite(lg).all() and np.array_equal(lg, lg0) and np.array_equal(pr, pr0)
    m.close()


def test_embed_mixed_is_embed_clips_of_mix(tmp_path):
    from nanowakeword_amd.augment import MixedClips, mixed_feature_batches
    from nanowakeword_amd.features import HipFeatures, generate_features
    N = 16000
    arena, t, ids, irs, want = speech(N)
    a, ia = dev_arena(arena), ir_arena(irs, N)
    f = HipFeatures()
    clips = f.mix(a, t, N, irs=ia, ir_ids=ids)
    assert np.array_equal(clips, want)
    got = f.embed_mixed(a, t, N, irs=ia, ir_ids=ids)
    assert got.shape == (12, 101, 64) and np.array_equal(got, f.embed_clips(clips, batch_size=12))
    path = str(tmp_path / "feats.npy")
    rows = generate_features(mixed_feature_batches(t, 5, irs=ia, ir_ids=ids), 12, path, MixedClips(f, a, N, irs=ia), 1.0)
    assert rows == 12 and np.array_equal(np.load(path), got)
    f.close()


def test_prepare_several_equals_one_at_a_time(model):
    """K = 3 responses of different lengths in one call against three calls of one - and both against the restatement's spectra"""
    import torch
    for M, N in ((2048, 1000), (32768, 16000)):
        rng = np.random.default_rng(M)
        irs = [rir_oracle.decaying(rng, L) for L in (1, 333, 2 * N)]
        assert rir_oracle.fft_size(N, 333) == M
        host = np.concatenate(irs)
        lens = np.array([h.size for h in irs], np.int32)
        offs = np.concatenate(([0], np.cumsum(lens.astype(np.int64))[:-1]))
        d = torch.from_numpy(host).cuda()
        together = torch.zeros((3, M), dtype=torch.float32, device="cuda")
        model.rir_prepare_dev(d.data_ptr(), offs, lens, N, M, together.data_ptr())
        apart = torch.zeros((3, M), dtype=torch.float32, device="cuda")
        for k in (2, 0, 1):
            model.rir_prepare_dev(d.data_ptr(), offs[k:k + 1], lens[k:k + 1], N, M, apart[k].data_ptr())
        torch.cuda.synchronize()
        got = together.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), apart.cpu().numpy().view(np.uint32))
        for k, h in enumerate(irs):
            sr, si = rir_oracle.prepare(h, N, M)
            assert np.array_equal(got[k, 0::2], sr) and np.array_equal(got[k, 1::2], si), (M, k)


def test_table_slots_wrap_on_a_stream(model):
    """six calls back to back on a stream of the caller's, one synchronise: more calls than slots, both tables different every time"""
    import torch
    name, N, irs, arena, items, ids, want = cases(2048)[1]
    a, ia = dev_arena(arena), ir_arena(irs, N)
    rep, rid, wrep = np.concatenate([items] * 3), np.tile(ids, 3), np.concatenate([want] * 3)
    model.mix(a, rep, N, irs=ia, ir_ids=rid)                               # the slots exist and hold the largest table: nothing below waits
    st = torch.cuda.Stream()
    n = len(rep)
    picks = [slice(0, 5), slice(0, n), slice(7, 9), slice(3, 20), slice(n - 1, n), slice(10, 25)]
    outs = [torch.zeros(((p.stop - p.start) * N + 1,), dtype=torch.int16, device="cuda") for p in picks]
    for k, (p, o) in enumerate(zip(picks, outs)):
        model.mix_dev(a.ptr, a.samples, rep[p], N, o.data_ptr() + 2 * (k % 2), stream=st.cuda_stream, irs=ia, ir_ids=rid[p])
    st.synchronize()
    for k, (p, o) in enumerate(zip(picks, outs)):
        got = o.cpu().numpy()[k % 2:][:(p.stop - p.start) * N].reshape(-1, N)
        assert np.array_equal(got, wrep[p]), k


def test_bad_items_raise_and_leave_the_next_call_alone(model):
    from nanowakeword_amd.augment import IrArena
    name, N, irs, arena, items, ids, want = cases(2048)[0]
    a, ia = dev_arena(arena), ir_arena(irs, N)
    good = rir_oracle.rir_items(ids)
    for k, (bad, field) in enumerate(rir_oracle.bad_rir_items(len(irs))):
        t = good.copy()
        t[(3 * k) % len(t)] = bad
        for ar in (a, arena):
            with pytest.raises(ValueError, match=rf"rir item {(3 * k) % len(t)}: {field}\b"):
                model.mix(ar, items, N, irs=ia, ir_ids=t)
        with pytest.raises(ValueError, match=rf"rir item {(3 * k) % len(t)}: {field}\b"):
            model.forward_mixed(a, items, N, irs=ia, ir_ids=t)
    bad_mix = items.copy(); bad_mix[4] = mix_oracle.bad_items(arena.size, N)[0][0]
    with pytest.raises(ValueError, match="mix item 4: fg_len"):
        model.mix(a, bad_mix, N, irs=ia, ir_ids=ids)
    with pytest.raises(ValueError):                                        # one without the other; ids of another length; another N
        model.mix(a, items, N, irs=ia)
    with pytest.raises(ValueError):
        model.mix(a, items, N, ir_ids=ids)
    with pytest.raises(ValueError):
        model.mix(a, items, N, irs=ia, ir_ids=ids[:-1])
    with pytest.raises(ValueError, match="prepared for clips"):
        model.mix(a, items, N - 1, irs=ia, ir_ids=ids)
    with pytest.raises(ValueError, match="overlap-save not built"):
        IrArena([np.ones(12770, np.float32)], 20000)
    with pytest.raises(ValueError, match="response 1: .*overlap-save not built"):     # the C-ABI's own check
        model.rir_prepare_dev(a.ptr, np.zeros(2, np.int64), np.array([5, 12770], np.int32), 20000, 32768, a.ptr)
    with pytest.raises(ValueError, match="not a transform size"):
        model.rir_prepare_dev(a.ptr, np.zeros(1, np.int64), np.array([5], np.int32), N, 4096, a.ptr)
    assert model.mix(a, items[:0], N, irs=ia, ir_ids=ids[:0]).shape == (0, N)         # B == 0: nothing to do
    assert np.array_equal(model.mix(a, items, N, irs=ia, ir_ids=ids), want)
