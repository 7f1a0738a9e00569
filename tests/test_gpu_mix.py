"""Clips mixed on the device (nww_mix_*, csrc/mix.hip) on the GPU: the edge table at every clip length and batch size against the numpy
restatement bit for bit, batch invariance, the reference's own chain (tests/golden/mix.npz), the forward / frontend forms against the
calls they compose, the table slots on a stream of the caller's, and the validation."""
import numpy as np
import pytest

import mix_oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig, raw_frontend_frames
from nanowakeword_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

EDGE_N = (1, 8, 250, 1001, 16000)
_EDGE = {}


def edge(N):
    """(arena, 65 items, their clips by the restatement): computed once per clip length"""
    if N not in _EDGE:
        arena, items = mix_oracle.edge_table(N)
        t = mix_oracle.table_of(items, 65)
        _EDGE[N] = (arena, t, mix_oracle.mix(arena, t, N))
    return _EDGE[N]


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


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("N", EDGE_N)
def test_edge_table_equals_restatement(model, N, B):
    arena, t, want = edge(N)
    t, want = t[-B:], want[-B:]                    # the table's special rows come last
    got = model.mix(dev_arena(arena), t, N)
    assert got.shape == (B, N) and got.dtype == np.int16
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if B == 3:                                     # the host-pointer call, and a table's first rows
        assert np.array_equal(model.mix(arena, t, N), want)
        assert np.array_equal(model.mix(arena, edge(N)[1][:3], N), edge(N)[2][:3])


def test_batch_invariance(model):
    N = 1001
    arena, t, want = edge(N)
    a = dev_arena(arena)
    assert np.array_equal(model.mix(a, t, N), want)
    assert np.array_equal(model.mix(a, t[::-1].copy(), N), want[::-1])
    for i in range(len(t)):
        assert np.array_equal(model.mix(a, t[i:i + 1], N)[0], want[i]), i


def test_against_reference_golden(model):
    arena, items, ref, meta = mix_oracle.load_golden()
    got = model.mix(dev_arena(arena), items, meta["N"])
    mix_oracle.golden_conditions(got, ref)
    assert np.array_equal(got, mix_oracle.mix(arena, items, meta["N"]))


def test_forward_mixed_is_forward_pcm_of_mix(model):
    N, B = 16000, 33
    arena, t, want = edge(N)
    a = dev_arena(arena)
    clips = model.mix(a, t[:B], N)
    assert np.array_equal(clips, want[:B])
    lg, pr = model.forward_mixed(a, t[:B], N)
    lg0, pr0 = model.forward_pcm(clips)
    assert np.isfinite(lg).all() and np.array_equal(lg, lg0) and np.array_equal(pr, pr0)
    assert np.unique(lg).size > 1                       # the clips differ, and so do their scores
    from nanowakeword_amd.session import HipSession
    s = HipSession(model, mode="e2e", clip_samples=N)
    assert np.array_equal(s.mix(a, t[:B]), clips) and np.array_equal(s.forward_mixed(a, t[:B])[0], pr0.reshape(-1, 1, 1))


@pytest.mark.parametrize("n", [16, 17])
def test_forward_mixed_raw_pcm_head(n):
    from nanowakeword_amd.session import HipModel
    probe = HeadConfig("e2e_quartznet", (1, 128), e2e_frontend_channels=32)
    cfg = HeadConfig("e2e_quartznet", (raw_frontend_frames(probe, n), 128), e2e_frontend_channels=32)
    m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))
    arena, items = mix_oracle.edge_table(n)
    t = mix_oracle.table_of(items, 33)
    a = dev_arena(arena)
    clips = m.mix(a, t, n)
    assert np.array_equal(clips, mix_oracle.mix(arena, t, n))
    lg, pr = m.forward_mixed(a, t, n)
    lg0, pr0 = m.forward_pcm(clips)
    assert np.isfinite(lg).all() and np.array_equal(lg, lg0) and np.array_equal(pr, pr0)
    m.close()


def test_embed_mixed_is_embed_clips_of_mix(tmp_path):
    from nanowakeword_amd.augment import MixedClips, mixed_feature_batches
    from nanowakeword_amd.features import HipFeatures, generate_features
    N = 16000
    arena, t, want = edge(N)
    a = dev_arena(arena)
    f = HipFeatures()
    clips = f.mix(a, t[:20], N)
    assert np.array_equal(clips, want[:20])
    got = f.embed_mixed(a, t[:20], N)
    assert got.shape == (20, 101, 64) and np.array_equal(got, f.embed_clips(clips, batch_size=20))
    # the feature job on tables instead of audio
    path = str(tmp_path / "feats.npy")
    rows = generate_features(mixed_feature_batches(t[:20], 8), 20, path, MixedClips(f, a, N), 1.0)
    assert rows == 20 and np.array_equal(np.load(path), got)
    f.close()


def test_table_slots_wrap_on_a_stream(model):
    """six calls back to back on a stream of the caller's, one synchronise: more calls than slots, every table different"""
    import torch
    N = 250
    arena, t, want = edge(N)
    a = dev_arena(arena)
    model.mix(a, t, N)                                  # the slots exist and hold 65 items: nothing below waits for the device
    st = torch.cuda.Stream()
    picks = [slice(0, 5), slice(0, 65), slice(30, 33), slice(7, 24), slice(64, 65), slice(20, 60)]
    outs = [torch.zeros(((p.stop - p.start) * N + 1,), dtype=torch.int16, device="cuda") for p in picks]
    for k, (p, o) in enumerate(zip(picks, outs)):
        model.mix_dev(a.ptr, a.samples, t[p], N, o.data_ptr() + 2 * (k % 2), stream=st.cuda_stream)       # every other output at an odd sample
    st.synchronize()
    for k, (p, o) in enumerate(zip(picks, outs)):
        got = o.cpu().numpy()[k % 2:][:(p.stop - p.start) * N].reshape(-1, N)
        assert np.array_equal(got, want[p]), k


def test_bad_items_raise_and_leave_the_next_call_alone(model):
    N = 250
    arena, t, want = edge(N)
    a = dev_arena(arena)
    for k, (bad, field) in enumerate(mix_oracle.bad_items(arena.size, N)):
        tb = t[:12].copy()
        tb[(5 * k) % 12] = bad
        with pytest.raises(ValueError, match=rf"mix item {(5 * k) % 12}: {field}\b"):
            model.mix(a, tb, N)
        with pytest.raises(ValueError, match=rf"mix item {(5 * k) % 12}: {field}\b"):
            model.mix(arena, tb, N)
    with pytest.raises(ValueError, match="mix item 0: fg_len"):
        model.forward_mixed(a, t[13:17], 100)           # items of another clip length: foregrounds of 250 samples
    assert model.mix(a, t[:0], N).shape == (0, N)       # B == 0: nothing to do
    with pytest.raises(ValueError):
        model.mix(a, t[:3], 0)
    with pytest.raises(ValueError, match="MIX_ITEM"):
        model.mix(a, np.zeros(3, np.float32), N)
    assert np.array_equal(model.mix(a, t, N), want)


def test_offsets_and_output_past_2_31(model):
    """an arena whose clips lie beyond sample 2^31 and a batch whose output does: the kernel's offsets are 64-bit where they must be"""
    import torch
    N = 16000
    arena, t, want = edge(N)
    off = 2 ** 31 + 1
    B = 2 ** 31 // N + 14                               # the last 13 clips start past element 2^31 of the output
    big = torch.zeros(off + arena.size, dtype=torch.int16, device="cuda")
    big[off:] = torch.from_numpy(arena).cuda()
    tb = mix_oracle.table_of(t[:32], B)                 # the edge table's own rows, over and over at other SNRs and levels
    rows = np.r_[0, 1, B - 15:B]
    expect = mix_oracle.mix(arena, tb[rows], N)
    tb["fg_off"] += off
    tb["bg_off"] += off
    out = torch.empty(B * N, dtype=torch.int16, device="cuda")
    model.mix_dev(big.data_ptr(), big.numel(), tb, N, out.data_ptr())
    torch.cuda.synchronize()
    assert (B - 13) * N > 2 ** 31
    got = out.view(B, N)[torch.from_numpy(rows).cuda()].cpu().numpy()
    assert np.array_equal(got, expect)
    del out, big
    torch.cuda.empty_cache()
