"""The batch frontend's flat items (an item = eight consecutive frames of the whole batch, edge frames handled per S1 trip) against
the library's own per-clip path, bit for bit, and against the oracle (run with -m gpu).

A single-clip call runs the two-frames-per-wave instances with the per-clip item map, which the flat items leave alone: that is the
oracle for bits.  For every case
  * HipModel.frontend of the whole batch equals the same clips pushed through one at a time (array_equal),
  * the batch result meets tests/parity.py's frontend criterion against the oracle,
and, because HipModel.frontend asks for the mels-major layout (never a flat launch) and a launch of fewer than
3 * CUs / ceil(T / 8) clips keeps the two-frames-per-wave map whatever its layout, the frames-major device entry point (what
forward_pcm launches) is driven as well: at the case's own batch size, at the smallest batch that does launch flat items (every wave one
item) and at one of more than two rounds of items per wave (the per-round advance and the next item's prefetch), on clips drawn at random
from the case's batch, against the same one-at-a-time rows.

The C API takes a dense [B][N] batch (no row stride argument), so the rows at an odd element stride are those of an odd clip length, and
the 2-byte path is also entered through a batch whose base pointer is 2 bytes off 4-byte alignment."""
import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_pcm, synth_state_dict
from parity import assert_frontend_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def HipModel():
    from nanowakeword_amd.session import HipModel
    return HipModel


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _clips(B, N, seed):
    """noise, one clip of zeros, one at +-32767"""
    x = synth_pcm("noise", B, N, seed=seed)
    x[1] = 0
    x[2] = np.where(np.random.default_rng(seed).integers(0, 2, N) > 0, 32767, -32767).astype(np.int16)
    return x


def _frames(center, N):
    return 1 + N // 160 if center else 1 + (N - 400) // 160


def _flat_batches(torch, T):
    """(the smallest batch whose frames-major launch uses flat items, a batch of more than two rounds of them).  fe2_launch keeps the
    two-frames-per-wave map while the batch's 8-frame groups fit 3 workgroups x 4 waves per CU four times over, and a launch has at most that
    many waves resident: beyond it every wave walks on to further items (the per-round advance of its clip and frame, the next item's
    first samples requested behind S2) - the benchmark's case.  The library has no entry point that says which map a launch took, and bit
    equality is the property under test, so the sizes restate the launcher's rule; the second one is eight times past it."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 3 * cus // ((T + 7) // 8) + 2, (2 * 12 * cus * 8 + T - 1) // T + 3


def _dev_frontend(torch, m, x, T, n_mels, offset=0):
    """frames-major log-mel [B, T, n_mels] of int16 clips through nww_frontend_dev; offset: int16 elements the batch starts behind a 4-byte
    aligned address"""
    B, N = x.shape
    buf = torch.zeros(B * N + 2, dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 4 == 0
    buf[offset:offset + B * N] = torch.from_numpy(np.ascontiguousarray(x).ravel()).cuda()
    out = torch.full((B, T, n_mels), float("nan"), dtype=torch.float32, device="cuda")
    m.frontend_dev(buf.data_ptr() + 2 * offset, B, N, out.data_ptr(), True, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


CASES = {
    # name: (n_mels, center, B, N, pointer offset)
    "default-17": (64, True, 17, 16000, 0),            # 1717 frames: items straddle clips, the launch's last item is short
    "default-33": (64, True, 33, 16000, 0),            # 3333 frames
    "40-nocenter-17": (40, False, 17, 16000, 0),       # 98 frames, no edge frame at all (the 20-tap instance)
    "odd-stride-17": (64, True, 17, 16001, 0),         # every other row 2 bytes off: the 2-byte path for every frame
    "odd-pointer-17": (64, True, 17, 16000, 1),        # the whole batch 2 bytes off
    "short-T3-40": (64, True, 40, 400, 0),             # T = 3: every frame an edge frame, an item spans three clips
    "short-T8-16": (64, True, 16, 1200, 0),            # T = 8: edge frames at both ends of every item (measured slower flat: the launcher
                                                       # keeps the per-clip map at exactly this length, at every batch size)
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_flat_items_equal_per_clip_path(HipModel, torch, golden_frontend, case):
    n_mels, center, B, N, offset = CASES[case]
    g = golden_frontend
    fb = g["fb64"] if n_mels == 64 else g["fb40"]
    T = _frames(center, N)
    cfg = HeadConfig("dnn", (T, n_mels))
    m = HipModel(cfg, FrontendConfig(n_mels=n_mels, center=center), state_dict=synth_state_dict(cfg), window=g["window"], mel_fb=fb)
    assert m.num_frames(N) == T
    x = _clips(B, N, seed=5)
    one = np.concatenate([m.frontend(x[i:i + 1]) for i in range(B)])             # [B, n_mels, T], the per-clip path
    assert np.isfinite(one).all() and np.ptp(one[0]) > 0.0
    db, mel = m.frontend(x, return_power=True)
    assert np.array_equal(db, one), (case, int((db != one).sum()))
    mo = oracle.mel_power(x, g["window"], fb, center=center)
    e_db, e_mel, _ = assert_frontend_close(mel, db, mo, oracle.logmel_db(mo), case)
    print(f"{case}: max dB err {e_db:.2e}, mel err {e_mel:.2e} x frame peak")
    # the frames-major device path at the case's batch size ...
    rows = np.ascontiguousarray(one.transpose(0, 2, 1))                         # [B, T, n_mels]
    dv = _dev_frontend(torch, m, x, T, n_mels, offset)
    assert np.array_equal(dv, rows), (case, "frames-major", int((dv != rows).sum()))
    # ... and where the launch takes flat items, one item per wave and more than two rounds of items: clips of the case's batch in random order
    for Bf in _flat_batches(torch, T):
        pick = np.random.default_rng(9 + Bf).integers(0, B, Bf)
        pick[:3] = (0, 1, 2)
        dv = _dev_frontend(torch, m, x[pick], T, n_mels, offset)
        bad = np.argwhere((dv != rows[pick]).any(axis=2))
        assert bad.size == 0, (case, "flat", Bf, len(bad), bad[:8].tolist())
    m.close()


def test_cnn_forward_pcm_batch_equals_single_clips(HipModel, torch, golden_frontend):
    g = golden_frontend
    cfg = HeadConfig("cnn", (101, 64))
    m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg), window=g["window"], mel_fb=g["fb64"])
    x = _clips(17, 16000, seed=6)
    one = [m.forward_pcm(x[i:i + 1]) for i in range(17)]
    l1, p1 = np.concatenate([o[0] for o in one]), np.concatenate([o[1] for o in one])
    assert np.isfinite(l1).all() and np.ptp(l1) > 0.0
    lg, pr = m.forward_pcm(x)
    assert np.array_equal(lg, l1) and np.array_equal(pr, p1), int((lg != l1).sum())
    # batches whose frontend launch takes flat items: one item per wave, and more than two rounds
    for Bf in _flat_batches(torch, 101):
        pick = np.random.default_rng(10 + Bf).integers(0, 17, Bf)
        lg, pr = m.forward_pcm(x[pick])
        assert np.array_equal(lg, l1[pick]) and np.array_equal(pr, p1[pick]), (Bf, int((lg != l1[pick]).sum()))
    m.close()
