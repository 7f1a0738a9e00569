"""tests/golden/rir.npz: the reference's route through an impulse response on seeded inputs, for tests/test_rir_host.py and
tests/test_gpu_rir.py.  The contract of nww_mix_rir_* is the float64 definition (tests/rir_oracle.py); this file is a second witness.

Runs only where a checkout of the reference is at hand (--reference, or NWW_REFERENCE); nothing here is needed at test time.  Eight of
tests/golden/mix.npz's items go through the reference's own mixing chain exactly as tools/make_mix_goldens.py takes them (its
``_mix_snr``, the placement without a real background, Gain), then through ApplyImpulseResponse, then through the level / clamp / int16
tail (augment_clips.py:246-259), all in float32 torch on the CPU.

torch_audiomentations, whose ApplyImpulseResponse the reference calls (augment_clips.py:150-157), is NOT installed where this was
written.  Its ``convolve`` is RESTATED here from its documented behaviour - rfft of signal and response at n = N + L - 1, the product,
irfft at n - and ApplyImpulseResponse as that convolution cut to the signal's length (compensate_for_propagation_delay is off in the
reference).  The responses come from tests/rir_oracle.py (golden_irs: integer arithmetic alone), so the file holds the item table, the
response ids, the int16 outputs and, as metadata, how the float64 definition compares with them."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import mix_oracle  # noqa: E402
import rir_oracle  # noqa: E402
from make_mix_goldens import load_mix_snr  # noqa: E402

N = 16000
PICK = (0, 5, 9, 12, 18, 23, 31, 38)         # of mix.npz's 40 items: every foreground length once, one without a background (9)


def convolve(signal, ir):
    """torch_audiomentations.utils.convolution.convolve(mode="full"), restated (see the module's header)"""
    import torch
    n = signal.shape[-1] + ir.shape[-1] - 1
    return torch.fft.irfft(torch.fft.rfft(signal, n=n) * torch.fft.rfft(ir, n=n), n=n)


def reference_clip(mix_snr, arena, it, h, N=N):
    import torch
    fg = torch.from_numpy(arena[int(it["fg_off"]):int(it["fg_off"]) + int(it["fg_len"])].astype(np.float32) / np.float32(32768.0))
    L = int(it["bg_len"])
    has_bg = L > 0
    if has_bg:
        bg = torch.from_numpy(arena[int(it["bg_off"]):int(it["bg_off"]) + L].astype(np.float32) / np.float32(32768.0))
        s0 = int(it["bg_start"])
        if len(bg) < N + s0:
            bg = bg.repeat(int(np.ceil((N + s0) / len(bg))))
        bg = bg[s0:s0 + N]
    else:
        bg = torch.zeros(N)
    if has_bg and bg.abs().max() > 1e-4:
        mixed = mix_snr(fg, bg, int(it["start"]), 20.0 * np.log10(float(it["snr_linear"])))
    else:
        mixed = torch.zeros(N)
        mixed[:len(fg)] = fg
    aug = (mixed * torch.tensor(float(it["gain"]), dtype=torch.float32)).reshape(1, 1, N)            # Gain
    aug = convolve(aug, torch.from_numpy(h).reshape(1, 1, -1))[..., :N]                               # ApplyImpulseResponse
    assert aug.dtype == torch.float32
    level = torch.tensor([float(it["level"])], dtype=torch.float32)
    peaks = torch.max(torch.abs(aug), dim=2, keepdim=True)[0]
    peaks[peaks < 1e-8] = 1.0
    scaled = aug * (level.unsqueeze(1).unsqueeze(2) / peaks)
    final = torch.clamp(scaled, -1.0, 1.0)
    return (final.numpy() * 32767).astype(np.int16).reshape(N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NWW_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "rir.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or NWW_REFERENCE) is needed")
    mix_snr = load_mix_snr(a.reference)
    arena, all_items, _, mix_meta = mix_oracle.load_golden()
    assert mix_meta["N"] == N
    items = all_items[list(PICK)].copy()
    irs = rir_oracle.golden_irs()
    ids = np.arange(len(items), dtype=np.int32)
    ref = np.stack([reference_clip(mix_snr, arena, it, irs[k]) for it, k in zip(items, ids)])
    ours = rir_oracle.definition(arena, items, ids, irs, N)
    d = np.abs(ref.astype(np.int32) - ours.astype(np.int32))
    meta = {"N": N, "items": int(len(items)), "arena_samples": int(arena.size), "arena_sum": int(arena.astype(np.int64).sum()),
            "ir_lengths": [int(h.size) for h in irs], "ir_abs_sums": [float(np.abs(h.astype(np.float64)).sum()) for h in irs],
            "differing_per_clip": [int(x) for x in (d > 0).sum(axis=1)], "samples_per_clip": N, "max_abs_diff": int(d.max()),
            "chain": "augment_clips._mix_snr + Gain + convolve (rfft / irfft at n = N + L - 1, restated) [:N] + the :246-259 tail, float32 torch, CPU"}
    np.savez_compressed(a.out, items=items, ir_ids=ids, ref=ref, meta=np.array(json.dumps(meta)))
    print(json.dumps(meta), os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
