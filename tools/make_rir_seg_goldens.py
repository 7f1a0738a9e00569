"""tests/golden/rir_seg.npz: the reference's route through an impulse response at the reference's own clip length (2 s), for
tests/test_rir_seg_host.py and tests/test_gpu_rir_seg.py.  The contract of nww_mix_rir_* is the float64 definition
(tests/rir_oracle.py); this file is a second witness for the segmented route, as tests/golden/rir.npz is for the one-workgroup route.

Runs only where a checkout of the reference is at hand (--reference, or NWW_REFERENCE); nothing here is needed at test time.  Four items
over mix_oracle.golden_arena() at N = 32000 - one without a background, one over a tiled 53-sample background, one over a cropped long
background, one over a background that wraps once - go through tools/make_rir_goldens.py's chain (``reference_clip``: the reference's
``_mix_snr``, Gain, the restated convolve at n = N + L - 1, the level / clamp / int16 tail; float32 torch on the CPU) against
rir_oracle.golden_irs()' responses of 8000 / 12001 / 16000 / 20000 taps.  The file holds the item table, the response ids, the int16
outputs and, as metadata, how the float64 definition compares with them."""
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
import rir_seg_oracle  # noqa: E402
from make_mix_goldens import load_mix_snr  # noqa: E402
from make_rir_goldens import reference_clip  # noqa: E402

N = 32000


def golden_items(offs, lens):
    nf = len(mix_oracle.GOLDEN_FG)
    db = lambda x: 10.0 ** (x / 20.0)
    fg = lambda k: dict(fg_off=int(offs[k]), fg_len=int(lens[k]))
    bg = lambda k: dict(bg_off=int(offs[nf + k]), bg_len=int(lens[nf + k]))
    return np.concatenate([
        mix_oracle.item(**fg(6), gain=db(1.5), level=0.9),                                                      # no background
        mix_oracle.item(**fg(7), **bg(0), bg_start=17, start=5000, snr=db(12.0), gain=db(-2.0), level=0.75),    # 53 samples, tiled
        mix_oracle.item(**fg(4), **bg(5), bg_start=9000, start=20000, snr=db(20.0), gain=db(0.5), level=0.6),   # 48000, cropped
        mix_oracle.item(**fg(3), **bg(4), bg_start=123, start=26999, snr=db(7.0), gain=db(3.0), level=1.0),     # 30001, wraps once
    ])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NWW_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "rir_seg.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or NWW_REFERENCE) is needed")
    mix_snr = load_mix_snr(a.reference)
    arena, offs, lens = mix_oracle.golden_arena()
    items = golden_items(offs, lens)
    for it in items:
        assert mix_oracle.bad_field(it, arena.size, N) is None
    irs = [rir_oracle.golden_irs()[k] for k in rir_seg_oracle.GOLDEN_IRS]
    ids = np.arange(len(items), dtype=np.int32)
    ref = np.stack([reference_clip(mix_snr, arena, it, irs[k], N) for it, k in zip(items, ids)])
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
