"""tests/golden/pitch.npz: the float64 DEFINITION of the pitch shift (tests/pitch_oracle.py: torch.stft / torch.istft in float64, the
textbook phase vocoder, the resampler as a direct sum) on seeded inputs, for tests/test_pitch_host.py and tests/test_gpu_pitch.py.  It
pins the definition against a change of torch; it is NOT the output of torch_audiomentations' PitchShift, which is not installed where
this was written and whose samples are not claimed.  Needs no checkout of the reference.

Four items at N = 4000 out of mix_oracle's golden arena (integer arithmetic alone) at ratios 9/8, 15/16, 128/125 and none; the file
holds the item table, the ratio ids, the ratios, the definition's int16 clips and, as metadata, how the float32 restatement of
csrc/pitch_plan.h compares with the definition on every item of tests/golden/mix.npz that has a background: its max-abs and rms error
over those of the same definition run in float32 torch ops, and after the int16 tail the share of samples that differ and the largest
difference."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import mix_oracle  # noqa: E402
import pitch_oracle  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "pitch.npz"))
    a = ap.parse_args()
    import torch
    arena, _, _ = mix_oracle.golden_arena()
    items, ids, N = pitch_oracle.golden_items(), np.array(pitch_oracle.GOLDEN_IDS, np.int32), pitch_oracle.GOLDEN_N
    assert mix_oracle.bad_field(items[0], arena.size, N) is None
    ref = pitch_oracle.definition(arena, items, ids, pitch_oracle.GOLDEN_RATIOS, N)
    ours = pitch_oracle.mix_aug(arena, items, ids, pitch_oracle.GOLDEN_RATIOS, N)
    d = np.abs(ref.astype(np.int32) - ours.astype(np.int32))
    acc = pitch_oracle.accuracy(*pitch_oracle.accuracy_clips())
    meta = {"N": N, "items": int(len(items)), "arena_samples": int(arena.size), "arena_sum": int(arena.astype(np.int64).sum()),
            "torch": torch.__version__, "restatement_differing_per_clip": [int(x) for x in (d > 0).sum(axis=1)],
            "restatement_max_abs_diff": int(d.max()),
            "accuracy_clips": "tests/golden/mix.npz items with a background, N = 16000, RATIOS in turn",
            "accuracy_max_abs_ratio": [round(r[0], 4) for r in acc], "accuracy_rms_ratio": [round(r[1], 4) for r in acc],
            "accuracy_int16_differing_share": [round(r[2], 6) for r in acc], "accuracy_int16_max_diff": [r[3] for r in acc],
            "chain": "mix_y float32 + definition_y float64 (stft 512 / 128 periodic Hann, vocoder, istft, direct-sum resampler) + the :246-259 tail float64"}
    np.savez_compressed(a.out, items=items, pitch_ids=ids, ratios=np.array(pitch_oracle.GOLDEN_RATIOS, np.int32), ref=ref,
                        meta=np.array(json.dumps(meta)))
    print(json.dumps(meta), os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
