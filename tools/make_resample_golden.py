"""tests/golden/resample.npz: the float64 DEFINITION of the ingest resampler (tests/resample_oracle.py) on speech-like
clips of half a second at eight rate pairs, after the int16 tail - and, in the metadata, what the float32 restatement makes of the same
clips: the share of samples that differ, the largest difference, and the float32 error before the tail in LSB.

    python tools/make_resample_golden.py            # writes tests/golden/resample.npz
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resample_oracle as ro  # noqa: E402


def accuracy(recs, ratios):
    """per clip (share of int16 samples differing, largest difference in LSB, float32 error before the tail in LSB)"""
    rows = []
    for x, r in zip(recs, ratios):
        a, b = ro.restatement(x, r, np.int16).astype(np.int32), ro.definition(x, r, np.int16).astype(np.int32)
        err = float(np.abs(ro.restatement_v(x, r).astype(np.float64) - ro.definition_v(x, r)).max())
        rows.append((float((a != b).mean()), int(np.abs(a - b).max()), err))
    return rows


def main():
    recs = ro.golden_recordings()
    ratios = [ro.rate_ratio(fs) for fs, _ in ro.GOLDEN_PAIRS]
    ref = [ro.definition(x, r, np.int16) for x, r in zip(recs, ratios)]
    rows = accuracy(recs, ratios)
    meta = {"pairs": ro.GOLDEN_PAIRS, "recording_sums": [int(x.astype(np.int64).sum()) for x in recs],
            "restatement_differing_share": [r[0] for r in rows], "restatement_max_abs_diff": [r[1] for r in rows],
            "restatement_float32_error_lsb": [r[2] for r in rows]}
    for (fs, C), r in zip(ro.GOLDEN_PAIRS, rows):
        print(f"{fs} Hz x{C}: differing {100 * r[0]:.3f} %, max {r[1]} LSB, float32 error {r[2]:.4f} LSB")
    np.savez_compressed(ro.golden_path(), ratios=np.array(ratios, np.int32), lengths=np.array([len(y) for y in ref], np.int64),
                        ref=np.concatenate(ref), meta=json.dumps(meta))
    print("wrote", ro.golden_path(), os.path.getsize(ro.golden_path()), "bytes")


if __name__ == "__main__":
    main()
