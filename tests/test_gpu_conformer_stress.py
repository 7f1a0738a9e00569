"""Conformer head on the HIP path under data that stresses its run-time scales (run with -m gpu): one loud frame in a clip (attn_x3 scales a
clip's rows by ONE power of two), one quiet clip around a full-scale row, a peaked softmax (scores x 2^18 in front of exp2), at one
shape per attention route; isolation of the clips at a batch larger than the grid; the three-launch path on the same loud frame.  Every case
against the float64 restatement, beside the float32-MFMA arithmetic on the same inputs and weights.  The cases and their conditioning
(asserted first, as test_gpu_transformer.py::test_peaked_softmax does) come from test_conformer_stress.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nanowakeword_amd.config import FrontendConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from test_conformer_stress import (B, LOUD, LOUD_CLIP, LOUD_ROW, PEAKED, SHAPES, assert_route, conditioned_case, config, loud_frame)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plain_models():
    """shape -> (default-arithmetic model, conv_arith = f32 model) on synth_state_dict: shared by the loud-frame and quiet-clip cases"""
    from nanowakeword_amd.session import HipModel
    made = {}

    def get(shape):
        if shape not in made:
            cfg = config(shape)
            sd = synth_state_dict(cfg)
            made[shape] = (HipModel(cfg, FrontendConfig(), state_dict=sd), HipModel(cfg, FrontendConfig(), state_dict=sd, conv_arith="f32"))
        return made[shape]
    yield get
    for pair in made.values():
        for m in pair:
            m.close()


def _assert_against_float64(shape, case, m, m32):
    """the route, then finite logits within LOGIT_ATOL x max(1, |ref64|) per clip, and - relative to max(1, |logit|max), the convention of
    test_heavy_tailed_weights_against_float64 - the default arithmetic no worse than 2 x the float32-MFMA one + 2e-6"""
    cfg, x, sd, ref, tol = conditioned_case(shape, case)
    assert_route(shape, m.describe_plan())
    assert "[f16x3]" not in m32.describe_plan() and "attn_x3" not in m32.describe_plan(), m32.describe_plan()
    assert m.feature_clamp == 0.0 and m32.feature_clamp == 0.0
    lg, _ = m.forward_features(x)
    l32, _ = m32.forward_features(x)
    scale = max(1.0, float(np.abs(ref).max()))
    with np.errstate(invalid="ignore"):
        share = float(np.nan_to_num(np.abs(lg - ref) / tol, nan=np.inf).max())
        rel = {"f16x3": float(np.nan_to_num(np.abs(lg - ref), nan=np.inf).max()) / scale, "f32": float(np.nan_to_num(np.abs(l32 - ref), nan=np.inf).max()) / scale}
    print(f"conformer stress {shape} {case}: max |dlogit| / (LOGIT_ATOL max(1, |ref|)) = {share:.3f}; / max(1, |logit|max): {rel}")
    assert np.isfinite(lg).all() and np.isfinite(l32).all(), (shape, case, lg, l32)
    assert np.all(np.abs(lg - ref) <= tol), (shape, case, lg, ref)
    assert rel["f16x3"] <= 2.0 * rel["f32"] + 2e-6, (shape, case, rel)


@pytest.mark.parametrize("case", list(LOUD))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_loud_frame(plain_models, shape, case):
    """One frame of clip 1 x 1e2 / x 1e4 - row 7, and row 0 and row T - 1 (the first query tile and the ragged last one).  Nothing normalises
    the Conformer's attention input, so the row is as loud in the residual stream as in the features: every other row of the clip sits 2^13
    below the maximum that attn_x3's clip scale is taken from, and the row's score with itself is ~1e8 (a softmax that rounds max x log2(e) at
    that size before it subtracts it loses the row: mha_h2.hip; that form measured 0.2 .. 1.02 off on six of these cases, this one 3e-7 .. 9e-7)."""
    _assert_against_float64(shape, case, *plain_models(shape))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_quiet_clip(plain_models, shape):
    """A whole clip x 2^-13 with one row left at full scale: the same ratio with the small rows the ones that matter."""
    _assert_against_float64(shape, "quiet_clip", *plain_models(shape))


@pytest.mark.parametrize("case", list(PEAKED))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_peaked_softmax(shape, case):
    """The q and k rows of in_proj x 2^3, 2^6, 2^9: scores x 2^6 .. 2^18, a one-hot softmax (not combined with the loud frame:
    test_gpu_transformer.py::test_peaked_softmax says why)."""
    from nanowakeword_amd.session import HipModel
    cfg, _, sd, _, _ = conditioned_case(shape, case)
    m, m32 = HipModel(cfg, FrontendConfig(), state_dict=sd), HipModel(cfg, FrontendConfig(), state_dict=sd, conv_arith="f32")
    try:
        _assert_against_float64(shape, case, m, m32)
    finally:
        m.close()
        m32.close()


def test_loud_frames_stay_in_their_clips(plain_models):
    """(101, 64), B = 300 - more clips than workgroups, so attn_x3's workgroups walk a second clip behind a loud one - with the x 1e4 frame in
    every 7th clip (1, 8, 15, ...): a clip without one gives the bits it gives in the same batch with no loud frame at all, every clip gives the
    bits it gives alone, and the first six clips (the row7_x1e4 case's) are within LOGIT_ATOL x max(1, |ref|) of float64."""
    shape, n = "101x64", 300
    cfg, x6, _, ref, tol = conditioned_case(shape, "row7_x1e4")
    m, _ = plain_models(shape)
    assert_route(shape, m.describe_plan())
    plain = synth_features(n, cfg.input_shape, seed=31)
    loud_clips = list(range(LOUD_CLIP, n, 7))
    x = loud_frame(plain, LOUD_ROW, 1e4, clips=loud_clips)
    assert np.array_equal(x[:B], x6)
    full, _ = m.forward_features(x)
    base, _ = m.forward_features(plain)
    assert np.isfinite(full).all() and np.isfinite(base).all()
    print("conformer stress isolation: max |dlogit| / (LOGIT_ATOL max(1, |ref|)) of the first six clips = %.3f" % float((np.abs(full[:B] - ref) / tol).max()))
    assert np.all(np.abs(full[:B] - ref) <= tol), (full[:B], ref)
    others = np.setdiff1d(np.arange(n), loud_clips)
    assert np.array_equal(full[others], base[others]), others[full[others] != base[others]]
    assert not np.array_equal(full[loud_clips], base[loud_clips])
    alone = np.concatenate([m.forward_features(x[i:i + 1])[0] for i in range(n)])
    assert np.array_equal(alone, full), np.flatnonzero(alone != full)


# NWW_ATTN_FUSED is read once per process: the three-launch path at attn_x3's shape needs a fresh one (test_gpu_variants.py's knob tests)
_THREE_LAUNCH_SCRIPT = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.environ["NWW_ROOT"], "tests"))
from nanowakeword_amd.config import FrontendConfig
from nanowakeword_amd.session import HipModel
from test_conformer_stress import conditioned_case
cfg, x, sd, ref, tol = conditioned_case("101x64", "row7_x1e4")
m = HipModel(cfg, FrontendConfig(), state_dict=sd)
plan = m.describe_plan()
assert all(w in plan for w in ("in_proj(head-major)", "mha_h2:", "out_proj+res")) and "attn_x3" not in plan, plan
assert m.feature_clamp == 0.0
lg, _ = m.forward_features(x)
m.close()
print("SHARE %.3f" % float(np.nan_to_num(np.abs(lg - ref) / tol, nan=np.inf).max()))
assert np.isfinite(lg).all(), lg
assert np.all(np.abs(lg - ref) <= tol), (lg, ref)
'''


def test_loud_frame_on_the_three_launch_path():
    """the x 1e4 loud frame at (101, 64) under NWW_ATTN_FUSED = 0: lin_x3 in_proj (every row scaled on its own), mha_h2, out_proj + residual"""
    e = dict(os.environ, NWW_ROOT=ROOT, NWW_ATTN_FUSED="0", PYTHONPATH=os.pathsep.join([ROOT] + sys.path))
    r = subprocess.run([sys.executable, "-c", _THREE_LAUNCH_SCRIPT], env=e, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "SHARE" in r.stdout
