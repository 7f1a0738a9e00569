"""The Conformer's stressed inputs (tests/test_gpu_conformer_stress.py runs them on the HIP path): one loud frame, one quiet clip, a peaked
softmax, at one shape per attention route.  Here, on the CPU: every case is well-conditioned - the float32 restatement stays within a tenth of
the logit bound of the float64 one - and the peaked cases keep their top two scores apart, so a kernel judged on them is judged fairly."""
import functools

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from oracle.heads import net_conformer
from parity import LOGIT_ATOL

B = 6
LOUD_CLIP, LOUD_ROW = 1, 7
QUIET_CLIP, QUIET_ROW, QUIET_RATIO = 3, 7, 2.0 ** -13

# one shape per attention route: name -> (HeadConfig arguments, what describe_plan() must and must not hold under the default arithmetic)
SHAPES = {
    "101x64": (dict(input_shape=(101, 64)), ["attn_x3:"], ["mha_h2:", "mha_core:", "mha_mfma:"]),                    # the default head
    "128x64": (dict(input_shape=(128, 64)), ["attn_x3:"], ["mha_h2:", "mha_core:", "mha_mfma:"]),                    # 8 key blocks, no ragged tile
    "40x64-d96": (dict(input_shape=(40, 64), embedding_dim=16, conformer_d_model=96, conformer_n_head=4),
                  ["in_proj(head-major)", "mha_h2:", "out_proj+res"], ["attn_x3:", "mha_core:", "mha_mfma:"]),      # lin_x3 + mha_h2       
    "33x64": (dict(input_shape=(33, 64)), ["in_proj(head-major)", "mha_h2:", "out_proj+res"],
              ["attn_x3:", "mha_core:", "mha_mfma:"]),                                                               # T <= 64 at d_model 144: second key tile ragged
    "130x64": (dict(input_shape=(130, 64)), ["mha_core:"], ["attn_x3:", "mha_h2:", "mha_mfma:"]),                    # T > 128
}

# synth_features' seed of the peaked cases: 31, 32, ... in order, the first whose smallest top-two score gap (float64, any block, clip, head and
# query) is >= 1e-4 of the row's largest score.  31 does at every shape; the measured gap, the same at all three factors, beside it
PEAKED_SEED = {"101x64": 31,        # 1.489e-4
               "128x64": 31,        # 1.025e-4
               "40x64-d96": 31,     # 3.010e-4
               "33x64": 31,         # 1.489e-4 (clip 0's first 33 rows are the (101, 64) clip's: the same pair of keys)
               "130x64": 31}        # 1.025e-4
MIN_GAP = 1e-4

LOUD = {"row7_x1e2": (LOUD_ROW, 1e2), "row7_x1e4": (LOUD_ROW, 1e4), "row0_x1e4": (0, 1e4), "last_row_x1e4": (-1, 1e4)}
PEAKED = {"x2^3": 8.0, "x2^6": 64.0, "x2^9": 512.0}
CASES = list(LOUD) + ["quiet_clip"] + list(PEAKED)


def config(shape):
    return HeadConfig("conformer", **SHAPES[shape][0])


def assert_route(shape, plan):
    want, unwanted = SHAPES[shape][1:]
    assert all(w in plan for w in want) and not any(w in plan for w in unwanted), (shape, plan)


def loud_frame(x, row, factor, clips=(LOUD_CLIP,)):
    """one frame of the given clips x factor (nothing clamps the features: the row stays loud in the residual stream of every block)"""
    x = x.copy()
    for c in clips:
        x[c, row] *= np.float32(factor)
    return x


def quiet_clip(x, ratio=QUIET_RATIO, clip=QUIET_CLIP, row=QUIET_ROW):
    """a whole clip x ratio with one of its rows back at full scale: the loud frame seen from the other side, every other row is the small one
    (in the features, where the fused input projection scales them; input_proj's bias and ff1 bring the residual stream's rows back to O(1))"""
    x = x.copy()
    keep = x[clip, row].copy()
    x[clip] *= np.float32(ratio)
    x[clip, row] = keep
    return x


def peaked(sd, cfg, s):
    """the q and k rows of every block's in_proj x s: raw scores x s^2"""
    D = cfg.conformer_d_model
    out = {k: np.array(v, np.float32, copy=True) for k, v in sd.items()}
    for i in range(cfg.n_blocks):
        p = f"model.conformer_blocks.{i}.attention.in_proj_"
        out[p + "weight"][:2 * D] *= np.float32(s)
        out[p + "bias"][:2 * D] *= np.float32(s)
    return out


def build_case(shape, case):
    """-> (cfg, features [B, T, F] float32, state dict) of one stressed case"""
    cfg = config(shape)
    sd = synth_state_dict(cfg)
    if case in PEAKED:
        return cfg, synth_features(B, cfg.input_shape, seed=PEAKED_SEED[shape]), peaked(sd, cfg, PEAKED[case])
    x = synth_features(B, cfg.input_shape, seed=31)
    if case == "quiet_clip":
        return cfg, quiet_clip(x), sd
    row, factor = LOUD[case]
    return cfg, loud_frame(x, row, factor), sd


def top_two_score_gaps(x, sd, cfg):
    """test_gpu_transformer.py's measure at the Conformer's attention: float64, per block, the smallest gap between the two largest scaled scores
    q.k / sqrt(dh) of any (clip, head, query), relative to max(1, the row's largest |score|).  The attention input is the oracle block's own."""
    f8 = np.float64
    w = {k: np.asarray(v, f8) for k, v in sd.items()}
    D, nh, T = cfg.conformer_d_model, cfg.conformer_n_head, x.shape[1]
    inputs = []
    net_conformer(np.asarray(x, f8), w, cfg, attn_inputs=inputs)
    assert len(inputs) == cfg.n_blocks
    gaps = []
    for i, h in enumerate(inputs):
        p = f"model.conformer_blocks.{i}.attention"
        qkv = h @ w[p + ".in_proj_weight"].T + w[p + ".in_proj_bias"]
        q, k = (qkv[..., j * D:(j + 1) * D].reshape(len(x), T, nh, D // nh).transpose(0, 2, 1, 3) for j in range(2))
        s = np.sort(q @ k.transpose(0, 1, 3, 2) / np.sqrt(f8(D // nh)), axis=-1)
        top = np.maximum(1.0, np.maximum(np.abs(s[..., 0]), np.abs(s[..., -1])))
        gaps.append(float(((s[..., -1] - s[..., -2]) / top).min()))
    return gaps


@functools.lru_cache(maxsize=None)
def conditioned_case(shape, case):
    """-> (cfg, x, sd, ref64 [B], tol [B]) with the case's fairness asserted: float32 numpy within 0.1 x LOGIT_ATOL x max(1, |ref64|) of float64,
    and for the peaked cases the top-two gap.  Evaluated once per process; nobody writes to what it returns."""
    cfg, x, sd = build_case(shape, case)
    ref = oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
    tol = LOGIT_ATOL * np.maximum(1.0, np.abs(ref))
    f32 = oracle.model_forward(x, sd, cfg).ravel()
    share = float((np.abs(f32 - ref) / tol).max())
    gap = min(top_two_score_gaps(x, sd, cfg)) if case in PEAKED else None
    print(f"conformer stress {shape} {case}: float32 vs float64 {float(np.abs(f32 - ref).max()):.2e} = {share:.3f} of the bound"
          + (f", top-two gap {gap:.3e}" if gap is not None else ""))
    assert np.isfinite(ref).all() and share <= 0.1, (shape, case, share)
    if gap is not None:
        assert gap >= MIN_GAP, (shape, case, gap)
    for a in (x, ref, tol, *sd.values()):
        a.setflags(write=False)
    return cfg, x, sd, ref, tol


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stressed_cases_are_well_conditioned(shape, case):
    conditioned_case(shape, case)


def test_loud_frame_moves_its_clip_only():
    """the case measures something: the x 1e4 frame moves clip 1's float64 logit, and no other clip's"""
    for shape in SHAPES:
        cfg, x, sd, ref, _ = conditioned_case(shape, "row7_x1e4")
        plain = oracle.model_forward(synth_features(B, cfg.input_shape, seed=31), sd, cfg, dtype=np.float64).ravel()
        others = np.arange(B) != LOUD_CLIP
        assert np.array_equal(ref[others], plain[others])
        assert abs(ref[LOUD_CLIP] - plain[LOUD_CLIP]) > 100 * LOGIT_ATOL, (shape, ref[LOUD_CLIP], plain[LOUD_CLIP])
