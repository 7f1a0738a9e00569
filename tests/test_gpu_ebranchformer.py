"""E-Branchformer head on the HIP path (run with -m gpu): reference goldens, the PCM composite, ONNX / .pt ingestion through the session,
the launch plan at the reference defaults, every fallback, every merge_x3 width against the float64 restatement, batch invariance, an
unclamped loud frame, the gate driven to both ends, every instance of attn_x3's branch form, and the Conformer's attention module left as
it was."""
import json
import os

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from parity import GOLDEN, assert_pcm_logits_vs_reference, head_golden_names, load_head_goldens

pytestmark = pytest.mark.gpu

LOGIT_ATOL = 1e-4
EMB_RTOL = 1e-4
MERGE_WIDTHS = (32, 64, 96, 128, 144, 192, 256)           # merge_x3_supported


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_ebranchformer.npz")


def _model(cfg, sd=None, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg) if sd is None else sd, **kw)


def _eb(shape, D=144, H=4, **kw):
    return HeadConfig("e_branchformer", shape, branchformer_d_model=D, branchformer_n_head=H, **kw)


def _head_plan(m):
    """the head's launches (the frontend runs for PCM input only; the sigmoid rides in the tail)"""
    return [l for l in m.describe_plan().strip().split("\n") if l.strip() and not l.startswith(("frontend:", "unary:sigmoid"))]


# ---- 1
@pytest.mark.parametrize("name", head_golden_names("heads_ebranchformer.npz"))
def test_features_vs_reference(golden, name):
    d, meta = golden
    cfg = HeadConfig(**meta[name])
    m = _model(cfg)
    feats = d[f"{name}/feats"]
    logits, probs, emb = m.forward_features(feats, return_embedding=True)
    ref, ref_e = d[f"{name}/logits_feat"].ravel(), d[f"{name}/emb_feat"]
    print(name, "max |dlogit| vs reference: %.2e" % np.abs(logits - ref).max(), "max |demb|: %.2e" % np.abs(emb - ref_e).max())
    assert np.abs(logits - ref).max() <= LOGIT_ATOL, (name, np.abs(logits - ref).max(), m.describe_plan())
    assert np.abs(emb - ref_e).max() <= EMB_RTOL * max(1.0, np.abs(ref_e).max()), (name, np.abs(emb - ref_e).max())
    assert np.abs(probs - oracle.sigmoid(ref)).max() <= 1e-5
    # ragged batches (tile edges, clips straddling the kernels' row tiles) against the restatement
    sd = synth_state_dict(cfg)
    for B in (1, 3, 33, 70):
        fx = synth_features(B, cfg.input_shape, seed=B)
        lg, _ = m.forward_features(fx)
        lo = oracle.model_forward(fx, sd, cfg).ravel()
        assert np.abs(lg - lo).max() <= LOGIT_ATOL, (name, B, np.abs(lg - lo).max())
    m.close()


# ---- 2
def test_pcm_vs_reference(golden, golden_frontend):
    from nanowakeword_amd.session import HipModel
    d, meta = golden
    g = golden_frontend
    name = "ebranchformer_101x64"
    cfg = HeadConfig(**meta[name])
    sd = synth_state_dict(cfg)
    m = HipModel(cfg, FrontendConfig(), state_dict=sd, window=g["window"], mel_fb=g["fb64"])
    lp, pp, err, _ = assert_pcm_logits_vs_reference(m, cfg, sd, g, g["pcm"], d[f"{name}/logits_pcm"].ravel(), what=name)
    print("PCM composite: max |dlogit| vs reference %.2e" % err.max())
    assert np.abs(pp - oracle.sigmoid(lp)).max() <= 1e-6
    m.close()


# ---- 3
def test_onnx_and_pt_through_the_session(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.weights import infer_head_config, load_session, save_bundle, state_dict_from_pt
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_e_branchformer.npz"), allow_pickle=False))
    feats, want = e["e_branchformer/feats"], e["e_branchformer/probs"]
    s = load_session(os.path.join(GOLDEN, "onnx", "e_branchformer.onnx"))
    assert np.abs(s.run(None, {"input": feats})[0].reshape(-1) - want).max() <= 1e-5
    # a .pt of the same weights -> bundle (n_head given: the weights do not record it) -> session
    cfg = HeadConfig(**json.loads(str(e["meta_json"]))["e_branchformer"])
    pt = str(tmp_path / "e_branchformer.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}, pt)
    sd = state_dict_from_pt(pt)
    c = infer_head_config(sd, input_shape=cfg.input_shape, n_head=cfg.branchformer_n_head)
    bundle = str(tmp_path / "e_branchformer_pt.nww.npz")
    save_bundle(bundle, c, sd, mode="features")
    s2 = load_session(bundle)
    assert np.abs(s2.run(None, {"input": feats})[0].reshape(-1) - want).max() <= 1e-5


# ---- 4
@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_plan_at_reference_defaults(shape):
    """Per block: the attention branch (one attn_x3 launch where T is in its range, else LayerNorm + in_proj, mha_h2, out_proj), LayerNorm +
    conv1 + GLU, the depthwise stage, merge_x3, ffn_x3: 5 / 7 launches; around them input_proj, the time mean and the tail."""
    cfg = _eb(shape)
    m = _model(cfg)
    plan = _head_plan(m)
    text = "\n".join(plan)
    assert m.feature_clamp == 0.0
    assert "layernorm:" not in text and "gemm:" not in text, text
    assert text.count("lin_x3:input_proj") == 1 and text.count("mean:time") == 1 and text.count("tail:") == 1, text
    assert text.count("layer_norm+conv1(pw)+glu") == 1 and text.count("dwconv1d+bn+swish:") == 1, text
    assert text.count("merge_x3:") == 1 and text.count("ffn_x3:") == 1 and "ln+linear1+swish+linear2+res)" in text, text
    if shape[0] > 64:
        assert text.count("attn_x3:") == 1 and "(ln+in_proj+softmax(qk)v+out_proj)" in text and "mha_h2:" not in text, text
        per_block = 5
    else:
        assert "attn_x3:" not in text and text.count("mha_h2:") == 1, text
        assert "attn_branch_norm+attention.in_proj" in text and text.count("attention.out_proj") == 1 and "out_proj+res" not in text, text
        per_block = 7
    assert len(plan) == 1 + per_block * cfg.n_blocks + 1 + 1, text
    m.close()


def _check(cfg, needles, batches=(1, 3, 33, 70), absent=(), sd=None, dtype=np.float64, **kw):
    """plan text holds every needle n_blocks times (and none of `absent`); logits at LOGIT_ATOL and embeddings at EMB_RTOL against the
    restatement in `dtype` at each batch size -> worst |dlogit|"""
    sd = synth_state_dict(cfg) if sd is None else sd
    m = _model(cfg, sd, **kw)
    text = m.describe_plan()
    assert m.feature_clamp == 0.0, text
    for n in needles:
        assert text.count(n) == cfg.n_blocks, (n, text)
    for n in absent:
        assert n not in text, (n, text)
    worst = 0.0
    for B in batches:
        fx = synth_features(B, cfg.input_shape, seed=B)
        lg, _, emb = m.forward_features(fx, return_embedding=True)
        e_ref = oracle.head_forward(fx, sd, cfg, dtype=dtype)
        ref = oracle.classify(e_ref, sd, cfg, dtype=dtype).ravel()
        assert np.isfinite(lg).all()
        worst = max(worst, float(np.abs(lg - ref).max()))
        assert np.abs(lg - ref).max() <= LOGIT_ATOL, (B, float(np.abs(lg - ref).max()), text)
        assert np.abs(emb - e_ref).max() <= EMB_RTOL * max(1.0, np.abs(e_ref).max()), (B, float(np.abs(emb - e_ref).max()))
    m.close()
    return worst


# ---- 5
def test_fallback_width_without_instances():
    cfg = _eb((16, 96), 48, 4, n_blocks=2, embedding_dim=32)
    worst = _check(cfg, ("branch_merge:", "final_norm", "merger.gate"), absent=("merge_x3:", "ffn_x3:", "attn_x3:"))
    print("d_model 48 (generic launches) max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("arith", ["bf16x6", "f32"])
@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_fallback_arithmetics(arith, shape):
    worst = _check(_eb(shape), ("branch_merge:", "final_norm"), absent=("merge_x3:", "attn_x3:"), batches=(1, 3, 33), conv_arith=arith)
    print(arith, shape, "max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("T,needles,absent", [
    (129, ("mha_core:", "merge_x3:", "ffn_x3:"), ("attn_x3:",)),
    (200, ("mha_core:", "merge_x3:", "ffn_x3:"), ("attn_x3:",)),
    (65, ("attn_x3:", "merge_x3:", "ffn_x3:"), ("mha_h2:", "mha_core:")),
    (128, ("attn_x3:", "merge_x3:", "ffn_x3:"), ("mha_h2:", "mha_core:")),
    (64, ("mha_h2:", "merge_x3:", "ffn_x3:", "attn_branch_norm+attention.in_proj"), ("attn_x3:",)),
    (33, ("mha_h2:", "merge_x3:", "ffn_x3:", "attn_branch_norm+attention.in_proj"), ("attn_x3:",)),
], ids=["T129", "T200", "T65", "T128", "T64", "T33"])
def test_attention_routes_at_the_default_width(T, needles, absent):
    """T > 128: attention on mha_core; T = 65 and 128: attn_x3's edges; T <= 64: the three-launch attention; merge_x3 and ffn_x3 throughout."""
    worst = _check(_eb((T, 64), n_blocks=2), needles, absent=absent, batches=(1, 3, 33))
    print("T", T, "max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("T", [66, 80, 81, 96, 97, 112, 113, 127])
def test_every_branch_instance_of_attn_x3(T):
    """The LayerNorm-in-front, no-residual form of attn_x3 is compiled per ceil(T / 16) = 5 .. 8: both sides of 80 | 81, 96 | 97 and 112 | 113 and
    the ends 66 and 127 reach every instance (T = 65, 101 and 128 above leave the six-tile one out).  At T = 81 and 97 clip 2 of a 33-clip batch
    also equals the same clip run alone, bit for bit: the kernel is clip-resident."""
    cfg = _eb((T, 64), n_blocks=1)
    worst = _check(cfg, ("attn_x3:", "merge_x3:", "ffn_x3:"), absent=("mha_h2:", "mha_core:"), batches=(1, 3, 33))
    print("T", T, "max |dlogit| vs float64: %.2e" % worst)
    if T in (81, 97):
        m = _model(cfg)
        x = synth_features(33, cfg.input_shape, seed=33)
        full, _, emb = m.forward_features(x, return_embedding=True)
        alone, _, emb1 = m.forward_features(np.ascontiguousarray(x[2:3]), return_embedding=True)
        assert alone[0] == full[2] and np.array_equal(emb1[0], emb[2]), (T, alone[0], full[2])
        m.close()


KNOBS = {
    "NWW_MERGE_FUSED": "assert 'merge_x3:' not in t and 'branch_merge:' in t and 'conv2(pw)' in t and 'merger.gate' in t and 'final_norm' in t, t",
    "NWW_ATTN_FUSED": "assert 'attn_x3:' not in t and 'mha_h2:' in t and 'attn_branch_norm+attention.in_proj' in t and 'merge_x3:' in t, t",
    "NWW_LIN_X3": "assert 'lin_x3:' not in t and 'layernorm:' in t and 'glu:' in t and 'gemm:' in t and 'merge_x3:' in t, t",
    "NWW_FFN_FUSED": "assert 'ffn_x3:' not in t and 'linear1+swish' in t and 'linear2+res' in t and 'merge_x3:' in t, t",
}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_knob_off_falls_back(knob):
    """Each selection knob of the head's fused pieces set to 0 (read once per process: a fresh interpreter): the general launches, same result."""
    import subprocess
    import sys
    code = ("import numpy as np, oracle\n"
            "from nanowakeword_amd.config import FrontendConfig, HeadConfig\n"
            "from nanowakeword_amd.session import HipModel\n"
            "from nanowakeword_amd.synth import synth_features, synth_state_dict\n"
            "cfg = HeadConfig('e_branchformer', (101, 64)); sd = synth_state_dict(cfg)\n"
            "m = HipModel(cfg, FrontendConfig(), state_dict=sd); t = m.describe_plan()\n"
            + KNOBS[knob] + "\n"
            "x = synth_features(5, cfg.input_shape, seed=4)\n"
            "d = np.abs(m.forward_features(x)[0] - oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()).max()\n"
            "assert d <= 1e-4, d\nprint('" + knob + "=0 max |dlogit| vs float64: %.2e' % d)\n")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    env[knob] = "0"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


def test_width_192_keeps_its_layernorm_out_of_in_proj():
    """d_model 192: lin_x3 has no LayerNorm + in_proj instance there (it would not fit the register file), so the branch's LayerNorm is a
    launch of its own in front of the plain in_proj instance; every other compiled width folds it in."""
    for D, folded in ((192, False), (256, True), (128, True)):
        m = _model(_eb((33, 32), D, 4, embedding_dim=32))
        text = m.describe_plan()
        assert ("attn_branch_norm+attention.in_proj" in text) == folded and ("layernorm:model.branchformer_blocks.0.attn_branch_norm" in text) != folded, (D, text)
        assert "lin_x3:model.branchformer_blocks.0" in text and "gemm:" not in text, (D, text)
        m.close()


# ---- 6
@pytest.mark.parametrize("T", [1, 5, 31, 32, 33, 64, 65, 101, 128])
@pytest.mark.parametrize("D,blocks", [(D, b) for D in MERGE_WIDTHS for b in (1, 2)])
def test_merge_widths_and_clip_lengths_vs_float64(D, blocks, T):
    """Every compiled merge_x3 width x clip lengths on both sides of its 64-row workgroups and 32-row tiles (many clips per tile, a clip ending
    on a tile's last row or one row into the next), one and two blocks (the second block's merge reads what the first block's ffn wrote)."""
    cfg = _eb((T, 32), D, 4, n_blocks=blocks, embedding_dim=32)
    worst = _check(cfg, ("merge_x3:",), absent=("branch_merge:",))
    print("D", D, "blocks", blocks, "T", T, "max |dlogit| vs float64: %.2e" % worst)


# ---- 7
@pytest.mark.parametrize("shape,B", [((16, 96), 4096), ((101, 64), 2048)])
def test_batch_invariance(shape, B):
    cfg = _eb(shape)
    m = _model(cfg)
    assert "merge_x3:" in m.describe_plan()
    x = synth_features(B, shape, seed=11)
    full, _ = m.forward_features(x)
    for i in (0, B - 1):
        alone, _ = m.forward_features(np.ascontiguousarray(x[i:i + 1]))
        assert alone[0] == full[i], (shape, i, alone[0], full[i])
    ref = oracle.model_forward(x[:8], synth_state_dict(cfg), cfg).ravel()
    assert np.abs(full[:8] - ref).max() <= LOGIT_ATOL
    m.close()


def test_batch_invariance_many_clips_per_tile():
    """T = 5: a 32-row tile holds rows of seven clips and clip 6 straddles the first tile's edge; B = 4099 leaves a ragged last tile."""
    cfg = _eb((5, 32), 64, 4, embedding_dim=32)
    m = _model(cfg)
    assert "merge_x3:" in m.describe_plan() and "mha_h2:" in m.describe_plan(), m.describe_plan()
    B = 4099
    x = synth_features(B, cfg.input_shape, seed=11)
    full, _ = m.forward_features(x)
    for i in (0, 6, 12, B - 1):
        alone, _ = m.forward_features(np.ascontiguousarray(x[i:i + 1]))
        assert alone[0] == full[i], (i, alone[0], full[i])
    ref = oracle.model_forward(x[:40], synth_state_dict(cfg), cfg, dtype=np.float64).ravel()
    assert np.abs(full[:40] - ref).max() <= LOGIT_ATOL
    m.close()


# ---- 8
@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_unclamped_loud_frame(shape):
    """Nothing clamps the features: one frame of one clip x 1e4 on the default weights stays finite and within LOGIT_ATOL max(1, |ref|) of
    float64.  The float32 restatement is asserted within a tenth of that first (seed 31), so the kernels are judged on a well-conditioned case."""
    cfg = _eb(shape)
    sd = synth_state_dict(cfg)
    x = synth_features(6, cfg.input_shape, seed=31)
    x[1, 7] *= np.float32(1e4)
    ref = oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
    tol = LOGIT_ATOL * np.maximum(1.0, np.abs(ref))
    assert np.all(np.abs(oracle.model_forward(x, sd, cfg).ravel() - ref) <= 0.1 * tol)
    m = _model(cfg, sd)
    assert m.feature_clamp == 0.0 and "merge_x3:" in m.describe_plan(), m.describe_plan()
    lg, _ = m.forward_features(x)
    assert np.isfinite(lg).all(), lg
    print("loud frame", shape, "max |dlogit| / max(1, |ref|) vs float64: %.2e" % float((np.abs(lg - ref) / np.maximum(1.0, np.abs(ref))).max()))
    assert np.all(np.abs(lg - ref) <= tol), (lg, ref)
    m.close()


# ---- 9
@pytest.mark.parametrize("bias", [30.0, -30.0], ids=["attention_only", "conv_only"])
@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_gate_driven_to_both_ends(shape, bias):
    """merger.gate.bias = +-30: g is 1 or 0 to float32 and the block passes one branch only - a merge with the branches swapped, or 1 - g on the
    wrong side, cannot pass both ends."""
    cfg = _eb(shape, n_blocks=2)
    sd = synth_state_dict(cfg)
    for i in range(cfg.n_blocks):
        sd[f"model.branchformer_blocks.{i}.merger.gate.bias"] = np.full(cfg.branchformer_d_model, bias, np.float32)
    worst = _check(cfg, ("merge_x3:",), batches=(1, 3, 33), sd=sd)
    # the two ends differ: the case distinguishes the branches
    x = synth_features(3, shape, seed=3)
    sd2 = dict(sd)
    for i in range(cfg.n_blocks):
        sd2[f"model.branchformer_blocks.{i}.merger.gate.bias"] = -sd[f"model.branchformer_blocks.{i}.merger.gate.bias"]
    assert np.abs(oracle.model_forward(x, sd, cfg, dtype=np.float64) - oracle.model_forward(x, sd2, cfg, dtype=np.float64)).max() > 100 * LOGIT_ATOL
    print("gate bias", bias, shape, "max |dlogit| vs float64: %.2e" % worst)


# ---- 10
def test_conformer_attention_module_untouched(golden_heads):
    """The new AttnArgs fields default to the Conformer's module: its plan still has one attn_x3 launch with the residual per block and its
    logits sit on the existing golden at the existing bar."""
    d, meta = golden_heads
    cfg = HeadConfig(**meta["conformer_101x64"])
    assert cfg.model_type == "conformer" and cfg.input_shape == (101, 64)
    m = _model(cfg)
    text = m.describe_plan()
    assert text.count("attn_x3:") == cfg.n_blocks and "(in_proj+softmax(qk)v+out_proj+res)" in text and "(ln+in_proj" not in text, text
    # heads.npz stores no features: its logits_feat are the reference's on synth_features(4, shape), as tests/test_gpu_parity.py feeds them
    logits, _ = m.forward_features(synth_features(4, cfg.input_shape))
    assert np.abs(logits - d["conformer_101x64/logits_feat"].ravel()).max() <= LOGIT_ATOL
    m.close()


def test_create_validates_heads():
    from nanowakeword_amd import _lib
    from nanowakeword_amd.session import HipModel
    cfg = _eb((16, 96), 128, 4)
    cfg.branchformer_n_head = 3                                        # past HeadConfig's own check: the C side refuses it too
    with pytest.raises(Exception, match="branchformer_d_model must be divisible by branchformer_n_head"):
        HipModel(cfg, FrontendConfig())
    with pytest.raises(Exception, match="head_dim"):
        HipModel(_eb((16, 96), 260, 2), FrontendConfig())
