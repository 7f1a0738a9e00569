"""Transformer head on the HIP path (run with -m gpu): reference goldens, the PCM composite, ONNX / .pt ingestion through the session,
the launch plan at the reference defaults, the generic fallback, batch invariance and the unclamped input projection; every instance
of the head's own kernels (mha_h2's exact-subtraction form at each head dim, the post-norm ffn_x3 at each width and at the clip lengths
that decide its time sums' segments) against the float64 restatement, clips longer than the attention kernels take, a peaked softmax."""
import json
import os

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from oracle.heads import transformer_input, transformer_layer
from parity import GOLDEN, assert_pcm_logits_vs_reference, head_golden_names, load_head_goldens

pytestmark = pytest.mark.gpu

LOGIT_ATOL = 1e-4
EMB_RTOL = 1e-4


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_transformer.npz")


def _model(cfg, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg), **kw)


@pytest.mark.parametrize("name", head_golden_names("heads_transformer.npz"))
def test_features_vs_reference(golden, name):
    d, meta = golden
    cfg = HeadConfig(**meta[name])
    m = _model(cfg)
    assert m.feature_clamp == 0.0, m.describe_plan()
    feats = d[f"{name}/feats"]
    logits, probs, emb = m.forward_features(feats, return_embedding=True)
    ref, ref_e = d[f"{name}/logits_feat"].ravel(), d[f"{name}/emb_feat"]
    assert np.abs(logits - ref).max() <= LOGIT_ATOL, (name, np.abs(logits - ref).max(), m.describe_plan())
    assert np.abs(emb - ref_e).max() <= EMB_RTOL * max(1.0, np.abs(ref_e).max()), (name, np.abs(emb - ref_e).max())
    assert np.abs(probs - oracle.sigmoid(ref)).max() <= 1e-5
    # ragged batches (tile edges, clips straddling 32-row tiles) against the restatement
    sd = synth_state_dict(cfg)
    for B in (1, 3, 33, 70):
        fx = synth_features(B, cfg.input_shape, seed=B)
        lg, _ = m.forward_features(fx)
        lo = oracle.model_forward(fx, sd, cfg).ravel()
        assert np.abs(lg - lo).max() <= LOGIT_ATOL, (name, B, np.abs(lg - lo).max())
    m.close()


def test_pcm_vs_reference(golden, golden_frontend):
    from nanowakeword_amd.session import HipModel
    d, meta = golden
    g = golden_frontend
    name = "transformer_101x64"
    cfg = HeadConfig(**meta[name])
    sd = synth_state_dict(cfg)
    m = HipModel(cfg, FrontendConfig(), state_dict=sd, window=g["window"], mel_fb=g["fb64"])
    lp, pp, _, _ = assert_pcm_logits_vs_reference(m, cfg, sd, g, g["pcm"], d[f"{name}/logits_pcm"].ravel(), what=name)
    assert np.abs(pp - oracle.sigmoid(lp)).max() <= 1e-6
    m.close()


def test_onnx_and_pt_through_the_session(tmp_path):
    """The session HipInterpreter.load_model holds per model (feature-input models also need the caller's preprocessor there)."""
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.weights import infer_head_config, load_session, save_bundle, state_dict_from_pt
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_transformer.npz"), allow_pickle=False))
    feats, want = e["transformer/feats"], e["transformer/probs"]
    s = load_session(os.path.join(GOLDEN, "onnx", "transformer.onnx"))
    assert np.abs(s.run(None, {"input": feats})[0].reshape(-1) - want).max() <= 1e-5
    # a .pt of the same weights -> bundle (n_head given: the weights do not record it) -> session
    cfg = HeadConfig(**json.loads(str(e["meta_json"]))["transformer"])
    pt = str(tmp_path / "transformer.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}, pt)
    sd = state_dict_from_pt(pt)
    c = infer_head_config(sd, input_shape=cfg.input_shape, n_head=cfg.transformer_n_head)
    bundle = str(tmp_path / "transformer_pt.nww.npz")
    save_bundle(bundle, c, sd, mode="features")
    s2 = load_session(bundle)
    assert np.abs(s2.run(None, {"input": feats})[0].reshape(-1) - want).max() <= 1e-5


@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_plan_at_reference_defaults(shape):
    cfg = HeadConfig("transformer", shape)
    m = _model(cfg)
    # the head's launches (the frontend runs for PCM input only; the sigmoid rides in the tail)
    plan = [l for l in m.describe_plan().strip().split("\n") if l.strip() and not l.startswith(("frontend:", "unary:sigmoid"))]
    text = "\n".join(plan)
    assert m.feature_clamp == 0.0
    assert "input_proj*sqrt(d)+pe" in text and "lin_x3:" in text, text
    assert "mha_h2:" in text and "post-norm" in text and "mean_finish:" in text, text
    assert "layernorm:" not in text and "gemm:" not in text, text
    assert len(plan) == 1 + 4 * cfg.n_blocks + 1 + 1, text
    m.close()


def test_fallback_width_matches_restatement():
    cfg = HeadConfig("transformer", (16, 96), n_blocks=2, embedding_dim=32, transformer_d_model=48, transformer_n_head=4)
    m = _model(cfg)
    text = m.describe_plan()
    assert "gemm:" in text and "layernorm:" in text and "ffn_x3" not in text, text
    sd = synth_state_dict(cfg)
    fx = synth_features(37, cfg.input_shape, seed=5)
    lg, _, emb = m.forward_features(fx, return_embedding=True)
    e_or = oracle.head_forward(fx, sd, cfg)
    assert np.abs(lg - oracle.model_forward(fx, sd, cfg).ravel()).max() <= LOGIT_ATOL
    assert np.abs(emb - e_or).max() <= EMB_RTOL * max(1.0, np.abs(e_or).max())
    m.close()
    # 12 input features: no short-K instance - the general GEMM, then the scale and the positional rows in one elementwise pass
    cfg = HeadConfig("transformer", (8, 12), embedding_dim=16, transformer_d_model=32, transformer_n_head=2)
    m = _model(cfg)
    assert "gemm:input_proj" in m.describe_plan() and "scale+pe:" in m.describe_plan()
    fx = synth_features(9, cfg.input_shape, seed=6)
    assert np.abs(m.forward_features(fx)[0] - oracle.model_forward(fx, synth_state_dict(cfg), cfg).ravel()).max() <= LOGIT_ATOL
    m.close()


@pytest.mark.parametrize("shape,B", [((16, 96), 4096), ((101, 64), 2048)])
def test_batch_invariance(shape, B):
    cfg = HeadConfig("transformer", shape)
    m = _model(cfg)
    x = synth_features(B, shape, seed=11)
    full, _ = m.forward_features(x)
    for i in (0, B - 1):
        alone, _ = m.forward_features(np.ascontiguousarray(x[i:i + 1]))
        assert alone[0] == full[i], (shape, i, alone[0], full[i])
    ref = oracle.model_forward(x[:8], synth_state_dict(cfg), cfg).ravel()
    assert np.abs(full[:8] - ref).max() <= LOGIT_ATOL
    m.close()


def test_create_validates_heads():
    from nanowakeword_amd.session import HipModel
    with pytest.raises(Exception, match="transformer_d_model must be divisible by transformer_n_head"):
        HipModel(HeadConfig("transformer", (16, 96), transformer_d_model=100, transformer_n_head=3), FrontendConfig())
    with pytest.raises(Exception, match="head_dim"):
        HipModel(HeadConfig("transformer", (16, 96), transformer_d_model=260, transformer_n_head=2), FrontendConfig())


FFN_WIDTHS = (32, 64, 96, 128, 144, 192, 256)             # the post-norm ffn_x3 instances (ffn_x3_post_supported)


def _check_against_float64(cfg, attn, ffn_fused, batches=(1, 3, 33, 70)):
    """plan: the attention kernel named, the post-norm ffn_x3 + mean_finish (or the fallback's layernorm + GEMMs) in every block;
    logits at LOGIT_ATOL and embeddings at EMB_RTOL against float64 at each batch size -> worst |dlogit|"""
    m = _model(cfg)
    text = m.describe_plan()
    assert m.feature_clamp == 0.0
    assert text.count(attn) == cfg.n_blocks and sum(text.count(k) for k in ("mha_h2:", "mha_mfma:", "mha_core:")) == cfg.n_blocks, text
    if ffn_fused:
        assert text.count("ffn_x3:") == cfg.n_blocks and text.count("post-norm") == cfg.n_blocks and text.count("+time sums") == 1, text
        assert text.count("mean_finish:") == 1 and "layernorm" not in text, text
    else:
        assert "ffn_x3:" not in text and "mean_finish:" not in text and "layernorm:" in text and "layernorm+mean:" in text, text
    sd = synth_state_dict(cfg)
    worst = 0.0
    for B in batches:
        fx = synth_features(B, cfg.input_shape, seed=B)
        lg, _, emb = m.forward_features(fx, return_embedding=True)
        e_ref = oracle.head_forward(fx, sd, cfg, dtype=np.float64)                  # the encoder evaluated once
        ref = oracle.classify(e_ref, sd, cfg, dtype=np.float64).ravel()
        assert np.isfinite(lg).all()
        worst = max(worst, float(np.abs(lg - ref).max()))
        assert np.abs(lg - ref).max() <= LOGIT_ATOL, (B, float(np.abs(lg - ref).max()), text)
        assert np.abs(emb - e_ref).max() <= EMB_RTOL * max(1.0, np.abs(e_ref).max()), (B, float(np.abs(emb - e_ref).max()))
    m.close()
    return worst


@pytest.mark.parametrize("D,heads", [(32, 4), (80, 4), (96, 4), (112, 4), (144, 4), (160, 4), (192, 4), (256, 4), (64, 16)])
def test_exact_subtraction_attention_head_dims(D, heads):
    """mha_h2's exact-subtraction instances at head dims 8, 20, 24, 28, 36, 40, 48, 64 and 4 (12, 16, 32 run in the goldens), T = 33: two
    key tiles, the second ragged.  Widths without a fused feed-forward run the fallback around the same attention kernel."""
    cfg = HeadConfig("transformer", (33, 32), n_blocks=2, embedding_dim=32, transformer_d_model=D, transformer_n_head=heads)
    worst = _check_against_float64(cfg, "mha_h2:", D in FFN_WIDTHS)
    print("head dim", D // heads, "D", D, "max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7, 31, 32, 33, 64, 65, 127, 128])
@pytest.mark.parametrize("D,blocks", [(D, 1) for D in FFN_WIDTHS] + [(96, 2), (144, 2)])
def test_post_norm_ffn_widths_and_clip_lengths(D, blocks, T):
    """The post-norm ffn_x3 at every compiled width x the clip lengths that decide its time sums: many clips per 32-row tile (T = 1 .. 31,
    ffn_x3_post_nseg(T) segments), a clip that ends on a tile's last row or one row into the next (32, 33, 64, 65, 127, 128); with two blocks
    the first stores its rows and the last sums them."""
    cfg = HeadConfig("transformer", (T, 32), n_blocks=blocks, embedding_dim=32, transformer_d_model=D, transformer_n_head=4)
    worst = _check_against_float64(cfg, "mha_h2:", True)
    print("D", D, "blocks", blocks, "T", T, "max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("T,D,heads,attn", [(129, 128, 4, "mha_core:"), (200, 128, 4, "mha_core:"), (33, 144, 8, "mha_core:")],
                         ids=["T129", "T200", "head_dim_18"])
def test_beyond_the_attention_kernels(T, D, heads, attn):
    """T > 128 (mha_h2_supported says no) and a head dim outside the compiled set: the attention falls to mha_core, the rest stays fused."""
    cfg = HeadConfig("transformer", (T, 32), n_blocks=2, embedding_dim=32, transformer_d_model=D, transformer_n_head=heads)
    worst = _check_against_float64(cfg, attn, True, batches=(1, 3, 33))
    print("T", T, "D", D, "heads", heads, "max |dlogit| vs float64: %.2e" % worst)


def top_two_score_gaps(x, sd, cfg):
    """float64: per block, the smallest gap between the two largest scaled scores q.k / sqrt(dh) of any (clip, head, query), relative
    to max(1, the row's largest |score|) - how far the softmax rows are from a tie in their argmax, in units of the scores' own
    rounding (a one-hot softmax flips on a near-tie in any float32 arithmetic)."""
    f8 = np.float64
    w = {k: np.asarray(v, f8) for k, v in sd.items()}
    D, nh, T = cfg.transformer_d_model, cfg.transformer_n_head, x.shape[1]
    h = transformer_input(np.asarray(x, f8), w, cfg)
    gaps = []
    for i in range(cfg.n_blocks):
        p = f"model.transformer_encoder.layers.{i}"
        qkv = h @ w[p + ".self_attn.in_proj_weight"].T + w[p + ".self_attn.in_proj_bias"]
        q, k = (qkv[..., j * D:(j + 1) * D].reshape(len(x), T, nh, D // nh).transpose(0, 2, 1, 3) for j in range(2))
        s = np.sort(q @ k.transpose(0, 1, 3, 2) / np.sqrt(f8(D // nh)), axis=-1)
        top = np.maximum(1.0, np.maximum(np.abs(s[..., 0]), np.abs(s[..., -1])))
        gaps.append(float(((s[..., -1] - s[..., -2]) / top).min()) if T > 1 else float("inf"))
        h = transformer_layer(h, w, p, nh)
    return gaps


def _peaked(sd, cfg, s):
    """the q and k rows of every in_proj x s: raw scores x s^2"""
    D = cfg.transformer_d_model
    out = {k: np.array(v, np.float32, copy=True) for k, v in sd.items()}
    for i in range(cfg.n_blocks):
        p = f"model.transformer_encoder.layers.{i}.self_attn.in_proj_"
        out[p + "weight"][:2 * D] *= np.float32(s)
        out[p + "bias"][:2 * D] *= np.float32(s)
    return out


@pytest.mark.parametrize("s,loud_row", [(8.0, False), (64.0, False), (512.0, False), (1.0, True)], ids=["x2^3", "x2^6", "x2^9", "row_x1e4"])
def test_peaked_softmax(s, loud_row):
    """What the exact-subtraction form is for: raw scores far above the softmax's range.  The default model with its q and k rows x 2^3,
    2^6, 2^9 (scores x 2^6 .. 2^18: the softmax is one-hot), and - nothing clamps the features - one frame of one clip x 1e4 on the plain
    weights: finite, and within LOGIT_ATOL of float64 relative to max(1, |ref|).

    A near-tie in a row's argmax flips a one-hot softmax in ANY float32 arithmetic, so the clips (seed 31) are ones whose closest top-two
    scores, in float64, are >= 1e-4 of the row's largest score apart (measured 1.03e-4, the same at every scale; 400 ulps of the
    two-term binary16 form); the loud frame is not combined with the scaled weights - in that clip the top two keys of some queries sit 1e-7
    of the score apart, a tie at float32's own resolution.  The float32 restatement itself is 4.4e-7 (6.4e-7 for the loud frame) from
    float64 on these inputs, and the test asserts that first: the case is well-conditioned before the kernel is judged on it."""
    cfg = HeadConfig("transformer", (101, 64))
    sd = _peaked(synth_state_dict(cfg), cfg, s)
    x = synth_features(6, cfg.input_shape, seed=31)
    if loud_row:
        x[1, 7] *= np.float32(1e4)
    else:
        assert min(top_two_score_gaps(x, sd, cfg)) >= 1e-4
    ref = oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
    tol = LOGIT_ATOL * np.maximum(1.0, np.abs(ref))
    assert np.all(np.abs(oracle.model_forward(x, sd, cfg).ravel() - ref) <= 0.1 * tol)
    from nanowakeword_amd.session import HipModel
    m = HipModel(cfg, FrontendConfig(), state_dict=sd)
    assert m.feature_clamp == 0.0 and "mha_h2:" in m.describe_plan() and "post-norm" in m.describe_plan(), m.describe_plan()
    lg, _ = m.forward_features(x)
    assert np.isfinite(lg).all(), lg
    print("peaked softmax x", s, "loud row", loud_row, "max |dlogit| / max(1, |ref|) vs float64: %.2e" % float((np.abs(lg - ref) / np.maximum(1.0, np.abs(ref))).max()))
    assert np.all(np.abs(lg - ref) <= tol), (lg, ref)
    m.close()


def test_batch_invariance_many_clips_per_tile():
    """T = 5: a 32-row tile holds rows of up to eight clips (ffn_x3_post_nseg(5) = 8 segments) and clip 6 straddles the first tile's edge;
    B = 4099 leaves a ragged last tile.  A clip alone equals the clip in the batch, bit for bit."""
    cfg = HeadConfig("transformer", (5, 32), embedding_dim=32, transformer_d_model=64, transformer_n_head=4)
    m = _model(cfg)
    assert "mha_h2:" in m.describe_plan() and "mean_finish:" in m.describe_plan(), m.describe_plan()
    B = 4099
    x = synth_features(B, cfg.input_shape, seed=11)
    full, _ = m.forward_features(x)
    for i in (0, 6, 7, B - 1):
        alone, _ = m.forward_features(np.ascontiguousarray(x[i:i + 1]))
        assert alone[0] == full[i], (i, alone[0], full[i])
    ref = oracle.model_forward(x[:40], synth_state_dict(cfg), cfg, dtype=np.float64).ravel()
    assert np.abs(full[:40] - ref).max() <= LOGIT_ATOL
    m.close()
