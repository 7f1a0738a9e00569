"""Transformer head on the HIP path (run with -m gpu): reference goldens, the PCM composite, ONNX / .pt ingestion through the session,
the launch plan at the reference defaults, the generic fallback, batch invariance and the unclamped input projection."""
import json
import os

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from parity import logit_bounds
from transformer_oracle import transformer_head, transformer_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOGIT_ATOL = 1e-4
EMB_RTOL = 1e-4


def _cfg(meta):
    m = dict(meta)
    m["input_shape"] = tuple(m["input_shape"])
    return HeadConfig(**m)


@pytest.fixture(scope="module")
def golden():
    d = dict(np.load(os.path.join(GOLDEN, "heads_transformer.npz"), allow_pickle=False))
    return d, json.loads(str(d["meta_json"]))


def _model(cfg, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg), **kw)


def _golden_names():
    d = np.load(os.path.join(GOLDEN, "heads_transformer.npz"), allow_pickle=False)
    return sorted(json.loads(str(d["meta_json"])))


@pytest.mark.parametrize("name", _golden_names())
def test_features_vs_reference(golden, name):
    d, meta = golden
    cfg = _cfg(meta[name])
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
        lo = transformer_model(fx, sd, cfg).ravel()
        assert np.abs(lg - lo).max() <= LOGIT_ATOL, (name, B, np.abs(lg - lo).max())
    m.close()


def test_pcm_vs_reference(golden, golden_frontend):
    from nanowakeword_amd.session import HipModel
    d, meta = golden
    g = golden_frontend
    name = "transformer_101x64"
    cfg = _cfg(meta[name])
    sd = synth_state_dict(cfg)
    m = HipModel(cfg, FrontendConfig(), state_dict=sd, window=g["window"], mel_fb=g["fb64"])
    rp = d[f"{name}/logits_pcm"].ravel()
    lp, pp = m.forward_pcm(g["pcm"])
    lm32 = oracle.frontend_logmel(g["pcm"], g["window"], g["fb64"], center=True).transpose(0, 2, 1)
    lm64 = oracle.frontend_logmel(g["pcm"], g["window"], g["fb64"], center=True, dtype=np.float64).astype(np.float32).transpose(0, 2, 1)
    l32 = transformer_model(np.ascontiguousarray(lm32), sd, cfg).ravel()
    lx = transformer_model(np.ascontiguousarray(lm64), sd, cfg).ravel()
    bound = logit_bounds(g["names"], rp, l32, lx)
    err = np.abs(lp - rp)
    assert np.all(err <= bound), [f"{n}: {e:.2e} > {b:.2e}" for n, e, b in zip(g["names"], err, bound) if e > b]
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
    cfg = _cfg(json.loads(str(e["meta_json"]))["transformer"])
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
    e_or = transformer_head(fx, sd, cfg)
    assert np.abs(lg - transformer_model(fx, sd, cfg).ravel()).max() <= LOGIT_ATOL
    assert np.abs(emb - e_or).max() <= EMB_RTOL * max(1.0, np.abs(e_or).max())
    m.close()
    # 12 input features: no short-K instance - the general GEMM, then the scale and the positional rows in one elementwise pass
    cfg = HeadConfig("transformer", (8, 12), embedding_dim=16, transformer_d_model=32, transformer_n_head=2)
    m = _model(cfg)
    assert "gemm:input_proj" in m.describe_plan() and "scale+pe:" in m.describe_plan()
    fx = synth_features(9, cfg.input_shape, seed=6)
    assert np.abs(m.forward_features(fx)[0] - transformer_model(fx, synth_state_dict(cfg), cfg).ravel()).max() <= LOGIT_ATOL
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
    ref = transformer_model(x[:8], synth_state_dict(cfg), cfg).ravel()
    assert np.abs(full[:8] - ref).max() <= LOGIT_ATOL
    m.close()


def test_create_validates_heads():
    from nanowakeword_amd.session import HipModel
    with pytest.raises(Exception, match="transformer_d_model must be divisible by transformer_n_head"):
        HipModel(HeadConfig("transformer", (16, 96), transformer_d_model=100, transformer_n_head=3), FrontendConfig())
    with pytest.raises(Exception, match="head_dim"):
        HipModel(HeadConfig("transformer", (16, 96), transformer_d_model=260, transformer_n_head=2), FrontendConfig())
