"""TCN head on the HIP path (run with -m gpu): reference goldens, ragged batches, the PCM composite, ONNX / .pt ingestion through the
session and the interpreter, the one-launch plan at the reference defaults, the generic fallback, batch invariance, the unclamped loud
frame and the receptive-field cone."""
import json
import os

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from parity import logit_bounds
from tcn_oracle import receptive_field, tcn_head, tcn_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOGIT_ATOL = 1e-4
LOGIT_ULPS = 2.4e-7        # + two float32 ulps of the logit: the loud-frame clip's logit is ~7e3, where float32 spacing is 5e-4
EMB_RTOL = 1e-4


def _cfg(meta):
    m = dict(meta)
    m["input_shape"] = tuple(m["input_shape"])
    return HeadConfig(**m)


def _close(got, ref):
    got, ref = np.ravel(got), np.ravel(ref)
    return np.all(np.abs(got - ref) <= LOGIT_ATOL + LOGIT_ULPS * np.abs(ref))


@pytest.fixture(scope="module")
def golden():
    d = dict(np.load(os.path.join(GOLDEN, "heads_tcn.npz"), allow_pickle=False))
    return d, json.loads(str(d["meta_json"]))


def _model(cfg, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg), **kw)


def _golden_names():
    d = np.load(os.path.join(GOLDEN, "heads_tcn.npz"), allow_pickle=False)
    return sorted(json.loads(str(d["meta_json"])))


def _plan(m):
    # the head's launches (the frontend runs for PCM input only; the sigmoid rides in the tail)
    return [l for l in m.describe_plan().strip().split("\n") if l.strip() and not l.startswith(("frontend:", "unary:sigmoid"))]


@pytest.mark.parametrize("name", _golden_names())
def test_features_vs_reference(golden, name):
    d, meta = golden
    cfg = _cfg(meta[name])
    m = _model(cfg)
    assert m.feature_clamp == 0.0, m.describe_plan()
    feats = d[f"{name}/feats"]
    logits, probs, emb = m.forward_features(feats, return_embedding=True)
    ref, ref_e = d[f"{name}/logits_feat"].ravel(), d[f"{name}/emb_feat"]
    assert _close(logits, ref), (name, logits, ref, m.describe_plan())
    assert np.abs(emb - ref_e).max() <= EMB_RTOL * max(1.0, np.abs(ref_e).max()), (name, np.abs(emb - ref_e).max())
    assert np.abs(probs - oracle.sigmoid(ref)).max() <= 1e-5
    # ragged batches (partial workgroups of clips) against the restatement
    sd = synth_state_dict(cfg)
    for B in (1, 3, 33, 70):
        fx = synth_features(B, cfg.input_shape, seed=B)
        lg, _ = m.forward_features(fx)
        lo = tcn_model(fx, sd, cfg).ravel()
        assert _close(lg, lo), (name, B, np.abs(lg - lo).max())
    m.close()


def test_loud_frame_is_not_clamped(golden):
    d, meta = golden
    cfg = _cfg(meta["tcn_16x96_outlier"])
    m = _model(cfg)
    assert m.feature_clamp == 0.0 and "tcn_x3:" in m.describe_plan()
    lg, _ = m.forward_features(d["tcn_16x96_outlier/feats"])
    ref = d["tcn_16x96_outlier/logits_feat"].ravel()
    assert abs(ref[1]) > 1e3 and _close(lg, ref), (lg, ref)
    # the other clips of the batch are those of the plain case, bit for bit
    plain, _ = m.forward_features(d["tcn_16x96/feats"])
    assert np.array_equal(plain[[0, 2, 3]], lg[[0, 2, 3]])
    m.close()


def test_pcm_vs_reference(golden, golden_frontend):
    from nanowakeword_amd.session import HipModel
    d, meta = golden
    g = golden_frontend
    name = "tcn_101x64"
    cfg = _cfg(meta[name])
    sd = synth_state_dict(cfg)
    m = HipModel(cfg, FrontendConfig(), state_dict=sd, window=g["window"], mel_fb=g["fb64"])
    assert "tcn_x3:" in m.describe_plan()
    rp = d[f"{name}/logits_pcm"].ravel()
    lp, pp = m.forward_pcm(g["pcm"])
    lm32 = oracle.frontend_logmel(g["pcm"], g["window"], g["fb64"], center=True).transpose(0, 2, 1)
    lm64 = oracle.frontend_logmel(g["pcm"], g["window"], g["fb64"], center=True, dtype=np.float64).astype(np.float32).transpose(0, 2, 1)
    l32 = tcn_model(np.ascontiguousarray(lm32), sd, cfg).ravel()
    lx = tcn_model(np.ascontiguousarray(lm64), sd, cfg).ravel()
    # the head on the device frontend's own log-mel agrees with the restatement on the same features at 1e-4 ...
    feats = np.ascontiguousarray(m.frontend(g["pcm"]).transpose(0, 2, 1))
    lf = tcn_model(feats, sd, cfg).ravel()
    assert np.abs(m.forward_features(feats)[0] - lf).max() <= LOGIT_ATOL
    # ... and the composite is within 1e-4 (plus the tonal clips' float32 noise) of the reference once the frontend's own deviation from
    # the exact frontend is carried through the exact head: the TCN normalises nothing, so a 0.015 dB difference in the near-silent
    # bins of one recording moves its logit by 1.4e-4 on every arithmetic
    bound = logit_bounds(g["names"], rp, l32, lx) + np.abs(lf - lx)
    err = np.abs(lp - rp)
    assert np.all(err <= bound), [f"{n}: {e:.2e} > {b:.2e}" for n, e, b in zip(g["names"], err, bound) if e > b]
    assert np.abs(pp - oracle.sigmoid(lp)).max() <= 1e-6
    m.close()


def test_onnx_pt_and_interpreter(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.interpreter import HipInterpreter
    from nanowakeword_amd.weights import infer_head_config, load_session, save_bundle, state_dict_from_pt
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_tcn.npz"), allow_pickle=False))
    feats, want = e["tcn/feats"], e["tcn/probs"]
    onnx = os.path.join(GOLDEN, "onnx", "tcn.onnx")
    s = load_session(onnx)
    assert np.abs(s.run(None, {"input": feats})[0].reshape(-1) - want).max() <= 1e-5
    class Pre:                                              # AudioFeatures protocol with scripted features: one clip's frames
        def __init__(self, clip):
            self.feature_buffer = clip

        def __call__(self, x):
            return len(x)

        def get_features(self, n):
            return self.feature_buffer[-n:][None]

        def reset(self):
            pass

    for i in range(len(feats)):
        it = HipInterpreter.load_model(onnx, preprocessor=Pre(feats[i]))
        assert list(it.models) == ["tcn"]
        for _ in range(3):
            it.predict(np.zeros(1280, np.int16))
        assert abs(it.raw_scores["tcn"] - want[i]) <= 1e-5, (i, it.raw_scores, want[i])
    # a .pt of the same weights -> bundle -> session
    cfg = _cfg(json.loads(str(e["meta_json"]))["tcn"])
    pt = str(tmp_path / "tcn.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}, pt)
    sd = state_dict_from_pt(pt)
    c = infer_head_config(sd, input_shape=cfg.input_shape)
    assert c == cfg
    bundle = str(tmp_path / "tcn_pt.nww.npz")
    save_bundle(bundle, c, sd, mode="features")
    s2 = load_session(bundle)
    assert np.abs(s2.run(None, {"input": feats})[0].reshape(-1) - want).max() <= 1e-5


@pytest.mark.parametrize("cfg", [HeadConfig("tcn", (16, 96)), HeadConfig("tcn", (101, 64)), HeadConfig("tcn", (98, 40)),
                                 HeadConfig("tcn", (16, 96), tcn_channels=[128, 128, 256, 256], tcn_kernel_size=4)],
                         ids=["16x96", "101x64", "98x40", "guide_16x96"])
def test_plan_is_one_launch(cfg):
    m = _model(cfg)
    plan = _plan(m)
    text = "\n".join(plan)
    assert m.feature_clamp == 0.0
    assert len(plan) == 2 and plan[0].startswith("tcn_x3:") and plan[1].startswith("tail:fc+classifier"), text
    assert "gemm:" not in text and "im2col:" not in text, text
    m.close()


@pytest.mark.parametrize("cfg,kw", [
    (HeadConfig("tcn", (16, 96)), {"conv_arith": "bf16x6"}),
    (HeadConfig("tcn", (101, 64)), {"conv_arith": "f32"}),
    (HeadConfig("tcn", (33, 40), tcn_channels=[24, 40]), {}),
    (HeadConfig("tcn", (20, 12), embedding_dim=32, tcn_channels=[16, 16, 32], tcn_kernel_size=2), {}),
    (HeadConfig("tcn", (101, 64), tcn_channels=[128, 128, 256, 256], tcn_kernel_size=4), {}),    # a 91-step cone: more than the LDS holds
], ids=["bf16x6", "f32", "odd_widths", "k2", "guide_101x64"])
def test_fallback_matches_restatement(cfg, kw):
    m = _model(cfg, **kw)
    text = m.describe_plan()
    assert "tcn_x3:" not in text and "im2col:" in text and "gemm:" in text and "last_row:" in text, text
    sd = synth_state_dict(cfg)
    fx = synth_features(37, cfg.input_shape, seed=5)
    lg, _, emb = m.forward_features(fx, return_embedding=True)
    assert _close(lg, tcn_model(fx, sd, cfg)), np.abs(lg - tcn_model(fx, sd, cfg).ravel()).max()
    e_or = tcn_head(fx, sd, cfg)
    assert np.abs(emb - e_or).max() <= EMB_RTOL * max(1.0, np.abs(e_or).max())
    m.close()


@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_fused_agrees_with_fallback(shape):
    cfg = HeadConfig("tcn", shape)
    fused, generic = _model(cfg), _model(cfg, conv_arith="bf16x9")
    assert "tcn_x3:" in fused.describe_plan() and "tcn_x3:" not in generic.describe_plan()
    fx = synth_features(300, shape, seed=8)
    a, _ = fused.forward_features(fx)
    b, _ = generic.forward_features(fx)
    assert _close(a, b), np.abs(a - b).max()
    fused.close(); generic.close()


@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_batch_invariance(shape):
    cfg = HeadConfig("tcn", shape)
    m = _model(cfg)
    B = 4096
    x = synth_features(B, shape, seed=11)
    full, _ = m.forward_features(x)
    for i in (0, 1, 5, 1000, B - 1):
        alone, _ = m.forward_features(np.ascontiguousarray(x[i:i + 1]))
        assert alone[0] == full[i], (shape, i, alone[0], full[i])
    # the same clip at other offsets of a large batch
    y = np.ascontiguousarray(np.roll(x, 7, axis=0))
    rolled, _ = m.forward_features(y)
    assert np.array_equal(rolled, np.roll(full, 7))
    ref = tcn_model(x[:8], synth_state_dict(cfg), cfg).ravel()
    assert _close(full[:8], ref)
    m.close()


def test_cone_only():
    """Rows older than the last step's receptive field are never read: 1e30 there leaves every logit bit-identical."""
    cfg = HeadConfig("tcn", (101, 64))
    R = receptive_field(cfg)
    m = _model(cfg)
    assert "tcn_x3:" in m.describe_plan() and f"last {R} steps" in m.describe_plan()
    x = synth_features(70, cfg.input_shape, seed=3)
    y = x.copy()
    y[:, : 101 - R] = 1e30
    a, _ = m.forward_features(x)
    b, _ = m.forward_features(y)
    assert np.array_equal(a, b)
    assert _close(a, tcn_model(x, synth_state_dict(cfg), cfg))
    m.close()
