"""TCN head on the HIP path (run with -m gpu): reference goldens, ragged batches, the PCM composite, ONNX / .pt ingestion through the
session and the interpreter, the one-launch plan at the reference defaults, the generic fallback, batch invariance, the unclamped loud
frame and the receptive-field cone; every instance of the fused kernel (cones across 32-row tiles, tap counts, depths, widths, the
degenerate clip lengths) against the float64 restatement."""
import json
import os

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from oracle import tcn_receptive_field
from parity import GOLDEN, assert_pcm_logits_vs_reference, head_golden_names, load_head_goldens

pytestmark = pytest.mark.gpu

LOGIT_ATOL = 1e-4
LOGIT_ULPS = 2.4e-7        # + two float32 ulps of the logit: the loud-frame clip's logit is ~7e3, where float32 spacing is 5e-4
EMB_RTOL = 1e-4


def _close(got, ref):
    got, ref = np.ravel(got), np.ravel(ref)
    return np.all(np.abs(got - ref) <= LOGIT_ATOL + LOGIT_ULPS * np.abs(ref))


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_tcn.npz")


def _model(cfg, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg), **kw)


def _plan(m):
    # the head's launches (the frontend runs for PCM input only; the sigmoid rides in the tail)
    return [l for l in m.describe_plan().strip().split("\n") if l.strip() and not l.startswith(("frontend:", "unary:sigmoid"))]


@pytest.mark.parametrize("name", head_golden_names("heads_tcn.npz"))
def test_features_vs_reference(golden, name):
    d, meta = golden
    cfg = HeadConfig(**meta[name])
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
        lo = oracle.model_forward(fx, sd, cfg).ravel()
        assert _close(lg, lo), (name, B, np.abs(lg - lo).max())
    m.close()


def test_loud_frame_is_not_clamped(golden):
    d, meta = golden
    cfg = HeadConfig(**meta["tcn_16x96_outlier"])
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
    cfg = HeadConfig(**meta[name])
    sd = synth_state_dict(cfg)
    m = HipModel(cfg, FrontendConfig(), state_dict=sd, window=g["window"], mel_fb=g["fb64"])
    assert "tcn_x3:" in m.describe_plan()
    # the head on the device frontend's own log-mel agrees with the restatement on the same features at 1e-4 ...
    feats = np.ascontiguousarray(m.frontend(g["pcm"]).transpose(0, 2, 1))
    lf = oracle.model_forward(feats, sd, cfg).ravel()
    assert np.abs(m.forward_features(feats)[0] - lf).max() <= LOGIT_ATOL
    # ... and the composite is within 1e-4 (plus the tonal clips' float32 noise) of the reference once the frontend's own deviation from
    # the exact frontend is carried through the exact head: the TCN normalises nothing, so a 0.015 dB difference in the near-silent
    # bins of one recording moves its logit by 1.4e-4 on every arithmetic
    lp, pp, _, _ = assert_pcm_logits_vs_reference(m, cfg, sd, g, g["pcm"], d[f"{name}/logits_pcm"].ravel(), extra=lambda lx: np.abs(lf - lx), what=name)
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
    cfg = HeadConfig(**json.loads(str(e["meta_json"]))["tcn"])
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
    assert _close(lg, oracle.model_forward(fx, sd, cfg)), np.abs(lg - oracle.model_forward(fx, sd, cfg).ravel()).max()
    e_or = oracle.head_forward(fx, sd, cfg)
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
    ref = oracle.model_forward(x[:8], synth_state_dict(cfg), cfg).ravel()
    assert _close(full[:8], ref)
    m.close()


def test_cone_only():
    """Rows older than the last step's receptive field are never read: 1e30 there leaves every logit bit-identical."""
    cfg = HeadConfig("tcn", (101, 64))
    R = tcn_receptive_field(cfg)
    m = _model(cfg)
    assert "tcn_x3:" in m.describe_plan() and f"last {R} steps" in m.describe_plan()
    x = synth_features(70, cfg.input_shape, seed=3)
    y = x.copy()
    y[:, : 101 - R] = 1e30
    a, _ = m.forward_features(x)
    b, _ = m.forward_features(y)
    assert np.array_equal(a, b)
    assert _close(a, oracle.model_forward(x, synth_state_dict(cfg), cfg))
    m.close()


# (T, F, channels, k): every family of tcn_x3's launch plan (tcn_x3_plan: S = min(T, R) cone rows per clip, NC = 32 RT / S clips per
# workgroup, instance <1> for widths <= 128 and <2> up to 256, where the input's padded width counts as a width)
_FUSED = [
    # the cone spans two or three 32-row tiles: dilated taps reach across tile boundaries
    (101, 64, [64, 64, 128], 4), (101, 64, [64, 64, 128], 5), (101, 64, [64, 64, 128, 128], 3), (101, 64, [128, 128, 128, 128], 4),
    (91, 64, [128, 128, 128, 128], 4),                       # T == R exactly
    (60, 64, [128, 128, 128, 128], 4),                       # T < R: S = 60
    (64, 40, [32, 64, 64, 128], 3),
    # taps and depth
    (16, 96, [64], 8), (50, 40, [32, 96], 6), (20, 41, [64, 64, 128, 128], 2),
    # widths: narrowing downsamples, instance <2> (by the channels, and by the input width alone), identity residuals under a wider input
    (40, 100, [128, 64, 32], 3), (16, 200, [160, 224], 2), (33, 200, [64, 64], 3), (16, 96, [96, 192, 256], 2), (30, 33, [32, 32], 3),
    # degenerate: one step (96 clips per workgroup), two steps
    (1, 96, [64, 64, 128], 3), (2, 12, [32], 2),
]


def fused_plan(cfg):
    """The fused kernel's launch plan restated (tcn_x3_plan in tcn_x3.hip): None where the stack goes to the im2col + GEMM fallback,
    else S (cone rows kept per clip), RT (32-row tiles per workgroup), NC (clips per workgroup) and the instance (1: widths <= 128,
    2: <= 256).  Tests assert the plan's own text; this is for the batch sizes and clips they pick around NC."""
    T, F = cfg.input_shape
    L, k = len(cfg.tcn_channels), cfg.tcn_kernel_size
    if not 1 <= L <= 4 or k < 2 or T < 1 or F < 1 or any(c <= 0 or c % 32 or c > 256 for c in cfg.tcn_channels):
        return None
    cmax = max([(F + 15) // 16 * 16] + list(cfg.tcn_channels))
    if cmax > 256:
        return None
    S, ld = min(T, tcn_receptive_field(cfg)), cmax + 4
    for rt in range(3 if cmax <= 128 else 1, 0, -1):
        if 32 * rt >= S and 3 * 32 * rt * (ld + 1) * 4 <= 160 * 1024:
            return {"S": S, "RT": rt, "NC": 32 * rt // S, "instance": 1 if cmax <= 128 else 2}
    return None


def _fused_id(c):
    return "%dx%d-%s-k%d" % (c[0], c[1], "_".join(map(str, c[2])), c[3])


@pytest.mark.parametrize("T,F,ch,k", _FUSED, ids=[_fused_id(c) for c in _FUSED])
def test_fused_instances_against_float64(T, F, ch, k):
    """Each case must plan onto tcn_x3 (a case that lands on the fallback fails) and agree, logits and embeddings, with the float64
    restatement and with the im2col + GEMM fallback (conv_arith = bf16x9) at batch sizes around the workgroup's clip count; a clip's
    logit does not depend on the batch it travels in, at the workgroup seams (clips NC - 1, NC) in particular."""
    cfg = HeadConfig("tcn", (T, F), tcn_channels=ch, tcn_kernel_size=k)
    S = min(T, tcn_receptive_field(cfg))
    fp = fused_plan(cfg)
    assert fp is not None and fp["S"] == S, (fp, S)
    NC = fp["NC"]
    fused, generic = _model(cfg), _model(cfg, conv_arith="bf16x9")
    text = fused.describe_plan()
    assert "tcn_x3:" in text and f"last {S} steps of {T}" in text and "im2col:" not in text, text
    assert "tcn_x3:" not in generic.describe_plan() and "im2col:" in generic.describe_plan(), generic.describe_plan()
    sd = synth_state_dict(cfg)
    worst = 0.0
    for B in ((1, 95, 96, 97, 300) if T == 1 else (1, NC + 1, 70, 300)):
        fx = synth_features(B, cfg.input_shape, seed=B)
        lg, _, emb = fused.forward_features(fx, return_embedding=True)
        e_ref = oracle.head_forward(fx, sd, cfg, dtype=np.float64)                  # the stack evaluated once
        ref = oracle.classify(e_ref, sd, cfg, dtype=np.float64).ravel()
        worst = max(worst, float((np.abs(lg - ref) / np.maximum(1.0, np.abs(ref))).max()))
        assert np.isfinite(lg).all()
        assert _close(lg, ref), (B, float(np.abs(lg - ref).max()), float(np.abs(ref).max()))
        assert np.abs(emb - e_ref).max() <= EMB_RTOL * max(1.0, np.abs(e_ref).max()), (B, float(np.abs(emb - e_ref).max()))
        lb, _ = generic.forward_features(fx)
        assert _close(lg, lb), (B, float(np.abs(lg - lb).max()))
        for i in sorted({0, NC - 1, NC, B - 1}):
            if 0 <= i < B:
                alone, _ = fused.forward_features(np.ascontiguousarray(fx[i:i + 1]))
                assert alone[0] == lg[i], (B, i, alone[0], lg[i])
    print(_fused_id((T, F, ch, k)), "S", S, "NC", NC, "instance", fp["instance"], "max |dlogit| / max(1, |logit|) vs float64: %.2e" % worst)
    fused.close(); generic.close()


def test_long_cone_reads_exactly_its_rows():
    """A cone of 91 rows (three 32-row tiles): rows older than it are never read (1e30 there leaves every logit bit-identical), and the
    rows inside it ARE read - its first row and its last, changed one at a time, change every clip's logit as the float64 restatement says
    they must (a kernel that reads a shorter cone than the plan states passes the first half alone)."""
    T = 101
    cfg = HeadConfig("tcn", (T, 64), tcn_channels=[128, 128, 128, 128], tcn_kernel_size=4)
    R = tcn_receptive_field(cfg)
    assert R == 91
    m = _model(cfg)
    assert "tcn_x3:" in m.describe_plan() and f"last {R} steps" in m.describe_plan()
    sd = synth_state_dict(cfg)
    x = synth_features(70, cfg.input_shape, seed=3)
    a, _ = m.forward_features(x)
    assert _close(a, oracle.model_forward(x, sd, cfg, dtype=np.float64))
    y = x.copy()
    y[:, : T - R] = 1e30
    b, _ = m.forward_features(y)
    assert np.array_equal(a, b)
    base = oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
    # the oldest row reaches the last step through the oldest tap of all eight convs only: + 3000 there moves every logit by >= 0.028
    # in float64 (+ 300 on the newest row: >= 6), ten times the tolerance and more, so a kernel that drops the row cannot pass
    for row, amp in ((T - R, 3000.0), (T - 1, 300.0)):
        z = x.copy()
        z[:, row] += np.float32(amp)
        want = oracle.model_forward(z, sd, cfg, dtype=np.float64).ravel()
        assert np.all(np.abs(want - base) > 10 * LOGIT_ATOL), (row, np.abs(want - base).min())     # the row matters in exact arithmetic
        c, _ = m.forward_features(z)
        assert np.all(c != a), (row, int((c == a).sum()))
        assert _close(c, want), (row, float(np.abs(c - want).max()))
    m.close()
