"""RNN head (bi-LSTM of hidden size 64) on the HIP path (run with -m gpu): reference goldens, the PCM composite, every instance of the
input projection fused into the recurrence (rnn_x3_kernel<4, 64, 3, 1, FIN>) at its smallest shapes against the float64 restatement
(tests/rnn_oracle.py), batch invariance, the routes that keep the precomputed gate pre-activations, feature magnitudes and the clamp,
ONNX / .pt ingestion through the session and the interpreter."""
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

import oracle
import rnn_oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from parity import GOLDEN, assert_pcm_logits_vs_reference, head_golden_names, load_head_goldens

pytestmark = pytest.mark.gpu

LOGIT_ATOL = 1e-4
LOGIT_ULPS = 2.4e-7        # + two float32 ulps of the logit
EMB_RTOL = 1e-4
FUSED = "+ input projection [f16x3]"
FORWARD_IH = r"(lin_x3|gemm):model\.layer1\.ih_l0( |$)"      # the forward direction's input projection as a launch of its own


def _err(got, ref):
    """|got - ref| in units of the tolerance LOGIT_ATOL + LOGIT_ULPS |ref| (<= 1 passes)."""
    got, ref = np.ravel(got).astype(np.float64), np.ravel(ref).astype(np.float64)
    return float((np.abs(got - ref) / (LOGIT_ATOL + LOGIT_ULPS * np.abs(ref))).max())


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_rnn.npz")


def _model(cfg, sd=None, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg) if sd is None else sd, **kw)


def _assert_xg_route(text):
    """The generic route: the forward direction's input projection is a launch of its own (lin_x3 / GEMM) in front of the recurrence."""
    assert "+ input projection" not in text and "lstm:model.layer1_l" in text, text
    assert re.search(FORWARD_IH, text, re.M), text


@pytest.mark.parametrize("name", head_golden_names("heads_rnn.npz"))
def test_features_vs_reference(golden, name):
    d, meta = golden
    cfg = HeadConfig(**meta[name])
    m = _model(cfg)
    text = m.describe_plan()
    if name in ("rnn_16x96", "rnn_101x64", "rnn_7x64_gelu"):
        assert f"lstm:model.layer1_l0 + first reverse step {FUSED}" in text and m.feature_clamp > 0, text
        assert not re.search(FORWARD_IH, text, re.M), text
    else:
        _assert_xg_route(text)
    assert "tail:layer2+classifier" in text, text
    feats = d[f"{name}/feats"]
    logits, probs, emb = m.forward_features(feats, return_embedding=True)
    ref, ref_e = d[f"{name}/logits_feat"].ravel(), d[f"{name}/emb_feat"]
    print(name, "vs reference: %.3f of the tolerance, |demb| %.2e" % (_err(logits, ref), np.abs(emb - ref_e).max()))
    assert _err(logits, ref) <= 1.0, (name, logits, ref, text)
    assert np.abs(emb - ref_e).max() <= EMB_RTOL * max(1.0, np.abs(ref_e).max()), (name, np.abs(emb - ref_e).max())
    assert np.abs(probs - oracle.sigmoid(ref)).max() <= 1e-5
    m.close()


def test_pcm_vs_reference(golden, golden_frontend, monkeypatch):
    from nanowakeword_amd.session import HipModel
    d, meta = golden
    g = golden_frontend
    name = "rnn_101x64"
    cfg = HeadConfig(**meta[name])
    sd = synth_state_dict(cfg)
    m = HipModel(cfg, FrontendConfig(), state_dict=sd, window=g["window"], mel_fb=g["fb64"])
    assert FUSED in m.describe_plan()
    # the shared composite check evaluates the head through oracle.model_forward, whose table has no entry for this head: for this test
    # it is the test-side restatement
    monkeypatch.setattr(oracle, "model_forward", rnn_oracle.model_forward)
    feats = np.ascontiguousarray(m.frontend(g["pcm"]).transpose(0, 2, 1))
    lf = rnn_oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel()
    assert _err(m.forward_features(feats)[0], lf) <= 1.0
    lp, pp, err, bound = assert_pcm_logits_vs_reference(m, cfg, sd, g, g["pcm"], d[f"{name}/logits_pcm"].ravel(), what=name)
    print(name, "PCM composite: worst |dlogit| / bound %.3f" % float((err / bound).max()))
    assert np.abs(pp - oracle.sigmoid(lp)).max() <= 1e-6
    m.close()


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("F", [32, 64, 96])
def test_fused_instances_against_float64(F, T):
    """T = 1: the forward launch is a single step with nothing to prefetch; T = 2: the first step that reads the h planes.  B = 1, 3, 17,
    33: a partial sixteen-clip workgroup, full + 1 and two + 1."""
    cfg = HeadConfig("rnn", (T, F))
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd)
    text = m.describe_plan()
    assert f"lstm:model.layer1_l0 + first reverse step {FUSED}" in text and m.feature_clamp > 0, text
    worst = 0.0
    for B in (1, 3, 17, 33):
        fx = synth_features(B, cfg.input_shape, seed=B)
        lg, _, emb = m.forward_features(fx, return_embedding=True)
        e_ref = rnn_oracle.head_forward(fx, sd, cfg, dtype=np.float64)
        ref = oracle.classify(e_ref, sd, cfg, dtype=np.float64).ravel()
        worst = max(worst, _err(lg, ref))
        assert np.isfinite(lg).all() and _err(lg, ref) <= 1.0, (B, _err(lg, ref))
        assert np.abs(emb - e_ref).max() <= EMB_RTOL * max(1.0, np.abs(e_ref).max()), (B, float(np.abs(emb - e_ref).max()))
    print("F", F, "T", T, "worst error vs float64: %.3f of the tolerance" % worst)
    m.close()


@pytest.mark.parametrize("shape", [(5, 32), (16, 96), (101, 64)])
def test_batch_invariance(shape):
    cfg = HeadConfig("rnn", shape)
    m = _model(cfg)
    assert FUSED in m.describe_plan()
    x = synth_features(33, shape, seed=11)
    full, _ = m.forward_features(x)
    for i in (0, 15, 16, 32):
        alone, _ = m.forward_features(np.ascontiguousarray(x[i:i + 1]))
        assert alone[0] == full[i], (shape, i, alone[0], full[i])
    m.close()


def test_knob_off_plans_the_xg_route(tmp_path):
    """NWW_RNN_IH_FUSED=0 (read once per process: a fresh interpreter) keeps the input projection a launch of its own for the LSTM and for
    the GRU head; against float64 it holds the same tolerance, and the fused run agrees with it within twice that."""
    out = str(tmp_path / "unfused.npz")
    code = ("import sys, numpy as np\n"
            "from nanowakeword_amd.config import FrontendConfig, HeadConfig\n"
            "from nanowakeword_amd.session import HipModel\n"
            "from nanowakeword_amd.synth import synth_features, synth_state_dict\n"
            "res = {}\n"
            "for mt, shape in (('rnn', (16, 96)), ('rnn', (101, 64)), ('rnn', (5, 32)), ('gru', (16, 64))):\n"
            "    cfg = HeadConfig(mt, shape); m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))\n"
            "    key = '%s_%dx%d' % ((mt,) + shape)\n"
            "    res[key + '/plan'] = np.array(m.describe_plan()); res[key + '/clamp'] = np.array(m.feature_clamp)\n"
            "    res[key + '/logits'] = m.forward_features(synth_features(33, shape, seed=6))[0]\n"
            "    m.close()\n"
            "np.savez(sys.argv[1], **res)\n")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]), NWW_RNN_IH_FUSED="0")
    r = subprocess.run([sys.executable, "-c", code, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    un = dict(np.load(out, allow_pickle=False))
    for shape in ((16, 96), (101, 64), (5, 32)):
        key = "rnn_%dx%d" % shape
        _assert_xg_route(str(un[key + "/plan"]))
        cfg = HeadConfig("rnn", shape)
        sd = synth_state_dict(cfg)
        x = synth_features(33, shape, seed=6)
        ref = rnn_oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
        m = _model(cfg, sd)
        assert FUSED in m.describe_plan()
        fused, _ = m.forward_features(x)
        m.close()
        print(key, "vs float64, in tolerances: unfused %.3f, fused %.3f; fused vs unfused %.3f"
              % (_err(un[key + "/logits"], ref), _err(fused, ref), _err(fused, un[key + "/logits"])))
        assert _err(un[key + "/logits"], ref) <= 1.0 and _err(fused, ref) <= 1.0
        assert _err(fused, un[key + "/logits"]) <= 2.0
    gp = str(un["gru_16x64/plan"])
    assert "+ input projection" not in gp and "gru:model.gru_l0 + first reverse step" in gp, gp


@pytest.mark.parametrize("cfg,kw", [
    (HeadConfig("rnn", (16, 96)), {"conv_arith": "f32"}),
    (HeadConfig("rnn", (16, 96)), {"conv_arith": "bf16x6"}),
    (HeadConfig("rnn", (16, 96)), {"conv_arith": "bf16x9"}),
    (HeadConfig("rnn", (9, 40)), {}),
    (HeadConfig("rnn", (9, 32), n_blocks=2), {}),
], ids=["f32", "bf16x6", "bf16x9", "F40", "two_blocks"])
def test_xg_routes_against_float64(cfg, kw):
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd, **kw)
    text = m.describe_plan()
    _assert_xg_route(text)
    worst = 0.0
    for B in (1, 17, 33):
        fx = synth_features(B, cfg.input_shape, seed=B + 40)
        lg, _, emb = m.forward_features(fx, return_embedding=True)
        e_ref = rnn_oracle.head_forward(fx, sd, cfg, dtype=np.float64)
        ref = oracle.classify(e_ref, sd, cfg, dtype=np.float64).ravel()
        worst = max(worst, _err(lg, ref))
        assert _err(lg, ref) <= 1.0, (B, _err(lg, ref), text)
        assert np.abs(emb - e_ref).max() <= EMB_RTOL * max(1.0, np.abs(e_ref).max())
    print(kw or cfg.input_shape, "worst error vs float64: %.3f of the tolerance" % worst)
    m.close()


def test_feature_magnitudes_and_clamp():
    cfg = HeadConfig("rnn", (5, 64))
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd)
    assert FUSED in m.describe_plan()
    cl = np.float32(m.feature_clamp)
    assert cl > 0
    rng = np.random.default_rng(5)
    x = synth_features(4, cfg.input_shape, seed=21)
    x[0] = rng.uniform(-1e-3, 1e-3, x[0].shape).astype(np.float32)                       # a quiet clip
    x[1] = np.where(rng.integers(0, 2, x[1].shape) == 1, cl, -cl).astype(np.float32)      # +-feature_clamp exactly
    x[2] = rng.standard_normal(x[2].shape).astype(np.float32) * np.array([0.5, 5e3, 0.5, 5e3, 0.5], np.float32)[:, None]   # frames 1e4 apart
    x[2] = np.clip(x[2], -cl, cl)
    assert np.abs(x).max() <= cl and np.abs(x[0]).max() <= 1e-3
    ref = rnn_oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lg, _ = m.forward_features(x)
    print("magnitudes: error vs float64 per clip, in tolerances:", [round(_err(lg[i], ref[i]), 3) for i in range(4)])
    assert _err(lg, ref) <= 1.0, (lg, ref)
    # one clip beyond the bound: the existing warning, and its neighbours do not move
    y = np.concatenate([x[:2], 4.0 * x[1:2], x[2:]])
    with pytest.warns(RuntimeWarning, match="clamps the head input"):
        ly, _ = m.forward_features(y)
    assert np.array_equal(ly[[0, 1, 3, 4]], lg)
    assert np.isfinite(ly[2])            # (the forward direction reads it clamped, the reverse direction's one step unclamped)
    m.close()


def test_onnx_pt_and_interpreter(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.interpreter import HipInterpreter
    from nanowakeword_amd.weights import infer_head_config, load_session, save_bundle, state_dict_from_pt
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_rnn.npz"), allow_pickle=False))
    feats, want = e["rnn/feats"], e["rnn/probs"]
    onnx = os.path.join(GOLDEN, "onnx", "rnn.onnx")
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

    # a .pt of the same weights -> bundle
    cfg = HeadConfig(**json.loads(str(e["meta_json"]))["rnn"])
    pt = str(tmp_path / "rnn.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}, pt)
    sd = state_dict_from_pt(pt)
    c = infer_head_config(sd, input_shape=cfg.input_shape)
    assert c == cfg
    bundle = str(tmp_path / "rnn_pt.nww.npz")
    save_bundle(bundle, c, sd, mode="features")
    s2 = load_session(bundle)
    assert np.abs(s2.run(None, {"input": feats})[0].reshape(-1) - want).max() <= 1e-5
    for path, key in ((onnx, "rnn"), (bundle, "rnn_pt")):
        for i in (0, len(feats) - 1):
            it = HipInterpreter.load_model(path, preprocessor=Pre(feats[i]))
            assert list(it.models) == [key], list(it.models)
            for _ in range(3):
                it.predict(np.zeros(1280, np.int16))
            assert abs(it.raw_scores[key] - want[i]) <= 1e-5, (path, i, it.raw_scores, want[i])


def test_other_bare_lstm_graphs_stay_refused():
    """A bare LSTM graph whose named tail is not model.layer2 keeps raising NotImplementedError (initialisers renamed in memory)."""
    import nanowakeword_amd.onnx_reader as rd
    from nanowakeword_amd import weights
    g = rd.read_onnx(os.path.join(GOLDEN, "onnx", "rnn.onnx"))
    g.initializers = {k.replace("model.layer2.", "model.fc."): v for k, v in g.initializers.items()}
    for n in g.nodes:
        n.inputs = [t.replace("model.layer2.", "model.fc.") for t in n.inputs]
    orig = rd.read_onnx
    rd.read_onnx = lambda _: g
    try:
        with pytest.raises(NotImplementedError):
            weights.load_session("renamed.onnx")
    finally:
        rd.read_onnx = orig
