"""Raw-PCM CNN head (model_type="e2e_cnn") on the GPU (run with -m gpu): PCM -> frontend, embedding and logit against the float64 restatement
(tests/e2e_cnn_oracle.py) at the smallest shapes where the strided 3x3 kernels can go wrong, the reference-generated fixtures, the three
activations, batch invariance bit for bit, the float32 route under every other arithmetic and NWW_CONV2S_X3=0, rescaled channels, clip
magnitudes, session, interpreter, streaming and ingestion.

Under the default arithmetic conv2 .. conv4 run as one conv2s_x3 launch each and conv1 as a conv2d_strided launch; every other conv_arith and
NWW_CONV2S_X3=0 take conv2d_strided for all four.  The plan names are asserted wherever a plan is chosen.

Tolerances, as tests/test_gpu_rnn.py states them: logits within 1e-4 + 2.4e-7 |ref|, embedding within 1e-4 max(1, |ref|max)."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import e2e_cnn_oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig, raw_frontend_frames
from nanowakeword_amd.synth import synth_pcm, synth_state_dict
from parity import GOLDEN, head_golden_names, load_head_goldens
from test_e2e_cnn_head import RESCALE, rel_logit_error, rescale_case, rescaled_sd

pytestmark = pytest.mark.gpu

LOGIT_ATOL = 1e-4
LOGIT_ULPS = 2.4e-7        # + two float32 ulps of the logit
EMB_RTOL = 1e-4
BATCHES = (1, 3, 17)
# samples -> the image's width W at depth 2: both parities of W at every stride-2 layer, and W = 1 at all of them
LENGTHS = {1: 1, 64: 1, 272: 5, 528: 9, 1040: 17, 4000: 63, 16000: 250}


def _err(got, ref):
    """|got - ref| in units of the tolerance LOGIT_ATOL + LOGIT_ULPS |ref| (<= 1 passes)."""
    got, ref = np.ravel(got).astype(np.float64), np.ravel(ref).astype(np.float64)
    return float((np.abs(got - ref) / (LOGIT_ATOL + LOGIT_ULPS * np.abs(ref))).max())


def _cfg(n, channels=32, depth=None, **kw):
    d = 2 if depth is None else depth
    probe = HeadConfig("e2e_cnn", (1, channels * 2 ** (d - 1)), e2e_frontend_channels=channels, e2e_frontend_depth=depth)
    return HeadConfig("e2e_cnn", (raw_frontend_frames(probe, n), probe.input_shape[1]), e2e_frontend_channels=channels, e2e_frontend_depth=depth, **kw)


def _model(cfg, sd=None, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg) if sd is None else sd, **kw)


def _pcm(B, n, seed=10):
    """B clips of n samples: noise, then the other kinds in turn"""
    kinds = ("noise", "speechlike", "loud", "sine", "square", "zeros", "chirp")
    return np.concatenate([synth_pcm(kinds[i % len(kinds)], 1, n, seed=seed + i) for i in range(B)], 0)


def _plan(m):
    lines = m.describe_plan().strip().split("\n")
    return [l for l in lines if l.startswith("frontend:")], [l for l in lines if not l.startswith(("frontend:", "unary:sigmoid"))]


def _assert_plan(m, x3=True, raw_x3=True, depth=2):
    """frontend lines and the head's six launches: conv1 on conv2d_strided, conv2 .. conv4 on conv2s_x3 (or all four on conv2d_strided)"""
    fe, head = _plan(m)
    text = m.describe_plan()
    if raw_x3:
        assert len(fe) == 1 and fe[0].startswith("frontend:raw_x3:model.frontend (%d stages" % depth), text
    else:
        assert len(fe) == depth and all(l.startswith("frontend:conv1d_strided:") for l in fe), text
    assert len(head) == 6 and head[0].startswith("conv2d_strided:model.backbone.conv1 ") and head[4] == "mean:plane" and head[5].startswith("tail:fc+classifier"), text
    for i in (2, 3, 4):
        assert head[i - 1].startswith(("conv2s_x3" if x3 else "conv2d_strided") + f":model.backbone.conv{i} "), text
    assert text.count("[f16x3]") == (3 if x3 else 0) + int(raw_x3) and "fe_stft_mel_db_kernel" not in text, text


def _check(m, cfg, sd, pcm, what):
    """frontend, embedding (the backbone alone on the device's own frontend output) and logits against float64 -> the logit error in
    units of the tolerance.  forward_features on frontend()'s output is forward_pcm, bit for bit."""
    f64, e64, l64 = e2e_cnn_oracle.forward(pcm, sd, cfg, dtype=np.float64)
    fe = m.frontend(pcm)
    assert fe.shape == f64.shape and np.abs(fe - f64).max() <= LOGIT_ATOL * max(1.0, np.abs(f64).max()), (what, np.abs(fe - f64).max())
    lg, pr = m.forward_pcm(pcm)
    lf, _, emb = m.forward_features(np.ascontiguousarray(fe.transpose(0, 2, 1)), return_embedding=True)
    assert np.array_equal(lf, lg), (what, lf, lg)
    assert np.isfinite(lg).all() and np.isfinite(emb).all(), what
    e_emb = float(np.abs(emb - e64).max())
    assert e_emb <= EMB_RTOL * max(1.0, np.abs(e64).max()), (what, e_emb, m.describe_plan())
    err = _err(lg, l64)
    assert err <= 1.0, (what, err, lg, l64.ravel(), m.describe_plan())
    assert np.abs(pr - 1.0 / (1.0 + np.exp(-lg.astype(np.float64)))).max() <= 1e-6
    return err


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_e2e_cnn.npz")


@pytest.fixture(scope="module")
def default_models():
    """samples -> (cfg, weights, default-arithmetic model) at channels 32 x depth 2, shared by the tests that only run it"""
    made = {}

    def get(n):
        if n not in made:
            cfg = _cfg(n)
            sd = synth_state_dict(cfg)
            made[n] = (cfg, sd, _model(cfg, sd))
        return made[n]
    yield get
    for _, _, m in made.values():
        m.close()


# ---- 1: against float64 at the smallest shapes where the kernel can go wrong
@pytest.mark.parametrize("n", sorted(LENGTHS))
def test_vs_float64_at_the_edge_widths(default_models, n):
    cfg, sd, m = default_models(n)
    assert cfg.input_shape == (LENGTHS[n], 64) and m.num_frames(n) == LENGTHS[n] and m.feature_clamp == 0.0
    _assert_plan(m)
    for B in BATCHES:
        print(n, "samples, B =", B, ": %.3f of the logit tolerance" % _check(m, cfg, sd, _pcm(B, n, seed=B), (n, B)))


@pytest.mark.parametrize("channels,depth,n,raw_x3", [(16, 2, 4000, True), (32, 3, 4000, True), (32, 3, 16000, True), (24, 2, 4000, False), (8, 1, 200, False),
                                                     (1, 1, 100, False)],
                         ids=["H32", "H128_4000", "H128_16000", "H48_generic_frontend", "H8", "H1"])
def test_other_heights(channels, depth, n, raw_x3):
    cfg = _cfg(n, channels, depth, embedding_dim=32)
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd)
    _assert_plan(m, raw_x3=raw_x3, depth=depth)
    for B in BATCHES:
        print(channels, depth, n, "B =", B, ": %.3f of the logit tolerance" % _check(m, cfg, sd, _pcm(B, n, seed=B), (channels, depth, n, B)))
    m.close()


# ---- 2: the reference's own numbers
@pytest.mark.parametrize("name", head_golden_names("heads_e2e_cnn.npz"))
def test_vs_reference_golden(golden, name):
    d, meta = golden
    cfg = HeadConfig(**meta[name])
    m = _model(cfg)
    _assert_plan(m, depth=cfg.e2e_frontend_depth or 2)
    pcm = d[f"{name}/pcm"]
    fe, ref_f = m.frontend(pcm), d[f"{name}/frontend"]
    assert np.abs(fe - ref_f).max() <= LOGIT_ATOL * max(1.0, np.abs(ref_f).max()), (name, np.abs(fe - ref_f).max())
    lg, _ = m.forward_pcm(pcm)
    err = _err(lg, d[f"{name}/logits"])
    print(name, "vs reference: %.3f of the logit tolerance" % err)
    assert err <= 1.0, (name, lg, d[f"{name}/logits"].ravel(), m.describe_plan())
    # the backbone alone on the reference's frontend output
    lf, _, emb = m.forward_features(np.ascontiguousarray(ref_f.transpose(0, 2, 1)), return_embedding=True)
    assert _err(lf, d[f"{name}/logits"]) <= 1.0 and np.abs(emb - d[f"{name}/emb"]).max() <= EMB_RTOL * max(1.0, np.abs(d[f"{name}/emb"]).max())
    m.close()


# ---- 3: the three activations
@pytest.mark.parametrize("act", ["relu", "gelu", "silu"])
def test_activations(act):
    n = 1040
    cfg = _cfg(n, activation=act)
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd)
    _assert_plan(m)
    assert sum(l.endswith(("+bn+" + act + " [f16x3]", "+bn+" + act + " [f32]")) for l in _plan(m)[1]) == 4, m.describe_plan()
    for B in BATCHES:
        print(act, "B =", B, ": %.3f of the logit tolerance" % _check(m, cfg, sd, _pcm(B, n, seed=20 + B), (act, B)))
    m.close()


# ---- 4: a clip's bits do not depend on its batch or slot
@pytest.mark.parametrize("n", [4000, 16000])
def test_batch_invariance(default_models, n):
    cfg, sd, m = default_models(n)
    _assert_plan(m)
    big = synth_pcm("noise", 70, n, seed=7)
    big[15] = synth_pcm("square", 1, n)[0]
    big[16] = 0
    l33, _ = m.forward_pcm(big[:33])
    f33 = m.frontend(big[:33])
    _, _, e33 = m.forward_features(np.ascontiguousarray(f33.transpose(0, 2, 1)), return_embedding=True)
    for i in (0, 15, 16, 32):
        l1, _ = m.forward_pcm(big[i:i + 1])
        assert l1[0] == l33[i], (n, i, l1[0], l33[i])
        assert np.array_equal(m.frontend(big[i:i + 1])[0], f33[i]), (n, i)
        _, _, e1 = m.forward_features(np.ascontiguousarray(f33[i:i + 1].transpose(0, 2, 1)), return_embedding=True)
        assert np.array_equal(e1[0], e33[i]), (n, i)
    l70, _ = m.forward_pcm(big)                     # ragged: 70 is no multiple of anything the kernels tile by
    assert np.array_equal(l70[:33], l33)
    assert m.forward_pcm(big[69:70])[0][0] == l70[69]


# ---- 5: the float32 route
@pytest.mark.parametrize("arith", ["f32", "bf16x6", "bf16x9"])
def test_arithmetics_take_conv2d_strided(arith):
    n = 1040
    cfg = _cfg(n)
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd, conv_arith=arith)
    _assert_plan(m, x3=False, raw_x3=False)
    for B in BATCHES:
        print(arith, "B =", B, ": %.3f of the logit tolerance" % _check(m, cfg, sd, _pcm(B, n, seed=30 + B), (arith, B)))
    m.close()


def test_knob_off_plans_conv2d_strided(default_models):
    """NWW_CONV2S_X3=0 (read once per process: a fresh interpreter): conv2d_strided for every conv; within the tolerance of float64 and
    within twice that of the default run."""
    n = 4000
    cfg, sd, m = default_models(n)
    pcm = _pcm(3, n, seed=40)
    l_def, _ = m.forward_pcm(pcm)
    code = ("import json, numpy as np\n"
            "from nanowakeword_amd.config import FrontendConfig, HeadConfig\n"
            "from nanowakeword_amd.session import HipModel\n"
            "from nanowakeword_amd.synth import synth_state_dict\n"
            "from test_gpu_e2e_cnn import _cfg, _pcm\n"
            "cfg = _cfg(4000); sd = synth_state_dict(cfg)\n"
            "m = HipModel(cfg, FrontendConfig(), state_dict=sd, tables='builtin')\n"                            # no mel tables: no torch import
            "print(json.dumps({'plan': m.describe_plan(), 'logits': [float(v) for v in m.forward_pcm(_pcm(3, 4000, seed=40))[0]]}))\n")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    env["NWW_CONV2S_X3"] = "0"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().split("\n")[-1])
    text = out["plan"]
    assert "conv2s_x3" not in text and text.count("conv2d_strided:model.backbone.conv") == 4 and "frontend:raw_x3:" in text, text
    lg = np.array(out["logits"], np.float32)
    l64 = e2e_cnn_oracle.forward(pcm, sd, cfg, dtype=np.float64)[2]
    print("NWW_CONV2S_X3=0: %.3f of the tolerance vs float64, %.3f vs the default run" % (_err(lg, l64), _err(lg, l_def)))
    assert _err(lg, l64) <= 1.0 and _err(lg, l_def) <= 2.0 and _err(l_def, l64) <= 1.0


# ---- 6: rescaled channels (tests/test_e2e_cnn_head.py has the cases and their CPU confirmation)
@pytest.mark.parametrize("name", list(RESCALE))
def test_rescaled_channels(name):
    cfg, _, pcm = rescale_case()
    sd = rescaled_sd(name)
    l64 = e2e_cnn_oracle.forward(pcm, sd, cfg, dtype=np.float64)[2]
    e32 = rel_logit_error(e2e_cnn_oracle.forward(pcm, sd, cfg)[2], l64)
    m = _model(cfg, sd)
    try:
        _, head = _plan(m)
        lg, _ = m.forward_pcm(pcm)
        e_dev = rel_logit_error(lg, l64)
        print(f"{name}: device vs float64 {e_dev:.2e}, float32 restatement {e32:.2e}, contract {2 * e32 + 2e-6:.2e}; plan: " + " | ".join(l.split(" ")[0] for l in head))
        _assert_plan(m)                                  # no range guard: the rescale must not move the plan
        assert m.feature_clamp == 0.0
        assert e_dev <= 2.0 * e32 + 2e-6, (name, e_dev, e32)
        assert _err(lg, l64) <= 1.0
    finally:
        m.close()


# ---- 7: magnitudes: nothing is clamped, nothing warns
def test_magnitudes(default_models):
    n = 4000
    cfg, sd, m = default_models(n)
    rng = np.random.default_rng(3)
    pcm = np.concatenate([synth_pcm("square", 1, n), rng.integers(-16, 17, size=(1, n)).astype(np.int16), np.zeros((1, n), np.int16)], 0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        err = _check(m, cfg, sd, pcm, "magnitudes")
        assert m.feature_clamp == 0.0
    print("full-scale square, +-16 LSB noise, zeros: %.3f of the logit tolerance" % err)
    # the quiet clip is not the silent one
    lg, _ = m.forward_pcm(pcm)
    assert lg[1] != lg[2]


# ---- 8: session, interpreter, streaming, ingestion
def test_session_and_streaming(default_models):
    from nanowakeword_amd.session import HipSession
    n, hop = 4000, 1280
    cfg, sd, m = default_models(n)
    with pytest.raises(ValueError, match="clip_samples"):
        HipSession(m, mode="e2e", clip_samples=16000)
    s = HipSession(m, mode="e2e", clip_samples=n)
    assert s.get_inputs()[0].shape == [None, 1, n]
    pcm = synth_pcm("noise", 3, n)
    out = s.run(None, {"input": pcm})[0]
    assert out.shape == (3, 1, 1)
    pf = (pcm.astype(np.float32) / np.float32(32768.0))[:, None, :]
    assert np.array_equal(s.run(None, {"input": pf})[0], out)
    assert np.array_equal(s.run_logits({"input": pcm}).ravel(), m.forward_pcm(pcm)[0])
    # streaming re-scores the whole window every hop: bit-equal to scoring the window itself
    S = 2
    audio = synth_pcm("noise", S, n + 3 * hop, seed=4)
    m.stream_open(S, n, hop)
    for j in range((n + 3 * hop) // hop):
        lg, _ = m.stream_push(audio[:, j * hop:(j + 1) * hop])
        end = (j + 1) * hop
        if end < n:
            assert np.array_equal(lg, np.zeros(S, np.float32))
        else:
            assert np.array_equal(lg, m.forward_pcm(np.ascontiguousarray(audio[:, end - n:end]))[0]), j
    m.stream_close()


def test_onnx_pt_and_bundle_through_session_and_interpreter(tmp_path):
    import torch
    from nanowakeword_amd.interpreter import HipInterpreter
    from nanowakeword_amd.weights import infer_head_config, load_session, save_bundle, state_dict_from_pt
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_e2e_cnn.npz"), allow_pickle=False))
    pcm, want = e["e2e_cnn/pcm"], e["e2e_cnn/probs"]
    onnx = os.path.join(GOLDEN, "onnx", "e2e_cnn.onnx")
    s = load_session(onnx)
    assert s.mode == "e2e" and s.clip_samples == 2000
    assert np.abs(s.run(None, {"input": pcm})[0].reshape(-1) - want).max() <= 1e-5
    assert _err(s.run_logits({"input": pcm}), e["e2e_cnn/logits"]) <= 1.0
    cfg = HeadConfig(**json.loads(str(e["meta_json"]))["e2e_cnn"])
    pt = str(tmp_path / "e2e_cnn.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}, pt)
    sd = state_dict_from_pt(pt)
    c = infer_head_config(sd, input_shape=cfg.input_shape)
    assert c == cfg
    bundle = str(tmp_path / "e2e_cnn_pt.nww.npz")
    save_bundle(bundle, c, sd, mode="e2e", clip_samples=2000)
    s2 = load_session(bundle)
    assert np.abs(s2.run(None, {"input": pcm})[0].reshape(-1) - want).max() <= 1e-5
    for path, key in ((bundle, "e2e_cnn_pt"), (onnx, "e2e_cnn")):
        it = HipInterpreter.load_model(path)
        assert len(it.predict_clip(pcm[0])) == 1
        assert abs(it.raw_scores[key] - float(want[0])) <= 1e-5, (path, it.raw_scores)


def test_create_refuses_what_headconfig_refuses():
    import ctypes
    from nanowakeword_amd import _lib
    lib = _lib.load_library()
    for field, value, msg in (("n_blocks", 0, "depth must be 1..4"), ("n_blocks", 5, "depth must be 1..4"), ("in_cols", 128, "gives 64 channels"),
                              ("layer_dim", 512, "must be <= 512"), ("mel_major_features", 1, "mel_major_features")):
        c = _lib.make_config(_cfg(16000), FrontendConfig())
        setattr(c, field, value)
        h = ctypes.c_void_p()
        assert lib.nww_create(ctypes.byref(c), ctypes.byref(h)) != 0, field
        assert msg in lib.nww_last_error(None).decode(), (field, lib.nww_last_error(None).decode())
    m = _model(_cfg(16000))
    with pytest.raises(ValueError, match="input_shape"):
        m.forward_pcm(synth_pcm("noise", 1, 8000))
    with pytest.raises(ValueError, match="no mel power"):
        m.frontend(synth_pcm("noise", 1, 16000), return_power=True)
    m.close()
