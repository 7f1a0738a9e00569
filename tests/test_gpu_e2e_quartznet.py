"""Raw-PCM QuartzNet head (model_type="e2e_quartznet") on the GPU: the learned frontend alone (nww_frontend) and PCM -> logit against the
float64 restatement (tests/raw_oracle.py) and the reference-generated fixtures, every frontend shape on the conv1d_strided launches, batch
invariance, the backbone against the quartznet head, session, streaming and ingestion.

Under the default arithmetic channels {16, 32} x depth {2, 3} run as ONE raw_x3 launch; every other shape, every other conv_arith and
NWW_RAW_FUSED=0 take one conv1d_strided launch per stage.  The plan names are asserted wherever a plan is chosen."""
import json
import os

import numpy as np
import pytest

import raw_oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig, raw_frontend_depth, raw_frontend_frames
from nanowakeword_amd.synth import synth_features, synth_pcm, synth_state_dict
from parity import GOLDEN, LOGIT_ATOL, head_golden_names, load_head_goldens

pytestmark = pytest.mark.gpu

# clip lengths at the stride and tile edges, with the stage-3 rows each gives at depth 3
LENGTHS = {16: 1, 17: 1, 4000: 16, 8000: 32, 8193: 33, 16000: 63, 16384: 64, 16385: 65, 32000: 125, 32768: 128}
KINDS = ("noise", "loud", "sine", "chirp", "square", "zeros")


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_e2e_quartznet.npz")


def _cfg(n, channels=32, depth=None, **kw):
    d = 3 if depth is None else depth
    probe = HeadConfig("e2e_quartznet", (1, channels * 2 ** (d - 1)), e2e_frontend_channels=channels, e2e_frontend_depth=depth)
    return HeadConfig("e2e_quartznet", (raw_frontend_frames(probe, n), probe.input_shape[1]), e2e_frontend_channels=channels, e2e_frontend_depth=depth, **kw)


def _model(cfg, sd=None, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg) if sd is None else sd, **kw)


def _frontend_lines(m):
    return [l for l in m.describe_plan().strip().split("\n") if l.startswith("frontend:")]


def _mixed_pcm(n, clips_per_kind=1, seed=10):
    return np.concatenate([synth_pcm(k, clips_per_kind, n, seed=seed) for k in KINDS], 0)


def _check_frontend(m, cfg, sd, pcm, what):
    """nww_frontend against float64: max |d| <= LOGIT_ATOL x max(1, |ref|max) (the QuartzNet bar) -> the error"""
    ref = raw_oracle.forward(pcm, sd, cfg, dtype=np.float64)[0]
    got = m.frontend(pcm)
    assert got.shape == ref.shape and np.isfinite(got).all(), (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= LOGIT_ATOL * max(1.0, float(np.abs(ref).max())), (what, err)
    return err


def _check_logits(m, cfg, sd, pcm, what):
    ref = raw_oracle.forward(pcm, sd, cfg, dtype=np.float64)[2].ravel()
    lg, pr = m.forward_pcm(pcm)
    err = float(np.abs(lg - ref).max())
    assert np.isfinite(lg).all() and err <= LOGIT_ATOL, (what, err, m.describe_plan())
    assert np.abs(pr - 1.0 / (1.0 + np.exp(-lg.astype(np.float64)))).max() <= 1e-6
    return err


# ---- 1: the frontend alone and PCM -> logit at every clip length, every clip kind
@pytest.mark.parametrize("n", sorted(LENGTHS))
def test_frontend_and_logits_vs_float64(n):
    cfg = _cfg(n)
    assert cfg.input_shape == (LENGTHS[n], 128)
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd)
    assert m.num_frames(n) == LENGTHS[n] and m.feature_clamp == 0.0
    pcm = _mixed_pcm(n)
    e_f = _check_frontend(m, cfg, sd, pcm, n)
    e_l = _check_logits(m, cfg, sd, pcm, n)
    print(n, "samples: frontend max |d| vs float64 %.2e, max |dlogit| %.2e" % (e_f, e_l))
    # time-major output of the device entry point is the transpose, bit for bit
    import torch
    dp = torch.from_numpy(pcm).cuda()
    out = torch.empty((pcm.shape[0], LENGTHS[n], 128), dtype=torch.float32, device="cuda")
    m.frontend_dev(dp.data_ptr(), pcm.shape[0], n, out.data_ptr(), frames_major=True)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().transpose(0, 2, 1), m.frontend(pcm))
    m.close()


@pytest.mark.parametrize("B", [1, 3, 33, 70])
def test_frontend_ragged_batches(B):
    for n in (4000, 8193):
        cfg = _cfg(n)
        sd = synth_state_dict(cfg)
        m = _model(cfg, sd)
        pcm = synth_pcm("noise", B, n, seed=B)
        _check_frontend(m, cfg, sd, pcm, (n, B))
        _check_logits(m, cfg, sd, pcm, (n, B))
        m.close()


def test_long_clip_takes_the_generic_blocks():
    """32769 samples give 129 rows: beyond qn_x3's clip-resident 128, so the backbone runs on its generic launches behind the same frontend."""
    n = 32769
    cfg = _cfg(n)
    assert cfg.input_shape[0] == 129
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd)
    text = m.describe_plan()
    assert "qn_x3:" not in text and text.count("dwconv1d:") == 3 and len(_frontend_lines(m)) == 1 and "frontend:raw_x3:" in text, text
    pcm = _mixed_pcm(n)
    _check_frontend(m, cfg, sd, pcm, n)
    print("129 rows: max |dlogit| vs float64 %.2e" % _check_logits(m, cfg, sd, pcm, n))
    m.close()


# ---- 2: the reference's own numbers
@pytest.mark.parametrize("name", head_golden_names("heads_e2e_quartznet.npz"))
def test_vs_reference_golden(golden, name):
    d, meta = golden
    cfg = HeadConfig(**meta[name])
    m = _model(cfg)
    pcm = d[f"{name}/pcm"]
    fe = m.frontend(pcm)
    ref_f = d[f"{name}/frontend"]
    assert np.abs(fe - ref_f).max() <= LOGIT_ATOL * max(1.0, np.abs(ref_f).max()), (name, np.abs(fe - ref_f).max())
    lg, _ = m.forward_pcm(pcm)
    err = np.abs(lg - d[f"{name}/logits"].ravel()).max()
    print(name, "max |dlogit| vs reference: %.2e" % err)
    assert err <= LOGIT_ATOL, (name, err, m.describe_plan())
    # the backbone alone on the reference's frontend output
    lf, _, emb = m.forward_features(np.ascontiguousarray(ref_f.transpose(0, 2, 1)), return_embedding=True)
    assert np.abs(lf - d[f"{name}/logits"].ravel()).max() <= LOGIT_ATOL and np.abs(emb - d[f"{name}/emb"]).max() <= 1e-4 * max(1.0, np.abs(d[f"{name}/emb"]).max())
    m.close()


# ---- 3: the plan, and every frontend shape and arithmetic on the conv1d_strided launches
def test_plan_at_reference_defaults():
    m = _model(_cfg(16000))
    lines = m.describe_plan().strip().split("\n")
    fe = _frontend_lines(m)
    assert fe == ["frontend:raw_x3:model.frontend (3 stages 1->128, conv+bn+relu) [f16x3]"], lines          # 1 + 3 + tail launches
    head = [l for l in lines if not l.startswith(("frontend:", "unary:sigmoid"))]
    assert len(head) == 4 and all(l.startswith("qn_x3:model.backbone.quartznet_blocks.") for l in head[:3]) and head[3].startswith("tail:fc+classifier"), lines
    assert "fe_stft_mel_db_kernel" not in "\n".join(lines)
    m.close()


@pytest.mark.parametrize("channels,depth,n,fused", [(24, 3, 4000, False), (32, 1, 500, False), (8, 4, 16000, False), (16, 2, 4000, True), (16, 3, 8193, True),
                                                    (32, 2, 2000, True), (32, 2, 4100, True), (64, 4, 8000, False)],
                         ids=["c24", "d1", "d4_c8", "c16_d2", "c16_d3", "c32_d2", "c32_d2_tiles", "c64_d4_width512"])
def test_frontend_shapes(channels, depth, n, fused):
    cfg = _cfg(n, channels, depth, embedding_dim=32)
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd)
    fe = _frontend_lines(m)
    if fused:
        assert len(fe) == 1 and fe[0].startswith("frontend:raw_x3:model.frontend (%d stages" % depth), fe
    else:
        assert len(fe) == depth and all(l.startswith("frontend:conv1d_strided:") for l in fe), fe
    pcm = _mixed_pcm(n)
    e_f = _check_frontend(m, cfg, sd, pcm, (channels, depth))
    e_l = _check_logits(m, cfg, sd, pcm, (channels, depth))
    print(channels, depth, "frontend %.2e logits %.2e vs float64" % (e_f, e_l))
    m.close()


@pytest.mark.parametrize("arith", ["f32", "bf16x6", "bf16x9", "f16x3"])
def test_arithmetics(arith):
    n = 8000
    cfg = _cfg(n)
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd, conv_arith=arith)
    text = m.describe_plan()
    fused = arith == "f16x3"
    assert text.count("frontend:conv1d_strided:") == (0 if fused else 3) and text.count("frontend:raw_x3:") == int(fused) and ("qn_x3:" in text) == fused, text
    pcm = _mixed_pcm(n)
    _check_frontend(m, cfg, sd, pcm, arith)
    print(arith, "max |dlogit| vs float64: %.2e" % _check_logits(m, cfg, sd, pcm, arith))
    m.close()


def test_knob_off_falls_back():
    """NWW_RAW_FUSED=0 (read once per process: a fresh interpreter): one conv1d_strided launch per stage, same bar."""
    import subprocess
    import sys
    code = ("import numpy as np, raw_oracle\n"
            "from nanowakeword_amd.config import FrontendConfig, HeadConfig\n"
            "from nanowakeword_amd.session import HipModel\n"
            "from nanowakeword_amd.synth import synth_pcm, synth_state_dict\n"
            "cfg = HeadConfig('e2e_quartznet', (33, 128)); sd = synth_state_dict(cfg)\n"
            "m = HipModel(cfg, FrontendConfig(), state_dict=sd, tables='builtin'); t = m.describe_plan()\n"        # no mel tables: no torch import
            "assert 'raw_x3' not in t and t.count('frontend:conv1d_strided:') == 3 and t.count('qn_x3:') == 3, t\n"
            "pcm = np.concatenate([synth_pcm(k, 1, 8193) for k in ('noise', 'loud', 'sine', 'chirp', 'square', 'zeros')], 0)\n"
            "f64, _, l64 = raw_oracle.forward(pcm, sd, cfg, dtype=np.float64)\n"
            "df = np.abs(m.frontend(pcm) - f64).max(); dl = np.abs(m.forward_pcm(pcm)[0] - l64.ravel()).max()\n"
            "assert df <= 1e-4 * max(1.0, np.abs(f64).max()) and dl <= 1e-4, (df, dl)\n"
            "print('NWW_RAW_FUSED=0 frontend %.2e logits %.2e vs float64' % (df, dl))\n")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    env["NWW_RAW_FUSED"] = "0"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- 4: a clip's result does not depend on its batch or slot
def test_batch_invariance():
    n = 4000
    cfg = _cfg(n)
    m = _model(cfg)
    big = synth_pcm("noise", 600, n, seed=7)
    big[5] = synth_pcm("square", 1, n)[0]
    l600, _ = m.forward_pcm(big)
    l70, _ = m.forward_pcm(big[:70])
    assert np.array_equal(l600[:70], l70)
    for i in (0, 5, 69, 599):
        l1, _ = m.forward_pcm(big[i:i + 1])
        assert l1[0] == l600[i], (i, l1[0], l600[i])
    f70 = m.frontend(big[:70])
    assert np.array_equal(m.frontend(big[69:70])[0], f70[69])
    m.close()


# ---- 5: full-scale input: nothing is clamped
def test_full_scale_square():
    n = 16000
    cfg = _cfg(n)
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd)
    pcm = np.concatenate([synth_pcm("square", 1, n), -synth_pcm("square", 1, n), np.full((1, n), -32768, np.int16), np.full((1, n), 32767, np.int16)], 0)
    e_f = _check_frontend(m, cfg, sd, pcm, "square")
    print("full-scale: frontend %.2e logits %.2e vs float64" % (e_f, _check_logits(m, cfg, sd, pcm, "square")))
    m.close()


# ---- 6: the backbone alone is the quartznet head
def test_backbone_equals_the_quartznet_head():
    cfg = _cfg(16000)
    sd = synth_state_dict(cfg)
    q, qsd = raw_oracle.as_quartznet(cfg, sd)
    m, mq = _model(cfg, sd), _model(q, qsd)
    x = synth_features(5, cfg.input_shape, seed=2) / np.float32(32.0)
    a, b = m.forward_features(x, return_embedding=True), mq.forward_features(x, return_embedding=True)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    # and PCM -> logit is the frontend's time-major output through it
    pcm = synth_pcm("noise", 3, 16000)
    feats = np.ascontiguousarray(m.frontend(pcm).transpose(0, 2, 1))
    assert np.array_equal(m.forward_pcm(pcm)[0], mq.forward_features(feats)[0])
    m.close(); mq.close()


# ---- 7: session, streaming, ingestion
def test_session_and_streaming():
    from nanowakeword_amd.session import HipSession
    n = 4000
    cfg = _cfg(n)
    m = _model(cfg)
    with pytest.raises(ValueError, match="clip_samples"):
        HipSession(m, mode="e2e", clip_samples=16000)
    s = HipSession(m, mode="e2e", clip_samples=n)
    assert s.get_inputs()[0].shape == [None, 1, n]
    pcm = synth_pcm("noise", 3, n)
    pf = (pcm.astype(np.float32) / np.float32(32768.0))[:, None, :]
    assert np.array_equal(s.run(None, {"input": pf})[0], s.run(None, {"input": pcm})[0])
    assert np.array_equal(s.run_logits({"input": pcm}).ravel(), m.forward_pcm(pcm)[0])
    # streaming re-scores the whole window every hop: bit-equal to scoring the window itself
    S, hop = 2, 800
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
    m.close()


def test_onnx_and_pt_through_the_session(tmp_path):
    import torch
    from nanowakeword_amd.weights import infer_head_config, load_session, save_bundle, state_dict_from_pt
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_e2e_quartznet.npz"), allow_pickle=False))
    pcm, want = e["e2e_quartznet/pcm"], e["e2e_quartznet/probs"]
    s = load_session(os.path.join(GOLDEN, "onnx", "e2e_quartznet.onnx"))
    assert s.mode == "e2e" and s.clip_samples == 2000
    assert np.abs(s.run(None, {"input": pcm})[0].reshape(-1) - want).max() <= 1e-5
    cfg = HeadConfig(**json.loads(str(e["meta_json"]))["e2e_quartznet"])
    pt = str(tmp_path / "e2e_quartznet.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}, pt)
    sd = state_dict_from_pt(pt)
    c = infer_head_config(sd, input_shape=cfg.input_shape)
    assert c == cfg
    bundle = str(tmp_path / "e2e_quartznet_pt.nww.npz")
    save_bundle(bundle, c, sd, mode="e2e", clip_samples=2000)
    s2 = load_session(bundle)
    assert np.abs(s2.run(None, {"input": pcm})[0].reshape(-1) - want).max() <= 1e-5


def test_create_refuses_what_headconfig_refuses():
    import ctypes
    from nanowakeword_amd import _lib
    lib = _lib.load_library()
    for field, value, msg in (("n_blocks", 0, "depth must be 1..4"), ("n_blocks", 5, "depth must be 1..4"), ("in_cols", 64, "gives 128 channels"),
                              ("layer_dim", 256, "must be <= 512"), ("mel_major_features", 1, "mel_major_features"), ("n_crnn_channels", 5, "1..4")):
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
