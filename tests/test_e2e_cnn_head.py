"""Raw-PCM CNN head (model_type="e2e_cnn"): configuration, frame law, state_dict spec, C-slot packing, .pt / .onnx ingestion and the numpy
restatement (tests/e2e_cnn_oracle.py) against the reference-generated fixtures and against itself in float64.  CPU only."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import e2e_cnn_oracle
from nanowakeword_amd.config import (HEAD_CODE, RAW_CNN_LAYERS, FrontendConfig, HeadConfig, head_macs, param_spec, raw_cnn_planes, raw_frontend_depth,
                                     raw_frontend_frames, raw_frontend_stages)
from nanowakeword_amd.synth import state_dict_checksum, synth_pcm, synth_state_dict
from parity import GOLDEN, LOGIT_ATOL, load_head_goldens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"e2e_cnn_16000", "e2e_cnn_4000", "e2e_cnn_4000_c16", "e2e_cnn_4000_d3", "e2e_cnn_4000_gelu", "e2e_cnn_1040_silu_e32"}


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_e2e_cnn.npz")


def _e2e(shape=(250, 64), **kw):
    return HeadConfig("e2e_cnn", shape, **kw)


def test_head_code_matches_header_and_defaults():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    assert int(re.search(r"#define NWW_HEAD_E2E_CNN (\d+)", hdr).group(1)) == HEAD_CODE["e2e_cnn"] == 13
    assert len(re.findall(r"^(?:int|int32_t|int64_t|void|float|const char\*)\s+nww_\w+\(", hdr, re.M)) == 48          # no new exported symbol
    cfg = HeadConfig("E2E_CNN", (250, 64))
    assert cfg.model_type == "e2e_cnn" and (cfg.e2e_frontend_channels, cfg.e2e_frontend_depth) == (32, None)
    # the depth default is this model type's own (model.py:110), not the raw QuartzNet's 3
    assert raw_frontend_depth(cfg) == 2 and raw_frontend_depth(HeadConfig("e2e_quartznet", (63, 128))) == 3
    assert raw_frontend_stages(cfg) == [(1, 32, 41, 16), (32, 64, 13, 4)]
    assert HeadConfig(**json.loads(json.dumps(cfg.to_dict()))) == cfg
    assert RAW_CNN_LAYERS == ((1, 24, 1, 2), (24, 48, 2, 2), (48, 64, 2, 2), (64, 96, 1, 1))
    # (H, W) at 1 s: the issue's 64x250, 64x125, 32x63, 16x32, 16x32
    assert raw_cnn_planes(cfg) == [(64, 250), (64, 125), (32, 63), (16, 32), (16, 32)]
    assert raw_cnn_planes(_e2e((1, 8), e2e_frontend_channels=8, e2e_frontend_depth=1)) == [(8, 1), (8, 1), (4, 1), (2, 1), (2, 1)]


def test_config_validation():
    for kw, msg in ((dict(e2e_frontend_depth=0), "depth must be 1..4"), (dict(e2e_frontend_depth=5), "depth must be 1..4"),
                    (dict(e2e_frontend_channels=0), "channels must be positive"), (dict(e2e_frontend_channels=512), "must be <= 512")):
        with pytest.raises(ValueError, match=msg):
            _e2e(**kw)
    with pytest.raises(ValueError, match="input_shape is what the backbone sees"):
        _e2e((250, 128))                                                                            # 128 is depth 3's width
    _e2e((63, 128), e2e_frontend_depth=3)
    _e2e((16, 512), e2e_frontend_channels=64, e2e_frontend_depth=4)
    _e2e((5, 1), e2e_frontend_channels=1, e2e_frontend_depth=1)
    _e2e(e2e_quartznet_config=[[0, 0, 0]] * 7, quartznet_config=[])                                 # this head reads neither list


def test_nww_config_keeps_its_size_and_packs_the_slots():
    from nanowakeword_amd import _lib
    assert ctypes.sizeof(_lib.NwwConfig) == 132
    c = _lib.make_config(_e2e((63, 32), e2e_frontend_channels=16, e2e_frontend_depth=2, embedding_dim=32, activation="silu"), FrontendConfig())
    assert (c.head_type, c.layer_dim, c.n_blocks, c.in_rows, c.in_cols, c.mel_major_features, c.embedding_dim, c.activation) == (13, 16, 2, 63, 32, 0, 32, 2)
    c = _lib.make_config(_e2e(), FrontendConfig())
    assert (c.layer_dim, c.n_blocks) == (32, 2)                                                     # depth None travels as 2
    c = _lib.make_config(_e2e((16, 128), e2e_frontend_depth=3), FrontendConfig())
    assert (c.layer_dim, c.n_blocks, c.in_cols) == (32, 3, 128)


def test_frame_law(golden):
    d, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        lens, rows = d[f"{name}/law_samples"], d[f"{name}/law_rows"]
        assert list(lens) == [1, 16, 17, 8193, 16000, 16384, 16385, 32769]
        assert [raw_frontend_frames(cfg, int(n)) for n in lens] == list(rows), name
        assert raw_frontend_frames(cfg, d[f"{name}/pcm"].shape[1]) == cfg.input_shape[0] == d[f"{name}/frontend"].shape[2]
    assert [raw_frontend_frames(_e2e(), n) for n in (1, 64, 272, 528, 1040, 4000, 16000)] == [1, 1, 5, 9, 17, 63, 250]
    with pytest.raises(ValueError):
        raw_frontend_frames(_e2e(), 0)


def test_param_spec_equals_reference_state_dict(golden):
    d, meta = golden
    assert set(meta) == CASES
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        ref = [(k, tuple(s)) for k, s in json.loads(str(d[f"{name}/ref_spec_json"])) if not k.endswith("num_batches_tracked")]
        assert sorted(ref) == sorted(param_spec(cfg).items()), name
    s = param_spec(_e2e())
    assert s["model.frontend.conv_blocks.0.weight"] == (32, 1, 41) and s["model.frontend.conv_blocks.3.weight"] == (64, 32, 13)
    assert "model.frontend.conv_blocks.6.weight" not in s
    assert [s[f"model.backbone.conv{i}.0.weight"] for i in (1, 2, 3, 4)] == [(24, 1, 3, 3), (48, 24, 3, 3), (64, 48, 3, 3), (96, 64, 3, 3)]
    assert s["model.backbone.conv3.1.running_var"] == (64,) and s["model.backbone.fc.weight"] == (64, 96)
    assert not any(k.endswith(".0.bias") for k in s if k.startswith("model.backbone.conv"))
    # randomised statistics in the numbered BatchNorms of the backbone, as in the frontend's
    sd = synth_state_dict(_e2e())
    for k in ("model.backbone.conv1.1", "model.backbone.conv4.1", "model.frontend.conv_blocks.4"):
        assert 0.5 <= sd[k + ".running_var"].min() < sd[k + ".running_var"].max() <= 1.5 and 0.5 <= sd[k + ".weight"].min() and np.abs(sd[k + ".running_mean"]).max() > 0


def test_existing_checksums_unchanged():
    """synth.py learned the numbered BatchNorms of the backbone's stages; the heads that were there keep their weights bit for bit."""
    for f in ("heads_e2e_quartznet.npz", "heads_quartznet.npz", "heads_rnn.npz"):
        d, meta = load_head_goldens(f)
        for name, m in meta.items():
            assert state_dict_checksum(synth_state_dict(HeadConfig(**m))) == str(d[f"{name}/sd_checksum"]), name
    # the CNN head's model.conv1 / model.conv2 are not the backbone's conv1 / conv2
    sd = synth_state_dict(HeadConfig("cnn", (16, 96)))
    assert np.abs(sd["model.conv1.bias"]).max() <= 0.1 and sd["model.conv2.weight"].shape == (32, 16, 3, 3)


def test_head_macs():
    E = 64
    fe = 250 * 13 * 32 * 64 + 1000 * 41 * 32                                                        # the upper estimate: 250 x 4 rows at stage 0
    bb = 9 * (1 * 24 * 64 * 125 + 24 * 48 * 32 * 63 + 48 * 64 * 16 * 32 + 64 * 96 * 16 * 32)
    assert head_macs(_e2e()) == fe + bb + 96 * E + E * (E // 2) + E // 2
    assert abs(bb / 1e6 - 65.1) < 0.1                                                               # "about 65 MMAC per clip"
    # W = 17, H = 64: 64x9, 32x5, 16x3, 16x3
    small = _e2e((17, 64))
    assert head_macs(small) - (17 * 13 * 32 * 64 + 68 * 41 * 32) - 96 * E - E * (E // 2) - E // 2 == 9 * (24 * 64 * 9 + 24 * 48 * 32 * 5 + 48 * 64 * 16 * 3 + 64 * 96 * 16 * 3)


def test_restatement_matches_reference_golden(golden):
    """The bar test_rnn_head.py holds its restatement to: logits within 1e-6, embedding within 1e-5 relative, in float32 and in float64."""
    d, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        assert state_dict_checksum(sd) == str(d[f"{name}/sd_checksum"]), name
        for dtype in (np.float32, np.float64):
            fe, emb, lg = e2e_cnn_oracle.forward(d[f"{name}/pcm"], sd, cfg, dtype=dtype)
            ref_f, ref_e = d[f"{name}/frontend"], d[f"{name}/emb"]
            assert fe.dtype == dtype and lg.dtype == dtype and lg.shape == d[f"{name}/logits"].shape
            assert fe.shape == ref_f.shape and np.abs(fe - ref_f).max() <= 2e-5 * max(1.0, np.abs(ref_f).max()), (name, np.abs(fe - ref_f).max())
            e_emb, e_lg = np.abs(emb - ref_e).max(), np.abs(lg - d[f"{name}/logits"]).max()
            print(name, dtype.__name__, "restatement vs reference: emb %.2e logits %.2e" % (e_emb, e_lg))
            assert e_emb <= 1e-5 * max(1.0, np.abs(ref_e).max()), (name, e_emb)
            assert e_lg <= 1e-6, (name, e_lg)


def test_restatement_float32_vs_float64(golden):
    """Seed 3 noise: the float32 restatement within a tenth of LOGIT_ATOL of float64, so float64 stands in for the reference on the GPU."""
    _, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        n = min(4000, 16 * 4 ** (raw_frontend_depth(cfg) - 1) * cfg.input_shape[0])
        cfg = HeadConfig(**dict(m, input_shape=(raw_frontend_frames(cfg, n), cfg.input_shape[1])))
        pcm = synth_pcm("noise", 3, n, seed=3)
        f32, e32, l32 = e2e_cnn_oracle.forward(pcm, sd, cfg)
        f64, e64, l64 = e2e_cnn_oracle.forward(pcm, sd, cfg, dtype=np.float64)
        assert f64.dtype == np.float64 and l64.dtype == np.float64 and l32.dtype == np.float32
        assert np.abs(f32 - f64).max() <= 2e-5 * max(1.0, np.abs(f64).max()), name
        assert np.abs(l32 - l64).max() <= LOGIT_ATOL / 10, (name, np.abs(l32 - l64).max())
        # the backbone alone on the time-major frontend output is the same function
        e_b, l_b = e2e_cnn_oracle.forward_features(np.ascontiguousarray(f64.transpose(0, 2, 1)), sd, cfg, dtype=np.float64)
        assert np.array_equal(e_b, e64) and np.array_equal(l_b, l64)


def test_strided_conv_edges_against_a_direct_sum():
    """Both parities of both extents at every stride the backbone has, W = 1 and H = 1 included: the last centre reads the padding when the
    extent is odd and does not when it is even."""
    rng = np.random.default_rng(5)
    w = rng.standard_normal((3, 2, 3, 3))
    for H, W in ((1, 1), (1, 4), (5, 1), (4, 6), (5, 7), (4, 7), (5, 6)):
        x = rng.standard_normal((1, 2, H, W))
        for sh, sw in ((1, 2), (2, 2), (1, 1)):
            y = e2e_cnn_oracle.conv2d_strided(x, w, (sh, sw))
            Ho, Wo = (H - 1) // sh + 1, (W - 1) // sw + 1
            assert y.shape == (1, 3, Ho, Wo)
            ref = np.zeros_like(y)
            for i in range(Ho):
                for j in range(Wo):
                    for a in range(3):
                        for b in range(3):
                            r, c = i * sh - 1 + a, j * sw - 1 + b
                            if 0 <= r < H and 0 <= c < W:
                                ref[0, :, i, j] += w[:, :, a, b] @ x[0, :, r, c]
            assert np.abs(y - ref).max() <= 1e-12, (H, W, sh, sw)


def test_pt_ingestion(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.weights import infer_head_config, state_dict_from_pt
    cfg = _e2e((16, 64), e2e_frontend_channels=16, e2e_frontend_depth=3, embedding_dim=32)
    sd = synth_state_dict(cfg)
    path = str(tmp_path / "e2e_cnn.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    got = state_dict_from_pt(path)
    c = infer_head_config(got, input_shape=(16, 64))
    assert c == cfg
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    # the default depth comes back as the number it stands for: the same model
    d2 = infer_head_config(synth_state_dict(_e2e()), input_shape=(250, 64))
    assert d2.model_type == "e2e_cnn" and d2.e2e_frontend_depth == 2 and param_spec(d2) == param_spec(_e2e())
    with pytest.raises(ValueError, match="input_shape"):
        infer_head_config(got)
    with pytest.raises(ValueError, match="gives 64 channels"):
        infer_head_config(got, input_shape=(16, 32))
    with pytest.raises(ValueError, match="e2e_cnn"):
        infer_head_config({"classifier.0.weight": np.zeros((8, 16), np.float32)})         # the in-scope list names the head
    # the raw QuartzNet is still told apart by its backbone
    q = HeadConfig("e2e_quartznet", (63, 128))
    assert infer_head_config(synth_state_dict(q), input_shape=(63, 128)).model_type == "e2e_quartznet"


def test_onnx_ingestion():
    from nanowakeword_amd.weights import state_dict_from_onnx
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_e2e_cnn.npz"), allow_pickle=False))
    want = HeadConfig(**json.loads(str(e["meta_json"]))["e2e_cnn"])
    cfg, sd, info = state_dict_from_onnx(os.path.join(GOLDEN, "onnx", "e2e_cnn.onnx"))
    assert info["mode"] == "e2e" and info["input_ndim"] == 3 and info["clip_samples"] == 2000 and info["frontend"] is None
    assert cfg == want and (cfg.e2e_frontend_channels, cfg.e2e_frontend_depth, cfg.embedding_dim, cfg.input_shape) == (8, 2, 16, (32, 16))
    ref = synth_state_dict(want)
    assert set(sd) == set(ref)
    # the exporter folds each BatchNorm into the conv in front of it: those come back folded (the same function), the rest bit for bit
    folded = ("model.frontend.", "model.backbone.conv")
    assert all(np.array_equal(sd[k], ref[k]) for k in ref if not k.startswith(folded))
    assert sum(not k.startswith(folded) for k in ref) == 6
    al = ref["model.backbone.conv2.1.weight"] / np.sqrt(ref["model.backbone.conv2.1.running_var"] + np.float32(1e-5))
    assert np.abs(sd["model.backbone.conv2.0.weight"] - al[:, None, None, None] * ref["model.backbone.conv2.0.weight"]).max() <= 1e-6
    lg = e2e_cnn_oracle.forward(e["e2e_cnn/pcm"], sd, cfg)[2].ravel()
    print("onnx: max |dlogit| vs the reference's logits: %.2e" % np.abs(lg - e["e2e_cnn/logits"]).max())
    assert np.abs(lg - e["e2e_cnn/logits"]).max() <= 1e-5
    assert np.abs(e2e_cnn_oracle.forward(e["e2e_cnn/pcm"], ref, want)[2].ravel() - e["e2e_cnn/logits"]).max() <= 1e-5
    # the other raw-PCM export still goes its own way, and LSTMModel stays refused
    assert state_dict_from_onnx(os.path.join(GOLDEN, "onnx", "e2e_quartznet.onnx"))[0].model_type == "e2e_quartznet"


def test_bundle_round_trip(tmp_path):
    from nanowakeword_amd.weights import load_bundle, save_bundle
    cfg = _e2e((63, 64), activation="gelu")
    sd = synth_state_dict(cfg)
    path = str(tmp_path / "e2e_cnn.nww.npz")
    save_bundle(path, cfg, sd, mode="e2e", clip_samples=4000)
    head, _, got, extras, meta = load_bundle(path)
    assert head == cfg and meta["clip_samples"] == 4000 and not extras and all(np.array_equal(got[k], sd[k]) for k in sd)


# ---- the rescaled-channel probe of tests/test_raw_x3_stress.py applied to the backbone (ReLU): one channel of a stage's BatchNorm (weight and
# bias) x G and the next stage's weights on that channel / G is the same function; tests/test_gpu_e2e_cnn.py runs the same cases on the device
RESCALE = {f"conv{i}_ch{c}_2^{e}": (i, c, 2.0 ** e) for i, c in ((2, 5), (3, 40)) for e in (8, 12)}
RESCALE_SAMPLES = 4000


def rescale_case():
    """(cfg, plain weights, four clips of different kinds): the reference defaults at 4000 samples"""
    cfg = _e2e((raw_frontend_frames(_e2e(), RESCALE_SAMPLES), 64))
    pcm = np.concatenate([synth_pcm(k, 1, RESCALE_SAMPLES, seed=12) for k in ("noise", "speechlike", "sine", "loud")], 0)
    return cfg, synth_state_dict(cfg), pcm


def rescaled_sd(name):
    i, c, G = RESCALE[name]
    sd = {k: v.copy() for k, v in rescale_case()[1].items()}
    sd[f"model.backbone.conv{i}.1.weight"][c] *= np.float32(G)
    sd[f"model.backbone.conv{i}.1.bias"][c] *= np.float32(G)
    sd[f"model.backbone.conv{i + 1}.0.weight"][:, c] /= np.float32(G)
    return sd


def rel_logit_error(got, l64):
    """max |got - float64| over max(1, |float64|max): the convention of tests/test_gpu_raw_x3_stress.py's contract"""
    return float(np.abs(np.ravel(got).astype(np.float64) - np.ravel(l64)).max()) / max(1.0, float(np.abs(l64).max()))


@pytest.mark.parametrize("name", list(RESCALE))
def test_rescaled_channels_are_the_same_function_and_a_fair_probe(name):
    """Before the device sees them: the float32 restatement gives the same function before and after, the chosen weights and clips keep the
    logits apart (ptp > 1e-2: an error would show), the rescaled channel matters to them, and the float32 restatement itself is within the
    bar the device is held to (LOGIT_ATOL) and leaves the contract 2 x its own error + 2e-6 above float32 rounding."""
    cfg, sd0, pcm = rescale_case()
    sd = rescaled_sd(name)
    i, c, G = RESCALE[name]
    l64_0 = e2e_cnn_oracle.forward(pcm, sd0, cfg, dtype=np.float64)[2]
    l64 = e2e_cnn_oracle.forward(pcm, sd, cfg, dtype=np.float64)[2]
    l32_0 = e2e_cnn_oracle.forward(pcm, sd0, cfg)[2]
    l32 = e2e_cnn_oracle.forward(pcm, sd, cfg)[2]
    assert np.abs(l64 - l64_0).max() <= 1e-12 and np.abs(l32 - l32_0).max() <= 2e-6, (name, np.abs(l32 - l32_0).max())
    assert np.ptp(l32) > 1e-2, (name, l32.ravel())
    e32 = rel_logit_error(l32, l64)
    print(name, "float32 restatement vs float64: %.2e (contract for the device: %.2e); logits" % (e32, 2 * e32 + 2e-6), l32.ravel())
    assert e32 <= LOGIT_ATOL / 10
    # the channel counts: without it the logits move by far more than the contract
    dead = {k: v.copy() for k, v in sd.items()}
    dead[f"model.backbone.conv{i + 1}.0.weight"][:, c] = 0
    assert np.abs(e2e_cnn_oracle.forward(pcm, dead, cfg, dtype=np.float64)[2] - l64).max() > 1e-4, name
    # and the rescaled channel's plane really is G times louder than its neighbours'
    fe = e2e_cnn_oracle.forward(pcm, sd, cfg, dtype=np.float64)[0]
    planes = e2e_cnn_oracle.backbone_planes(fe, {k: np.asarray(v, np.float64) for k, v in sd.items()}, cfg)[i - 1]
    rest = np.delete(planes, c, axis=1)
    assert np.abs(planes[:, c]).max() > G / 64 * np.abs(rest).max(), name
