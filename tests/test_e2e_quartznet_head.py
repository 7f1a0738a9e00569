"""Raw-PCM QuartzNet head (model_type="e2e_quartznet"): configuration, frame law, state_dict spec, C-slot packing, .pt / .onnx ingestion and
the numpy restatement (tests/raw_oracle.py) against the reference-generated fixtures and against itself in float64.  CPU only."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import oracle
import raw_oracle
from nanowakeword_amd.config import HEAD_CODE, FrontendConfig, HeadConfig, head_macs, param_spec, raw_frontend_frames, raw_frontend_stages
from nanowakeword_amd.synth import state_dict_checksum, synth_pcm, synth_state_dict
from parity import GOLDEN, LOGIT_ATOL, load_head_goldens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_QC = [[64, 11, 1], [64, 13, 1], [64, 17, 1]]
CASES = {"e2e_quartznet_16000", "e2e_quartznet_8000", "e2e_quartznet_4000_c16_d2", "e2e_quartznet_4000_reps", "e2e_quartznet_4000_even_k",
         "e2e_quartznet_4000_gelu"}


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_e2e_quartznet.npz")


def _e2e(shape=(63, 128), **kw):
    return HeadConfig("e2e_quartznet", shape, **kw)


def test_head_code_matches_header_and_defaults():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    assert int(re.search(r"#define NWW_HEAD_E2E_QUARTZNET (\d+)", hdr).group(1)) == HEAD_CODE["e2e_quartznet"] == 11
    assert len(re.findall(r"^(?:int|int32_t|int64_t|void|float|const char\*)\s+nww_\w+\(", hdr, re.M)) == 48          # no new exported symbol
    cfg = HeadConfig("E2E_QuartzNet", (63, 128))
    assert cfg.model_type == "e2e_quartznet" and (cfg.e2e_frontend_channels, cfg.e2e_frontend_depth, cfg.e2e_quartznet_config) == (32, None, DEFAULT_QC)
    assert raw_frontend_stages(cfg) == [(1, 32, 41, 16), (32, 64, 13, 4), (64, 128, 13, 4)]
    assert HeadConfig(**json.loads(json.dumps(cfg.to_dict()))) == cfg
    # dicts written before the fields existed still load, for every head
    old = HeadConfig("quartznet", (16, 96)).to_dict()
    for k in ("e2e_frontend_channels", "e2e_frontend_depth", "e2e_quartznet_config"):
        del old[k]
    c = HeadConfig(**old)
    assert (c.e2e_frontend_channels, c.e2e_frontend_depth, c.e2e_quartznet_config) == (32, None, DEFAULT_QC)


def test_config_validation():
    for kw, msg in ((dict(e2e_frontend_depth=0), "depth must be 1..4"), (dict(e2e_frontend_depth=5), "depth must be 1..4"),
                    (dict(e2e_frontend_channels=0), "channels must be positive"), (dict(e2e_frontend_channels=256), "must be <= 512"),
                    (dict(e2e_quartznet_config=[]), "e2e_quartznet_config must have 1..4"), (dict(e2e_quartznet_config=[[8, 3, 1]] * 5), "1..4"),
                    (dict(e2e_quartznet_config=[[0, 3, 1]]), "channels must be positive"), (dict(e2e_quartznet_config=[[8, 0, 1]]), "kernel sizes must be 1..65535"),
                    (dict(e2e_quartznet_config=[[8, 3, 0]]), "repetitions must be >= 1"), (dict(e2e_quartznet_config=[[8, 3, 9], [8, 3, 8]]), "17 blocks; at most 16")):
        with pytest.raises(ValueError, match=msg):
            _e2e(**kw)
    with pytest.raises(ValueError, match="input_shape is what the backbone sees"):
        _e2e((63, 64))
    _e2e((63, 64), e2e_frontend_depth=2)
    _e2e((16, 512), e2e_frontend_channels=64, e2e_frontend_depth=4)
    HeadConfig("cnn", (16, 96), e2e_frontend_depth=9, e2e_quartznet_config=[[0, 0, 0]] * 7)            # other heads ignore the fields
    # the quartznet_config of this head is not validated, its own e2e_quartznet_config is
    _e2e(quartznet_config=[[0, 0, 0]] * 7)


def test_nww_config_keeps_its_size_and_packs_the_slots():
    from nanowakeword_amd import _lib
    assert ctypes.sizeof(_lib.NwwConfig) == 132
    offs = {n: getattr(_lib.NwwConfig, n).offset for n, _ in _lib.NwwConfig._fields_}
    assert (offs["layer_dim"], offs["n_blocks"], offs["n_crnn_channels"], offs["crnn_channels"], offs["mel_major_features"], offs["quartznet_kr"]) == (56, 60, 72, 76, 100, 116)
    c = _lib.make_config(_e2e((32, 32), e2e_frontend_channels=16, e2e_frontend_depth=2, e2e_quartznet_config=[[64, 11, 2], [48, 13, 1]]), FrontendConfig())
    assert (c.head_type, c.layer_dim, c.n_blocks, c.in_rows, c.in_cols, c.mel_major_features) == (11, 16, 2, 32, 32, 0)
    assert (c.n_crnn_channels, list(c.crnn_channels)[:2], list(c.quartznet_kr)) == (2, [64, 48], [11 + 2 * 65536, 13 + 65536, 0, 0])
    c = _lib.make_config(_e2e(), FrontendConfig())
    assert (c.layer_dim, c.n_blocks) == (32, 3)                                                     # depth None travels as 3


def test_frame_law(golden):
    d, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        lens, rows = d[f"{name}/law_samples"], d[f"{name}/law_rows"]
        assert list(lens) == [1, 16, 17, 8193, 16000, 16384, 16385, 32769]
        assert [raw_frontend_frames(cfg, int(n)) for n in lens] == list(rows), name
        assert raw_frontend_frames(cfg, d[f"{name}/pcm"].shape[1]) == cfg.input_shape[0] == d[f"{name}/frontend"].shape[2]
    assert [raw_frontend_frames(_e2e(), n) for n in (1, 16, 17, 8193, 16000, 16384, 16385, 32769)] == [1, 1, 1, 33, 63, 64, 65, 129]
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
    assert s["model.frontend.conv_blocks.6.weight"] == (128, 64, 13) and s["model.frontend.conv_blocks.7.running_var"] == (128,)
    assert not any(k.endswith("conv_blocks.0.bias") for k in s)
    assert s["model.backbone.quartznet_blocks.0.residual_connector.0.weight"] == (64, 128, 1) and s["model.backbone.fc.weight"] == (64, 64)
    # randomised statistics in the numbered BatchNorms of the frontend; an O(1) first layer (its input is PCM / 32768)
    sd = synth_state_dict(_e2e())
    for k in ("model.frontend.conv_blocks.1", "model.frontend.conv_blocks.4", "model.frontend.conv_blocks.7"):
        assert 0.5 <= sd[k + ".running_var"].min() < sd[k + ".running_var"].max() <= 1.5 and 0.5 <= sd[k + ".weight"].min() and np.abs(sd[k + ".running_mean"]).max() > 0
    assert np.abs(sd["model.frontend.conv_blocks.0.weight"]).max() > 0.3


def test_existing_checksums_unchanged():
    """synth.py learned the numbered BatchNorms of conv_blocks; the heads that were there keep their weights bit for bit."""
    d, meta = load_head_goldens("heads_quartznet.npz")
    for name, m in meta.items():
        assert state_dict_checksum(synth_state_dict(HeadConfig(**m))) == str(d[f"{name}/sd_checksum"]), name


def test_head_macs():
    E = 64
    # head_macs does not know the clip length: an upper estimate with rows of a stage = rows of the next x its stride (1008, 252);
    # raw_frontend_macs counts the frame law's rows (1000, 250) for a clip length
    from nanowakeword_amd.config import raw_frontend_macs
    assert raw_frontend_macs(_e2e(), 16000) == 63 * 13 * 64 * 128 + 250 * 13 * 32 * 64 + 1000 * 41 * 32 == 14677248
    fe = 63 * 13 * 64 * 128 + 252 * 13 * 32 * 64 + 1008 * 41 * 32
    qn = 63 * (11 * 128 + 2 * 128 * 64) + 63 * (13 * 64 + 64 * 64) + 63 * (17 * 64 + 64 * 64)
    assert head_macs(_e2e()) == fe + qn + 64 * E + E * (E // 2) + E // 2
    assert abs(fe / 1e6 - 14.7) < 0.1 and abs(qn / 1e6 - 1.8) < 0.1
    a, b = _e2e((16, 64), e2e_frontend_depth=2), _e2e((16, 32), e2e_frontend_depth=1)
    # one more stage (and four times the stage-0 rows); block 0 trades its projection 2 x 32 x 64 for an identity residual at 64 x 64
    assert head_macs(a) - head_macs(b) == 16 * 13 * 32 * 64 + (64 - 16) * 41 * 32 + 16 * 11 * (64 - 32)


def test_restatement_matches_reference_golden(golden):
    """The bar the other heads' restatements are held to: LOGIT_ATOL on the logits, 2e-5 relative on the embedding (and on the frontend)."""
    d, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        assert state_dict_checksum(sd) == str(d[f"{name}/sd_checksum"]), name
        fe, emb, lg = raw_oracle.forward(d[f"{name}/pcm"], sd, cfg)
        ref_f, ref_e = d[f"{name}/frontend"], d[f"{name}/emb"]
        assert fe.shape == ref_f.shape and np.abs(fe - ref_f).max() <= 2e-5 * max(1.0, np.abs(ref_f).max()), (name, np.abs(fe - ref_f).max())
        assert np.abs(emb - ref_e).max() <= 2e-5 * max(1.0, np.abs(ref_e).max()), (name, np.abs(emb - ref_e).max())
        err = np.abs(lg - d[f"{name}/logits"]).max()
        print(name, "restatement max |dlogit| vs reference: %.2e" % err)
        assert lg.dtype == np.float32 and err <= LOGIT_ATOL, (name, err)


def test_restatement_float32_vs_float64(golden):
    """Seed 3 noise: the float32 restatement within a tenth of LOGIT_ATOL of float64, so float64 stands in for the reference on the GPU."""
    _, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        n = 4000 if cfg.input_shape[0] < 32 or cfg.e2e_frontend_depth == 2 else 8000
        cfg = HeadConfig(**dict(m, input_shape=(raw_frontend_frames(cfg, n), cfg.input_shape[1])))
        pcm = synth_pcm("noise", 4, n, seed=3)
        f32, e32, l32 = raw_oracle.forward(pcm, sd, cfg)
        f64, e64, l64 = raw_oracle.forward(pcm, sd, cfg, dtype=np.float64)
        assert f64.dtype == np.float64 and l64.dtype == np.float64
        assert np.abs(f32 - f64).max() <= 2e-5 * max(1.0, np.abs(f64).max()), name
        assert np.abs(l32 - l64).max() <= LOGIT_ATOL / 10, (name, np.abs(l32 - l64).max())


def test_backbone_is_the_quartznet_head():
    cfg = _e2e()
    sd = synth_state_dict(cfg)
    q, qsd = raw_oracle.as_quartznet(cfg, sd)
    assert sorted(param_spec(q)) == sorted(qsd)
    fe, emb, lg = raw_oracle.forward(synth_pcm("noise", 2, 16000), sd, cfg)
    feats = np.ascontiguousarray(fe.transpose(0, 2, 1))
    assert np.array_equal(oracle.head_forward(feats, qsd, q), emb) and np.array_equal(oracle.model_forward(feats, qsd, q), lg)


def test_pt_ingestion(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.weights import infer_head_config, state_dict_from_pt
    cfg = _e2e((16, 32), e2e_frontend_channels=16, e2e_frontend_depth=2, e2e_quartznet_config=[[64, 11, 2], [48, 13, 1]], embedding_dim=32)
    sd = synth_state_dict(cfg)
    path = str(tmp_path / "e2e_qn.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    got = state_dict_from_pt(path)
    c = infer_head_config(got, input_shape=(16, 32))
    assert c == cfg
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    # the default depth comes back as the number it stands for: the same model
    d3 = infer_head_config(synth_state_dict(_e2e()), input_shape=(63, 128))
    assert d3.e2e_frontend_depth == 3 and param_spec(d3) == param_spec(_e2e())
    with pytest.raises(ValueError, match="input_shape"):
        infer_head_config(got)
    with pytest.raises(ValueError, match="gives 32 channels"):
        infer_head_config(got, input_shape=(16, 64))
    with pytest.raises(ValueError, match="e2e_quartznet"):
        infer_head_config({"classifier.0.weight": np.zeros((8, 16), np.float32)})         # the in-scope list names the head


def test_onnx_ingestion():
    from nanowakeword_amd.weights import state_dict_from_onnx
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_e2e_quartznet.npz"), allow_pickle=False))
    want = HeadConfig(**json.loads(str(e["meta_json"]))["e2e_quartznet"])
    cfg, sd, info = state_dict_from_onnx(os.path.join(GOLDEN, "onnx", "e2e_quartznet.onnx"))
    assert info["mode"] == "e2e" and info["input_ndim"] == 3 and info["clip_samples"] == 2000 and info["frontend"] is None
    assert cfg == want and (cfg.e2e_frontend_channels, cfg.e2e_frontend_depth, cfg.e2e_quartznet_config) == (8, 2, [[16, 5, 1], [16, 7, 2]])
    ref = synth_state_dict(want)
    assert set(sd) == set(ref)
    # the exporter folds each BatchNorm into the conv in front of it: those come back folded (the same function), the rest bit for bit
    folded = ("frontend.", "pointwise_conv.", "batch_norm.", "residual_connector.")
    assert all(np.array_equal(sd[k], ref[k]) for k in ref if not any(f in k for f in folded))
    # unfolded: alpha w of the original weights is the folded weight, beta the folded BatchNorm's bias
    al = ref["model.frontend.conv_blocks.1.weight"] / np.sqrt(ref["model.frontend.conv_blocks.1.running_var"] + np.float32(1e-5))
    assert np.abs(sd["model.frontend.conv_blocks.0.weight"] - al[:, None, None] * ref["model.frontend.conv_blocks.0.weight"]).max() <= 1e-6
    lg = raw_oracle.forward(e["e2e_quartznet/pcm"], sd, cfg)[2].ravel()
    print("onnx: max |dlogit| vs the reference's logits: %.2e" % np.abs(lg - e["e2e_quartznet/logits"]).max())
    assert np.abs(lg - e["e2e_quartznet/logits"]).max() <= LOGIT_ATOL
    assert np.abs(raw_oracle.forward(e["e2e_quartznet/pcm"], ref, want)[2].ravel() - e["e2e_quartznet/logits"]).max() <= LOGIT_ATOL


def test_bundle_round_trip(tmp_path):
    from nanowakeword_amd.weights import load_bundle, save_bundle
    cfg = _e2e((16, 128))
    sd = synth_state_dict(cfg)
    path = str(tmp_path / "e2e_qn.nww.npz")
    save_bundle(path, cfg, sd, mode="e2e", clip_samples=4000)
    head, _, got, extras, meta = load_bundle(path)
    assert head == cfg and meta["clip_samples"] == 4000 and not extras and all(np.array_equal(got[k], sd[k]) for k in sd)
