"""QuartzNet head (model_type="quartznet"): configuration, state_dict spec, C-slot packing, .pt / .onnx ingestion and the numpy restatement
(oracle/heads.py) against the reference-generated fixtures and against itself in float64.  CPU only."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import HEAD_CODE, FrontendConfig, HeadConfig, head_macs, param_spec, quartznet_blocks
from nanowakeword_amd.synth import state_dict_checksum, synth_features, synth_state_dict
from parity import GOLDEN, LOGIT_ATOL, load_head_goldens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = [[256, 33, 1], [256, 33, 1], [512, 39, 1]]


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_quartznet.npz")


def _qn(shape, qc=None, **kw):
    return HeadConfig("quartznet", shape, **({} if qc is None else {"quartznet_config": qc}), **kw)


def test_head_code_matches_header():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    assert int(re.search(r"#define NWW_HEAD_QUARTZNET (\d+)", hdr).group(1)) == HEAD_CODE["quartznet"] == 10
    cfg = HeadConfig("QuartzNet", (16, 96))
    assert cfg.model_type == "quartznet" and cfg.quartznet_config == DEFAULT
    # round trip through to_dict (JSON and back: tuples become lists), and configs written before the field existed still load
    assert HeadConfig(**json.loads(json.dumps(cfg.to_dict()))) == cfg
    assert _qn((16, 96), ((64, 11, 2), (64, 13, 1))).quartznet_config == [[64, 11, 2], [64, 13, 1]]
    old = HeadConfig("conformer", (16, 96)).to_dict()
    del old["quartznet_config"]
    assert HeadConfig(**old).quartznet_config == DEFAULT


def test_config_validation_and_limits():
    for qc, msg in (([], "1..4"), ([[8, 3, 1]] * 5, "1..4"), ([[0, 3, 1]], "channels must be positive"), ([[8, 0, 1]], "kernel sizes must be 1..65535"), ([[8, 65536, 1]], "kernel sizes must be 1..65535"),
                    ([[8, 3, 0]], "repetitions must be >= 1"), ([[8, 3]], "channels, kernel, repetitions"), ([[8, 3, 9], [8, 3, 8]], "17 blocks; at most 16")):
        with pytest.raises(ValueError, match=msg):
            _qn((16, 96), qc)
    assert len(quartznet_blocks(_qn((16, 96), [[8, 3, 8], [8, 5, 8]]))) == 16
    HeadConfig("cnn", (16, 96), quartznet_config=[[0, 0, 0]] * 7)                       # other heads ignore the field
    assert quartznet_blocks(_qn((33, 64), [[64, 11, 2], [32, 13, 1]])) == [(64, 64, 11), (64, 64, 11), (64, 32, 13)]


def test_nww_config_keeps_its_size_and_packs_the_entries():
    from nanowakeword_amd import _lib
    assert ctypes.sizeof(_lib.NwwConfig) == 132
    offs = {n: getattr(_lib.NwwConfig, n).offset for n, _ in _lib.NwwConfig._fields_}
    assert (offs["n_crnn_channels"], offs["crnn_channels"], offs["conformer_d_model"], offs["act_dtype"], offs["quartznet_kr"]) == (72, 76, 92, 112, 116)
    c = _lib.make_config(_qn((33, 64), [[64, 11, 2], [48, 13, 1]]), FrontendConfig())
    assert (c.head_type, c.n_crnn_channels, list(c.crnn_channels), list(c.quartznet_kr)) == (10, 2, [64, 48, 32, 0], [11 + 2 * 65536, 13 + 65536, 0, 0])
    c = _lib.make_config(HeadConfig("tcn", (16, 96)), FrontendConfig())
    assert list(c.quartznet_kr) == [0, 0, 0, 0] and c.n_crnn_channels == 3
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    assert "int32_t quartznet_kr[4];" in hdr and "kernel + 65536 * repetitions" in hdr


def test_param_spec_equals_reference_state_dict(golden):
    d, meta = golden
    assert len(meta) == 9
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        ref = [(k, tuple(s)) for k, s in json.loads(str(d[f"{name}/ref_spec_json"])) if not k.endswith("num_batches_tracked")]
        assert sorted(ref) == sorted(param_spec(cfg).items()), name
    s = param_spec(_qn((101, 64)))
    assert s["model.quartznet_blocks.0.depthwise_conv.weight"] == (64, 1, 33) and s["model.quartznet_blocks.0.pointwise_conv.weight"] == (256, 64, 1)
    assert s["model.quartznet_blocks.0.residual_connector.0.weight"] == (256, 64, 1) and s["model.quartznet_blocks.0.residual_connector.1.running_var"] == (256,)
    assert not any(k.startswith("model.quartznet_blocks.1.residual_connector") for k in s)          # 256 -> 256: identity residual
    assert s["model.quartznet_blocks.2.depthwise_conv.weight"] == (256, 1, 39) and s["model.fc.weight"] == (64, 512)
    # randomised BatchNorm statistics, also in the projection's (a numbered member of an nn.Sequential)
    sd = synth_state_dict(_qn((16, 96)))
    for k in ("model.quartznet_blocks.0.batch_norm", "model.quartznet_blocks.0.residual_connector.1"):
        assert 0.5 <= sd[k + ".running_var"].min() < sd[k + ".running_var"].max() <= 1.5 and 0.5 <= sd[k + ".weight"].min() and np.abs(sd[k + ".running_mean"]).max() > 0


def test_head_macs():
    T, F, E = 101, 64, 64
    hand = T * (33 * 64 + 64 * 256 + 64 * 256) + T * (33 * 256 + 256 * 256) + T * (39 * 256 + 256 * 512 + 256 * 512) + 512 * E + E * (E // 2) + E // 2
    assert head_macs(_qn((T, F))) == hand == 38515040
    contractions = T * (2 * 64 * 256 + 256 * 256 + 2 * 256 * 512)
    assert abs(contractions / 1e6 - 36.4) < 0.05
    a, b = _qn((33, 64), [[64, 11, 2]]), _qn((33, 64), [[64, 11, 1]])
    assert head_macs(a) - head_macs(b) == 33 * (11 * 64 + 64 * 64)                             # an identity-residual block


def test_restatement_matches_reference_golden(golden):
    """The bar tests/test_oracle_golden.py holds the other heads' restatements to: LOGIT_ATOL on the logits, 2e-5 relative on the embedding."""
    d, meta = golden
    assert {"quartznet_16x96", "quartznet_101x64", "quartznet_98x40", "quartznet_33x64_reps", "quartznet_101x64_e2e_widths", "quartznet_33x64_even_k",
            "quartznet_5x12", "quartznet_16x96_outlier", "quartznet_16x96_gelu"} == set(meta)
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        assert state_dict_checksum(sd) == str(d[f"{name}/sd_checksum"]), name
        feats = d[f"{name}/feats"]
        emb = oracle.head_forward(feats, sd, cfg)
        ref_e = d[f"{name}/emb_feat"]
        assert np.abs(emb - ref_e).max() <= 2e-5 * max(1.0, np.abs(ref_e).max()), (name, np.abs(emb - ref_e).max())
        lg = oracle.model_forward(feats, sd, cfg)
        err = np.abs(lg - d[f"{name}/logits_feat"]).max()
        print(name, "restatement max |dlogit| vs reference: %.2e" % err)
        assert lg.dtype == np.float32 and err <= LOGIT_ATOL, (name, err)
    # the outlier case: one frame x32 (the reference's own float32 logit loses about a digit per x10 of it and sits 1e-5 from float64 here, so
    # LOGIT_ATOL still means something; the x1e4 frame is judged against float64 on the GPU); it differs from its plain twin in that clip only
    a, b = d["quartznet_16x96/logits_feat"].ravel(), d["quartznet_16x96_outlier/logits_feat"].ravel()
    assert np.abs(d["quartznet_16x96_outlier/feats"]).max() > 2000 and a[0] == b[0] and a[2] == b[2] and abs(a[1] - b[1]) > 1.0
    assert d["quartznet_101x64/logits_pcm"].shape == (16, 1)


def test_restatement_float32_vs_float64(golden):
    _, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        x = synth_features(6, cfg.input_shape, seed=3)
        e64 = oracle.head_forward(x, sd, cfg, dtype=np.float64)
        assert e64.dtype == np.float64
        e32 = oracle.head_forward(x, sd, cfg)
        assert np.abs(e32 - e64).max() <= 2e-5 * max(1.0, np.abs(e64).max()), (name, np.abs(e32 - e64).max())
        assert np.abs(oracle.model_forward(x, sd, cfg) - oracle.model_forward(x, sd, cfg, dtype=np.float64)).max() <= LOGIT_ATOL, name


def test_even_kernel_padding_and_kernel_longer_than_the_clip():
    """padding='same' with an even kernel: (k - 1) // 2 rows in front, k // 2 behind.  An impulse at t0 through taps w lands at
    t0 + (k - 1) // 2 - j for tap j; a kernel longer than the clip only ever sees its middle taps."""
    for T, k in ((9, 4), (9, 5), (5, 8), (5, 9), (3, 12)):
        w = np.arange(1, k + 1, dtype=np.float64).reshape(1, 1, k)
        for t0 in (0, T // 2, T - 1):
            x = np.zeros((1, T, 1)); x[0, t0, 0] = 1.0
            y = oracle.depthwise_same(x, w, np.zeros(1))[0, :, 0]
            want = np.zeros(T)
            for j in range(k):
                t = t0 + (k - 1) // 2 - j
                if 0 <= t < T:
                    want[t] = w[0, 0, j]
            assert np.array_equal(y, want), (T, k, t0, y, want)
    torch = pytest.importorskip("torch")
    for T, k in ((9, 4), (5, 8), (5, 9)):
        conv = torch.nn.Conv1d(3, 3, k, padding="same", groups=3).double()
        x = torch.randn(2, 3, T, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            ref = conv(x).numpy().transpose(0, 2, 1)
        got = oracle.depthwise_same(x.numpy().transpose(0, 2, 1), conv.weight.detach().numpy(), conv.bias.detach().numpy())
        assert np.abs(got - ref).max() <= 1e-12, (T, k)


def test_activation_reaches_the_classifier_only():
    relu, gelu = _qn((16, 96)), _qn((16, 96), activation="gelu")
    sd = synth_state_dict(relu)
    assert state_dict_checksum(sd) == state_dict_checksum(synth_state_dict(gelu))
    x = synth_features(4, (16, 96), seed=5)
    assert np.array_equal(oracle.head_forward(x, sd, relu), oracle.head_forward(x, sd, gelu))          # the blocks stay ReLU
    assert np.abs(oracle.model_forward(x, sd, relu) - oracle.model_forward(x, sd, gelu)).max() > 1e-3
    e = oracle.head_forward(x, sd, gelu)
    assert np.array_equal(oracle.model_forward(x, sd, gelu), oracle.classify(e, sd, gelu))


def test_pt_ingestion(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.weights import infer_head_config, state_dict_from_pt
    # repetitions come back run-length merged: [64, 11] twice (the second an identity residual), then [64, 13], then [96, 13] twice
    cfg = _qn((33, 64), [[64, 11, 2], [64, 13, 1], [96, 13, 2]], embedding_dim=32)
    sd = synth_state_dict(cfg)
    path = str(tmp_path / "qn.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    got = state_dict_from_pt(path)
    c = infer_head_config(got, input_shape=(33, 64))
    assert c == cfg and c.quartznet_config == [[64, 11, 2], [64, 13, 1], [96, 13, 2]]
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    # entries the user wrote apart that are equal merge too: the same model
    split = _qn((33, 64), [[64, 11, 1], [64, 11, 1]], embedding_dim=32)
    merged = infer_head_config(synth_state_dict(split), input_shape=(33, 64))
    assert merged.quartznet_config == [[64, 11, 2]] and param_spec(merged) == param_spec(split)
    with pytest.raises(ValueError, match="input_shape"):
        infer_head_config(got)
    with pytest.raises(ValueError, match="expects 64 features"):
        infer_head_config(got, input_shape=(33, 40))
    with pytest.raises(ValueError, match="quartznet"):
        infer_head_config({"classifier.0.weight": np.zeros((8, 16), np.float32)})         # the in-scope list names the head


def test_onnx_ingestion():
    from nanowakeword_amd.weights import state_dict_from_onnx
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_quartznet.npz"), allow_pickle=False))
    want = HeadConfig(**json.loads(str(e["meta_json"]))["quartznet"])
    cfg, sd, info = state_dict_from_onnx(os.path.join(GOLDEN, "onnx", "quartznet.onnx"))
    assert info["mode"] == "features" and info["input_ndim"] == 3
    assert cfg == want and cfg.quartznet_config == [[32, 5, 1], [48, 7, 2]]
    ref = synth_state_dict(want)
    assert set(sd) == set(ref)
    # the exporter folds each BatchNorm into the 1x1 conv in front of it: those come back folded (the same function), the rest bit for bit
    folded = ("pointwise_conv.", "batch_norm.", "residual_connector.")
    assert all(np.array_equal(sd[k], ref[k]) for k in ref if not any(f in k for f in folded))
    lg = oracle.model_forward(e["quartznet/feats"], sd, cfg).ravel()
    print("onnx: max |dlogit| vs the reference's logits: %.2e" % np.abs(lg - e["quartznet/logits"]).max())
    assert np.abs(lg - e["quartznet/logits"]).max() <= LOGIT_ATOL
    assert np.abs(oracle.model_forward(e["quartznet/feats"], ref, want).ravel() - e["quartznet/logits"]).max() <= LOGIT_ATOL
