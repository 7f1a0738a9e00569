"""Transformer head (model_type="transformer"): configuration, state_dict spec, C-slot mapping, .pt / .onnx ingestion and the numpy
restatement against the reference-generated fixtures.  CPU only."""
import json
import os
import re

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import HEAD_CODE, FrontendConfig, HeadConfig, head_macs, param_spec
from nanowakeword_amd.synth import positional_encoding, state_dict_checksum, synth_state_dict
from parity import GOLDEN, load_head_goldens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_transformer.npz")


def test_head_code_matches_header():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    assert int(re.search(r"#define NWW_HEAD_TRANSFORMER (\d+)", hdr).group(1)) == HEAD_CODE["transformer"] == 7
    cfg = HeadConfig("Transformer", (16, 96))
    assert cfg.model_type == "transformer" and (cfg.transformer_d_model, cfg.transformer_n_head) == (128, 4)
    # configs written before the Transformer fields existed still load
    old = HeadConfig("conformer", (16, 96)).to_dict()
    del old["transformer_d_model"], old["transformer_n_head"]
    assert HeadConfig(**old).transformer_d_model == 128


def test_param_spec_equals_reference_state_dict(golden):
    d, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        ref = [(k, tuple(s)) for k, s in json.loads(str(d[f"{name}/ref_spec_json"])) if not k.endswith("num_batches_tracked")]
        assert sorted(ref) == sorted(param_spec(cfg).items()), name
        assert param_spec(cfg)["model.pos_encoder.pe"] == (5000, 1, cfg.transformer_d_model)


def test_head_macs():
    T, F, D, E = 16, 96, 128, 64
    per_layer = T * 3 * D * D + 2 * T * T * D + T * D * D + 2 * T * D * 4 * D
    assert head_macs(HeadConfig("transformer", (T, F))) == T * F * D + per_layer + D * E + E * (E // 2) + E // 2
    assert abs(per_layer / 1e6 - 3.2) < 0.05                             # ~3.4 M with the input projection
    two = HeadConfig("transformer", (101, 64), n_blocks=2, transformer_d_model=64, transformer_n_head=2)
    one = HeadConfig("transformer", (101, 64), n_blocks=1, transformer_d_model=64, transformer_n_head=2)
    assert head_macs(two) - head_macs(one) == 101 * 3 * 64 * 64 + 2 * 101 * 101 * 64 + 101 * 64 * 64 + 2 * 101 * 64 * 256


def test_make_config_maps_the_shared_attention_slots():
    from nanowakeword_amd import _lib
    c = _lib.make_config(HeadConfig("transformer", (16, 96), transformer_d_model=64, transformer_n_head=8, conformer_d_model=144), FrontendConfig())
    assert (c.head_type, c.conformer_d_model, c.conformer_n_head) == (7, 64, 8)
    c = _lib.make_config(HeadConfig("conformer", (16, 96), transformer_d_model=64, transformer_n_head=8), FrontendConfig())
    assert (c.head_type, c.conformer_d_model, c.conformer_n_head) == (5, 144, 4)


def test_synth_pe_is_the_sinusoidal_table():
    cfg = HeadConfig("transformer", (16, 96), transformer_d_model=32, transformer_n_head=2)
    pe = synth_state_dict(cfg)["model.pos_encoder.pe"]
    t = np.arange(5000)[:, None].astype(np.float64)
    div = np.exp(np.arange(0, 32, 2) * (-np.log(10000.0) / 32))
    assert pe.shape == (5000, 1, 32) and pe.dtype == np.float32
    assert np.abs(pe[:, 0, 0::2] - np.sin(t * div)).max() < 2e-3                   # float32 arguments up to 5000
    assert np.abs(pe[:100, 0, 1::2] - np.cos(t[:100] * div)).max() < 1e-5
    assert np.array_equal(positional_encoding(5000, 32), pe)


def test_restatement_matches_reference_golden(golden):
    d, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        assert state_dict_checksum(sd) == str(d[f"{name}/sd_checksum"]), name
        feats = d[f"{name}/feats"]
        emb = oracle.head_forward(feats, sd, cfg)
        ref_e = d[f"{name}/emb_feat"]
        assert np.abs(emb - ref_e).max() <= 1e-5 * max(1.0, np.abs(ref_e).max()), (name, np.abs(emb - ref_e).max())
        lg = oracle.model_forward(feats, sd, cfg)
        assert np.abs(lg - d[f"{name}/logits_feat"]).max() <= 1e-5, (name, np.abs(lg - d[f"{name}/logits_feat"]).max())
    # the outlier case differs from its plain twin in exactly the clip with the loud frame
    a, b = d["transformer_16x96/logits_feat"].ravel(), d["transformer_16x96_outlier/logits_feat"].ravel()
    assert np.array_equal(a[[0, 2, 3]], b[[0, 2, 3]]) and abs(a[1] - b[1]) > 1e-2
    assert np.abs(d["transformer_16x96_outlier/feats"]).max() > 1e5


def test_pt_ingestion(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.weights import infer_head_config, state_dict_from_pt
    cfg = HeadConfig("transformer", (33, 64), n_blocks=2, embedding_dim=32, transformer_d_model=64, transformer_n_head=8)
    sd = synth_state_dict(cfg)
    path = str(tmp_path / "tf.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    got = state_dict_from_pt(path)
    c = infer_head_config(got, input_shape=(33, 64))
    assert (c.model_type, c.n_blocks, c.transformer_d_model, c.transformer_n_head, c.embedding_dim) == ("transformer", 2, 64, 4, 32)
    c = infer_head_config(got, input_shape=(33, 64), n_head=8)
    assert c.transformer_n_head == 8 and c == cfg
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="input_shape"):
        infer_head_config(got)


def test_onnx_ingestion():
    from nanowakeword_amd.weights import state_dict_from_onnx
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_transformer.npz"), allow_pickle=False))
    want = HeadConfig(**json.loads(str(e["meta_json"]))["transformer"])
    cfg, sd, info = state_dict_from_onnx(os.path.join(GOLDEN, "onnx", "transformer.onnx"))
    assert info["mode"] == "features" and info["input_ndim"] == 3
    assert cfg == want and cfg.transformer_n_head == 8
    ref = synth_state_dict(want)
    assert set(sd) == set(ref) and all(np.array_equal(sd[k], ref[k]) for k in ref)
    lg = oracle.model_forward(e["transformer/feats"], sd, cfg).ravel()
    assert np.abs(lg - e["transformer/logits"]).max() <= 1e-5
