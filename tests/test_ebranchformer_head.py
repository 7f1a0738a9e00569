"""E-Branchformer head (model_type="e_branchformer"): configuration, state_dict spec, C-slot mapping, .pt / .onnx ingestion and the numpy
restatement (oracle/heads.py) against the reference-generated fixtures and against itself in float64.  CPU only."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import HEAD_CODE, FrontendConfig, HeadConfig, head_macs, param_spec
from nanowakeword_amd.synth import state_dict_checksum, synth_features, synth_state_dict
from parity import GOLDEN, load_head_goldens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_ebranchformer.npz")


def test_head_code_matches_header():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    assert int(re.search(r"#define NWW_HEAD_E_BRANCHFORMER (\d+)", hdr).group(1)) == HEAD_CODE["e_branchformer"] == 9
    cfg = HeadConfig("E_Branchformer", (16, 96))
    assert cfg.model_type == "e_branchformer" and (cfg.branchformer_d_model, cfg.branchformer_n_head) == (144, 4)
    # configs written before the E-Branchformer fields existed still load
    old = HeadConfig("conformer", (16, 96)).to_dict()
    del old["branchformer_d_model"], old["branchformer_n_head"]
    assert HeadConfig(**old).branchformer_d_model == 144


def test_config_validation():
    with pytest.raises(ValueError, match="branchformer_d_model must be divisible by branchformer_n_head"):
        HeadConfig("e_branchformer", (16, 96), branchformer_d_model=100, branchformer_n_head=3)
    with pytest.raises(ValueError, match="branchformer_d_model must be divisible by branchformer_n_head"):
        HeadConfig("e_branchformer", (16, 96), branchformer_n_head=0)
    HeadConfig("cnn", (16, 96), branchformer_d_model=100, branchformer_n_head=3)          # other heads ignore the fields


def test_nww_config_keeps_its_size_and_the_shared_attention_slots():
    from nanowakeword_amd import _lib
    assert ctypes.sizeof(_lib.NwwConfig) == 132
    c = _lib.make_config(HeadConfig("e_branchformer", (16, 96), branchformer_d_model=64, branchformer_n_head=8, conformer_d_model=144), FrontendConfig())
    assert (c.head_type, c.conformer_d_model, c.conformer_n_head) == (9, 64, 8)
    c = _lib.make_config(HeadConfig("conformer", (16, 96), branchformer_d_model=64, branchformer_n_head=8), FrontendConfig())
    assert (c.head_type, c.conformer_d_model, c.conformer_n_head) == (5, 144, 4)


def test_param_spec_equals_reference_state_dict(golden):
    d, meta = golden
    assert len(meta) == 4
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        ref = [(k, tuple(s)) for k, s in json.loads(str(d[f"{name}/ref_spec_json"])) if not k.endswith("num_batches_tracked")]
        assert sorted(ref) == sorted(param_spec(cfg).items()), name
        per_block = [k for k in param_spec(cfg) if k.startswith("model.branchformer_blocks.0.")]
        assert len(per_block) == 28, per_block
    s = param_spec(HeadConfig("e_branchformer", (101, 64)))
    assert s["model.branchformer_blocks.0.merger.gate.weight"] == (144, 144)
    assert s["model.branchformer_blocks.0.conv_branch.depthwise_conv.weight"] == (144, 1, 31)
    assert s["model.branchformer_blocks.0.attention.in_proj_weight"] == (432, 144)


def test_head_macs():
    T, F, D, E = 101, 64, 144, 64
    # per row: in_proj 3 D^2, out_proj D^2, conv1 2 D^2, depthwise 31 D, conv2 D^2, gate D^2, linear1 + linear2 8 D^2; per clip q k^T and p v
    per_block = T * (3 * D * D + D * D + 2 * D * D + 31 * D + D * D + D * D + 8 * D * D) + 2 * T * T * D
    assert head_macs(HeadConfig("e_branchformer", (T, F))) == T * F * D + per_block + D * E + E * (E // 2) + E // 2
    two, one = (HeadConfig("e_branchformer", (T, F), n_blocks=n) for n in (2, 1))
    assert head_macs(two) - head_macs(one) == per_block
    # about 0.7 x the Conformer's (a second feed-forward module against the gate)
    ratio = head_macs(one) / head_macs(HeadConfig("conformer", (T, F)))
    assert 0.6 < ratio < 0.8, ratio


def test_restatement_matches_reference_golden(golden):
    """The bar tests/test_oracle_golden.py and the other heads' restatements use: 1e-5 on the logits, 1e-5 relative on the embedding."""
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
        assert lg.dtype == np.float32 and np.abs(lg - d[f"{name}/logits_feat"]).max() <= 1e-5, (name, np.abs(lg - d[f"{name}/logits_feat"]).max())


def test_restatement_float32_vs_float64(golden):
    _, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        x = synth_features(6, cfg.input_shape, seed=3)
        e64 = oracle.head_forward(x, sd, cfg, dtype=np.float64)
        assert e64.dtype == np.float64
        e32 = oracle.head_forward(x, sd, cfg)
        assert np.abs(e32 - e64).max() <= 1e-5 * max(1.0, np.abs(e64).max()), (name, np.abs(e32 - e64).max())
        assert np.abs(oracle.model_forward(x, sd, cfg) - oracle.model_forward(x, sd, cfg, dtype=np.float64)).max() <= 1e-5, name


def test_gate_ends_select_one_branch():
    """merger.gate.bias = +30 / -30: g is 1 / 0 to float32, the block passes the attention / the conv branch only (the restatement has
    the branches the right way round: with g = 1 the conv module's weights past the gate stop mattering, with g = 0 the attention's)."""
    cfg = HeadConfig("e_branchformer", (16, 32), embedding_dim=16, branchformer_d_model=32, branchformer_n_head=4)
    x = synth_features(3, cfg.input_shape, seed=2)
    bump = np.linspace(-0.25, 0.25, 32).astype(np.float32)             # not uniform over the features: final_norm removes a uniform shift
    for bias, dead in ((30.0, "conv_branch.conv2.bias"), (-30.0, "attention.out_proj.bias")):
        sd = synth_state_dict(cfg)
        sd["model.branchformer_blocks.0.merger.gate.bias"] = np.full(32, bias, np.float32)
        base = oracle.head_forward(x, sd, cfg, dtype=np.float64)
        sd2 = dict(sd)
        # a change of the dead branch's output moves nothing (conv2's bias also shifts the gate's input: +-30 dominates it)
        sd2["model.branchformer_blocks.0." + dead] = sd["model.branchformer_blocks.0." + dead] + bump
        assert np.abs(oracle.head_forward(x, sd2, cfg, dtype=np.float64) - base).max() <= 1e-9, dead
        live = "attention.out_proj.bias" if dead.startswith("conv") else "conv_branch.conv2.bias"
        sd3 = dict(sd)
        sd3["model.branchformer_blocks.0." + live] = sd["model.branchformer_blocks.0." + live] + bump
        assert np.abs(oracle.head_forward(x, sd3, cfg, dtype=np.float64) - base).max() >= 1e-4, live


def test_pt_ingestion(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.weights import infer_head_config, state_dict_from_pt
    cfg = HeadConfig("e_branchformer", (33, 64), n_blocks=2, embedding_dim=32, branchformer_d_model=64, branchformer_n_head=8)
    sd = synth_state_dict(cfg)
    path = str(tmp_path / "eb.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    got = state_dict_from_pt(path)
    c = infer_head_config(got, input_shape=(33, 64))
    assert (c.model_type, c.n_blocks, c.branchformer_d_model, c.branchformer_n_head, c.embedding_dim) == ("e_branchformer", 2, 64, 4, 32)
    c = infer_head_config(got, input_shape=(33, 64), n_head=8)
    assert c.branchformer_n_head == 8 and c == cfg
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="input_shape"):
        infer_head_config(got)
    with pytest.raises(ValueError, match="e_branchformer"):
        infer_head_config({"classifier.0.weight": np.zeros((8, 16), np.float32)})         # the in-scope list names the head


def test_onnx_ingestion():
    from nanowakeword_amd.weights import state_dict_from_onnx
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_e_branchformer.npz"), allow_pickle=False))
    want = HeadConfig(**json.loads(str(e["meta_json"]))["e_branchformer"])
    cfg, sd, info = state_dict_from_onnx(os.path.join(GOLDEN, "onnx", "e_branchformer.onnx"))
    assert info["mode"] == "features" and info["input_ndim"] == 3
    assert cfg == want and cfg.branchformer_n_head == 8
    ref = synth_state_dict(want)
    assert set(sd) == set(ref)
    # the exporter folds the BatchNorm into the depthwise conv: those tensors come back folded (the same function), the rest bit for bit
    folded = ("depthwise_conv.", "batch_norm.")
    assert all(np.array_equal(sd[k], ref[k]) for k in ref if not any(f in k for f in folded))
    lg = oracle.model_forward(e["e_branchformer/feats"], sd, cfg).ravel()
    assert np.abs(lg - e["e_branchformer/logits"]).max() <= 1e-5
    assert np.abs(oracle.model_forward(e["e_branchformer/feats"], ref, want).ravel() - e["e_branchformer/logits"]).max() <= 1e-5
