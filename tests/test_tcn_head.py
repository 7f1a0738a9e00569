"""TCN head (model_type="tcn"): configuration, state_dict spec, C-slot mapping, .pt / .onnx ingestion and the numpy restatement
against the reference-generated fixtures.  CPU only."""
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
    return load_head_goldens("heads_tcn.npz")


def test_head_code_matches_header():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    assert int(re.search(r"#define NWW_HEAD_TCN (\d+)", hdr).group(1)) == HEAD_CODE["tcn"] == 8
    cfg = HeadConfig("TCN", (16, 96))
    assert cfg.model_type == "tcn" and (cfg.tcn_channels, cfg.tcn_kernel_size) == ([64, 64, 128], 3)
    # configs written before the TCN fields existed still load
    old = HeadConfig("conformer", (16, 96)).to_dict()
    del old["tcn_channels"], old["tcn_kernel_size"]
    assert HeadConfig(**old).tcn_channels == [64, 64, 128]


def test_config_rejects_what_the_reference_or_the_abi_cannot_take():
    with pytest.raises(ValueError, match="tcn_kernel_size"):
        HeadConfig("tcn", (16, 96), tcn_kernel_size=1)
    with pytest.raises(ValueError, match="1..4 levels"):
        HeadConfig("tcn", (16, 96), tcn_channels=[32] * 5)
    with pytest.raises(ValueError, match="1..4 levels"):
        HeadConfig("tcn", (16, 96), tcn_channels=[])
    with pytest.raises(ValueError, match="positive"):
        HeadConfig("tcn", (16, 96), tcn_channels=[64, 0])
    HeadConfig("cnn", (16, 96), tcn_kernel_size=1)          # other heads ignore the TCN fields


def test_param_spec_equals_reference_state_dict(golden):
    d, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        ref = [(k, tuple(s)) for k, s in json.loads(str(d[f"{name}/ref_spec_json"])) if not k.endswith("num_batches_tracked")]
        assert sorted(ref) == sorted(param_spec(cfg).items()), name
    # the downsample exists only where the widths differ: (101, 64) block 0 has none, (16, 96) block 0 has one
    assert "model.tcn_blocks.0.downsample.weight" not in param_spec(HeadConfig("tcn", (101, 64)))
    assert param_spec(HeadConfig("tcn", (16, 96)))["model.tcn_blocks.0.downsample.weight"] == (64, 96, 1)
    assert param_spec(HeadConfig("tcn", (16, 96)))["model.tcn_blocks.2.conv2.weight"] == (128, 128, 3)


def test_head_macs():
    T, F, E = 16, 96, 64
    conv = T * 3 * (96 * 64 + 64 * 64) + T * 96 * 64 + T * 3 * (64 * 64 * 2) + T * 3 * (64 * 128 + 128 * 128) + T * 64 * 128
    assert head_macs(HeadConfig("tcn", (T, F))) == conv + 128 * E + E * (E // 2) + E // 2
    assert abs(conv / 1e6 - 2.29) < 0.01                     # the reference's full-sequence count at (16, 96)
    full = head_macs(HeadConfig("tcn", (101, 64))) - 128 * E - E * (E // 2) - E // 2
    assert abs(full / 1e6 - 13.2) < 0.05


def test_make_config_maps_the_shared_slots():
    from nanowakeword_amd import _lib
    c = _lib.make_config(HeadConfig("tcn", (16, 96), tcn_channels=[24, 40, 56], tcn_kernel_size=5, layer_dim=77,
                                    crnn_cnn_channels=[8, 8]), FrontendConfig())
    assert (c.head_type, c.layer_dim, c.n_crnn_channels) == (8, 5, 3)
    assert list(c.crnn_channels)[:3] == [24, 40, 56]
    c = _lib.make_config(HeadConfig("crnn", (16, 96), tcn_channels=[24, 40, 56], tcn_kernel_size=5), FrontendConfig())
    assert (c.head_type, c.layer_dim, c.n_crnn_channels) == (2, 128, 3) and list(c.crnn_channels)[:3] == [16, 32, 32]


def test_create_rejects_bad_tcn_configs():
    """nww_create itself refuses what HeadConfig refuses (a C caller fills nww_config directly)."""
    import ctypes as C
    from nanowakeword_amd import _lib
    lib = _lib.load_library()
    for k, n, ch, msg in ((1, 3, (64, 64, 128), b"tcn_kernel_size"), (3, 0, (), b"1..4 levels"), (3, 5, (8,) * 4, b"1..4 levels"),
                          (3, 2, (64, -1), b"positive")):
        c = _lib.make_config(HeadConfig("tcn", (16, 96)), FrontendConfig())
        c.layer_dim, c.n_crnn_channels = k, n
        for i, v in enumerate(ch[:4]):
            c.crnn_channels[i] = v
        h = C.c_void_p()
        assert lib.nww_create(C.byref(c), C.byref(h)) != 0
        assert msg in lib.nww_last_error(None), lib.nww_last_error(None)


def test_restatement_matches_reference_golden(golden):
    d, meta = golden
    assert {"tcn_16x96", "tcn_101x64", "tcn_98x40", "tcn_16x96_guide", "tcn_33x64_nods", "tcn_5x12", "tcn_16x96_outlier",
            "tcn_16x96_gelu"} <= set(meta)
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        assert state_dict_checksum(sd) == str(d[f"{name}/sd_checksum"]), name
        feats = d[f"{name}/feats"]
        emb = oracle.head_forward(feats, sd, cfg)
        ref_e = d[f"{name}/emb_feat"]
        assert np.abs(emb - ref_e).max() <= 1e-5 * max(1.0, np.abs(ref_e).max()), (name, np.abs(emb - ref_e).max())
        ref = d[f"{name}/logits_feat"]
        lg = oracle.model_forward(feats, sd, cfg)
        assert np.all(np.abs(lg - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))), (name, np.abs(lg - ref).max())
    # the outlier case differs from its plain twin in exactly the clip with the loud frame
    a, b = d["tcn_16x96/logits_feat"].ravel(), d["tcn_16x96_outlier/logits_feat"].ravel()
    assert np.array_equal(a[[0, 2, 3]], b[[0, 2, 3]]) and abs(a[1] - b[1]) > 1e-2
    assert np.abs(d["tcn_16x96_outlier/feats"]).max() > 1e5


def test_restatement_reads_only_the_cone():
    """The head depends on the last 1 + 2 (k - 1) (2^L - 1) steps only (29 at the defaults, 91 for the guide's stack)."""
    cfg = HeadConfig("tcn", (101, 64))
    assert oracle.tcn_receptive_field(cfg) == 29
    assert oracle.tcn_receptive_field(HeadConfig("tcn", (16, 96), tcn_channels=[128, 128, 256, 256], tcn_kernel_size=4)) == 91
    sd = synth_state_dict(cfg)
    x = synth_features(3, cfg.input_shape, seed=4)
    y = x.copy()
    y[:, : 101 - 29] = 1e3
    assert np.array_equal(oracle.model_forward(x, sd, cfg), oracle.model_forward(y, sd, cfg))
    y[:, 101 - 29] += 1.0
    assert not np.array_equal(oracle.model_forward(x, sd, cfg), oracle.model_forward(y, sd, cfg))


def test_pt_ingestion(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.weights import infer_head_config, state_dict_from_pt
    for cfg in (HeadConfig("tcn", (33, 40), embedding_dim=32, tcn_channels=[32, 48, 48], tcn_kernel_size=4),
                HeadConfig("tcn", (101, 64))):
        sd = synth_state_dict(cfg)
        path = str(tmp_path / "tcn.pt")
        torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
        got = state_dict_from_pt(path)
        c = infer_head_config(got, input_shape=cfg.input_shape)
        assert c == cfg, (c, cfg)
        assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
        with pytest.raises(ValueError, match="input_shape"):
            infer_head_config(got)


def test_onnx_ingestion():
    from nanowakeword_amd.weights import state_dict_from_onnx
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_tcn.npz"), allow_pickle=False))
    want = HeadConfig(**json.loads(str(e["meta_json"]))["tcn"])
    cfg, sd, info = state_dict_from_onnx(os.path.join(GOLDEN, "onnx", "tcn.onnx"))
    assert info["mode"] == "features" and info["input_ndim"] == 3
    assert cfg == want and cfg.tcn_channels == [16, 32]
    ref = synth_state_dict(want)
    assert set(sd) == set(ref) and all(np.array_equal(sd[k], ref[k]) for k in ref)
    lg = oracle.model_forward(e["tcn/feats"], sd, cfg).ravel()
    assert np.abs(lg - e["tcn/logits"]).max() <= 1e-5
