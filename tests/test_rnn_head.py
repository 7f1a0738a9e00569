"""RNN head (model_type="rnn": a bidirectional nn.LSTM of hidden size 64): configuration, state_dict spec, C-slot mapping, .pt / .onnx
ingestion and the numpy restatement (tests/rnn_oracle.py) against the reference-generated fixtures.  CPU only."""
import json
import os
import re

import numpy as np
import pytest

import oracle
import rnn_oracle
from nanowakeword_amd.config import HEAD_CODE, HEAD_TYPES, FrontendConfig, HeadConfig, head_macs, param_spec
from nanowakeword_amd.synth import state_dict_checksum, synth_state_dict
from parity import GOLDEN, load_head_goldens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"rnn_16x96": (16, 96), "rnn_101x64": (101, 64), "rnn_98x40": (98, 40), "rnn_12x32_nb2": (12, 32), "rnn_7x64_gelu": (7, 64)}


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_rnn.npz")


def test_head_code_matches_header():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    assert int(re.search(r"#define NWW_HEAD_RNN (\d+)", hdr).group(1)) == HEAD_CODE["rnn"] == 12
    assert "rnn" in HEAD_TYPES and HeadConfig("RNN", (16, 96)).model_type == "rnn"
    assert "rnn" not in oracle.heads._NETS                  # the restatement lives with the tests (rnn_oracle.py)


def test_golden_cases_are_the_issues(golden):
    d, meta = golden
    assert {n: tuple(m["input_shape"]) for n, m in meta.items()} == CASES
    assert meta["rnn_12x32_nb2"]["n_blocks"] == 2
    assert (meta["rnn_7x64_gelu"]["activation"], meta["rnn_7x64_gelu"]["embedding_dim"]) == ("gelu", 16)
    for name in CASES:
        assert d[f"{name}/feats"].shape[0] == 4
        assert ("%s/logits_pcm" % name in d) == (CASES[name] == (101, 64))


def test_param_spec_equals_reference_state_dict(golden):
    d, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        ref = [(k, tuple(s)) for k, s in json.loads(str(d[f"{name}/ref_spec_json"])) if not k.endswith("num_batches_tracked")]
        assert sorted(ref) == sorted(param_spec(cfg).items()), name
    s = param_spec(HeadConfig("rnn", (16, 96), n_blocks=2, embedding_dim=32))
    assert s["model.layer1.weight_ih_l0"] == (256, 96) and s["model.layer1.weight_ih_l1_reverse"] == (256, 128)
    assert s["model.layer1.weight_hh_l1"] == (256, 64) and s["model.layer1.bias_hh_l0_reverse"] == (256,)
    assert s["model.layer2.weight"] == (32, 128) and s["model.layer2.bias"] == (32,)


def test_layer_dim_is_not_read():
    a, b = HeadConfig("rnn", (16, 96)), HeadConfig("rnn", (16, 96), layer_dim=200)
    assert param_spec(a) == param_spec(b) and head_macs(a) == head_macs(b)
    from nanowakeword_amd import _lib
    c = _lib.make_config(b, FrontendConfig())
    assert (c.head_type, c.layer_dim, c.n_blocks) == (12, 64, 1)
    c = _lib.make_config(HeadConfig("gru", (16, 96), layer_dim=200), FrontendConfig())
    assert (c.head_type, c.layer_dim) == (3, 200)


def test_head_macs():
    T, F, E, H = 101, 64, 64, 64
    cls = E * (E // 2) + E // 2
    # one layer: T forward cells and ONE reverse cell (out[:, -1] reads the reverse direction's first step), four gates each
    assert head_macs(HeadConfig("rnn", (T, F))) == (T + 1) * 4 * H * (F + H) + 2 * H * E + cls
    # two layers: the first runs both directions in full, its 128 outputs feed the second
    T, F = 12, 32
    want = 2 * T * 4 * H * (F + H) + (T + 1) * 4 * H * (2 * H + H) + 2 * H * E + cls
    assert head_macs(HeadConfig("rnn", (T, F), n_blocks=2)) == want
    assert abs(head_macs(HeadConfig("rnn", (16, 96))) / 1e6 - 0.707) < 0.001


def test_infer_head_config_roundtrip(golden):
    from nanowakeword_amd.weights import infer_head_config
    _, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        assert infer_head_config(sd, input_shape=cfg.input_shape, activation=cfg.activation) == cfg, name
    cfg = HeadConfig("rnn", (16, 96))
    sd = synth_state_dict(cfg)
    with pytest.raises(ValueError, match="input_shape"):
        infer_head_config(sd)
    with pytest.raises(ValueError, match="expects 96 features"):
        infer_head_config(sd, input_shape=(16, 64))
    # LSTMModel's keys stay out of scope
    with pytest.raises(ValueError):
        infer_head_config({"classifier.0.weight": np.zeros((32, 64), np.float32), "model.lstm.weight_ih_l0": np.zeros((4, 4))}, (16, 96))
    lstm = {k.replace("model.layer1.", "model.lstm.").replace("model.layer2.", "model.fc."): v for k, v in sd.items()}
    with pytest.raises(ValueError, match="in-scope"):
        infer_head_config(lstm, (16, 96))
    # the DNN head shares the prefix model.layer1 and is still told apart
    dnn = HeadConfig("dnn", (16, 96), layer_dim=32)
    assert infer_head_config(synth_state_dict(dnn), input_shape=(16, 96)).model_type == "dnn"


def test_restatement_matches_reference_golden(golden):
    d, meta = golden
    for name, m in meta.items():
        cfg = HeadConfig(**m)
        sd = synth_state_dict(cfg)
        assert state_dict_checksum(sd) == str(d[f"{name}/sd_checksum"]), name
        feats = d[f"{name}/feats"]
        ref, ref_e = d[f"{name}/logits_feat"], d[f"{name}/emb_feat"]
        for dt in (np.float32, np.float64):
            lg = rnn_oracle.model_forward(feats, sd, cfg, dtype=dt)
            assert lg.dtype == dt and np.abs(lg - ref).max() <= 1e-6, (name, dt, np.abs(lg - ref).max())
            emb = rnn_oracle.head_forward(feats, sd, cfg, dtype=dt)
            assert np.abs(emb - ref_e).max() <= 1e-5 * max(1.0, np.abs(ref_e).max()), (name, dt, np.abs(emb - ref_e).max())
        # the gates are not saturated: the logits differ between clips
        assert np.ptp(ref) > 1e-2, (name, ref.ravel())


def test_pt_ingestion(tmp_path):
    torch = pytest.importorskip("torch")
    from nanowakeword_amd.weights import infer_head_config, load_bundle, save_bundle, state_dict_from_pt
    for cfg in (HeadConfig("rnn", (33, 40), embedding_dim=32, n_blocks=2), HeadConfig("rnn", (101, 64))):
        sd = synth_state_dict(cfg)
        path = str(tmp_path / "rnn.pt")
        torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
        got = state_dict_from_pt(path)
        c = infer_head_config(got, input_shape=cfg.input_shape)
        assert c == cfg, (c, cfg)
        assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
        b = str(tmp_path / "rnn.nww.npz")
        save_bundle(b, c, got, mode="features")
        head, _, sd2, _, meta = load_bundle(b)
        assert head == cfg and meta["mode"] == "features" and all(np.array_equal(sd2[k], sd[k]) for k in sd)


def test_onnx_ingestion():
    from nanowakeword_amd.onnx_reader import read_onnx
    from nanowakeword_amd.weights import state_dict_from_onnx
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_rnn.npz"), allow_pickle=False))
    want = HeadConfig(**json.loads(str(e["meta_json"]))["rnn"])
    path = os.path.join(GOLDEN, "onnx", "rnn.onnx")
    cfg, sd, info = state_dict_from_onnx(path)
    assert info["mode"] == "features" and info["input_ndim"] == 3
    assert cfg == want and cfg.input_shape == (6, 32) and cfg.embedding_dim == 16
    # nn.LSTM's [i, f, g, o] rows come back bit for bit from the exporter's [i, o, f, c] packing
    ref = synth_state_dict(want)
    assert set(sd) == set(ref) and all(np.array_equal(sd[k], ref[k]) for k in ref)
    lg = rnn_oracle.model_forward(e["rnn/feats"], sd, cfg).ravel()
    assert np.abs(lg - e["rnn/logits"]).max() <= 1e-5
    # the file holds the export's graph and weights only: one LSTM node, no convolution
    g = read_onnx(path)
    assert [n.op_type for n in g.nodes].count("LSTM") == 1 and not any(n.op_type == "Conv" for n in g.nodes)


def test_other_bare_lstm_graphs_stay_refused():
    """A bare LSTM graph whose last Linear is not model.layer2 (LSTMModel's) keeps raising NotImplementedError."""
    from nanowakeword_amd import weights
    from nanowakeword_amd.onnx_reader import read_onnx
    g = read_onnx(os.path.join(GOLDEN, "onnx", "rnn.onnx"))
    g.initializers = {k.replace("model.layer2.", "model.fc."): v for k, v in g.initializers.items()}
    for n in g.nodes:
        n.inputs = [t.replace("model.layer2.", "model.fc.") for t in n.inputs]
    import nanowakeword_amd.onnx_reader as rd
    orig = rd.read_onnx
    rd.read_onnx = lambda _: g
    try:
        with pytest.raises(NotImplementedError, match="LSTMModel"):
            weights.state_dict_from_onnx("renamed")
    finally:
        rd.read_onnx = orig
