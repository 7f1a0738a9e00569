"""Weight ingestion for the HIP path.

* ``state_dict_from_pt``  : the reference's final artefact ``<name>.pt`` = ``torch.save(model.state_dict())``
                            (reference: nanowakeword/_export/pytorch.py:26-46) -> {key: float32 ndarray}.
* ``infer_head_config``   : recover Model()'s hyper-parameters from the state_dict keys/shapes
                            (the .pt carries no config; reference: nanowakeword/modules/model.py:67-296).
* ``state_dict_from_onnx`` : the reference's deployable ``<name>.onnx`` (reference: nanowakeword/_export/onnx.py:157-229,
                            TorchScript exporter of torch 2.8) -> (HeadConfig, state_dict, info): undoes what the exporter
                            did to the weights (Conv+BN folding, Linear -> MatMul with transposed weight, GRU gate
                            re-packing) by walking the graph; no ``onnx`` package needed (``onnx_reader``).
* ``save_bundle/load_bundle/load_session`` : a self-describing ``*.nww.npz`` (config JSON + tensors +
                            optional frontend tables) that ``HipInterpreter.load_model`` accepts as a path,
                            playing the role the ``.onnx`` file plays for the reference interpreter.
"""
from __future__ import annotations

import json
import re
from typing import Mapping, Optional, Tuple

import numpy as np

from .config import FrontendConfig, HeadConfig, RAW_HEADS, RNN_HIDDEN, param_spec, raw_frontend_frames


def state_dict_from_pt(path: str) -> dict:
    import torch
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, Mapping):
        raise TypeError(f"{path} does not hold a state_dict")
    if "model_state_dict" in sd:                       # training checkpoints (train_model.py:675-705)
        sd = sd["model_state_dict"]
    return {k: v.detach().cpu().numpy().astype(np.float32) if hasattr(v, "detach") else np.asarray(v, np.float32)
            for k, v in sd.items() if not k.endswith("num_batches_tracked")}


def infer_head_config(sd: Mapping, input_shape: Optional[Tuple[int, int]] = None, activation: str = "relu",
                      n_head: Optional[int] = None) -> HeadConfig:
    """Model type / layer_dim / n_blocks / embedding_dim from key names and shapes.  ``input_shape`` is needed
    when the weights do not determine it (DNN/CNN flatten sizes fix only T*F or (T//4)*(F//4)).  ``n_head``: the
    Transformer's / E-Branchformer's attention heads (transformer_n_head / branchformer_n_head), which no weight shape records;
    default 4 as Model()'s."""
    keys = set(sd)
    shp = lambda k: tuple(np.shape(sd[k]))
    E = shp("classifier.0.weight")[1]
    kw = dict(embedding_dim=E, activation=activation)

    def n_indexed(pattern):
        idx = [int(m.group(1)) for k in keys for m in [re.match(pattern, k)] if m]
        return max(idx) + 1 if idx else 0

    def raw_frontend_shape(what):
        """(channels, depth) of the raw-PCM heads' frontend from its weights; input_shape must be what the backbone sees"""
        if input_shape is None:
            raise ValueError(f"{what}: the clip length is not in the weights; pass input_shape=(rows, channels) as the backbone sees it")
        depth = n_indexed(r"model\.frontend\.conv_blocks\.(\d+)\.running_var") // 3 + 1
        ch = shp("model.frontend.conv_blocks.0.weight")[0]
        if input_shape[1] != ch * 2 ** (depth - 1):
            raise ValueError(f"input_shape F={input_shape[1]} but the raw frontend gives {ch * 2 ** (depth - 1)} channels")
        return ch, depth

    if "model.layer1.weight_hh_l0" in keys and "model.layer2.weight" in keys:      # RNNModel (architectures.py:149-161)
        F = shp("model.layer1.weight_ih_l0")[1]
        if shp("model.layer1.weight_hh_l0") != (4 * RNN_HIDDEN, RNN_HIDDEN):
            raise ValueError(f"rnn: unexpected recurrent weight shape {shp('model.layer1.weight_hh_l0')} (an nn.LSTM of hidden size {RNN_HIDDEN})")
        if input_shape is None:
            raise ValueError("rnn: the sequence length is not in the weights; pass input_shape=(T, F)")
        if input_shape[1] != F:
            raise ValueError(f"input_shape F={input_shape[1]} but the LSTM expects {F} features")
        cfg = HeadConfig("rnn", input_shape, n_blocks=n_indexed(r"model\.layer1\.weight_hh_l(\d+)$"), **kw)
    elif "model.layer1.weight" in keys:
        L, TF = shp("model.layer1.weight")
        if input_shape is None:
            raise ValueError(f"dnn weights fix T*F={TF} only: pass input_shape=(T, F)")
        cfg = HeadConfig("dnn", input_shape, layer_dim=L, n_blocks=n_indexed(r"model\.blocks\.(\d+)\.fcn_layer\.weight"), **kw)
    elif "model.conv1.weight" in keys:
        if input_shape is None:
            raise ValueError("cnn weights fix (T//4)*(F//4) only: pass input_shape=(T, F)")
        cfg = HeadConfig("cnn", input_shape, **kw)
    elif "model.cnn.0.weight" in keys:
        chans = []
        i = 0
        while f"model.cnn.{4*i}.weight" in keys:
            chans.append(shp(f"model.cnn.{4*i}.weight")[0]); i += 1
        if input_shape is None:
            raise ValueError("crnn: pass input_shape=(T, F)")
        L = shp("model.rnn.weight_hh_l0")[1]
        gates = shp("model.rnn.weight_hh_l0")[0] // L          # nn.GRU stacks 3 gates, nn.LSTM 4 (architectures.py:238-254)
        if gates not in (3, 4) or shp("model.rnn.weight_hh_l0")[0] != gates * L:
            raise ValueError(f"crnn: unexpected recurrent weight shape {shp('model.rnn.weight_hh_l0')}")
        cfg = HeadConfig("crnn", input_shape, layer_dim=L, n_blocks=n_indexed(r"model\.rnn\.weight_hh_l(\d+)$"),
                         crnn_cnn_channels=chans, crnn_rnn_type="lstm" if gates == 4 else "gru", **kw)
    elif "model.gru.weight_hh_l0" in keys:
        L = shp("model.gru.weight_hh_l0")[1]
        F = shp("model.gru.weight_ih_l0")[1]
        if input_shape is None:
            raise ValueError("gru: the sequence length is not in the weights; pass input_shape=(T, F)")
        if input_shape[1] != F:
            raise ValueError(f"input_shape F={input_shape[1]} but the GRU expects {F} features")
        cfg = HeadConfig("gru", input_shape, layer_dim=L, n_blocks=n_indexed(r"model\.gru\.weight_hh_l(\d+)$"), **kw)
    elif "model.init_conv.0.weight" in keys:
        if input_shape is None:
            raise ValueError("bcresnet is shape-independent; pass the input_shape=(T, F) you will feed")
        cfg = HeadConfig("bcresnet", input_shape, **kw)
    elif "model.input_proj.weight" in keys and any(k.startswith("model.conformer_blocks.") for k in keys):
        D, F = shp("model.input_proj.weight")
        if input_shape is None:
            raise ValueError("conformer: pass input_shape=(T, F)")
        nb = n_indexed(r"model\.conformer_blocks\.(\d+)\.layer_norm\.weight")
        cfg = HeadConfig("conformer", input_shape, n_blocks=nb, conformer_d_model=D, **kw)
        cfg.conformer_n_head = 4          # not recoverable from weights; Model()'s default (model.py:252)
    elif "model.input_proj.weight" in keys and "model.pos_encoder.pe" in keys:
        D, F = shp("model.input_proj.weight")
        if input_shape is None:
            raise ValueError("transformer: pass input_shape=(T, F)")
        nb = n_indexed(r"model\.transformer_encoder\.layers\.(\d+)\.norm1\.weight")
        # n_head is not recoverable from the weights: Model()'s default (model.py:201) unless the caller says otherwise
        cfg = HeadConfig("transformer", input_shape, n_blocks=nb, transformer_d_model=D, transformer_n_head=n_head or 4, **kw)
    elif "model.input_proj.weight" in keys and any(k.startswith("model.branchformer_blocks.") for k in keys):
        D, F = shp("model.input_proj.weight")
        if input_shape is None:
            raise ValueError("e_branchformer: pass input_shape=(T, F)")
        nb = n_indexed(r"model\.branchformer_blocks\.(\d+)\.final_norm\.weight")
        # n_head is not recoverable from the weights: Model()'s default (model.py:273) unless the caller says otherwise
        cfg = HeadConfig("e_branchformer", input_shape, n_blocks=nb, branchformer_d_model=D, branchformer_n_head=n_head or 4, **kw)
    elif "model.tcn_blocks.0.conv1.weight" in keys:
        if input_shape is None:
            raise ValueError("tcn: the sequence length is not in the weights; pass input_shape=(T, F)")
        nl = n_indexed(r"model\.tcn_blocks\.(\d+)\.conv1\.weight")
        chans = [shp(f"model.tcn_blocks.{i}.conv1.weight")[0] for i in range(nl)]
        _, F, k = shp("model.tcn_blocks.0.conv1.weight")
        if input_shape[1] != F:
            raise ValueError(f"input_shape F={input_shape[1]} but the TCN expects {F} features")
        cfg = HeadConfig("tcn", input_shape, tcn_channels=chans, tcn_kernel_size=k, **kw)
    elif "model.frontend.conv_blocks.0.weight" in keys and any(k.startswith("model.backbone.quartznet_blocks.") for k in keys):
        ch, depth = raw_frontend_shape("e2e_quartznet")
        cfg = HeadConfig("e2e_quartznet", input_shape, e2e_frontend_channels=ch, e2e_frontend_depth=depth,
                         e2e_quartznet_config=_quartznet_entries(shp, n_indexed, "model.backbone."), **kw)
    elif "model.frontend.conv_blocks.0.weight" in keys and "model.backbone.conv1.0.weight" in keys:
        ch, depth = raw_frontend_shape("e2e_cnn")
        cfg = HeadConfig("e2e_cnn", input_shape, e2e_frontend_channels=ch, e2e_frontend_depth=depth, **kw)
    elif any(k.startswith("model.quartznet_blocks.") for k in keys):
        if input_shape is None:
            raise ValueError("quartznet: the sequence length is not in the weights; pass input_shape=(T, F)")
        F = shp("model.quartznet_blocks.0.pointwise_conv.weight")[1]
        if input_shape[1] != F:
            raise ValueError(f"input_shape F={input_shape[1]} but the QuartzNet expects {F} features")
        qc = _quartznet_entries(shp, n_indexed, "model.")
        cfg = HeadConfig("quartznet", input_shape, quartznet_config=qc, **kw)
    elif "model.conv_block.0.weight" in keys:
        cfg = HeadConfig("e2e_dnn", input_shape or (64, 101), **kw)
    else:
        raise ValueError("state_dict does not belong to an in-scope head (dnn/cnn/crnn-gru/gru/rnn/bcresnet/conformer/transformer/tcn/e_branchformer/quartznet/e2e_dnn/e2e_quartznet/e2e_cnn)")
    spec = param_spec(cfg)
    for k, s in spec.items():
        if k not in keys:
            raise KeyError(f"Missing key(s) in state_dict: '{k}'")
        if shp(k) != s:
            raise ValueError(f"size mismatch for {k}: checkpoint {shp(k)} vs model {s} (wrong input_shape?)")
    return cfg


def _quartznet_entries(shp, n_indexed, prefix):
    """[channels, kernel, repetitions] entries from the block shapes under ``prefix``: consecutive blocks of equal (channels, kernel) are
    one entry again."""
    qc = []
    for i in range(n_indexed(re.escape(prefix) + r"quartznet_blocks\.(\d+)\.pointwise_conv\.weight")):
        co = shp(f"{prefix}quartznet_blocks.{i}.pointwise_conv.weight")[0]
        k = shp(f"{prefix}quartznet_blocks.{i}.depthwise_conv.weight")[2]
        if qc and qc[-1][:2] == [co, k]:
            qc[-1][2] += 1
        else:
            qc.append([co, k, 1])
    return qc


# ---------------------------------------------------------------------------------------------------------------------
# .onnx ingestion
_WRAP = "trained_model."                 # InferenceWrapper attribute name, _export/onnx.py:163-172


def _bn_identity(sd, prefix, c, beta=None):
    """BatchNorm tensors that make ``prefix`` the exact map x -> x + beta: the exporter has already folded the trained
    statistics into the preceding Conv.  running_var = 1 - eps so that var + eps rounds to exactly 1.0f."""
    sd[prefix + ".weight"] = np.ones(c, np.float32)
    sd[prefix + ".bias"] = np.zeros(c, np.float32) if beta is None else np.asarray(beta, np.float32)
    sd[prefix + ".running_mean"] = np.zeros(c, np.float32)
    sd[prefix + ".running_var"] = np.full(c, np.float32(1.0) - np.float32(1e-5), np.float32)


def _consumers(g, tensor):
    return [n for n in g.nodes if tensor in n.inputs]


def _activation_after(g, tensor) -> str:
    ops = {n.op_type for n in _consumers(g, tensor)}
    if "Relu" in ops:
        return "relu"
    if "Sigmoid" in ops and "Mul" in ops:
        return "silu"                                  # x * sigmoid(x)
    if "Div" in ops or "Erf" in ops:
        return "gelu"                                  # 0.5 x (1 + erf(x / sqrt 2))
    raise ValueError(f"unrecognised activation pattern after '{tensor}': {sorted(ops)}")


def _unpack_onnx_gru(sd, prefix, layer, W, R, B, hidden):
    """ONNX GRU packs gates [z, r, h] per direction; nn.GRU stores [r, z, n] (torch symbolic for aten::gru)."""
    H = hidden
    perm = np.r_[H:2 * H, 0:H, 2 * H:3 * H]
    for d, sfx in enumerate(("", "_reverse")):
        sd[f"{prefix}.weight_ih_l{layer}{sfx}"] = np.ascontiguousarray(W[d][perm], np.float32)
        sd[f"{prefix}.weight_hh_l{layer}{sfx}"] = np.ascontiguousarray(R[d][perm], np.float32)
        sd[f"{prefix}.bias_ih_l{layer}{sfx}"] = np.ascontiguousarray(B[d][:3 * H][perm], np.float32)
        sd[f"{prefix}.bias_hh_l{layer}{sfx}"] = np.ascontiguousarray(B[d][3 * H:][perm], np.float32)


def _unpack_onnx_lstm(sd, prefix, layer, W, R, B, hidden):
    """ONNX LSTM packs gates [i, o, f, c] per direction; nn.LSTM stores [i, f, g, o] (torch symbolic for aten::lstm)."""
    H = hidden
    perm = np.r_[0:H, 2 * H:3 * H, 3 * H:4 * H, H:2 * H]
    for d, sfx in enumerate(("", "_reverse")):
        sd[f"{prefix}.weight_ih_l{layer}{sfx}"] = np.ascontiguousarray(W[d][perm], np.float32)
        sd[f"{prefix}.weight_hh_l{layer}{sfx}"] = np.ascontiguousarray(R[d][perm], np.float32)
        sd[f"{prefix}.bias_ih_l{layer}{sfx}"] = np.ascontiguousarray(B[d][:4 * H][perm], np.float32)
        sd[f"{prefix}.bias_hh_l{layer}{sfx}"] = np.ascontiguousarray(B[d][4 * H:][perm], np.float32)


def state_dict_from_onnx(path_or_bytes):
    """Recover (HeadConfig, state_dict, info) from a reference-exported ONNX model.

    ``info``: {"mode": "e2e"|"features", "clip_samples", "frontend": FrontendConfig|None, "opset", "producer"}.
    The state_dict uses the reference's ``Model.state_dict()`` keys.  Convs the exporter fused with their BatchNorm
    come back as (folded weight, folded bias, identity BatchNorm) - the same function, so logits agree with the
    original state_dict to float32 rounding of the folding itself.
    """
    from .onnx_reader import read_onnx
    g = read_onnx(path_or_bytes)
    if len(g.inputs) != 1 or g.inputs[0][1] is None:
        raise ValueError("expected one graph input with a static shape (reference exports name it 'input')")
    in_shape = g.inputs[0][1]
    named = {k[len(_WRAP):]: v for k, v in g.initializers.items() if k.startswith(_WRAP)}
    sd = {k: np.asarray(v, np.float32) for k, v in named.items()}
    anon = lambda t: t in g.initializers and not t.startswith(_WRAP)

    # Linear on a 3-D input is exported as MatMul(x, W^T) + Add(bias): the bias keeps its name.
    for n in g.nodes:
        if n.op_type != "MatMul" or len(n.inputs) != 2 or not anon(n.inputs[1]):
            continue
        bias = [t for c in _consumers(g, n.outputs[0]) if c.op_type == "Add" for t in c.inputs if t.startswith(_WRAP)]
        if len(bias) != 1:
            raise ValueError(f"MatMul '{n.name}': cannot identify the Linear it came from")
        b = bias[0][len(_WRAP):]
        key = b[:-len("in_proj_bias")] + "in_proj_weight" if b.endswith("in_proj_bias") else b[:-len("bias")] + "weight"
        sd[key] = np.ascontiguousarray(g.initializers[n.inputs[1]].T, np.float32)

    convs = [n for n in g.nodes if n.op_type == "Conv" and anon(n.inputs[1])]
    grus = [n for n in g.nodes if n.op_type == "GRU"]
    lstms = [n for n in g.nodes if n.op_type == "LSTM"]
    # a bare LSTM graph is the RNN head where its last Linear is named model.layer2 (RNNModel, architectures.py:149-161); LSTMModel's is not
    rnn_head = bool(lstms) and not convs and "model.layer2.weight" in named and "model.layer2.bias" in named
    if lstms and not rnn_head and not any(n.op_type == "Conv" and anon(n.inputs[1]) for n in g.nodes):
        raise NotImplementedError("model_type='lstm' (LSTMModel) is out of scope; the CRNN's LSTM backend is supported")

    def folded(node, wkey, bias_key, bn_prefix):
        W = np.asarray(g.initializers[node.inputs[1]], np.float32)
        b = np.asarray(g.initializers[node.inputs[2]], np.float32) if len(node.inputs) > 2 else np.zeros(W.shape[0], np.float32)
        sd[wkey] = W
        if bias_key is not None:
            sd[bias_key] = b
            _bn_identity(sd, bn_prefix, W.shape[0])
        else:
            _bn_identity(sd, bn_prefix, W.shape[0], beta=b)

    def gru_layers(prefix):
        for l, n in enumerate(grus):
            if n.attrs.get("direction") != b"bidirectional" or n.attrs.get("linear_before_reset", 0) != 1:
                raise ValueError(f"GRU node '{n.name}': expected the bidirectional nn.GRU export")
            H = int(n.attrs["hidden_size"])
            W, R, B = (np.asarray(g.initializers[t]) for t in n.inputs[1:4])
            _unpack_onnx_gru(sd, prefix, l, W, R, B, H)

    def lstm_layers(prefix):
        for l, n in enumerate(lstms):
            if n.attrs.get("direction") != b"bidirectional":
                raise ValueError(f"LSTM node '{n.name}': expected the bidirectional nn.LSTM export")
            H = int(n.attrs["hidden_size"])
            W, R, B = (np.asarray(g.initializers[t]) for t in n.inputs[1:4])
            _unpack_onnx_lstm(sd, prefix, l, W, R, B, H)

    def quartznet_blocks(prefix):
        # the depthwise conv keeps its name, the pointwise conv and the projection are folded with their BatchNorms
        i = 0
        while f"{_WRAP}{prefix}quartznet_blocks.{i}.depthwise_conv.weight" in g.initializers:
            p = f"{prefix}quartznet_blocks.{i}"
            dw = next(n for n in g.nodes if n.op_type == "Conv" and n.inputs[1] == f"{_WRAP}{p}.depthwise_conv.weight")
            pw = [n for n in convs if n.inputs[0] == dw.outputs[0]]
            sc = [n for n in convs if n.inputs[0] == dw.inputs[0]]
            if len(pw) != 1 or len(sc) > 1:
                raise ValueError(f"quartznet block {i}: unexpected graph structure")
            W = np.asarray(g.initializers[pw[0].inputs[1]], np.float32)
            folded(pw[0], f"{p}.pointwise_conv.weight", f"{p}.pointwise_conv.bias", f"{p}.batch_norm")
            if sc:
                folded(sc[0], f"{p}.residual_connector.0.weight", f"{p}.residual_connector.0.bias", f"{p}.residual_connector.1")
            elif W.shape[0] != W.shape[1]:
                raise ValueError(f"quartznet block {i}: widths differ but no projection was found")
            i += 1

    def raw_frontend_chain(what):
        # RawAudioFrontend: the chain of strided convs from the graph input, each folded with its BatchNorm (the convs have no bias of
        # their own, so the folded bias is the BatchNorm's beta) -> (the last stage's output tensor, the number of stages)
        if len(in_shape) not in (2, 3):
            raise ValueError(f"{what} model with input shape {in_shape}: expected [batch, 1, samples]")
        t, stage = g.inputs[0][0], 0
        while True:
            nxt = [n for n in convs if n.inputs[0] == t and int(n.attrs.get("strides", [1])[0]) > 1]
            if len(nxt) != 1:
                break
            folded(nxt[0], f"model.frontend.conv_blocks.{3*stage}.weight", None, f"model.frontend.conv_blocks.{3*stage+1}")
            relu = [n for n in _consumers(g, nxt[0].outputs[0]) if n.op_type == "Relu"]
            if len(relu) != 1:
                raise ValueError(f"{what} frontend stage {stage}: expected Conv -> Relu")
            t, stage = relu[0].outputs[0], stage + 1
        if stage == 0:
            raise ValueError(f"{what}: no strided frontend conv reads the graph input")
        return t, stage

    def raw_input_shape(model_type, stage):
        width = sd[f"model.frontend.conv_blocks.{3*(stage-1)}.weight"].shape[0]
        probe = HeadConfig(model_type, (1, width), e2e_frontend_channels=int(sd["model.frontend.conv_blocks.0.weight"].shape[0]), e2e_frontend_depth=stage)
        return (raw_frontend_frames(probe, clip_samples), width)

    mode, clip_samples, fe = "features", 16000, None
    if any(k.startswith("model.backbone.quartznet_blocks.") for k in named):        # E2ERawQuartzNet: learned filters on raw PCM, no STFT
        mode = "e2e"
        _, stage = raw_frontend_chain("e2e_quartznet")
        clip_samples = int(in_shape[-1])
        quartznet_blocks("model.backbone.")
        input_shape = raw_input_shape("e2e_quartznet", stage)
    elif "model.backbone.fc.weight" in named and any(g.initializers[n.inputs[1]].ndim == 4 for n in convs):   # E2ERawCNN: the same frontend, then
        mode = "e2e"                                                                # RawAudioBackbone's four Conv2d, each folded with its BatchNorm2d
        t, stage = raw_frontend_chain("e2e_cnn")
        clip_samples = int(in_shape[-1])
        from .config import RAW_CNN_LAYERS
        unsq = [n for n in _consumers(g, t) if n.op_type == "Unsqueeze"]
        if len(unsq) != 1:
            raise ValueError("e2e_cnn: expected the frontend's output to be unsqueezed into a one-channel image")
        conv2d = [n for n in convs if g.initializers[n.inputs[1]].ndim == 4]          # in graph order: conv1 .. conv4
        if len(conv2d) != len(RAW_CNN_LAYERS) or conv2d[0].inputs[0] != unsq[0].outputs[0]:
            raise ValueError(f"e2e_cnn: expected {len(RAW_CNN_LAYERS)} Conv2d behind the unsqueezed frontend output, found {len(conv2d)}")
        for i, (n, (cin, co, sh, sw)) in enumerate(zip(conv2d, RAW_CNN_LAYERS), start=1):
            W = g.initializers[n.inputs[1]]
            if tuple(W.shape) != (co, cin, 3, 3) or [int(v) for v in n.attrs.get("strides", [1, 1])] != [sh, sw] \
                    or [int(v) for v in n.attrs.get("pads", [0, 0, 0, 0])] != [1, 1, 1, 1]:
                raise ValueError(f"e2e_cnn backbone conv{i}: expected Conv2d({cin}, {co}, 3, stride ({sh}, {sw}), padding 1), got weights {tuple(W.shape)}")
            folded(n, f"model.backbone.conv{i}.0.weight", None, f"model.backbone.conv{i}.1")
        input_shape = raw_input_shape("e2e_cnn", stage)
    elif "model.mel_spec.real_basis" in named:                                        # E2E_MelSpectrogram_CNN
        mode = "e2e"
        clip_samples = int(in_shape[-1])
        rb, fb = named["model.mel_spec.real_basis"], named["model.mel_spec.mel_fb"]
        stft = [n for n in g.nodes if n.op_type == "Conv" and n.inputs[1] == _WRAP + "model.mel_spec.real_basis"]
        hop = int(stft[0].attrs["strides"][0])
        center = any(n.op_type == "Pad" and n.attrs.get("mode") == b"reflect" for n in g.nodes)
        fe = FrontendConfig(n_fft=int(rb.shape[-1]), win_length=int(rb.shape[-1]), hop_length=hop, n_mels=int(fb.shape[1]), center=center)
        for i, n in enumerate(convs):
            folded(n, f"model.conv_block.{4*i}.weight", f"model.conv_block.{4*i}.bias", f"model.conv_block.{4*i+1}")
        n_frames = fe.n_frames(clip_samples)
        input_shape = (fe.n_mels, n_frames)
    else:
        if len(in_shape) != 3:
            raise ValueError(f"feature-mode model with input shape {in_shape}: expected [batch, T, F]")
        input_shape = (int(in_shape[1]), int(in_shape[2]))
        if "model.block1.depthwise.weight" in named:                                # BcResNet
            folded(convs[0], "model.init_conv.0.weight", None, "model.init_conv.1")
            for i in (1, 2, 3):
                dw = next(n for n in g.nodes if n.op_type == "Conv" and n.inputs[1] == f"{_WRAP}model.block{i}.depthwise.weight")
                pw = [n for n in convs if n.inputs[0] == dw.outputs[0]]
                sc = [n for n in convs if n.inputs[0] == dw.inputs[0]]
                if len(pw) != 1 or len(sc) != 1:
                    raise ValueError(f"bcresnet block{i}: unexpected graph structure")
                folded(pw[0], f"model.block{i}.pointwise.weight", None, f"model.block{i}.bn1")
                folded(sc[0], f"model.block{i}.shortcut.0.weight", None, f"model.block{i}.shortcut.1")
        elif any(k.startswith("model.conformer_blocks.") for k in named):           # Conformer
            for i, n in enumerate(convs):
                p = f"model.conformer_blocks.{i}.conv_module"
                folded(n, f"{p}.depthwise_conv.weight", f"{p}.depthwise_conv.bias", f"{p}.batch_norm")
        elif any(k.startswith("model.branchformer_blocks.") for k in named):        # E-Branchformer: the same ConvolutionModule
            for i, n in enumerate(convs):
                p = f"model.branchformer_blocks.{i}.conv_branch"
                folded(n, f"{p}.depthwise_conv.weight", f"{p}.depthwise_conv.bias", f"{p}.batch_norm")
        elif any(k.startswith("model.quartznet_blocks.") for k in named):           # QuartzNet
            quartznet_blocks("model.")
        elif (grus or lstms) and convs:                                             # CRNN (GRU or LSTM backend)
            for i, n in enumerate(convs):
                folded(n, f"model.cnn.{4*i}.weight", f"model.cnn.{4*i}.bias", f"model.cnn.{4*i+1}")
            gru_layers("model.rnn") if grus else lstm_layers("model.rnn")
        elif grus:                                                                  # GRU
            gru_layers("model.gru")
        elif rnn_head:                                                              # RNN (bi-LSTM)
            lstm_layers("model.layer1")

    cls = [n for n in g.nodes if n.op_type == "Gemm" and len(n.inputs) > 1 and n.inputs[1] == _WRAP + "classifier.0.weight"]
    if len(cls) != 1:
        raise ValueError("no 'classifier.0' Gemm: not a reference Model export")
    act = _activation_after(g, cls[0].outputs[0])
    cfg = infer_head_config(sd, input_shape=input_shape, activation=act)
    if cfg.model_type in ("conformer", "transformer", "e_branchformer"):
        sm = [n for n in g.nodes if n.op_type == "Softmax"]
        qk = g.producer_of(sm[0].inputs[0]) if sm else None
        sc_node = g.producer_of(qk.inputs[0]) if qk is not None else None
        c = None
        if sc_node is not None and sc_node.op_type == "Mul":
            c = next((g.constant(t) for t in sc_node.inputs if g.constant(t) is not None), None)
        D = {"conformer": cfg.conformer_d_model, "transformer": cfg.transformer_d_model, "e_branchformer": cfg.branchformer_d_model}[cfg.model_type]
        if c is not None:
            n_head = D // int(round(1.0 / float(np.asarray(c).ravel()[0]) ** 2))
        else:
            # nn.TransformerEncoderLayer exports scaled_dot_product_attention with a scale computed from the shape at run time; the
            # query then goes through Reshape(q, [batch, n_head, T, head_dim]), whose only constant entry is n_head
            n_head = None
            q = g.producer_of(sc_node.inputs[0]) if sc_node is not None and sc_node.op_type == "Mul" else None
            shape = g.producer_of(q.inputs[1]) if q is not None and q.op_type == "Reshape" else None
            if shape is not None and shape.op_type == "Concat" and len(shape.inputs) == 4:
                h = g.constant(shape.inputs[1])
                n_head = int(np.asarray(h).ravel()[0]) if h is not None else None
            if not n_head:
                raise ValueError(f"{cfg.model_type}: cannot find the attention scale (1/sqrt(head_dim)) or head count in the graph")
        if cfg.model_type == "conformer":
            cfg.conformer_n_head = n_head
        elif cfg.model_type == "e_branchformer":
            cfg.branchformer_n_head = n_head
        else:
            cfg.transformer_n_head = n_head
    if g.metadata.get("mode") == "e2e" and mode != "e2e":
        raise ValueError("ONNX metadata says mode=e2e but the graph has no mel front end")
    info = {"mode": mode, "clip_samples": clip_samples, "frontend": fe, "opset": g.opset, "producer": g.producer,
            "input_ndim": len(in_shape)}
    return cfg, sd, info


def save_bundle(path: str, head: HeadConfig, state_dict: Mapping, frontend: Optional[FrontendConfig] = None,
                mode: str = "e2e", clip_samples: int = 16000, window=None, mel_fb=None):
    if not path.endswith(".npz"):
        raise ValueError("bundle path must end in .npz (convention: <name>.nww.npz)")
    fe = frontend or FrontendConfig()
    meta = {"format": "nww-bundle-1", "head": head.to_dict(), "frontend": fe.__dict__, "mode": mode, "clip_samples": clip_samples}
    arrays = {"__config__": np.array(json.dumps(meta))}
    spec = param_spec(head)
    for k in spec:
        a = state_dict[k]
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        arrays["sd/" + k] = np.asarray(a, np.float32)
    sd_keys = set(state_dict)
    if window is None and "model.mel_spec.real_basis" in sd_keys:
        rb = np.asarray(state_dict["model.mel_spec.real_basis"], np.float32)
        pad = (fe.n_fft - fe.win_length) // 2
        window = rb.reshape(rb.shape[0], -1)[0, pad:pad + fe.win_length]
    if mel_fb is None and "model.mel_spec.mel_fb" in sd_keys:
        mel_fb = np.asarray(state_dict["model.mel_spec.mel_fb"], np.float32)
    if window is not None:
        arrays["frontend.window"] = np.asarray(window, np.float32)
    if mel_fb is not None:
        arrays["frontend.mel_fb"] = np.asarray(mel_fb, np.float32)
    np.savez(path, **arrays)


def load_bundle(path: str):
    z = np.load(path, allow_pickle=False)
    meta = json.loads(str(z["__config__"]))
    if meta.get("format") != "nww-bundle-1":
        raise ValueError(f"{path}: not a nww bundle")
    hd = dict(meta["head"]); hd["input_shape"] = tuple(hd["input_shape"])
    head = HeadConfig(**hd)
    fe = FrontendConfig(**meta["frontend"])
    sd = {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
    extras = {k: z[k] for k in ("frontend.window", "frontend.mel_fb") if k in z.files}
    return head, fe, sd, extras, meta


def load_session(path: str, device: int = 0):
    """Bundle or reference .onnx -> finalized HipModel -> HipSession (raises if the HIP library or a GPU is missing)."""
    from .session import HipModel, HipSession
    if path.endswith((".pt", ".pth")):
        raise ValueError(f"{path}: a raw PyTorch state_dict carries no architecture; convert it once with "
                         "weights.state_dict_from_pt() + infer_head_config() + save_bundle() "
                         "and load the resulting .nww.npz")
    if path.endswith(".onnx"):                          # the reference's own artefact (nanointerpreter.py:955-959)
        head, sd, info = state_dict_from_onnx(path)
        fe = info["frontend"] or FrontendConfig()
        extras, meta = {}, {"mode": info["mode"], "clip_samples": info["clip_samples"], "input_ndim": info["input_ndim"]}
    else:
        head, fe, sd, extras, meta = load_bundle(path)
    # feature-mode heads never run the frontend and e2e exports carry their own tables (model.mel_spec.*): neither
    # needs torch to rebuild torchaudio's float32 tables
    feature_mode = meta.get("mode", "e2e") == "features" or head.model_type in RAW_HEADS       # (learned filters: no mel tables at all)
    own_tables = "frontend.window" in extras or any(k.startswith("model.mel_spec.") for k in sd)
    model = HipModel(head, fe, device=device, state_dict=sd, window=extras.get("frontend.window"),
                     mel_fb=extras.get("frontend.mel_fb"), tables="builtin" if (feature_mode or own_tables) else "torchaudio")
    name = path.rsplit("/", 1)[-1]
    for ext in (".nww.npz", ".npz", ".onnx"):
        if name.endswith(ext):
            name = name[:-len(ext)]
            break
    s = HipSession(model, mode=meta.get("mode", "e2e"), clip_samples=int(meta.get("clip_samples", 16000)),
                   input_ndim=int(meta.get("input_ndim", 3)), name=name)
    s.name = name
    return s
