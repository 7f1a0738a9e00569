"""Numpy float32 restatement of the Transformer head (TransformerModel, architectures.py:164-206) from oracle.heads primitives.

Eval mode: dropout is identity; nn.TransformerEncoderLayer(batch_first=True) with torch's defaults - post-norm, ReLU,
layer_norm_eps 1e-5, no final norm.  Test infrastructure only (the oracle package has no Transformer of its own)."""
import numpy as np

from oracle.heads import F32, act, layer_norm, linear, mha


def transformer_head(x, sd, cfg, dtype=F32):
    """features [B, T, F] -> embedding [B, E]."""
    x = np.ascontiguousarray(x, dtype=dtype)
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    D, T = cfg.transformer_d_model, x.shape[1]
    h = linear(x, sd["model.input_proj.weight"], sd["model.input_proj.bias"]) * dtype(np.sqrt(D))
    h = h + sd["model.pos_encoder.pe"][:T, 0][None]                 # pe[t] over the batch (architectures.py:41-48)
    for i in range(cfg.n_blocks):
        p = f"model.transformer_encoder.layers.{i}"
        h = layer_norm(h + mha(h, sd, p + ".self_attn", cfg.transformer_n_head), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"])
        f = linear(np.maximum(linear(h, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"]), 0), sd[p + ".linear2.weight"], sd[p + ".linear2.bias"])
        h = layer_norm(h + f, sd[p + ".norm2.weight"], sd[p + ".norm2.bias"])
    return linear(h.mean(axis=1), sd["model.output_proj.weight"], sd["model.output_proj.bias"]).astype(dtype)


def transformer_model(x, sd, cfg, dtype=F32):
    """Model.forward: the head, then Model.classifier (model.py:291-296) -> logits [B, 1]."""
    e = transformer_head(x, sd, cfg, dtype)
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    h = act(linear(e, sd["classifier.0.weight"], sd["classifier.0.bias"]), cfg.activation)
    return linear(h, sd["classifier.3.weight"], sd["classifier.3.bias"]).astype(dtype)
