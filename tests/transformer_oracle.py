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


def top_two_score_gaps(x, sd, cfg):
    """float64: per block, the smallest gap between the two largest scaled scores q.k / sqrt(dh) of any (clip, head, query), relative
    to max(1, the row's largest |score|) - how far the softmax rows are from a tie in their argmax, in units of the scores' own
    rounding (a one-hot softmax flips on a near-tie in any float32 arithmetic)."""
    f8 = np.float64
    w = {k: np.asarray(v, f8) for k, v in sd.items()}
    D, nh, T = cfg.transformer_d_model, cfg.transformer_n_head, x.shape[1]
    h = linear(np.asarray(x, f8), w["model.input_proj.weight"], w["model.input_proj.bias"]) * np.sqrt(f8(D)) + w["model.pos_encoder.pe"][:T, 0][None]
    gaps = []
    for i in range(cfg.n_blocks):
        p = f"model.transformer_encoder.layers.{i}"
        qkv = h @ w[p + ".self_attn.in_proj_weight"].T + w[p + ".self_attn.in_proj_bias"]
        q, k = (qkv[..., j * D:(j + 1) * D].reshape(len(x), T, nh, D // nh).transpose(0, 2, 1, 3) for j in range(2))
        s = np.sort(q @ k.transpose(0, 1, 3, 2) / np.sqrt(f8(D // nh)), axis=-1)
        top = np.maximum(1.0, np.maximum(np.abs(s[..., 0]), np.abs(s[..., -1])))
        gaps.append(float(((s[..., -1] - s[..., -2]) / top).min()) if T > 1 else float("inf"))
        h = layer_norm(h + mha(h, w, p + ".self_attn", nh), w[p + ".norm1.weight"], w[p + ".norm1.bias"])
        f = linear(np.maximum(linear(h, w[p + ".linear1.weight"], w[p + ".linear1.bias"]), 0), w[p + ".linear2.weight"], w[p + ".linear2.bias"])
        h = layer_norm(h + f, w[p + ".norm2.weight"], w[p + ".norm2.bias"])
    return gaps
