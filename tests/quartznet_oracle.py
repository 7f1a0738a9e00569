"""Numpy restatement of the QuartzNet head (QuartzNetBlock / QuartzNetModel, architectures.py:370-437) from oracle.heads primitives.
Eval mode: dropout is identity, BatchNorm uses its running statistics.  Time-major throughout (x [B, T, C]); per block

    d = depthwise_conv(x)                    groups = C, bias, zero padding 'same': (k - 1) // 2 rows in front, the rest behind
    y = batch_norm(pointwise_conv(d))        no activation between the two convs
    r = BN(conv1x1(x)) where the widths differ, else x
    x = relu(y + r)                          nn.ReLU, hard-wired: activation_function reaches the classifier only

then the mean over time and fc.  Every primitive follows its input's dtype, so float64 inputs give the float64 yardstick.  Test
infrastructure only (the oracle package has no QuartzNet of its own: net_quartznet has the signature of the functions in
oracle.heads._NETS)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle.heads import F32, batch_norm, classify, linear


def depthwise_same(x, w, b):
    """nn.Conv1d(C, C, k, padding='same', groups=C) time-major: x [B, T, C], w [C, 1, k], b [C] -> [B, T, C],
    y[t, c] = b[c] + sum_j w[c, 0, j] x[t + j - (k - 1) // 2, c] with zeros outside the clip (PyTorch pads the odd row behind)."""
    k = w.shape[2]
    left = (k - 1) // 2
    xp = np.pad(x, ((0, 0), (left, k - 1 - left), (0, 0)))
    win = sliding_window_view(xp, k, axis=1)                                  # [B, T, C, k]
    return np.einsum("btck,ck->btc", win, w[:, 0, :], optimize=True).astype(x.dtype) + b


def quartznet_block(x, sd, p):
    d = depthwise_same(x, sd[p + ".depthwise_conv.weight"], sd[p + ".depthwise_conv.bias"])
    y = batch_norm(linear(d, sd[p + ".pointwise_conv.weight"][:, :, 0], sd[p + ".pointwise_conv.bias"]), sd, p + ".batch_norm", axis=2)
    r = x
    if p + ".residual_connector.0.weight" in sd:
        r = batch_norm(linear(x, sd[p + ".residual_connector.0.weight"][:, :, 0], sd[p + ".residual_connector.0.bias"]), sd,
                       p + ".residual_connector.1", axis=2)
    return np.maximum(y + r, 0).astype(x.dtype)


def net_quartznet(x, sd, cfg):
    h = x
    for i in range(sum(r for _, _, r in cfg.quartznet_config)):
        h = quartznet_block(h, sd, f"model.quartznet_blocks.{i}")
    return linear(h.mean(axis=1), sd["model.fc.weight"], sd["model.fc.bias"])


def head_forward(x, sd, cfg, dtype=F32):
    """features [B, T, F] -> embedding [B, E] (oracle.head_forward's contract)."""
    x = np.ascontiguousarray(x, dtype=dtype)
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    return net_quartznet(x, sd, cfg).astype(dtype)


def model_forward(x, sd, cfg, dtype=F32):
    """Model.forward: the head, then Model.classifier -> logits [B, 1]."""
    return classify(head_forward(x, sd, cfg, dtype), sd, cfg, dtype)
