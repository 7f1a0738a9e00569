"""Numpy float32 restatement of the TCN head (TemporalBlock / TCNModel, architectures.py:290-367) from oracle.heads primitives.

Eval mode: dropout is identity.  Level i: causal Conv1d of dilation 2^i with zero history (padding (k - 1) 2^i, the right end chopped),
relu(relu(conv2(relu(conv1(x)))) + res), res = x or the 1x1 downsample when the widths differ; the head is fc of the last time step.
Test infrastructure only (the oracle package has no TCN of its own)."""
import numpy as np

from oracle.heads import F32, act, linear


def causal_conv(x, w, b, dil):
    """x [B, T, Cin], w [Cout, Cin, k] (nn.Conv1d), b [Cout] -> y [B, T, Cout]: y[t] = b + sum_j w[:, :, j] x[t - (k - 1 - j) dil]."""
    B, T, _ = x.shape
    k = w.shape[2]
    y = np.zeros((B, T, w.shape[0]), x.dtype) + b
    for j in range(k):
        s = (k - 1 - j) * dil
        if s >= T:
            continue
        y[:, s:] += x[:, : T - s] @ w[:, :, j].T
    return y


def tcn_sequence(x, sd, cfg, dtype=F32):
    """features [B, T, F] -> the last block's output [B, T, C] (every step)."""
    h = np.ascontiguousarray(x, dtype=dtype)
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    for i, _ in enumerate(cfg.tcn_channels):
        p = f"model.tcn_blocks.{i}"
        d = 2 ** i
        o = np.maximum(causal_conv(h, sd[p + ".conv1.weight"], sd[p + ".conv1.bias"], d), 0)
        o = np.maximum(causal_conv(o, sd[p + ".conv2.weight"], sd[p + ".conv2.bias"], d), 0)
        if p + ".downsample.weight" in sd:
            res = causal_conv(h, sd[p + ".downsample.weight"], sd[p + ".downsample.bias"], 1)
        else:
            res = h
        h = np.maximum(o + res, 0).astype(dtype)
    return h


def receptive_field(cfg):
    return 1 + 2 * (cfg.tcn_kernel_size - 1) * (2 ** len(cfg.tcn_channels) - 1)


def fused_plan(cfg):
    """The fused kernel's launch plan restated (tcn_x3_plan in tcn_x3.hip): None where the stack goes to the im2col + GEMM fallback,
    else S (cone rows kept per clip), RT (32-row tiles per workgroup), NC (clips per workgroup) and the instance (1: widths <= 128,
    2: <= 256).  Tests assert the plan's own text; this is for the batch sizes and clips they pick around NC."""
    T, F = cfg.input_shape
    L, k = len(cfg.tcn_channels), cfg.tcn_kernel_size
    if not 1 <= L <= 4 or k < 2 or T < 1 or F < 1 or any(c <= 0 or c % 32 or c > 256 for c in cfg.tcn_channels):
        return None
    cmax = max([(F + 15) // 16 * 16] + list(cfg.tcn_channels))
    if cmax > 256:
        return None
    S, ld = min(T, receptive_field(cfg)), cmax + 4
    for rt in range(3 if cmax <= 128 else 1, 0, -1):
        if 32 * rt >= S and 3 * 32 * rt * (ld + 1) * 4 <= 160 * 1024:
            return {"S": S, "RT": rt, "NC": 32 * rt // S, "instance": 1 if cmax <= 128 else 2}
    return None


def tcn_head(x, sd, cfg, dtype=F32):
    """features [B, T, F] -> embedding [B, E] = fc(tcn_out[:, :, T - 1])."""
    last = tcn_sequence(x, sd, cfg, dtype)[:, -1]
    return linear(last, np.asarray(sd["model.fc.weight"], dtype), np.asarray(sd["model.fc.bias"], dtype)).astype(dtype)


def tcn_model(x, sd, cfg, dtype=F32):
    """Model.forward: the head, then Model.classifier (model.py:291-296) -> logits [B, 1]."""
    e = tcn_head(x, sd, cfg, dtype)
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    h = act(linear(e, sd["classifier.0.weight"], sd["classifier.0.bias"]), cfg.activation)
    return linear(h, sd["classifier.3.weight"], sd["classifier.3.bias"]).astype(dtype)
