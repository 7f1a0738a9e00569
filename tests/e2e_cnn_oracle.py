"""numpy restatement of the raw-PCM CNN head (model_type="e2e_cnn": RawAudioFrontend + RawAudioBackbone, architectures.py:692-710, 739-795).
The frontend comes from tests/raw_oracle.py; the backbone - four stages of zero-padded strided Conv2d (3x3, no bias), BatchNorm2d (eval)
and the activation, the global mean, the Linear - is restated here on oracle.heads.batch_norm / linear and oracle.classify.  Every
primitive follows its input's dtype, so the same code is the float32 and the float64 yardstick.  Test helper only: nothing under
nanowakeword_amd/ imports it."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
from scipy.special import erf

from oracle.heads import batch_norm, classify, linear

import raw_oracle
from nanowakeword_amd.config import RAW_CNN_LAYERS


def conv2d_strided(x, w, stride):
    """nn.Conv2d(Cin, Cout, 3, stride, padding=1, bias=False): x [B,Cin,H,W], w [Cout,Cin,3,3] -> [B,Cout,(H - 1) // sh + 1, (W - 1) // sw + 1]."""
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    win = sliding_window_view(xp, (3, 3), axis=(2, 3))[:, :, ::stride[0], ::stride[1]]      # [B,Cin,Ho,Wo,3,3]
    return np.ascontiguousarray(np.einsum("bchwij,ocij->bohw", win, w, optimize=True).astype(x.dtype))


def act(x, kind):
    """nn.ReLU / nn.GELU (exact erf form) / nn.SiLU in x's dtype."""
    if kind == "relu":
        return np.maximum(x, 0)
    if kind == "gelu":
        return (0.5 * x * (1.0 + erf(x / np.sqrt(x.dtype.type(2.0))))).astype(x.dtype)
    if kind == "silu":
        return (x / (1.0 + np.exp(-x))).astype(x.dtype)
    raise ValueError(kind)


def backbone_planes(image, sd, cfg):
    """image [B,H,W] (the frontend's [B,C,rows]) -> the four stages' outputs [B,Cout,Ho,Wo]."""
    h, out = image[:, None], []
    for i, (_, _, sh, sw) in enumerate(RAW_CNN_LAYERS, start=1):
        h = conv2d_strided(h, sd[f"model.backbone.conv{i}.0.weight"], (sh, sw))
        h = act(batch_norm(h, sd, f"model.backbone.conv{i}.1", axis=1), cfg.activation).astype(image.dtype)
        out.append(h)
    return out


def backbone(image, sd, cfg):
    """image [B,H,W] -> embedding [B,E]."""
    h = backbone_planes(image, sd, cfg)[-1]
    return linear(h.mean(axis=(2, 3)), sd["model.backbone.fc.weight"], sd["model.backbone.fc.bias"])


def forward(pcm, sd, cfg, dtype=np.float32):
    """int16 [B,N] -> (frontend [B,C,rows], embedding [B,E], logits [B,1]) in `dtype`."""
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    fe = raw_oracle.raw_frontend(raw_oracle.pcm_to_float(pcm, dtype), sd, cfg)
    emb = backbone(fe, sd, cfg).astype(dtype)
    return fe, emb, classify(emb, sd, cfg, dtype)


def forward_features(feats, sd, cfg, dtype=np.float32):
    """time-major frontend output [B,rows,C] -> (embedding, logits): the backbone alone."""
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    emb = backbone(np.ascontiguousarray(np.asarray(feats, dtype=dtype).transpose(0, 2, 1)), sd, cfg).astype(dtype)
    return emb, classify(emb, sd, cfg, dtype)
