"""numpy restatement of the raw-PCM head (model_type="e2e_quartznet": RawAudioFrontend + QuartzNetModel, architectures.py:692-710, 798-817).
The frontend - zero-padded strided Conv1d (no bias), BatchNorm1d (eval), ReLU per stage - is restated here; the backbone is
oracle.heads.quartznet_block / linear under the model.backbone prefix, the classifier oracle.classify.  Every primitive follows its input's
dtype, so the same code is the float32 and the float64 yardstick.  Test helper only: nothing under nanowakeword_amd/ imports it."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle.heads import batch_norm, classify, linear, quartznet_block

from nanowakeword_amd.config import raw_frontend_stages


def conv1d_strided(x, w, stride):
    """nn.Conv1d(Cin, Cout, k, stride, padding=k // 2, bias=False): x [B,Cin,L], w [Cout,Cin,k] -> [B,Cout,(L - 1) // stride + 1] for odd k."""
    k = w.shape[2]
    xp = np.pad(x, ((0, 0), (0, 0), (k // 2, k // 2)))
    win = sliding_window_view(xp, k, axis=2)[:, :, ::stride]                  # [B,Cin,L',k]
    return np.einsum("bclk,ock->bol", win, w, optimize=True).astype(x.dtype)


def raw_frontend(x, sd, cfg):
    """x [B,N] (PCM / 32768) -> [B, C, rows], the reference's layout."""
    h = x[:, None, :]
    for i, (_, _, _, stride) in enumerate(raw_frontend_stages(cfg)):
        h = conv1d_strided(h, sd[f"model.frontend.conv_blocks.{3 * i}.weight"], stride)
        h = np.maximum(batch_norm(h, sd, f"model.frontend.conv_blocks.{3 * i + 1}", axis=1), 0).astype(x.dtype)
    return h


def backbone(feats, sd, cfg):
    """feats [B,rows,C] -> embedding [B,E]: the QuartzNet under model.backbone."""
    h = feats
    for i in range(sum(r for _, _, r in cfg.e2e_quartznet_config)):
        h = quartznet_block(h, sd, f"model.backbone.quartznet_blocks.{i}")
    return linear(h.mean(axis=1), sd["model.backbone.fc.weight"], sd["model.backbone.fc.bias"])


def pcm_to_float(pcm, dtype=np.float32):
    return (np.asarray(pcm).astype(dtype) / dtype(32768.0)).astype(dtype)


def forward(pcm, sd, cfg, dtype=np.float32):
    """int16 [B,N] -> (frontend [B,C,rows], embedding [B,E], logits [B,1]) in `dtype`."""
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    fe = raw_frontend(pcm_to_float(pcm, dtype), sd, cfg)
    emb = backbone(np.ascontiguousarray(fe.transpose(0, 2, 1)), sd, cfg).astype(dtype)
    return fe, emb, classify(emb, sd, cfg, dtype)


def as_quartznet(cfg, sd):
    """The backbone as a model_type="quartznet" head: the same weights under the other prefix."""
    from nanowakeword_amd.config import HeadConfig
    q = HeadConfig("quartznet", cfg.input_shape, embedding_dim=cfg.embedding_dim, activation=cfg.activation, quartznet_config=cfg.e2e_quartznet_config)
    qsd = {k.replace("model.backbone.", "model."): v for k, v in sd.items() if not k.startswith("model.frontend.")}
    return q, qsd
