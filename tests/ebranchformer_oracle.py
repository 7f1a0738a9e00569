"""Numpy restatement of the E-Branchformer head (MergingModule / EBranchformerBlock / EBranchformerModel, architectures.py:546-616)
from oracle.heads primitives.  Eval mode: dropout is identity.  Per block on the residual stream x [B, T, D]:

    a = MHA(LN_attn(x))                      no residual here
    c = ConvolutionModule(x)                 the Conformer's module
    g = sigmoid(gate(c))                     the gate reads the CONV branch
    x = LN_final(x + a g + c (1 - g))
    x = x + FFN(x)                           full residual

then the mean over time (no LayerNorm in front of it) and output_proj.  Every primitive follows its input's dtype, so float64 inputs
give the float64 yardstick.  Test infrastructure only (the oracle package has no E-Branchformer of its own yet: net_e_branchformer has
the signature of the functions in oracle.heads._NETS)."""
import numpy as np

from oracle.heads import F32, _conv_module, _ffn, classify, layer_norm, linear, mha, sigmoid


def branchformer_block(x, sd, p, n_head):
    a = mha(layer_norm(x, sd[p + ".attn_branch_norm.weight"], sd[p + ".attn_branch_norm.bias"]), sd, p + ".attention", n_head)
    c = _conv_module(x, sd, p + ".conv_branch")
    g = sigmoid(linear(c, sd[p + ".merger.gate.weight"], sd[p + ".merger.gate.bias"]))
    x = layer_norm(x + (a * g + c * (1 - g)), sd[p + ".final_norm.weight"], sd[p + ".final_norm.bias"])
    return x + _ffn(x, sd, p + ".ffn")


def net_e_branchformer(x, sd, cfg):
    h = linear(x, sd["model.input_proj.weight"], sd["model.input_proj.bias"])
    for i in range(cfg.n_blocks):
        h = branchformer_block(h, sd, f"model.branchformer_blocks.{i}", cfg.branchformer_n_head)
    return linear(h.mean(axis=1), sd["model.output_proj.weight"], sd["model.output_proj.bias"])


def head_forward(x, sd, cfg, dtype=F32):
    """features [B, T, F] -> embedding [B, E] (oracle.head_forward's contract)."""
    x = np.ascontiguousarray(x, dtype=dtype)
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    return net_e_branchformer(x, sd, cfg).astype(dtype)


def model_forward(x, sd, cfg, dtype=F32):
    """Model.forward: the head, then Model.classifier -> logits [B, 1]."""
    return classify(head_forward(x, sd, cfg, dtype), sd, cfg, dtype)
