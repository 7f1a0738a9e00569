"""The plan-time-scaled conv trunks' stressed models and clips (tests/test_gpu_trunk_stress.py runs them on the HIP path), and a numpy
emulator of the two-term binary16 arithmetic under the planner's scales and range guard (nww_plan.hip: add_trunk, add_conv_mfma, fc1's
a_range in add_gemm).  trunk_x3 (both convolutions), fc1 behind it and conv3_x3 take their powers of two from a worst-case bound on the
whole tensor, so a model whose channel gains spread - one channel of a layer x 2^g, the next layer's weights on that channel / 2^g: the same
function, bit for bit in float32 - pushes every OTHER channel g bits down the scaled operand, towards binary16's subnormals.  The guard's
mean over the channels (f16_layer_typ) cannot see that: the loud channel lifts the mean by 2^g / Cout and hides the rest.  Since this file
the guard also holds the bound against the operand as its quietest consumer row sees it (the raw frontend's rule, f16_rows_seen), and
what it refuses stays on the three-term bf16 form.

Heads: cnn, crnn, e2e_dnn with ReLU only - GELU and SiLU are not positively homogeneous, so a channel rescale is not the same function under
them.  BcResNet has a file of its own, tests/test_bcresnet_stress.py: its shortcuts are 1x1 convolutions with a BatchNorm, so a per-channel
rescale of a block's output is undone in the next block's pointwise and shortcut columns, and its operands are scaled per pixel row.

The emulator's table at (37, 28) ((24, 16) tells the same; table() prints both) - max |logit - float64| / max(1, |logit|max) on 33 clips of
synth_features(seed 9), every operand the device splits under the plan's scales split as split_h2.h does (hi = RN16(v), lo = RN16(v - hi),
gradual underflow), the rest float64.  Case: head - link (l0: layer 0's channel 3 x 2^g and layer 1's weights on it / 2^g; l01: that and
channel 5 of layer 1) - 2^g.  Windows in log2: bound over f16_layer_typ's mean, and over the operand as its quietest consumer row sees it,
each for trunk_x3's conv2 operand / the operand of what reads the trunk (consumer: fc1 for cnn, the third conv for crnn and e2e_dnn).
"mean guard" = before the per-row rule (bound <= 2^16 x mean), "per-row guard" = since (that, bound <= 2^20 x the quietest row's view, and
every row's RMS weight within 2^17 of the tensor's largest weight).  Forms as trunk/consumer: 2 = two binary16 terms, 3 = the fall-back to
three bf16 terms (emulated as exact).  The float32 oracle's own error is 4.8e-7 (cnn), 1.3e-6 (crnn), 1.8e-6 (e2e_dnn) on every row:

case               windows, log2: mean trunk/consumer, rows trunk/consumer | mean guard: forms, error | per-row guard: forms, error
cnn                9.9 / 13.4   10.0 / 13.4 | 2/2 1.4e-07 | 2/2 1.4e-07
crnn              10.4 / 14.2   10.3 / 14.1 | 2/2 3.4e-07 | 2/2 3.4e-07
e2e_dnn           10.4 / 14.8   10.4 / 14.7 | 2/2 2.4e-07 | 2/2 2.4e-07
cnn-l0-2^8        13.2 / 16.6   17.0 / 20.4 | 2/3 1.1e-07 | 2/3 1.1e-07
cnn-l0-2^-8       10.0 / 11.8   16.3 / 17.8 | 2/2 2.3e-07 | 2/2 2.3e-07
cnn-l1-2^8         9.9 / 18.1   10.0 / 21.2 | 2/3 9.4e-08 | 2/3 9.4e-08
cnn-l1-2^-8        9.9 / 13.5   10.0 / 19.1 | 2/2 3.6e-07 | 2/2 3.6e-07
cnn-l01-2^8       13.2 / 21.4   17.0 / 28.4 | 2/3 1.1e-07 | 2/3 1.1e-07
cnn-l0-2^12       13.3 / 16.7   21.0 / 24.4 | 2/3 1.4e-06 | 3/3 0.0e+00
cnn-l0-2^-12      10.0 / 11.8   20.3 / 21.7 | 2/2 1.9e-06 | 3/3 0.0e+00
cnn-l1-2^12        9.9 / 18.3   10.0 / 25.2 | 2/3 9.4e-08 | 2/3 9.4e-08
cnn-l1-2^-12       9.9 / 13.5   10.0 / 23.1 | 2/2 4.9e-06 | 2/3 9.4e-08
cnn-l01-2^12      13.3 / 21.6   21.0 / 36.4 | 2/3 1.4e-06 | 3/3 0.0e+00
cnn-l0-2^16       13.3 / 16.7   25.0 / 28.4 | 2/3 1.6e-05 | 3/3 0.0e+00
cnn-l0-2^-16      10.0 / 11.8   24.3 / 25.7 | 2/2 3.2e-05 | 3/3 0.0e+00
cnn-l1-2^16        9.9 / 18.3   10.0 / 29.2 | 2/3 9.5e-08 | 2/3 9.5e-08
cnn-l1-2^-16       9.9 / 13.5   10.0 / 27.1 | 2/2 1.1e-04 | 2/3 9.2e-08
cnn-l01-2^16      13.3 / 21.7   25.0 / 44.4 | 2/3 2.5e-05 | 3/3 0.0e+00
cnn-l0-2^20       13.3 / 16.7   29.0 / 32.4 | 2/3 1.9e-04 | 3/3 0.0e+00
cnn-l0-2^-20      10.0 / 11.8   28.3 / 29.7 | 2/2 3.7e-04 | 3/3 0.0e+00
cnn-l1-2^20        9.9 / 18.3   10.0 / 33.2 | 2/3 6.7e-07 | 3/3 0.0e+00
cnn-l1-2^-20       9.9 / 13.5   10.0 / 31.1 | 2/2 1.8e-03 | 3/3 0.0e+00
cnn-l01-2^20      13.3 / 21.7   29.0 / 52.4 | 2/3 5.6e-03 | 3/3 0.0e+00
crnn-l0-2^8       12.9 / 16.8   16.7 / 20.5 | 2/3 3.0e-07 | 2/3 3.0e-07
crnn-l0-2^-8      10.4 / 12.7   16.6 / 18.5 | 2/2 3.7e-07 | 2/2 3.7e-07
crnn-l1-2^8       10.4 / 18.6   10.3 / 21.4 | 2/3 2.9e-07 | 2/3 2.9e-07
crnn-l1-2^-8      10.4 / 14.3   10.3 / 20.1 | 2/2 7.0e-07 | 2/3 2.9e-07
crnn-l2-2^8       10.4 / 14.2   10.3 / 14.1 | 2/2 3.4e-07 | 2/2 3.4e-07
crnn-l2-2^-8      10.4 / 14.2   10.3 / 14.1 | 2/2 3.4e-07 | 2/2 3.4e-07
crnn-l01-2^8      12.9 / 20.9   16.7 / 26.9 | 2/3 3.0e-07 | 2/3 3.0e-07
crnn-l0-2^12      13.0 / 16.9   20.7 / 24.5 | 2/3 1.0e-06 | 3/3 8.8e-08
crnn-l0-2^-12     10.4 / 12.7   20.6 / 22.5 | 2/2 3.1e-06 | 3/3 8.8e-08
crnn-l1-2^12      10.4 / 18.7   10.3 / 25.4 | 2/3 2.9e-07 | 2/3 2.9e-07
crnn-l1-2^-12     10.4 / 14.3   10.3 / 24.1 | 2/2 1.5e-05 | 2/3 2.9e-07
crnn-l2-2^12      10.4 / 14.2   10.3 / 14.1 | 2/2 3.4e-07 | 2/2 3.4e-07
crnn-l2-2^-12     10.4 / 14.2   10.3 / 14.1 | 2/2 3.4e-07 | 2/2 3.4e-07
crnn-l01-2^12     13.0 / 21.3   20.7 / 34.9 | 2/3 1.0e-06 | 3/3 8.8e-08
crnn-l0-2^16      13.0 / 16.9   24.7 / 28.5 | 2/3 1.6e-05 | 3/3 8.8e-08
crnn-l0-2^-16     10.4 / 12.7   24.6 / 26.5 | 2/2 7.4e-05 | 3/3 8.8e-08
crnn-l1-2^16      10.4 / 18.8   10.3 / 29.4 | 2/3 2.9e-07 | 2/3 2.9e-07
crnn-l1-2^-16     10.4 / 14.3   10.3 / 28.1 | 2/2 2.1e-04 | 2/3 2.9e-07
crnn-l2-2^16      10.4 / 14.2   10.3 / 14.1 | 2/2 3.4e-07 | 2/2 3.4e-07
crnn-l2-2^-16     10.4 / 14.2   10.3 / 14.1 | 2/2 3.4e-07 | 2/2 3.4e-07
crnn-l01-2^16     13.0 / 21.4   24.7 / 42.9 | 2/3 1.6e-05 | 3/3 8.8e-08
crnn-l0-2^20      13.0 / 16.9   28.7 / 32.5 | 2/3 2.9e-04 | 3/3 8.8e-08
crnn-l0-2^-20     10.4 / 12.7   28.6 / 30.5 | 2/2 9.7e-04 | 3/3 8.8e-08
crnn-l1-2^20      10.4 / 18.8   10.3 / 33.4 | 2/3 2.9e-07 | 2/3 2.9e-07
crnn-l1-2^-20     10.4 / 14.3   10.3 / 32.1 | 2/2 5.4e-03 | 2/3 2.9e-07
crnn-l2-2^20      10.4 / 14.2   10.3 / 14.1 | 2/2 3.4e-07 | 2/2 3.4e-07
crnn-l2-2^-20     10.4 / 14.2   10.3 / 14.1 | 2/2 3.4e-07 | 2/2 3.4e-07
crnn-l01-2^20     13.0 / 21.4   28.7 / 50.9 | 2/3 2.9e-04 | 3/3 8.8e-08
e2e_dnn-l0-2^8    13.3 / 17.6   17.1 / 21.4 | 2/3 2.8e-07 | 2/3 2.8e-07
e2e_dnn-l0-2^-8   10.4 / 13.1   16.7 / 19.0 | 2/2 4.9e-07 | 2/2 4.9e-07
e2e_dnn-l1-2^8    10.4 / 18.7   10.4 / 22.6 | 2/3 2.5e-07 | 2/3 2.5e-07
e2e_dnn-l1-2^-8   10.4 / 14.9   10.4 / 20.5 | 2/2 6.0e-07 | 2/3 2.5e-07
e2e_dnn-l01-2^8   13.3 / 21.3   17.1 / 27.8 | 2/3 2.8e-07 | 2/3 2.8e-07
e2e_dnn-l0-2^12   13.4 / 17.7   21.1 / 25.4 | 2/3 8.6e-07 | 3/3 3.0e-07
e2e_dnn-l0-2^-12  10.4 / 13.0   20.7 / 22.9 | 2/2 9.0e-06 | 3/3 3.0e-07
e2e_dnn-l1-2^12   10.4 / 18.8   10.4 / 26.6 | 2/3 2.5e-07 | 2/3 2.5e-07
e2e_dnn-l1-2^-12  10.4 / 14.9   10.4 / 24.5 | 2/2 5.5e-06 | 2/3 2.5e-07
e2e_dnn-l01-2^12  13.4 / 21.7   21.1 / 35.8 | 2/3 8.6e-07 | 3/3 3.0e-07
e2e_dnn-l0-2^16   13.4 / 17.7   25.1 / 29.4 | 2/3 1.4e-05 | 3/3 3.0e-07
e2e_dnn-l0-2^-16  10.4 / 13.0   24.7 / 26.9 | 2/2 1.0e-04 | 3/3 3.0e-07
e2e_dnn-l1-2^16   10.4 / 18.8   10.4 / 30.6 | 2/3 2.5e-07 | 2/3 2.5e-07
e2e_dnn-l1-2^-16  10.4 / 14.9   10.4 / 28.5 | 2/2 1.1e-04 | 2/3 2.5e-07
e2e_dnn-l01-2^16  13.4 / 21.7   25.1 / 43.8 | 2/3 1.4e-05 | 3/3 3.0e-07
e2e_dnn-l0-2^20   13.4 / 17.7   29.1 / 33.4 | 2/3 1.9e-04 | 3/3 3.0e-07
e2e_dnn-l0-2^-20  10.4 / 13.0   28.7 / 30.9 | 2/2 2.1e-03 | 3/3 3.0e-07
e2e_dnn-l1-2^20   10.4 / 18.8   10.4 / 34.6 | 2/3 2.5e-07 | 2/3 2.5e-07
e2e_dnn-l1-2^-20  10.4 / 14.9   10.4 / 32.5 | 2/2 2.3e-03 | 2/3 2.5e-07
e2e_dnn-l01-2^20  13.4 / 21.7   29.1 / 51.8 | 2/3 1.9e-04 | 3/3 3.0e-07

Under the mean's guard the emulator leaves 2 x float32 + 2e-6 from 2^12 on and the 1e-4 bar at 2^16 .. 2^20, worst where a QUIET channel
(x 2^-g) feeds fc1 / the third conv on two terms: 1.8e-3 .. 5.4e-3 at 2^-20.  The per-row guard moves every such layer, and everything it leaves
on two terms is inside the bars (test_guard_leaves_only_sound_cases).  What reads the trunk already falls back at 2^8 under the mean's guard
(conv2's worst-case bound rises with the loud channel, the mean hardly): see test_gpu_trunk_stress.py.  Since the guard alone would tax a model at 2^8 already, the library also BALANCES the channel gains of a ReLU model before it plans
(balance() restates balance_channel_gains: the rescale above by the planner's own hand, undoing a channel that lies 2^4 or more off its layer's
median), so every case in the table ends on two terms at the plain weights' windows and error (test_balanced_models_keep_the_two_term_kernels);
the guard's columns above are what a head that cannot be balanced (GELU, SiLU) gets.  numpy only: nothing here loads the native library."""
import functools
import math

import numpy as np
import pytest

from nanowakeword_amd.config import HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from oracle import heads as oh
import oracle

HEADS = ("cnn", "crnn", "e2e_dnn")
SHAPES = ((24, 16), (37, 28))          # test_gpu_trunk_stress.py asserts that the plain plan at these shows every kernel named above
BATCH = 33                              # the GPU file also runs the first 8: a whole tile and a ragged last one
GS = (8, 12, 16, 20)
CH_A, CH_B = 3, 5                       # the rescaled channel of a link, and of the link behind it in the two-layer cases
FEATURE_BOUND, FEATURE_TYP = 8192.0, 32.0          # NWW_F16_FEATURE_BOUND, F16_FEATURES.typ
MEAN_LOG2 = 16                          # f16_range_factor(): nww_knobs().f16_range_log2
ROWS_LOG2 = MEAN_LOG2 + 4               # f16_rows_ok: 2^4 x f16_range_factor(), the raw frontend's window
BAR = 1e-4                              # test_heavy_tailed_weights_against_float64's contract, relative to max(1, |ref|max)


def bars_ok(err, f32):
    return err <= 2.0 * f32 + 2e-6 and err <= BAR


# ---- the heads' layers: (conv prefix, BatchNorm prefix or None) per stage, and the Linear weights that read the last stage's channels in
# contiguous blocks of K / C columns (fc1 of the flattened [C, H/4, W/4]; the recurrent input projections of the [C * H] sequence rows)
LAYERS = {"cnn": [("model.conv1", None), ("model.conv2", None)],
          "crnn": [(f"model.cnn.{4 * i}", f"model.cnn.{4 * i + 1}") for i in range(3)],
          "e2e_dnn": [(f"model.conv_block.{4 * i}", f"model.conv_block.{4 * i + 1}") for i in range(3)]}
CONSUMERS = {"cnn": ("model.fc1.weight",), "crnn": ("model.rnn.weight_ih_l0", "model.rnn.weight_ih_l0_reverse"), "e2e_dnn": ()}
LINKS = {"cnn": (0, 1), "crnn": (0, 1, 2), "e2e_dnn": (0, 1)}       # link k: layer k's channel x 2^g, layer k + 1's weights on it / 2^g


def config(head, shape):
    return HeadConfig(head, shape)


def rescale(sd, head, link, channel, g):
    """channel of layer `link` x 2^g - its BatchNorm's weight and bias where it has one (the running statistics and the convolution stay),
    else the convolution's weights and bias - and the next layer's weights on that channel / 2^g.  ReLU and max-pool are positively
    homogeneous and 2^g a power of two: the same function, and the same bits in float32 and in float64"""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    G = np.float32(2.0 ** g)
    conv, bn = LAYERS[head][link]
    for key in ((bn + ".weight", bn + ".bias") if bn else (conv + ".weight", conv + ".bias")):
        out[key][channel] *= G
    if link + 1 < len(LAYERS[head]):
        out[LAYERS[head][link + 1][0] + ".weight"][:, channel] /= G
    else:
        assert CONSUMERS[head], "nothing behind the last layer takes 1 / G"
        C = out[conv + ".weight"].shape[0]
        for key in CONSUMERS[head]:
            per = out[key].shape[1] // C
            out[key][:, channel * per:(channel + 1) * per] /= G
    return out


# name -> (head, ((link, channel, g), ...)): one channel per link, two channels in two successive layers, the quiet-channel mirror
RESCALE = {}
for _h in HEADS:
    for _g in GS:
        for _l in LINKS[_h]:
            RESCALE[f"{_h}-l{_l}-2^{_g}"] = (_h, ((_l, CH_A, _g),))
            RESCALE[f"{_h}-l{_l}-2^-{_g}"] = (_h, ((_l, CH_A, -_g),))
        RESCALE[f"{_h}-l01-2^{_g}"] = (_h, ((0, CH_A, _g), (1, CH_B, _g)))
# whole clips of plain-weight features x 2^e (they stay inside the +-8192 the two-term kernels clamp to), and one such clip among ordinary ones
DATA = {"x2^-10": -10, "x2^-5": -5, "x2^5": 5}
MIXED_CLIP, MIXED_EXP = 5, -10
KEEPS_TWO_TERM = [n for n, (_, steps) in RESCALE.items() if all(g == 8 for _, _, g in steps)]      # the guard must not tax these


# heads that balance_channel_gains cannot touch (GELU, SiLU), where the range guard alone decides; the same weight edits, no longer the same
# function but a model like any other, judged against float64 on those weights.  name -> (head, activation, steps, the forms
# (trunk, consumer) under the mean's guard, the forms under the per-row guard).  The l1-2^-g rows are the ones where ONLY the rule in
# add_gemm (fc1) / add_conv_mfma (conv3_x3) moves anything: the trunk stays on two terms and what reads it falls back
UNBALANCED = {"cnn-gelu-l0-2^8": ("cnn", "gelu", ((0, CH_A, 8),), (True, False), (True, False)),
              "cnn-gelu-l0-2^20": ("cnn", "gelu", ((0, CH_A, 20),), (True, False), (False, False)),
              "cnn-gelu-l0-2^-20": ("cnn", "gelu", ((0, CH_A, -20),), (True, True), (False, False)),
              "cnn-gelu-l1-2^-20": ("cnn", "gelu", ((1, CH_A, -20),), (True, True), (False, False)),
              "cnn-gelu-l01-2^20": ("cnn", "gelu", ((0, CH_A, 20), (1, CH_B, 20)), (True, False), (False, False))}
UNBALANCED.update({f"cnn-gelu-l1-2^-{g}": ("cnn", "gelu", ((1, CH_A, -g),), (True, True), (True, False)) for g in (12, 16)})
UNBALANCED.update({f"crnn-gelu-l1-2^-{g}": ("crnn", "gelu", ((1, CH_A, -g),), (True, True), (True, False)) for g in GS})
UNBALANCED.update({f"e2e_dnn-silu-l1-2^-{g}": ("e2e_dnn", "silu", ((1, CH_A, -g),), (True, True), (True, False)) for g in GS})
# a ReLU model most of whose channels are nearly dead (9 of conv1's 16 BatchNorm channels x 2^-24, nothing behind them compensating): the
# dead channels are worth nothing to conv2 and must neither move nor set the median
DEAD_CHANNELS, DEAD_LOG2 = tuple(range(0, 16, 2)) + (1,), -24


def unbalanced_case(name, shape):
    """-> (cfg, state dict) of an UNBALANCED case"""
    head, activation, steps, _, _ = UNBALANCED[name]
    cfg = HeadConfig(head, shape, activation=activation)
    sd = synth_state_dict(cfg)
    for link, channel, g in steps:
        sd = rescale(sd, head, link, channel, g)
    return cfg, sd


def dead_channel_case(shape):
    """-> (cfg, state dict): the crnn head with DEAD_CHANNELS of its first BatchNorm x 2^DEAD_LOG2"""
    cfg = config("crnn", shape)
    sd = {k: np.array(v, copy=True) for k, v in synth_state_dict(cfg).items()}
    for c in DEAD_CHANNELS:
        sd["model.cnn.1.weight"][c] *= np.float32(2.0 ** DEAD_LOG2)
        sd["model.cnn.1.bias"][c] *= np.float32(2.0 ** DEAD_LOG2)
    return cfg, sd


@functools.lru_cache(maxsize=None)
def base_case(head, shape):
    """-> (cfg, synth_state_dict, features [BATCH, *shape], float64 logits, float32 oracle logits): evaluated once, read-only"""
    cfg = config(head, shape)
    sd = synth_state_dict(cfg)
    feats = synth_features(BATCH, shape, seed=9)
    l64 = oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel()
    l32 = oracle.model_forward(feats, sd, cfg).ravel()
    for a in (feats, l64, l32, *sd.values()):
        a.setflags(write=False)
    return cfg, sd, feats, l64, l32


@functools.lru_cache(maxsize=None)
def rescaled_sd(name, shape):
    head, steps = RESCALE[name]
    sd = base_case(head, shape)[1]
    for link, channel, g in steps:
        sd = rescale(sd, head, link, channel, g)
    for a in sd.values():
        a.setflags(write=False)
    return sd


def data_feats(name, shape):
    feats = synth_features(BATCH, shape, seed=9) * np.float32(2.0 ** DATA[name])
    assert np.abs(feats).max() < FEATURE_BOUND
    return feats


def mixed_feats(shape):
    feats = synth_features(BATCH, shape, seed=9)
    feats[MIXED_CLIP] *= np.float32(2.0 ** MIXED_EXP)
    return feats


# ---- the planner's arithmetic (nww_plan.hip), in float64 as there
def f16_pow2_floor(x):
    return math.ldexp(1.0, math.frexp(x)[1] - 1)


def f16_scale(bound):
    if not bound > 1e-30:
        bound = 1e-30
    if not bound < 1e30:
        return 0.0
    return min(f16_pow2_floor(65504.0 / (bound * 1.02)), 2.0 ** 40)


def f16_wscale(w):
    return f16_scale(float(np.abs(np.asarray(w, np.float64)).max()) * 2.0)


def stage_params(sd, head):
    """per conv stage: w [Cout, Cin * 9], b, and the folded BatchNorm (fold_batchnorms: float32, al = w / sqrt(var + eps), be = b - mean al)"""
    out = []
    for conv, bn in LAYERS[head]:
        w = np.asarray(sd[conv + ".weight"], np.float32)
        st = dict(w=w.reshape(w.shape[0], -1), w4=w, b=np.asarray(sd[conv + ".bias"], np.float32), al=None, be=None)
        if bn:
            inv = np.float32(1.0) / np.sqrt(np.asarray(sd[bn + ".running_var"], np.float32) + np.float32(1e-5))
            st["al"] = (np.asarray(sd[bn + ".weight"], np.float32) * inv).astype(np.float32)
            st["be"] = (np.asarray(sd[bn + ".bias"], np.float32) - np.asarray(sd[bn + ".running_mean"], np.float32) * st["al"]).astype(np.float32)
        out.append(st)
    return out


def f16_layer_bound(st, in_bound):
    t = np.abs(st["w"].astype(np.float64)).sum(1) * in_bound + np.abs(st["b"].astype(np.float64))
    if st["al"] is not None:
        t = t * np.abs(st["al"].astype(np.float64)) + np.abs(st["be"].astype(np.float64))
    return float(t.max())


def f16_layer_typ(st, typ_in):
    q = np.sqrt((st["w"].astype(np.float64) ** 2).sum(1))
    if st["al"] is not None:
        q = q * np.abs(st["al"].astype(np.float64))
    return float(q.mean()) * typ_in


def f16_rows(w, typ_in):
    """f16_rows_moments: per consumer row co, sig2 = sum_k w^2 typ_in[channel of k]^2 and norm2 = sum_k w^2; w [Cout, K], the channel of
    column k is k // (K / len(typ_in))"""
    w2 = np.asarray(w, np.float64) ** 2
    t2 = np.repeat(np.asarray(typ_in, np.float64) ** 2, w2.shape[1] // len(typ_in))
    return (w2 * t2).sum(1), w2.sum(1)


def f16_rows_seen(sig2, norm2):
    """the operand as its quietest consumer row sees it: min over the rows with any weight of sqrt(sig2 / norm2); inf if there is none"""
    live = norm2 > 0
    return float(np.sqrt(sig2[live] / norm2[live]).min()) if live.any() else math.inf


def f16_rows_weights_ok(w):
    """one power of two per tensor puts the largest weight in [2^14, 2^15) and a weight's lo term keeps its 11 bits down to 2^-3: every
    row's RMS weight within 2^17 of the largest weight"""
    w = np.asarray(w, np.float64)
    norm2 = (w ** 2).sum(1)
    live = norm2 > 0
    return bool((np.abs(w).max() <= np.sqrt(norm2[live] / w.shape[1]) * 2.0 ** 17).all())


def f16_rows_typ(sig2, st):
    """per output channel: sqrt(sig2 + b^2), through the folded BatchNorm sqrt(sig2 al^2 + (b al + be)^2)"""
    b = st["b"].astype(np.float64)
    if st["al"] is None:
        return np.sqrt(sig2 + b * b)
    al, be = st["al"].astype(np.float64), st["be"].astype(np.float64)
    return np.sqrt(sig2 * al * al + (b * al + be) ** 2)


BALANCE_MIN_LOG2, BALANCE_MAX_LOG2 = 4.0, 40.0


def balance(sd, cfg):
    """balance_channel_gains (nww_plan.hip), which runs on the loaded weights before anything else under the two-term arithmetic and ReLU:
    per layer in front of a plan-time-scaled operand (conv1, conv2), a channel whose worst-case bound lies 2^4 .. 2^40 off the layer's median
    channel (the upper median over the channels that count: worth, below) is multiplied by the power of two that brings it next to the median - its BatchNorm's weight and bias where
    there is one, else its convolution row and bias - and the next layer's weights on it divided by the same: rescale() by the planner's own
    hand, the same function and the same float32 bits.  -> a new state dict (the input's arrays where nothing moved)"""
    head = cfg.model_type
    assert cfg.activation == "relu"
    out = dict(sd)
    in_bound = FEATURE_BOUND
    for link in (0, 1):
        conv, bn = LAYERS[head][link]
        nxt = LAYERS[head][link + 1][0] + ".weight" if link + 1 < len(LAYERS[head]) else "model.fc1.weight"
        w = np.asarray(out[conv + ".weight"], np.float64)
        t = np.abs(w.reshape(w.shape[0], -1)).sum(1) * in_bound + np.abs(np.asarray(out[conv + ".bias"], np.float64))
        if bn:
            al = np.asarray(out[bn + ".weight"], np.float64) / np.sqrt(np.asarray(out[bn + ".running_var"], np.float64) + 1e-5)
            t = t * np.abs(al) + np.abs(np.asarray(out[bn + ".bias"], np.float64) - np.asarray(out[bn + ".running_mean"], np.float64) * al)
        # a channel's worth to the next layer: its bound x the 2-norm of the weights that read it; under 2^-8 of the best it neither moves nor counts
        wn = np.asarray(out[nxt], np.float64).reshape(out[nxt].shape[0], -1)
        worth = t * np.sqrt((wn.reshape(wn.shape[0], len(t), -1) ** 2).sum(axis=(0, 2)))
        counts = (worth > 0) & (worth >= worth.max() * 2.0 ** -8)
        med = np.sort(t[counts])[counts.sum() // 2] if counts.any() else 0.0
        exps = np.zeros(len(t), int)
        for c in range(len(t)):
            if med > 0 and counts[c]:
                l = math.log2(t[c] / med)
                if BALANCE_MIN_LOG2 <= abs(l) <= BALANCE_MAX_LOG2:
                    exps[c] = -int(math.copysign(math.floor(abs(l) + 0.5), l))
        if exps.any():
            keys = (bn + ".weight", bn + ".bias") if bn else (conv + ".weight", conv + ".bias")
            for k in keys + (nxt,):
                out[k] = np.array(out[k], np.float32, copy=True)
            per = out[nxt].reshape(out[nxt].shape[0], -1).shape[1] // len(t)
            flat = out[nxt].reshape(out[nxt].shape[0], -1)                  # a view: channel c is columns c per .. c per + per - 1
            for c in np.nonzero(exps)[0]:
                for k in keys:
                    out[k][c] *= np.float32(2.0 ** exps[c])
                flat[:, c * per:(c + 1) * per] *= np.float32(2.0 ** -exps[c])
        in_bound = float((t * 2.0 ** exps).max())
    return out


def plan(sd, cfg, guard="rows"):
    """-> dict(trunk, consumer: the two-term verdicts of trunk_x3 and of what reads it (fc1 / the third conv), the scales, and the windows in
    log2: mean1 / mean2 = bound over f16_layer_typ's mean, rows1 / rows2 = bound over the quietest consumer row's view).
    guard = "mean": before the per-row rule, "rows": with it"""
    head = cfg.model_type
    st = stage_params(sd, head)
    bound1 = f16_layer_bound(st[0], FEATURE_BOUND)
    bound2 = f16_layer_bound(st[1], bound1)
    typ1 = f16_layer_typ(st[0], FEATURE_TYP)
    typ2 = f16_layer_typ(st[1], typ1)
    sig1, _ = f16_rows(st[0]["w"], [FEATURE_TYP])
    ch1 = f16_rows_typ(sig1, st[0])
    sig2, norm2 = f16_rows(st[1]["w"], ch1)
    ch2 = f16_rows_typ(sig2, st[1])
    seen1 = f16_rows_seen(sig2, norm2)
    cw = np.asarray(sd["model.fc1.weight"], np.float32) if head == "cnn" else st[2]["w"]
    seen2 = f16_rows_seen(*f16_rows(cw, ch2))
    p = dict(bound1=bound1, bound2=bound2, mean1=math.log2(bound1 / typ1), mean2=math.log2(bound2 / typ2),
             rows1=math.log2(bound1 / seen1) if seen1 > 0 else math.inf, rows2=math.log2(bound2 / seen2) if seen2 > 0 else math.inf)
    rows = guard == "rows"
    p["trunk"] = p["mean1"] <= MEAN_LOG2 and (not rows or (p["rows1"] <= ROWS_LOG2 and f16_rows_weights_ok(st[0]["w"]) and f16_rows_weights_ok(st[1]["w"])))
    # a trunk on three terms reports no range: what reads it stays on three terms too
    p["consumer"] = p["trunk"] and p["mean2"] <= MEAN_LOG2 and (not rows or (p["rows2"] <= ROWS_LOG2 and f16_rows_weights_ok(cw)))
    p.update(f_in=f16_scale(FEATURE_BOUND), f_s1=f16_scale(bound1), f_w1=f16_wscale(st[0]["w"]), f_w2=f16_wscale(st[1]["w"]),
             f_s2=f16_scale(bound2), f_wc=f16_wscale(cw))
    return p


# ---- the two-term arithmetic (split_h2.h)
def _split(v):
    """nww_split2h: hi = RN16(v) (v_cvt_pk_f16_f32: round to nearest even, gradual underflow, inf past 65520), lo = RN16(v - hi) with the
    remainder exact in float32 (v_fma_mix_f32 reads the binary16 half in place)"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _contract2(x, w, xs, ws, op):
    """op(x, w) with both operands as two binary16 terms of value x scale: the three products the kernels keep (hi hi, lo hi, hi lo; binary16
    products are exact in the float32 accumulator, whose own rounding the float64 sum here leaves out)"""
    xh, xl = _split(np.asarray(x, np.float64).astype(np.float32) * np.float32(xs))
    wh, wl = _split(np.asarray(w, np.float32) * np.float32(ws))
    return (op(xh, wh) + op(xl, wh) + op(xh, wl)) / (float(xs) * float(ws))


def _conv(x, w):
    return oh.conv2d(x, w)


def forward(feats, sd, cfg, p=None):
    """the head in float64; with a plan p, the operands of the layers it leaves on the two-term form go through _contract2 under its scales:
    conv1's input (clamped to the feature bound) and conv2's operand in trunk_x3, fc1's / the third conv's operand, and their weights"""
    head = cfg.model_type
    st = stage_params(sd, head)
    sd64 = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    h = np.asarray(feats, np.float64)[:, None]
    two = [bool(p and p["trunk"]), bool(p and p["trunk"]), bool(p and p["consumer"])]
    scales = [(p["f_in"], p["f_w1"]), (p["f_s1"], p["f_w2"]), (p["f_s2"], p["f_wc"])] if p else [None] * 3
    for i, s in enumerate(st):
        if two[i]:
            if i == 0:
                h = np.clip(h, -FEATURE_BOUND, FEATURE_BOUND)
            y = _contract2(h, s["w4"], *scales[i], _conv)
        else:
            y = _conv(h, s["w4"].astype(np.float64))
        y = y + s["b"].astype(np.float64).reshape(1, -1, 1, 1)
        if s["al"] is not None:
            y = y * s["al"].astype(np.float64).reshape(1, -1, 1, 1) + s["be"].astype(np.float64).reshape(1, -1, 1, 1)
        y = np.maximum(y, 0.0)
        h = oh.avgpool_export(y, (1, 4)) if (head == "e2e_dnn" and i == 2) else oh.maxpool2(y)
    if head == "cnn":
        a = h.reshape(h.shape[0], -1)
        y = _contract2(a, sd["model.fc1.weight"], *scales[2], lambda x, w: x @ w.T) if two[2] else a @ sd64["model.fc1.weight"].T
        e = oh.linear(np.maximum(y + sd64["model.fc1.bias"], 0.0), sd64["model.fc2.weight"], sd64["model.fc2.bias"])
    elif head == "crnn":
        B, C, H, W = h.shape
        seq = np.ascontiguousarray(h.reshape(B, C * H, W).transpose(0, 2, 1))
        e = oh.linear(oh.bigru_last(seq, sd64, "model.rnn", cfg.n_blocks, cfg.layer_dim, lstm=cfg.crnn_rnn_type == "lstm"),
                      sd64["model.fc.weight"], sd64["model.fc.bias"])
    else:
        a = h.reshape(h.shape[0], -1)
        e = oh.linear(np.maximum(oh.batch_norm(oh.linear(a, sd64["model.fc1.weight"], sd64["model.fc1.bias"]), sd64, "model.bn1"), 0.0),
                      sd64["model.out.weight"], sd64["model.out.bias"])
    return oracle.classify(e, sd, cfg, dtype=np.float64).ravel()


def rel_err(x, ref):
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(x, np.float64) - ref)
    return float(np.nan_to_num(d, nan=np.inf).max()) / max(1.0, float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def emulated(name, shape, guard):
    """-> (plan, the emulator's error under it, the float32 oracle's error) of a RESCALE case, or of the plain weights when name is a head"""
    head = name if name in HEADS else RESCALE[name][0]
    cfg, sd0, feats, l64, l32 = base_case(head, shape)
    sd = sd0 if name in HEADS else rescaled_sd(name, shape)
    p = plan(sd, cfg, guard)
    return p, rel_err(forward(feats, sd, cfg, p), l64), rel_err(l32, l64)


def _row(name, shape):
    (po, eo, f32), (pn, en, _) = emulated(name, shape, "mean"), emulated(name, shape, "rows")
    form = lambda p: f"{2 if p['trunk'] else 3}/{2 if p['consumer'] else 3}"
    return (f"{name:18s} {shape[0]:3d}x{shape[1]:<3d} mean 2^{po['mean1']:4.1f} / 2^{po['mean2']:4.1f}  rows 2^{po['rows1']:4.1f} / 2^{po['rows2']:4.1f}  "
            f"mean {form(po)} {eo:.1e}  rows {form(pn)} {en:.1e}  f32 {f32:.1e}")


def table(shapes=SHAPES):
    """the docstring's table (python -c "import test_trunk_stress as t; print(t.table())" from tests/)"""
    return "\n".join(_row(n, s) for s in shapes for n in list(HEADS) + list(RESCALE))


# ---- the tests
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("head", HEADS)
def test_forward_restates_the_oracle(head, shape):
    """forward() without a plan is the float64 oracle: to 1e-12 on the cnn head, and to the rounding of the float32 BatchNorm fold the device
    does (fold_batchnorms; one float32 rounding of alpha and of beta per channel and stage, 6e-8 each) on the heads that have one"""
    cfg, sd, feats, l64, _ = base_case(head, shape)
    d = float(np.abs(forward(feats, sd, cfg) - l64).max()) / max(1.0, float(np.abs(l64).max()))
    print(f"{head} {shape}: forward() without a plan vs the float64 oracle {d:.2e}")
    assert d <= (1e-12 if head == "cnn" else 5e-7), (head, shape, d)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(RESCALE))
def test_rescale_preserves_the_function(name, shape):
    """float32 oracle: the same bits as on the plain weights, in every case - the oracle applies a BatchNorm as x alpha + beta with alpha and
    beta from float32 parameters x 2^g, which is exact, so no case needs an ulp of allowance; float64: 1e-12 relative.  And the case is
    well-conditioned: the float32 oracle is within a tenth of the 1e-4 bar of float64"""
    head = RESCALE[name][0]
    cfg, _, feats, l64, l32 = base_case(head, shape)
    sd = rescaled_sd(name, shape)
    assert np.array_equal(oracle.model_forward(feats, sd, cfg).ravel(), l32), name
    assert np.abs(oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel() - l64).max() <= 1e-12 * max(1.0, np.abs(l64).max()), name
    assert np.ptp(l64) > 1e-2 and rel_err(l32, l64) <= BAR / 10, (name, float(np.ptp(l64)), rel_err(l32, l64))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("head", HEADS)
def test_plain_weights_and_data_cases(head, shape):
    """plain weights: both guards keep every layer on two terms, and the emulator is inside the bars on the plain clips, on whole batches
    x 2^-10 / 2^-5 / 2^5 and on one quiet clip among ordinary ones (no scale depends on the data: the quiet clip's logit is the one it has alone)"""
    cfg, sd, feats, l64, l32 = base_case(head, shape)
    p = plan(sd, cfg)
    assert p["trunk"] and p["consumer"] and plan(sd, cfg, "mean")["trunk"] and plan(sd, cfg, "mean")["consumer"], p
    for what, x in [("plain", feats)] + [(n, data_feats(n, shape)) for n in DATA] + [("mixed", mixed_feats(shape))]:
        ref = oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
        f32 = rel_err(oracle.model_forward(x, sd, cfg).ravel(), ref)
        got = forward(x, sd, cfg, p)
        err = rel_err(got, ref)
        print(f"{head} {shape} {what}: emulated {err:.2e}, float32 oracle {f32:.2e}, |logit|max {np.abs(ref).max():.3g}")
        assert f32 <= BAR / 10 and bars_ok(err, f32), (head, shape, what, err, f32)
        if what == "mixed":
            alone = forward(x[MIXED_CLIP:MIXED_CLIP + 1], sd, cfg, p)
            assert abs(alone[0] - got[MIXED_CLIP]) <= 1e-12 * max(1.0, abs(alone[0]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(RESCALE))
def test_guard_leaves_only_sound_cases(name, shape):
    """every layer the per-row guard leaves on the two-term form is emulated inside the bars; 2^8 on one or two layers stays on two terms
    in trunk_x3; and the per-row guard only ever adds fall-backs to the mean's"""
    po, eo, f32 = emulated(name, shape, "mean")
    pn, en, _ = emulated(name, shape, "rows")
    print(_row(name, shape))
    assert bars_ok(en, f32), (name, shape, en, f32)
    assert (po["trunk"] or not pn["trunk"]) and (po["consumer"] or not pn["consumer"]), name
    if name in KEEPS_TWO_TERM:
        # under the guard alone trunk_x3 keeps its two-term form at 2^8; what reads it does not everywhere, before or since the per-row rule
        # (bound / mean 2^16.6 .. 2^18.7): hence balance(), see test_balanced_models_keep_the_two_term_kernels
        assert pn["trunk"], (name, pn)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(HEADS) + list(RESCALE))
def test_balanced_models_keep_the_two_term_kernels(name, shape):
    """what the library makes of a model before it plans (balance): the plain weights are left alone to the bit; every rescaled case is still
    the same function with the same float32 bits, is planned on two terms throughout (2^8 and 2^20 alike: the guard has nothing left to
    refuse), and the emulator on it is inside the bars"""
    head = name if name in HEADS else RESCALE[name][0]
    cfg, sd0, feats, l64, l32 = base_case(head, shape)
    sd = sd0 if name in HEADS else rescaled_sd(name, shape)
    bal = balance(sd, cfg)
    if name in HEADS:
        assert all(bal[k] is sd[k] for k in sd), name
    assert np.array_equal(oracle.model_forward(feats, bal, cfg).ravel(), l32), name
    p = plan(bal, cfg)
    err, f32 = rel_err(forward(feats, bal, cfg, p), l64), rel_err(l32, l64)
    print(f"{name} {shape} balanced: windows mean 2^{p['mean1']:.1f} / 2^{p['mean2']:.1f}, rows 2^{p['rows1']:.1f} / 2^{p['rows2']:.1f}, emulated {err:.2e}, float32 {f32:.2e}")
    assert p["trunk"] and p["consumer"], (name, p)
    assert bars_ok(err, f32), (name, err, f32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(UNBALANCED))
def test_unbalanced_cases_are_decided_as_stated(name, shape):
    """the restated guard gives each UNBALANCED case the forms its row states, before the per-row rule and with it (the device is held to
    the same in test_gpu_trunk_stress.py)"""
    cfg, sd = unbalanced_case(name, shape)
    po, pn = plan(sd, cfg, "mean"), plan(sd, cfg)
    print(f"{name} {shape}: windows mean 2^{pn['mean1']:.1f} / 2^{pn['mean2']:.1f}, rows 2^{pn['rows1']:.1f} / 2^{pn['rows2']:.1f}")
    assert (po["trunk"], po["consumer"]) == UNBALANCED[name][3] and (pn["trunk"], pn["consumer"]) == UNBALANCED[name][4], (name, po, pn)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("loud", [False, True], ids=["dead", "dead+loud"])
def test_balance_with_a_majority_of_dead_channels(shape, loud):
    """9 of conv1's 16 channels nearly dead (x 2^-24, nothing compensating): they are worth nothing to conv2, so they neither move nor drag
    the median down, and the live ones stay where they are; with a live channel x 2^12 and conv2's weights on it / 2^12 on top, that channel
    alone is brought back.  The same float32 bits, two terms throughout, the emulator inside the bars"""
    cfg, sd = dead_channel_case(shape)
    if loud:
        sd = rescale(sd, "crnn", 0, CH_A, 12)
    feats = base_case("crnn", shape)[2]
    l64, l32 = oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel(), oracle.model_forward(feats, sd, cfg).ravel()
    bal = balance(sd, cfg)
    moved = np.log2(bal["model.cnn.1.weight"] / sd["model.cnn.1.weight"])
    assert np.array_equal(oracle.model_forward(feats, bal, cfg).ravel(), l32)
    p = plan(bal, cfg)
    err, f32 = rel_err(forward(feats, bal, cfg, p), l64), rel_err(l32, l64)
    print(f"dead channels {shape} loud={loud}: moved by 2^{moved.astype(int).tolist()}, rows 2^{p['rows1']:.1f} / 2^{p['rows2']:.1f}, emulated {err:.2e}, "
          f"float32 {f32:.2e}, logit ptp {np.ptp(l64):.3g}")
    assert (np.delete(moved, CH_A) == 0).all() and moved[CH_A] == (-12 if loud else 0), moved
    assert p["trunk"] and p["consumer"], p
    assert np.ptp(l64) > 1e-2 and f32 <= BAR / 10 and bars_ok(err, f32), (err, f32)


# the cnn head at 2^20 under the mean's guard: the finding.  (37, 28): emulated 1.9e-4 and 5.6e-3 against a bar of 1e-4
TEETH = ["cnn-l0-2^20", "cnn-l01-2^20"]


@pytest.mark.parametrize("name", TEETH)
def test_cases_have_teeth(name):
    """the mean's guard keeps these on two terms and the emulator is outside the bars there; the per-row guard moves them"""
    po, eo, f32 = emulated(name, SHAPES[1], "mean")
    pn, _, _ = emulated(name, SHAPES[1], "rows")
    print(_row(name, SHAPES[1]))
    assert po["trunk"] and not bars_ok(eo, f32), (name, eo, f32)
    assert not pn["trunk"], name

