"""The plan-time-scaled conv trunks on the HIP path (run with -m gpu) under the models and clips of tests/test_trunk_stress.py: one channel of a
layer x 2^8 .. 2^20 with the next layer's weights on it divided by the same power of two (the same function), two such channels in two
successive layers, the quiet-channel mirror x 2^-g, whole batches of features x 2^-10 / 2^-5 / 2^5 and one quiet clip among ordinary ones - the
cnn, crnn and e2e_dnn heads at (24, 16) and (37, 28), batches of 33 and 8.  Every case under the default arithmetic beside a conv_arith = "f32"
model on the same weights, against the float64 oracle, at test_heavy_tailed_weights_against_float64's contract relative to max(1, |ref|max):
f16x3 <= 2 x f32 + 2e-6, f16x3 <= 1e-4, every logit finite.  The library balances the channel gains of these ReLU models before it plans, so
every case must keep its two-term kernels (asserted, with the restated balance and guard); GELU / SiLU heads, which cannot be balanced, are
held to the restated range guard alone, each of its three places (add_trunk, add_gemm, add_conv_mfma) deciding some case by itself.  Each case prints the plan taken and both errors."""
import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig
from test_trunk_stress import (BAR, DATA, HEADS, MIXED_CLIP, RESCALE, SHAPES, UNBALANCED, balance, base_case, data_feats, dead_channel_case,
                               mixed_feats, plan, rescale, rescaled_sd, unbalanced_case)

pytestmark = pytest.mark.gpu
BATCHES = (33, 8)
_ids = lambda s: "%dx%d" % s


def _model(cfg, sd, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=sd, **kw)


@pytest.fixture(scope="module")
def plain_models():
    """(head, shape) -> (default-arithmetic model, conv_arith = f32 model) on synth_state_dict, built once"""
    made = {}

    def get(head, shape):
        if (head, shape) not in made:
            cfg, sd, _, _, _ = base_case(head, shape)
            made[head, shape] = (_model(cfg, sd), _model(cfg, sd, conv_arith="f32"))
        return made[head, shape]
    yield get
    for m, m32 in made.values():
        m.close()
        m32.close()


def _forms(m, head):
    """-> (trunk_x3 on two terms, what reads it - fc1 / the third conv on conv3_x3 - on two terms); the kernels themselves must be planned"""
    lines = m.describe_plan().splitlines()
    trunk = [l for l in lines if "trunk_x3:" in l]
    cons = [l for l in lines if ("gemm:fc1" in l if head == "cnn" else "conv3_x3" in l)]
    assert len(trunk) == 1 and len(cons) == 1, lines
    return "[f16x3]" in trunk[0], "[f16x3]" in cons[0]


def _hold(what, head, m, m32, cfg, sd, feats):
    """both batch sizes against the float64 oracle -> (the forms planned, the default arithmetic's logits on the whole batch)"""
    forms = _forms(m, head)
    assert "[f16x3]" not in m32.describe_plan(), m32.describe_plan()
    ref = oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel()
    out = None
    for B in BATCHES:
        lg, _ = m.forward_features(feats[:B])
        l32, _ = m32.forward_features(feats[:B])
        scale = max(1.0, float(np.abs(ref[:B]).max()))
        e, f = float(np.abs(lg.astype(np.float64) - ref[:B]).max()) / scale, float(np.abs(l32.astype(np.float64) - ref[:B]).max()) / scale
        print(f"{what} B={B}: plan trunk_x3 {'two' if forms[0] else 'three'}-term, {'fc1' if head == 'cnn' else 'conv3_x3'} {'two' if forms[1] else 'three'}-term; "
              f"max |dlogit| / max(1, |logit|max) vs float64: f16x3 {e:.2e}, f32 {f:.2e} (|logit|max {np.abs(ref[:B]).max():.3g})")
        assert np.isfinite(lg).all() and np.isfinite(l32).all(), what
        assert e <= 2.0 * f + 2e-6, (what, B, e, f)
        assert e <= BAR, (what, B, e)
        out = lg if out is None else out
    return forms, out


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("head", HEADS)
def test_plain_weights_and_data_cases(plain_models, head, shape):
    """the plain weights keep trunk_x3, fc1's gemm and conv3_x3 on the two-term form at these shapes (so the shapes reach the kernels), on the
    plain clips and on quiet / loud ones; a quiet clip in an ordinary batch gives the bits it gives alone (no scale depends on the data)"""
    cfg, sd, feats, _, _ = base_case(head, shape)
    m, m32 = plain_models(head, shape)
    assert _forms(m, head) == (True, True), m.describe_plan()
    p = plan(sd, cfg)
    assert p["trunk"] and p["consumer"]
    _hold(f"{head} {shape} plain", head, m, m32, cfg, sd, feats)
    for name in DATA:
        _hold(f"{head} {shape} features {name}", head, m, m32, cfg, sd, data_feats(name, shape))
    mixed = mixed_feats(shape)
    _, full = _hold(f"{head} {shape} one quiet clip", head, m, m32, cfg, sd, mixed)
    alone, _ = m.forward_features(mixed[MIXED_CLIP:MIXED_CLIP + 1])
    assert full[MIXED_CLIP] == alone[0] and full[MIXED_CLIP] != full[MIXED_CLIP + 1]


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("name", list(RESCALE))
def test_rescaled_channels(name, shape):
    head = RESCALE[name][0]
    cfg, _, feats, _, _ = base_case(head, shape)
    sd = rescaled_sd(name, shape)
    m, m32 = _model(cfg, sd), _model(cfg, sd, conv_arith="f32")
    try:
        forms, _ = _hold(f"{name} {shape}", head, m, m32, cfg, sd, feats)
        # the library balances the channel gains of a ReLU model before it plans (test_trunk_stress.balance restates it), so every case keeps
        # its two-term kernels; the guard on the balanced weights is the one test_trunk_stress.py restates (and holds to the emulator)
        # (2^8 included: the guard alone would send fc1 / conv3_x3 behind a conv1 or conv2 channel x 2^8 to three terms - bound / mean
        # 2^16.6 .. 2^18.7 against the 2^16 window, before the per-row rule as after it - and the balancing is what keeps them)
        p = plan(balance(sd, cfg), cfg)
        assert forms == (p["trunk"], p["consumer"]) == (True, True), (name, p, m.describe_plan())
    finally:
        m.close()
        m32.close()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("name", list(UNBALANCED))
def test_unbalanced_heads_are_left_to_the_guard(name, shape):
    """GELU / SiLU heads cannot be balanced (they are not positively homogeneous), so there the range guard alone decides.  The device plan is
    the restated guard's - the forms each case states, among them the rows where only add_gemm's (fc1) or add_conv_mfma's (conv3_x3) per-row
    rule moves anything: trunk_x3 stays on two terms, what reads it falls back - and the logits are inside the bars"""
    head = UNBALANCED[name][0]
    cfg, sd = unbalanced_case(name, shape)
    feats = base_case(head, shape)[2]
    m, m32 = _model(cfg, sd), _model(cfg, sd, conv_arith="f32")
    try:
        forms, _ = _hold(f"{name} {shape}", head, m, m32, cfg, sd, feats)
        p = plan(sd, cfg)
        assert forms == (p["trunk"], p["consumer"]) == UNBALANCED[name][4], (name, p, m.describe_plan())
    finally:
        m.close()
        m32.close()


@pytest.mark.parametrize("loud", [False, True], ids=["dead", "dead+loud"])
def test_majority_of_dead_channels(loud):
    """a ReLU crnn head with 9 of conv1's 16 channels nearly dead, and with a live channel x 2^12 (compensated) on top: the dead channels do
    not set the balance, the model keeps its two-term kernels and is inside the bars"""
    shape = SHAPES[1]
    cfg, sd = dead_channel_case(shape)
    if loud:
        sd = rescale(sd, "crnn", 0, 3, 12)
    m, m32 = _model(cfg, sd), _model(cfg, sd, conv_arith="f32")
    try:
        forms, _ = _hold(f"crnn dead channels loud={loud} {shape}", "crnn", m, m32, cfg, sd, base_case("crnn", shape)[2])
        p = plan(balance(sd, cfg), cfg)
        assert forms == (p["trunk"], p["consumer"]) == (True, True), (p, m.describe_plan())
    finally:
        m.close()
        m32.close()
