"""The BcResNet head on the HIP path (run with -m gpu) under the models and clips of tests/test_bcresnet_stress.py: one channel of a link
x 2^+-8 .. 2^+-24 with what reads it divided by the same power of two (the same function) - the init conv's BatchNorm, a block's two
BatchNorms, a depthwise row against its pointwise column, two links at once - whole batches of features x 2^-10 / 2^-5 / 2^5, one quiet clip
among ordinary ones and a quiet clip with one frame at full scale, at (32, 40) and (70, 64), batches of 33 and 8.  Every case under the
default arithmetic beside a conv_arith = "f32" model on the same weights, against the float64 oracle, relative to max(1, |ref|max):
f16x3 <= 2 x f32 + 2e-6, f16x3 <= 1e-4, every logit finite.  The library balances the channel gains of these models before it plans, so
every ReLU case and every depthwise case keeps its two-term kernels; GELU / SiLU BatchNorm links cannot be balanced and are held to the
restated per-block guard (test_bcresnet_stress.plan): the device's forms must be its forms.  Each case prints the plan taken and both errors.

Measured on an MI355X, 33 clips, max |logit - float64| / max(1, |logit|max), worst of both shapes; "before" = the library without the
balance and the guard (every block on two terms), "now" = with them; the conv_arith = "f32" model stands at 1.3e-6 .. 2.4e-6 throughout:

link (cases)                      | before: worst, where; cases outside the bars        | now: worst, forms
plain relu / gelu / silu          | 2.5e-6 / 2.1e-6 / 2.3e-6; none                      | the same bits, 2/2/2
l0  (ReLU, 2^+-8 .. 2^+-24)       | 4.1e-5 at 2^-24; 2^+-24                             | 2.5e-6, 2/2/2
l1                                | 6.7e-5 at 2^-24; 2^-24, and 2^-20 at (70, 64)       | 2.5e-6, 2/2/2
l2                                | 2.2e-5 at 2^24; 2^-20, 2^+-24                       | 2.5e-6, 2/2/2
l3  (float32 tail: the control)   | 2.5e-6; none                                        | 2.5e-6, 2/2/2
dw1 / dw2 / dw3                   | 2.5e-5 / 6.9e-5 / 1.8e-5 at 2^-24, 2^-24, 2^24      | 2.5e-6, 2/2/2
l0 + l1                           | 1.0e-4 at 2^-24 (70, 64); 2^+-24, 2^-20 at (70, 64) | 2.5e-6, 2/2/2
GELU / SiLU dw1 .. dw3 at 2^+-24  | 1.6e-5 .. 7.7e-5; 19 of 24                          | 2.1e-6 / 2.3e-6, 2/2/2
GELU / SiLU l0, 2^+-12 .. 2^+-24  | 6.2e-5 / 6.4e-5 at 2^-24; 2^+-24                    | 2.3e-6 / 3.1e-6; 3/2/2 from 2^+-16 on
GELU / SiLU l1                    | 8.4e-5 / 7.9e-5 at 2^-24; 2^-24 (SiLU: 2^24 too)    | 2.6e-6 / 2.8e-6; 2/3/2 from 2^+-16 on
GELU / SiLU l2                    | 2.3e-5 at 2^-24; 2^+-24, 2^-20                      | 2.1e-6 / 2.3e-6; 2/2/3 from 2^+-16 on
act_dtype = "f16", ReLU l0 .. l2, dw1 .. dw3 at 2^+-12, 2^+-20: |dlogit| up to 1.3e-1 before (bar 1e-2), 5.9e-3 now (the plain weights' figure)

The device errors before the fix are the emulator's (l0-2^-24: 4.1e-5 emulated and measured; l1-2^-24: 6.9e-5 / 6.7e-5; dw2-2^-24: 6.9e-5 both):
accumulation order, which the emulator leaves out, costs the device about 2e-6 on every row and nothing more.  On three terms now: the block
behind the rescaled link in every GELU / SiLU BatchNorm-link case from 2^+-16 on (60 of the 72 runs), nothing else; 2^+-12 stays on two.
The 2^+-16 cases were inside the bars on two terms as well (device 1.7e-6 .. 2.2e-6, emulated 3.6e-7): the guard's window is the planner's
usual 2^16 and errs to the slow side there."""
import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig
from nanowakeword_amd.synth import synth_features
from test_bcresnet_stress import (BAR, CASES, DATA, DW_ANY, MIXED_CLIP, RESCALE, SHAPES, UNBALANCED_CASES, _case_ids, balance, base_case, case_sd, data_feats,
                                  loud_frame_feats, mixed_feats, plan)

pytestmark = pytest.mark.gpu
BATCHES = (33, 8)
_ids = lambda s: "%dx%d" % s
F16_ACT_BAR = 1e-2                      # test_bcresnet_f16_activations' bar on |dlogit|


def _model(cfg, sd, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=sd, **kw)


def _forms(m):
    """-> per block, whether its two products run on two binary16 terms; each block has exactly one line that names its pointwise"""
    lines = m.describe_plan().splitlines()
    out = []
    for i in (1, 2, 3):
        mine = [l for l in lines if f"model.block{i}.pointwise" in l]
        assert len(mine) == 1, lines
        out.append("[f16x3]" in mine[0])
    return tuple(out)


def _hold(what, m, m32, cfg, sd, feats):
    """both batch sizes against the float64 oracle -> (the forms planned, the default arithmetic's logits on the whole batch)"""
    forms = _forms(m)
    assert "[f16x3]" not in m32.describe_plan(), m32.describe_plan()
    ref = oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel()
    out = None
    for B in BATCHES:
        lg, _ = m.forward_features(feats[:B])
        l32, _ = m32.forward_features(feats[:B])
        scale = max(1.0, float(np.abs(ref[:B]).max()))
        e, f = float(np.abs(lg.astype(np.float64) - ref[:B]).max()) / scale, float(np.abs(l32.astype(np.float64) - ref[:B]).max()) / scale
        print(f"{what} B={B}: blocks {'/'.join('2' if b else '3' for b in forms)}; max |dlogit| / max(1, |logit|max) vs float64: "
              f"f16x3 {e:.2e}, f32 {f:.2e} (|logit|max {np.abs(ref[:B]).max():.3g})")
        assert np.isfinite(lg).all() and np.isfinite(l32).all(), what
        assert e <= 2.0 * f + 2e-6, (what, B, e, f)
        assert e <= BAR, (what, B, e)
        out = lg if out is None else out
    return forms, out


def _case(name, shape):
    """one case on the device -> the forms planned"""
    cfg, sd = case_sd(name, shape)
    m, m32 = _model(cfg, sd), _model(cfg, sd, conv_arith="f32")
    try:
        forms, _ = _hold(f"{name} {shape}", m, m32, cfg, sd, base_case(shape)[2])
        p = plan(balance(sd, cfg), cfg)
        assert forms == p["blocks"], (name, p, m.describe_plan())
        return forms
    finally:
        m.close()
        m32.close()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("activation", ["relu", "gelu", "silu"])
def test_plain_weights_and_data_cases(activation, shape):
    """the plain weights reach every kernel under test at these shapes - the front kernel, two chained blocks, the last block with the fused
    mean, all on two terms - and are inside the bars on the plain clips and on quiet / loud ones; a quiet clip in an ordinary batch gives
    the bits it gives alone (every scale is taken inside a clip)"""
    cfg, sd, feats, _, _ = base_case(shape, activation)
    m, m32 = _model(cfg, sd), _model(cfg, sd, conv_arith="f32")
    try:
        lines = m.describe_plan().splitlines()
        assert any("conv1_dw_x3" in l and "[f16x3]" in l for l in lines), lines
        assert sum("bc_chain:" in l and "[f16x3]" in l for l in lines) == 2, lines
        assert any("dual_x3:model.block3" in l and "+ global_avg_pool" in l and "[f16x3]" in l for l in lines), lines
        assert _forms(m) == plan(sd, cfg)["blocks"] == (True, True, True)
        _hold(f"bcresnet {activation} {shape} plain", m, m32, cfg, sd, feats)
        for name in DATA:
            _hold(f"bcresnet {activation} {shape} features {name}", m, m32, cfg, sd, data_feats(name, shape))
        for what, x in (("one quiet clip", mixed_feats(shape)), ("a quiet clip with one loud frame", loud_frame_feats(shape))):
            _, full = _hold(f"bcresnet {activation} {shape} {what}", m, m32, cfg, sd, x)
            alone, _ = m.forward_features(x[MIXED_CLIP:MIXED_CLIP + 1])
            assert full[MIXED_CLIP] == alone[0] and full[MIXED_CLIP] != full[MIXED_CLIP + 1]
    finally:
        m.close()
        m32.close()


@pytest.mark.parametrize("name,shape", CASES, ids=_case_ids)
def test_rescaled_channels(name, shape):
    """the ReLU cases: balanced at load time, so all on two terms (the restated balance and guard say the same) and inside the bars"""
    assert _case(name, shape) == (True, True, True)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("name", list(DW_ANY))
def test_depthwise_links_under_gelu_and_silu(name, shape):
    """a depthwise row against its pointwise column is balanced under every activation"""
    assert _case(name, shape) == (True, True, True)


@pytest.mark.parametrize("name,shape", UNBALANCED_CASES, ids=[f"{n}-{_ids(s)}" for n, s in UNBALANCED_CASES])
def test_unbalanced_heads_are_left_to_the_guard(name, shape):
    """GELU / SiLU BatchNorm links: the device plan is the restated guard's, block by block, and the logits are inside the bars"""
    _case(name, shape)


def test_batch_invariance_past_the_persistent_grid():
    """300 clips at (32, 40) - more than bc_chain's persistent workgroups - on a rescaled case that stays on two terms: the first 33 logits
    are the bits of the 33-clip run"""
    shape, name = SHAPES[0], "l1-2^-24"
    cfg, sd = case_sd(name, shape)
    feats = np.concatenate([base_case(shape)[2], synth_features(267, shape, seed=10)])
    m = _model(cfg, sd)
    try:
        assert _forms(m) == (True, True, True), m.describe_plan()
        small, _ = m.forward_features(feats[:33])
        big, _ = m.forward_features(feats)
        ref = oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel()
        e = float(np.abs(big.astype(np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))
        print(f"{name} {shape} B=300: f16x3 {e:.2e} vs float64")
        assert np.array_equal(big[:33], small)
        assert e <= BAR, e
    finally:
        m.close()


F16_ACT_CASES = [n for n, steps in RESCALE.items() if len(steps) == 1 and abs(steps[0][2]) in (12, 20)]


@pytest.mark.parametrize("name", F16_ACT_CASES)
def test_f16_activation_storage(name):
    """act_dtype = "f16": the tensors between the kernels carry ONE plan-time power of two each (capped at typ x 2^16), so without the
    balance a loud channel must either saturate or flush its neighbours.  The ReLU BatchNorm-link and depthwise cases at 2^+-12 and 2^+-20
    against float64 at that mode's bar, 1e-2 on |dlogit| (test_bcresnet_f16_activations)"""
    shape = SHAPES[0]
    cfg, sd = case_sd(name, shape)
    feats = base_case(shape)[2]
    ref = oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel()
    m = _model(cfg, sd, act_dtype="f16")
    try:
        assert m.describe_plan().count("(f16 activations)") == 3, m.describe_plan()
        lg, _ = m.forward_features(feats)
        e = float(np.abs(lg.astype(np.float64) - ref).max())
        print(f"{name} {shape} act_dtype=f16: max |dlogit| vs float64 {e:.2e}")
        assert np.isfinite(lg).all() and e <= F16_ACT_BAR, (name, e)
    finally:
        m.close()


@pytest.mark.parametrize("name", ["gelu-l1-2^-20", "silu-l0-2^20"])
def test_f16_activation_storage_unbalanceable_is_finite(name):
    """GELU / SiLU BatchNorm links under 16-bit storage are out of this file's scope: printed, and held to finite logits only"""
    shape = SHAPES[0]
    cfg, sd = case_sd(name, shape)
    feats = base_case(shape)[2]
    ref = oracle.model_forward(feats, sd, cfg, dtype=np.float64).ravel()
    m = _model(cfg, sd, act_dtype="f16")
    try:
        lg, _ = m.forward_features(feats)
        print(f"{name} {shape} act_dtype=f16: max |dlogit| vs float64 {float(np.abs(lg.astype(np.float64) - ref).max()):.2e}")
        assert np.isfinite(lg).all(), name
    finally:
        m.close()
