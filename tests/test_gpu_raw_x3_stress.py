"""The raw-PCM frontend on the HIP path under models and clips that stress raw_x3's plan-time plane scales (run with -m gpu): one channel of a
stage x 2^8 .. 2^20 with the next stage's weights on it divided by the same power of two (the same function; tests/test_raw_x3_stress.py has the
cases and a numpy emulation of the kernel on them), quiet clips down to +-1 LSB, one full-scale sample at the tile and halo edges, a quiet clip
in a loud batch, heavy-tailed frontend weights.  Every case against the float64 restatement at the bars of test_gpu_e2e_quartznet.py, beside a
conv_arith = "f32" model on the same weights, whatever plan was chosen; the plan is asserted where the range guard must not move it and checked
against the CPU restatement of the guard everywhere else."""
import numpy as np
import pytest

import raw_oracle
from nanowakeword_amd.config import FrontendConfig
from nanowakeword_amd.synth import synth_pcm
from parity import LOGIT_ATOL
from test_gpu_e2e_quartznet import _check_frontend, _check_logits, _frontend_lines
from test_raw_x3_stress import (HEAVY, KEEPS_FUSED, MAIN, RESCALE, SHAPES, base_case, heavy_frontend_sd, impulse, plan, quiet_noise, rescaled_sd)

pytestmark = pytest.mark.gpu


def _model(cfg, sd, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=sd, **kw)


@pytest.fixture(scope="module")
def plain_models():
    """shape -> (default-arithmetic model, conv_arith = f32 model, the f32 model's frontend on the four clips) on synth_state_dict"""
    made = {}

    def get(shape):
        if shape not in made:
            cfg, sd, pcm, _, _ = base_case(shape)
            m, m32 = _model(cfg, sd), _model(cfg, sd, conv_arith="f32")
            made[shape] = (m, m32, m32.frontend(pcm))
        return made[shape]
    yield get
    for m, m32, _ in made.values():
        m.close()
        m32.close()


def _plan_form(m, depth):
    """the frontend's lines are one of the two known forms -> True for the one-launch one"""
    fe = _frontend_lines(m)
    if len(fe) == 1 and fe[0].startswith("frontend:raw_x3:model.frontend (%d stages" % depth):
        return True
    assert len(fe) == depth and all(l.startswith("frontend:conv1d_strided:") for l in fe), fe
    return False


def _hold(what, m, m32, cfg, sd, pcm):
    """the existing bars on frontend and logit, then - relative to max(1, |ref|max), test_heavy_tailed_weights_against_float64's convention -
    the default arithmetic no worse than 2 x the float32 one + 2e-6, on the frontend and on the logit -> the figures"""
    e_f, e_l = _check_frontend(m, cfg, sd, pcm, what), _check_logits(m, cfg, sd, pcm, what)
    f_f, f_l = _check_frontend(m32, cfg, sd, pcm, what), _check_logits(m32, cfg, sd, pcm, what)
    f64, _, l64 = raw_oracle.forward(pcm, sd, cfg, dtype=np.float64)
    sf, sl = max(1.0, float(np.abs(f64).max())), max(1.0, float(np.abs(l64).max()))
    fused = _plan_form(m, len(_frontend_lines(m32)))
    print(f"{what}: plan {'raw_x3' if fused else 'conv1d_strided per stage'}; frontend max |d| vs float64 {e_f:.2e} (f32 model {f_f:.2e}, bar {LOGIT_ATOL * sf:.2e}), "
          f"logit {e_l:.2e} (f32 model {f_l:.2e}, bar {LOGIT_ATOL:.0e})")
    assert "raw_x3" not in m32.describe_plan() and "[f16x3]" not in m32.describe_plan()
    assert e_f / sf <= 2.0 * f_f / sf + 2e-6, (what, e_f, f_f, sf)
    assert e_l / sl <= 2.0 * f_l / sl + 2e-6, (what, e_l, f_l, sl)
    return fused


# ---- 1: the function-preserving rescale
@pytest.mark.parametrize("shape", list(SHAPES))
def test_plain_weights_stay_on_raw_x3(plain_models, shape):
    cfg, sd, pcm, _, _ = base_case(shape)
    m, m32, _ = plain_models(shape)
    assert _hold(shape, m, m32, cfg, sd, pcm) and plan(sd, cfg)[1], m.describe_plan()


@pytest.mark.parametrize("name", list(RESCALE))
def test_rescaled_channels(plain_models, name):
    shape = RESCALE[name][0]
    cfg, _, pcm, _, _ = base_case(shape)
    sd = rescaled_sd(name)
    m, m32 = _model(cfg, sd), _model(cfg, sd, conv_arith="f32")
    try:
        fused = _hold(name, m, m32, cfg, sd, pcm)
        # the guard on the device is the one test_raw_x3_stress.py restates (and holds to the emulator)
        assert fused == plan(sd, cfg)[1], (name, m.describe_plan())
        if name in KEEPS_FUSED:
            assert fused, (name, m.describe_plan())
        # float32 path: the fold is float64 rounded once and G a power of two, so the rescaled model is the plain one bit for bit
        assert np.array_equal(m32.frontend(pcm), plain_models(shape)[2]), name
    finally:
        m.close()
        m32.close()


# ---- 2: quiet clips, and one full-scale sample at the tile and halo edges (main shape: 8193 samples, 33 rows)
N_MAIN = SHAPES[MAIN][2]
QUIET = {"noise_1lsb": lambda: quiet_noise(1, N_MAIN, 2), "noise_16lsb": lambda: quiet_noise(16, N_MAIN, 2), "noise_256lsb": lambda: quiet_noise(256, N_MAIN, 2),
         "impulse_0": lambda: impulse(N_MAIN, 0), "impulse_4095": lambda: impulse(N_MAIN, 4095), "impulse_4096": lambda: impulse(N_MAIN, 4096),
         "impulse_last": lambda: impulse(N_MAIN, N_MAIN - 1)}


@pytest.mark.parametrize("clip", list(QUIET))
def test_quiet_clips(plain_models, clip):
    cfg, sd, _, _, _ = base_case(MAIN)
    m, m32, _ = plain_models(MAIN)
    pcm = QUIET[clip]()
    assert _hold(clip, m, m32, cfg, sd, pcm), m.describe_plan()
    # what the clip is worth beside the bias
    zero = raw_oracle.forward(np.zeros_like(pcm), sd, cfg, dtype=np.float64)[0]
    moved = float(np.abs(raw_oracle.forward(pcm, sd, cfg, dtype=np.float64)[0] - zero).max())
    print(f"{clip}: the clip moves the float64 frontend by {moved:.2e}")
    assert moved > 0.0, clip


def test_quiet_clip_in_a_loud_batch(plain_models):
    """one +-1 LSB clip among 70 loud ones gives the bits it gives alone: no scale depends on the data"""
    m, _, _ = plain_models(MAIN)
    assert _plan_form(m, 3)
    batch = synth_pcm("loud", 71, N_MAIN, seed=8)
    batch[37] = quiet_noise(1, N_MAIN)[0]
    alone_f, alone_l = m.frontend(batch[37:38]), m.forward_pcm(batch[37:38])[0]
    full_f, full_l = m.frontend(batch), m.forward_pcm(batch)[0]
    assert np.array_equal(full_f[37], alone_f[0]) and full_l[37] == alone_l[0]
    assert not np.array_equal(full_f[36], alone_f[0])


# ---- 3: heavy-tailed frontend weights through forward_pcm
@pytest.mark.parametrize("name", list(HEAVY))
def test_heavy_tailed_frontend_weights(name):
    cfg, _, pcm, _, _ = base_case(MAIN)
    sd = heavy_frontend_sd(name)
    m, m32 = _model(cfg, sd), _model(cfg, sd, conv_arith="f32")
    try:
        fused = _hold("heavy-tailed " + name, m, m32, cfg, sd, pcm)
        assert fused == plan(sd, cfg)[1], (name, m.describe_plan())
    finally:
        m.close()
        m32.close()
