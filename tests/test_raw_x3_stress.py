"""The raw-PCM frontend's stressed models and clips (tests/test_gpu_raw_x3_stress.py runs them on the HIP path), and a numpy emulator of
raw_x3.hip's arithmetic under plan_raw_frontend's plan-time scales.  raw_x3 is the one two-term binary16 kernel whose plane scales come from
a worst-case bound alone (|x| <= 1 through the folded weights' row 1-norms), so a model whose folded BatchNorm gains spread - one channel of a
stage x G = 2^g, the next stage's weights on that channel / G: the same function, bit for bit in float32 - pushes every OTHER channel g bits
down its plane.  Here, on the CPU: the rescale leaves the restatement alone, the emulator is inside the frontend bar on the plain weights and
outside it on the rescaled models that the planner's range guard therefore has to send to the per-stage launches, and every model the guard
leaves on raw_x3 is emulated at a quarter of the bar or better.  numpy only: nothing here loads the native library."""
import functools
import math

import numpy as np
import pytest

import raw_oracle
from nanowakeword_amd.config import HeadConfig, raw_frontend_frames
from nanowakeword_amd.synth import synth_pcm, synth_state_dict
from parity import LOGIT_ATOL
from test_gpu_parity import _heavy_tailed

# ---- shapes: name -> (channels, depth, samples); the main one gives 33 rows (two tiles of 32)
SHAPES = {"c32_d3": (32, 3, 8193), "c16_d3": (16, 3, 4000), "c32_d2": (32, 2, 4100)}
MAIN = "c32_d3"
CHANNEL = 3                                   # the one rescaled channel
CHANNELS_8 = tuple(range(1, 32, 4))           # the eight of the 8-channel case
RAW_RANGE_LOG2 = 16 + 4                       # plan_raw_frontend's window: 2^4 x f16_range_factor() (nww_knobs().f16_range_log2 = 16)
RAW_PCM_TYP = 2.0 ** -5                       # plan_raw_frontend's stated typical |x|: 1024 LSB, -30 dBFS


def _case(shape, g, stages, channels=(CHANNEL,)):
    return (shape, g, tuple(stages), tuple(channels))


# name -> (shape, log2 G, rescaled stages, rescaled channels).  Stage i rescaled = channel c of stage i x G, stage i + 1's weights on it / G,
# so the last stage cannot be: depth 2 has stage 0 only
RESCALE = {f"{MAIN}-2^{g}-s{''.join(map(str, st))}": _case(MAIN, g, st) for g in (8, 12, 16, 20) for st in ((0,), (1,), (0, 1))}
RESCALE[f"{MAIN}-2^12-s01-8ch"] = _case(MAIN, 12, (0, 1), CHANNELS_8)
RESCALE.update({f"c16_d3-2^{g}-s{''.join(map(str, st))}": _case("c16_d3", g, st) for g in (12, 20) for st in ((0,), (1,), (0, 1))})
RESCALE.update({f"c32_d2-2^{g}-s0": _case("c32_d2", g, (0,)) for g in (12, 20)})
# the emulator under the unguarded scales is outside the frontend bar on these (measured beside each in test_cases_have_teeth's output)
TEETH = [f"{MAIN}-2^12-s01", f"{MAIN}-2^16-s01", f"{MAIN}-2^20-s0", f"{MAIN}-2^20-s1", f"{MAIN}-2^20-s01"]
# one stage x 2^8 costs nothing (emulated 4e-7): the guard must leave these on the one-launch path
KEEPS_FUSED = [f"{MAIN}-2^8-s0", f"{MAIN}-2^8-s1"]

# heavy-tailed frontend weights (test_gpu_parity._heavy_tailed on the three frontend conv tensors only): name -> (factor, seed)
HEAVY = {"x2^12": (2.0 ** 12, 77),      # float64 oracle, the four clips: logit ptp 2.12 (the default seed does; nothing collapses)
         "x2^20": (2.0 ** 20, 77)}      # 2.12


def config(shape):
    channels, depth, n = SHAPES[shape]
    probe = HeadConfig("e2e_quartznet", (1, channels * 2 ** (depth - 1)), e2e_frontend_channels=channels, e2e_frontend_depth=depth)
    return HeadConfig("e2e_quartznet", (raw_frontend_frames(probe, n), probe.input_shape[1]), e2e_frontend_channels=channels, e2e_frontend_depth=depth)


def rescale(sd, stage, channels, G):
    """channels of stage `stage` x G (its BatchNorm's weight and bias), stage + 1's conv weights on them / G: ReLU is positively homogeneous
    and G a power of two, so the network is the same function and its float32 evaluation the same bits"""
    assert G == 2.0 ** round(math.log2(G))
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    bn, nxt = f"model.frontend.conv_blocks.{3 * stage + 1}", f"model.frontend.conv_blocks.{3 * stage + 3}.weight"
    assert nxt in out, "the last stage has no conv behind it to take 1 / G"
    for c in channels:
        out[bn + ".weight"][c] *= np.float32(G)
        out[bn + ".bias"][c] *= np.float32(G)
        out[nxt][:, c, :] /= np.float32(G)
    return out


def stress_pcm(n):
    """the four clips of the rescale cases: noise (+-8192), a sine, zeros, +-16 LSB noise"""
    quiet = np.random.default_rng(5).integers(-16, 17, size=(1, n)).astype(np.int16)
    return np.concatenate([synth_pcm(k, 1, n, seed=10) for k in ("noise", "sine", "zeros")] + [quiet], 0)


def quiet_noise(lsb, n, clips=1, seed=6):
    return np.random.default_rng([seed, lsb]).integers(-lsb, lsb + 1, size=(clips, n)).astype(np.int16)


def impulse(n, at):
    x = np.zeros((1, n), np.int16)
    x[0, at] = 32767
    return x


@functools.lru_cache(maxsize=None)
def base_case(shape):
    """-> (cfg, synth_state_dict, the four clips, float64 frontend, float64 logits): evaluated once, read-only"""
    cfg = config(shape)
    sd = synth_state_dict(cfg)
    pcm = stress_pcm(SHAPES[shape][2])
    f64, _, l64 = raw_oracle.forward(pcm, sd, cfg, dtype=np.float64)
    for a in (pcm, f64, l64, *sd.values()):
        a.setflags(write=False)
    return cfg, sd, pcm, f64, l64


@functools.lru_cache(maxsize=None)
def rescaled_sd(name):
    shape, g, stages, channels = RESCALE[name]
    sd = base_case(shape)[1]
    for s in stages:
        sd = rescale(sd, s, channels, 2.0 ** g)
    for a in sd.values():
        a.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def heavy_frontend_sd(name):
    factor, seed = HEAVY[name]
    sd = dict(base_case(MAIN)[1])
    convs = {k: v for k, v in sd.items() if k.startswith("model.frontend.conv_blocks.") and v.ndim == 3}
    assert len(convs) == 3
    sd.update(_heavy_tailed(convs, factor, seed=seed))
    for a in sd.values():
        a.setflags(write=False)
    return sd


# ---- plan_raw_frontend's arithmetic (nww_plan.hip, nww_weights.hip)
def fold(sd, i):
    """fold_raw_frontend: the stage's BatchNorm folded into its conv in float64, rounded once -> (w [Cout, Cin, k], b [Cout]) float32"""
    w = np.asarray(sd[f"model.frontend.conv_blocks.{3 * i}.weight"], np.float32).astype(np.float64)
    g, b, mu, var = (np.asarray(sd[f"model.frontend.conv_blocks.{3 * i + 1}.{s}"], np.float32).astype(np.float64)
                     for s in ("weight", "bias", "running_mean", "running_var"))
    al = g / np.sqrt(var + 1e-5)
    return (al[:, None, None] * w).astype(np.float32), (b - mu * al).astype(np.float32)


def f16_pow2_floor(x):
    return math.ldexp(1.0, math.frexp(x)[1] - 1)


def f16_scale(bound):
    """|v| <= bound times this stays inside binary16 with 2 % to spare: a power of two, at most 2^40; 0 = no usable bound"""
    if not bound > 1e-30:
        bound = 1e-30
    if not bound < 1e30:
        return 0.0
    return min(f16_pow2_floor(65504.0 / (bound * 1.02)), 2.0 ** 40)


def f16_wscale(w):
    return f16_scale(float(np.abs(np.asarray(w, np.float64)).max()) * 2.0)


def plan(sd, cfg):
    """-> per stage dict(w, b, bound (of its output), and behind stage 0: ws, sc (of the plane it reads), un, window = the bound of that plane
    over the smallest input magnitude any of its output channels lives on, as plan_raw_frontend's guard takes it), and fused = the guard's verdict.
    typ of a channel: sqrt(sum_q w_q^2 typ_q^2 + b^2) from RAW_PCM_TYP - per channel, so that a rescaled channel carries its G into the next
    stage's sum with the 1 / G of the weights on it (a mean over the channels would take G / Cout for the magnitude of all of them)"""
    stages, bound, typ, fused = [], 1.0, None, True
    for i in range(len([k for k in sd if k.startswith("model.frontend.conv_blocks.") and k.endswith(".running_var")])):
        w, b = fold(sd, i)
        w64, b64 = w.astype(np.float64), b.astype(np.float64)
        st = dict(w=w, b=b)
        if i > 0:
            st["ws"], st["sc"] = f16_wscale(w), f16_scale(bound)
            st["un"] = np.float32(1.0) / np.float32(st["ws"] * st["sc"])
        sig2 = (w64 ** 2 * (RAW_PCM_TYP ** 2 if typ is None else typ[None, :, None] ** 2)).sum(axis=(1, 2))
        if i > 0:
            # the plane this stage reads: what its input is worth to output channel co is typ_co / ||w_co||_2, the input magnitude that would
            # give the channel its typical output through the row's 2-norm - the plane's absolute error reaches it through the same norm
            norm = np.sqrt((w64 ** 2).sum(axis=(1, 2)))
            live = norm > 0
            eff = float((np.sqrt(sig2[live]) / norm[live]).min()) if live.any() else 0.0
            st["window"] = bound / eff if eff > 0 else math.inf
            fused = fused and st["window"] <= 2.0 ** RAW_RANGE_LOG2
        typ = np.sqrt(sig2 + b64 ** 2)
        bound = float((np.abs(w64).sum(axis=(1, 2)) * bound + np.abs(b64)).max()) * (1.0 + 1e-6)
        st["bound"] = bound
        stages.append(st)
    return stages, fused


# ---- raw_x3.hip's arithmetic
def _split(v):
    """nww_split2h: hi = RN16(v), lo = RN16(v - hi) (the remainder is exact in float32)"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _stage0(pcm, w, b):
    """float32 fmaf chain in tap order from the bias, taps x 2^-15, on the int16 samples, zero padding 20 -> [B, L0, C1] (pre-ReLU)"""
    B, n = pcm.shape
    L = (n - 1) // 16 + 1
    xp = np.zeros((B, 16 * (L - 1) + 41), np.float64)
    hi = min(n, xp.shape[1] - 20)
    xp[:, 20:20 + hi] = pcm[:, :hi]
    taps = (w[:, 0, :] * np.float32(1.0 / 32768.0)).astype(np.float32).astype(np.float64)       # [C1, 41]
    acc = np.broadcast_to(b.astype(np.float32), (B, L, len(b))).copy()
    for j in range(41):
        # one fmaf: the product of a 16-bit sample and a 24-bit tap is exact in float64
        acc = (acc.astype(np.float64) + xp[:, j:j + 16 * (L - 1) + 1:16, None] * taps[None, None, :, j]).astype(np.float32)
    return acc


def _stage(h, st, products=3):
    """one strided stage (k 13, stride 4, padding 6) on the matrix pipe: h [B, Lin, Cin] float32 >= 0 -> [B, Lout, Cout] float32 after ReLU.
    K-chunk = 16 channels of one tap; per chunk wl.xh, wh.xl, wh.xh (binary16 products are exact), each chunk's sum added to a float32
    accumulator; then fmaf(acc, un, bias)"""
    B, Lin, Cin = h.shape
    w, b = st["w"], st["b"]
    Cout, Lout = w.shape[0], (Lin - 1) // 4 + 1
    xh, xl = _split(h * np.float32(st["sc"]))
    wh, wl = _split(w * np.float32(st["ws"]))                                                  # [Cout, Cin, 13]
    pad = ((0, 0), (6, max(0, 4 * (Lout - 1) + 13 - 6 - Lin)), (0, 0))
    xh, xl = np.pad(xh, pad), np.pad(xl, pad)
    acc = np.zeros((B, Lout, Cout), np.float32)
    terms = [(wl, xh), (wh, xl), (wh, xh)][3 - products:]
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(13):
            rows = slice(j, j + 4 * (Lout - 1) + 1, 4)
            for c0 in range(0, Cin, 16):
                for wt, xt in terms:
                    acc = (acc.astype(np.float64) + xt[:, rows, c0:c0 + 16] @ wt[:, c0:c0 + 16, j].T).astype(np.float32)
        v = (acc.astype(np.float64) * np.float64(st["un"]) + b.astype(np.float64)).astype(np.float32)
    return np.maximum(v, np.float32(0.0))


def emulate(pcm, sd, cfg):
    """raw_x3's frontend [B, C, rows] float32 for int16 pcm [B, N] under plan()'s scales, whatever the guard says.  The halo rows a workgroup
    recomputes are the rows themselves (no scale depends on the data), so the tiles are not restated."""
    stages, _ = plan(sd, cfg)
    h = np.maximum(_stage0(np.asarray(pcm), stages[0]["w"], stages[0]["b"]), np.float32(0.0))
    for st in stages[1:]:
        h = _stage(h, st)
    return np.ascontiguousarray(h.transpose(0, 2, 1))


def bar(ref):
    return LOGIT_ATOL * max(1.0, float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def emulated_error(name):
    """max |emulated frontend - float64| of a RESCALE case (None: the shape's plain weights) on the four clips"""
    shape = name if name in SHAPES else RESCALE[name][0]
    cfg, sd0, pcm, f64, _ = base_case(shape)
    with np.errstate(invalid="ignore"):
        d = np.abs(emulate(pcm, sd0 if name in SHAPES else rescaled_sd(name), cfg) - f64)
    return float(np.nan_to_num(d, nan=np.inf).max())


# ---- the tests
@pytest.mark.parametrize("name", list(RESCALE))
def test_rescale_preserves_the_function(name):
    """float32 restatement: the same bits; float64: 1e-12 relative (the rescaled BatchNorm parameters are float32 x 2^g, exact)"""
    cfg, sd0, pcm, f64, l64 = base_case(RESCALE[name][0])
    sd = rescaled_sd(name)
    a, b = raw_oracle.forward(pcm, sd0, cfg), raw_oracle.forward(pcm, sd, cfg)
    assert np.array_equal(a[0], b[0]), name
    g64, _, m64 = raw_oracle.forward(pcm, sd, cfg, dtype=np.float64)
    assert np.abs(g64 - f64).max() <= 1e-12 * np.abs(f64).max() and np.abs(m64 - l64).max() <= 1e-12 * max(1.0, np.abs(l64).max()), name


@pytest.mark.parametrize("shape", list(SHAPES))
def test_emulator_inside_the_bar_on_plain_weights(shape):
    cfg, sd, pcm, f64, _ = base_case(shape)
    err = emulated_error(shape)
    f32 = float(np.abs(raw_oracle.forward(pcm, sd, cfg)[0] - f64).max())
    print(f"{shape}: emulated raw_x3 {err:.2e}, float32 restatement {f32:.2e}, bar {bar(f64):.2e}")
    assert plan(sd, cfg)[1] and err <= bar(f64) / 4, (shape, err)


@pytest.mark.parametrize("name", TEETH)
def test_cases_have_teeth(name):
    """raw_x3 under the bound-only scales is outside the frontend bar on these: why plan_raw_frontend has its range guard, which sends them
    to the per-stage launches"""
    f64 = base_case(RESCALE[name][0])[3]
    err = emulated_error(name)
    print(f"{name}: emulated raw_x3 {err:.2e}, bar {bar(f64):.2e}")
    assert err > bar(f64), (name, err)
    assert not plan(rescaled_sd(name), config(RESCALE[name][0]))[1], name


@pytest.mark.parametrize("name", list(RESCALE))
def test_guard_leaves_only_sound_cases_fused(name):
    """what the guard (plan()'s restatement of it; the GPU file asserts the device plan agrees) leaves on raw_x3 is emulated at <= bar / 4"""
    shape = RESCALE[name][0]
    stages, fused = plan(rescaled_sd(name), config(shape))
    err = emulated_error(name)
    print(f"{name}: windows 2^{[round(math.log2(s['window']), 1) for s in stages[1:]]}, fused {fused}, emulated raw_x3 {err:.2e}, bar {bar(base_case(shape)[3]):.2e}")
    if name in KEEPS_FUSED:
        assert fused, name
    if fused:
        assert err <= bar(base_case(shape)[3]) / 4, (name, err)


@pytest.mark.parametrize("name", list(HEAVY))
def test_heavy_tailed_seed_leaves_something_to_measure(name):
    """the project's practice: a seed under which the logits collapse is changed.  float64 oracle on the four clips: the logits' ptp stays above
    1e-2, the float32 restatement within a tenth of the bars; and where the guard leaves the model on raw_x3 the emulator is at <= bar / 4"""
    cfg, _, pcm, _, _ = base_case(MAIN)
    sd = heavy_frontend_sd(name)
    f64, _, l64 = raw_oracle.forward(pcm, sd, cfg, dtype=np.float64)
    f32, _, l32 = raw_oracle.forward(pcm, sd, cfg)
    stages, fused = plan(sd, cfg)
    with np.errstate(invalid="ignore"):
        err = float(np.nan_to_num(np.abs(emulate(pcm, sd, cfg) - f64), nan=np.inf).max())
    print(f"heavy-tailed {name}: logit ptp {float(np.ptp(l64)):.3e}, |frontend|max {float(np.abs(f64).max()):.3g}, float32 restatement {float(np.abs(f32 - f64).max()):.2e} / "
          f"{float(np.abs(l32 - l64).max()):.2e}, windows 2^{[round(math.log2(s['window']), 1) for s in stages[1:]]}, fused {fused}, emulated raw_x3 {err:.2e}, bar {bar(f64):.2e}")
    assert np.ptp(l64) > 1e-2, (name, np.ptp(l64))
    assert np.abs(f32 - f64).max() <= bar(f64) / 10 and np.abs(l32 - l64).max() <= LOGIT_ATOL / 10, name
    if fused:
        assert err <= bar(f64) / 4, (name, err)
