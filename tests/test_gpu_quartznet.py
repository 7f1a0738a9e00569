"""QuartzNet head on the HIP path (run with -m gpu): reference goldens, the PCM composite, ONNX / .pt ingestion through the session, the
launch plan at the reference defaults, every fallback, fused widths x clip lengths x kernel sizes against the float64 restatement, batch
invariance, an unclamped loud frame, the halo at both ends of a clip, the two halves of the K = 2 Cin operand, what nww_create refuses, and
a TCN and a Conformer case left as they were; widths whose second workgroup shares its blocks among the waves differently from the first,
projections from 512 and 288 channels, one outlier depthwise channel and dead BatchNorm channels beside the float32 path."""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict
from parity import GOLDEN, assert_pcm_logits_vs_reference, head_golden_names, load_head_goldens

pytestmark = pytest.mark.gpu

LOGIT_ATOL = 1e-4
EMB_RTOL = 1e-4
# qn_x3 takes any Cin (a multiple of 4) and Cout (a multiple of 32) up to 512 at run time; its compiled instances differ in the row tiles
# (T <= 32 / 64 / 128).  These widths reach every way it shares output blocks among its waves (1, 2, 3-4, 5-8 blocks, and two workgroups a clip)
FUSED_WIDTHS = (32, 64, 96, 128, 160, 256, 512)


@pytest.fixture(scope="module")
def golden():
    return load_head_goldens("heads_quartznet.npz")


def _model(cfg, sd=None, **kw):
    from nanowakeword_amd.session import HipModel
    return HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg) if sd is None else sd, **kw)


def _qn(shape, qc=None, **kw):
    return HeadConfig("quartznet", shape, **({} if qc is None else {"quartznet_config": qc}), **kw)


def _nblocks(cfg):
    return sum(r for _, _, r in cfg.quartznet_config)


def _head_plan(m):
    """the head's launches (the frontend runs for PCM input only; the sigmoid rides in the tail)"""
    return [l for l in m.describe_plan().strip().split("\n") if l.strip() and not l.startswith(("frontend:", "unary:sigmoid"))]


# ---- 1
@pytest.mark.parametrize("name", head_golden_names("heads_quartznet.npz"))
def test_features_vs_reference(golden, name):
    d, meta = golden
    cfg = HeadConfig(**meta[name])
    m = _model(cfg)
    assert m.feature_clamp == 0.0, m.describe_plan()
    feats = d[f"{name}/feats"]
    logits, probs, emb = m.forward_features(feats, return_embedding=True)
    ref, ref_e = d[f"{name}/logits_feat"].ravel(), d[f"{name}/emb_feat"]
    print(name, "max |dlogit| vs reference: %.2e" % np.abs(logits - ref).max(), "max |demb|: %.2e" % np.abs(emb - ref_e).max())
    assert np.abs(logits - ref).max() <= LOGIT_ATOL, (name, np.abs(logits - ref).max(), m.describe_plan())
    assert np.abs(emb - ref_e).max() <= EMB_RTOL * max(1.0, np.abs(ref_e).max()), (name, np.abs(emb - ref_e).max())
    assert np.abs(probs - oracle.sigmoid(ref)).max() <= 1e-5
    # ragged batches against the restatement
    sd = synth_state_dict(cfg)
    for B in (1, 3, 33, 70):
        fx = synth_features(B, cfg.input_shape, seed=B)
        lg, _ = m.forward_features(fx)
        lo = oracle.model_forward(fx, sd, cfg).ravel()
        assert np.abs(lg - lo).max() <= LOGIT_ATOL, (name, B, np.abs(lg - lo).max())
    m.close()


# ---- 2
def test_pcm_vs_reference(golden, golden_frontend):
    from nanowakeword_amd.session import HipModel
    d, meta = golden
    g = golden_frontend
    name = "quartznet_101x64"
    cfg = HeadConfig(**meta[name])
    sd = synth_state_dict(cfg)
    m = HipModel(cfg, FrontendConfig(), state_dict=sd, window=g["window"], mel_fb=g["fb64"])
    lp, pp, err, _ = assert_pcm_logits_vs_reference(m, cfg, sd, g, g["pcm"], d[f"{name}/logits_pcm"].ravel(), what=name)
    print("PCM composite: max |dlogit| vs reference %.2e" % err.max())
    assert np.abs(pp - oracle.sigmoid(lp)).max() <= 1e-6
    m.close()


# ---- 3
def test_onnx_and_pt_through_the_session(tmp_path):
    import torch
    from nanowakeword_amd.weights import infer_head_config, load_session, save_bundle, state_dict_from_pt
    e = dict(np.load(os.path.join(GOLDEN, "onnx", "expected_quartznet.npz"), allow_pickle=False))
    feats, want = e["quartznet/feats"], e["quartznet/probs"]
    s = load_session(os.path.join(GOLDEN, "onnx", "quartznet.onnx"))
    assert np.abs(s.run(None, {"input": feats})[0].reshape(-1) - want).max() <= 1e-5
    cfg = HeadConfig(**json.loads(str(e["meta_json"]))["quartznet"])
    pt = str(tmp_path / "quartznet.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg).items()}, pt)
    sd = state_dict_from_pt(pt)
    c = infer_head_config(sd, input_shape=cfg.input_shape)
    assert c == cfg
    bundle = str(tmp_path / "quartznet_pt.nww.npz")
    save_bundle(bundle, c, sd, mode="features")
    s2 = load_session(bundle)
    assert np.abs(s2.run(None, {"input": feats})[0].reshape(-1) - want).max() <= 1e-5


# ---- 4
@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_plan_at_reference_defaults(shape):
    """One qn_x3 launch per block - the last one also takes the time mean - and the tail: four launches."""
    cfg = _qn(shape)
    m = _model(cfg)
    plan = _head_plan(m)
    text = "\n".join(plan)
    assert m.feature_clamp == 0.0
    assert text.count("qn_x3:") == 3 and text.count("tail:") == 1, text
    for needle in ("gemm:", "lin_x3:", "dwconv1d", "add+relu", "mean:time\n", "unary:"):
        assert needle not in text, (needle, text)
    assert "(dw33+pw+bn+proj+relu)" in plan[0] and "(dw33+pw+bn+x+relu)" in plan[1] and "(dw39+pw+bn+proj+relu+mean:time)" in plan[2], text
    assert plan[3].startswith("tail:fc+classifier"), text
    assert len(plan) == 4, text
    m.close()


def _check(cfg, needles, batches=(1, 3, 33, 70), absent=(), sd=None, dtype=np.float64, count=None, **kw):
    """plan text holds every needle once per block (or `count` times) and none of `absent`; logits at LOGIT_ATOL and embeddings at EMB_RTOL
    against the restatement in `dtype` at each batch size -> worst |dlogit|"""
    sd = synth_state_dict(cfg) if sd is None else sd
    m = _model(cfg, sd, **kw)
    text = m.describe_plan()
    assert m.feature_clamp == 0.0, text
    for n in needles:
        assert text.count(n) == (_nblocks(cfg) if count is None else count), (n, text)
    for n in absent:
        assert n not in text, (n, text)
    worst = 0.0
    for B in batches:
        fx = synth_features(B, cfg.input_shape, seed=B)
        lg, _, emb = m.forward_features(fx, return_embedding=True)
        e_ref = oracle.head_forward(fx, sd, cfg, dtype=dtype)
        ref = oracle.classify(e_ref, sd, cfg, dtype=dtype).ravel()
        assert np.isfinite(lg).all()
        worst = max(worst, float(np.abs(lg - ref).max()))
        assert np.abs(lg - ref).max() <= LOGIT_ATOL, (B, float(np.abs(lg - ref).max()), text)
        assert np.abs(emb - e_ref).max() <= EMB_RTOL * max(1.0, np.abs(e_ref).max()), (B, float(np.abs(emb - e_ref).max()))
    m.close()
    return worst


GENERIC = ("dwconv1d:", "pointwise_conv+bn", "add+relu:")


# ---- 5
def test_fallback_width_without_an_instance():
    cfg = _qn((16, 96), [[48, 11, 1], [80, 13, 2]], embedding_dim=32)
    worst = _check(cfg, GENERIC, absent=("qn_x3:",))
    print("widths 48 / 80 (generic launches) max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("qc,fused,mean_launch", [([[64, 11, 1], [80, 11, 1]], 1, 1), ([[80, 11, 1], [96, 13, 1]], 1, 0)], ids=["fused_then_generic", "generic_then_fused"])
def test_fallback_mixed_blocks(qc, fused, mean_launch):
    """Each block chooses on its own: a block the fused kernel takes in front of one it does not (Cout = 80), and the other way round; the
    time mean rides in the last block's launch only when that block is fused."""
    cfg = _qn((33, 64), qc, embedding_dim=32)
    m = _model(cfg)
    plan = _head_plan(m)
    text = "\n".join(plan)
    assert text.count("qn_x3:") == fused and text.count("dwconv1d:") == 1 and text.count("add+relu:") == 1, text
    assert sum(l.startswith("mean:time") for l in plan) == mean_launch and text.count("+mean:time") == 1 - mean_launch, text
    m.close()
    worst = _check(cfg, ())
    print(qc, "max |dlogit| vs float64: %.2e" % worst)


def test_fallback_even_kernel():
    cfg = _qn((33, 64), [[128, 8, 1], [128, 8, 1]], embedding_dim=32)
    worst = _check(cfg, GENERIC, absent=("qn_x3:",))
    print("even k (generic launches) max |dlogit| vs float64: %.2e" % worst)


def test_fallback_kernel_beyond_the_fused_range():
    worst = _check(_qn((64, 64), [[64, 41, 1], [64, 51, 1]], embedding_dim=32), GENERIC, absent=("qn_x3:",), batches=(1, 3, 33))
    print("k = 41 / 51 (generic launches) max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("T", [129, 200])
def test_fallback_long_clip(T):
    cfg = _qn((T, 64), [[64, 33, 1], [128, 39, 1]], embedding_dim=32)
    m = _model(cfg)
    assert sum(l.startswith("mean:time") for l in _head_plan(m)) == 1, m.describe_plan()
    m.close()
    worst = _check(cfg, GENERIC, absent=("qn_x3:",), batches=(1, 3, 33))
    print("T", T, "(generic launches) max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("arith", ["bf16x6", "bf16x9", "f32"])
@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_fallback_arithmetics(arith, shape):
    worst = _check(_qn(shape), GENERIC, absent=("qn_x3:",), batches=(1, 3, 33), conv_arith=arith)
    print(arith, shape, "max |dlogit| vs float64: %.2e" % worst)


def test_knob_off_falls_back():
    """NWW_QN_FUSED=0 (read once per process: a fresh interpreter): the generic launches, same result."""
    import subprocess
    import sys
    code = ("import numpy as np, oracle\n"
            "from nanowakeword_amd.config import FrontendConfig, HeadConfig\n"
            "from nanowakeword_amd.session import HipModel\n"
            "from nanowakeword_amd.synth import synth_features, synth_state_dict\n"
            "cfg = HeadConfig('quartznet', (101, 64)); sd = synth_state_dict(cfg)\n"
            "m = HipModel(cfg, FrontendConfig(), state_dict=sd); t = m.describe_plan()\n"
            "assert 'qn_x3:' not in t and t.count('dwconv1d:') == 3 and t.count('add+relu:') == 3 and t.count('residual_connector+bn') == 2 and 'mean:time' in t, t\n"
            "assert m.feature_clamp == 0.0\n"
            "x = synth_features(5, cfg.input_shape, seed=4)\n"
            "d = np.abs(m.forward_features(x)[0] - oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()).max()\n"
            "assert d <= 1e-4, d\nprint('NWW_QN_FUSED=0 max |dlogit| vs float64: %.2e' % d)\n")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    env["NWW_QN_FUSED"] = "0"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- 6
@pytest.mark.parametrize("k", [3, 33, 39])
@pytest.mark.parametrize("T", [1, 5, 31, 32, 33, 64, 65, 101, 128])
@pytest.mark.parametrize("W,blocks", [(W, b) for W in FUSED_WIDTHS for b in (1, 2)])
def test_fused_widths_lengths_and_kernels_vs_float64(W, blocks, T, k):
    """Every width class x clip lengths on both sides of the 32-row tiles and of the three instances x the smallest and the two default kernel
    sizes (k > T included).  F = 32: one block is a projected residual (an identity one at W = 32), the second block an identity residual
    reading what the first wrote; the last block always carries the time mean."""
    cfg = _qn((T, 32), [[W, k, blocks]], embedding_dim=32)
    worst = _check(cfg, ("qn_x3:",), absent=("dwconv1d:", "add+relu:", "mean:time\n"), batches=(1, 3, 33))
    print("W", W, "blocks", blocks, "T", T, "k", k, "max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("k", [3, 33, 39])
@pytest.mark.parametrize("T", [1, 5, 31, 32, 33, 64, 65, 101, 128])
@pytest.mark.parametrize("F,W", [(96, 160), (256, 128)])
def test_fused_projection_over_several_chunks_vs_float64(F, W, T, k):
    """A projected residual whose Cin spans more than one 64-channel chunk (96 = 64 + 32, 256 = 4 x 64) with Cout != Cin: the d and x columns
    of every chunk after the first sit at their own offsets in the packed K = 2 Cin operand, at every clip length and kernel size class."""
    cfg = _qn((T, F), [[W, k, 1]], embedding_dim=32)
    worst = _check(cfg, ("qn_x3:",), absent=("dwconv1d:", "add+relu:", "mean:time\n"), batches=(1, 3, 33))
    print("F", F, "W", W, "T", T, "k", k, "max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("F", [40, 64, 96, 12, 100])
def test_fused_feature_counts(F):
    """Block 0 at the feature counts of the three frontends and two that are not multiples of 32: the channel count is zero-padded inside the kernel."""
    worst = _check(_qn((33, F), [[64, 11, 1], [128, 13, 1]], embedding_dim=32), ("qn_x3:",), absent=("dwconv1d:",))
    print("F", F, "max |dlogit| vs float64: %.2e" % worst)


# W in 288 .. 480: the second workgroup of a clip (blockIdx.y == 1) holds 1, 2, 4, 5 or 7 output blocks and so shares them among its waves in
# another way (8, 4, 2, 1, 1 waves a block) than the first workgroup of the same launch, which holds 8
SPLIT_WIDTHS = (288, 320, 384, 416, 480)
EDGE_T = (5, 33, 65, 128)                                  # the three instances, T = 128 at the last row of the largest
EDGE_K = (3, 39)


@pytest.mark.parametrize("k", EDGE_K)
@pytest.mark.parametrize("T", EDGE_T)
@pytest.mark.parametrize("W", SPLIT_WIDTHS)
def test_fused_second_workgroup_in_another_wave_class_vs_float64(W, T, k):
    """Block 0 projects F = 32 into both workgroups; block 1 is an identity residual that reads x at channel offsets past 256 and carries the
    time mean, whose second workgroup writes 32 .. 224 channels."""
    cfg = _qn((T, 32), [[W, k, 2]], embedding_dim=32)
    worst = _check(cfg, ("qn_x3:",), absent=("dwconv1d:", "add+relu:", "mean:time\n"), batches=(1, 3, 33))
    print("W", W, "T", T, "k", k, "max |dlogit| vs float64: %.2e" % worst)


@pytest.mark.parametrize("k", EDGE_K)
@pytest.mark.parametrize("T", EDGE_T)
@pytest.mark.parametrize("W0,W1", [(512, 96), (288, 512)], ids=["512_to_96", "288_to_512"])
def test_fused_long_and_ragged_projections_vs_float64(W0, W1, T, k):
    """A projection down from Cin = 512 (eight 64-channel chunks, K = 1024), and one from Cin = 288 = 4 x 64 + 32 (a last chunk of 32 channels)
    into the two workgroups of Cout = 512."""
    cfg = _qn((T, 32), [[W0, k, 1], [W1, k, 1]], embedding_dim=32)
    worst = _check(cfg, ("qn_x3:",), absent=("dwconv1d:", "add+relu:", "mean:time\n"), batches=(1, 3, 33))
    print("W", W0, "->", W1, "T", T, "k", k, "max |dlogit| vs float64: %.2e" % worst)


# feature seeds picked on the CPU: the first of 1, 2, .. at which the three CPU-side conditions of the test hold (1 for all three variants)
OUTLIER_SEED = {"dw_outlier_identity": 1, "dw_outlier_projection": 1, "dead_bn_channels": 1}


@pytest.mark.parametrize("variant", sorted(OUTLIER_SEED))
def test_outlier_depthwise_channel_and_dead_batchnorm_channels(variant):
    """qn_x3 gives a row ONE power of two for both operands, sized by amax - the largest tap L1 norm over ALL channels - times the
    neighbourhood's |x|, and plan_quartznet takes ONE f16_wscale for the whole folded [W_pw' ; W_res'] matrix.  (a) one depthwise channel of
    the identity block x 2^12 moves every other channel's d columns 12 bits down binary16's range; (b) the same on a projection block, where
    the x columns go down too; (c) running_var = 1e-8 on one channel of a pointwise and of a projection BatchNorm: folded rows ~300 x their
    neighbours, a trained model's dead channels.  The suite's heavy-tailed contract, relative to max(1, |ref|max) on 24 clips: the default plan
    <= 2 x the float32 MFMA path's error + 2e-6, and <= 1e-4 - after the case is shown to matter and to be well-conditioned on the CPU."""
    cfg = _qn((33, 64), [[128, 11, 1], [128, 11, 1], [64, 13, 1]], embedding_dim=32)
    base = synth_state_dict(cfg)
    sd = {key: np.array(v, copy=True) for key, v in base.items()}
    if variant == "dead_bn_channels":
        sd["model.quartznet_blocks.0.batch_norm.running_var"][7] = np.float32(1e-8)
        sd["model.quartznet_blocks.2.residual_connector.1.running_var"][9] = np.float32(1e-8)
    else:
        blk = 1 if variant == "dw_outlier_identity" else 2
        sd[f"model.quartznet_blocks.{blk}.depthwise_conv.weight"][5] *= np.float32(2.0 ** 12)
    x = synth_features(24, cfg.input_shape, seed=OUTLIER_SEED[variant])
    ref = oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.isfinite(ref).all() and np.ptp(ref) > 1e-2, ref
    assert np.abs(ref - oracle.model_forward(x, base, cfg, dtype=np.float64).ravel()).max() > 100 * LOGIT_ATOL
    assert np.abs(oracle.model_forward(x, sd, cfg).ravel() - ref).max() / scale <= 0.1 * 1e-4
    rel = {}
    for arith, fused in (("f16x3", 3), ("f32", 0)):
        m = _model(cfg, sd, **({} if arith == "f16x3" else {"conv_arith": arith}))            # f16x3 is the default plan
        assert m.describe_plan().count("qn_x3:") == fused and m.feature_clamp == 0.0, (arith, m.describe_plan())
        lg, _ = m.forward_features(x)
        assert np.isfinite(lg).all(), (variant, arith, lg)
        rel[arith] = float(np.abs(lg.astype(np.float64) - ref).max()) / scale
        m.close()
    print(variant, "max |dlogit| / max(1, |ref|max) vs float64:", rel, "scale", scale)
    assert rel["f16x3"] <= 2.0 * rel["f32"] + 2e-6, (variant, rel)
    assert rel["f16x3"] <= 1e-4, (variant, rel)


# ---- 7
@pytest.mark.parametrize("shape,B", [((16, 96), 4096), ((101, 64), 2048)])
def test_batch_invariance(shape, B):
    cfg = _qn(shape)
    m = _model(cfg)
    assert m.describe_plan().count("qn_x3:") == 3
    x = synth_features(B, shape, seed=11)
    full, _ = m.forward_features(x)
    for i in (0, B - 1):
        alone, _ = m.forward_features(np.ascontiguousarray(x[i:i + 1]))
        assert alone[0] == full[i], (shape, i, alone[0], full[i])
    ref = oracle.model_forward(x[:8], synth_state_dict(cfg), cfg).ravel()
    assert np.abs(full[:8] - ref).max() <= LOGIT_ATOL
    m.close()


def test_batch_invariance_many_short_clips():
    """T = 5 with k = 9 > T, B = 4099: more clips than resident workgroups (each walks several clips) and a ragged end."""
    cfg = _qn((5, 32), [[64, 9, 2]], embedding_dim=32)
    m = _model(cfg)
    assert m.describe_plan().count("qn_x3:") == 2, m.describe_plan()
    B = 4099
    x = synth_features(B, cfg.input_shape, seed=11)
    full, _ = m.forward_features(x)
    for i in (0, 6, 1500, B - 1):
        alone, _ = m.forward_features(np.ascontiguousarray(x[i:i + 1]))
        assert alone[0] == full[i], (i, alone[0], full[i])
    ref = oracle.model_forward(x[:40], synth_state_dict(cfg), cfg, dtype=np.float64).ravel()
    assert np.abs(full[:40] - ref).max() <= LOGIT_ATOL
    m.close()


# ---- 8
LOUD_SEED = {(16, 96): 31, (101, 64): 31}


@pytest.mark.parametrize("shape", [(16, 96), (101, 64)])
def test_unclamped_loud_frame(shape):
    """Nothing clamps the features: one frame of one clip x 1e4 on the default weights stays finite and within LOGIT_ATOL max(1, |ref|) of
    float64.  The float32 restatement is asserted within a tenth of that first (the seed was picked on the CPU for that), so the kernels are
    judged on a well-conditioned case."""
    cfg = _qn(shape)
    sd = synth_state_dict(cfg)
    x = synth_features(6, cfg.input_shape, seed=LOUD_SEED[shape])
    x[1, 7] *= np.float32(1e4)
    ref = oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
    tol = LOGIT_ATOL * np.maximum(1.0, np.abs(ref))
    assert np.all(np.abs(oracle.model_forward(x, sd, cfg).ravel() - ref) <= 0.1 * tol)
    m = _model(cfg, sd)
    assert m.feature_clamp == 0.0 and m.describe_plan().count("qn_x3:") == 3, m.describe_plan()
    lg, _ = m.forward_features(x)
    assert np.isfinite(lg).all(), lg
    print("loud frame", shape, "max |dlogit| / max(1, |ref|) vs float64: %.2e" % float((np.abs(lg - ref) / np.maximum(1.0, np.abs(ref))).max()))
    assert np.all(np.abs(lg - ref) <= tol), (lg, ref)
    m.close()


# ---- 9
@pytest.mark.parametrize("shape,qc", [((101, 64), None), ((16, 96), None), ((5, 32), [[64, 9, 2]]), ((33, 64), [[64, 33, 1], [64, 39, 1]])],
                         ids=["101x64", "16x96", "5x32_k9", "33x64_k33_k39"])
def test_halo_at_both_ends(shape, qc):
    """A clip that is zero except its first and last frames, between two dense clips: its first and last outputs see the zero halo, not the
    clip's other end (a wrap) nor the neighbours' rows.  The dense neighbours keep their own results."""
    cfg = _qn(shape, qc, embedding_dim=32)
    sd = synth_state_dict(cfg)
    m = _model(cfg, sd)
    assert m.describe_plan().count("qn_x3:") == _nblocks(cfg), m.describe_plan()
    x = synth_features(3, shape, seed=9)
    edge = np.zeros(shape, np.float32)
    edge[0], edge[-1] = x[1, 0], x[1, -1]
    x[1] = edge
    lg, _, emb = m.forward_features(x, return_embedding=True)
    e_ref = oracle.head_forward(x, sd, cfg, dtype=np.float64)
    ref = oracle.classify(e_ref, sd, cfg, dtype=np.float64).ravel()
    print("halo", shape, "max |dlogit| vs float64: %.2e" % np.abs(lg - ref).max())
    assert np.abs(lg - ref).max() <= LOGIT_ATOL, (lg, ref)
    assert np.abs(emb - e_ref).max() <= EMB_RTOL * max(1.0, np.abs(e_ref).max())
    # both ends matter to the case: without its last frame the clip's logit moves by far more than the bar
    cut = x[1:2].copy()
    cut[0, -1] = 0
    assert abs(oracle.model_forward(cut, sd, cfg, dtype=np.float64).ravel()[0] - ref[1]) > 100 * LOGIT_ATOL
    alone, _ = m.forward_features(np.ascontiguousarray(x[1:2]))
    assert alone[0] == lg[1]
    m.close()


# ---- 10
def test_the_two_halves_of_the_contraction():
    """A projected-residual block with the projection zeroed against the same block with the pointwise conv zeroed: the two results differ
    by far more than the bar (asserted), so a kernel that swaps the d and x halves of its K = 2 Cin operand cannot pass both."""
    cfg = _qn((33, 64), [[128, 11, 1]], embedding_dim=32)
    base = synth_state_dict(cfg)
    p = "model.quartznet_blocks.0."
    no_proj, no_pw = dict(base), dict(base)
    no_proj[p + "residual_connector.0.weight"] = np.zeros_like(base[p + "residual_connector.0.weight"])
    no_pw[p + "pointwise_conv.weight"] = np.zeros_like(base[p + "pointwise_conv.weight"])
    x = synth_features(3, cfg.input_shape, seed=3)
    a, b = (oracle.model_forward(x, sd, cfg, dtype=np.float64) for sd in (no_proj, no_pw))
    assert np.abs(a - b).max() > 100 * LOGIT_ATOL, np.abs(a - b).max()
    for name, sd in (("projection zeroed", no_proj), ("pointwise zeroed", no_pw)):
        worst = _check(cfg, ("qn_x3:",), batches=(1, 3, 33), sd=sd)
        print(name, "max |dlogit| vs float64: %.2e" % worst)


# ---- 11
def test_create_refuses_what_headconfig_refuses():
    from nanowakeword_amd import _lib
    from nanowakeword_amd.session import HipModel
    with pytest.raises(ValueError, match="1..4"):
        _qn((16, 96), [[32, 3, 1]] * 5)
    cfg = _qn((16, 96), [[32, 3, 1]] * 4)
    cfg.quartznet_config = [[32, 3, 1]] * 5                             # past HeadConfig's own check: the C side refuses it too
    with pytest.raises(Exception, match=r"quartznet_config must have 1..4 \[channels, kernel, repetitions\] entries \(got 5\)"):
        HipModel(cfg, FrontendConfig())
    cfg.quartznet_config = [[32, 3, 1], [0, 3, 1]]
    with pytest.raises(Exception, match=r"quartznet_config\[1\] channels = 0 must be positive"):
        HipModel(cfg, FrontendConfig())
    cfg.quartznet_config = [[32, 0, 1]]
    with pytest.raises(Exception, match="kernel size must be >= 1"):
        HipModel(cfg, FrontendConfig())
    cfg.quartznet_config = [[32, 3, 0]]
    with pytest.raises(Exception, match="repetitions must be >= 1"):
        HipModel(cfg, FrontendConfig())
    cfg.quartznet_config = [[32, 3, 9], [32, 3, 8]]
    with pytest.raises(Exception, match="expands to 17 blocks; at most 16"):
        HipModel(cfg, FrontendConfig())
    # the codes: more than four entries and more than 16 blocks are NWW_ERR_UNSUPPORTED (6), a zero channel count NWW_ERR_INVALID (1)
    lib = _lib.load_library()
    for qc, code in (([[32, 3, 1]] * 5, 6), ([[32, 3, 9], [32, 3, 8]], 6), ([[0, 3, 1]], 1)):
        cfg.quartznet_config = qc
        c = _lib.make_config(cfg, FrontendConfig())
        h = ctypes.c_void_p()
        assert lib.nww_create(ctypes.byref(c), ctypes.byref(h)) == code and not h.value, (qc, code)


# ---- 12
def test_conformer_and_tcn_untouched(golden_heads):
    d, meta = golden_heads
    cfg = HeadConfig(**meta["conformer_101x64"])
    m = _model(cfg)
    text = m.describe_plan()
    assert text.count("attn_x3:") == cfg.n_blocks and text.count("ffn_x3:") == 2 * cfg.n_blocks and "qn_x3" not in text and "dwconv1d+bn+swish:" in text, text
    # heads.npz stores no features: its logits_feat are the reference's on synth_features(4, shape), as tests/test_gpu_parity.py feeds them
    logits, _ = m.forward_features(synth_features(4, cfg.input_shape))
    assert np.abs(logits - d["conformer_101x64/logits_feat"].ravel()).max() <= LOGIT_ATOL
    m.close()
    t, tmeta = load_head_goldens("heads_tcn.npz")
    cfg = HeadConfig(**tmeta["tcn_101x64"])
    m = _model(cfg)
    text = m.describe_plan()
    assert text.count("tcn_x3:") == 1 and "qn_x3" not in text and m.feature_clamp == 0.0, text
    logits, _ = m.forward_features(t["tcn_101x64/feats"])
    ref = t["tcn_101x64/logits_feat"].ravel()
    assert np.all(np.abs(logits - ref) <= LOGIT_ATOL * np.maximum(1.0, np.abs(ref))), (logits, ref)
    m.close()
