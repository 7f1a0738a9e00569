"""The fused conv trunk's start-up on the HIP path (run with -m gpu): a workgroup's FIRST item reaches the LDS planes from registers loaded at
kernel entry (the chunk path, trunk_b.hip) or through the general loader (shapes without the chunk path; trunk.hip's float32 instance), every
later item through the steady-state path.  Batches of B clips are three distinct clips repeated, so that on a full grid the same clip is some
workgroup's first item and another's second or third: each logit must be, bit for bit, that clip's own B = 1 logit (where every workgroup has
one item and the strips are cut differently), and within 1e-4 of oracle.model_forward.  cnn head, all through HipModel.forward_features:

  (24, 16), (101, 64) B = 600   two or three items per workgroup on 256 CUs; (101, 64) takes the cost-weighted split of the grid over its two
                                uneven strips (B >= 2 x grid)
  (24, 16) B = 257 / 5          one workgroup with a second item, the rest without (the guard of the second item's request) / the small-batch
                                strip counts
  (24, 18) B = 3 / 600          width not a multiple of four: no chunk path, the general loader stages every item
  conv_arith bf16x6 / f32       the three-term instances of the same body / trunk.hip's loader, at the first two cases ((24, 18) too for f32)
"""
import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict

pytestmark = pytest.mark.gpu
BAR = 1e-4
N_DISTINCT = 3


@pytest.fixture(scope="module")
def cases():
    """(shape, conv_arith) -> (model, the three clips, their B = 1 logits, their oracle logits); built once, read-only"""
    made, refs = {}, {}

    def get(shape, arith):
        if shape not in refs:
            cfg = HeadConfig("cnn", shape)
            sd = synth_state_dict(cfg)
            clips = synth_features(N_DISTINCT, shape, seed=21)
            refs[shape] = (cfg, sd, clips, oracle.model_forward(clips, sd, cfg).ravel())
        cfg, sd, clips, ref = refs[shape]
        if (shape, arith) not in made:
            from nanowakeword_amd.session import HipModel
            m = HipModel(cfg, FrontendConfig(), state_dict=sd, conv_arith=arith)
            alone = np.array([m.forward_features(clips[k:k + 1])[0][0] for k in range(N_DISTINCT)], np.float32)
            made[shape, arith] = (m, alone)
        m, alone = made[shape, arith]
        return m, clips, alone, ref
    yield get
    for m, _ in made.values():
        m.close()


def _trunk_step(m):
    lines = [l for l in m.describe_plan().splitlines() if "trunk_x3:" in l or "trunk:" in l]
    assert len(lines) == 1, m.describe_plan()
    return lines[0]


def _hold(cases, shape, arith, B):
    m, clips, alone, ref = cases(shape, arith)
    step = _trunk_step(m)
    if arith == "f32":
        assert "trunk_x3:" not in step, step
    else:
        assert "trunk_x3:" in step and ("[f16x3]" in step) == (arith is None), step
    pick = np.arange(B) % N_DISTINCT
    lg, _ = m.forward_features(clips[pick])
    err = float(np.abs(lg - ref[pick]).max())
    differ = int((lg.view(np.uint32) != alone[pick].view(np.uint32)).sum())
    print(f"cnn {shape} conv_arith={arith or 'default'} B={B}: {step.strip()}; {differ} of {B} logits differ from the clip's B = 1 logit; "
          f"max |dlogit| vs oracle {err:.2e} (B = 1: {float(np.abs(alone - ref).max()):.2e})")
    assert len(set(alone.view(np.uint32).tolist())) == N_DISTINCT, alone          # the clips are told apart
    assert differ == 0, (shape, arith, B, differ)
    assert err <= BAR and float(np.abs(alone - ref).max()) <= BAR, (shape, arith, B, err)


@pytest.mark.parametrize("arith", [None, "bf16x6", "f32"], ids=["default", "bf16x6", "f32"])
@pytest.mark.parametrize("shape", [(24, 16), (101, 64)], ids=["24x16", "101x64"])
def test_first_item_against_later_items(cases, shape, arith):
    _hold(cases, shape, arith, 600)


@pytest.mark.parametrize("B", [257, 5])
def test_batch_size_edges(cases, B):
    _hold(cases, (24, 16), None, B)


@pytest.mark.parametrize("arith", [None, "f32"], ids=["default", "f32"])
@pytest.mark.parametrize("B", [3, 600])
def test_width_without_the_chunk_path(cases, B, arith):
    _hold(cases, (24, 18), arith, B)
