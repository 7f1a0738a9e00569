"""fc1 on the two-row-tile ("ping-pong") instance of gemm_x3_kernel (run with -m gpu): the CNN head on (101, 64), K = 12 800 in 16 split-K
chunks of 25 k-tiles, through the PCM entry point (the fused trunk writes fc1's operand as tiles).  The logits must equal, bit for bit,
those of the one-tile-per-workgroup kernel (NWW_GEMM_PP=0) at batch sizes where half 1 of a workgroup has no row tile (65), where waves
of a tile lie beyond M (129), where an odd tile count leaves the last workgroup half empty (300) and where every tile is full (512);
a clip's logit must not depend on its batch; and the oracle's tolerance holds.  Knobs are read once per process: one child per setting."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_pcm, synth_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (65, 129, 300, 512)

_SCRIPT = r'''
import sys
import numpy as np
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.session import HipModel, torchaudio_tables
from nanowakeword_amd.synth import synth_pcm, synth_state_dict
fe = FrontendConfig()
cfg = HeadConfig("cnn", (101, 64))
window, fb = torchaudio_tables(fe)
m = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg), window=window, mel_fb=fb)
assert "gemm:fc1 [f16x3]" in m.describe_plan(), m.describe_plan()
pcm = synth_pcm("noise", 512, 16000)
out = {}
for B in (65, 129, 300, 512):
    out["b%d" % B] = m.forward_pcm(pcm[:B])[0]
out["alone8"] = m.forward_pcm(pcm[:8])[0]
m.close()
np.savez(sys.argv[1], **out)
'''


def _run(tmp, name, env):
    path = os.path.join(tmp, name + ".npz")
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + sys.path), **env)
    r = subprocess.run([sys.executable, "-c", _SCRIPT, path], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-4000:])
    return dict(np.load(path))


@pytest.fixture(scope="module")
def logits(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fc1_pp"))
    return {"pp": _run(tmp, "pp", {}), "old": _run(tmp, "old", {"NWW_GEMM_PP": "0"})}


@pytest.mark.parametrize("B", BATCHES)
def test_new_kernel_against_old(logits, B):
    new, old = logits["pp"]["b%d" % B], logits["old"]["b%d" % B]
    assert new.shape == (B,) and np.all(np.isfinite(new))
    assert np.array_equal(new, old), (B, int((new != old).sum()), float(np.abs(new - old).max()))


def test_batch_invariance(logits):
    assert np.array_equal(logits["pp"]["b300"][:8], logits["pp"]["alone8"])      # alone: gemm_x3_chain_kernel


def test_oracle(logits):
    from nanowakeword_amd.session import torchaudio_tables
    fe = FrontendConfig()
    cfg = HeadConfig("cnn", (101, 64))
    window, fb = torchaudio_tables(fe)
    pcm = synth_pcm("noise", 512, 16000)[:8]
    lm = oracle.frontend_logmel(pcm, window, fb).transpose(0, 2, 1)
    ref = oracle.model_forward(np.ascontiguousarray(lm), synth_state_dict(cfg), cfg).ravel()
    err = float(np.abs(logits["pp"]["b129"][:8] - ref).max())
    print("fc1 ping-pong, B = 129, first 8 clips: max|dlogit| vs oracle = %.2e" % err)
    assert err <= 1e-4, err
