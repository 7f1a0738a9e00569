"""Bounded, seeded runs of the fuzzers and the small-call soak (tools/fuzz_frontend.py, tools/fuzz_heads.py,
tools/stress_small_calls.py) inside `pytest -m gpu`: the tools that found real bugs (an inline-asm MFMA hazard among them) now run
wherever the GPU suite runs.  About a minute together; the tools themselves take any case count and seed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

# picked for what its 30 draws cover, from a listing made without a GPU (fuzz_heads.draw_new_head + test_gpu_tcn.fused_plan): 14 Transformer
# and 16 TCN cases, all 16 on the fused kernel, 6 of them with a cone longer than 32 rows
NEW_HEADS_SEED = 18


def test_fuzz_frontend_bounded():
    import fuzz_frontend
    lines = []
    bad = fuzz_frontend.run(n_cases=14, seed=4, max_batch=40, log=lines.append)
    assert bad == 0, "\n".join(lines)


def test_fuzz_heads_bounded():
    import fuzz_heads
    lines = []
    worst, ran = fuzz_heads.run(n_cases=28, seed=4, log=lines.append)
    assert ran >= 14 and worst <= 1e-4, "\n".join(lines)


def test_fuzz_new_heads_bounded():
    """The Transformer and TCN kinds on a seed of their own (the default kinds' 28 cases above stay the cases they have always been):
    1e-4 against the restatements - absolute for the Transformer, relative to max(1, |logit|) for the TCN, which normalises nothing - and
    floors on what the seed's cases exercise (listed without a GPU when the seed was picked): both kinds, the fused TCN kernel, cones of
    more than one 32-row tile."""
    import fuzz_heads
    lines, stats = [], {}
    worst, ran = fuzz_heads.run(n_cases=30, seed=NEW_HEADS_SEED, kinds=("transformer", "tcn"), log=lines.append, stats=stats)
    text = "\n".join(lines + [str(stats)])
    assert worst <= 1e-4, text
    assert stats["ran_transformer"] >= 10 and stats["ran_tcn"] >= 10 and ran == stats["ran_transformer"] + stats["ran_tcn"], text
    assert stats["tcn_fused"] >= 8 and stats["tcn_fused_long_cone"] >= 3 and stats["refused"] <= 2, text


@pytest.mark.parametrize("head", ["cnn", "dnn", "crnn"])
def test_small_call_soak_bounded(head):
    """random B = 1..20 host-pointer calls (zero-copy staging, completion word) == the bulk kernels' logits, bit for bit"""
    import stress_small_calls
    lines = []
    bad = stress_small_calls.run(n_calls=2500, head=head, seed=4, log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    assert bad == 0, "\n".join(lines)
