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


# likewise for the E-Branchformer and QuartzNet kinds, with newest_heads_coverage below standing in for the planner: the first of seeds
# 0, 1, .. whose 30 draws meet every floor of test_fuzz_newest_heads_bounded (the branch form of attn_x3 needs 144 / 4 at 64 < T <= 128 and
# is the rare one) - 13 E-Branchformer cases, all 13 with merge_x3 and 2 with the branch attn_x3; 17 QuartzNet cases, 7 entirely on qn_x3,
# 7 mixing fused and general blocks, 8 with a fused block wider than 256
NEWEST_HEADS_SEED = 50


def qn_x3_takes(T, cin, cout, k):
    """qn_x3_supported (qn_x3.hip) restated: the block goes to the fused kernel under the default arithmetic"""
    return 1 <= T <= 128 and 4 <= cin <= 512 and cin % 4 == 0 and 32 <= cout <= 512 and cout % 32 == 0 and k % 2 == 1 and 1 <= k <= 39


def merge_x3_takes(D):
    """merge_x3_supported (merge_x3.hip) restated"""
    return D in (32, 64, 96, 128, 144, 192, 256)


def branch_attn_x3_takes(T, D, n_head):
    """attn_x3_supported (attn_x3.hip) restated: the attention branch is one launch"""
    return D == 144 and n_head == 4 and 64 < T <= 128


def newest_heads_coverage(cfgs):
    """what a list of drawn E-Branchformer / QuartzNet configurations would count in fuzz_heads.run's stats if none were refused (used
    without a GPU to pick NEWEST_HEADS_SEED; the test asserts the floors on the stats the run itself takes from describe_plan())"""
    from nanowakeword_amd.config import quartznet_blocks
    c = dict.fromkeys(("ran_e_branchformer", "ran_quartznet", "qn_all_fused", "qn_mixed", "qn_wide", "eb_merge_x3", "eb_branch_attn"), 0)
    for cfg in cfgs:
        T = cfg.input_shape[0]
        if cfg.model_type == "e_branchformer":
            c["ran_e_branchformer"] += 1
            c["eb_merge_x3"] += merge_x3_takes(cfg.branchformer_d_model)
            c["eb_branch_attn"] += branch_attn_x3_takes(T, cfg.branchformer_d_model, cfg.branchformer_n_head)
        elif cfg.model_type == "quartznet":
            blocks = quartznet_blocks(cfg)
            fused = [qn_x3_takes(T, cin, cout, k) for cin, cout, k in blocks]
            c["ran_quartznet"] += 1
            c["qn_all_fused"] += all(fused)
            c["qn_mixed"] += any(fused) and not all(fused)
            c["qn_wide"] += any(f and b[1] > 256 for f, b in zip(fused, blocks))
    return c


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


def test_fuzz_newest_heads_bounded():
    """The E-Branchformer and QuartzNet kinds on a seed of their own: 1e-4 against the restatements - absolute for the E-Branchformer,
    relative to max(1, |logit|) for QuartzNet, which only a folded BatchNorm normalises - and floors on what the seed's 30 cases exercise,
    read from describe_plan() by the run: both kinds, QuartzNet stacks entirely on qn_x3, stacks that mix fused and general blocks, fused
    blocks of more than 256 output channels (two workgroups a clip), merge_x3, and the branch form of attn_x3."""
    import fuzz_heads
    lines, stats = [], {}
    worst, ran = fuzz_heads.run(n_cases=30, seed=NEWEST_HEADS_SEED, kinds=("e_branchformer", "quartznet"), log=lines.append, stats=stats)
    text = "\n".join(lines + [str(stats)])
    assert worst <= 1e-4, text
    assert stats["ran_e_branchformer"] >= 10 and stats["ran_quartznet"] >= 10 and ran == stats["ran_e_branchformer"] + stats["ran_quartznet"], text
    assert stats["qn_all_fused"] >= 6 and stats["qn_mixed"] >= 3 and stats["qn_wide"] >= 3, text
    assert stats["eb_merge_x3"] >= 6 and stats["eb_branch_attn"] >= 2 and stats["refused"] <= 2, text


@pytest.mark.parametrize("head", ["cnn", "dnn", "crnn"])
def test_small_call_soak_bounded(head):
    """random B = 1..20 host-pointer calls (zero-copy staging, completion word) == the bulk kernels' logits, bit for bit"""
    import stress_small_calls
    lines = []
    bad = stress_small_calls.run(n_calls=2500, head=head, seed=4, log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    assert bad == 0, "\n".join(lines)
