#!/usr/bin/env python3
"""Random head shapes against the oracle (features in, logits out): a wider net than the parametrised GPU tests for the
shape-dependent kernel choices (lin_x3 / ffn_x3 / mha_mfma widths and tails, conv3_x3 fits / strips / k-split passes, padded recurrent
widths, BcResNet strips, trunk strips).  Kinds "transformer", "tcn", "e_branchformer" and "quartznet" are not in the default set: name
them.  A TCN or QuartzNet case is scored relative to max(1, |logit|) - nothing, or only a folded BatchNorm, normalises those heads - and each
logs which fused kernels planned.
usage: python tools/fuzz_heads.py [n_cases] [seed] [kinds, comma-separated] [act_dtype]   (needs an MI355X)
With act_dtype = f16 / bf16 (BcResNet only) the pass mark is 3e-2 / 2e-1 instead of 1e-4: on random features and planes of a few pixels
the 16-bit modes are noisier than on log-mel clips (round 4: worst of 80 / 60 cases 1.7e-2 / 9.5e-2; float32 storage 3.6e-5 of 250)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.session import HipModel
from nanowakeword_amd.synth import synth_features, synth_state_dict


def draw_new_head(kind, rng, act):
    """a HeadConfig of kind "transformer" / "tcn" / "e_branchformer" / "quartznet" from rng (no GPU needed: a seed's cases can be listed
    beforehand)"""
    if kind == "e_branchformer":
        # every merge_x3 width with 2, 4 or 8 heads ((144, 4) four times: the one shape whose attention branch is one attn_x3 launch, for
        # 64 < T <= 128); (48, 4) and (80, 4) have no merge_x3 / ffn_x3 instance and run the general launches
        pairs = [(d, nh) for d in (32, 64, 96, 128, 144, 192, 256) for nh in (2, 4, 8)] + [(144, 4)] * 3 + [(48, 4), (80, 4)]
        d, nh = pairs[rng.integers(0, len(pairs))]
        return HeadConfig("e_branchformer", (int(rng.integers(1, 201)), int(rng.choice([32, 40, 64]))), embedding_dim=16, activation=act,
                          branchformer_d_model=d, branchformer_n_head=nh, n_blocks=int(rng.integers(1, 4)))
    if kind == "quartznet":
        # 1 .. 4 entries of 1 .. 3 repetitions (12 blocks at most, inside the 16 the head takes).  Widths: multiples of 32 up to 512, and about
        # one in six 48 or 80 (no qn_x3 instance: that block alone goes to the general launches); k odd 3 .. 39, and about one in eight even or
        # 41 (general launches too); T > 128 sends every block there
        qc = []
        for _ in range(int(rng.integers(1, 5))):
            w = int(rng.choice([48, 80])) if rng.integers(0, 6) == 0 else 32 * int(rng.integers(1, 17))
            k = int(rng.choice([4, 8, 12, 41])) if rng.integers(0, 8) == 0 else 2 * int(rng.integers(1, 20)) + 1
            qc.append([w, k, int(rng.integers(1, 4))])
        return HeadConfig("quartznet", (int(rng.integers(1, 161)), int(rng.choice([12, 32, 40, 64, 96, 100]))), embedding_dim=16, activation=act,
                          quartznet_config=qc)
    if kind == "transformer":
        # every width with a post-norm ffn_x3 and head dims of mha_h2's exact-subtraction form; (48, 4) and (144, 8) fall back (no fused
        # feed-forward / head dim 18); T > 128: mha_core around the fused rest
        d, nh = [(32, 4), (32, 8), (64, 4), (64, 16), (96, 4), (128, 4), (128, 4), (128, 8), (144, 4), (192, 4), (256, 4), (256, 8), (48, 4), (144, 8)][rng.integers(0, 14)]
        return HeadConfig("transformer", (int(rng.integers(1, 201)), int(rng.choice([32, 40, 64]))), embedding_dim=16, activation=act,
                          transformer_d_model=d, transformer_n_head=nh, n_blocks=int(rng.integers(1, 4)))
    # 1 .. 4 levels of multiples of 32 (two draws in three stay at <= 128: the instance whose cone may span three 32-row tiles), k 2 .. 6
    top = 4 if rng.integers(0, 3) else 8
    chans = [32 * int(rng.integers(1, top + 1)) for _ in range(int(rng.integers(1, 5)))]
    return HeadConfig("tcn", (int(rng.integers(1, 121)), int(rng.choice([12, 32, 40, 41, 64, 96, 200]))), embedding_dim=16, activation=act,
                      tcn_channels=chans, tcn_kernel_size=int(rng.integers(2, 7)))


def run(n_cases=40, seed=0, log=print, kinds=("conformer", "crnn", "bcresnet", "cnn", "e2e_dnn", "dnn", "gru"), act_dtype=None, tol=1e-4, stats=None):
    """-> (worst |dlogit|, cases that ran); stats (a dict, optional) receives per-kind counts: ran, refused, for the TCN how many cases
    planned the fused kernel and how many of those kept a cone of more than 32 rows, and - all read from describe_plan() - for QuartzNet the
    cases with every block on qn_x3, with fused and general blocks mixed, and with a fused block of Cout > 256 (two workgroups a clip), for
    the E-Branchformer the cases with merge_x3 and with the branch form of attn_x3"""
    rng = np.random.default_rng(seed)
    worst, ran = 0.0, 0
    stats = {} if stats is None else stats
    for key in ("ran_transformer", "ran_tcn", "refused", "tcn_fused", "tcn_fused_long_cone", "ran_e_branchformer", "ran_quartznet", "qn_all_fused",
                "qn_mixed", "qn_wide", "eb_merge_x3", "eb_branch_attn"):
        stats[key] = 0
    for case in range(n_cases):
        kind = rng.choice(list(kinds))
        act = str(rng.choice(["relu", "gelu", "silu"]))
        if kind == "conformer":
            # (144, 4) three times: the default width, whose attention is one clip-resident kernel for 64 < T <= 128 (round 6); 192 / 256: the
            # fused kernels' wide instances; two blocks: the feed-forward launch with and without the Linears / the time sums folded into it
            d, nh = [(32, 2), (32, 8), (64, 4), (96, 4), (96, 2), (128, 4), (144, 4), (144, 4), (144, 4), (144, 8), (80, 4), (192, 4), (256, 4), (256, 8)][rng.integers(0, 14)]
            cfg = HeadConfig("conformer", (int(rng.integers(3, 140)), int(rng.choice([32, 40, 64]))), embedding_dim=16,
                             conformer_d_model=d, conformer_n_head=nh, activation=act, n_blocks=int(rng.choice([1, 1, 2])))
        elif kind == "crnn":
            # conv stacks the fused trunk takes and does not take, 64+ channel stages (k-split passes), clips up to 2.6 s (row strips), recurrent
            # widths between the register-resident ones (zero-padded instances) and above them
            chans = [[16, 32, 32], [16, 32, 32], [16, 32, 64], [16, 32, 64, 64], [32, 64], [32, 32, 64], [16, 32, 96, 32], [8, 16], [16, 32]][rng.integers(0, 9)]
            cfg = HeadConfig("crnn", (int(rng.integers(16, 120) if rng.integers(0, 4) else rng.integers(120, 260)), int(rng.choice([32, 40, 64, 96]))), embedding_dim=16, activation=act,
                             crnn_rnn_type=str(rng.choice(["gru", "lstm"])), layer_dim=int(rng.choice([20, 32, 48, 64, 96, 100, 128, 160])), crnn_cnn_channels=chans)
        elif kind == "bcresnet":
            cfg = HeadConfig("bcresnet", (int(rng.integers(16, 110)), int(rng.choice([32, 40, 64]))), embedding_dim=16, activation=act)
        elif kind == "cnn":
            cfg = HeadConfig("cnn", (int(rng.integers(8, 120)), int(rng.choice([32, 40, 64, 96]))), embedding_dim=16, activation=act)
        elif kind == "dnn":                                 # any flattened size (K % 4 != 0 included), tiny to default widths
            cfg = HeadConfig("dnn", (int(rng.integers(4, 110)), int(rng.choice([32, 40, 41, 63, 64, 96]))), activation=act,
                             layer_dim=int(rng.choice([8, 20, 32, 128])), n_blocks=int(rng.integers(0, 3)), embedding_dim=int(rng.choice([8, 16, 64])))
        elif kind in ("transformer", "tcn", "e_branchformer", "quartznet"):
            cfg = draw_new_head(kind, rng, act)
        elif kind == "gru":
            cfg = HeadConfig("gru", (int(rng.integers(4, 110)), int(rng.choice([32, 40, 64, 96]))), embedding_dim=16, activation=act,
                             layer_dim=int(rng.choice([20, 32, 48, 64, 96, 100, 128, 160])), n_blocks=int(rng.integers(1, 3)))
        else:
            cfg = HeadConfig("e2e_dnn", (int(rng.choice([32, 40, 64])), int(rng.integers(32, 130))), embedding_dim=16, activation=act)
        B = int(rng.choice([1, 2, 5, 17, 33, 130, 300]))
        try:
            sd = synth_state_dict(cfg)
            m = HipModel(cfg, FrontendConfig(n_mels=min(cfg.input_shape[1], 128) if kind != "e2e_dnn" else cfg.input_shape[0]), state_dict=sd,
                         act_dtype=act_dtype if kind == "bcresnet" else None)
        except (NotImplementedError, ValueError) as e:
            log(f"case {case}: {kind} {cfg.input_shape} refused at create: {str(e)[:80]}")
            stats["refused"] += 1
            continue
        x = synth_features(B, cfg.input_shape, seed=case)
        lg, _ = m.forward_features(x)
        ref = oracle.model_forward(x, sd, cfg).ravel()
        err = float(np.abs(lg - ref).max())
        note = ""
        if kind == "transformer":
            plan = m.describe_plan()
            note = (f" d={cfg.transformer_d_model}/{cfg.transformer_n_head} blocks={cfg.n_blocks} "
                    f"{'mha_h2' if 'mha_h2:' in plan else 'mha_core' if 'mha_core:' in plan else 'mha_mfma'} {'ffn_x3' if 'ffn_x3:' in plan else 'ffn fallback'}")
            stats["ran_transformer"] += 1
        elif kind == "tcn":
            err = float((np.abs(lg - ref) / np.maximum(1.0, np.abs(ref))).max())
            fused, S = "tcn_x3:" in m.describe_plan(), min(cfg.input_shape[0], oracle.tcn_receptive_field(cfg))
            note = f" ch={cfg.tcn_channels} k={cfg.tcn_kernel_size} S={S} {'tcn_x3' if fused else 'fallback'} (relative)"
            stats["ran_tcn"] += 1
            stats["tcn_fused"] += fused
            stats["tcn_fused_long_cone"] += fused and S > 32
        elif kind == "e_branchformer":
            plan = m.describe_plan()
            merge, branch = "merge_x3:" in plan, "attn_x3:" in plan and "(ln+in_proj" in plan
            note = (f" d={cfg.branchformer_d_model}/{cfg.branchformer_n_head} blocks={cfg.n_blocks} {'merge_x3' if merge else 'merge fallback'} "
                    f"{'attn_x3' if branch else 'mha_h2' if 'mha_h2:' in plan else 'mha_core' if 'mha_core:' in plan else 'mha_mfma'}")
            stats["ran_e_branchformer"] += 1
            stats["eb_merge_x3"] += merge
            stats["eb_branch_attn"] += branch
        elif kind == "quartznet":
            err = float((np.abs(lg - ref) / np.maximum(1.0, np.abs(ref))).max())
            couts = [c for c, _, r in cfg.quartznet_config for _ in range(r)]
            fused = [int(l.split("model.quartznet_blocks.")[1].split()[0]) for l in m.describe_plan().split("\n") if l.startswith("qn_x3:")]
            note = f" config={cfg.quartznet_config} qn_x3 on {len(fused)} of {len(couts)} blocks (relative)"
            stats["ran_quartznet"] += 1
            stats["qn_all_fused"] += len(fused) == len(couts)
            stats["qn_mixed"] += 0 < len(fused) < len(couts)
            stats["qn_wide"] += any(couts[i] > 256 for i in fused)
        worst, ran = max(worst, err), ran + 1
        flag = "" if err <= tol else "   <-- FAIL"
        log(f"case {case}: {kind} {cfg.input_shape} B={B} act={act}{note} max|dlogit| {err:.2e}{flag}")
        m.close()
    return worst, ran


if __name__ == "__main__":
    ad = sys.argv[4] if len(sys.argv) > 4 else None
    tol = {"f16": 3e-2, "bf16": 2e-1}.get(ad, 1e-4)
    kw = {"kinds": tuple(sys.argv[3].split(","))} if len(sys.argv) > 3 and sys.argv[3] else {}
    worst, ran = run(int(sys.argv[1]) if len(sys.argv) > 1 else 40, int(sys.argv[2]) if len(sys.argv) > 2 else 0, act_dtype=ad, tol=tol, **kw)
    print("WORST", worst, "of", ran, "cases")
    sys.exit(0 if worst <= tol else 1)
