#!/usr/bin/env python3
"""Dump every head's launch plan and the hashes of what it computes, under every arithmetic and every plan knob.

The planner (csrc/nww_plan.hip) turns a head's weights into an ordered list of named steps.  A change to the planner that is meant
to leave behaviour alone is right exactly when that list and the bits it computes are unchanged, so: run this before and after,
and `cmp` the two files.  profiles/plan_dump.txt holds the last recorded dump (written with --stream).

    python tools/dump_plans.py --stream --out profiles/plan_dump.txt

For each row of tests/test_gpu_parity.py:_F64_HEADS and of EXTRA_HEADS and each conv_arith in (default, f32, bf16x6, bf16x9) a child prints
describe_plan() and one SHA-256 over the float32 logits and embedding bytes of synth_features at B = 1, 3 and 64; a combination
the library refuses prints the refusal; the raw-PCM heads (PCM_HEADS) follow on PCM.  --stream adds the CRNN head scoring a few
streaming hops (the ring / sequence captures of the conv stem run only there).  The knobs are read once per process, so every
setting is a fresh child, one after another, each under its own time limit; the first child that fails ends the run.

The dump is written compactly, to stay a file one can commit and diff: every distinct step name once (`s<n> name`), every
distinct plan once as its step numbers in launch order (`p<n> ...`), then one line per row: setting | row | plan | hash.  A row
of a knob's child that repeats the default child's row is left out.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KNOBS = ("NWW_TRUNK", "NWW_CONV_MFMA", "NWW_CONV3_X3", "NWW_GEMM_X3", "NWW_LIN_X3", "NWW_FFN_FUSED", "NWW_ATTN_FUSED",
         "NWW_MERGE_FUSED", "NWW_QN_FUSED", "NWW_RAW_FUSED", "NWW_CONV2S_X3", "NWW_RNN_IH_FUSED", "NWW_MHA_MFMA", "NWW_BC_FRONT", "NWW_BC_CHAIN",
         "NWW_TAIL")
SETTINGS = [()] + [((k, "0"),) for k in KNOBS] + [(("NWW_GEMM_X3", "2"),), (("NWW_BC_FRONT", "2"),)]
ARITHS = ("default", "f32", "bf16x6", "bf16x9")
BATCHES = (1, 3, 64)
CHILD_SECONDS = 600
# feature-path rows beside _F64_HEADS: the bi-LSTM head has no oracle.heads._NETS entry, so that test's list cannot carry it
EXTRA_HEADS = (("rnn", (101, 64), {}, "rnn"), ("rnn", (16, 96), {}, "rnn-16x96"))
# the raw-PCM heads: (head, what the backbone sees of a clip under the default frontend, the clip's length in samples)
PCM_HEADS = (("e2e_quartznet", (33, 128), 8193), ("e2e_cnn", (63, 64), 4000))


def _sha(arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def child(stream: bool) -> int:
    import numpy as np
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipModel, NwwError
    from nanowakeword_amd.synth import synth_features, synth_pcm, synth_state_dict
    from test_gpu_parity import _F64_HEADS, _F64_IDS

    feats = {}
    for head, shape, kw, rid in [(*r, i) for r, i in zip(_F64_HEADS, _F64_IDS)] + list(EXTRA_HEADS):
        cfg = HeadConfig(head, shape, **kw)
        sd = synth_state_dict(cfg)
        for B in BATCHES:
            if (B, tuple(shape)) not in feats:
                feats[(B, tuple(shape))] = synth_features(B, cfg.input_shape)
        for arith in ARITHS:
            print(f"--- {rid} {shape[0]}x{shape[1]} conv_arith={arith}")
            try:
                m = HipModel(cfg, FrontendConfig(n_mels=cfg.input_shape[1]), state_dict=sd, tables="builtin", conv_arith=arith)
            except NwwError as e:
                print(f"refused: {e}")
                continue
            print(m.describe_plan().rstrip("\n"))
            outs = [m.forward_features(feats[(B, tuple(shape))], return_embedding=True) for B in BATCHES]
            print("sha256 " + _sha(a for lg, _, emb in outs for a in (lg, emb)))
            m.close()
            sys.stdout.flush()
    # the raw-PCM heads: the raw frontend's plan (frontend:* lines) and the logits of the whole model
    for head, shape, n in PCM_HEADS:
        cfg = HeadConfig(head, shape)
        sd, pcm = synth_state_dict(cfg), synth_pcm("noise", 3, n)
        for arith in ARITHS:
            print(f"--- {head} {shape[0]}x{shape[1]} conv_arith={arith}")
            try:
                m = HipModel(cfg, FrontendConfig(), state_dict=sd, tables="builtin", conv_arith=arith)
            except NwwError as e:
                print(f"refused: {e}")
                continue
            print(m.describe_plan().rstrip("\n"))
            print("sha256 " + _sha((m.forward_pcm(pcm)[0], m.frontend(pcm))))
            m.close()
    if stream:
        # the CRNN stem's third stage reads the fused trunk's rings and writes the recurrent layers' sequence rows only on this path
        S, W, hop, n_hops = 3, 16000, 1280, 18
        for kw in ({}, {"crnn_cnn_channels": [16, 32, 64, 64]}):
            cfg = HeadConfig("crnn", (101, 64), **kw)
            print(f"--- stream crnn channels={kw.get('crnn_cnn_channels', 'default')} S={S} window={W} hop={hop}")
            m = HipModel(cfg, FrontendConfig(n_mels=64), state_dict=synth_state_dict(cfg), tables="builtin")
            print(m.describe_plan().rstrip("\n"))
            pcm = np.concatenate([synth_pcm("speechlike", 2, hop * n_hops), synth_pcm("noise", 1, hop * n_hops)])
            m.stream_open(S, W, hop)
            print("sha256 " + _sha(a for i in range(n_hops) for a in m.stream_push(np.ascontiguousarray(pcm[:, i * hop:(i + 1) * hop]))))
            m.stream_close()
            m.close()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="write the dump here (default: stdout)")
    ap.add_argument("--stream", action="store_true", help="add the CRNN streaming rows")
    ap.add_argument("--only", help="comma-separated settings to run, e.g. default,NWW_TRUNK=0 (default: all)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.stream)
    only = set(args.only.split(",")) if args.only else None
    steps, plans, table, default_rows = {}, {}, [], set()      # step name -> number, plan (step numbers) -> number, the row lines
    rc = 0
    for setting in SETTINGS:
        label = " ".join(f"{k}={v}" for k, v in setting) or "default"
        if only is not None and label not in only:
            continue
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(dict(setting))
        cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child"] + (["--stream"] if args.stream else [])
        print(f"[dump_plans] {label}", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        rows = r.stdout.split("--- ")[1:]
        if not setting:
            default_rows = set(rows)
        for row in rows:
            if setting and row in default_rows:                # a knob leaves most heads alone
                continue
            name, *lines = row.rstrip("\n").split("\n")
            if not lines or not lines[-1].startswith("sha256 "):                # a refusal, or a child that ended early: as printed
                table.append(f"{label} | {name} | " + " / ".join(lines))
                continue
            plan = " ".join(str(steps.setdefault(l, len(steps) + 1)) for l in lines[:-1])
            table.append(f"{label} | {name} | p{plans.setdefault(plan, len(plans) + 1)} | {lines[-1][7:]}")
        if r.returncode != 0:
            print(f"[dump_plans] child '{label}' exited {r.returncode}: stopping", file=sys.stderr)
            rc = 1
            break
    out = open(args.out, "w") if args.out else sys.stdout
    out.write("".join(f"s{n} {l}\n" for l, n in steps.items()) + "".join(f"p{n} {p}\n" for p, n in plans.items()) + "\n".join(table) + "\n")
    if args.out:
        out.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
