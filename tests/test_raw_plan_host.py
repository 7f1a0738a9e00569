"""What consecutive windows of a raw-PCM head share (csrc/raw_plan.h) on the CPU.  tests/hostemu/raw_plan_check.cpp, a stand-alone g++
program, checks nww_raw_edge_rows and nww_plan_hop_raw against a brute-force walk over receptive fields: depths 1-4, every window of
16..1100 samples plus 4000, 4096, 15999, 16000, 16001 and 32000, hops of one row, five rows, the largest sharing hop, the next one and
one that is no whole row; and the pool's row count for 1, 2 and 7 windows.  Then the float64 restatement of the frontend
(tests/raw_oracle.py, which e2e_cnn_oracle.py shares) on random PCM: every row the plan calls interior is the span's row w k + t to
1e-12, and the rows just outside - el - 1 and T - er - are not, so the plan is tight and not merely safe.  No GPU, and no library is
loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import raw_oracle
from conftest import ROOT
from nanowakeword_amd.config import HeadConfig, raw_frontend_depth, raw_frontend_frames
from nanowakeword_amd.synth import synth_pcm, synth_state_dict

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("raw_plan") / "raw_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostemu", "raw_plan_check.cpp"),
                    os.path.join(CSRC, "fe_tables.cpp")], check=True)
    return exe


def _plan(exe, depth, W, hop):
    T, k, el, er, shared = (int(v) for v in subprocess.run([exe, str(depth), str(W), str(hop)], capture_output=True, text=True, check=True).stdout.split())
    return T, k, el, er, bool(shared)


def test_plan_against_brute_force(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]


def test_the_issue_examples(checker):
    assert _plan(checker, 3, 16000, 1280) == (63, 5, 2, 2, True)
    assert _plan(checker, 3, 4096, 256) == (16, 1, 2, 1, True)
    assert _plan(checker, 3, 4000, 256)[:4] == (16, 1, 2, 2)
    assert _plan(checker, 2, 16000, 1280) == (250, 20, 2, 1, True)
    assert not _plan(checker, 3, 16000, 1000)[4] and not _plan(checker, 3, 4000, 1000)[4] and not _plan(checker, 3, 16, 8)[4]


@pytest.mark.parametrize("head,W,hop", [("e2e_quartznet", 4096, 256), ("e2e_quartznet", 4096, 1280), ("e2e_quartznet", 4000, 512),
                                        ("e2e_cnn", 4096, 64), ("e2e_cnn", 4096, 1280)])
def test_interior_rows_are_the_span_rows_in_float64(checker, head, W, hop):
    probe = HeadConfig(head, (1, 128 if head == "e2e_quartznet" else 64))
    cfg = HeadConfig(head, (raw_frontend_frames(probe, W), probe.input_shape[1]))
    T, k, el, er, shared = _plan(checker, raw_frontend_depth(cfg), W, hop)
    assert shared and T == cfg.input_shape[0] and T - er - k > el >= 1 and er >= 1
    sd = {key: np.asarray(v, np.float64) for key, v in synth_state_dict(cfg).items()}
    B = 3
    span = (B - 1) * hop + W
    assert raw_frontend_frames(cfg, span) == (B - 1) * k + T
    pcm = synth_pcm("loud", 1, span, seed=W + hop)
    pool = raw_oracle.raw_frontend(raw_oracle.pcm_to_float(pcm, np.float64), sd, cfg)[0].T          # [rows][C]
    wins = np.stack([pcm[0, w * hop:w * hop + W] for w in range(B)])
    rows = raw_oracle.raw_frontend(raw_oracle.pcm_to_float(wins, np.float64), sd, cfg).transpose(0, 2, 1)   # [B][T][C]
    assert pool.shape[0] == (B - 1) * k + T and rows.shape[1] == T and np.abs(pool).max() > 1e-3
    for w in range(B):
        d = np.abs(rows[w, el:T - er] - pool[w * k + el:w * k + T - er]).max()
        assert d <= 1e-12, (w, d)
    # the middle window's rows just outside the interior see its own zero padding where the span sees audio
    assert np.abs(rows[1, el - 1] - pool[k + el - 1]).max() > 1e-6
    assert np.abs(rows[1, T - er] - pool[k + T - er]).max() > 1e-6
