"""The window / hop arithmetic of streaming and recording scoring (csrc/stream_plan.h: which frames a hop invalidates, which pooled
rows are kept, how the recomputed rows are cut into at most four strips) on the CPU: tests/hostemu/stream_plan_check.cpp, a stand-alone
g++ program, checks nww_plan_hop against brute force over sample spans and receptive fields for n_fft 400, hop_length 160, centre 0 / 1,
windows 4800 / 16000 / 24000 and every hop that is a multiple of 8 samples up to the window, under a predicate that accepts every strip
and one that accepts at most 5 pooled rows.  No GPU, and no library is loaded into Python."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")


def test_plan_hop_against_brute_force(tmp_path):
    exe = str(tmp_path / "stream_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostemu", "stream_plan_check.cpp"),
                    os.path.join(CSRC, "fe_tables.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]
