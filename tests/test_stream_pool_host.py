"""The per-stream state of a stream batch whose streams push, join and reset on their own (csrc/stream_pool.h: ring offsets, fill counts,
log-mel ring rows, the not-full / whole / primed partition of a call, its table, the aligned flag) on the CPU:
tests/hostemu/stream_pool_check.cpp, a stand-alone g++ program built with -fsanitize=address,undefined, checks it against brute force -
one sample counter and one list of frame origins per stream, the rings emulated cell by cell from the table alone - over random schedules
for windows 4800 / 16000, hops 640 / 1280 / 296 / the window itself and centre 0 / 1.  No GPU, and no library is loaded into Python."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")


def test_stream_pool_against_brute_force(tmp_path):
    exe = str(tmp_path / "stream_pool_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "hostemu", "stream_pool_check.cpp"), os.path.join(CSRC, "fe_tables.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]
