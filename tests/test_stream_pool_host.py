"""The one ring state of a stream batch (csrc/stream_pool.h: ring offsets, fill counts, log-mel ring rows, the not-full / whole / primed
partition of a pool call, its table, what a lock-step push reads and commits, alignment and who ends and restores it) on the CPU:
tests/hostemu/stream_pool_check.cpp, a stand-alone g++ program built with -fsanitize=address,undefined, checks it against brute force -
one sample counter and one list of frame origins per stream, the rings emulated cell by cell from what a call hands to the device alone -
over random schedules of pool pushes, resets, lock-step pushes (some failing) and whole-batch resets, with aligned stretches in which the
two kinds of push hand over to one another, for windows 4800 / 16000, hops 640 / 1280 / 296 / the window itself, centre 0 / 1, and pools
that do and do not keep frames.  No GPU, and no library is loaded into Python."""
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
