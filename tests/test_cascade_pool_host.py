"""Cascades on stream pools (nww_cascade_stream_push_some) on the CPU: the three declarations of include/nww.h, the open rule in numpy
(config.cascade_pool_open), and what the device's pool select takes from the table of a pool call - the ring offset of each scored
stream from the entry's own stream and position, and the two compacted lists of the open entries - in
tests/hostemu/pool_cascade_check.cpp, a stand-alone g++ program with its own main, built with -fsanitize=address,undefined, against rings
emulated cell by cell over random join / skip / reset schedules (windows 3200 / 4800, hops 320 / 296).  No GPU, and no library is
loaded into Python."""
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from nanowakeword_amd.config import cascade_open, cascade_pool_open

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")


def test_header_declares_the_pool_entry_points():
    hdr = open(os.path.join(ROOT, "include", "nww.h")).read()
    for name in ("nww_cascade_stream_push_some", "nww_cascade_stream_push_some_dev", "nww_cascade_stream_reset_some"):
        assert len(re.findall(r"^extern int %s\(nww_handle\* gate, nww_handle\* verifier, const int32_t\* idx, int32_t n[,)]" % name, hdr, re.M)) == 1, name
    # declared `extern`: the pinned count of declarations that start a line with their return type has not moved
    assert len(re.findall(r"^(?:int|int32_t|int64_t|void|float|const char\*)\s+nww_\w+\(", hdr, re.M)) == 48
    from nanowakeword_amd import _lib
    assert {"nww_cascade_stream_push_some", "nww_cascade_stream_push_some_dev", "nww_cascade_stream_reset_some"} <= set(_lib.SYMBOLS)
    # the 4.8d block no longer says that cascades need lock-step
    assert "nww_stream_push* / nww_cascade_stream_push* work as before" in hdr and "A cascade does not need lock-step" in hdr


def test_cascade_pool_open():
    p = np.array([0.0, 0.2, 0.5, 0.7, 1.0, np.nan, 0.3, 0.9], np.float32)
    scored = np.array([1, 1, 0, 1, 1, 1, 0, 0], bool)
    # threshold 0 (and below) opens exactly the scored streams: a stream that holds no window is never open
    for thr in (0.0, -1.0):
        assert np.array_equal(cascade_pool_open(p, scored, thr), scored)
    assert cascade_open(p, 0.0).all()                                    # (the dense rule alone would open them all)
    # a NaN probability opens - on a scored stream only
    assert cascade_pool_open(p, scored, 0.95).tolist() == [False, False, False, False, True, True, False, False]
    assert not cascade_pool_open(np.array([np.nan], np.float32), [False], 0.5).any()
    # a threshold above 1 closes all (but a NaN, which no comparison closes)
    assert cascade_pool_open(p, scored, 2.0).tolist() == [False] * 5 + [True, False, False]
    assert not cascade_pool_open(p[:5], scored[:5], 2.0).any()
    # equality with the threshold opens: the comparison is float(p) < thr in double precision
    thr = float(np.float32(0.7))
    assert cascade_pool_open(p, scored, thr).tolist() == [False, False, False, True, True, True, False, False]
    assert not cascade_pool_open(p, scored, float(np.nextafter(np.float64(thr), 1.0)))[3]
    assert cascade_pool_open(p, scored, 0.7)[3] == (float(np.float32(0.7)) >= 0.7)      # the float32 0.7 against the double 0.7
    out = cascade_pool_open(p, scored.astype(np.uint8), 0.5)
    assert out.dtype == bool and out.shape == p.shape


def test_pool_select_against_brute_force(tmp_path):
    exe = str(tmp_path / "pool_cascade_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "hostemu", "pool_cascade_check.cpp"), os.path.join(CSRC, "fe_tables.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]
