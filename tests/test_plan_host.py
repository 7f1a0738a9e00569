"""The planner's value arithmetic (csrc/plan_host.h: the two-term binary16 scales, a layer's bound and typical magnitude, the range
guards on the mean and per consumer row, the load-time channel balance) on the CPU: tests/hostemu/plan_host_check.cpp, a stand-alone g++
program against that header alone, holds f16_scale / f16_wscale to the binary16 range, f16_layer_bound to sampled and sign-aligned
inputs, F16Range::ok / f16_rows_ok / f16_rows_weights_ok to a model with uniform channel gains and one whose gains spread by 2^24, and
balance_channels to a float32 forward of a tiny conv + ReLU + Linear net, bit for bit.  No GPU, and no library is loaded into Python."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "nanowakeword_amd", "csrc")


def test_plan_value_arithmetic(tmp_path):
    exe = str(tmp_path / "plan_host_check")
    # plain g++, no ROCm include path: the header takes nothing from HIP
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "hostemu", "plan_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]
