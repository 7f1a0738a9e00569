#!/usr/bin/env python3
"""Frontend launch alone, launched back to back on one stream and timed with events: ms per launch of nww_frontend_dev (frames-major) for
B device-resident clips of N samples.  For A/B work run it once per library (NWW_LIB_PATH), alternating the builds.
usage (GPU box): python tools/fe_ab.py [B [N [n_mels [center]]]]      (defaults 4096 16000 64 1)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.session import HipModel
from nanowakeword_amd.synth import synth_pcm, synth_state_dict


def main():
    a = [int(x) for x in sys.argv[1:]] + [4096, 16000, 64, 1][len(sys.argv) - 1:]
    B, N, n_mels, center = a[0], a[1], a[2], bool(a[3])
    T = 1 + N // 160 if center else 1 + (N - 400) // 160
    cfg = HeadConfig("dnn", (T, n_mels))
    m = HipModel(cfg, FrontendConfig(n_mels=n_mels, center=center), state_dict=synth_state_dict(cfg))
    pcm = torch.from_numpy(synth_pcm("noise", 64, N, seed=1)).cuda().repeat((B + 63) // 64, 1)[:B].contiguous()
    out = torch.empty((B, T, n_mels), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()          # a stream of its own: the library runs a null stream's work on its private stream, outside the events
    s = st.cuda_stream
    torch.cuda.synchronize()
    for _ in range(50):
        m.frontend_dev(pcm.data_ptr(), B, N, out.data_ptr(), 1, s)
    torch.cuda.synchronize()
    res = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(300):
            m.frontend_dev(pcm.data_ptr(), B, N, out.data_ptr(), 1, s)
        e1.record(st)
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / 300)
    print(os.path.basename(os.environ.get("NWW_LIB_PATH", "default")), f"B={B} N={N} T={T} n_mels={n_mels} center={int(center)}", "ms/launch",
          " ".join(f"{x:.4f}" for x in res), "min %.4f med %.4f" % (min(res), float(np.median(res))), "sum", float(out.double().sum()), flush=True)
    m.close()


if __name__ == "__main__":
    main()
