#!/usr/bin/env python3
"""The program a kernel trace of recording scoring runs: `rocprofv3 --kernel-trace --stats -d DIR -o rec -- python tools/recording_trace.py
[head]` - 50 passes of 4096 windows (1 s, hop 80 ms) of one recording on the device, on the route NWW_REC_SHARED selects."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.session import HipModel
from nanowakeword_amd.synth import synth_pcm, synth_state_dict

head = sys.argv[1] if len(sys.argv) > 1 else "cnn"
W, hop, B = 16000, 1280, 4096
cfg = HeadConfig(head, (101, 64))
m = HipModel(cfg, FrontendConfig(), state_dict=synth_state_dict(cfg))
n = W + (B - 1) * hop
rec = torch.from_numpy(synth_pcm("speechlike", 1, n, seed=10)[0]).cuda()
lg = torch.empty(B, dtype=torch.float32, device="cuda:0")
s = torch.cuda.Stream()
print("route", m.recording_route(W, hop))
for _ in range(50):
    m.forward_recording_dev(rec.data_ptr(), n, W, hop, lg.data_ptr(), 0, B, s.cuda_stream)
torch.cuda.synchronize()
m.close()
