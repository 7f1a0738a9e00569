#!/usr/bin/env python3
"""Measure every BASELINE.json config on ONE MI355X (the multi-GPU ones at their per-GPU batch):
clips/s PCM->logit with PCM resident in HBM, per-launch times, max |dlogit| vs the oracle on a few clips.
Prints one JSON line per config.  (bench.py remains the contract benchmark for configs[1].)
--rnn [out]: the RNN head's fused / unfused input projection A/B (rnn_main) -> profiles/rnn_bench_configs.jsonl.
--recording [out]: recording scoring, shared-frame against strided route against pre-materialised windows (recording_main) ->
profiles/recording_bench_configs.jsonl.
--recording-raw [out] [--parent DIR]: the same workload for the raw-PCM heads plus a row of 1024 streams, shared rows against
NWW_REC_SHARED = NWW_STREAM_INC = 0 and against the package of a built checkout of the parent commit (recording_raw_main) ->
profiles/raw_recording_bench_configs.jsonl.
--cascade [out]: a gate + verifier cascade against the gate alone and the verifier alone (cascade_main) -> profiles/cascade_bench_configs.jsonl.
--stream-pool [out]: 1024 streams per tick, lock-step against push_some (all streams, a random half) against whole-window re-scoring
(stream_pool_main) -> profiles/stream_pool_bench_configs.jsonl.
--cascade-pool [out]: 1024 streams per tick through a gate + verifier pair, nww_cascade_stream_push_some_dev against push_some on both
models against the lock-step cascade (cascade_pool_main) -> profiles/cascade_pool_bench_configs.jsonl.
--bank [out]: several heads as one bank call (nww_bank_*: one frontend pass) against the same handles called one after the other, on
batches, a stream pool and a recording (bank_main) -> profiles/bank_bench_configs.jsonl.
--mix [out]: clips mixed on the device (nww_mix_*) alone and in front of the CNN head, against uploading the pre-mixed batch and against
the same chain in torch ops (mix_main) -> profiles/mix_bench_configs.jsonl.
--mix-rir [out]: the same clips through room impulse responses (nww_mix_rir_*) alone and in front of the CNN head, against the calls
without responses and against torch.fft.rfft / irfft plus the tail on the same card (mix_rir_main) -> profiles/mix_rir_bench_configs.jsonl.
--mix-rir-seg [out]: the same protocol at clips of 2 s on the segmented route (NWW_RIR_SEGMENTED), with --mix-rir's one-workgroup route in
the same session as the per-transform yardstick (mix_rir_seg_main) -> profiles/mix_rir_seg_bench_configs.jsonl.
--mix-pitch [out]: half of --mix's clips shifted in pitch (nww_mix_aug_*) alone and in front of the CNN head, against the calls without
a shift and against the same definition in torch ops on the same card (mix_pitch_main) -> profiles/mix_pitch_bench_configs.jsonl.
--resample [out]: recordings brought to 16 kHz mono int16 (nww_resample_dev) - 4 096 mono clips of 1 s at 22 050 Hz, and 16 stereo
recordings of 60 s at 48 kHz - against a device-to-device copy that moves the same bytes in the same run (resample_main) ->
profiles/resample_bench_configs.jsonl."""
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("NWW_BENCH_PACKAGE_ROOT") or ROOT)      # (the package of another checkout: --recording-raw --parent)


def raw_frontend_legs(torch, m, cfg, sd, pcm, pcm_h, logits, stream, steps):
    """The raw-PCM head's extra legs: the learned frontend alone (nww_frontend_dev), an outside yardstick that is not code under test - the
    same folded three-stage chain as torch.nn.functional.conv1d + ReLU in float32 on the same device tensors (MIOpen) - both alternating
    three times in this session, the ratio to the frontend's HBM and float32-FMA bounds, and the oracle leg on the tests' restatement."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import raw_oracle
    from nanowakeword_amd.config import raw_frontend_macs, raw_frontend_stages
    B, N = pcm_h.shape
    T, C = cfg.input_shape
    fe_out = torch.empty((B, T, C), dtype=torch.float32, device=pcm.device)
    ws, bs = [], []
    strides = [s for _, _, _, s in raw_frontend_stages(cfg)]
    for i in range(len(strides)):
        w, p = sd[f"model.frontend.conv_blocks.{3*i}.weight"].astype(np.float64), f"model.frontend.conv_blocks.{3*i+1}"
        al = sd[p + ".weight"].astype(np.float64) / np.sqrt(sd[p + ".running_var"].astype(np.float64) + 1e-5)
        ws.append(torch.from_numpy((w * al[:, None, None]).astype(np.float32)).to(pcm.device))
        bs.append(torch.from_numpy((sd[p + ".bias"] - sd[p + ".running_mean"] * al).astype(np.float32)).to(pcm.device))
    x = (pcm.to(torch.float32) / 32768.0).unsqueeze(1).contiguous()

    def ours():
        m.frontend_dev(pcm.data_ptr(), B, N, fe_out.data_ptr(), True, stream)

    # the generic plan in the same session: the knob is read once per process, and another conv_arith takes the very launches
    # NWW_RAW_FUSED=0 takes (one conv1d_strided per stage)
    from nanowakeword_amd.session import HipModel
    mg = HipModel(cfg, m.fe, device=0, state_dict=sd, conv_arith="f32")
    mg.reserve(B, N)
    ge_out = torch.empty_like(fe_out)

    def generic():
        mg.frontend_dev(pcm.data_ptr(), B, N, ge_out.data_ptr(), True, stream)

    def chain():
        h = x
        for i, (w, b) in enumerate(zip(ws, bs)):
            h = torch.relu(torch.nn.functional.conv1d(h, w, b, stride=strides[i], padding=w.shape[2] // 2))
        return h

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    runs = [(round(timed(ours), 4), round(timed(chain), 4), round(timed(generic), 4)) for _ in range(3)]
    ours_ms, chain_ms, generic_ms = (min(r[q] for r in runs) for q in range(3))
    fused_vs_generic = float((ge_out - fe_out).abs().max())
    generic_plan = [l for l in mg.describe_plan().split("\n") if l.startswith("frontend:")]
    mg.close()
    agree = float((chain().transpose(1, 2) - fe_out).abs().max())
    macs = raw_frontend_macs(cfg, N)                           # rows from the frame law at this clip length
    hbm_ms = B * (N * 2 + T * C * 4) / 8e12 * 1e3                # int16 PCM in, float32 rows out at 8 TB/s
    fma_ms = 2 * macs * B / 157.3e12 * 1e3                      # float32 vector FMA peak of the card
    ref = raw_oracle.forward(pcm_h[:8], sd, cfg)[2].ravel()
    t0 = time.perf_counter(); k = 0
    while time.perf_counter() - t0 < 3.0:
        raw_oracle.forward(pcm_h[:32], sd, cfg); k += 32
    return {"generic_frontend_plan": generic_plan, "generic_frontend_ms_alternating": [r[2] for r in runs], "generic_frontend_ms": generic_ms,
            "frontend_over_generic": round(ours_ms / generic_ms, 3), "max_abs_frontend_vs_generic": fused_vs_generic,
            "frontend_ms_alternating": [r[0] for r in runs], "torch_conv1d_chain_ms_alternating": [r[1] for r in runs],
            "frontend_plan": [l for l in m.describe_plan().split("\n") if l.startswith("frontend:")], "frontend_mmac_per_clip": round(macs / 1e6, 2),
            "frontend_ms": ours_ms, "torch_conv1d_chain_ms": chain_ms, "frontend_over_torch_chain": round(ours_ms / chain_ms, 3),
            "max_abs_frontend_vs_torch_chain": agree, "frontend_hbm_bound_ms": round(hbm_ms, 4), "frontend_f32_fma_bound_ms": round(fma_ms, 4),
            "frontend_over_hbm_bound": round(ours_ms / hbm_ms, 1), "frontend_over_f32_fma_bound": round(ours_ms / fma_ms, 1),
            "max_abs_dlogit_vs_oracle": float(np.abs(logits[:8].cpu().numpy() - ref).max()),
            "cpu_oracle_clips_per_s": round(k / (time.perf_counter() - t0), 1)}


def raw_cnn_backbone_legs(torch, m, cfg, sd, pcm, pcm_h, logits, stream, steps):
    """The raw-PCM CNN head's extra legs: the backbone alone (nww_forward_features_dev on the frontend's resident output) three ways,
    alternating three times in this session - the default plan, the generic plan (conv_arith = "f32" takes the very launches
    NWW_CONV2S_X3=0 takes for the backbone: conv2d_strided for every conv) and an outside yardstick that is not code under test, the same
    folded four-stage chain as torch.nn.functional.conv2d + the activation + the mean in float32 on the same device tensors (MIOpen) -,
    the MFMA time of the three-product work at peak, the HBM time of the bytes the layers move, and the oracle leg on the tests'
    restatement."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import e2e_cnn_oracle
    from nanowakeword_amd.config import RAW_CNN_LAYERS, raw_cnn_planes
    from nanowakeword_amd.session import HipModel
    B, N = pcm_h.shape
    T, C = cfg.input_shape
    fe_out = torch.empty((B, T, C), dtype=torch.float32, device=pcm.device)
    m.frontend_dev(pcm.data_ptr(), B, N, fe_out.data_ptr(), True, stream)
    torch.cuda.synchronize()
    image = fe_out.transpose(1, 2).unsqueeze(1).contiguous()                      # [B, 1, H, W], as the reference's backbone sees it
    ws, bs = [], []
    for i in range(1, 5):
        w, p = sd[f"model.backbone.conv{i}.0.weight"].astype(np.float64), f"model.backbone.conv{i}.1"
        al = sd[p + ".weight"].astype(np.float64) / np.sqrt(sd[p + ".running_var"].astype(np.float64) + 1e-5)
        ws.append(torch.from_numpy((w * al[:, None, None, None]).astype(np.float32)).to(pcm.device))
        bs.append(torch.from_numpy((sd[p + ".bias"] - sd[p + ".running_mean"] * al).astype(np.float32)).to(pcm.device))
    act = {"relu": torch.relu, "gelu": torch.nn.functional.gelu, "silu": torch.nn.functional.silu}[cfg.activation]
    lg_def, lg_gen = torch.empty(B, dtype=torch.float32, device=pcm.device), torch.empty(B, dtype=torch.float32, device=pcm.device)
    mg = HipModel(cfg, m.fe, device=0, state_dict=sd, conv_arith="f32")
    mg.reserve(B, N)

    def ours():
        m.forward_features_dev(fe_out.data_ptr(), B, lg_def.data_ptr(), 0, stream)

    def generic():
        mg.forward_features_dev(fe_out.data_ptr(), B, lg_gen.data_ptr(), 0, stream)

    def chain():
        h = image
        for (w, b), (_, _, sh, sw) in zip(zip(ws, bs), RAW_CNN_LAYERS):
            h = act(torch.nn.functional.conv2d(h, w, b, stride=(sh, sw), padding=1))
        return h.mean(dim=(2, 3))

    def timed(fn, k):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3
    runs = [(round(timed(ours, steps), 4), round(timed(chain, steps), 4), round(timed(generic, max(2, steps // 10)), 4)) for _ in range(3)]
    ours_ms, chain_ms, generic_ms = (min(r[q] for r in runs) for q in range(3))
    # the generic plan's per-launch times (conv1's cost as a launch of its own is the same launch in both plans)
    mg.set_profiling(True)
    for _ in range(3):
        generic()
    torch.cuda.synchronize()
    gprof = {n: round(ms / max(c, 1), 4) for n, ms, c in mg.get_profile() if c > 0}
    generic_plan = [l for l in mg.describe_plan().split("\n") if l.startswith(("conv2d_strided:", "conv2s_x3:", "mean:"))]
    mg.close()
    planes = raw_cnn_planes(cfg)
    macs3 = sum(9 * cin * co * h * w for (cin, co, _, _), (h, w) in list(zip(RAW_CNN_LAYERS, planes[1:]))[1:])      # conv2 .. conv4
    mfma_ms = 3 * 2 * macs3 * B / 2.5e15 * 1e3                  # three products per operand pair at the card's 2.5 PFLOP/s (binary16, dense)
    moved = planes[0][0] * planes[0][1] + sum(2 * co * h * w for (_, co, _, _), (h, w) in zip(RAW_CNN_LAYERS, planes[1:]))
    hbm_ms = B * moved * 4 / 8e12 * 1e3                          # every plane written once and read once (conv4's by the mean), float32, at 8 TB/s
    ref = e2e_cnn_oracle.forward(pcm_h[:8], sd, cfg)[2].ravel()
    t0 = time.perf_counter(); k = 0
    while time.perf_counter() - t0 < 3.0:
        e2e_cnn_oracle.forward(pcm_h[:8], sd, cfg); k += 8
    return {"backbone_plan": [l for l in m.describe_plan().split("\n") if l.startswith(("conv2d_strided:", "conv2s_x3:", "mean:"))],
            "backbone_ms_alternating": [r[0] for r in runs], "backbone_ms": ours_ms,
            "generic_backbone_plan": generic_plan, "generic_backbone_ms_alternating": [r[2] for r in runs], "generic_backbone_ms": generic_ms,
            "generic_backbone_kernel_ms": gprof,
            "torch_conv2d_chain_ms_alternating": [r[1] for r in runs], "torch_conv2d_chain_ms": chain_ms,
            "backbone_over_generic": round(ours_ms / generic_ms, 3), "backbone_over_torch_chain": round(ours_ms / chain_ms, 3),
            "max_abs_dlogit_default_vs_generic": float((lg_def - lg_gen).abs().max()),
            "backbone_mmac_per_clip_conv2_4": round(macs3 / 1e6, 2), "backbone_mfma_x3_at_peak_ms": round(mfma_ms, 4),
            "backbone_hbm_bytes_per_clip": moved * 4, "backbone_hbm_bound_ms": round(hbm_ms, 4),
            "backbone_over_mfma_x3_at_peak": round(ours_ms / mfma_ms, 1), "backbone_over_hbm_bound": round(ours_ms / hbm_ms, 1),
            "max_abs_dlogit_vs_oracle": float(np.abs(logits[:8].cpu().numpy() - ref).max()),
            "cpu_oracle_clips_per_s": round(k / (time.perf_counter() - t0), 1)}


RNN_CASES = [((101, 64), "pcm", 2048), ((101, 64), "pcm", 4096), ((16, 96), "features", 2048), ((16, 96), "features", 4096)]
RNN_WARMUP, RNN_STEPS, RNN_REPEATS = 20, 100, 3


def rnn_child():
    """One process = one setting of NWW_RNN_IH_FUSED (the knob is read once): every RNN_CASES row, ms per step as the median of RNN_STEPS
    device-event timings behind RNN_WARMUP warm-up steps, and max |dlogit| of 8 clips against the float64 restatement of the tests."""
    import torch
    import oracle
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rnn_oracle
    from nanowakeword_amd.config import FrontendConfig, HeadConfig, head_macs
    from nanowakeword_amd.session import HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_features, synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    for shape, source, B in RNN_CASES:
        cfg = HeadConfig("rnn", shape)
        sd = synth_state_dict(cfg)
        m = HipModel(cfg, fe, device=0, state_dict=sd, window=window, mel_fb=fb)
        ts = torch.cuda.Stream(dev)                   # the launches and the events that time them go to this one stream
        stream = ts.cuda_stream
        logits = torch.empty(B, dtype=torch.float32, device=dev)
        if source == "pcm":
            host = synth_pcm("noise", B, 16000, seed=10)
            x = torch.from_numpy(host).to(dev)
            m.reserve(B, 16000)
            step = lambda: m.forward_pcm_dev(x.data_ptr(), B, 16000, logits.data_ptr(), 0, stream)
            lm = oracle.frontend_logmel(host[:8], window, fb, n_mels=fe.n_mels, center=fe.center).transpose(0, 2, 1)
            ref = rnn_oracle.model_forward(np.ascontiguousarray(lm), sd, cfg, dtype=np.float64).ravel()
        else:
            host = synth_features(B, shape, seed=10)
            x = torch.from_numpy(host).to(dev)
            m.reserve(B, 0)
            step = lambda: m.forward_features_dev(x.data_ptr(), B, logits.data_ptr(), 0, stream)
            ref = rnn_oracle.model_forward(host[:8], sd, cfg, dtype=np.float64).ravel()
        for _ in range(RNN_WARMUP):
            step()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
        for e0, e1 in ev:
            e0.record(ts); step(); e1.record(ts)
        torch.cuda.synchronize()
        ms = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))
        plan = [l for l in m.describe_plan().split("\n") if l.startswith(("lstm:", "lin_x3:model.layer1", "gemm:model.layer1"))]
        print(json.dumps({"shape": list(shape), "source": source, "batch": B, "ms_per_step": round(ms, 4), "plan": plan,
                          "mmac_per_clip": round(head_macs(cfg) / 1e6, 3),
                          "max_abs_dlogit_vs_float64": float(np.abs(logits[:8].cpu().numpy() - ref).max())}), flush=True)
        m.close()


def rnn_main(out_path):
    """The RNN head's A/B: NWW_RNN_IH_FUSED = 1 and 0 alternated, RNN_REPEATS fresh processes each, one after another; per row the median
    of the repeats, their spread (max - min), and whether the fused route wins by more than the larger spread.  Then the per-launch breakdown
    of tools/profile_head.py under each setting, in runs of their own."""
    import subprocess

    def run(args, knob):
        env = dict(os.environ, NWW_RNN_IH_FUSED=knob)
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"child {args} (NWW_RNN_IH_FUSED={knob}) exited {r.returncode}")
        return r.stdout
    runs = {"1": [], "0": []}
    for _ in range(RNN_REPEATS):
        for knob in ("1", "0"):
            runs[knob].append([json.loads(l) for l in run([os.path.abspath(__file__), "--rnn-child"], knob).splitlines() if l.startswith("{")])
    lines = []
    for i, (shape, source, B) in enumerate(RNN_CASES):
        T, F = shape
        f = [r[i]["ms_per_step"] for r in runs["1"]]
        u = [r[i]["ms_per_step"] for r in runs["0"]]
        fm, um = float(np.median(f)), float(np.median(u))
        spread = max(max(f) - min(f), max(u) - min(u))
        lines.append({"config": f"rnn {T}x{F} from {source} B={B}", "head": "rnn", "batch": B, "warmup": RNN_WARMUP, "steps": RNN_STEPS,
                      "fused_ms_repeats": f, "unfused_ms_repeats": u, "fused_ms_per_step": round(fm, 4), "unfused_ms_per_step": round(um, 4),
                      "spread_ms": round(spread, 4), "fused_faster_by_ms": round(um - fm, 4), "fused_wins": bool(um - fm > spread),
                      "fused_clips_per_s": round(B / fm * 1e3, 1), "unfused_clips_per_s": round(B / um * 1e3, 1),
                      "xg_bytes_each_way": B * T * 4 * 64 * 4,          # T x 4H float32 gate pre-activations per clip, written then read
                      "mmac_per_clip": runs["1"][0][i]["mmac_per_clip"],
                      "max_abs_dlogit_vs_float64": {"fused": max(r[i]["max_abs_dlogit_vs_float64"] for r in runs["1"]),
                                                    "unfused": max(r[i]["max_abs_dlogit_vs_float64"] for r in runs["0"])},
                      "fused_plan": runs["1"][0][i]["plan"], "unfused_plan": runs["0"][0][i]["plan"]})
    for knob in ("1", "0"):
        txt = run([os.path.join(ROOT, "tools", "profile_head.py"), "rnn", "4096"], knob)
        lines.append({"config": "rnn 101x64 from pcm B=4096 per-launch (tools/profile_head.py)", "NWW_RNN_IH_FUSED": int(knob),
                      "launch_ms": {m.group(1): float(m.group(2)) for m in (re.match(r"(.*?\S)\s+([0-9.]+) ms", l) for l in txt.splitlines()) if m}})
    text = "".join(json.dumps(l) + "\n" for l in lines)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


REC_HEADS, REC_W, REC_HOP, REC_B = ("cnn", "gru"), 16000, 1280, 4096
REC_HOST_WARMUP, REC_HOST_STEPS = 2, 5


def recording_child():
    """One process = one setting of NWW_REC_SHARED (read once).  Per head: 4096 windows of 1 s, a hop of 80 ms, one pass, the PCM already on
    the device - forward_pcm_dev on the pre-materialised windows (the path recording scoring does not touch: the baseline) and
    forward_recording_dev on the recording, ms per call as the median of RNN_STEPS device-event timings behind RNN_WARMUP warm-up calls;
    then host to host, forward_pcm on the host windows against forward_recording on the host recording (wall clock, median of
    REC_HOST_STEPS); and whether the two agree bit for bit."""
    import torch
    from numpy.lib.stride_tricks import sliding_window_view
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    n = REC_W + (REC_B - 1) * REC_HOP
    rec_h = synth_pcm("speechlike", 1, n, seed=10)[0]
    win_h = np.ascontiguousarray(sliding_window_view(rec_h, REC_W)[::REC_HOP])
    assert win_h.shape == (REC_B, REC_W)
    rec, win = torch.from_numpy(rec_h).to(dev), torch.from_numpy(win_h).to(dev)
    for head in REC_HEADS:
        cfg = HeadConfig(head, (101, 64))
        m = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg), window=window, mel_fb=fb)
        ts = torch.cuda.Stream(dev)
        stream = ts.cuda_stream
        lg_w = torch.empty(REC_B, dtype=torch.float32, device=dev)
        lg_r = torch.empty(REC_B, dtype=torch.float32, device=dev)
        m.reserve(REC_B, REC_W)
        legs = {"windows": lambda: m.forward_pcm_dev(win.data_ptr(), REC_B, REC_W, lg_w.data_ptr(), 0, stream),
                "recording": lambda: m.forward_recording_dev(rec.data_ptr(), n, REC_W, REC_HOP, lg_r.data_ptr(), 0, REC_B, stream)}
        out = {"head": head, "route": m.recording_route(REC_W, REC_HOP), "windows": REC_B, "window": REC_W, "hop": REC_HOP}
        for name, step in legs.items():
            for _ in range(RNN_WARMUP):
                step()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
            for e0, e1 in ev:
                e0.record(ts); step(); e1.record(ts)
            torch.cuda.synchronize()
            out[name + "_ms"] = round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)
        out["bit_identical"] = bool(torch.equal(lg_w, lg_r))

        def wall(fn):
            for _ in range(REC_HOST_WARMUP):
                fn()
            t = []
            for _ in range(REC_HOST_STEPS):
                t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
            return round(float(np.median(t)), 3)
        out["host_windows_ms"] = wall(lambda: m.forward_pcm(win_h))
        out["host_recording_ms"] = wall(lambda: m.forward_recording(rec_h, REC_W, REC_HOP, max_batch=REC_B))
        out["host_bit_identical"] = bool(np.array_equal(m.forward_pcm(win_h)[0], m.forward_recording(rec_h, REC_W, REC_HOP, max_batch=REC_B)[0]))
        print(json.dumps(out), flush=True)
        m.close()


def recording_main(out_path):
    """NWW_REC_SHARED = 1 and 0 alternated, RNN_REPEATS fresh processes each, one after another (the protocol of --rnn); per head the
    medians of the repeats, their spread (max - min), and whether the shared-frame route beats the strided one by more than the spread."""
    import subprocess

    def run(knob):
        env = dict(os.environ, NWW_REC_SHARED=knob)
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--recording-child"], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"child (NWW_REC_SHARED={knob}) exited {r.returncode}")
        return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    runs = {"1": [], "0": []}
    for _ in range(RNN_REPEATS):
        for knob in ("1", "0"):
            runs[knob].append(run(knob))
    lines = []
    for i, head in enumerate(REC_HEADS):
        assert all(r[i]["route"] == int(k) and r[i]["bit_identical"] and r[i]["host_bit_identical"] for k in runs for r in runs[k]), head
        sh = [r[i]["recording_ms"] for r in runs["1"]]
        st = [r[i]["recording_ms"] for r in runs["0"]]
        base = [r[i]["windows_ms"] for k in ("1", "0") for r in runs[k]]
        shm, stm, bm = float(np.median(sh)), float(np.median(st)), float(np.median(base))
        spread = max(max(sh) - min(sh), max(st) - min(st))
        hw = [r[i]["host_windows_ms"] for k in ("1", "0") for r in runs[k]]
        hs, ht = [r[i]["host_recording_ms"] for r in runs["1"]], [r[i]["host_recording_ms"] for r in runs["0"]]
        lines.append({"config": f"recording {head} 101x64 W={REC_W} hop={REC_HOP} {REC_B} windows per pass", "head": head, "windows": REC_B,
                      "warmup": RNN_WARMUP, "steps": RNN_STEPS, "materialised_windows_ms_repeats": base, "strided_ms_repeats": st,
                      "shared_ms_repeats": sh, "materialised_windows_ms": round(bm, 4), "strided_ms": round(stm, 4), "shared_ms": round(shm, 4),
                      "spread_ms": round(spread, 4), "shared_faster_by_ms": round(stm - shm, 4), "shared_wins": bool(stm - shm > spread),
                      "materialised_windows_per_s": round(REC_B / bm * 1e3, 1), "strided_windows_per_s": round(REC_B / stm * 1e3, 1),
                      "shared_windows_per_s": round(REC_B / shm * 1e3, 1), "bit_identical_to_windows": True,
                      "host_to_host": {"steps": REC_HOST_STEPS, "forward_pcm_on_windows_ms_repeats": hw, "forward_recording_shared_ms_repeats": hs,
                                       "forward_recording_strided_ms_repeats": ht, "forward_pcm_on_windows_ms": round(float(np.median(hw)), 3),
                                       "forward_recording_shared_ms": round(float(np.median(hs)), 3),
                                       "forward_recording_strided_ms": round(float(np.median(ht)), 3),
                                       "bytes_uploaded": {"windows": REC_B * REC_W * 2, "recording": (REC_W + (REC_B - 1) * REC_HOP) * 2}}})
    lines.append({"config": "recording: default of NWW_REC_SHARED by the rule 'shared beats strided on both heads by more than the spread'",
                  "NWW_REC_SHARED_default": int(all(l["shared_wins"] for l in lines))})
    text = "".join(json.dumps(l) + "\n" for l in lines)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


RAW_REC_HEADS = (("e2e_quartznet", (63, 128)), ("e2e_cnn", (250, 64)))
RAW_REC_STREAMS = 1024


def recording_raw_child():
    """recording_child for the raw-PCM heads, one process = one setting (NWW_REC_SHARED and NWW_STREAM_INC, read once; or the package of
    another checkout, NWW_BENCH_PACKAGE_ROOT).  Per head: the 4096 windows of --recording through forward_pcm_dev (materialised) and
    forward_recording_dev, device-event medians as there and whether the two agree bit for bit; then RAW_REC_STREAMS streams, ms per hop of
    stream_push_dev behind the pushes that fill the window and RNN_WARMUP more."""
    import torch
    from numpy.lib.stride_tricks import sliding_window_view
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipModel
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    n = REC_W + (REC_B - 1) * REC_HOP
    rec_h = synth_pcm("speechlike", 1, n, seed=10)[0]
    win_h = np.ascontiguousarray(sliding_window_view(rec_h, REC_W)[::REC_HOP])
    rec, win = torch.from_numpy(rec_h).to(dev), torch.from_numpy(win_h).to(dev)
    chunk = torch.from_numpy(synth_pcm("speechlike", RAW_REC_STREAMS, REC_HOP, seed=11)).to(dev)

    def timed(ts, step):
        for _ in range(RNN_WARMUP):
            step()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
        for e0, e1 in ev:
            e0.record(ts); step(); e1.record(ts)
        torch.cuda.synchronize()
        return round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)

    for head, shape in RAW_REC_HEADS:
        cfg = HeadConfig(head, shape)
        m = HipModel(cfg, FrontendConfig(), device=0, state_dict=synth_state_dict(cfg))
        ts = torch.cuda.Stream(dev)
        stream = ts.cuda_stream
        lg_w = torch.empty(REC_B, dtype=torch.float32, device=dev)
        lg_r = torch.empty(REC_B, dtype=torch.float32, device=dev)
        lg_s = torch.empty(RAW_REC_STREAMS, dtype=torch.float32, device=dev)
        m.reserve(REC_B, REC_W)
        out = {"head": head, "route": m.recording_route(REC_W, REC_HOP), "windows": REC_B, "window": REC_W, "hop": REC_HOP}
        out["windows_ms"] = timed(ts, lambda: m.forward_pcm_dev(win.data_ptr(), REC_B, REC_W, lg_w.data_ptr(), 0, stream))
        out["recording_ms"] = timed(ts, lambda: m.forward_recording_dev(rec.data_ptr(), n, REC_W, REC_HOP, lg_r.data_ptr(), 0, REC_B, stream))
        out["bit_identical"] = bool(torch.equal(lg_w, lg_r))
        m.stream_open(RAW_REC_STREAMS, REC_W, REC_HOP)
        for _ in range(REC_W // REC_HOP + 1):
            m.stream_push_dev(chunk.data_ptr(), lg_s.data_ptr(), 0, stream)
        out["streams"] = RAW_REC_STREAMS
        out["stream_ms_per_hop"] = timed(ts, lambda: m.stream_push_dev(chunk.data_ptr(), lg_s.data_ptr(), 0, stream))
        m.stream_close()
        print(json.dumps(out), flush=True)
        m.close()


def recording_raw_main(out_path, parent_root):
    """The raw-PCM heads' recording and stream rows: the shared route (the default), NWW_REC_SHARED = NWW_STREAM_INC = 0 on the same build
    and - with --parent DIR, a built checkout of the parent commit - that commit's package, alternated, RNN_REPEATS fresh processes each;
    per head the medians of the repeats, their spread (max - min) and whether the shared route beats the strided one by more than three
    times the spread (the rule the planner's default follows)."""
    import subprocess

    def run(setting):
        env = dict(os.environ)
        if setting == "parent":
            env["NWW_BENCH_PACKAGE_ROOT"] = parent_root
        else:
            env.update(NWW_REC_SHARED=setting, NWW_STREAM_INC="3" if setting == "1" else "0")
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--recording-raw-child"], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"child ({setting}) exited {r.returncode}")
        print(f"[{setting}] {r.stdout.strip()}", file=sys.stderr, flush=True)
        return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    settings =("1", "0") + (("parent",) if parent_root else ())
    runs = {s: [] for s in settings}
    for _ in range(RNN_REPEATS):
        for s in settings:
            runs[s].append(run(s))
    lines = []
    for i, (head, shape) in enumerate(RAW_REC_HEADS):
        assert all(r[i]["bit_identical"] for s in runs for r in runs[s]), head
        assert all(r[i]["route"] == (1 if s == "1" else 0) for s in runs for r in runs[s]), head
        line = {"config": f"recording {head} {shape[0]}x{shape[1]} W={REC_W} hop={REC_HOP} {REC_B} windows per pass, {RAW_REC_STREAMS} streams",
                "head": head, "windows": REC_B, "streams": RAW_REC_STREAMS, "warmup": RNN_WARMUP, "steps": RNN_STEPS, "repeats": RNN_REPEATS}
        for key, name in (("recording_ms", "recording"), ("stream_ms_per_hop", "stream_hop")):
            rep = {s: [r[i][key] for r in runs[s]] for s in settings}
            med = {s: float(np.median(v)) for s, v in rep.items()}
            spread = max(max(v) - min(v) for v in rep.values())
            line[name] = {"shared_ms_repeats": rep["1"], "strided_ms_repeats": rep["0"], "shared_ms": round(med["1"], 4), "strided_ms": round(med["0"], 4),
                          "spread_ms": round(spread, 4), "shared_faster_by_ms": round(med["0"] - med["1"], 4),
                          "shared_wins": bool(med["0"] - med["1"] > 3 * spread)}
            if parent_root:
                line[name].update(parent_ms_repeats=rep["parent"], parent_ms=round(med["parent"], 4))
        base = [r[i]["windows_ms"] for s in settings for r in runs[s]]
        line["materialised_windows_ms"] = round(float(np.median(base)), 4)
        line["bit_identical_to_windows"] = True
        lines.append(line)
    text = "".join(json.dumps(l) + "\n" for l in lines)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


CAS_VERIFIERS = (("cnn", (101, 64)), ("e2e_cnn", (250, 64)))
CAS_GATE = ("e2e_dnn", (64, 101))
CAS_HOST_WINDOWS = 200                 # host to host: a recording of 16000 + 199 * 1280 samples (about 17 s), every chunk through predict()


def cascade_child():
    """One process: per verifier, REC_B windows of 1 s every 80 ms with the PCM on the device - the gate alone and the verifier alone on all
    windows (forward_recording_dev), then the cascade at thresholds that open 0 %, about 5 % and 100 % of the windows, taken from the
    gate's own score quantiles; ms per call as the median of RNN_STEPS device-event timings behind RNN_WARMUP warm-up calls.  Then host to
    host on a shorter recording: HipInterpreter.score_recording of the pair on the batch path against the same interpreter's predict()
    loop (wall clock, one pass each behind a warm-up pass), and whether the two agree."""
    import torch
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.interpreter import HipInterpreter
    from nanowakeword_amd.session import HipCascade, HipModel, HipSession, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    n = REC_W + (REC_B - 1) * REC_HOP
    rec_h = synth_pcm("speechlike", 1, n, seed=10)[0]
    rec = torch.from_numpy(rec_h).to(dev)
    gcfg = HeadConfig(*CAS_GATE)
    for head, shape in CAS_VERIFIERS:
        gate = HipModel(gcfg, fe, device=0, state_dict=synth_state_dict(gcfg), window=window, mel_fb=fb)
        cfg = HeadConfig(head, shape)
        ver = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg), window=window, mel_fb=fb)
        cas = HipCascade(gate, ver)
        ts = torch.cuda.Stream(dev)
        stream = ts.cuda_stream
        gp, lg, pr = (torch.empty(REC_B, dtype=torch.float32, device=dev) for _ in range(3))
        gate.reserve(REC_B, REC_W); ver.reserve(REC_B, REC_W)
        gate.forward_recording_dev(rec.data_ptr(), n, REC_W, REC_HOP, lg.data_ptr(), gp.data_ptr(), REC_B, stream)
        torch.cuda.synchronize()
        q = np.sort(gp.cpu().numpy().astype(np.float64))
        thr = {"0": float(np.nextafter(q[-1], np.inf)), "5": float(q[-(REC_B // 20)]), "100": float(q[0])}
        casc = lambda t: (lambda: cas.forward_recording_dev(rec.data_ptr(), n, REC_W, REC_HOP, gp.data_ptr(), lg.data_ptr(), pr.data_ptr(), REC_B,
                                                            stream, gate_threshold=t))
        legs = {"gate": lambda: gate.forward_recording_dev(rec.data_ptr(), n, REC_W, REC_HOP, 0, gp.data_ptr(), REC_B, stream),
                "verifier": lambda: ver.forward_recording_dev(rec.data_ptr(), n, REC_W, REC_HOP, lg.data_ptr(), pr.data_ptr(), REC_B, stream),
                "cascade_0": casc(thr["0"]), "cascade_5": casc(thr["5"]), "cascade_100": casc(thr["100"])}
        out = {"verifier": head, "gate": CAS_GATE[0], "windows": REC_B, "window": REC_W, "hop": REC_HOP, "thresholds": thr,
               "gate_route": gate.recording_route(REC_W, REC_HOP), "verifier_route": ver.recording_route(REC_W, REC_HOP)}
        for name, step in legs.items():
            for _ in range(RNN_WARMUP):
                got = step()
            torch.cuda.synchronize()
            if name.startswith("cascade"):
                out[name + "_open"] = got[1]
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
            for e0, e1 in ev:
                e0.record(ts); step(); e1.record(ts)
            torch.cuda.synchronize()
            out[name + "_ms"] = round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)
        # host to host
        short = np.ascontiguousarray(rec_h[:REC_W + (CAS_HOST_WINDOWS - 1) * REC_HOP])
        it = HipInterpreter({"gate": HipSession(gate, name="gate"), "kw": HipSession(ver, name="kw")})
        it.cascade_config = {"gate": "gate", "verifier": "kw", "gate_threshold": thr["5"]}

        def loop():
            it.reset()
            return np.array([it.predict(short[i:i + REC_HOP]).scores["kw"] for i in range(0, len(short), REC_HOP)], np.float32)

        def wall(fn):
            fn()
            t0 = time.perf_counter()
            r = fn()
            return round((time.perf_counter() - t0) * 1e3, 3), r
        out["host_batch_ms"], a = wall(lambda: it.score_recording(short)["kw"])
        out["host_open"] = list(it.models["kw"].last_cascade)
        out["host_loop_ms"], b = wall(loop)
        out["host_chunks"], out["host_samples"], out["host_equal"] = len(a), len(short), bool(np.array_equal(a, b))
        print(json.dumps(out), flush=True)
        gate.close(); ver.close()


def cascade_main(out_path):
    """RNN_REPEATS fresh child processes, one after another, each under its own time limit; per verifier the medians of the repeats, their
    spread (max - min over the repeats, the largest of the legs compared), and the three written-down differences."""
    import subprocess
    runs = []
    for _ in range(RNN_REPEATS):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--cascade-child"], env=dict(os.environ),
                           cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"cascade child exited {r.returncode}")
        runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")])
    lines = []
    for i, (head, shape) in enumerate(CAS_VERIFIERS):
        rep = {k: [r[i][k + "_ms"] for r in runs] for k in ("gate", "verifier", "cascade_0", "cascade_5", "cascade_100", "host_batch", "host_loop")}
        med = {k: float(np.median(v)) for k, v in rep.items()}
        spread = max(max(v) - min(v) for k, v in rep.items() if not k.startswith("host"))
        first = runs[0][i]
        assert all(r[i]["host_equal"] for r in runs), head
        lines.append({"config": f"cascade {CAS_GATE[0]} {CAS_GATE[1][0]}x{CAS_GATE[1][1]} -> {head} {shape[0]}x{shape[1]} W={REC_W} hop={REC_HOP} "
                                f"{REC_B} windows, PCM on the device",
                      "gate": CAS_GATE[0], "verifier": head, "windows": REC_B, "warmup": RNN_WARMUP, "steps": RNN_STEPS, "repeats": RNN_REPEATS,
                      "thresholds": first["thresholds"], "open_windows": {k: first[f"cascade_{k}_open"] for k in ("0", "5", "100")},
                      "gate_route": first["gate_route"], "verifier_route": first["verifier_route"],
                      "ms_repeats": {k: v for k, v in rep.items() if not k.startswith("host")},
                      "gate_ms": round(med["gate"], 4), "verifier_alone_ms": round(med["verifier"], 4), "cascade_0pct_ms": round(med["cascade_0"], 4),
                      "cascade_5pct_ms": round(med["cascade_5"], 4), "cascade_100pct_ms": round(med["cascade_100"], 4), "spread_ms": round(spread, 4),
                      "select_and_readback_ms": round(med["cascade_0"] - med["gate"], 4),
                      "gather_and_scatter_ms": round(med["cascade_100"] - med["gate"] - med["verifier"], 4),
                      "cascade_5pct_faster_than_verifier_alone_by_ms": round(med["verifier"] - med["cascade_5"], 4),
                      "cascade_5pct_wins": bool(med["verifier"] - med["cascade_5"] > spread),
                      "verifier_alone_over_cascade_5pct": round(med["verifier"] / med["cascade_5"], 2),
                      "host_to_host": {"samples": first["host_samples"], "chunks": first["host_chunks"], "windows_open": first["host_open"],
                                       "score_recording_batch_ms_repeats": rep["host_batch"], "predict_loop_ms_repeats": rep["host_loop"],
                                       "score_recording_batch_ms": round(med["host_batch"], 3), "predict_loop_ms": round(med["host_loop"], 3),
                                       "loop_over_batch": round(med["host_loop"] / med["host_batch"], 1), "equal": True}})
    text = "".join(json.dumps(l) + "\n" for l in lines)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


POOL_HEADS, POOL_STREAMS = ("crnn", "cnn"), 1024


def stream_pool_child():
    """One process = one setting of NWW_STREAM_INC (read once).  Per head: POOL_STREAMS streams, 1 s windows, 80 ms hops, device-resident
    chunks; ms per tick as the median of RNN_STEPS device-event timings behind the pushes that fill the windows and RNN_WARMUP more, each
    leg on a batch of its own: lock-step stream_push_dev, push_some with every stream listed, push_some with a random half listed (eight
    seeded halves in turn, so the streams' ring positions drift apart)."""
    import torch
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    S = POOL_STREAMS
    parts = [torch.from_numpy(synth_pcm("speechlike", S, REC_HOP, seed=20 + i)).to(dev) for i in range(4)]
    rng = np.random.default_rng(5)
    every = np.arange(S, dtype=np.int32)
    halves = [np.sort(rng.permutation(S)[:S // 2]).astype(np.int32) for _ in range(8)]
    half_parts = [[p[torch.from_numpy(h.astype(np.int64)).to(dev)].contiguous() for p in parts] for h in halves]
    fill = REC_W // REC_HOP + 1

    def timed(ts, step):
        for i in range(RNN_WARMUP):
            step(i)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
        for i, (e0, e1) in enumerate(ev):
            e0.record(ts); step(RNN_WARMUP + i); e1.record(ts)
        torch.cuda.synchronize()
        return round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)

    for head in POOL_HEADS:
        cfg = HeadConfig(head, (101, 64))
        m = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg), window=window, mel_fb=fb)
        ts = torch.cuda.Stream(dev)
        stream = ts.cuda_stream
        lg = torch.empty(S, dtype=torch.float32, device=dev)
        out = {"head": head, "streams": S, "window": REC_W, "hop": REC_HOP}

        def lock(i):
            m.stream_push_dev(parts[i % 4].data_ptr(), lg.data_ptr(), 0, stream)

        def some_all(i):
            m.stream_push_some_dev(every, parts[i % 4].data_ptr(), lg.data_ptr(), 0, stream)

        def some_half(i):
            m.stream_push_some_dev(halves[i % 8], half_parts[i % 8][i % 4].data_ptr(), lg.data_ptr(), 0, stream)

        for name, step in (("lock_step", lock), ("some_all", some_all), ("some_half", some_half)):
            m.stream_open(S, REC_W, REC_HOP)
            for i in range(fill):
                (lock if name == "lock_step" else some_all)(i)
            out[name + "_ms"] = timed(ts, step)
            if name != "lock_step":
                out[name + "_stats"] = list(m.stream_pool_stats())
            m.stream_close()
        out["route"] = out["some_all_stats"][1]
        print(json.dumps(out), flush=True)
        m.close()


def stream_pool_main(out_path):
    """NWW_STREAM_INC = 3 (the default) and 0 alternated, RNN_REPEATS fresh processes each, one after another (the protocol of --recording);
    per head the medians of the repeats and their spread (max - min) for (a) lock-step nww_stream_push_dev, (b) push_some with every
    stream listed, (c) push_some with a random half listed, each on the shared-frame route, and (d) the same two push_some legs re-scoring
    whole windows (NWW_STREAM_INC=0); and whether (b) beats (d) by more than the spread."""
    import subprocess

    def run(knob):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--stream-pool-child"],
                           env=dict(os.environ, NWW_STREAM_INC=knob), cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"child (NWW_STREAM_INC={knob}) exited {r.returncode}")
        print(f"[NWW_STREAM_INC={knob}] {r.stdout.strip()}", file=sys.stderr, flush=True)
        return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    runs = {"3": [], "0": []}
    for _ in range(RNN_REPEATS):
        for knob in ("3", "0"):
            runs[knob].append(run(knob))
    lines = []
    for i, head in enumerate(POOL_HEADS):
        assert all(r[i]["route"] == (1 if k == "3" else 0) for k in runs for r in runs[k]), head
        rep = {"a_lock_step": [r[i]["lock_step_ms"] for r in runs["3"]], "b_push_some_all": [r[i]["some_all_ms"] for r in runs["3"]],
               "c_push_some_half": [r[i]["some_half_ms"] for r in runs["3"]], "d_whole_windows_all": [r[i]["some_all_ms"] for r in runs["0"]],
               "d_whole_windows_half": [r[i]["some_half_ms"] for r in runs["0"]], "lock_step_whole_windows": [r[i]["lock_step_ms"] for r in runs["0"]]}
        med = {k: float(np.median(v)) for k, v in rep.items()}
        spread = max(max(v) - min(v) for v in rep.values())
        line = {"config": f"stream pool {head} 101x64 W={REC_W} hop={REC_HOP} {POOL_STREAMS} streams, ms per tick", "head": head, "streams": POOL_STREAMS,
                "warmup": RNN_WARMUP, "steps": RNN_STEPS, "repeats": RNN_REPEATS}
        for k in rep:
            line[k + "_ms_repeats"] = rep[k]
            line[k + "_ms"] = round(med[k], 4)
        line.update(spread_ms=round(spread, 4), b_over_a_ms=round(med["b_push_some_all"] - med["a_lock_step"], 4),
                    b_faster_than_d_by_ms=round(med["d_whole_windows_all"] - med["b_push_some_all"], 4),
                    c_faster_than_d_by_ms=round(med["d_whole_windows_half"] - med["c_push_some_half"], 4),
                    lock_step_wins_over_b=bool(med["b_push_some_all"] - med["a_lock_step"] > spread),
                    shared_frames_win=bool(med["d_whole_windows_all"] - med["b_push_some_all"] > spread and
                                           med["d_whole_windows_half"] - med["c_push_some_half"] > spread))
        lines.append(line)
    text = "".join(json.dumps(l) + "\n" for l in lines)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


CPOOL_OPEN = ("5", "50")               # per cent of the scored streams the thresholds open, from the gate's own score quantiles


def cascade_pool_child():
    """One process: per verifier, POOL_STREAMS streams, 1 s windows, 80 ms hops, device-resident chunks, the CAS_GATE gate; every leg on a
    fresh batch filled by pushes that list every stream, ms per tick as the median of RNN_STEPS device-event timings behind RNN_WARMUP
    warm-up calls.  Settings: every stream listed / a random half listed (eight seeded halves in turn).  Legs: gate_some - the gate's
    push_some alone; new - nww_cascade_stream_push_some_dev at thresholds that open about 5 % and 50 % of the scored streams; today - what
    the entry points before it allow, push_some on the gate plus push_some on a verifier batch for every listed stream; lock -
    nww_cascade_stream_push_dev with all streams; verifier_open - the verifier's forward_pcm_dev alone on as many windows as the new call
    opened."""
    import torch
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipCascade, HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    S = POOL_STREAMS
    parts = [torch.from_numpy(synth_pcm("speechlike", S, REC_HOP, seed=20 + i)).to(dev) for i in range(4)]
    clips = torch.from_numpy(synth_pcm("speechlike", S, REC_W, seed=30)).to(dev)
    rng = np.random.default_rng(5)
    every = np.arange(S, dtype=np.int32)
    halves = [np.sort(rng.permutation(S)[:S // 2]).astype(np.int32) for _ in range(8)]
    half_parts = [[p[torch.from_numpy(h.astype(np.int64)).to(dev)].contiguous() for p in parts] for h in halves]
    listed = {"all": lambda i: (every, parts[i % 4]), "half": lambda i: (halves[i % 8], half_parts[i % 8][i % 4])}
    fill = REC_W // REC_HOP + 1
    gcfg = HeadConfig(*CAS_GATE)

    def timed(ts, step):
        for i in range(RNN_WARMUP):
            step(i)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
        opened = []
        for i, (e0, e1) in enumerate(ev):
            e0.record(ts); opened.append(step(RNN_WARMUP + i)); e1.record(ts)
        torch.cuda.synchronize()
        return round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4), opened

    for head, shape in CAS_VERIFIERS:
        gate = HipModel(gcfg, fe, device=0, state_dict=synth_state_dict(gcfg), window=window, mel_fb=fb)
        cfg = HeadConfig(head, shape)
        ver = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg), window=window, mel_fb=fb)
        cas = HipCascade(gate, ver)
        ts = torch.cuda.Stream(dev)
        stream = ts.cuda_stream
        gp, lg, pr = (torch.empty(S, dtype=torch.float32, device=dev) for _ in range(3))
        gate.reserve(S, REC_W); ver.reserve(S, REC_W)
        out = {"verifier": head, "gate": CAS_GATE[0], "streams": S, "window": REC_W, "hop": REC_HOP}

        def fresh(with_verifier=False):
            gate.stream_open(S, REC_W, REC_HOP)
            if with_verifier:
                ver.stream_open(S, REC_W, REC_HOP)
            for i in range(fill):
                gate.stream_push_some_dev(every, parts[i % 4].data_ptr(), lg.data_ptr(), gp.data_ptr(), stream)
                if with_verifier:
                    ver.stream_push_some_dev(every, parts[i % 4].data_ptr(), lg.data_ptr(), pr.data_ptr(), stream)
            torch.cuda.synchronize()

        fresh()
        q = np.sort(gp.cpu().numpy().astype(np.float64))
        thr = {"5": float(q[-(S // 20)]), "50": float(q[S // 2])}
        out["thresholds"] = thr
        out["gate_route"] = gate.stream_pool_stats()[1]
        gate.stream_close()
        for setting, pick in listed.items():
            def gate_some(i):
                ids, chunk = pick(i)
                gate.stream_push_some_dev(ids, chunk.data_ptr(), lg.data_ptr(), gp.data_ptr(), stream)

            def today(i):
                ids, chunk = pick(i)
                gate.stream_push_some_dev(ids, chunk.data_ptr(), 0, gp.data_ptr(), stream)
                ver.stream_push_some_dev(ids, chunk.data_ptr(), lg.data_ptr(), pr.data_ptr(), stream)

            fresh()
            out[f"gate_some_{setting}_ms"], _ = timed(ts, gate_some)
            gate.stream_close()
            fresh(with_verifier=True)
            out[f"today_{setting}_ms"], _ = timed(ts, today)
            out["verifier_route"] = ver.stream_pool_stats()[1]
            gate.stream_close(); ver.stream_close()
            for pct in CPOOL_OPEN:
                def new(i):
                    ids, chunk = pick(i)
                    return cas.stream_push_some_dev(ids, chunk.data_ptr(), gp.data_ptr(), lg.data_ptr(), pr.data_ptr(), stream, gate_threshold=thr[pct])

                fresh()
                out[f"new_{setting}_{pct}_ms"], opened = timed(ts, new)
                gate.stream_close()
                n_open = int(np.median(opened))
                out[f"new_{setting}_{pct}_open"] = n_open
                out[f"verifier_open_{setting}_{pct}_ms"], _ = timed(
                    ts, lambda i: ver.forward_pcm_dev(clips.data_ptr(), max(n_open, 1), REC_W, lg.data_ptr(), pr.data_ptr(), stream))
        for pct in CPOOL_OPEN:
            fresh()
            out[f"lock_{pct}_ms"], opened = timed(
                ts, lambda i: cas.stream_push_dev(parts[i % 4].data_ptr(), gp.data_ptr(), lg.data_ptr(), pr.data_ptr(), stream, gate_threshold=thr[pct]))
            out[f"lock_{pct}_open"] = int(np.median(opened))
            gate.stream_close()
        print(json.dumps(out), flush=True)
        gate.close(); ver.close()


def cascade_pool_main(out_path):
    """RNN_REPEATS fresh child processes, one after another, each under its own time limit (the protocol of --cascade); per verifier and
    setting the medians of the repeats and their spread (max - min, the largest of the legs), and per threshold (a) the new call, (b) today's
    two push_some calls, (c) the lock-step cascade with all streams as the floor, and the share of (a) that is neither the gate's
    push_some nor the verifier on the open windows: the select, the count's read-back, the gather and the scatter."""
    import subprocess
    runs = []
    for _ in range(RNN_REPEATS):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--cascade-pool-child"], env=dict(os.environ),
                           cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"cascade-pool child exited {r.returncode}")
        print(f"[cascade-pool child] {r.stdout.strip()}", file=sys.stderr, flush=True)
        runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")])
    lines = []
    for i, (head, shape) in enumerate(CAS_VERIFIERS):
        first = runs[0][i]
        rep = {k[:-3]: [r[i][k] for r in runs] for k in first if k.endswith("_ms")}
        med = {k: float(np.median(v)) for k, v in rep.items()}
        spread = max(max(v) - min(v) for v in rep.values())
        for setting in ("all", "half"):
            line = {"config": f"cascade pool {CAS_GATE[0]} {CAS_GATE[1][0]}x{CAS_GATE[1][1]} -> {head} {shape[0]}x{shape[1]} W={REC_W} hop={REC_HOP} "
                              f"{POOL_STREAMS} streams, {setting} listed, ms per tick",
                    "gate": CAS_GATE[0], "verifier": head, "streams": POOL_STREAMS, "listed": POOL_STREAMS if setting == "all" else POOL_STREAMS // 2,
                    "warmup": RNN_WARMUP, "steps": RNN_STEPS, "repeats": RNN_REPEATS, "thresholds": first["thresholds"],
                    "gate_route": first["gate_route"], "verifier_route": first["verifier_route"],
                    "ms_repeats": {k: v for k, v in rep.items() if setting in k or k.startswith("lock")},
                    "gate_push_some_ms": round(med[f"gate_some_{setting}"], 4), "b_today_two_push_some_ms": round(med[f"today_{setting}"], 4),
                    "spread_ms": round(spread, 4)}
            for pct in CPOOL_OPEN:
                a, b = med[f"new_{setting}_{pct}"], med[f"today_{setting}"]
                line[f"open_{pct}pct"] = {
                    "open_streams": first[f"new_{setting}_{pct}_open"], "a_new_call_ms": round(a, 4),
                    "c_lock_step_all_streams_ms": round(med[f"lock_{pct}"], 4), "c_open_streams": first[f"lock_{pct}_open"],
                    "verifier_on_open_windows_ms": round(med[f"verifier_open_{setting}_{pct}"], 4),
                    "select_readback_gather_scatter_ms": round(a - med[f"gate_some_{setting}"] - med[f"verifier_open_{setting}_{pct}"], 4),
                    "a_faster_than_b_by_ms": round(b - a, 4), "b_over_a": round(b / a, 2), "a_wins": bool(b - a > spread),
                    "a_loses": bool(a - b > spread)}
            lines.append(line)
    text = "".join(json.dumps(l) + "\n" for l in lines)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


BANK_B = 4096
# (name, workload, [(head, seed)]): 1 s clips, 64 mel; the DNN heads are the reference's default model_type with weights of their own
BANK_SETTINGS = [
    ("batch 2 dnn", "batch", [("dnn", 1), ("dnn", 2)]),
    ("batch 4 dnn", "batch", [("dnn", 1), ("dnn", 2), ("dnn", 3), ("dnn", 4)]),
    ("batch cnn+gru+crnn", "batch", [("cnn", 1), ("gru", 1), ("crnn", 1)]),
    ("stream pool 4 dnn, all listed", "pool_all", [("dnn", 1), ("dnn", 2), ("dnn", 3), ("dnn", 4)]),
    ("stream pool 4 dnn, a random half", "pool_half", [("dnn", 1), ("dnn", 2), ("dnn", 3), ("dnn", 4)]),
    ("recording cnn+dnn", "recording", [("cnn", 1), ("dnn", 1)]),
]


def bank_child():
    """One process, every BANK_SETTINGS row: the members as ONE bank call (session.HipBank, PCM on the device) against the same handles
    called one after the other through the single-handle entry points, ms per call as the median of RNN_STEPS device-event timings behind
    RNN_WARMUP warm-up calls; and the leader's frontend entry of nww_get_profile on its single call (what a follower no longer runs).
    Stream rows: POOL_STREAMS streams, 80 ms hops; the bank's batch is the leader's, the baseline opens one batch per handle."""
    import torch
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipBank, HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    B, S, W, hop = BANK_B, POOL_STREAMS, REC_W, REC_HOP
    ts = torch.cuda.Stream(dev)
    stream = ts.cuda_stream
    pcm = torch.from_numpy(synth_pcm("noise", B, W, seed=10)).to(dev)
    rec_n = W + (B - 1) * hop
    rec = torch.from_numpy(synth_pcm("speechlike", 1, rec_n, seed=3)[0]).to(dev)
    parts = [torch.from_numpy(synth_pcm("speechlike", S, hop, seed=20 + i)).to(dev) for i in range(4)]
    rng = np.random.default_rng(5)
    every = np.arange(S, dtype=np.int32)
    halves = [np.sort(rng.permutation(S)[:S // 2]).astype(np.int32) for _ in range(8)]
    half_parts = [[p[torch.from_numpy(h.astype(np.int64)).to(dev)].contiguous() for p in parts] for h in halves]
    fill = W // hop + 1
    models = {}

    def model(head, seed):
        if (head, seed) not in models:
            cfg = HeadConfig(head, (101, 64))
            models[(head, seed)] = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg, seed=seed), window=window, mel_fb=fb)
        return models[(head, seed)]

    def timed(step):
        for i in range(RNN_WARMUP):
            step(i)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
        for i, (e0, e1) in enumerate(ev):
            e0.record(ts); step(RNN_WARMUP + i); e1.record(ts)
        torch.cuda.synchronize()
        return round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)

    def frontend_ms(lead, step):
        lead.set_profiling(True)
        for i in range(20):
            step(i)
        torch.cuda.synchronize()
        name, ms, cnt = lead.get_profile()[0]
        lead.set_profiling(False)
        return round(ms / max(cnt, 1), 4)

    for name, work, heads in BANK_SETTINGS:
        ms = [model(h, s) for h, s in heads]
        k = len(ms)
        bank = HipBank({str(j): m for j, m in enumerate(ms)})
        n = {"batch": B, "recording": B, "pool_all": S, "pool_half": S // 2}[work]
        lg = torch.empty(k * n, dtype=torch.float32, device=dev)
        rows = [lg[j * n:(j + 1) * n] for j in range(k)]
        out = {"setting": name, "workload": work, "members": [h for h, _ in heads], "k": k, "items": n}
        if work == "batch":
            def one(m, row):
                m.forward_pcm_dev(pcm.data_ptr(), B, W, row.data_ptr(), 0, stream)
            sep = timed(lambda i: [one(m, r) for m, r in zip(ms, rows)])
            want = lg.clone()
            bnk = timed(lambda i: bank.forward_pcm_dev(pcm.data_ptr(), B, W, lg.data_ptr(), 0, stream))
            fe_ms = frontend_ms(ms[0], lambda i: one(ms[0], rows[0]))
        elif work == "recording":
            def one(m, row):
                m.forward_recording_dev(rec.data_ptr(), rec_n, W, hop, row.data_ptr(), 0, B, stream)
            sep = timed(lambda i: [one(m, r) for m, r in zip(ms, rows)])
            want = lg.clone()
            bnk = timed(lambda i: bank.forward_recording_dev(rec.data_ptr(), rec_n, W, hop, lg.data_ptr(), 0, B, stream))
            fe_ms = frontend_ms(ms[0], lambda i: one(ms[0], rows[0]))
            out["route"] = ms[0].recording_route(W, hop)
        else:
            def args(i):
                return (every, parts[i % 4]) if work == "pool_all" else (halves[i % 8], half_parts[i % 8][i % 4])

            def one(m, row, i):
                ids, chunk = args(i)
                m.stream_push_some_dev(ids, chunk.data_ptr(), row.data_ptr(), 0, stream)
            for m in ms:                                           # the baseline: a batch per handle, each filled
                m.stream_open(S, W, hop)
                for i in range(fill):
                    m.stream_push_some_dev(every, parts[i % 4].data_ptr(), rows[0].data_ptr(), 0, stream)
            sep = timed(lambda i: [one(m, r, i) for m, r in zip(ms, rows)])
            fe_ms = frontend_ms(ms[0], lambda i: one(ms[0], rows[0], RNN_WARMUP + RNN_STEPS + i))
            for m in ms:
                m.stream_close()
            bank.stream_open(S, W, hop)                            # the bank: the leader's batch alone, filled, then the same calls
            for i in range(fill):
                bank.stream_push_some_dev(every, parts[i % 4].data_ptr(), lg.data_ptr(), 0, stream)

            def step(i):
                ids, chunk = args(i)
                bank.stream_push_some_dev(ids, chunk.data_ptr(), lg.data_ptr(), 0, stream)
            bnk = timed(step)
            out["route"] = bank.stream_pool_stats()[1]
            bank.stream_close()
            want = None
        if want is not None:                                       # the timed bank call wrote what the separate calls wrote
            torch.cuda.synchronize()
            out["bit_identical"] = bool(torch.equal(want, lg))
        out.update(bank_ms=bnk, separate_ms=sep, frontend_ms=fe_ms)
        print(json.dumps(out), flush=True)
    for m in models.values():
        m.close()


def bank_main(out_path):
    """RNN_REPEATS fresh processes, one after another, every setting in each; per setting the medians of the repeats and their spread
    (max - min, the larger of the two legs), the saving (separate - bank) against the expected (k - 1) x the leader's frontend entry, and
    whether the bank is faster by more than the spread."""
    import subprocess
    runs = []
    for _ in range(RNN_REPEATS):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--bank-child"], env=dict(os.environ), cwd=ROOT,
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"child exited {r.returncode}")
        print(r.stdout.strip(), file=sys.stderr, flush=True)
        runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")])
    lines = []
    for i, (name, work, heads) in enumerate(BANK_SETTINGS):
        rep = {key: [r[i][key] for r in runs] for key in ("bank_ms", "separate_ms", "frontend_ms")}
        med = {key: float(np.median(v)) for key, v in rep.items()}
        spread = max(max(rep[key]) - min(rep[key]) for key in ("bank_ms", "separate_ms"))
        k = len(heads)
        saved, expected = med["separate_ms"] - med["bank_ms"], (k - 1) * med["frontend_ms"]
        line = {"config": f"bank: {name}, 1 s clips, 64 mel, {runs[0][i]['items']} items, ms per call", "workload": work, "members": [h for h, _ in heads],
                "k": k, "warmup": RNN_WARMUP, "steps": RNN_STEPS, "repeats": RNN_REPEATS}
        for key in rep:
            line[key + "_repeats"] = rep[key]
            line[key] = round(med[key], 4)
        line.update(spread_ms=round(spread, 4), saved_ms=round(saved, 4), expected_saving_ms=round(expected, 4),
                    saved_over_expected=round(saved / expected, 3) if expected > 0 else None, bank_wins=bool(saved > spread))
        for key in ("route", "bit_identical"):
            if key in runs[0][i]:
                line[key] = runs[0][i][key] if key == "route" else all(r[i][key] for r in runs)
        lines.append(line)
    text = "".join(json.dumps(l) + "\n" for l in lines)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


MIX_B, MIX_N, MIX_COPY_CEILING = 4096, 16000, 6.29e12          # the measured-copy ceiling in bytes / s


def torch_mix(torch, arena, tab, N):
    """The chain of nww_mix_dev in torch ops on the device, as augment_clips writes it for one clip (float32 means, its own op order):
    arena int16 [samples], tab a dict of [B] device tensors -> int16 [B, N]"""
    i = torch.arange(N, device=arena.device)[None, :]
    j = i - tab["start"][:, None]
    in_fg = (j >= 0) & (j < tab["fg_len"][:, None])
    f = torch.where(in_fg, arena[(tab["fg_off"][:, None] + j.clamp(min=0)).clamp(max=arena.numel() - 1)], 0).to(torch.float32) / 32768.0
    b = arena[tab["bg_off"][:, None] + (tab["bg_start"][:, None] + i) % tab["bg_len"][:, None]].to(torch.float32) / 32768.0
    n = tab["fg_len"][:, None].to(torch.float32)
    eps = torch.finfo(torch.float32).eps
    fr = torch.sqrt((f * f).sum(1, keepdim=True) / n + eps)
    br = torch.sqrt((torch.where(in_fg, b, 0.0) ** 2).sum(1, keepdim=True) / n + eps).clamp(min=0.005)
    scale = tab["snr_linear"][:, None] * br / fr
    srms = torch.sqrt(((f * scale) ** 2).sum(1, keepdim=True) / n + eps)
    scale = torch.where(srms < 0.01, scale * (0.01 / srms), scale)
    y = (b + f * scale) * tab["gain"][:, None]
    pk = y.abs().amax(1, keepdim=True)
    pk = torch.where(pk < 1e-8, torch.ones_like(pk), pk)
    return (torch.clamp(y * (tab["level"][:, None] / pk), -1.0, 1.0) * 32767).to(torch.int16)


def mix_child():
    """One process: MIX_B clips of MIX_N samples out of a device-resident arena of 64 foregrounds of 0.5 - 1 s and 16 backgrounds of 1 - 10 s
    (augment.draw_mix_items, every clip with a background), CNN head.  ms per call as the median of RNN_STEPS device-event timings behind
    RNN_WARMUP warm-up calls, every leg on one stream: (a) mix_dev alone, (b) forward_mixed_dev, (r) forward_pcm_dev on the resident mixed
    clips, (c) the pre-mixed batch copied up from pinned host memory + forward_pcm_dev, (d) the chain in torch ops; and whether (d)'s clips
    are (a)'s to within 1 LSB."""
    import torch
    from nanowakeword_amd.augment import ClipArena, draw_mix_items
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    cfg = HeadConfig("cnn", (101, 64))
    m = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg), window=window, mel_fb=fb)
    rng = np.random.default_rng(7)
    fg_len = rng.integers(MIX_N // 2, MIX_N + 1, 64)
    bg_len = rng.integers(MIX_N, 10 * MIX_N + 1, 16)
    clips = [synth_pcm("speechlike", 1, int(n), seed=100 + k)[0] for k, n in enumerate(fg_len)] + \
            [synth_pcm("noise", 1, int(n), seed=200 + k)[0] for k, n in enumerate(bg_len)]
    arena = ClipArena(clips, device=0)
    items = draw_mix_items(rng, arena, rng.integers(0, 64, MIX_B), 64 + np.arange(16), MIX_N)
    B, N = MIX_B, MIX_N
    ts = torch.cuda.Stream(dev)
    stream = ts.cuda_stream
    m.reserve(B, N)
    pcm = torch.empty((B, N), dtype=torch.int16, device=dev)
    lg, pr = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(2))
    m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream)
    torch.cuda.synchronize()
    pcm_host = pcm.cpu().pin_memory()
    up = torch.empty_like(pcm)
    tab = {k: torch.from_numpy(np.ascontiguousarray(items[k]).astype(np.float32 if items[k].dtype.kind == "f" else np.int64)).to(dev) for k in items.dtype.names}

    def upload_forward():
        with torch.cuda.stream(ts):
            up.copy_(pcm_host, non_blocking=True)
        m.forward_pcm_dev(up.data_ptr(), B, N, lg.data_ptr(), pr.data_ptr(), stream)

    def torch_leg():
        with torch.cuda.stream(ts), torch.no_grad():
            return torch_mix(torch, arena._dev, tab, N)
    legs = {"mix": lambda: m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream),
            "mix_forward": lambda: m.forward_mixed_dev(arena.ptr, arena.samples, items, N, lg.data_ptr(), pr.data_ptr(), stream),
            "resident_forward": lambda: m.forward_pcm_dev(pcm.data_ptr(), B, N, lg.data_ptr(), pr.data_ptr(), stream),
            "upload_forward": upload_forward, "torch_mix": torch_leg}
    # what the passes of mix.hip cost: the same table without peak normalisation (no pass 2), and without backgrounds (no pass 1, half the reads)
    no_peak, no_bg = items.copy(), items.copy()
    no_peak["flags"] = 0
    no_bg["bg_len"] = 0
    legs["mix_no_peak"] = lambda: m.mix_dev(arena.ptr, arena.samples, no_peak, N, pcm.data_ptr(), stream)
    legs["mix_no_background"] = lambda: m.mix_dev(arena.ptr, arena.samples, no_bg, N, pcm.data_ptr(), stream)
    read = int((2 * (2 * items["fg_len"].astype(np.int64) + N)).sum())
    out = {"B": B, "N": N, "arena_samples": arena.samples, "algorithmic_read_bytes": read, "algorithmic_written_bytes": 2 * B * N,
           "batch_bytes": 2 * B * N}
    for name, step in legs.items():
        for _ in range(RNN_WARMUP):
            got = step()
        torch.cuda.synchronize()
        if name == "torch_mix":
            d = (got.to(torch.int32) - pcm.to(torch.int32)).abs()
            out["torch_mix_max_lsb"], out["torch_mix_differing_share"] = int(d.max()), round(float((d > 0).float().mean()), 6)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
        for e0, e1 in ev:
            e0.record(ts); step(); e1.record(ts)
        torch.cuda.synchronize()
        out[name + "_ms"] = round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)
    print(json.dumps(out), flush=True)
    m.close()


def mix_main(out_path):
    """RNN_REPEATS fresh child processes, one after another, each under its own time limit; the medians of the repeats, their spread (max -
    min over the repeats, the largest of the legs compared), and the claim: mixing on the device in front of the head costs less over
    the head on resident PCM than uploading the mixed batch does, by more than the spread."""
    import subprocess
    runs = []
    for _ in range(RNN_REPEATS):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--mix-child"], env=dict(os.environ), cwd=ROOT,
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"mix child exited {r.returncode}")
        runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][0])
    names = ("mix", "mix_forward", "resident_forward", "upload_forward", "torch_mix", "mix_no_peak", "mix_no_background")
    rep = {k: [r[k + "_ms"] for r in runs] for k in names}
    med = {k: float(np.median(v)) for k, v in rep.items()}
    spread = max(max(rep[k]) - min(rep[k]) for k in ("mix_forward", "resident_forward", "upload_forward"))
    first = runs[0]
    moved = first["algorithmic_read_bytes"] + first["algorithmic_written_bytes"]
    line = {"config": f"mix B={MIX_B} N={MIX_N}, foregrounds of 0.5-1 s, device-resident arena, cnn 101x64", "B": MIX_B, "N": MIX_N,
            "warmup": RNN_WARMUP, "steps": RNN_STEPS, "repeats": RNN_REPEATS, "ms_repeats": rep,
            "algorithmic_bytes": moved, "mix_ms": round(med["mix"], 4),
            "mix_fraction_of_copy_ceiling": round(moved / (med["mix"] * 1e-3) / MIX_COPY_CEILING, 3),
            "mix_forward_ms": round(med["mix_forward"], 4), "resident_forward_ms": round(med["resident_forward"], 4),
            "upload_forward_ms": round(med["upload_forward"], 4), "torch_mix_ms": round(med["torch_mix"], 4), "spread_ms": round(spread, 4),
            "mix_over_resident_ms": round(med["mix_forward"] - med["resident_forward"], 4),
            "upload_over_resident_ms": round(med["upload_forward"] - med["resident_forward"], 4),
            "mix_costs_less_than_upload": bool((med["upload_forward"] - med["mix_forward"]) > spread),
            "clips_per_s": {k: round(MIX_B / (med[k] * 1e-3)) for k in ("mix_forward", "resident_forward", "upload_forward")},
            "torch_mix_over_mix": round(med["torch_mix"] / med["mix"], 1),
            "mix_without_peak_pass_ms": round(med["mix_no_peak"], 4), "mix_without_backgrounds_ms": round(med["mix_no_background"], 4),
            "torch_mix_max_lsb": first["torch_mix_max_lsb"], "torch_mix_differing_share": first["torch_mix_differing_share"]}
    text = json.dumps(line) + "\n"
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


def mix_rir_child():
    """One process: mix_child's arena and table, every clip with a response drawn from 64 of 0.25 - 1 s (exponentially decaying noise,
    energy-normalised), M = 32768.  ms per call as the median of RNN_STEPS device-event timings behind RNN_WARMUP warm-up calls, every leg
    on one stream: (a) mix_dev with responses alone, (b) forward_mixed_dev with them, (r) forward_mixed_dev without - the parent's
    number -, (d) the reference's route in torch ops on the same card: rfft / irfft at n = N + L_max - 1 on a resident float32 batch of
    the same shape against the 64 responses' spectra (prepared once, as ours are, and gathered per clip), cut to N, then the peak /
    level / clamp / int16 tail."""
    import torch
    from nanowakeword_amd.augment import ClipArena, IrArena, draw_mix_items, draw_rir_ids
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    cfg = HeadConfig("cnn", (101, 64))
    m = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg), window=window, mel_fb=fb)
    rng = np.random.default_rng(7)
    fg_len = rng.integers(MIX_N // 2, MIX_N + 1, 64)
    bg_len = rng.integers(MIX_N, 10 * MIX_N + 1, 16)
    clips = [synth_pcm("speechlike", 1, int(n), seed=100 + k)[0] for k, n in enumerate(fg_len)] + \
            [synth_pcm("noise", 1, int(n), seed=200 + k)[0] for k, n in enumerate(bg_len)]
    arena = ClipArena(clips, device=0)
    items = draw_mix_items(rng, arena, rng.integers(0, 64, MIX_B), 64 + np.arange(16), MIX_N)
    ir_len = rng.integers(MIX_N // 4, MIX_N + 1, 64)
    responses = [(rng.standard_normal(int(L)) * np.exp(-6.0 * np.arange(int(L)) / int(L))).astype(np.float32) for L in ir_len]
    irs = IrArena(responses, MIX_N, device=0, normalize="energy").prepare(m)
    ids = draw_rir_ids(rng, 64, MIX_B, 1.0)
    B, N = MIX_B, MIX_N
    ts = torch.cuda.Stream(dev)
    stream = ts.cuda_stream
    m.reserve(B, N)
    pcm = torch.empty((B, N), dtype=torch.int16, device=dev)
    lg, pr = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(2))
    # (d)'s inputs, resident: a float32 batch, the responses' spectra at n, the ids and levels
    m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream)
    torch.cuda.synchronize()
    y = pcm.to(torch.float32) / 32768.0
    Lmax = int(ir_len.max())
    n = N + Lmax - 1
    hp = np.zeros((64, Lmax), np.float32)
    for k in range(64):
        hp[k, :irs.lengths[k]] = irs.host[irs.offsets[k]:irs.offsets[k] + irs.lengths[k]]
    Hs = torch.fft.rfft(torch.from_numpy(hp).to(dev), n=n)
    tid = torch.from_numpy(ids.astype(np.int64)).to(dev)
    level = torch.from_numpy(np.ascontiguousarray(items["level"])).to(dev)[:, None]

    def torch_leg():
        with torch.cuda.stream(ts), torch.no_grad():
            w = torch.fft.irfft(torch.fft.rfft(y, n=n) * Hs[tid], n=n)[:, :N]
            pk = w.abs().amax(1, keepdim=True)
            pk = torch.where(pk < 1e-8, torch.ones_like(pk), pk)
            return (torch.clamp(w * (level / pk), -1.0, 1.0) * 32767).to(torch.int16)
    legs = {"mix_rir": lambda: m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream, irs=irs, ir_ids=ids),
            "mix_rir_forward": lambda: m.forward_mixed_dev(arena.ptr, arena.samples, items, N, lg.data_ptr(), pr.data_ptr(), stream, irs=irs, ir_ids=ids),
            "mix_forward": lambda: m.forward_mixed_dev(arena.ptr, arena.samples, items, N, lg.data_ptr(), pr.data_ptr(), stream),
            "mix": lambda: m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream),
            "torch_fft": torch_leg}
    out = {"B": B, "N": N, "M": irs.M, "responses": 64, "ir_len_min": int(ir_len.min()), "ir_len_max": Lmax, "torch_fft_n": n}
    for name, step in legs.items():
        for _ in range(RNN_WARMUP):
            step()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
        for e0, e1 in ev:
            e0.record(ts); step(); e1.record(ts)
        torch.cuda.synchronize()
        out[name + "_ms"] = round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)
    print(json.dumps(out), flush=True)
    m.close()


def mix_rir_main(out_path):
    """RNN_REPEATS fresh child processes, one after another, each under its own time limit; the medians of the repeats with their spread
    (max - min over the repeats).  No claim is asserted: (a) against (d) and (b) against (r) are written down as measured."""
    import subprocess
    runs = []
    for _ in range(RNN_REPEATS):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--mix-rir-child"], env=dict(os.environ), cwd=ROOT,
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"mix-rir child exited {r.returncode}")
        runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][0])
    names = ("mix_rir", "mix_rir_forward", "mix_forward", "mix", "torch_fft")
    rep = {k: [r[k + "_ms"] for r in runs] for k in names}
    med = {k: float(np.median(v)) for k, v in rep.items()}
    first = runs[0]
    line = {"config": f"mix-rir B={MIX_B} N={MIX_N}, every clip through one of 64 responses of 0.25-1 s, M={first['M']}, cnn 101x64", "B": MIX_B,
            "N": MIX_N, "M": first["M"], "warmup": RNN_WARMUP, "steps": RNN_STEPS, "repeats": RNN_REPEATS, "ms_repeats": rep,
            "spread_ms": {k: round(max(v) - min(v), 4) for k, v in rep.items()},
            "mix_rir_ms": round(med["mix_rir"], 4), "torch_fft_ms": round(med["torch_fft"], 4), "torch_fft_n": first["torch_fft_n"],
            "torch_fft_over_mix_rir": round(med["torch_fft"] / med["mix_rir"], 2),
            "mix_rir_forward_ms": round(med["mix_rir_forward"], 4), "mix_forward_ms": round(med["mix_forward"], 4), "mix_ms": round(med["mix"], 4),
            "rir_over_mix_forward_ms": round(med["mix_rir_forward"] - med["mix_forward"], 4),
            "clips_per_s": {k: round(MIX_B / (med[k] * 1e-3)) for k in ("mix_rir", "mix_rir_forward", "mix_forward")}}
    text = json.dumps(line) + "\n"
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


def torch_pitch_shift(torch, y, p, q, win, taps):
    """The definition of nww_mix_aug_*'s pitch shift (include/nww.h) in float32 torch ops on a batch y [b, N] at ONE ratio p / q:
    torch.stft, the textbook vocoder (angle, wrap, cumsum, polar), torch.istft, and the resampler as one conv1d of q output channels -
    channel phi holds phase phi's taps behind (phi p) div q zeros - at stride p, the channels interleaved.  taps: float32 [q, 16]."""
    F = torch.nn.functional
    b, N = y.shape
    X = torch.stft(y, 512, 128, window=win, center=True, pad_mode="reflect", return_complex=True)       # [b, 257, T]
    T = X.shape[2]
    T_out = -(-T * p // q)
    t = torch.arange(T_out, device=y.device)
    i, alpha = (t * q) // p, ((t * q) % p).to(torch.float32) / p
    Xz = F.pad(X, (0, 2))
    X0, X1 = Xz[:, :, i], Xz[:, :, i + 1]
    mag = alpha * X1.abs() + (1.0 - alpha) * X0.abs()
    adv = torch.linspace(0, np.pi * 128, 257, device=y.device)[None, :, None]
    d = X1.angle() - X0.angle() - adv
    d = d - 2 * np.pi * torch.round(d / (2 * np.pi)) + adv
    phase = torch.cumsum(torch.cat([X[:, :, :1].angle(), d[:, :, :-1]], dim=2), dim=2)
    s = torch.istft(torch.polar(mag, phase), 512, 128, window=win, center=True)                       # [b, 128 (T_out - 1)]
    S = s.shape[1]
    a = (torch.arange(q) * p) // q
    w = torch.zeros((q, 1, p + 16), dtype=torch.float32, device=y.device)
    for phi in range(q):
        w[phi, 0, int(a[phi]):int(a[phi]) + 16] = taps[phi]
    m = -(-N // q)
    need = (m - 1) * p + p + 16
    sp = F.pad(s, (7, max(need - S - 7, 0)))[:, None, :]
    out = F.conv1d(sp, w, stride=p)[:, :, :m].transpose(1, 2).reshape(b, -1)[:, :N]
    Ly = -(-S * q // p)
    if Ly < N:
        out = torch.cat([out[:, :Ly], torch.zeros((b, N - Ly), dtype=out.dtype, device=out.device)], dim=1)
    return out


def mix_pitch_child():
    """One process: mix_child's arena and table; half the clips draw one of 64 of augment.pitch_ratios() (the 64 nearest 1 of its 72: a
    model holds at most 64), as the reference shifts half its clips.  ms per call as the median of RNN_STEPS device-event timings behind
    RNN_WARMUP warm-up calls, every leg on one stream: (a) mix_dev with the ratios alone, (b) forward_mixed_dev with them, (r)
    forward_mixed_dev and mix_dev without, (s) forward_pcm_dev on the resident clips, (d) the same definition in torch ops on the same
    card on a resident float32 batch of the shifted clips, ratio by ratio (torch_pitch_shift), plus the peak / level / clamp / int16 tail
    over the batch.  (d) starts from the int16 clips of (r) as floats, so its samples are not compared with (a)'s here: torch_pitch_shift is
    the float32 yardstick of tests/pitch_oracle.py batched, and as far from the float64 definition as that yardstick is (1e-4 .. 2e-3 on
    its clips, the float32 angle sums' error)."""
    import torch
    from nanowakeword_amd.augment import ClipArena, PitchBank, draw_mix_items, draw_pitch_ids, pitch_ratios
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pitch_oracle
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    cfg = HeadConfig("cnn", (101, 64))
    m = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg), window=window, mel_fb=fb)
    rng = np.random.default_rng(7)
    fg_len = rng.integers(MIX_N // 2, MIX_N + 1, 64)
    bg_len = rng.integers(MIX_N, 10 * MIX_N + 1, 16)
    clips = [synth_pcm("speechlike", 1, int(n), seed=100 + k)[0] for k, n in enumerate(fg_len)] + \
            [synth_pcm("noise", 1, int(n), seed=200 + k)[0] for k, n in enumerate(bg_len)]
    arena = ClipArena(clips, device=0)
    items = draw_mix_items(rng, arena, rng.integers(0, 64, MIX_B), 64 + np.arange(16), MIX_N)
    ratios = sorted(sorted(pitch_ratios(), key=lambda r: abs(np.log(r[0] / r[1])))[:64], key=lambda r: r[0] / r[1])
    bank = PitchBank(ratios).prepare(m)
    ids = draw_pitch_ids(rng, len(ratios), MIX_B, 0.5)
    B, N = MIX_B, MIX_N
    ts = torch.cuda.Stream(dev)
    stream = ts.cuda_stream
    m.reserve(B, N)
    pcm, plain = (torch.empty((B, N), dtype=torch.int16, device=dev) for _ in range(2))
    lg, pr = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(2))
    m.mix_dev(arena.ptr, arena.samples, items, N, plain.data_ptr(), stream)
    torch.cuda.synchronize()
    # (d)'s inputs, resident: the float32 clips, the rows of every ratio, its taps, the levels
    y = plain.to(torch.float32) / 32768.0
    win = torch.hann_window(512, periodic=True, device=dev)
    groups = [(p, q, torch.from_numpy(np.flatnonzero(ids == k)).to(dev), torch.from_numpy(pitch_oracle.resample_table(p, q)).to(dev))
              for k, (p, q) in enumerate(ratios) if (ids == k).any()]
    level = torch.from_numpy(np.ascontiguousarray(items["level"])).to(dev)[:, None]

    def torch_leg():
        with torch.cuda.stream(ts), torch.no_grad():
            w = y.clone()
            for p, q, rows, taps in groups:
                w[rows] = torch_pitch_shift(torch, y[rows], p, q, win, taps)
            pk = w.abs().amax(1, keepdim=True)
            pk = torch.where(pk < 1e-8, torch.ones_like(pk), pk)
            return (torch.clamp(w * (level / pk), -1.0, 1.0) * 32767).to(torch.int16)
    legs = {"mix_aug": lambda: m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream, pitch=bank, pitch_ids=ids),
            "mix_aug_forward": lambda: m.forward_mixed_dev(arena.ptr, arena.samples, items, N, lg.data_ptr(), pr.data_ptr(), stream, pitch=bank,
                                                           pitch_ids=ids),
            "mix_forward": lambda: m.forward_mixed_dev(arena.ptr, arena.samples, items, N, lg.data_ptr(), pr.data_ptr(), stream),
            "resident_forward": lambda: m.forward_pcm_dev(plain.data_ptr(), B, N, lg.data_ptr(), pr.data_ptr(), stream),
            "mix": lambda: m.mix_dev(arena.ptr, arena.samples, items, N, plain.data_ptr(), stream),
            "torch_pitch": torch_leg}
    out = {"B": B, "N": N, "ratios": len(ratios), "shifted": int((ids >= 0).sum()), "ratios_drawn": len(groups)}
    steps = {"torch_pitch": max(RNN_STEPS // 10, 5)}                    # hundreds of launches a call: fewer timed calls say the same
    for name, step in legs.items():
        for _ in range(RNN_WARMUP if name != "torch_pitch" else 2):
            step()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps.get(name, RNN_STEPS))]
        for e0, e1 in ev:
            e0.record(ts); step(); e1.record(ts)
        torch.cuda.synchronize()
        out[name + "_ms"] = round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)
    print(json.dumps(out), flush=True)
    m.close()


def mix_pitch_main(out_path):
    """RNN_REPEATS fresh child processes, one after another, each under its own time limit; the medians of the repeats with their spread
    (max - min over the repeats).  No claim is asserted: every ratio is written down as measured."""
    import subprocess
    runs = []
    for _ in range(RNN_REPEATS):
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--mix-pitch-child"], env=dict(os.environ),
                           cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"mix-pitch child exited {r.returncode}")
        runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][0])
    names = ("mix_aug", "mix_aug_forward", "mix_forward", "resident_forward", "mix", "torch_pitch")
    rep = {k: [r[k + "_ms"] for r in runs] for k in names}
    med = {k: float(np.median(v)) for k, v in rep.items()}
    first = runs[0]
    line = {"config": f"mix-pitch B={MIX_B} N={MIX_N}, half the clips shifted by one of {first['ratios']} ratios within +-2 semitones, cnn 101x64",
            "B": MIX_B, "N": MIX_N, "shifted": first["shifted"], "ratios": first["ratios"], "ratios_drawn": first["ratios_drawn"],
            "warmup": RNN_WARMUP, "steps": RNN_STEPS, "repeats": RNN_REPEATS, "ms_repeats": rep,
            "spread_ms": {k: round(max(v) - min(v), 4) for k, v in rep.items()},
            "mix_aug_ms": round(med["mix_aug"], 4), "mix_ms": round(med["mix"], 4), "mix_aug_over_mix": round(med["mix_aug"] / med["mix"], 1),
            "pitch_us_per_shifted_clip": round((med["mix_aug"] - med["mix"]) / first["shifted"] * 1e3, 3),
            "torch_pitch_ms": round(med["torch_pitch"], 4), "torch_pitch_over_mix_aug": round(med["torch_pitch"] / med["mix_aug"], 2),
            "mix_aug_forward_ms": round(med["mix_aug_forward"], 4), "mix_forward_ms": round(med["mix_forward"], 4),
            "resident_forward_ms": round(med["resident_forward"], 4),
            "pitch_over_mix_forward_ms": round(med["mix_aug_forward"] - med["mix_forward"], 4),
            "mix_aug_forward_over_resident_forward": round(med["mix_aug_forward"] / med["resident_forward"], 2),
            "torch_pitch_steps": max(RNN_STEPS // 10, 5),
            "clips_per_s": {k: round(MIX_B / (med[k] * 1e-3)) for k in ("mix_aug", "mix_aug_forward", "mix_forward", "resident_forward")}}
    text = json.dumps(line) + "\n"
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


RESAMPLE_CORPORA = (("tts", 4096, 22050, 22050, 1), ("backgrounds", 16, 60 * 48000, 48000, 2))      # (name, recordings, frames, Hz, channels)


def resample_child():
    """One process, both corpora of RESAMPLE_CORPORA in turn, int16 noise resident in HBM -> 16 kHz mono int16 in one table per corpus.
    ms per call as the median of RNN_STEPS device-event timings behind RNN_WARMUP warm-up calls, both legs on one stream: (r)
    nww_resample_dev - the host's checks and the table's upload are inside the call - and (c) a device-to-device copy of half the bytes
    (r) reads and writes together, which therefore moves the same bytes."""
    import torch
    from nanowakeword_amd.augment import PCM_S16, RESAMPLE_ITEM, resample_ratio, resampled_length
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipModel
    from nanowakeword_amd.synth import synth_state_dict
    dev = torch.device("cuda", 0)
    cfg = HeadConfig("cnn", (101, 64))
    m = HipModel(cfg, FrontendConfig(), device=0, state_dict=synth_state_dict(cfg))
    ts = torch.cuda.Stream(dev)
    stream = ts.cuda_stream
    out = {}
    for name, n, frames, hz, ch in RESAMPLE_CORPORA:
        p, q = resample_ratio(hz)
        m.resample_set_ratios([p], [q])
        length = resampled_length(frames, hz)
        items = np.zeros(n, RESAMPLE_ITEM)
        items["src_off"], items["dst_off"] = np.arange(n, dtype=np.int64) * frames * ch, np.arange(n, dtype=np.int64) * length
        items["src_frames"], items["channels"], items["rate_id"] = frames, ch, 0
        src_values, dst_values = n * frames * ch, n * length
        src = torch.randint(-20000, 20000, (src_values,), dtype=torch.int16, device=dev)
        dst = torch.empty((dst_values,), dtype=torch.int16, device=dev)
        moved = 2 * (src_values + dst_values)
        a, b = (torch.empty((moved // 2,), dtype=torch.uint8, device=dev) for _ in range(2))

        def copy_leg():
            with torch.cuda.stream(ts):
                b.copy_(a)
        legs = {"resample": lambda: m.resample_dev(src.data_ptr(), src_values, PCM_S16, items, dst.data_ptr(), dst_values, PCM_S16, stream),
                "copy": copy_leg}
        row = {"recordings": n, "frames": frames, "hz": hz, "channels": ch, "ratio": [p, q], "outputs": dst_values, "bytes_moved": moved}
        for leg, step in legs.items():
            for _ in range(RNN_WARMUP):
                step()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
            for e0, e1 in ev:
                e0.record(ts); step(); e1.record(ts)
            torch.cuda.synchronize()
            row[leg + "_ms"] = round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)
        out[name] = row
        del src, dst, a, b
    print(json.dumps(out), flush=True)
    m.close()


def resample_main(out_path):
    """RNN_REPEATS fresh child processes, one after another, each under its own time limit; the medians of the repeats with their spread
    (max - min over the repeats).  No claim is asserted: bytes over time for both legs, and the resampler's as a share of the copy's."""
    import subprocess
    runs = []
    for _ in range(RNN_REPEATS):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--resample-child"], env=dict(os.environ),
                           cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"resample child exited {r.returncode}")
        runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][0])
    line = {"config": "resample to 16 kHz mono int16: 4096 mono clips of 1 s at 22050 Hz; 16 stereo recordings of 60 s at 48 kHz", "warmup": RNN_WARMUP,
            "steps": RNN_STEPS, "repeats": RNN_REPEATS}
    for name, *_ in RESAMPLE_CORPORA:
        first = runs[0][name]
        rep = {k: [r[name][k + "_ms"] for r in runs] for k in ("resample", "copy")}
        med = {k: float(np.median(v)) for k, v in rep.items()}
        line[name] = dict(first, ms_repeats=rep, spread_ms={k: round(max(v) - min(v), 4) for k, v in rep.items()},
                          resample_ms=round(med["resample"], 4), copy_ms=round(med["copy"], 4),
                          resample_bytes_per_s=round(first["bytes_moved"] / (med["resample"] * 1e-3)),
                          copy_bytes_per_s=round(first["bytes_moved"] / (med["copy"] * 1e-3)),
                          share_of_copy=round(med["copy"] / med["resample"], 4),
                          source_seconds_per_s=round(first["recordings"] * first["frames"] / first["hz"] / (med["resample"] * 1e-3)))
    text = json.dumps(line) + "\n"
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


MIX_SEG_N = 32000             # the reference's shortest clip (transform_clips.py: min_allowable_length)


def mix_rir_seg_child():
    """One process: mix_rir_child's workload at clips of 2 s - the same 64 + 16 recordings, foregrounds cut to the clip, 64 responses of
    0.25 - 1 s (4000 .. 16 000 taps: one partition, two segments, so two transforms per clip) on the segmented route.  Legs as there:
    (a) mix_dev with responses alone, (b) forward_mixed_dev with them (cnn 201x64), (r) forward_mixed_dev without, (m) mix_dev without,
    (d) torch.fft.rfft / irfft at n = N + L_max - 1 plus the tail on a resident float32 batch.  (d)'s batch is (m)'s int16 clips as
    floats - levelled and quantised, where (a) convolves the float32 clip before the level - so its samples are not (a)'s:
    torch_fft_max_lsb / torch_fft_differing_share only record that it computes the same convolution to within that quantisation."""
    import torch
    from nanowakeword_amd.augment import RIR_SEGMENTED, ClipArena, IrArena, draw_mix_items, draw_rir_ids, rir_parts
    from nanowakeword_amd.config import FrontendConfig, HeadConfig
    from nanowakeword_amd.session import HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    dev = torch.device("cuda", 0)
    fe = FrontendConfig()
    window, fb = torchaudio_tables(fe)
    B, N = MIX_B, MIX_SEG_N
    cfg = HeadConfig("cnn", (fe.n_frames(N), 64))
    m = HipModel(cfg, fe, device=0, state_dict=synth_state_dict(cfg), window=window, mel_fb=fb)
    rng = np.random.default_rng(7)
    fg_len = rng.integers(N // 2, N + 1, 64)
    bg_len = rng.integers(N, 10 * N + 1, 16)
    clips = [synth_pcm("speechlike", 1, int(n), seed=100 + k)[0] for k, n in enumerate(fg_len)] + \
            [synth_pcm("noise", 1, int(n), seed=200 + k)[0] for k, n in enumerate(bg_len)]
    arena = ClipArena(clips, device=0)
    items = draw_mix_items(rng, arena, rng.integers(0, 64, B), 64 + np.arange(16), N)
    ir_len = rng.integers(4000, 16001, 64)
    responses = [(rng.standard_normal(int(L)) * np.exp(-6.0 * np.arange(int(L)) / int(L))).astype(np.float32) for L in ir_len]
    irs = IrArena(responses, N, device=0, normalize="energy", segmented=True).prepare(m)
    assert irs.M == RIR_SEGMENTED
    ids = draw_rir_ids(rng, 64, B, 1.0)
    Q = -(-N // 16384)
    pairs = int(sum(sum(1 for q in range(Q) for p in range(rir_parts(N, int(ir_len[k]))) if p <= q) for k in ids))
    ts = torch.cuda.Stream(dev)
    stream = ts.cuda_stream
    m.reserve(B, N)
    pcm = torch.empty((B, N), dtype=torch.int16, device=dev)
    lg, pr = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(2))
    m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream)
    torch.cuda.synchronize()
    y = pcm.to(torch.float32) / 32768.0
    Lmax = int(ir_len.max())
    n = N + Lmax - 1
    hp = np.zeros((64, Lmax), np.float32)
    for k in range(64):
        hp[k, :irs.lengths[k]] = irs.host[irs.offsets[k]:irs.offsets[k] + irs.lengths[k]]
    Hs = torch.fft.rfft(torch.from_numpy(hp).to(dev), n=n)
    tid = torch.from_numpy(ids.astype(np.int64)).to(dev)
    level = torch.from_numpy(np.ascontiguousarray(items["level"])).to(dev)[:, None]

    def torch_leg():
        with torch.cuda.stream(ts), torch.no_grad():
            w = torch.fft.irfft(torch.fft.rfft(y, n=n) * Hs[tid], n=n)[:, :N]
            pk = w.abs().amax(1, keepdim=True)
            pk = torch.where(pk < 1e-8, torch.ones_like(pk), pk)
            return (torch.clamp(w * (level / pk), -1.0, 1.0) * 32767).to(torch.int16)
    legs = {"mix_rir_seg": lambda: m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream, irs=irs, ir_ids=ids),
            "mix_rir_seg_forward": lambda: m.forward_mixed_dev(arena.ptr, arena.samples, items, N, lg.data_ptr(), pr.data_ptr(), stream, irs=irs,
                                                               ir_ids=ids),
            "mix_forward": lambda: m.forward_mixed_dev(arena.ptr, arena.samples, items, N, lg.data_ptr(), pr.data_ptr(), stream),
            "mix": lambda: m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream),
            "torch_fft": torch_leg}
    out = {"B": B, "N": N, "M": irs.M, "responses": 64, "ir_len_min": int(ir_len.min()), "ir_len_max": Lmax, "torch_fft_n": n, "segments": Q,
           "transforms": pairs, "scratch_bytes": 4 * B * N + 4 * B * Q}
    for name, step in legs.items():
        for _ in range(RNN_WARMUP):
            got = step()
        torch.cuda.synchronize()
        if name == "torch_fft":                                              # pcm still holds (a)'s clips: legs (r) and (m) ran after it
            m.mix_dev(arena.ptr, arena.samples, items, N, pcm.data_ptr(), stream, irs=irs, ir_ids=ids)
            torch.cuda.synchronize()
            d = (got.to(torch.int32) - pcm.to(torch.int32)).abs()
            out["torch_fft_max_lsb"], out["torch_fft_differing_share"] = int(d.max()), round(float((d > 0).float().mean()), 6)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(RNN_STEPS)]
        for e0, e1 in ev:
            e0.record(ts); step(); e1.record(ts)
        torch.cuda.synchronize()
        out[name + "_ms"] = round(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])), 4)
    print(json.dumps(out), flush=True)
    m.close()


def mix_rir_seg_main(out_path):
    """RNN_REPEATS fresh child processes of the segmented route, then as many of --mix-rir's (the one-workgroup route at clips of 1 s: the
    per-transform yardstick of this session), one after another, each under its own time limit; the medians of the repeats with their
    spread (max - min over the repeats).  No claim is asserted; written down as measured: the segmented call against the torch route and
    whether it beats it by more than the spread, the time per (segment, partition) transform against the one-workgroup route's per clip
    (each of them less the mixing call without responses), and what the float32 scratch - written once and read once - costs at the
    measured copy ceiling as a share of the call."""
    import subprocess

    def repeats(flag, names):
        runs = []
        for _ in range(RNN_REPEATS):
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), flag], env=dict(os.environ), cwd=ROOT,
                               stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                raise SystemExit(f"{flag} exited {r.returncode}")
            runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][0])
        rep = {k: [r[k + "_ms"] for r in runs] for k in names}
        return runs[0], rep, {k: float(np.median(v)) for k, v in rep.items()}
    first, rep, med = repeats("--mix-rir-seg-child", ("mix_rir_seg", "mix_rir_seg_forward", "mix_forward", "mix", "torch_fft"))
    one_first, one_rep, one_med = repeats("--mix-rir-child", ("mix_rir", "mix"))
    spread = {k: round(max(v) - min(v), 4) for k, v in rep.items()}
    per_transform_us = (med["mix_rir_seg"] - med["mix"]) / first["transforms"] * 1e3
    one_per_clip_us = (one_med["mix_rir"] - one_med["mix"]) / one_first["B"] * 1e3
    scratch_ms = 2 * first["scratch_bytes"] / MIX_COPY_CEILING * 1e3
    line = {"config": f"mix-rir-seg B={MIX_B} N={MIX_SEG_N}, every clip through one of 64 responses of 0.25-1 s, segmented route, cnn 201x64", "B": MIX_B,
            "N": MIX_SEG_N, "M": first["M"], "segments": first["segments"], "transforms": first["transforms"], "warmup": RNN_WARMUP,
            "steps": RNN_STEPS, "repeats": RNN_REPEATS, "ms_repeats": rep, "spread_ms": spread,
            "mix_rir_seg_ms": round(med["mix_rir_seg"], 4), "torch_fft_ms": round(med["torch_fft"], 4), "torch_fft_n": first["torch_fft_n"],
            "torch_fft_over_mix_rir_seg": round(med["torch_fft"] / med["mix_rir_seg"], 2),
            "beats_torch_fft_by_more_than_the_spread": bool(med["torch_fft"] - med["mix_rir_seg"] > max(spread["torch_fft"], spread["mix_rir_seg"])),
            "torch_fft_max_lsb": first["torch_fft_max_lsb"], "torch_fft_differing_share": first["torch_fft_differing_share"],
            "mix_rir_seg_forward_ms": round(med["mix_rir_seg_forward"], 4), "mix_forward_ms": round(med["mix_forward"], 4), "mix_ms": round(med["mix"], 4),
            "rir_over_mix_forward_ms": round(med["mix_rir_seg_forward"] - med["mix_forward"], 4),
            "clips_per_s": {k: round(MIX_B / (med[k] * 1e-3)) for k in ("mix_rir_seg", "mix_rir_seg_forward", "mix_forward")},
            "one_workgroup_route": {"N": one_first["N"], "M": one_first["M"], "ms_repeats": one_rep, "mix_rir_ms": round(one_med["mix_rir"], 4),
                                    "mix_ms": round(one_med["mix"], 4)},
            "us_per_transform_segmented": round(per_transform_us, 4), "us_per_clip_one_workgroup": round(one_per_clip_us, 4),
            "transform_cost_ratio": round(per_transform_us / one_per_clip_us, 3),
            "scratch_bytes": first["scratch_bytes"], "scratch_ms_at_copy_ceiling": round(scratch_ms, 4),
            "scratch_share_of_mix_rir_seg": round(scratch_ms / med["mix_rir_seg"], 4)}
    text = json.dumps(line) + "\n"
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


def main():
    if "--resample-child" in sys.argv[1:]:
        return resample_child()
    if "--resample" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--resample"]
        return resample_main(rest[0] if rest else os.path.join(ROOT, "profiles", "resample_bench_configs.jsonl"))
    if "--mix-pitch-child" in sys.argv[1:]:
        return mix_pitch_child()
    if "--mix-pitch" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--mix-pitch"]
        return mix_pitch_main(rest[0] if rest else os.path.join(ROOT, "profiles", "mix_pitch_bench_configs.jsonl"))
    if "--mix-rir-seg-child" in sys.argv[1:]:
        return mix_rir_seg_child()
    if "--mix-rir-seg" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--mix-rir-seg"]
        return mix_rir_seg_main(rest[0] if rest else os.path.join(ROOT, "profiles", "mix_rir_seg_bench_configs.jsonl"))
    if "--mix-rir-child" in sys.argv[1:]:
        return mix_rir_child()
    if "--mix-rir" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--mix-rir"]
        return mix_rir_main(rest[0] if rest else os.path.join(ROOT, "profiles", "mix_rir_bench_configs.jsonl"))
    if "--mix-child" in sys.argv[1:]:
        return mix_child()
    if "--mix" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--mix"]
        return mix_main(rest[0] if rest else os.path.join(ROOT, "profiles", "mix_bench_configs.jsonl"))
    if "--bank-child" in sys.argv[1:]:
        return bank_child()
    if "--bank" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--bank"]
        return bank_main(rest[0] if rest else os.path.join(ROOT, "profiles", "bank_bench_configs.jsonl"))
    if "--cascade-pool-child" in sys.argv[1:]:
        return cascade_pool_child()
    if "--cascade-pool" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--cascade-pool"]
        return cascade_pool_main(rest[0] if rest else os.path.join(ROOT, "profiles", "cascade_pool_bench_configs.jsonl"))
    if "--stream-pool-child" in sys.argv[1:]:
        return stream_pool_child()
    if "--stream-pool" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--stream-pool"]
        return stream_pool_main(rest[0] if rest else os.path.join(ROOT, "profiles", "stream_pool_bench_configs.jsonl"))
    if "--cascade-child" in sys.argv[1:]:
        return cascade_child()
    if "--cascade" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--cascade"]
        return cascade_main(rest[0] if rest else os.path.join(ROOT, "profiles", "cascade_bench_configs.jsonl"))
    if "--rnn-child" in sys.argv[1:]:
        return rnn_child()
    if "--recording-child" in sys.argv[1:]:
        return recording_child()
    if "--recording-raw-child" in sys.argv[1:]:
        return recording_raw_child()
    if "--recording-raw" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--recording-raw"]
        parent = rest.pop(rest.index("--parent") + 1) if "--parent" in rest else None
        rest = [a for a in rest if a != "--parent"]
        return recording_raw_main(rest[0] if rest else os.path.join(ROOT, "profiles", "raw_recording_bench_configs.jsonl"), parent)
    if "--recording" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--recording"]
        return recording_main(rest[0] if rest else os.path.join(ROOT, "profiles", "recording_bench_configs.jsonl"))
    if "--rnn" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--rnn"]
        return rnn_main(rest[0] if rest else os.path.join(ROOT, "profiles", "rnn_bench_configs.jsonl"))
    import torch
    import oracle
    from nanowakeword_amd.config import FrontendConfig, HeadConfig, head_macs
    from nanowakeword_amd.session import HipModel, torchaudio_tables
    from nanowakeword_amd.synth import synth_pcm, synth_state_dict
    oracle_forward = oracle.model_forward
    dev = torch.device("cuda", 0)
    only = sys.argv[1:]
    configs = [
        ("C1 dnn 40-mel no-center B=32", HeadConfig("dnn", (98, 40)), FrontendConfig(n_mels=40, center=False), 32, 200),
        ("C1' dnn 40-mel no-center B=4096", HeadConfig("dnn", (98, 40)), FrontendConfig(n_mels=40, center=False), 4096, 30),
        ("C2 cnn 64-mel B=4096", HeadConfig("cnn", (101, 64)), FrontendConfig(), 4096, 30),
        ("C3 bcresnet 64-mel B=8192/GPU (fp32)", HeadConfig("bcresnet", (101, 64)), FrontendConfig(), 8192, 10),
        ("C3b bcresnet 64-mel B=8192/GPU (bf16 activations)", HeadConfig("bcresnet", (101, 64)), FrontendConfig(), 8192, 10),
        ("C3c bcresnet 64-mel B=8192/GPU (f16 activations)", HeadConfig("bcresnet", (101, 64)), FrontendConfig(), 8192, 10),
        ("C4 crnn-gru 64-mel streaming S=1024 x 125 hops", HeadConfig("crnn", (101, 64)), FrontendConfig(), 1024, 0),
        ("C5 conformer 64-mel B=2048/GPU", HeadConfig("conformer", (101, 64)), FrontendConfig(), 2048, 10),
        ("e2e_dnn 64-mel B=4096", HeadConfig("e2e_dnn", (64, 101)), FrontendConfig(), 4096, 20),
        ("gru 64-mel B=4096", HeadConfig("gru", (101, 64)), FrontendConfig(), 4096, 10),
        ("tcn 64-mel B=4096", HeadConfig("tcn", (101, 64)), FrontendConfig(), 4096, 30),
        ("e_branchformer 64-mel B=2048", HeadConfig("e_branchformer", (101, 64)), FrontendConfig(), 2048, 10),
        ("quartznet 64-mel B=2048", HeadConfig("quartznet", (101, 64)), FrontendConfig(), 2048, 30),
        ("e2e_quartznet 1 s B=2048", HeadConfig("e2e_quartznet", (63, 128)), FrontendConfig(), 2048, 30),
        ("e2e_cnn 1 s B=2048", HeadConfig("e2e_cnn", (250, 64)), FrontendConfig(), 2048, 20),
        # the reference's other activations (model.py:81-87) at speed: each within 1.15 x of its ReLU row
        ("C2-gelu cnn 64-mel B=4096 activation=gelu", HeadConfig("cnn", (101, 64), activation="gelu"), FrontendConfig(), 4096, 30),
        ("C2-silu cnn 64-mel B=4096 activation=silu", HeadConfig("cnn", (101, 64), activation="silu"), FrontendConfig(), 4096, 30),
        ("C3-gelu bcresnet 64-mel B=8192/GPU activation=gelu", HeadConfig("bcresnet", (101, 64), activation="gelu"), FrontendConfig(), 8192, 10),
        ("C3-silu bcresnet 64-mel B=8192/GPU activation=silu", HeadConfig("bcresnet", (101, 64), activation="silu"), FrontendConfig(), 8192, 10),
    ]
    for name, cfg, fe, B, steps in configs:
        if only and not any(o in name for o in only):
            continue
        sd = synth_state_dict(cfg)
        window, fb = torchaudio_tables(fe)
        m = HipModel(cfg, fe, device=0, state_dict=sd, window=window, mel_fb=fb, act_dtype="bf16" if "bf16 activations" in name else "f16" if "f16 activations" in name else None)
        stream = torch.cuda.current_stream(dev).cuda_stream
        out = {"config": name, "head": cfg.model_type, "batch": B, "mmac_per_clip": round(head_macs(cfg) / 1e6, 2)}
        if "streaming" in name:
            S, hop, n_hops = B, 1280, 125
            m.stream_open(S, 16000, hop)
            chunks = torch.from_numpy(synth_pcm("noise", S, hop * 4, seed=1)).to(dev)
            logits = torch.empty(S, dtype=torch.float32, device=dev)
            for i in range(15):                                   # fill the windows (12.5 hops) + warm up
                m.stream_push_dev(chunks[:, (i % 4) * hop:(i % 4 + 1) * hop].contiguous().data_ptr(), logits.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            parts = [chunks[:, k * hop:(k + 1) * hop].contiguous() for k in range(4)]
            t0 = time.perf_counter()
            for i in range(n_hops):
                m.stream_push_dev(parts[i % 4].data_ptr(), logits.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out.update({"hops_per_s_per_stream": round(n_hops / dt, 1), "window_scores_per_s": round(S * n_hops / dt, 1),
                        "realtime_streams_supported": int(S * n_hops / dt / 12.5), "ms_per_hop": round(dt / n_hops * 1e3, 3)})
        else:
            pcm_h = synth_pcm("noise", B, 16000, seed=10)
            pcm = torch.from_numpy(pcm_h).to(dev)
            logits = torch.empty(B, dtype=torch.float32, device=dev)
            m.reserve(B, 16000)
            for _ in range(3):
                m.forward_pcm_dev(pcm.data_ptr(), B, 16000, logits.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            m.set_profiling(True)
            t0 = time.perf_counter()
            for _ in range(steps):
                m.forward_pcm_dev(pcm.data_ptr(), B, 16000, logits.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            prof = m.get_profile()
            m.set_profiling(False)
            out.update({"clips_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 4),
                        "head_tflops": round(2 * head_macs(cfg) * B * steps / dt / 1e12, 2),
                        "kernel_ms": {n: round(ms / max(c, 1), 4) for n, ms, c in prof if c > 0}})
            if cfg.model_type == "e2e_quartznet":
                out.update(raw_frontend_legs(torch, m, cfg, sd, pcm, pcm_h, logits, stream, steps))
                print(json.dumps(out), flush=True)
                m.close()
                continue
            if cfg.model_type == "e2e_cnn":
                out.update(raw_cnn_backbone_legs(torch, m, cfg, sd, pcm, pcm_h, logits, stream, steps))
                print(json.dumps(out), flush=True)
                m.close()
                continue
            n_chk = 8
            lm = oracle.frontend_logmel(pcm_h[:n_chk], window, fb, n_mels=fe.n_mels, center=fe.center)
            if cfg.model_type != "e2e_dnn":
                lm = lm.transpose(0, 2, 1)
            ref = oracle_forward(np.ascontiguousarray(lm), sd, cfg).ravel()
            out["max_abs_dlogit_vs_oracle"] = float(np.abs(logits[:n_chk].cpu().numpy() - ref).max())
            t0 = time.perf_counter(); k = 0
            while time.perf_counter() - t0 < 3.0:
                lm = oracle.frontend_logmel(pcm_h[:32], window, fb, n_mels=fe.n_mels, center=fe.center)
                lm = lm if cfg.model_type == "e2e_dnn" else lm.transpose(0, 2, 1)
                oracle_forward(np.ascontiguousarray(lm), sd, cfg); k += 32
            out["cpu_oracle_clips_per_s"] = round(k / (time.perf_counter() - t0), 1)
        print(json.dumps(out), flush=True)
        m.close()


if __name__ == "__main__":
    main()
