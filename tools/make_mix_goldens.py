"""tests/golden/mix.npz: the reference's own mixing chain on seeded inputs, for tests/test_mix_host.py and tests/test_gpu_mix.py.

Runs only where a checkout of the reference is at hand (--reference, or NWW_REFERENCE); nothing here is needed at test time.  It loads
the reference's nanowakeword/data/augment_clips.py read-only for its ``_mix_snr`` - torch_audiomentations, torchaudio and the package's
logger, which that module imports and ``_mix_snr`` does not use, are stubbed in sys.modules for the import - and follows the module's
own steps around it: the background tiled and cropped to the clip (:201-204), the real-background test and the placement without one
(:218-231), Gain as the multiplication by 10^(dB/20) it is, and the level / clamp / int16 tail (:246-259), all in float32 torch on the
CPU.  The inputs come from tests/mix_oracle.py (golden_arena: integer arithmetic alone), so the file holds only the item table, the
reference's int16 outputs and, as metadata, how the numpy restatement compares with them (the share of differing samples - the test
caps it at 0.5 % - and the largest difference)."""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import mix_oracle  # noqa: E402

N = 16000
SEED = 20240611


def load_mix_snr(ref: str):
    stubs = {}
    for name, attrs in (("torch_audiomentations", ("Compose", "PitchShift", "Gain", "ApplyImpulseResponse")), ("torchaudio", ()),
                        ("nanowakeword", ()), ("nanowakeword.utils", ()), ("nanowakeword.utils.logger", ("print_warning", "print_info"))):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, object)
        stubs[name] = m
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("_ref_augment_clips", os.path.join(ref, "nanowakeword", "data", "augment_clips.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod._mix_snr


def draw_items(offs, lens):
    """40 items over golden_arena's 8 foregrounds and 6 backgrounds: every foreground five times, every background at least five times
    and four items without one; positions, crops, SNRs (5..30 dB), gains (-3..3 dB) and levels (0.5..1) from a seeded generator whose
    draws are stored, not redrawn"""
    rng = np.random.default_rng(SEED)
    nf = len(mix_oracle.GOLDEN_FG)
    rows = []
    for k in range(40):
        f = k % nf
        b = -1 if k % 10 == 9 else nf + (k * 5 + k // nf) % len(mix_oracle.GOLDEN_BG)
        crop = int(rng.integers(0, max(int(lens[f]) - N, 0) + 1))
        fg_len = min(int(lens[f]) - crop, N)
        it = dict(fg_off=int(offs[f]) + crop, fg_len=fg_len, start=int(rng.integers(0, N - fg_len + 1)),
                  snr=10.0 ** (rng.uniform(5.0, 30.0) / 20.0), gain=10.0 ** (rng.uniform(-3.0, 3.0) / 20.0), level=rng.uniform(0.5, 1.0), flags=1)
        if b >= 0:
            L = int(lens[b])
            it.update(bg_off=int(offs[b]), bg_len=L, bg_start=int(rng.integers(0, L)) if L < N else int(rng.integers(0, L - N + 1)))
        rows.append(mix_oracle.item(**it))
    return np.concatenate(rows)


def reference_clip(mix_snr, arena, it):
    import torch
    fg = torch.from_numpy(arena[int(it["fg_off"]):int(it["fg_off"]) + int(it["fg_len"])].astype(np.float32) / np.float32(32768.0))
    L = int(it["bg_len"])
    has_bg = L > 0
    if has_bg:
        bg = torch.from_numpy(arena[int(it["bg_off"]):int(it["bg_off"]) + L].astype(np.float32) / np.float32(32768.0))
        s0 = int(it["bg_start"])
        if len(bg) < N + s0:                                          # tiled, then cropped at s0: sample i is bg[(s0 + i) % L]
            bg = bg.repeat(int(np.ceil((N + s0) / len(bg))))
        bg = bg[s0:s0 + N]
    else:
        bg = torch.zeros(N)
    if has_bg and bg.abs().max() > 1e-4:
        snr_db = 20.0 * np.log10(float(it["snr_linear"]))
        mixed = mix_snr(fg, bg, int(it["start"]), snr_db)
    else:
        mixed = torch.zeros(N)
        mixed[:len(fg)] = fg
    aug = (mixed * torch.tensor(float(it["gain"]), dtype=torch.float32)).reshape(1, 1, N)            # Gain
    level = torch.tensor([float(it["level"])], dtype=torch.float32)
    peaks = torch.max(torch.abs(aug), dim=2, keepdim=True)[0]
    peaks[peaks < 1e-8] = 1.0
    scaled = aug * (level.unsqueeze(1).unsqueeze(2) / peaks)
    final = torch.clamp(scaled, -1.0, 1.0)
    return (final.numpy() * 32767).astype(np.int16).reshape(N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NWW_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "mix.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or NWW_REFERENCE) is needed")
    mix_snr = load_mix_snr(a.reference)
    arena, offs, lens = mix_oracle.golden_arena()
    items = draw_items(offs, lens)
    for it in items:
        assert mix_oracle.bad_field(it, arena.size, N) is None
    ref = np.stack([reference_clip(mix_snr, arena, it) for it in items])
    ours = mix_oracle.mix(arena, items, N)
    d = np.abs(ref.astype(np.int32) - ours.astype(np.int32))
    meta = {"N": N, "items": int(len(items)), "arena_samples": int(arena.size), "arena_sum": int(arena.astype(np.int64).sum()),
            "differing_samples": int((d > 0).sum()), "samples": int(d.size), "differing_share": float((d > 0).mean()), "max_abs_diff": int(d.max()),
            "chain": "augment_clips._mix_snr + Gain + the :246-259 level/clamp/int16 tail, float32 torch on the CPU"}
    np.savez_compressed(a.out, items=items, ref=ref, meta=np.array(json.dumps(meta)))
    print(json.dumps(meta), os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
