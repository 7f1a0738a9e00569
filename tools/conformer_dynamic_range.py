"""How loud may one frame be?  Conformer head (101, 64) - the attn_x3 route, whose operand rows share ONE power of two per clip - six clips of
synth_features(seed=31), frame [1, 7] times 1e2, 1e3, ... 1e8.  Reference: the same network in float64 (oracle).  Prints, per factor, the
worst |logit - ref64| / max(1, |ref64|) of the default plan, of conv_arith = f32 and of the float32 numpy restatement, and the first factor
at which the default plan leaves LOGIT_ATOL (1e-4).  NWW_ATTN_FUSED=0 in the environment measures the three-launch path instead."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import oracle
from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.session import HipModel
from nanowakeword_amd.synth import synth_features, synth_state_dict

LOGIT_ATOL = 1e-4
cfg = HeadConfig("conformer", (101, 64))
sd = synth_state_dict(cfg)
base = synth_features(6, cfg.input_shape, seed=31)
models = {"default": HipModel(cfg, FrontendConfig(), state_dict=sd), "f32": HipModel(cfg, FrontendConfig(), state_dict=sd, conv_arith="f32")}
print("attention route:", [l.split(":")[0] for l in models["default"].describe_plan().split("\n") if "attn_x3" in l or "mha_" in l])
print("| factor | default plan | conv_arith f32 | float32 numpy | ref64 of clip 1 |")
print("|---|---|---|---|---|")
first_out = None
for p in range(2, 9):
    x = base.copy()
    x[1, 7] *= np.float32(10.0 ** p)
    ref = oracle.model_forward(x, sd, cfg, dtype=np.float64).ravel()
    den = np.maximum(1.0, np.abs(ref))
    with np.errstate(invalid="ignore", over="ignore"):
        err = {k: float(np.nan_to_num(np.abs(m.forward_features(x)[0] - ref) / den, nan=np.inf).max()) for k, m in models.items()}
        err["numpy"] = float(np.nan_to_num(np.abs(oracle.model_forward(x, sd, cfg).ravel() - ref) / den, nan=np.inf).max())
    if first_out is None and not err["default"] <= LOGIT_ATOL:
        first_out = p
    print(f"| 1e{p} | {err['default']:.2e} | {err['f32']:.2e} | {err['numpy']:.2e} | {ref[1]:.4f} |")
for m in models.values():
    m.close()
print("first factor outside LOGIT_ATOL x max(1, |ref|):", "none up to 1e8" if first_out is None else f"1e{first_out}")
