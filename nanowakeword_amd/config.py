"""Head / frontend configuration and the state_dict key+shape specification.

The hot path accepts exactly the hyper-parameters the reference's ``Model``
factory reads for the in-scope heads (reference: nanowakeword/modules/model.py:67-296)
and the frontend parameters of ``E2E_MelSpectrogram_CNN``'s ``T.MelSpectrogram``
(reference: nanowakeword/modules/architectures.py:830-837).

``param_spec`` lists every tensor of ``Model.state_dict()`` (minus
``num_batches_tracked``) for a head, with the same keys, so that a reference
``state_dict`` can be fed to ``nww_load_tensor`` unchanged.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass, field, asdict
from typing import Dict, List, Optional, Tuple

HEAD_TYPES = ("dnn", "cnn", "crnn", "gru", "bcresnet", "conformer", "e2e_dnn", "transformer", "tcn", "e_branchformer",
              "quartznet", "e2e_quartznet", "rnn", "e2e_cnn")
ACTIVATIONS = ("relu", "gelu", "silu")

# integer codes shared with include/nww.h
HEAD_CODE = {"dnn": 0, "cnn": 1, "crnn": 2, "gru": 3, "bcresnet": 4, "conformer": 5, "e2e_dnn": 6, "transformer": 7, "tcn": 8,
             "e_branchformer": 9, "quartznet": 10, "e2e_quartznet": 11, "rnn": 12, "e2e_cnn": 13}
# RNNModel's nn.LSTM has a fixed hidden size (architectures.py:152-154); layer_dim is not read
RNN_HIDDEN = 64
ACT_CODE = {"relu": 0, "gelu": 1, "silu": 2}
# nww_config carries at most 4 [channels, kernel, repetitions] entries of a QuartzNet and the planner at most 16 blocks
QUARTZNET_MAX_ENTRIES, QUARTZNET_MAX_BLOCKS = 4, 16
# RawAudioFrontend (architectures.py:692-710): stage 0 is Conv1d(k 41, stride 16, pad 20), every later stage Conv1d(k 13, stride 4, pad 6)
RAW_FRONTEND_MAX_DEPTH, RAW_FRONTEND_MAX_WIDTH = 4, 512
# the raw-PCM heads (mode="e2e" on learned filters): RawAudioFrontend, then a backbone on its output
RAW_HEADS = ("e2e_quartznet", "e2e_cnn")
# RawAudioBackbone (architectures.py:739-762): (Cin, Cout, stride over the image's H, stride over its W) of conv1..conv4; each is
# Conv2d(3x3, pad 1, no bias) + BatchNorm2d + the activation, then the global mean and Linear(96, E)
RAW_CNN_LAYERS = ((1, 24, 1, 2), (24, 48, 2, 2), (48, 64, 2, 2), (64, 96, 1, 1))
# rows of the Transformer's positional-encoding buffer (PositionalEncoding(max_len=5000), architectures.py:31)
PE_MAX_LEN = 5000


@dataclass
class FrontendConfig:
    """STFT -> mel -> dB parameters (torchaudio MelSpectrogram/AmplitudeToDB semantics)."""
    sample_rate: int = 16000
    n_fft: int = 400
    win_length: int = 400
    hop_length: int = 160
    n_mels: int = 64
    center: bool = True          # reflect-pad n_fft//2 each side (reference e2e path)
    f_min: float = 0.0
    f_max: float = 8000.0
    amin: float = 1e-10          # AmplitudeToDB clamp floor
    db_multiplier: float = 10.0  # stype="power"

    def n_frames(self, n_samples: int) -> int:
        """Frame law (bit-exact requirement). center: 1+N//hop ; else 1+(N-n_fft)//hop."""
        if self.center:
            if n_samples <= self.n_fft // 2:
                raise ValueError("reflect padding needs more than n_fft//2 samples")
            return 1 + n_samples // self.hop_length
        if n_samples < self.n_fft:
            raise ValueError(f"clip shorter than n_fft={self.n_fft} samples")
        return 1 + (n_samples - self.n_fft) // self.hop_length


@dataclass
class HeadConfig:
    """Mirror of the kwargs/config keys Model() reads (model.py:68-69,81-90,212-261)."""
    model_type: str = "dnn"
    input_shape: Tuple[int, int] = (16, 96)   # (T, F) as the reference's input_shape
    layer_dim: int = 128
    n_blocks: int = 1
    embedding_dim: int = 64
    activation: str = "relu"
    crnn_cnn_channels: List[int] = field(default_factory=lambda: [16, 32, 32])
    crnn_rnn_type: str = "gru"
    conformer_d_model: int = 144
    conformer_n_head: int = 4
    transformer_d_model: int = 128     # model.py:200-201 config keys of the Transformer head
    transformer_n_head: int = 4
    tcn_channels: List[int] = field(default_factory=lambda: [64, 64, 128])   # model.py:228-229 config keys of the TCN head
    tcn_kernel_size: int = 3
    branchformer_d_model: int = 144    # model.py:263-274 config keys of the E-Branchformer head
    branchformer_n_head: int = 4
    # model.py:239-248 config key of the QuartzNet head: [[channels, kernel, repetitions], ...]
    quartznet_config: List[List[int]] = field(default_factory=lambda: [[256, 33, 1], [256, 33, 1], [512, 39, 1]])
    # model.py:99-100,119-132 config keys of the raw-PCM heads (mode="e2e"); depth None is the model type's own default (3 for e2e_quartznet, 2 for e2e_cnn)
    e2e_frontend_channels: int = 32
    e2e_frontend_depth: Optional[int] = None
    e2e_quartznet_config: List[List[int]] = field(default_factory=lambda: [[64, 11, 1], [64, 13, 1], [64, 17, 1]])

    def __post_init__(self):
        self.model_type = self.model_type.lower()
        self.activation = self.activation.lower()
        self.input_shape = tuple(int(v) for v in self.input_shape)
        if self.model_type not in HEAD_TYPES:
            raise ValueError(f"Unsupported model_type: '{self.model_type}'.")
        if self.activation not in ACTIVATIONS:
            # the reference silently falls back to ReLU (model.py:86-87)
            self.activation = "relu"
        # CRNNModel: 'gru' -> nn.GRU, anything else -> nn.LSTM (architectures.py:238-254); the reference's default
        # config value is "lstm" (model.py:214), BASELINE config 4 names the GRU - HeadConfig defaults to the latter
        self.crnn_rnn_type = "gru" if str(self.crnn_rnn_type).lower() == "gru" else "lstm"
        self.tcn_channels = [int(v) for v in self.tcn_channels]
        self.tcn_kernel_size = int(self.tcn_kernel_size)
        if self.model_type == "tcn":
            # nww_config carries at most 4 levels; kernel size 1 breaks the reference (its chomp out[:, :, :-0] is empty)
            if not 1 <= len(self.tcn_channels) <= 4:
                raise ValueError(f"tcn_channels must have 1..4 levels (got {len(self.tcn_channels)})")
            if any(c <= 0 for c in self.tcn_channels):
                raise ValueError(f"tcn_channels must be positive (got {self.tcn_channels})")
            if self.tcn_kernel_size < 2:
                raise ValueError(f"tcn_kernel_size must be >= 2 (got {self.tcn_kernel_size})")

        self.branchformer_d_model, self.branchformer_n_head = int(self.branchformer_d_model), int(self.branchformer_n_head)
        if self.model_type == "e_branchformer":
            # nn.MultiheadAttention's own requirement (embed_dim divisible by num_heads)
            if self.branchformer_d_model <= 0 or self.branchformer_n_head <= 0 or self.branchformer_d_model % self.branchformer_n_head:
                raise ValueError(f"branchformer_d_model must be divisible by branchformer_n_head "
                                 f"(got {self.branchformer_d_model} / {self.branchformer_n_head})")

        self.quartznet_config = self._quartznet_entries("quartznet_config", self.quartznet_config, self.model_type == "quartznet")
        self.e2e_quartznet_config = self._quartznet_entries("e2e_quartznet_config", self.e2e_quartznet_config, self.model_type == "e2e_quartznet")
        self.e2e_frontend_channels = int(self.e2e_frontend_channels)
        self.e2e_frontend_depth = None if self.e2e_frontend_depth is None else int(self.e2e_frontend_depth)
        if self.model_type in RAW_HEADS:
            depth = raw_frontend_depth(self)
            if not 1 <= depth <= RAW_FRONTEND_MAX_DEPTH:
                raise ValueError(f"e2e_frontend_depth must be 1..{RAW_FRONTEND_MAX_DEPTH} (got {depth})")
            if self.e2e_frontend_channels <= 0:
                raise ValueError(f"e2e_frontend_channels must be positive (got {self.e2e_frontend_channels})")
            width = self.e2e_frontend_channels * 2 ** (depth - 1)
            if width > RAW_FRONTEND_MAX_WIDTH:
                raise ValueError(f"the raw frontend's final width e2e_frontend_channels * 2^(depth - 1) = {width} must be <= {RAW_FRONTEND_MAX_WIDTH}")
            if self.input_shape[1] != width:
                raise ValueError(f"input_shape is what the backbone sees, (rows, {width}) for e2e_frontend_channels = {self.e2e_frontend_channels} "
                                 f"at depth {depth} (got {self.input_shape})")

    @staticmethod
    def _quartznet_entries(name, entries, validate):
        """[[channels, kernel, repetitions], ...] as lists of ints; the limits hold for the head that reads the field."""
        if not validate:
            return [[int(v) for v in e] for e in entries]
        qc = [list(e) for e in entries]
        if not 1 <= len(qc) <= QUARTZNET_MAX_ENTRIES:
            raise ValueError(f"{name} must have 1..{QUARTZNET_MAX_ENTRIES} [channels, kernel, repetitions] entries (got {len(qc)})")
        if any(len(e) != 3 for e in qc):
            raise ValueError(f"{name} entries must be [channels, kernel, repetitions] (got {qc})")
        qc = [[int(v) for v in e] for e in qc]
        if any(c <= 0 for c, _, _ in qc):
            raise ValueError(f"{name} channels must be positive (got {qc})")
        if any(k < 1 or k > 0xFFFF for _, k, _ in qc):
            raise ValueError(f"{name} kernel sizes must be 1..65535 (got {qc})")
        if any(r < 1 for _, _, r in qc):
            raise ValueError(f"{name} repetitions must be >= 1 (got {qc})")
        if sum(r for _, _, r in qc) > QUARTZNET_MAX_BLOCKS:
            raise ValueError(f"{name} expands to {sum(r for _, _, r in qc)} blocks; at most {QUARTZNET_MAX_BLOCKS} are supported")
        return qc

    def to_dict(self):
        return asdict(self)


def quartznet_blocks(cfg: "HeadConfig"):
    """(Cin, Cout, k) of every QuartzNetBlock in order (QuartzNetModel.__init__, architectures.py:410-423)."""
    out, cin = [], cfg.input_shape[1]
    for c, k, r in (cfg.e2e_quartznet_config if cfg.model_type == "e2e_quartznet" else cfg.quartznet_config):
        for _ in range(r):
            out.append((cin, c, k))
            cin = c
    return out


def raw_frontend_depth(cfg: "HeadConfig") -> int:
    """Stages of the raw-PCM frontend: e2e_frontend_depth, or the model type's default (model.py:111, 121)."""
    if cfg.e2e_frontend_depth is None:
        return 2 if cfg.model_type == "e2e_cnn" else 3
    return cfg.e2e_frontend_depth


def raw_cnn_planes(cfg: "HeadConfig"):
    """(H, W) of the RawAudioBackbone's image and of every conv's output: per axis (n - 1) // stride + 1 (3x3, pad 1)."""
    h, w = cfg.input_shape[1], cfg.input_shape[0]        # the image is the frontend's output: channels high, rows wide
    out = [(h, w)]
    for _, _, sh, sw in RAW_CNN_LAYERS:
        h, w = (h - 1) // sh + 1, (w - 1) // sw + 1
        out.append((h, w))
    return out


def raw_frontend_stages(cfg: "HeadConfig"):
    """(Cin, Cout, kernel, stride) of every RawAudioFrontend stage (architectures.py:692-710); padding is kernel // 2 zeros each side."""
    out, cin = [], 1
    for i in range(raw_frontend_depth(cfg)):
        co = cfg.e2e_frontend_channels * 2 ** i
        out.append((cin, co, 41 if i == 0 else 13, 16 if i == 0 else 4))
        cin = co
    return out


def raw_frontend_frames(cfg: "HeadConfig", n_samples: int) -> int:
    """Frame law of the raw frontend (bit-exact requirement): per stage L' = (L - 1) // stride + 1, for any L >= 1."""
    n = int(n_samples)
    if n < 1:
        raise ValueError("a clip needs at least one sample")
    for _, _, _, s in raw_frontend_stages(cfg):
        n = (n - 1) // s + 1
    return n


def recording_windows(n: int, window: int, hop: int, offset: int = 0) -> int:
    """Windows pcm[offset + i * hop : offset + i * hop + window] that fit in a recording of n samples (nww_recording_windows): 0 when
    it is shorter than one window; a trailing partial hop is ignored."""
    n, window, hop, offset = int(n), int(window), int(hop), int(offset)
    if window <= 0 or hop <= 0 or offset < 0:
        raise ValueError("window and hop must be positive and offset non-negative")
    return 0 if n - offset < window else 1 + (n - offset - window) // hop


def cascade_open(gate_probs, gate_threshold: float):
    """Which windows a cascade's gate opens: bool array, False exactly where float(p) < gate_threshold for the float32 probability p
    the gate wrote (the reference's `gate_score_ < gate_threshold`, nanointerpreter.py:660-669, 758-769).  The comparison is made in
    double precision, so a probability equal to the threshold is open, a NaN is open, a threshold <= 0 opens every window and one > 1
    closes every window.  The device's select (cascade.hip) applies the same rule."""
    import numpy as np
    p = np.asarray(gate_probs, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ~(p < float(gate_threshold))


def cascade_pool_open(gate_probs, scored, gate_threshold: float):
    """Which listed streams of a pool call (nww_cascade_stream_push_some) a cascade's gate opens: `scored` [n] bool says whose ring holds
    a window, and only those are candidates for cascade_open's rule - a stream that holds no window is never open, so a threshold <= 0
    opens exactly the scored streams.  The device's pool select (cascade.hip) applies the same rule."""
    import numpy as np
    return np.asarray(scored, dtype=bool) & cascade_open(gate_probs, gate_threshold)


def clip_samples(cfg: "HeadConfig", fe: "FrontendConfig") -> int:
    """The clip length a PCM head was built for, from its input_shape: the whole number of frame hops that gives its frames on the mel
    frontends (16000 for 101 centred frames), every stage's longest input on the raw-PCM heads (16000 for 250 rows at depth 2)."""
    if cfg.model_type in RAW_HEADS:
        n = cfg.input_shape[0]
        for _, _, _, s in reversed(raw_frontend_stages(cfg)):
            n *= s
        return n
    frames = cfg.input_shape[1] if cfg.model_type == "e2e_dnn" else cfg.input_shape[0]
    return (frames - 1) * fe.hop_length + (0 if fe.center else fe.n_fft)


def raw_frontend_macs_upper(cfg: "HeadConfig") -> int:
    """An UPPER estimate of the raw frontend's multiply-accumulates from the config alone: the clip length is not in it, so rows of a stage
    are taken as rows of the next x its stride (1008 and 252 for e2e_quartznet's defaults where a 1 s clip has 1000 and 250: 14.74 against
    14.68 MMAC); raw_frontend_macs(cfg, n_samples) is the exact count for a clip length."""
    m, rows = 0, cfg.input_shape[0]
    for cin, co, k, stride in reversed(raw_frontend_stages(cfg)):
        m += rows * k * cin * co
        rows *= stride
    return m


def raw_frontend_macs(cfg: "HeadConfig", n_samples: int) -> int:
    """Multiply-accumulates of the raw frontend for a clip of n_samples, rows from the frame law."""
    m, n = 0, int(n_samples)
    for cin, co, k, s in raw_frontend_stages(cfg):
        n = (n - 1) // s + 1
        m += n * k * cin * co
    return m


def _bn(spec, prefix, c):
    spec[prefix + ".weight"] = (c,)
    spec[prefix + ".bias"] = (c,)
    spec[prefix + ".running_mean"] = (c,)
    spec[prefix + ".running_var"] = (c,)


def _lin(spec, prefix, out_f, in_f):
    spec[prefix + ".weight"] = (out_f, in_f)
    spec[prefix + ".bias"] = (out_f,)


def _ln(spec, prefix, d):
    spec[prefix + ".weight"] = (d,)
    spec[prefix + ".bias"] = (d,)


def _raw_frontend(spec, cfg):
    """RawAudioFrontend's nn.Sequential: Conv1d (no bias), BatchNorm1d, ReLU per stage."""
    for i, (cin, co, k, _) in enumerate(raw_frontend_stages(cfg)):
        spec[f"model.frontend.conv_blocks.{3*i}.weight"] = (co, cin, k)
        _bn(spec, f"model.frontend.conv_blocks.{3*i+1}", co)


def _gru(spec, prefix, input_size, hidden, n_layers, gates=3):
    """nn.GRU (gates = 3: r, z, n) / nn.LSTM (gates = 4: i, f, g, o) parameter names, bidirectional."""
    for l in range(n_layers):
        isz = input_size if l == 0 else 2 * hidden
        for sfx in ("", "_reverse"):
            spec[f"{prefix}.weight_ih_l{l}{sfx}"] = (gates * hidden, isz)
            spec[f"{prefix}.weight_hh_l{l}{sfx}"] = (gates * hidden, hidden)
            spec[f"{prefix}.bias_ih_l{l}{sfx}"] = (gates * hidden,)
            spec[f"{prefix}.bias_hh_l{l}{sfx}"] = (gates * hidden,)


def crnn_cnn_out(input_shape, channels):
    """(C, H, W) after the CRNN conv stack: each stage MaxPool2d(2) floor mode."""
    h, w = input_shape
    for _ in channels:
        h, w = h // 2, w // 2
    return channels[-1], h, w


def param_spec(cfg: HeadConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """Keys/shapes of Model.state_dict() for the head (num_batches_tracked omitted)."""
    T, F = cfg.input_shape
    L, E, nb = cfg.layer_dim, cfg.embedding_dim, cfg.n_blocks
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    mt = cfg.model_type
    if mt == "dnn":                       # architectures.py:110-126
        _lin(s, "model.layer1", L, T * F)
        _ln(s, "model.layernorm1", L)
        for i in range(nb):
            _lin(s, f"model.blocks.{i}.fcn_layer", L, L)
            _ln(s, f"model.blocks.{i}.layer_norm", L)
        _lin(s, "model.last_layer", E, L)
    elif mt == "cnn":                     # architectures.py:51-80
        s["model.conv1.weight"] = (16, 1, 3, 3); s["model.conv1.bias"] = (16,)
        s["model.conv2.weight"] = (32, 16, 3, 3); s["model.conv2.bias"] = (32,)
        _lin(s, "model.fc1", 128, 32 * (T // 4) * (F // 4))
        _lin(s, "model.fc2", E, 128)
    elif mt == "crnn":                    # architectures.py:209-287
        cin = 1
        for i, c in enumerate(cfg.crnn_cnn_channels):
            s[f"model.cnn.{4*i}.weight"] = (c, cin, 3, 3); s[f"model.cnn.{4*i}.bias"] = (c,)
            _bn(s, f"model.cnn.{4*i+1}", c)
            cin = c
        C, H, W = crnn_cnn_out((T, F), cfg.crnn_cnn_channels)
        _gru(s, "model.rnn", C * H, L, nb, gates=4 if cfg.crnn_rnn_type == "lstm" else 3)
        _lin(s, "model.fc", E, 2 * L)
    elif mt == "gru":                     # architectures.py:129-145
        _gru(s, "model.gru", F, L, nb)
        _lin(s, "model.fc", E, 2 * L)
    elif mt == "rnn":                     # architectures.py:149-161 (RNNModel: bi-LSTM of hidden size 64, layer_dim ignored)
        _gru(s, "model.layer1", F, RNN_HIDDEN, nb, gates=4)
        _lin(s, "model.layer2", E, 2 * RNN_HIDDEN)
    elif mt == "bcresnet":                # architectures.py:620-687
        s["model.init_conv.0.weight"] = (32, 1, 3, 3)
        _bn(s, "model.init_conv.1", 32)
        for i, (ci, co) in enumerate(((32, 64), (64, 128), (128, 256)), start=1):
            s[f"model.block{i}.depthwise.weight"] = (ci, 1, 3, 3)
            s[f"model.block{i}.pointwise.weight"] = (co, ci, 1, 1)
            _bn(s, f"model.block{i}.bn1", co)
            s[f"model.block{i}.shortcut.0.weight"] = (co, ci, 1, 1)
            _bn(s, f"model.block{i}.shortcut.1", co)
        _lin(s, "model.fc", E, 256)
    elif mt == "conformer":               # architectures.py:441-543
        D = cfg.conformer_d_model
        _lin(s, "model.input_proj", D, F)
        for i in range(nb):
            p = f"model.conformer_blocks.{i}"
            for ff in ("ff1", "ff2"):
                _ln(s, f"{p}.{ff}.layer_norm", D)
                _lin(s, f"{p}.{ff}.linear1", 4 * D, D)
                _lin(s, f"{p}.{ff}.linear2", D, 4 * D)
            s[f"{p}.attention.in_proj_weight"] = (3 * D, D)
            s[f"{p}.attention.in_proj_bias"] = (3 * D,)
            _lin(s, f"{p}.attention.out_proj", D, D)
            _ln(s, f"{p}.conv_module.layer_norm", D)
            s[f"{p}.conv_module.conv1.weight"] = (2 * D, D, 1); s[f"{p}.conv_module.conv1.bias"] = (2 * D,)
            s[f"{p}.conv_module.depthwise_conv.weight"] = (D, 1, 31); s[f"{p}.conv_module.depthwise_conv.bias"] = (D,)
            _bn(s, f"{p}.conv_module.batch_norm", D)
            s[f"{p}.conv_module.conv2.weight"] = (D, D, 1); s[f"{p}.conv_module.conv2.bias"] = (D,)
            _ln(s, f"{p}.layer_norm", D)
        _lin(s, "model.output_proj", E, D)
    elif mt == "transformer":             # architectures.py:164-206 (TransformerModel), PositionalEncoding :26-48
        D = cfg.transformer_d_model
        _lin(s, "model.input_proj", D, F)
        s["model.pos_encoder.pe"] = (PE_MAX_LEN, 1, D)
        for i in range(nb):
            p = f"model.transformer_encoder.layers.{i}"
            s[f"{p}.self_attn.in_proj_weight"] = (3 * D, D)
            s[f"{p}.self_attn.in_proj_bias"] = (3 * D,)
            _lin(s, f"{p}.self_attn.out_proj", D, D)
            _lin(s, f"{p}.linear1", 4 * D, D)
            _lin(s, f"{p}.linear2", D, 4 * D)
            _ln(s, f"{p}.norm1", D)
            _ln(s, f"{p}.norm2", D)
        _lin(s, "model.output_proj", E, D)
    elif mt == "e_branchformer":          # architectures.py:546-616 (EBranchformerBlock, EBranchformerModel)
        D = cfg.branchformer_d_model
        _lin(s, "model.input_proj", D, F)
        for i in range(nb):
            p = f"model.branchformer_blocks.{i}"
            _ln(s, f"{p}.attn_branch_norm", D)
            s[f"{p}.attention.in_proj_weight"] = (3 * D, D)
            s[f"{p}.attention.in_proj_bias"] = (3 * D,)
            _lin(s, f"{p}.attention.out_proj", D, D)
            _ln(s, f"{p}.conv_branch.layer_norm", D)
            s[f"{p}.conv_branch.conv1.weight"] = (2 * D, D, 1); s[f"{p}.conv_branch.conv1.bias"] = (2 * D,)
            s[f"{p}.conv_branch.depthwise_conv.weight"] = (D, 1, 31); s[f"{p}.conv_branch.depthwise_conv.bias"] = (D,)
            _bn(s, f"{p}.conv_branch.batch_norm", D)
            s[f"{p}.conv_branch.conv2.weight"] = (D, D, 1); s[f"{p}.conv_branch.conv2.bias"] = (D,)
            _lin(s, f"{p}.merger.gate", D, D)
            _ln(s, f"{p}.final_norm", D)
            _ln(s, f"{p}.ffn.layer_norm", D)
            _lin(s, f"{p}.ffn.linear1", 4 * D, D)
            _lin(s, f"{p}.ffn.linear2", D, 4 * D)
        _lin(s, "model.output_proj", E, D)
    elif mt == "tcn":                     # architectures.py:290-367 (TemporalBlock, TCNModel)
        k, cin = cfg.tcn_kernel_size, F
        for i, co in enumerate(cfg.tcn_channels):
            p = f"model.tcn_blocks.{i}"
            s[f"{p}.conv1.weight"] = (co, cin, k); s[f"{p}.conv1.bias"] = (co,)
            s[f"{p}.conv2.weight"] = (co, co, k); s[f"{p}.conv2.bias"] = (co,)
            if cin != co:                 # the 1x1 downsample exists only when the widths differ
                s[f"{p}.downsample.weight"] = (co, cin, 1); s[f"{p}.downsample.bias"] = (co,)
            cin = co
        _lin(s, "model.fc", E, cin)
    elif mt in ("quartznet", "e2e_quartznet"):   # architectures.py:370-437 (QuartzNetBlock, QuartzNetModel); :798-817 E2ERawQuartzNet
        qp = "model."
        if mt == "e2e_quartznet":
            qp = "model.backbone."
            _raw_frontend(s, cfg)
        for i, (cin, co, k) in enumerate(quartznet_blocks(cfg)):
            p = f"{qp}quartznet_blocks.{i}"
            s[f"{p}.depthwise_conv.weight"] = (cin, 1, k); s[f"{p}.depthwise_conv.bias"] = (cin,)
            s[f"{p}.pointwise_conv.weight"] = (co, cin, 1); s[f"{p}.pointwise_conv.bias"] = (co,)
            _bn(s, f"{p}.batch_norm", co)
            if cin != co:                 # the projected residual exists only when the widths differ
                s[f"{p}.residual_connector.0.weight"] = (co, cin, 1); s[f"{p}.residual_connector.0.bias"] = (co,)
                _bn(s, f"{p}.residual_connector.1", co)
        _lin(s, f"{qp}fc", E, quartznet_blocks(cfg)[-1][1])
    elif mt == "e2e_cnn":                 # architectures.py:739-795 (RawAudioBackbone, E2ERawCNN)
        _raw_frontend(s, cfg)
        for i, (cin, co, _, _) in enumerate(RAW_CNN_LAYERS, start=1):
            s[f"model.backbone.conv{i}.0.weight"] = (co, cin, 3, 3)
            _bn(s, f"model.backbone.conv{i}.1", co)
        _lin(s, "model.backbone.fc", E, 96)
    elif mt == "e2e_dnn":                 # architectures.py:840-865 (E2E_MelSpectrogram_CNN body)
        cin = 1
        for i, c in enumerate((16, 32, 64)):
            s[f"model.conv_block.{4*i}.weight"] = (c, cin, 3, 3); s[f"model.conv_block.{4*i}.bias"] = (c,)
            _bn(s, f"model.conv_block.{4*i+1}", c)
            cin = c
        _lin(s, "model.fc1", 128, 256)
        _bn(s, "model.bn1", 128)
        _lin(s, "model.out", E, 128)
    # Model.classifier: model.py:291-296
    _lin(s, "classifier.0", E // 2, E)
    _lin(s, "classifier.3", 1, E // 2)
    return s


def head_macs(cfg: HeadConfig) -> int:
    """Multiply-accumulates per clip of the head's contractions (SURVEY.md §8a figures)."""
    T, F = cfg.input_shape
    L, E, nb = cfg.layer_dim, cfg.embedding_dim, cfg.n_blocks
    mt = cfg.model_type
    m = E * (E // 2) + E // 2
    if mt == "dnn":
        m += T * F * L + nb * L * L + L * E
    elif mt == "cnn":
        m += 9 * 16 * T * F + 9 * 16 * 32 * (T // 2) * (F // 2) + 32 * (T // 4) * (F // 4) * 128 + 128 * E
    elif mt == "e2e_dnn":
        h, w = T, F   # here input_shape = (n_mels, frames)
        m += 9 * 16 * h * w + 9 * 16 * 32 * (h // 2) * (w // 2) + 9 * 32 * 64 * (h // 4) * (w // 4) + 256 * 128 + 128 * E
    elif mt == "crnn":
        h, w, cin = T, F, 1
        for c in cfg.crnn_cnn_channels:
            m += 9 * cin * c * h * w
            h, w, cin = h // 2, w // 2, c
        I = cin * h
        for l in range(nb):
            isz = I if l == 0 else 2 * L
            steps_rev = w if l < nb - 1 else 1
            ng = 4 if cfg.crnn_rnn_type == "lstm" else 3
            m += w * ng * L * (isz + L) + steps_rev * ng * L * (isz + L)
        m += 2 * L * E
    elif mt == "gru":
        for l in range(nb):
            isz = F if l == 0 else 2 * L
            steps_rev = T if l < nb - 1 else 1
            m += T * 3 * L * (isz + L) + steps_rev * 3 * L * (isz + L)
        m += 2 * L * E
    elif mt == "rnn":
        # the same T + 1-cell count as the GRU head, four gates, hidden size 64
        H = RNN_HIDDEN
        for l in range(nb):
            isz = F if l == 0 else 2 * H
            steps_rev = T if l < nb - 1 else 1
            m += (T + steps_rev) * 4 * H * (isz + H)
        m += 2 * H * E
    elif mt == "bcresnet":
        h, w = T, F
        m += 9 * 32 * h * w
        h, w = h // 2, w // 2
        for ci, co, sh, sw in ((32, 64, 2, 2), (64, 128, 2, 2), (128, 256, 2, 1)):
            ho, wo = (h - 1) // sh + 1, (w - 1) // sw + 1
            m += 9 * ci * ho * wo + 2 * ci * co * ho * wo
            h, w = ho, wo
        m += 256 * E
    elif mt == "conformer":
        D = cfg.conformer_d_model
        m += T * F * D + D * E
        per = 2 * (2 * T * D * 4 * D) + T * 3 * D * D + 2 * T * T * D + T * D * D \
            + T * D * 2 * D + 31 * T * D + T * D * D
        m += nb * per
    elif mt == "transformer":
        D = cfg.transformer_d_model
        m += T * F * D + D * E
        # in_proj, q k^T and (softmax) v, out_proj, linear1, linear2
        per = T * 3 * D * D + 2 * T * T * D + T * D * D + 2 * T * D * 4 * D
        m += nb * per
    elif mt == "e_branchformer":
        D = cfg.branchformer_d_model
        m += T * F * D + D * E
        # per row: in_proj 3 D^2, out_proj D^2, conv1 2 D^2, depthwise 31 D, conv2 D^2, gate D^2, ffn 8 D^2; q k^T and (softmax) v 2 T D
        m += nb * T * (16 * D * D + 31 * D + 2 * T * D)
    elif mt == "tcn":
        # the reference's full-sequence count: conv1, conv2 (and the downsample) at every step, then fc of the last step
        k, cin = cfg.tcn_kernel_size, F
        for co in cfg.tcn_channels:
            m += T * k * cin * co + T * k * co * co + (T * cin * co if cin != co else 0)
            cin = co
        m += cin * E
    elif mt in ("quartznet", "e2e_quartznet"):
        if mt == "e2e_quartznet":
            m += raw_frontend_macs_upper(cfg)
        # per step: depthwise k Cin, pointwise Cin Cout, the projected residual Cin Cout where the widths differ; then fc
        for cin, co, k in quartznet_blocks(cfg):
            m += T * (k * cin + cin * co + (cin * co if cin != co else 0))
        m += quartznet_blocks(cfg)[-1][1] * E
    elif mt == "e2e_cnn":
        # the raw frontend by the same upper estimate as e2e_quartznet's; the backbone exactly: every output pixel of a conv counts all
        # nine taps, as the reference's zero-padded Conv2d does, then fc
        m += raw_frontend_macs_upper(cfg)
        for (cin, co, _, _), (h, w) in zip(RAW_CNN_LAYERS, raw_cnn_planes(cfg)[1:]):
            m += 9 * cin * co * h * w
        m += 96 * E
    return int(m)
