"""numpy restatement of the RNN head (model_type="rnn": RNNModel, architectures.py:149-161): a bidirectional nn.LSTM of hidden size 64 over
time, its output at the last frame, Linear(128, E), then the shared classifier.  The recurrence is oracle.heads.bigru_last(lstm=True), which
follows its input's dtype, so the same code is the float32 and the float64 yardstick.  Test helper only: nothing under nanowakeword_amd/
imports it, and oracle.heads._NETS has no entry for this head."""
import numpy as np

from oracle.heads import bigru_last, classify, linear

HIDDEN = 64


def head_forward(x, sd, cfg, dtype=np.float32):
    """features [B,T,F] -> embedding [B,E] in `dtype`."""
    x = np.ascontiguousarray(x, dtype=dtype)
    sd = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    last = bigru_last(x, sd, "model.layer1", cfg.n_blocks, HIDDEN, lstm=True)
    return linear(last, sd["model.layer2.weight"], sd["model.layer2.bias"]).astype(dtype)


def model_forward(x, sd, cfg, dtype=np.float32):
    """features [B,T,F] -> logits [B,1] in `dtype`."""
    return classify(head_forward(x, sd, cfg, dtype), sd, cfg, dtype)
