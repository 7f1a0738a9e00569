"""The large-batch classifier tail (persistent workgroups, weights in LDS, split-K partials summed in the tail) against the
small-batch kernels it must equal bit for bit (run with -m gpu).

For the CNN head (the tail receives fc1's split-K partials), the GRU head (plain x rows), the Transformer / TCN heads (plain rows
too, K = 128, from mean_finish / tcn_x3, whose grids depend on B), the E-Branchformer (K = 144, rows from the time mean behind ffn_x3) and
QuartzNet (rows from qn_x3 +mean:time, each workgroup walking B / gridDim.x clips; K = 512 at the defaults, beyond the large-batch kernel's
LDS budget, and K = 128 on a one-block configuration, inside it): logits AND embeddings of the first
B clips of one clip set at B in {17, 1024, 1025, 4096, 4099} equal those of the same clips pushed through in batches of 8 (the
deferred-reduce small path) and of 1.  A CNN head whose tail weights exceed the kernel's LDS budget (embedding_dim 256) keeps the
earlier kernel at every batch size: its plan step says so, and the results agree in the same way."""
import numpy as np
import pytest

from nanowakeword_amd.config import FrontendConfig, HeadConfig
from nanowakeword_amd.synth import synth_features, synth_state_dict

pytestmark = pytest.mark.gpu
SIZES = (17, 1024, 1025, 4096, 4099)
NOTE = "(large batches: persistent, weights in LDS)"


@pytest.fixture(scope="module")
def HipModel():
    from nanowakeword_amd.session import HipModel
    return HipModel


def _in_batches(m, x, n):
    lg, pr, em = [], [], []
    for i in range(0, len(x), n):
        l, p, e = m.forward_features(x[i:i + n], return_embedding=True)
        lg.append(l.copy()); pr.append(p.copy()); em.append(e.copy())
    return np.concatenate(lg), np.concatenate(pr), np.concatenate(em)


def _check(HipModel, cfg, sizes, want_batch_kernel):
    sd = synth_state_dict(cfg)
    m = HipModel(cfg, FrontendConfig(), state_dict=sd)
    tail = [s for s in m.describe_plan().strip().split("\n") if "tail:" in s]
    assert len(tail) == 1, tail
    assert (NOTE in tail[0]) == want_batch_kernel, tail
    x = synth_features(max(sizes), cfg.input_shape, seed=11)
    l8, p8, e8 = _in_batches(m, x, 8)
    l1, p1, e1 = _in_batches(m, x, 1)
    assert np.isfinite(l8).all() and np.ptp(l8) > 0.0 and np.ptp(e8) > 0.0
    assert np.array_equal(l8, l1) and np.array_equal(p8, p1) and np.array_equal(e8, e1)
    for B in sizes:
        lg, pr, em = m.forward_features(x[:B], return_embedding=True)
        assert lg.shape == (B,) and em.shape == (B, cfg.embedding_dim)
        assert np.array_equal(lg, l8[:B]), (B, int((lg != l8[:B]).sum()))
        assert np.array_equal(em, e8[:B]), (B, int((em != e8[:B]).sum()))
        assert np.array_equal(pr, p8[:B]), B
    m.close()


# the two newest heads at (16, 96): the tail's operand does not depend on T and the 4099 single-clip calls stay short.  QuartzNet's default tail
# has K = 512: (E + 8) rows of 516 floats alone are 149 KB, past TB_LDS_MAX = 96 KB, so it keeps the earlier kernel at every batch size (as the
# embedding_dim 256 case below); [[128, 33, 1]] (K = 128, 50 KB) has a qn_x3 +mean:time launch feed the persistent kernel
_TAIL_HEADS = [("cnn", (101, 64), {}, True), ("gru", (101, 64), {}, True), ("transformer", (101, 64), {}, True), ("tcn", (101, 64), {}, True),
               ("e_branchformer", (16, 96), {}, True), ("quartznet", (16, 96), {}, False),
               ("quartznet", (16, 96), {"quartznet_config": [[128, 33, 1]]}, True)]


@pytest.mark.parametrize("head,shape,kw,want_batch_kernel", _TAIL_HEADS, ids=[h + ("-128_33_1" if kw else "") for h, _, kw, _ in _TAIL_HEADS])
def test_large_batch_tail_equals_small_batches(HipModel, head, shape, kw, want_batch_kernel):
    _check(HipModel, HeadConfig(head, shape, **kw), SIZES, want_batch_kernel)


def test_tail_weights_beyond_lds_budget_fall_back(HipModel):
    # We = [256][128] floats = 128 KB: beyond what the large-batch kernel stages; the earlier kernel runs, deferred partials included
    _check(HipModel, HeadConfig("cnn", (101, 64), embedding_dim=256), (1025, 4099), False)
