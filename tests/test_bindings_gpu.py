"""The ops that take the engine's buffers as one dict (csrc/bindings/torch_ops.cpp: sgd, fc_chain,
wgrad_sgd, backward_fused): what they reject on the host -- a missing, mis-shaped or mis-typed buffer,
an incomplete group, a configuration the launch does not exist in -- is rejected BEFORE anything is
launched (the weights stay bit for bit), and the one-launch backward is one stateless call."""
import pytest
import torch

from dmlc.engine.fused import HAND_WORDS, SEG_OFF, FusedCifarEngine

pytestmark = pytest.mark.gpu


def _engine(B, **kw):
    g = torch.Generator().manual_seed(B)
    n = 2 * B + 16
    data = torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (n,), dtype=torch.int32, generator=g)
    return FusedCifarEngine(B, data, labels, seed=3, lr=1e-4, **kw)


@pytest.fixture(scope="module")
def eng16():
    return _engine(16)              # the smallest kernel batch


def _refresh(eng, buf):
    """ops.sgd in mode 3 (the shadow refresh) on ``buf``."""
    eng.ops.sgd(eng.master, buf, SEG_OFF, eng._sched(), eng.order_desc, 3, 0, True, False, eng.Bv, False)


def _rejected(eng, call, match):
    before = eng.master.clone()
    with pytest.raises(RuntimeError, match=match):
        call()
    torch.cuda.synchronize()
    assert torch.equal(eng.master, before)


def test_missing_key_is_named(eng16):
    buf = {k: t for k, t in eng16.buf.items() if k != "w2f"}
    _rejected(eng16, lambda: _refresh(eng16, buf), r"'w2f'")


def test_wrong_shape_is_named(eng16):
    buf = dict(eng16.buf, w2f=torch.zeros(64, 1599, dtype=torch.bfloat16, device=eng16.device))
    _rejected(eng16, lambda: _refresh(eng16, buf), r"w2f has shape")


def test_wrong_dtype_is_named(eng16):
    buf = dict(eng16.buf, stats=eng16.stats.to(torch.float64))
    _rejected(eng16, lambda: _refresh(eng16, buf), r"stats must be")


def test_master_must_be_the_dicts(eng16):
    _rejected(eng16, lambda: eng16.ops.sgd(eng16.master.clone(), eng16.buf, SEG_OFF, eng16._sched(), eng16.order_desc,
                                           3, 0, True, False, eng16.Bv, False), r"master must be buf")


def test_incomplete_dgrad_group_is_rejected(eng16):
    """The chain's conv2 dgrad needs am2, w2d, dp1 and dy2 together."""
    e = eng16
    buf = {k: t for k, t in e.buf.items() if k != "am2"}
    _rejected(e, lambda: e.ops.fc_chain(e.master, buf, e.bidx, None, 1, SEG_OFF, e._sched(), e.Bv, 1.0 / e.Bv, True,
                                        fuse_sgd=True, dw_tasks=True, dgrad=True, fc_sgd=False), r"'am2'")


def _backward_fused(e, buf):
    e.ops.backward_fused(e.master, buf, e.bidx, None, 1, SEG_OFF, e._sched(), e.order_desc, e.cy, e.cx, e.groups2,
                         e.Bv, 1.0 / e.Bv, e.relu_logits)


def test_backward_fused_unmet_preconditions():
    """g1 + 4 g2 = 144 + 96 != 256: the launcher's own check refuses the role map."""
    e = _engine(144, variant={"bwd_fused": False}, g2=24)
    assert not e.bwd_fused and e.g1 + 4 * e.g2 != 256
    _rejected(e, lambda: _backward_fused(e, e.buf), r"bwd_hand")       # this engine keeps no hand-off words
    buf = dict(e.buf, bwd_hand=torch.zeros(HAND_WORDS, dtype=torch.int32, device=e.device))
    _rejected(e, lambda: _backward_fused(e, buf), r"HIP launch failed")


def test_backward_fused_is_one_stateless_call():
    e = _engine(144)
    assert e.bwd_fused
    for _ in range(2):
        e._forward(e.bidx, None, 1, train=True)
        e._fc_src = None                     # (the engine's own pairing check: the op is called directly)
        _backward_fused(e, e.buf)
    torch.cuda.synchronize()
    e.check_barriers()
    assert e.global_step() == 2 and bool(torch.isfinite(e.master).all())
