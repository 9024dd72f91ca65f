"""Exact tests of the conv / pool / argmax / conv-backward kernels (cnn_conv.hip, cnn_split.hip,
conv2_core.h, w1_common.h, wgrad_core.h and the shadow layouts the SGD kernel writes).

The inputs are the integer cases of tests/exact_ref.py: every intermediate value is an integer bf16
holds exactly and every fp32 sum stays below 2^24, so each kernel has to reproduce the fp64 oracle BIT
FOR BIT, element for element -- pooled values, argmax bytes (winner, tie rule, TF-SAME border, the
no-gradient code), the gathered crop, the conv2 input gradient through the flipped ci-major shadow
w2d and the weight / bias gradients.  No tolerance anywhere: every comparison is torch.equal, and a
failure names the image, pooled row / column and channel of the first mismatches.

The whole-tensor 1e-2 norms of tests/test_cnn_kernels_gpu.py cannot see a wrong border column, a wrong
last pooled row, one wrong image or one wrong 8-channel chunk, and nothing else compares the argmax
bytes with anything independent; the bitwise variant-against-variant tests (tests/test_fused_gpu.py,
tests/test_bwd_fused_gpu.py) inherit exactly that strength.  These tests close the gap, and they run
the crop offsets (0, 8) and (8, 0) that no other test passes."""
import json

import pytest
import torch

import exact_ref as X
from dmlc.engine.fused import FusedCifarEngine
from dmlc.models import cifar_cnn as M

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NHWC = ("image", "row", "col", "channel")
HWIO = ("kh", "kw", "ci", "co")


def _where(name, got, want, axes):
    """Where ``got`` differs from ``want``: the count, the extent along every axis and the first few
    mismatches with both values -- a localised bug (one border column, one image, one channel chunk)
    reads straight off the message."""
    bad = (got != want).nonzero()
    lines = [f"{name}: {bad.shape[0]} of {got.numel()} elements differ from the oracle"]
    for k, ax in enumerate(axes):
        u = bad[:, k].unique().tolist()
        lines.append(f"  {ax}s: {u if len(u) <= 12 else f'{len(u)} of {got.shape[k]} ({u[:6]} ... {u[-3:]})'}")
    for i in bad[:8].tolist():
        pos = ", ".join(f"{ax} {v}" for ax, v in zip(axes, i))
        lines.append(f"  {pos}: kernel {got[tuple(i)].item():g}, oracle {want[tuple(i)].item():g}")
    return "\n".join(lines)


class _Tally:
    """Compared-element count of one test, printed (pytest -s) once every comparison passed."""

    def __init__(self, tag):
        self.tag, self.n = tag, {}

    def equal(self, name, got, want, axes=NHWC):
        got = got.detach().cpu()
        got = (got.double() if got.is_floating_point() else got.to(torch.int64)).reshape(want.shape)
        want = want.to(got.dtype)
        assert torch.equal(got, want), _where(f"{self.tag} {name}", got, want, axes)
        self.n[name] = self.n.get(name, 0) + got.numel()

    def write(self):
        assert self.n and all(self.n.values())
        print(json.dumps({"exact": self.tag, "compared": self.n, "compared_total": sum(self.n.values()), "differing": 0}))


def _engine(case, Bv=None, **kw):
    return FusedCifarEngine(Bv or case.B, case.data, case.labels, flat_params=case.flat,
                            crop_offset=(case.cy, case.cx), seed=11, **kw)


def _forward(eng, idx):
    """One training forward (conv part; the fc chain that would follow is dropped) into cleared
    outputs, so nothing a previous launch wrote can pass."""
    eng.p1.fill_(float("nan"))
    eng.p2.fill_(float("nan"))
    eng.am1.fill_(77)
    eng.am2.fill_(77)
    eng._forward(idx, None, 1, train=True)
    eng._reset_step_state()
    torch.cuda.synchronize()
    eng.check_barriers()


def _check_forward(t, eng, case, rows, what):
    """p1 / am1 / p2 / am2 (and the forward's image copy) of dataset rows ``rows`` against the oracle."""
    rows = rows.cpu().long()
    t.equal(f"p1[{what}]", eng.p1, case.p1[rows])
    t.equal(f"am1[{what}]", eng.am1, case.am1[rows])
    t.equal(f"p2[{what}]", eng.p2, case.p2[rows])
    t.equal(f"am2[{what}]", eng.am2, case.am2[rows])
    assert torch.equal(eng.xraw.cpu(), case.data[rows].view(-1, 3072)), f"{t.tag} xraw[{what}]"


# every forward launch the engine can take: constructor arguments and the path they must select
FWD = {
    "conv12": (dict(conv_split=1), lambda e: e.fused_fwd and e.conv_split == 1 and e.xraw_prefetch),
    "conv1_conv2": (dict(conv_split=1, variant={"split_fwd": True}), lambda e: not e.fused_fwd and e.conv_split == 1),
    "conv12_split": (dict(conv_split=2, conv1_split=2), lambda e: e.fwd12_split),
    "conv1_split2_conv2_split": (dict(conv_split=2, conv1_split=2, variant={"fwd12_split": False}),
                                 lambda e: e.conv_split == 2 and e.conv1_split == 2 and not e.fwd12_split),
    "conv1_split4_conv2_split": (dict(conv_split=2, conv1_split=4),
                                 lambda e: e.conv_split == 2 and e.conv1_split == 4 and not e.fwd12_split),
}
# crop (4, 4) for every launch; the corners (0, 8) and (8, 0) for the two one-launch forwards
FWD_CASES = [(name, 0) for name in FWD] + [(name, c) for name in ("conv12", "conv12_split") for c in (1, 2)]


@pytest.mark.parametrize("name,ci", FWD_CASES, ids=[f"{n}-crop{X.GPU_CASES[c][2]}{X.GPU_CASES[c][3]}" for n, c in FWD_CASES])
def test_forward_is_bit_exact(name, ci):
    """B = 16 (one row tile): pooled values and argmax bytes of both layers equal the oracle, through
    the engine's own batch rows (``idx is eng.bidx``: the prefetched xraw path of conv12_fwd) and
    through an explicit index list in another order."""
    case = X.make_exact_case(*X.GPU_CASES[ci])
    kw, selected = FWD[name]
    eng = _engine(case, **kw)
    assert selected(eng), f"{name}: the engine chose another forward path"
    t = _Tally(f"fwd_{name}_crop{case.cy}{case.cx}")
    _forward(eng, eng.bidx)
    _check_forward(t, eng, case, eng.bidx, "bidx")
    perm = torch.randperm(case.B, generator=torch.Generator().manual_seed(5)).to(torch.int32)
    assert not torch.equal(perm, eng.bidx.cpu())
    _forward(eng, eng._padded(perm))
    _check_forward(t, eng, case, perm, "list")
    t.write()


@pytest.mark.parametrize("split", [1, 2])
def test_forward_padded_batch_repeats_last_row(split):
    """Bv = 12 in a kernel batch of 16: rows 0..11 equal the oracle, rows 12..15 -- the padded index
    list repeats the last row -- equal row 11's outputs."""
    case = X.make_exact_case(*X.GPU_CASES[0])
    eng = _engine(case, Bv=12, conv_split=split, conv1_split=2)
    assert (eng.Bv, eng.B) == (12, 16)
    t = _Tally(f"fwd_bv12_split{split}")
    for what, idx in (("bidx", eng.bidx), ("list", eng._padded(torch.tensor([9, 3, 15, 0, 7, 1, 12, 5, 2, 14, 6, 10],
                                                                           dtype=torch.int32)))):
        rows = idx.cpu().long()
        assert rows.numel() == 16 and bool((rows[12:] == rows[11]).all()) and rows[:12].unique().numel() == 12
        _forward(eng, idx)
        _check_forward(t, eng, case, rows, what)
        for buf in (eng.p1, eng.am1, eng.p2, eng.am2):
            assert torch.equal(buf[12:], buf[11:12].expand_as(buf[12:]))
    t.write()


def _backward(t, case, reduce, **kw):
    """The engine's conv backward without the fc chain on the exact forward state: an integer dp2 into
    eng.dp2, then conv2 dgrad + wgrad + the slab reduction; dy2, dp1 and the conv segments of the flat
    gradient must equal the oracle.  ``reduce``: the reduction inside the wgrad launch (the default
    variant), else the wgrad launch + the reduce-only SGD launch (variant wgrad_sgd off)."""
    eng = _engine(case, variant=None if reduce else {"wgrad_sgd": False}, **kw)
    assert eng._grad_in_launch == reduce
    eng.keep_dp1 = True
    B = case.B
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(6)).to(torch.int32)
    ids = eng._padded(perm)
    rows = perm.long()
    _forward(eng, ids)
    _check_forward(t, eng, case, rows, "list")            # the state the backward starts from
    eng.dp2.copy_(case.dp2[rows].to(BF16))
    for buf in (eng.dy2, eng.dp1, eng.grad):
        buf.fill_(float("nan"))                           # every compared element must be written
    if reduce:
        eng._conv_backward(src=(ids, None, 1), reduce=True)
    else:
        eng._conv_backward(src=(ids, None, 1))
        eng._sgd(mode=1)
    torch.cuda.synchronize()
    eng.check_barriers()
    t.equal("dy2", eng.dy2, case.dy2[rows])
    t.equal("dp1", eng.dp1, case.dp1[rows])
    g = M.views(eng.grad)
    t.equal("conv2_kernel grad", g["conv2_kernel"], case.gw2, HWIO)
    t.equal("conv2_bias grad", g["conv2_bias"], case.gb2, ("co",))
    t.equal("conv1_kernel grad", g["conv1_kernel"], case.gw1, HWIO)
    t.equal("conv1_bias grad", g["conv1_bias"], case.gb1, ("co",))
    return eng


@pytest.mark.parametrize("ci", [0, 1], ids=["crop44", "crop08"])
@pytest.mark.parametrize("groups", [None, (5, 3)], ids=["groups-default", "groups-5-3"])
@pytest.mark.parametrize("dsplit", [1, 2])
@pytest.mark.parametrize("reduce", [False, True], ids=["wgrad+sgd", "wgrad_sgd"])
def test_conv_backward_is_bit_exact(reduce, dsplit, groups, ci):
    """B = 16: both conv2 dgrad kernels (one / two workgroups per image), the default image groups and
    an uneven g1 = 5, g2 = 3 (groups of 4, 3, 3, 3, 3 and 6, 5, 5 images), the centre crop and (0, 8)
    for the conv1 weight gradient's image gather."""
    case = X.make_exact_case(*X.GPU_CASES[ci])
    kw = dict(dgrad_split=dsplit)
    if groups:
        kw.update(g1=groups[0], g2=groups[1])
    t = _Tally(f"bwd_{'reduce' if reduce else 'launches'}_d{dsplit}_g{'53' if groups else 'def'}_crop{case.cy}{case.cx}")
    eng = _backward(t, case, reduce, **kw)
    assert eng.dgrad_split == dsplit and (not groups or (eng.g1, eng.g2) == groups)
    t.write()


def test_conv_backward_is_bit_exact_on_the_ragged_256_block_map():
    """B = 144 through the in-launch reduction: 128 conv1 roles over 144 images (16 of them take two)
    and 4 x 32 conv2 roles over groups of 5 and 4 images, the conv1 roles helping the conv2 reduction."""
    case = X.make_exact_case(*X.GPU_CASES[3])
    t = _Tally("bwd_reduce_b144")
    eng = _backward(t, case, True)
    assert (eng.B, eng.g1, eng.g2, eng.conv_split, eng.dgrad_split) == (144, 128, 32, 1, 1)
    t.write()
