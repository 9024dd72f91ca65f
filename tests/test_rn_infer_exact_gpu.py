"""Bit-exact tests of k_rn_infer (csrc/kernels/resnet_infer.hip), the whole eval-mode ResNet-20 in one
launch, LAYER BY LAYER.

torch.ops.dmlc.rn_infer takes the images, the 19 forward shadows, master / state with offset lists,
idx, labels and the grid as arguments, so every test here is ONE launch on buffers it builds from a
case of tests/rn_exact_ref.py (make_infer_case) and compares with the fp64 oracle infer_exact, which
rounds to bf16 exactly where the kernel stores an operand.  The cases keep every fp32 sum of the kernel
exact in any order (asserted by the oracle per layer, on the CPU), so a correct kernel reproduces the
logits BIT FOR BIT: every comparison is torch.equal and a failure names the case, the image and the
class.

A ``layer`` case puts dense signed weights and a per-channel BatchNorm (sc in {1/2, 1, 2} times a signed
gamma, non-zero shift) on ONE layer and makes every other layer a non-negative carrier that brings data
to all its channels and borders and carries every element of its output to the logits
(tests/test_rn_exact_ref.py proves the latter with autograd); its pytest id names the layer and its
geometry, so a failure localises: a stale halo pixel, a wrong border row of a stride-2 layer, the wrong
half of an option-A shortcut, one BN row at a wrong offset, a rounding of the last layer, a wrong tie
rule.  master and state hold NaN between the (shuffled) tables; logits are pre-filled with NaN, pred
and correct with a sentinel."""
import json

import pytest
import torch

import rn_exact_ref as X
from dmlc.ops import _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7777
_dev_cache = {}


def _ops():
    _ext.hip()
    return torch.ops.dmlc


def _device_case(case):
    """(case, device buffers) -- uploaded once per case for the whole module"""
    if case not in _dev_cache:
        c = X.make_infer_case(*case)
        b = X.infer_buffers(c, case[2])
        wf = [X.shadow_fwd(w.double()).to(torch.bfloat16).to(DEV).contiguous() for w in c.w]
        _dev_cache[case] = (c, b, wf, c.images.to(DEV), c.labels.to(DEV), b.master.to(DEV), b.state.to(DEV))
    return _dev_cache[case]


def _where(tag, name, got, want, rows):
    bad = (got != want).nonzero()
    lines = [f"{tag} {name}: {bad.shape[0]} of {got.numel()} elements differ from the oracle"]
    for i in bad[:10].tolist():
        pos = f"image {i[0]} (data row {rows[i[0]]})" + (f", class {i[1]}" if len(i) > 1 else "")
        lines.append(f"  {pos}: kernel {got[tuple(i)].item():g}, oracle {want[tuple(i)].item():g}")
    return "\n".join(lines)


class _Tally:
    """Compared-element count of one test, printed (pytest -s) once every comparison passed."""

    def __init__(self, tag):
        self.tag, self.n = tag, {}

    def equal(self, name, got, want, rows):
        got = got.detach().cpu()
        got = got.double() if got.is_floating_point() else got.to(torch.int64)
        want = want.to(got.dtype)
        assert got.shape == want.shape and torch.equal(got, want), _where(self.tag, name, got, want, rows)
        self.n[name] = self.n.get(name, 0) + got.numel()

    def write(self):
        assert self.n and all(self.n.values())
        print(json.dumps({"exact": self.tag, "compared": self.n, "compared_total": sum(self.n.values()), "differing": 0}))


def _run(t, case, idx, blocks, nrows=X.INFER_ROWS):
    """One launch on the first ``nrows`` data rows (``idx`` None: all of them, in order) against the
    oracle's rows: logits, pred and correct = (pred == labels[idx])."""
    c, b, wf, images, labels, master, state = _device_case(case)
    rows = list(range(nrows)) if idx is None else list(idx)
    assert all(0 <= r < nrows for r in rows)
    n = len(rows)
    logits = torch.full((n, 10), float("nan"), dtype=torch.float32, device=DEV)
    pred = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    correct = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    idx_t = None if idx is None else torch.tensor(rows, dtype=torch.int32, device=DEV)
    _ops().rn_infer(images[:nrows].contiguous(), idx_t, labels[:nrows].contiguous(), wf, master, state, b.gamma_off,
                    b.beta_off, b.mm_off, b.mv_off, b.fcw_off, b.fcb_off, logits, pred, correct, blocks)
    torch.cuda.synchronize()
    r = torch.tensor(rows)
    t.equal("logits", logits, c.o.logits[r], rows)
    t.equal("pred", pred, c.o.pred[r], rows)
    t.equal("correct", correct, (c.o.pred[r] == c.labels.long()[r]).long(), rows)
    return c


@pytest.mark.parametrize("case", X.INFER_CASES, ids=[X.infer_case_id(c) for c in X.INFER_CASES])
def test_infer_is_bit_exact(case):
    """All 19 ``layer`` cases, ``range`` (pixels over 0..255), ``pool`` (pre-pool values of up to 11
    significant bits: the last layer must stay fp32) and ``tie`` (exact ties: pred is the FIRST maximum,
    and image 0 is labelled with the later one).  Three distinct images in ONE workgroup (blocks=1,
    idx=None): the per-image halo re-zeroing, the reuse of r2 by the next stem input and the next-image
    stem prefetch all run; image 1 is bright and image 2 all-zero (``tie``: three single-colour images)."""
    t = _Tally(f"infer_{X.infer_case_id(case)}")
    c = _run(t, case, None, 1, nrows=3)
    if case[0] == "tie":
        assert c.o.tie[:3].tolist() == [True, False, True] and int(c.labels[0]) != int(c.o.pred[0])
    t.write()


GRIDS = {                                            # idx (rows of the 5 data rows), blocks
    "n1": ([3], 1),
    "n5-blocks2": ([4, 2, 0, 3, 1], 2),              # a permutation; workgroups take 3 and 2 images
    "repeats-blocks2": ([1, 1, 4, 1, 0, 2, 2], 2),
    "blocks-gt-n": ([2, 0, 1], 8),
    "blocks0": (None, 0),                            # the default grid
}


@pytest.mark.parametrize("grid", list(GRIDS), ids=list(GRIDS))
@pytest.mark.parametrize("layer", X.INFER_GEOM_LAYERS, ids=[X.infer_layer_id(l) for l in X.INFER_GEOM_LAYERS])
def test_infer_grids_are_bit_exact(layer, grid):
    """One ``layer`` case per geometry at N = 1, at N = 5 on two workgroups, with repeated rows, with more
    workgroups asked for than images, and on the default grid; labels has one entry per DATA row and
    correct must equal pred == labels[idx]."""
    idx, blocks = GRIDS[grid]
    t = _Tally(f"infer_{X.infer_layer_id(layer)}_{grid}")
    _run(t, ("layer", layer, 100 + layer), idx, blocks)
    t.write()
