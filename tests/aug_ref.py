"""Exact integer cases of the augmented conv step (per-image random crop + flip), shared by
tests/test_augment.py (preconditions, CPU) and tests/test_augment_gpu.py (the kernels, bit for bit).

The oracle is tests/exact_ref.py, unmodified: the host reference ``apply_augment(data, words)`` is
written into the centre (4, 4) of a zeroed 32x32 batch, and ``conv_fwd_exact`` / ``conv_bwd_exact`` run
on that batch at crop (4, 4) -- so the kernels, which crop and flip the RAW images by the words, must
reproduce what the oracle computes from the already augmented images.  The inputs are drawn exactly as
``exact_ref.make_exact_case`` draws them."""
import functools
import types

import torch

import exact_ref as X
from dmlc.data.order import apply_augment, aug_words
from dmlc.models import cifar_cnn as M

# the B = 16 word table by batch row, as (cy, cx, flip): the four corners, the centre and mixed
# offsets, each corner and the centre both unflipped and flipped
TABLE16 = ((0, 0, 0), (0, 0, 1), (0, 8, 0), (0, 8, 1), (8, 0, 0), (8, 0, 1), (8, 8, 0), (8, 8, 1),
           (4, 4, 0), (4, 4, 1), (3, 5, 1), (5, 3, 0), (1, 7, 1), (7, 1, 0), (2, 6, 0), (6, 2, 1))
CENTRE = 4 | 4 << 4                      # word 68: the centre crop, no flip
# (batch, input seed) of the cases; B = 144 takes the words of shuffle seed 11, step 3
AUG_CASES = ((16, 1), (16, 2), (144, 4))


def pack(table) -> torch.Tensor:
    return torch.tensor([cy | cx << 4 | flip << 8 for cy, cx, flip in table], dtype=torch.int32)


def case_words(B: int) -> torch.Tensor:
    return pack(TABLE16) if B == 16 else aug_words(11, 3, torch.arange(B))


def centred(x24: torch.Tensor) -> torch.Tensor:
    """[B, 24, 24, 3] uint8 images in the centre (4, 4) of a zeroed [B, 32, 32, 3] batch."""
    out = torch.zeros(x24.shape[0], 32, 32, 3, dtype=torch.uint8)
    out[:, 4:28, 4:28] = x24
    return out


@functools.lru_cache(maxsize=None)
def make_aug_case(B, seed):
    """Inputs as make_exact_case(B, seed), the word table of the case, and the oracle's results for
    batch row b = dataset row b augmented by word b.  Asserts the oracle's preconditions (every value
    a bf16 integer, fp32 partial sums below 2^24, both pools exercised).  Cached, read-only."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
    data = ri(0, 3, B, 32, 32, 3).to(torch.uint8)
    w1 = ri(-1, 1, 5, 5, 3, 64)
    b1 = ri(-8, 2, 64)
    w2 = (torch.rand(5, 5, 64, 64, generator=g) < X.W2_DENSITY) * (2 * ri(0, 1, 5, 5, 64, 64) - 1)
    b2 = ri(-8, 2, 64)
    dp2 = ri(-3, 3, B, 6, 6, 64)
    words = case_words(B)
    xa = centred(apply_augment(data, words))
    y1, p1, am1, y2, p2, am2 = X.conv_fwd_exact(xa, 4, 4, w1, b1, w2, b2)
    bwd = X.conv_bwd_exact(xa, 4, 4, w2, p1, am1, am2, dp2)

    for name, v in (("y1", y1), ("y2", y2), ("dy2", bwd["dy2"]), ("dp1", bwd["dp1"]), ("dY1", bwd["dY1"])):
        assert int(v.abs().max()) <= 256, f"{name} leaves the bf16 integers: {int(v.abs().max())}"
    assert bwd["partial_bound"] < 2 ** 24, f"a weight-gradient partial sum can reach {bwd['partial_bound']}"
    X._pool_preconditions("pool1", y1, p1, am1, X.pool_first_argmax(y1.clamp(min=0))[2])
    X._pool_preconditions("pool2", y2, p2, am2, X.pool_first_argmax(y2.clamp(min=0))[2])

    flat = M.init_flat_params(torch.Generator().manual_seed(seed))
    v = M.views(flat)
    for k, t in (("conv1_kernel", w1), ("conv1_bias", b1), ("conv2_kernel", w2), ("conv2_bias", b2)):
        v[k].copy_(t.to(torch.float32))
    return types.SimpleNamespace(B=B, cy=4, cx=4, data=data, labels=torch.zeros(B, dtype=torch.int32), flat=flat,
                                 words=words, w1=w1, b1=b1, w2=w2, b2=b2, y1=y1, p1=p1, am1=am1, y2=y2, p2=p2,
                                 am2=am2, dp2=dp2, partial_bound=bwd["partial_bound"],
                                 **{k: bwd[k] for k in ("dy2", "dp1", "dY1", "gw1", "gb1", "gw2", "gb2")})


def rows_case(case, rows, words):
    """The oracle for an arbitrary pairing: batch row i = dataset row rows[i] augmented by words[i]
    (an explicit index list through the by-batch-row table).  Forward and backward, as integers."""
    rows = rows.long()
    xa = centred(apply_augment(case.data[rows], words))
    y1, p1, am1, y2, p2, am2 = X.conv_fwd_exact(xa, 4, 4, case.w1, case.b1, case.w2, case.b2)
    bwd = X.conv_bwd_exact(xa, 4, 4, case.w2, p1, am1, am2, case.dp2[rows])
    assert max(int(v.abs().max()) for v in (y1, y2, bwd["dy2"], bwd["dp1"], bwd["dY1"])) <= 256
    assert bwd["partial_bound"] < 2 ** 24
    return types.SimpleNamespace(p1=p1, am1=am1, p2=p2, am2=am2, y2=y2, dp2=case.dp2[rows],
                                 **{k: bwd[k] for k in ("dy2", "dp1", "gw1", "gb1", "gw2", "gb2")})
