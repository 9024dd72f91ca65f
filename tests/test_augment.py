"""Per-image random crop + flip (augmentation), host side: the keyed draw (data/order.py, twin of
common.h aug_word), the host reference apply_augment, the eager engine's use of both, the routing of
--augment, and the preconditions of the exact cases tests/test_augment_gpu.py runs on the kernels."""
import pytest
import torch

import aug_ref as A
import exact_ref as X
from dmlc import config as C
from dmlc.data.order import OrderSpec, apply_augment, aug_hash, aug_words, unpack_aug
from dmlc.engine.eager import EagerTrainer
from dmlc.engine.trainer import pick_impl

# (seed, step, g) -> h, word, (cy, cx, flip): computed from the definition on the CPU
ANCHORS = (((0, 0, 0), 0x951D42A2, 274, (2, 1, 1)),
           ((0, 0, 1), 0x28B4F6AF, 40, (8, 2, 0)),
           ((0, 1, 0), 0x06D07382, 4, (4, 0, 0)),
           ((11, 7, 5), 0xC916A559, 341, (5, 5, 1)),
           ((11, 2456, 255), 0x471F280F, 81, (1, 5, 0)),
           ((123456789, 2 ** 32 + 3, 1023), 0xF8BA9B69, 389, (5, 8, 1)))


def test_anchor_words():
    for (seed, step, g), h, word, triple in ANCHORS:
        gt = torch.tensor([g])
        assert int(aug_hash(seed, step, gt)) == h, (seed, step, g)
        w = aug_words(seed, step, gt)
        assert w.dtype == torch.int32 and int(w) == word
        assert tuple(int(t) for t in unpack_aug(w)) == triple
    # through OrderSpec: row g of rank 0 at batch >= g + 1
    assert int(OrderSpec(4096, 256, seed=11).augment(2456)[255]) == 81
    assert int(OrderSpec(4096, 512, 2, 1, seed=123456789).augment(2 ** 32 + 3)[511]) == 389


@pytest.mark.parametrize("seed", [0, 11])
def test_range_and_spread(seed):
    o = OrderSpec(1 << 15, 256, seed=seed)
    tables = [o.augment(s) for s in range(64)]
    w = torch.stack(tables)
    cy, cx, flip = unpack_aug(w)
    assert bool(((w >= 0) & (w < 512) & (cy <= 8) & (cx <= 8)).all())
    assert bool(((cy | cx << 4 | flip << 8) == w).all())
    combo = (cy * 9 + cx) * 2 + flip
    counts = torch.bincount(combo.reshape(-1), minlength=162)
    assert counts.numel() == 162 and int(counts.min()) > 0, "a (cy, cx, flip) combination never occurs"
    share = float(flip.float().mean())
    print(f"seed {seed}: min/max count {int(counts.min())}/{int(counts.max())} of {w.numel() / 162:.0f}, flip {share:.3f}")
    assert 0.48 <= share <= 0.52
    for a, b in zip(tables, tables[1:]):
        assert not torch.equal(a, b)


@pytest.mark.parametrize("W", [2, 4])
def test_ranks_carry_the_union_batch_words(W):
    B, n = 24, 4096
    single = OrderSpec(n, W * B, seed=7)
    specs = [OrderSpec(n, B, W, r, seed=7) for r in range(W)]
    for step in (0, 1, single.period, 3 * single.period + 5):
        assert torch.equal(torch.cat([s.augment(step) for s in specs]), single.augment(step))
        assert torch.equal(torch.cat([specs[0].augment(step, rank=r) for r in range(W)]), single.augment(step))


def test_padding_rows_repeat_the_last_valid_word():
    o = OrderSpec(1000, 12, 2, 1, seed=3)
    w, p = o.augment(9), o.augment(9, pad_to=16)
    assert w.shape == (12,) and p.shape == (16,) and p.dtype == torch.int32
    assert torch.equal(p[:12], w) and bool((p[12:] == w[11]).all())


def test_apply_augment_matches_the_index_formula():
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (40, 32, 32, 3), generator=g, dtype=torch.uint8)
    words = aug_words(5, 17, torch.arange(40))
    words[:16] = A.pack(A.TABLE16)
    out = apply_augment(x, words)
    assert out.shape == (40, 24, 24, 3) and out.dtype == torch.uint8
    want = torch.empty_like(out)
    for b in range(40):
        cy, cx, flip = (int(t) for t in unpack_aug(words[b]))
        for y in range(24):
            for xx in range(24):
                want[b, y, xx] = x[b, cy + y, cx + 23 - xx if flip else cx + xx]
    assert torch.equal(out, want)
    assert torch.equal(apply_augment(x, torch.full((40,), A.CENTRE, dtype=torch.int32)), x[:, 4:28, 4:28])


def test_eager_engine_draws_the_keyed_words():
    g = torch.Generator().manual_seed(1)
    data = torch.randint(0, 256, (96, 32, 32, 3), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (96,), generator=g)
    a, b = (EagerTrainer("cifar_cnn", 16, data, labels, seed=5, augment=True) for _ in range(2))
    plain = EagerTrainer("cifar_cnn", 16, data, labels, seed=5)
    for step in (0, 3, 7):                       # 7: the second epoch (6 steps each)
        x, y = a.batch(step)
        rows = a.order.batch(step)
        assert torch.equal(x, apply_augment(data[rows], a.order.augment(step)).float())
        assert torch.equal(y, labels[rows])
        xb, _ = b.batch(step)
        assert torch.equal(x, xb)
        assert torch.equal(plain.batch(step)[0], data[rows][:, 4:28, 4:28].float())
    assert not torch.equal(a.order.augment(0), a.order.augment(1))
    x0, x6 = a.batch(0)[0], a.batch(6)[0]
    assert not torch.equal(x0, x6)
    # a rank of a two-rank run takes its rows of the union batch
    r1 = EagerTrainer("cifar_cnn", 8, data, labels, seed=5, augment=True, world_size=2, rank=1)
    assert torch.equal(r1.batch(2)[0], a.batch(2)[0][8:])


def test_augment_routes_the_cnn_to_the_fused_engine():
    cuda = torch.device("cuda")
    assert pick_impl(C.TrainConfig(augment=True), cuda) == "fused"
    assert pick_impl(C.TrainConfig(augment=True, dtype="fp8"), cuda) == "fused"
    assert pick_impl(C.TrainConfig(augment=True, model="resnet20", crop=32), cuda) == "eager"
    assert pick_impl(C.TrainConfig(augment=True, dtype="fp32"), cuda) == "hipf32"
    assert pick_impl(C.TrainConfig(augment=True), torch.device("cpu")) == "eager"


@pytest.mark.parametrize("B,seed", A.AUG_CASES)
def test_exact_case_preconditions(B, seed):
    """make_aug_case asserts the oracle's preconditions (|value| <= 256, partial sums < 2^24, both
    pools exercised); here also that the inputs are make_exact_case's and that the case tells the
    augmented step from the centre crop."""
    case = A.make_aug_case(B, seed)
    plain = X.make_exact_case(B, seed, 4, 4)
    for k in ("data", "w1", "b1", "w2", "b2", "dp2", "flat"):
        assert torch.equal(getattr(case, k), getattr(plain, k)), k
    if B == 16:
        assert [tuple(int(t[i]) for t in unpack_aug(case.words)) for i in range(16)] == list(A.TABLE16)
    else:
        assert torch.equal(case.words, OrderSpec(B, B, seed=11).augment(3))
    print(f"B={B} seed={seed}: max |y2| {int(case.y2.abs().max())}, partial bound {case.partial_bound:.3g}")
    assert int(case.y2.abs().max()) <= 256 and case.partial_bound < 2 ** 24
    differ = int((case.p1 != plain.p1).flatten(1).any(1).sum())
    centre = int((case.words == A.CENTRE).sum())
    assert differ == B - centre and differ >= B - 1, (differ, centre)
    assert not torch.equal(case.gw1, plain.gw1)
    # an explicit list pairs other dataset rows with the same by-batch-row table
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5))
    r = A.rows_case(case, perm, case.words)
    assert not torch.equal(r.p1, case.p1[perm])
