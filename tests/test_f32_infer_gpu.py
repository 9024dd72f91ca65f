"""k_cnn_infer_f32 (csrc/kernels/f32_infer.hip), the eval-mode CIFAR-10 CNN in true fp32 in one launch,
through ops/f32.py cnn_infer_f32 and EagerTrainer.infer / infer_logits / evaluate on the hip_f32 backend:
logits against cnn_forward in float64, bitwise image independence, predictions and hits, evaluation
leaving the parameters alone, and the binding's argument checks."""
import pytest
import torch

from dmlc.engine.eager import EagerTrainer
from dmlc.models import cifar_cnn as M

pytestmark = pytest.mark.gpu
SEED = 3          # chosen on the CPU: see test_evaluate_matches_fp64_and_leaves_the_parameters_alone


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _data():
    g = torch.Generator().manual_seed(SEED)
    return (torch.randint(0, 256, (64, 32, 32, 3), dtype=torch.uint8, generator=g),
            torch.randint(0, 10, (64,), dtype=torch.int32, generator=g))


def _ref64(data, flat, relu_logits):
    """models/cifar_cnn.py cnn_forward on the CPU in float64: same centre crops, same flat weights."""
    return M.cnn_forward(data[:, 4:28, 4:28, :].double(), M.views(flat.cpu().double()), relu_logits)


@pytest.fixture(scope="module", params=[(True, 0), (False, 0), (True, 3), (False, 3)],
                ids=["relu-fresh", "linear-fresh", "relu-trained", "linear-trained"])
def case(request):
    """(hip_f32 trainer at the seeded init or 3 of its own training steps on, its 64 images, labels,
    their float64 logits)"""
    relu_logits, steps = request.param
    data, labels = _data()
    tr = EagerTrainer("cifar_cnn", 16, data, labels, device="cuda", dtype="fp32", seed=SEED, lr=1e-6,
                      relu_logits=relu_logits, backend="hip_f32")
    for _ in range(steps):
        tr.step()
    flat = tr.flat_params()
    assert torch.isfinite(flat).all()
    return tr, data, labels, _ref64(data, flat, relu_logits)


@pytest.mark.parametrize("n,blocks,use_idx", [(1, None, False), (16, None, False), (17, None, False), (40, None, False),
                                              (40, 1, False), (40, 2, False), (40, 2, True)])
def test_logits_against_fp64(case, n, blocks, use_idx):
    """rel(kernel, float64 cnn_forward) < 1e-4, the bound tests/test_f32_gpu.py asserts for this engine's
    logits.  One row of a tile; a full tile; a tile plus one row; three tiles on three, one and two
    workgroups (the persistent loop reuses LDS and the slab across tiles); a permutation with repeats.
    Measured on an MI355X over the 28 cases: 2.1e-7 (n = 1, relu-fresh) .. 1.1e-6 (n = 1, relu-trained),
    7.4e-7 .. 8.5e-7 at n = 40 whatever the grid."""
    tr, data, labels, ref = case
    idx = None
    if use_idx:
        idx = torch.cat([torch.randperm(64, generator=torch.Generator().manual_seed(3))[:n - 3], torch.tensor([5, 5, 63])])
    got, pred, hits = tr.infer(data if use_idx else data[:n], labels if use_idx else labels[:n], idx=idx, blocks=blocks)
    want = ref[idx] if use_idx else ref[:n]
    lab = labels[idx] if use_idx else labels[:n]
    err = _rel(got.cpu(), want)
    print(f"f32_cnn_infer n={n} blocks={blocks} idx={use_idx}: rel(kernel, fp64) {err:.3e}")
    assert got.shape == (n, 10) and got.dtype == torch.float32
    assert err < 1e-4, err
    assert torch.equal(pred.long(), got.argmax(1))
    assert torch.equal(hits, (pred == lab.cuda()).int())


def test_image_independence_bitwise(case):
    """An image's logits do not depend on N, on its row in the tile or on the grid."""
    tr, data, labels, _ = case
    full = tr.infer_logits(data[:40])
    for blocks in (1, 2):
        assert torch.equal(tr.infer_logits(data[:40], blocks=blocks), full), blocks
    for i in (0, 15, 16, 39):
        assert torch.equal(tr.infer_logits(data[i:i + 1])[0], full[i]), i
    assert torch.equal(tr.infer_logits(data[5:30]), full[5:30])


def test_evaluate_matches_fp64_and_leaves_the_parameters_alone(case):
    tr, data, labels, ref = case
    top2 = ref.topk(2, dim=1).values
    # no prediction may hinge on fp32 rounding: every image's float64 top-2 gap exceeds 1e-3 * max|logit|
    # (SEED is chosen so; checked for all 64 images, never skipped)
    gap, bound = float((top2[:, 0] - top2[:, 1]).min()), 1e-3 * float(ref.abs().max())
    print(f"evaluate: smallest fp64 top-2 gap {gap:.4f}, bound {bound:.4f}")
    assert gap > bound, "pick another SEED"
    before, step = tr.model.flat.detach().clone(), tr.global_step
    acc = tr.evaluate(data, labels, impl="hip")
    torch.cuda.synchronize()
    assert torch.equal(tr.model.flat.detach().view(torch.int32), before.view(torch.int32)) and tr.global_step == step
    assert acc == int((ref.argmax(1) == labels.long()).sum()) / 64
    assert acc == tr.evaluate(data, labels, impl="batched")
    assert tr.evaluate(data, labels, max_batches=2, impl="hip") == int(tr.infer(data[:32], labels[:32])[2].sum()) / 32


@pytest.mark.parametrize("bad", ["dtype", "shape", "hits_without_labels", "scratch", "flat", "blocks", "labels"])
def test_binding_rejects_bad_arguments(bad):
    """Each bad argument raises in the binding, before any launch (the outputs stay as they were)."""
    data, labels = _data()
    n = 40
    images, lab = data[:n].cuda(), labels[:n].cuda()
    flat = M.init_flat_params(torch.Generator().manual_seed(SEED)).cuda()
    logits = torch.full((n, 10), -7.0, device="cuda")
    hits = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty(3, 16, 2304, device="cuda")              # n = 40: three tiles
    blocks = 0
    if bad == "dtype":
        images = images.to(torch.int8)
    elif bad == "shape":
        images = images[:, :, :24].contiguous()
    elif bad == "hits_without_labels":
        lab = None
    elif bad == "scratch":
        scratch = scratch[:2]
    elif bad == "flat":
        flat = flat[:-64]
    elif bad == "blocks":
        blocks = -1
    else:
        lab = lab[:-1]
    import dmlc.ops._ext as E
    E.hip()
    with pytest.raises(RuntimeError):
        torch.ops.dmlc.f32_cnn_infer(images, None, lab, 4, 4, flat, [s.offset for s in M.PARAM_SPECS], True, scratch,
                                     logits, None, hits, blocks)
    torch.cuda.synchronize()
    assert bool((logits == -7.0).all()) and bool((hits == -7).all())
