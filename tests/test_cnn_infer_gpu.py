"""k_cnn_infer (csrc/kernels/cnn_infer.hip), the whole eval-mode CIFAR-10 CNN in one launch, through
FusedCifarEngine.infer / infer_logits / evaluate: logits against a plain fp64 forward, bitwise image
independence, evaluation leaving the training state alone, and the binding's argument checks."""
import pytest
import torch
import torch.nn.functional as F

from dmlc.engine.fused import SEG_OFF, FusedCifarEngine
from dmlc.models import cifar_cnn as M

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _ref(images, flat, relu_logits, rounded):
    """models/cifar_cnn.py in fp64 on the CPU from the fp32 master, centre crop (4, 4).  ``rounded``: the
    weights (not the biases), p1, p2, h1 and h2 go through bf16, where the kernel rounds."""
    rb = (lambda t: t.to(BF16).double()) if rounded else (lambda t: t.double())
    p = M.views(flat.float().cpu())
    x = images.cpu()[:, 4:28, 4:28, :].double().permute(0, 3, 1, 2)
    for c in ("conv1", "conv2"):
        x = F.conv2d(x, rb(p[f"{c}_kernel"]).permute(3, 2, 0, 1), p[f"{c}_bias"].double(), padding=2)
        x = rb(M.tf_same_maxpool_3x3s2(F.relu(x)))
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    x = rb(F.relu(x @ rb(p["full_weight_1"]) + p["full_bias_1"].double()))
    x = rb(F.relu(x @ rb(p["full_weight_2"]) + p["full_bias_2"].double()))
    x = x @ rb(p["full_weight_3"]) + p["full_bias_3"].double()
    return F.relu(x) if relu_logits else x


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def _engine(relu_logits, steps, seed=0, lr=1e-5):
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (64, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (64,), dtype=torch.int32, generator=g)
    eng = FusedCifarEngine(16, data, labels, device="cuda", seed=seed, lr=lr, relu_logits=relu_logits)
    if steps:                              # 3 steps: the shadows as the SGD leaves them, fc1n parity slot 1
        eng.capture(steps_per_graph=1)
        eng.run(steps)
        torch.cuda.synchronize()
        assert eng.global_step() == steps
    return eng, data, labels


@pytest.fixture(scope="module", params=[(True, 0), (False, 0), (True, 3), (False, 3)],
                ids=["relu-fresh", "linear-fresh", "relu-trained", "linear-trained"])
def case(request):
    """(engine, its 64 images, labels, fp64 logits without and with the kernel's roundings)"""
    relu_logits, steps = request.param
    eng, data, labels = _engine(relu_logits, steps)
    flat = eng.flat_params()
    assert torch.isfinite(flat).all()
    return eng, data, labels, _ref(data, flat, relu_logits, False), _ref(data, flat, relu_logits, True)


@pytest.mark.parametrize("n,blocks", [(1, None), (16, None), (17, None), (37, 2), (5, 8)])
def test_logits_against_fp64(case, n, blocks):
    """rel(kernel, fp64) <= 3 * e_model, e_model = rel(fp64 with the kernel's bf16 roundings, fp64) of the
    same inputs (the rule of tests/test_rn_infer_gpu.py).  One valid row of a tile; one full tile; a full
    tile plus a one-row tile; a wrapping persistent loop whose partial last tile lands on a workgroup that
    has run one; more workgroups than tiles.  Measured on an MI355X, rel(kernel, fp64) / e_model over the
    five cases: relu-fresh 3.4e-3..4.3e-3 / 3.7e-3..4.3e-3 (ratio 0.89..1.00), linear-fresh 4.0e-3..5.5e-3
    (0.97..1.02), relu-trained 5.7e-3..7.7e-3 (1.00), linear-trained 6.9e-3..9.6e-3 (1.00): the kernel's
    error is the operand roundings'."""
    eng, data, labels, ref, ref_rounded = case
    got, pred, correct = eng.infer(data[:n], labels[:n], blocks=blocks)
    e_model, err = _rel(ref_rounded[:n], ref[:n]), _rel(got, ref[:n])
    print(f"cnn_infer n={n} blocks={blocks}: rel(kernel, fp64) {err:.3e}, e_model {e_model:.3e}, ratio {err / e_model:.2f}")
    assert got.shape == (n, 10) and got.dtype == torch.float32
    assert err <= 3 * e_model, (err, e_model)
    assert torch.equal(pred.long(), got.argmax(1))
    assert torch.equal(correct, (pred == labels[:n].cuda()).int())


def test_image_independence_bitwise(case):
    """idx with a permutation and repeats gives the rows of the same images run by position; an image's
    logits do not depend on N, on its row in the tile or on the grid."""
    eng, data, labels, _, _ = case
    full, pred, _ = eng.infer(data[:37], labels[:37])
    for blocks in (1, 2, 3):
        assert torch.equal(eng.infer_logits(data[:37], blocks=blocks), full), blocks
    for i in (0, 15, 16, 36):
        assert torch.equal(eng.infer_logits(data[i:i + 1])[0], full[i]), i
    assert torch.equal(eng.infer_logits(data[5:30]), full[5:30])
    perm = torch.cat([torch.randperm(37, generator=torch.Generator().manual_seed(3)), torch.tensor([4, 4, 36, 0])])
    lg, pr, co = eng.infer(data[:37], labels[:37], idx=perm, blocks=2)
    assert torch.equal(lg, full[perm.cuda()]) and torch.equal(pr, pred[perm.cuda()])
    assert torch.equal(co, (pr == labels[perm].cuda()).int())


@pytest.mark.parametrize("relu_logits", [True, False])
def test_evaluate_leaves_training_alone(relu_logits):
    # (lr 1e-6: at the other cases' 1e-5, three steps on raw 0..255 pixels halve the logits and spread the 64
    # images' top-2 gaps until, whatever the seed, some image's gap falls below the bound)
    eng, data, labels = _engine(relu_logits, 3, seed=5, lr=1e-6)
    ref = _ref(data, eng.flat_params(), relu_logits, False)
    e_model = _rel(_ref(data, eng.flat_params(), relu_logits, True), ref)
    top2 = ref.topk(2, dim=1).values
    # no prediction may hinge on less than the error test_logits_against_fp64 allows (an absolute error of
    # 3 * e_model * |ref| in the worst case on one logit): the seed is chosen so; checked, never skipped
    gap, bound = float((top2[:, 0] - top2[:, 1]).min()), 3 * e_model * float(ref.norm())
    print(f"evaluate relu_logits={relu_logits}: smallest fp64 top-2 gap {gap:.3f}, bound {bound:.3f}")
    assert gap > bound, "pick another seed"
    names = ("master", "fc1n", "w1f", "w2f", "w2d", "fc2t", "fc3t", "bidx", "xraw", "stats", "step_t")
    before = [getattr(eng, k).clone() for k in names]
    acc = eng.evaluate(data, labels, impl="hip")
    torch.cuda.synchronize()
    for k, b in zip(names, before):
        assert torch.equal(getattr(eng, k).view(torch.uint8), b.view(torch.uint8)), k
    assert acc == eng.evaluate(data, labels) == int(eng.infer(data, labels)[2].sum()) / 64
    assert acc == int((ref.argmax(1) == labels.long()).sum()) / 64
    eng.run(1)                             # and training goes on
    torch.cuda.synchronize()
    assert eng.global_step() == 4 and torch.isfinite(eng.master).all()


@pytest.mark.parametrize("bad", ["dtype", "shape", "correct_without_labels", "scratch"])
def test_binding_rejects_bad_arguments(bad):
    """Each bad argument raises in the binding, before any launch (the outputs stay as they were)."""
    eng, data, labels = _engine(True, 0)
    dev, n = eng.device, 40
    images, lab = data[:n].to(dev), labels[:n].to(dev)
    logits = torch.full((n, 10), -7.0, device=dev)
    correct = torch.full((n,), -7, dtype=torch.int32, device=dev)
    scratch = torch.empty(3, 16, 2304, dtype=BF16, device=dev)      # n = 40: three tiles
    if bad == "dtype":
        images = images.to(torch.int8)
    elif bad == "shape":
        images = images[:, :, :24].contiguous()
    elif bad == "correct_without_labels":
        lab = None
    else:
        scratch = scratch[:2]
    with pytest.raises(RuntimeError):
        eng.ops.cnn_infer(images, None, lab, 4, 4, eng.w1f, eng.w2f, eng.fc1n, eng.step_t, eng.fc2t, eng.fc3t,
                          eng.master, SEG_OFF, True, scratch, logits, None, correct, 0)
    torch.cuda.synchronize()
    assert bool((logits == -7.0).all()) and bool((correct == -7).all())
