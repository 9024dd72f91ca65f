"""k_rn_infer (csrc/kernels/resnet_infer.hip), the whole eval-mode ResNet-20 in one launch, through
FusedResNetEngine.infer / infer_logits / evaluate: logits against a plain fp64 forward, bitwise image
independence, and evaluation leaving the training state alone."""
import pytest
import torch
import torch.nn.functional as F

from dmlc.engine.fused_resnet import FusedResNetEngine
from dmlc.models import resnet as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _ref(images, flat, state, round_acts):
    """Eval-mode models/resnet.py in fp64 on the CPU.  The conv kernels are the fp32 master rounded to
    bf16 (what the shadows hold), everything else fp32 -> fp64; ``round_acts`` rounds to bf16 where the
    kernel stores an operand: the input, each a-conv output after ReLU, each block output."""
    p, st = R._views(flat.float().cpu(), R.PARAM_SPECS), R._views(state.float().cpu(), R.STATE_SPECS)
    rb = (lambda t: t.to(BF16).double()) if round_acts else (lambda t: t)

    def conv_bn(x, pre, stride):
        z = R._conv3x3(x, p[f"{pre}/conv/kernel"].to(BF16).double(), stride)
        sc = p[f"{pre}/bn/gamma"].double() / torch.sqrt(st[f"{pre}/bn/moving_variance"].double() + R.BN_EPS)
        sh = p[f"{pre}/bn/beta"].double() - st[f"{pre}/bn/moving_mean"].double() * sc
        return z * sc[None, :, None, None] + sh[None, :, None, None]

    x = F.relu(conv_bn(rb(images.cpu().double().permute(0, 3, 1, 2)), "stem", 1))
    cin = 16
    for s, wdt in enumerate(R.WIDTHS):
        for b in range(R.BLOCKS):
            stride = 2 if (s > 0 and b == 0) else 1
            y = rb(F.relu(conv_bn(x, f"stage{s}/block{b}/a", stride)))
            y = conv_bn(y, f"stage{s}/block{b}/b", 1)
            sc = F.pad(x[:, :, ::2, ::2], (0, 0, 0, 0, 0, wdt - cin)) if stride == 2 else x
            x, cin = rb(F.relu(y + sc)), wdt
    return x.mean(dim=(2, 3)) @ p["fc/weights"].double() + p["fc/biases"].double()


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def _engine(seed=0, **kw):
    """A batch-16 engine on 64 random images whose BN parameters and moving statistics are random
    (gamma, variance in [0.5, 1.5], beta and mean non-zero), so a folding error shows."""
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (64, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (64,), dtype=torch.int32, generator=g)
    flat, state = R.init_flat_params(torch.Generator().manual_seed(seed))
    for s in R.PARAM_SPECS:
        if s.name.endswith("gamma"):
            flat[s.offset:s.offset + s.numel] = 0.5 + torch.rand(s.numel, generator=g)
        elif s.name.endswith("beta") or s.name.endswith("biases"):
            flat[s.offset:s.offset + s.numel] = torch.randn(s.numel, generator=g)
    for s in R.STATE_SPECS:
        v = 0.5 + torch.rand(s.numel, generator=g) if s.name.endswith("variance") else 20.0 * torch.randn(s.numel, generator=g)
        state[s.offset:s.offset + s.numel] = v
    return FusedResNetEngine(16, data, labels, device="cuda", flat_params=flat, state=state, lr=1e-3, seed=seed, **kw)


@pytest.fixture(scope="module", params=["fresh", "trained"])
def case(request):
    """(engine, 7 images, their labels, fp64 logits without and with the kernel's roundings)"""
    eng = _engine()
    if request.param == "trained":        # the shadows and the moving statistics as the SGD kernel leaves them
        eng.capture(steps_per_graph=1)
        eng.run(3)
        torch.cuda.synchronize()
    g = torch.Generator().manual_seed(7)
    images = torch.randint(0, 256, (7, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (7,), dtype=torch.int32, generator=g)
    flat, state = eng.flat_params(), eng.state.cpu()
    assert torch.isfinite(flat).all() and torch.isfinite(state).all()
    return eng, images, labels, _ref(images, flat, state, False), _ref(images, flat, state, True)


@pytest.mark.parametrize("n,blocks", [(1, None), (5, 2), (7, 3)])
def test_logits_against_fp64(case, n, blocks):
    """rel(kernel, fp64) <= 3 * e_model, e_model = rel(fp64 with the kernel's bf16 roundings, fp64) of the
    same inputs; the factor covers fp32 accumulation, fp32 BN coefficients and the rounding flips they
    cause.  The small grids make every workgroup take two or three images (halo re-zeroing, rotation).
    Measured on an MI355X, rel(kernel, fp64) / e_model for (1, None), (5, 2), (7, 3): fresh engine
    8.9e-4 / 1.26e-3, 9.4e-4 / 1.07e-3, 9.4e-4 / 1.05e-3; after 3 steps 7.1e-4 / 7.4e-4, 5.8e-4 / 6.5e-4,
    6.5e-4 / 6.1e-4."""
    eng, images, _, ref, ref_rounded = case
    got = eng.infer_logits(images[:n], blocks=blocks)
    e_model, err = _rel(ref_rounded[:n], ref[:n]), _rel(got, ref[:n])
    print(f"rn_infer n={n} blocks={blocks}: rel(kernel, fp64) {err:.3e}, e_model {e_model:.3e}")
    assert got.shape == (n, 10) and got.dtype == torch.float32
    assert err <= 3 * e_model, (err, e_model)


def test_image_independence_bitwise(case):
    eng, images, labels, _, _ = case
    full, pred, correct = eng.infer(images, labels)
    for blocks in (1, 3):
        assert torch.equal(eng.infer_logits(images, blocks=blocks), full), blocks
    for i in range(7):
        assert torch.equal(eng.infer_logits(images[i:i + 1])[0], full[i]), i
    perm = torch.tensor([3, 6, 0, 5, 1, 4, 2, 3, 3])          # other positions, another batch size, repeats
    lg, pr, co = eng.infer(images, labels, idx=perm, blocks=2)
    assert torch.equal(lg, full[perm.cuda()])
    assert torch.equal(pred.long(), full.argmax(1)) and torch.equal(pr.long(), lg.argmax(1))
    assert torch.equal(correct, (pred == labels.cuda()).int()) and torch.equal(co, (pr == labels[perm].cuda()).int())


def test_evaluate_leaves_training_alone():
    runs = []
    for with_eval in (False, True):
        eng = _engine(seed=1)
        eng.capture(steps_per_graph=1)
        eng.run(2)
        if with_eval:
            acc = eng.evaluate(eng.data, eng.labels, impl="hip")
            assert 0.0 <= acc <= 1.0
        eng.run(2)
        torch.cuda.synchronize()
        runs.append([t.detach().cpu().contiguous().view(torch.int32) for t in (eng.master, eng.state, eng.stats)])
    for name, a, b in zip(("flat_params", "state", "stats ring"), *runs):
        assert torch.equal(a, b), name
