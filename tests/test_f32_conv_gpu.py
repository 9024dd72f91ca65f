"""Direct conv2 kernel of the fp32 step (csrc/kernels/f32_conv.hip, ops/f32.py conv_same(impl="direct")):
forward and data gradient against float64 CPU conv2d / autograd -- exact on integers, at the fp32 bound on
floats --, bitwise independence of batch and grid, the autograd wiring, the whole model and a captured step."""
import pytest
import torch
import torch.nn.functional as F

from dmlc.models import cifar_cnn as M

pytestmark = pytest.mark.gpu


def _ops():
    import dmlc.ops._ext as E
    E.hip()
    return torch.ops.dmlc


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _ref(x, w, bias, dgrad):
    """float64 CPU reference, NHWC: conv2d(x, w) + bias, or with dgrad its input gradient for dy = x."""
    w64 = w.cpu().double().permute(3, 2, 0, 1)
    if not dgrad:
        y = F.conv2d(x.cpu().double().permute(0, 3, 1, 2), w64, None if bias is None else bias.cpu().double(), padding=2)
        return y.permute(0, 2, 3, 1)
    x0 = torch.zeros(x.shape, dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_()
    F.conv2d(x0, w64, padding=2).backward(x.cpu().double().permute(0, 3, 1, 2))
    return x0.grad.permute(0, 2, 3, 1)


def _ints(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (B, 12, 12, 64), generator=g).float().cuda()
    w = torch.randint(-2, 3, (5, 5, 64, 64), generator=g).float().cuda()
    return x, w, torch.randint(-8, 9, (64,), generator=g).float().cuda()


@pytest.mark.parametrize("dgrad", [False, True])
@pytest.mark.parametrize("B,blocks", [(1, 0), (3, 0), (5, 2)])     # (5, 2): workgroups loop over 3 and 2 images
def test_conv2_direct_is_exact_on_integers(dgrad, B, blocks):
    x, w, b = _ints(B, 10 * B + dgrad)                             # |partial sums| <= 1600 * 6 + 8 << 2^24: exact
    bias = None if dgrad else b
    got = _ops().f32_conv2_direct(x, w, bias, dgrad, blocks)
    assert torch.equal(got.cpu().double(), _ref(x, w, bias, dgrad))


@pytest.mark.parametrize("dgrad", [False, True])
def test_conv2_direct_matches_fp64_on_floats(dgrad):
    """Measured on an MI355X: 4.4e-7 (forward) and 4.8e-7 (data gradient) relative."""
    g = torch.Generator().manual_seed(int(dgrad))
    x = torch.randn(3, 12, 12, 64, generator=g).cuda()
    w = (0.05 * torch.randn(5, 5, 64, 64, generator=g)).cuda()
    bias = None if dgrad else torch.randn(64, generator=g).cuda()
    err = _rel(_ops().f32_conv2_direct(x, w.view(1600, 64), bias, dgrad).cpu(), _ref(x, w, bias, dgrad))
    print(f"conv2 direct dgrad={dgrad}: rel {err:.3g}")
    assert err < 2e-6          # the bound of test_implicit_conv_gemm_matches_explicit_im2col: same MFMA, same K


@pytest.mark.parametrize("dgrad", [False, True])
def test_conv2_direct_is_independent_of_batch_and_grid(dgrad):
    ops = _ops()
    g = torch.Generator().manual_seed(2 + dgrad)
    x = torch.randn(5, 12, 12, 64, generator=g).cuda()
    w = (0.05 * torch.randn(5, 5, 64, 64, generator=g)).cuda()
    bias = None if dgrad else torch.randn(64, generator=g).cuda()
    got = ops.f32_conv2_direct(x, w, bias, dgrad, 2)
    assert torch.equal(got, torch.cat([ops.f32_conv2_direct(x[i:i + 1], w, bias, dgrad) for i in range(5)]))
    assert torch.equal(got, ops.f32_conv2_direct(x, w, bias, dgrad, 0))
    assert torch.equal(got, ops.f32_conv2_direct(x, w, bias, dgrad, 2))


def test_conv_same_direct_autograd_matches_gemm():
    from dmlc.ops.f32 import conv_same
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 12, 12, 64, generator=g).cuda().requires_grad_()
    w = (0.05 * torch.randn(5, 5, 64, 64, generator=g)).cuda().requires_grad_()
    b = torch.randn(64, generator=g).cuda().requires_grad_()
    gy = torch.randn(2, 12, 12, 64, generator=g).cuda()
    (yd, *gd), (yg, *gg) = [(y.detach(), *torch.autograd.grad(y, (x, w, b), gy))
                            for y in (conv_same(x, w, b, impl=i) for i in ("direct", "gemm"))]
    assert _rel(yd, yg) < 2e-6 and _rel(gd[0], gg[0]) < 2e-6
    assert torch.equal(gd[1], gg[1]) and torch.equal(gd[2], gg[2])     # the same weight-gradient kernel and inputs


@pytest.mark.parametrize("B", [1, 8])
def test_model_with_direct_conv2_matches_fp64(B):
    """Measured on an MI355X: at most 7.5e-7 (B = 1) and 1.8e-6 (B = 8) over the logits and the ten gradients."""
    flat = M.init_flat_params(torch.Generator().manual_seed(B))
    g = torch.Generator().manual_seed(B)
    x = torch.randint(0, 256, (B, 24, 24, 3), generator=g).float().cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    hip = M.CifarCNN(flat, relu_logits=False, backend="hip_f32", conv2_impl="direct").cuda()
    logits = hip(x)
    F.cross_entropy(logits, y).backward()
    ref = M.CifarCNN(flat.double(), relu_logits=False)
    ref.flat.data = ref.flat.data.double()
    l64 = ref(x.cpu().double())
    F.cross_entropy(l64, y.cpu()).backward()
    errs = {"logits": _rel(logits.detach().cpu(), l64.detach())}
    g64 = M.views(ref.flat.grad)
    errs.update({n: _rel(v, g64[n]) for n, v in M.views(hip.flat.grad.cpu()).items()})
    print(f"direct conv2 model vs fp64, B={B}: " + ", ".join(f"{n} {e:.3g}" for n, e in errs.items()))
    assert max(errs.values()) < 1e-4, errs       # the fp32 bound of test_cnn_logits_and_grads_match_fp64


def test_captured_direct_step_equals_the_eager_step():
    from dmlc.engine.eager import EagerTrainer
    g = torch.Generator().manual_seed(7)
    data = torch.randint(0, 256, (128, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (128,), dtype=torch.int32, generator=g)
    tr = EagerTrainer("cifar_cnn", 16, data, labels, device="cuda", dtype="fp32", seed=3, lr=1e-4, graph=True,
                      backend="hip_f32", conv2_impl="direct")
    for _ in range(3):                                  # warm-up steps; the third one captures
        tr.step()
    assert tr.graph is not None and tr.model.conv2_impl == "direct"
    for _ in range(2):                                  # replay, then the same step eagerly from the same weights
        before = tr.model.flat.detach().clone()
        tr.step()
        got = [tr.last_loss.clone(), tr.last_acc.clone(), tr.model.flat.detach().clone()]
        with torch.no_grad():
            tr.model.flat.copy_(before)
        tr.model.flat.grad = None
        loss, acc = tr._fwd_bwd_sgd(tr._xs, tr._ys, tr._lr_t)
        for a, e in zip(got, [loss, acc, tr.model.flat.detach()]):
            assert torch.equal(a, e)


@pytest.mark.parametrize("case", ["H24", "C32", "strided", "cpu", "dgrad_bias"])
def test_conv2_direct_rejects_bad_arguments(case):
    x, w, b = torch.zeros(2, 12, 12, 64).cuda(), torch.zeros(5, 5, 64, 64).cuda(), torch.zeros(64).cuda()
    args = {"H24": (torch.zeros(2, 24, 24, 64).cuda(), w, b, False),
            "C32": (torch.zeros(2, 12, 12, 32).cuda(), w, b, False),
            "strided": (torch.zeros(2, 12, 12, 128).cuda()[..., ::2], w, b, False),
            "cpu": (x.cpu(), w, b, False),
            "dgrad_bias": (x, w, b, True)}[case]
    with pytest.raises(RuntimeError):
        _ops().f32_conv2_direct(*args)
