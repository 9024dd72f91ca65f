"""Direct conv2 weight + bias gradient of the fp32 step (csrc/kernels/f32_conv.hip k_f32_conv2_wgrad,
ops/f32.py conv_same(impl="direct_all")) against float64 CPU autograd: exact on integers, at the fp32 bound on
floats, reproducible, the autograd wiring, the whole model and a captured step."""
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


def _ref(x, dy):
    """float64 CPU reference [1601, 64]: the weight gradient of conv2d in HWIO order, then sum(dy) as the last row."""
    w = torch.zeros(64, 64, 5, 5, dtype=torch.float64, requires_grad=True)
    d64 = dy.cpu().double()
    F.conv2d(x.cpu().double().permute(0, 3, 1, 2), w, padding=2).backward(d64.permute(0, 3, 1, 2))
    return torch.cat([w.grad.permute(2, 3, 1, 0).reshape(1600, 64), d64.sum((0, 1, 2))[None]])


@pytest.mark.parametrize("B,groups", [(1, 0), (3, 0), (5, 1), (7, 2)])   # (5, 1): one group walks 5 images; (7, 2): 4 + 3
def test_conv2_wgrad_is_exact_on_integers(B, groups):
    g = torch.Generator().manual_seed(B)
    x = torch.randint(-3, 4, (B, 12, 12, 64), generator=g).float().cuda()
    dy = torch.randint(-2, 3, (B, 12, 12, 64), generator=g).float().cuda()   # |partial sums| <= 6 * 144 * 7 < 2^24: exact
    assert torch.equal(_ops().f32_conv2_wgrad(x, dy, groups).cpu().double(), _ref(x, dy))


def _floats(B):
    g = torch.Generator().manual_seed(B)
    return torch.randn(B, 12, 12, 64, generator=g).cuda(), torch.randn(B, 12, 12, 64, generator=g).cuda()


def test_conv2_wgrad_matches_fp64_on_floats():
    """Measured on an MI355X: 2.0e-7 relative."""
    x, dy = _floats(3)
    err = _rel(_ops().f32_conv2_wgrad(x, dy).cpu(), _ref(x, dy))
    print(f"conv2 wgrad: rel {err:.3g}")
    assert err < 2e-6                  # the bound of test_conv2_direct_matches_fp64_on_floats: same MFMA, shorter sums


def test_conv2_wgrad_is_reproducible():
    """Measured on an MI355X: groups 2 against the default at B = 5: 3.2e-7 relative."""
    ops, (x, dy) = _ops(), _floats(5)
    g2, g0 = ops.f32_conv2_wgrad(x, dy, 2), ops.f32_conv2_wgrad(x, dy, 0)
    assert torch.equal(g2, ops.f32_conv2_wgrad(x, dy, 2)) and torch.equal(g0, ops.f32_conv2_wgrad(x, dy, 0))
    print(f"conv2 wgrad groups 2 vs 0: {_rel(g2, g0):.3g}")
    assert _rel(g2, g0) < 2e-6         # another summation order: the float bound, not bitwise


def test_conv_same_direct_all_autograd():
    from dmlc.ops.f32 import conv_same
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 12, 12, 64, generator=g).cuda().requires_grad_()
    w = (0.05 * torch.randn(5, 5, 64, 64, generator=g)).cuda().requires_grad_()
    b = torch.randn(64, generator=g).cuda().requires_grad_()
    gy = torch.randn(2, 12, 12, 64, generator=g).cuda()
    (ya, *ga), (yd, *gd) = [(y.detach(), *torch.autograd.grad(y, (x, w, b), gy))
                            for y in (conv_same(x, w, b, impl=i) for i in ("direct_all", "direct"))]
    assert torch.equal(ya, yd) and torch.equal(ga[0], gd[0])           # the same forward and data-gradient kernel
    ref = _ref(x.detach(), gy)
    assert _rel(ga[1].cpu().reshape(1600, 64), ref[:1600]) < 2e-6 and _rel(ga[2].cpu(), ref[1600]) < 2e-6


@pytest.mark.parametrize("B", [1, 8])
def test_model_with_direct_all_conv2_matches_fp64(B):
    """Measured on an MI355X: at most 7.5e-7 (B = 1) and 1.8e-6 (B = 8) over the logits and the ten gradients."""
    flat = M.init_flat_params(torch.Generator().manual_seed(B))
    g = torch.Generator().manual_seed(B)
    x = torch.randint(0, 256, (B, 24, 24, 3), generator=g).float().cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    hip = M.CifarCNN(flat, relu_logits=False, backend="hip_f32", conv2_impl="direct_all").cuda()
    logits = hip(x)
    F.cross_entropy(logits, y).backward()
    ref = M.CifarCNN(flat.double(), relu_logits=False)
    ref.flat.data = ref.flat.data.double()
    l64 = ref(x.cpu().double())
    F.cross_entropy(l64, y.cpu()).backward()
    errs = {"logits": _rel(logits.detach().cpu(), l64.detach())}
    g64 = M.views(ref.flat.grad)
    errs.update({n: _rel(v, g64[n]) for n, v in M.views(hip.flat.grad.cpu()).items()})
    print(f"direct_all conv2 model vs fp64, B={B}: " + ", ".join(f"{n} {e:.3g}" for n, e in errs.items()))
    assert max(errs.values()) < 1e-4, errs       # the bound of test_model_with_direct_conv2_matches_fp64


def test_captured_direct_all_step_equals_the_eager_step():
    from dmlc.engine.eager import EagerTrainer
    g = torch.Generator().manual_seed(7)
    data = torch.randint(0, 256, (128, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (128,), dtype=torch.int32, generator=g)
    tr = EagerTrainer("cifar_cnn", 16, data, labels, device="cuda", dtype="fp32", seed=3, lr=1e-4, graph=True,
                      backend="hip_f32", conv2_impl="direct_all")
    for _ in range(3):                                  # warm-up steps; the third one captures
        tr.step()
    assert tr.graph is not None and tr.model.conv2_impl == "direct_all"
    for _ in range(2):                                  # replay, then the same step eagerly from the same weights
        before = tr.model.flat.detach().clone()
        tr.step()
        got = [tr.last_loss.clone(), tr.last_acc.clone(), tr.model.flat.detach().clone()]
        with torch.no_grad():
            tr.model.flat.copy_(before)
        tr.model.flat.grad = None
        loss, acc = tr._fwd_bwd_sgd(tr._xs, tr._ys, tr._lr_t)
        assert all(torch.equal(a, e) for a, e in zip(got, [loss, acc, tr.model.flat.detach()]))


@pytest.mark.parametrize("case", ["H24", "C32", "batch", "strided", "cpu", "groups"])
def test_conv2_wgrad_rejects_bad_arguments(case):
    x, z = torch.zeros(2, 12, 12, 64).cuda(), lambda *s: torch.zeros(*s).cuda()
    args = {"H24": (z(2, 24, 24, 64), z(2, 24, 24, 64), 0), "C32": (z(2, 12, 12, 32), z(2, 12, 12, 32), 0),
            "batch": (x, z(3, 12, 12, 64), 0), "strided": (x, z(2, 12, 12, 128)[..., ::2], 0),
            "cpu": (x, x.cpu(), 0), "groups": (x, x, -1)}[case]
    with pytest.raises(RuntimeError):
        _ops().f32_conv2_wgrad(*args)
