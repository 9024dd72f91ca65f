"""conv1's direct backward of the fp32 step (csrc/kernels/f32_conv1.hip, ops/f32.py conv1_impl="direct") against
float64 CPU autograd: the dense form (f32_conv1_wgrad) and the form that rebuilds dy from the pooled gradient and
the argmax bytes (f32_conv1_wgrad_pool), exact on integers, at the fp32 bound on floats, reproducible; the whole
model, a captured step, and the argument checks."""
import pytest
import torch
import torch.nn.functional as F

from dmlc.models import cifar_cnn as M

pytestmark = pytest.mark.gpu
CASES = [(1, 0), (3, 0), (5, 1), (7, 2)]    # (B, groups); (5, 1): one group walks 5 images; (7, 2): 4 + 3


def _ops():
    import dmlc.ops._ext as E
    E.hip()
    return torch.ops.dmlc


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _ref(x, dy):
    """float64 CPU reference [76, 64]: the weight gradient of conv2d in HWIO order, then sum(dy) as row 75."""
    w = torch.zeros(64, 3, 5, 5, dtype=torch.float64, requires_grad=True)
    d64 = dy.cpu().double()
    F.conv2d(x.cpu().double().permute(0, 3, 1, 2), w, padding=2).backward(d64.permute(0, 3, 1, 2))
    return torch.cat([w.grad.permute(2, 3, 1, 0).reshape(75, 64), d64.sum((0, 1, 2))[None]])


def _pool_dy(y, dp):
    """dy of pool(relu(y)) by float64 CPU autograd."""
    y64 = y.cpu().double().requires_grad_()
    F.max_pool2d(torch.relu(y64).permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1).backward(dp.cpu().double())
    return y64.grad


@pytest.mark.parametrize("B,groups", CASES)
def test_conv1_wgrad_is_exact_on_integers(B, groups):
    g = torch.Generator().manual_seed(B)
    x = torch.randint(-3, 4, (B, 24, 24, 3), generator=g).float().cuda()
    dy = torch.randint(-2, 3, (B, 24, 24, 64), generator=g).float().cuda()   # |partial sums| <= 7 * 576 * 6 < 2^24: exact
    assert torch.equal(_ops().f32_conv1_wgrad(x, dy, groups).cpu().double(), _ref(x, dy))


@pytest.mark.parametrize("B,groups,planes", [c + ("perm",) for c in CASES] + [(3, 0, "const")])
def test_conv1_wgrad_pool_is_exact_on_integers(B, groups, planes):
    ops = _ops()
    g = torch.Generator().manual_seed(10 + B)
    if planes == "perm":    # every (image, channel) plane a permutation of -288 .. 287: no ties, about half the windows masked
        y = (torch.stack([torch.randperm(576, generator=g) for _ in range(B * 64)]) - 288).view(B, 64, 24, 24)
        y = y.permute(0, 2, 3, 1).float().contiguous().cuda()
    else:                   # constant positive planes: every argmax byte 0, all four owners of a pixel at the borders
        y = (1 + torch.arange(64.0)).expand(B, 24, 24, 64).contiguous().cuda()
    x = torch.randint(-3, 4, (B, 24, 24, 3), generator=g).float().cuda()
    dp = torch.randint(-2, 3, (B, 12, 12, 64), generator=g).float().cuda()
    arg = ops.f32_relu_pool_fwd(y, 0)[1]
    assert planes == "perm" or int(arg.max()) == 0
    dy = _pool_dy(y, dp)                                # |dy| <= 8, |sums| <= 7 * 576 * 3 * 8 < 2^24: exact
    assert torch.equal(ops.f32_conv1_wgrad_pool(x, dp, arg, groups).cpu().double(), _ref(x, dy))


def _floats(B):
    g = torch.Generator().manual_seed(B)
    x, y = torch.randn(B, 24, 24, 3, generator=g).cuda(), torch.randn(B, 24, 24, 64, generator=g).cuda()
    dp = torch.randn(B, 12, 12, 64, generator=g).cuda()
    return x, y, dp, _ops().f32_relu_pool_fwd(y, 0)[1]


def test_conv1_wgrad_matches_fp64_on_floats():
    """Measured on an MI355X: dense 2.9e-7, pool form 1.3e-7 relative."""
    ops, (x, y, dp, arg) = _ops(), _floats(3)
    dense = _rel(ops.f32_conv1_wgrad(x, y).cpu(), _ref(x, y))          # y as a dense gradient
    pool = _rel(ops.f32_conv1_wgrad_pool(x, dp, arg).cpu(), _ref(x, _pool_dy(y, dp)))
    print(f"conv1 wgrad: dense rel {dense:.3g}, pool rel {pool:.3g}")
    assert dense < 2e-6 and pool < 2e-6    # the bound of test_conv2_wgrad_matches_fp64_on_floats: same MFMA and sums


def test_conv1_wgrad_is_reproducible():
    """Measured on an MI355X: groups 2 against the default at B = 5: dense 4.7e-7, pool form 2.0e-7 relative."""
    ops, (x, y, dp, arg) = _ops(), _floats(5)
    for name, f in (("dense", lambda n: ops.f32_conv1_wgrad(x, y, n)), ("pool", lambda n: ops.f32_conv1_wgrad_pool(x, dp, arg, n))):
        g2, g0 = f(2), f(0)
        assert torch.equal(g2, f(2)) and torch.equal(g0, f(0))
        print(f"conv1 wgrad {name}, groups 2 vs 0: {_rel(g2, g0):.3g}")
        assert _rel(g2, g0) < 2e-6         # another summation order: the float bound, not bitwise


@pytest.mark.parametrize("B", [1, 8])
def test_model_with_direct_conv1_matches_fp64(B):
    """Measured on an MI355X: at most 7.5e-7 (B = 1) and 1.8e-6 (B = 8) over the logits and the ten gradients, fused or not."""
    flat = M.init_flat_params(torch.Generator().manual_seed(B))
    g = torch.Generator().manual_seed(B)
    x = torch.randint(0, 256, (B, 24, 24, 3), generator=g).float().cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    ref = M.CifarCNN(flat.double(), relu_logits=False)
    ref.flat.data = ref.flat.data.double()
    l64 = ref(x.cpu().double())
    F.cross_entropy(l64, y.cpu()).backward()
    g64 = M.views(ref.flat.grad)
    gemm = M.CifarCNN(flat, relu_logits=False, backend="hip_f32", conv1_impl="gemm").cuda()(x)
    for fused in (True, False):             # one launch for the stage's backward / the dense weight gradient
        hip = M.CifarCNN(flat, relu_logits=False, backend="hip_f32", fused=fused, conv1_impl="direct").cuda()
        logits = hip(x)
        assert torch.equal(logits, gemm)    # the forward kernels are those of "gemm"
        F.cross_entropy(logits, y).backward()
        errs = {"logits": _rel(logits.detach().cpu(), l64.detach())}
        errs.update({n: _rel(v, g64[n]) for n, v in M.views(hip.flat.grad.cpu()).items()})
        print(f"direct conv1 model vs fp64, B={B}, fused={fused}: " + ", ".join(f"{n} {e:.3g}" for n, e in errs.items()))
        assert max(errs.values()) < 1e-4, errs      # the bound of test_model_with_direct_all_conv2_matches_fp64


def test_captured_direct_conv1_step_equals_the_eager_step():
    from dmlc.engine.eager import EagerTrainer
    g = torch.Generator().manual_seed(7)
    data = torch.randint(0, 256, (128, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (128,), dtype=torch.int32, generator=g)
    tr = EagerTrainer("cifar_cnn", 16, data, labels, device="cuda", dtype="fp32", seed=3, lr=1e-4, graph=True,
                      backend="hip_f32", conv1_impl="direct")
    for _ in range(3):                                  # warm-up steps; the third one captures
        tr.step()
    assert tr.graph is not None and tr.model.conv1_impl == "direct"
    for _ in range(2):                                  # replay, then the same step eagerly from the same weights
        before = tr.model.flat.detach().clone()
        tr.step()
        got = [tr.last_loss.clone(), tr.last_acc.clone(), tr.model.flat.detach().clone()]
        with torch.no_grad():
            tr.model.flat.copy_(before)
        tr.model.flat.grad = None
        loss, acc = tr._fwd_bwd_sgd(tr._xs, tr._ys, tr._lr_t)
        assert all(torch.equal(a, e) for a, e in zip(got, [loss, acc, tr.model.flat.detach()]))


@pytest.mark.parametrize("case", ["H12", "C4", "batch", "strided", "cpu", "arg_dtype", "groups"])
def test_conv1_wgrad_rejects_bad_arguments(case):
    ops, z = _ops(), lambda *s: torch.zeros(*s).cuda()
    x, dy, dp, arg = z(2, 24, 24, 3), z(2, 24, 24, 64), z(2, 12, 12, 64), z(2, 12, 12, 64).byte()
    dense, pool = {"H12": ((z(2, 12, 12, 3), dy, 0), (z(2, 12, 12, 3), dp, arg, 0)),
                   "C4": ((z(2, 24, 24, 4), dy, 0), (z(2, 24, 24, 4), dp, arg, 0)),
                   "batch": ((x, z(3, 24, 24, 64), 0), (x, dp, z(3, 12, 12, 64).byte(), 0)),
                   "strided": ((x, z(2, 24, 24, 128)[..., ::2], 0), (x, z(2, 12, 12, 128)[..., ::2], arg, 0)),
                   "cpu": ((x, dy.cpu(), 0), (x, dp, arg.cpu(), 0)),
                   "arg_dtype": ((x, dy.double(), 0), (x, dp, arg.int(), 0)),
                   "groups": ((x, dy, -1), (x, dp, arg, -1))}[case]
    with pytest.raises(RuntimeError):
        ops.f32_conv1_wgrad(*dense)
    with pytest.raises(RuntimeError):
        ops.f32_conv1_wgrad_pool(*pool)
