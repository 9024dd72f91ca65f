"""ReLU + pool and loss-head kernels of the fp32 step (csrc/kernels/f32_pool.hip, ops/f32.py relu_pool /
xent_head): exact against float64 CPU autograd of the PyTorch expressions on integer data, the tie rule,
the loss head at the fp32 bound, and the whole model fused against unfused, eager against captured."""
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


def _pool_ref(y, dp):
    """(p, dy) of pool(relu(y)) by float64 CPU autograd."""
    y64 = y.cpu().double().requires_grad_()
    p = F.max_pool2d(torch.relu(y64).permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1)
    p.backward(dp.cpu().double())
    return p.detach(), y64.grad


def _first_max(z):
    return torch.where(z == z.max(1, keepdim=True).values, torch.arange(z.shape[1]), z.shape[1]).min(1).values


# blocks > 0: fewer workgroups than units (4 per image at H = 24, 1 at H = 12), so each loops over several
@pytest.mark.parametrize("B,H,blocks", [(1, 24, 0), (3, 24, 0), (1, 12, 0), (3, 12, 0), (5, 24, 3), (5, 12, 2)])
def test_relu_pool_is_exact(B, H, blocks):
    ops, HO = _ops(), H // 2
    g = torch.Generator().manual_seed(100 * H + B)
    # every (image, channel) plane is a permutation of -H*H/2 .. H*H/2 - 1: no ties, about half the windows masked
    planes = torch.stack([torch.randperm(H * H, generator=g) for _ in range(B * 64)]) - H * H // 2
    y = planes.view(B, 64, H, H).permute(0, 2, 3, 1).float().contiguous().cuda()
    dp = torch.randint(-4, 5, (B, HO, HO, 64), generator=g).float().cuda()
    p, arg = ops.f32_relu_pool_fwd(y, blocks)
    dy = ops.f32_relu_pool_bwd(dp, arg, blocks)
    p_ref, dy_ref = _pool_ref(y, dp)
    assert torch.equal(p.cpu().double(), p_ref)
    assert torch.equal(dy.cpu().double(), dy_ref)
    a = arg.cpu().long()
    keep = a != 255
    assert torch.equal(~keep, p_ref == 0)
    b, i, j, c = torch.meshgrid(torch.arange(B), torch.arange(HO), torch.arange(HO), torch.arange(64), indexing="ij")
    picked = y.cpu()[b[keep], (2 * i + a // 3)[keep], (2 * j + a % 3)[keep], c[keep]]     # out of range: IndexError
    assert torch.equal(picked, p.cpu()[keep])


@pytest.mark.parametrize("H", [24, 12])
def test_relu_pool_ties_go_to_the_first_tap(H):
    ops = _ops()
    g = torch.Generator().manual_seed(H)
    y = (1 + torch.arange(64.0)).expand(2, H, H, 64).contiguous().cuda()          # constant positive planes
    dp = torch.randint(-4, 5, (2, H // 2, H // 2, 64), generator=g).float().cuda()
    p, arg = ops.f32_relu_pool_fwd(y, 0)
    assert int(arg.max()) == 0
    p_ref, dy_ref = _pool_ref(y, dp)                                             # PyTorch's CPU pool: first index too
    assert torch.equal(p.cpu().double(), p_ref)
    assert torch.equal(ops.f32_relu_pool_bwd(dp, arg, 0).cpu().double(), dy_ref)


@pytest.mark.parametrize("relu_logits", [False, True])
@pytest.mark.parametrize("B", [1, 3, 100])
def test_xent_head_matches_fp64(B, relu_logits):
    """Measured on an MI355X: loss within 9.5e-8, dlogits within 1.2e-7 of float64 over the six cases."""
    from dmlc.ops.f32 import xent_head
    g = torch.Generator().manual_seed(B)
    logits = (3 * torch.randn(B, 10, generator=g)).cuda().requires_grad_()
    labels = torch.randint(0, 10, (B,), generator=g, dtype=torch.int64 if B == 3 else torch.int32).cuda()
    loss, hits = xent_head(logits, labels, relu_logits)
    loss.backward()
    l64 = logits.detach().cpu().double().requires_grad_()
    z = torch.relu(l64) if relu_logits else l64
    ref = F.cross_entropy(z, labels.cpu().long())
    ref.backward()
    e_loss = abs(float(loss.detach()) - float(ref.detach())) / abs(float(ref.detach()))
    e_grad = _rel(logits.grad.cpu(), l64.grad)
    print(f"xent_head B={B} relu={relu_logits}: loss rel {e_loss:.3g}, dlogits rel {e_grad:.3g}")
    assert e_loss < 1e-4 and e_grad < 1e-4          # the fp32 bound of tests/test_f32_gpu.py against float64
    assert int(hits) == int((_first_max(z.detach()) == labels.cpu()).sum())


@pytest.mark.parametrize("relu_logits,expect", [(True, 3), (False, 2)])
def test_xent_head_hit_count_takes_the_first_maximum(relu_logits, expect):
    rows = [([2, 2, 1], 0), ([2, 2, 1], 1), ([0, 3, 3], 1), ([0, 3, 3], 2), ([-2, -1, -1], 0)]   # last: relu -> all 0
    logits = torch.tensor([r + [min(r) - 1] * 7 for r, _ in rows], dtype=torch.float32).cuda()
    labels = torch.tensor([l for _, l in rows], dtype=torch.int32).cuda()
    assert int(_ops().f32_xent_head(logits, labels, relu_logits)[1]) == expect


@pytest.mark.parametrize("B", [2, 20])
def test_model_fused_matches_unfused(B):
    """Measured on an MI355X: flat gradient fused vs unfused 0 (B = 2) and 5.1e-8 (B = 20) relative."""
    flat = M.init_flat_params(torch.Generator().manual_seed(B))
    g = torch.Generator().manual_seed(B + 1)
    x = torch.randint(0, 256, (B, 24, 24, 3), generator=g).float().cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    fused = M.CifarCNN(flat, backend="hip_f32", fused=True).cuda()
    plain = M.CifarCNN(flat, backend="hip_f32", fused=False).cuda()
    assert torch.equal(fused(x).detach(), plain(x).detach())
    F.cross_entropy(plain(x), y).backward()
    grads = []
    for _ in range(2):
        fused.flat.grad = None
        loss, hits = fused.loss_and_hits(x, y)
        loss.backward()
        grads.append(fused.flat.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert int(hits) == int((_first_max(plain(x).detach().cpu()) == y.cpu()).sum())
    print(f"fused vs unfused flat gradient, B={B}: rel {_rel(grads[0], plain.flat.grad):.3g}")
    assert _rel(grads[0], plain.flat.grad) < 1e-6


def test_captured_fused_step_equals_the_eager_step():
    from dmlc.engine.eager import EagerTrainer
    g = torch.Generator().manual_seed(7)
    data = torch.randint(0, 256, (128, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (128,), dtype=torch.int32, generator=g)
    tr = EagerTrainer("cifar_cnn", 16, data, labels, device="cuda", dtype="fp32", seed=3, lr=1e-4, graph=True,
                      backend="hip_f32")
    for _ in range(3):                                  # warm-up steps; the third one captures
        tr.step()
    assert tr.graph is not None and tr.model.fused
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
