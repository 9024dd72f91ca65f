"""The integer oracle of tests/exact_ref.py against brute force and fp64 autograd (CPU only), and the
preconditions of every case the GPU tests (tests/test_cnn_exact_gpu.py) feed the kernels."""
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
from dmlc.models import cifar_cnn as M

F64 = torch.float64


def _brute_pool(y):
    """The definition, cell by cell: first strict maximum over the real cells in the order d."""
    B, H, _, C = y.shape
    HO = H // 2
    p = torch.zeros(B, HO, HO, C, dtype=y.dtype)
    am = torch.zeros(B, HO, HO, C, dtype=torch.uint8)
    tie = torch.zeros(B, HO, HO, C, dtype=torch.bool)
    for b in range(B):
        for py in range(HO):
            for px in range(HO):
                for c in range(C):
                    best, arg, count = None, None, 0
                    for d in range(9):
                        yy, xx = 2 * py + d // 3, 2 * px + d % 3
                        if yy >= H or xx >= H:
                            continue                              # TF-SAME padding: never a candidate
                        v = float(y[b, yy, xx, c])
                        if best is None or v > best:
                            best, arg, count = v, d, 1
                        elif v == best:
                            count += 1
                    p[b, py, px, c] = best
                    am[b, py, px, c] = arg if best > 0 else 255
                    tie[b, py, px, c] = best > 0 and count > 1
    return p, am, tie


def test_pool_values_match_tf_same_maxpool():
    g = torch.Generator().manual_seed(0)
    y = torch.randint(0, 5, (3, 12, 12, 8), generator=g).to(F64)
    p, am, _ = X.pool_first_argmax(y)
    want = M.tf_same_maxpool_3x3s2(y.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert torch.equal(p, want)
    assert torch.equal(am == 255, want == 0)


def test_pool_bytes_match_brute_force_with_ties_and_zero_windows():
    g = torch.Generator().manual_seed(1)
    y = torch.randint(0, 3, (2, 8, 8, 4), generator=g)          # values 0..2: nearly every window ties
    y[0, 0:3, 0:3, :] = 0                                       # an all-zero window (code 255)
    y[0, 4:7, 4:7, 0] = 2                                       # a nine-way tie: code 0
    y[1, 6:8, 6:8, :] = 0
    y[1, 7, 7, :] = 2                                           # the corner window: only d = 4 can win
    y[1, 7, 2, 1] = 2                                           # last real row, d = 3 / 5 of two windows
    y[1, 6, 2, 1] = 2                                           # ... tied with the row above: d = 0 / 2 first
    p, am, tie = X.pool_first_argmax(y)
    bp, bam, btie = _brute_pool(y)
    assert torch.equal(p, bp) and torch.equal(am, bam) and torch.equal(tie, btie)
    assert bool((am[0, 0, 0] == 255).all()) and int(am[0, 2, 2, 0]) == 0 and bool((am[1, 3, 3] == 4).all())
    assert bool(tie.any()) and bool((am == 255).any())
    # the padded row / column never wins
    assert not bool(((am[:, 3] >= 6) & (am[:, 3] <= 8)).any())
    assert not bool(((am[:, :, 3] % 3 == 2) & (am[:, :, 3] != 255)).any())


def test_pool_bwd_matches_max_pool_autograd_on_tie_free_input():
    g = torch.Generator().manual_seed(2)
    y = torch.rand(2, 12, 12, 8, generator=g, dtype=F64) + 0.1   # positive reals: no tie, no code 255
    # (integer gradients: a cell that wins up to four windows sums them exactly in any order)
    dp = torch.randint(-9, 10, (2, 6, 6, 8), generator=g).to(F64)
    _, am, tie = X.pool_first_argmax(y)
    assert not bool(tie.any()) and not bool((am == 255).any())
    yn = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
    M.tf_same_maxpool_3x3s2(yn).backward(dp.permute(0, 3, 1, 2))
    assert torch.equal(X.pool_bwd_exact(dp, am, 12), yn.grad.permute(0, 2, 3, 1))


def test_conv_bwd_matches_fp64_autograd_of_the_model():
    """conv_fwd_exact / conv_bwd_exact against autograd through the conv part of M.cnn_forward (the same
    ops, fp64) on random reals: no ties, so autograd's max-pool routing is unambiguous."""
    g = torch.Generator().manual_seed(3)
    B, cy, cx = 3, 1, 7
    data = torch.randint(0, 256, (B, 32, 32, 3), dtype=torch.uint8, generator=g)
    w1 = (torch.randn(5, 5, 3, 64, generator=g, dtype=F64) * 0.02).requires_grad_(True)
    b1 = (torch.randn(64, generator=g, dtype=F64) * 0.5).requires_grad_(True)
    w2 = (torch.randn(5, 5, 64, 64, generator=g, dtype=F64) * 0.02).requires_grad_(True)
    b2 = (torch.randn(64, generator=g, dtype=F64) * 0.5).requires_grad_(True)
    dp2 = torch.randn(B, 6, 6, 64, generator=g, dtype=F64)
    # the conv part of M.cnn_forward, line for line, keeping p1
    x = X.crop(data, cy, cx).permute(0, 3, 1, 2)
    a1 = F.conv2d(x, w1.permute(3, 2, 0, 1), b1, padding=2)
    q1 = M.tf_same_maxpool_3x3s2(F.relu(a1))
    q1.retain_grad()
    a2 = F.conv2d(q1, w2.permute(3, 2, 0, 1), b2, padding=2)
    a2.retain_grad()
    q2 = M.tf_same_maxpool_3x3s2(F.relu(a2))
    q2.backward(dp2.permute(0, 3, 1, 2))

    with torch.no_grad():
        y1, p1, am1, y2, p2, am2 = X.conv_fwd_exact(data, cy, cx, w1, b1, w2, b2, as_int=False)
        r = X.conv_bwd_exact(data, cy, cx, w2, p1, am1, am2, dp2, as_int=False)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-11, atol=1e-11)     # fp64 summation order only
    assert close(y1, nhwc(a1)) and close(p1, nhwc(q1)) and close(y2, nhwc(a2)) and close(p2, nhwc(q2))
    assert bool((am2 == 255).any()) and bool((am1 < 9).any())
    assert close(r["dy2"], nhwc(a2.grad)) and close(r["dp1"], nhwc(q1.grad))
    assert close(r["gw1"], w1.grad) and close(r["gb1"], b1.grad)
    assert close(r["gw2"], w2.grad) and close(r["gb2"], b2.grad)
    assert r["gw1"].abs().max() > 1 and r["gw2"].abs().max() > 1e-3


@pytest.mark.parametrize("B,seed,cy,cx", X.GPU_CASES)
def test_gpu_cases_meet_their_preconditions(B, seed, cy, cx):
    """make_exact_case asserts them itself; here also that the flat buffer carries the integer weights
    and that the case is what the GPU tests expect (shapes, value ranges, a gradient to compare)."""
    c = X.make_exact_case(B, seed, cy, cx)
    v = M.views(c.flat)
    assert torch.equal(v["conv1_kernel"].double(), c.w1.double()) and torch.equal(v["conv2_bias"].double(), c.b2.double())
    assert torch.equal(v["conv2_kernel"].to(torch.bfloat16).double(), c.w2.double())
    assert c.data.dtype == torch.uint8 and int(c.data.max()) == 3 and tuple(c.data.shape) == (B, 32, 32, 3)
    assert tuple(c.am1.shape) == (B, 12, 12, 64) and tuple(c.am2.shape) == (B, 6, 6, 64)
    assert tuple(c.gw1.shape) == (5, 5, 3, 64) and tuple(c.gw2.shape) == (5, 5, 64, 64)
    assert int(c.dp2.abs().max()) == 3 and bool(c.dy2.any()) and bool(c.dp1.any()) and bool(c.gw1.any())
    # every value the kernels store as bf16 survives the round trip
    for t in (c.p1, c.p2, c.dy2, c.dp1, c.dY1):
        assert torch.equal(t.to(torch.bfloat16).to(torch.int64), t)
    for t in (c.gw1, c.gb1, c.gw2, c.gb2):
        assert torch.equal(t.to(torch.float32).to(torch.int64), t)
