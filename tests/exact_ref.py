"""Integer oracle of the conv half of the CIFAR-10 CNN step: conv1 -> ReLU -> pool1 -> conv2 -> ReLU ->
pool2 forward (pooled values AND argmax bytes) and its backward (pool / ReLU backward through the
argmax bytes, the conv2 input gradient, both weight and bias gradients).  Plain torch on the CPU in
fp64, no project kernel.

Why integers: with small integer pixels, weights, biases and upstream gradients every value of the
step is an integer that bf16 holds exactly (|v| <= 256), every bf16 x bf16 product is exact in fp32
and every fp32 sum is exact while its partial sums stay below 2^24 -- whatever the summation order.
A correct kernel therefore reproduces this oracle bit for bit, element for element, argmax bytes
included, and small integers tie all the time, so the tie rule ("first maximum in the order d = 3 dy
+ dx") and the TF-SAME padding taps decide most windows instead of a handful.

Layouts: activations NHWC ([B, H, H, C]) as the kernels keep them, weights in the TF layout (HWIO) of
models/cifar_cnn.py.  Every function computes in fp64 (exact for these integers; the CPU tests also
feed them tie-free random reals to compare with autograd); ``as_int`` asserts that every result is an
integer and returns int64.
"""
import functools
import types

import torch
import torch.nn.functional as F

from dmlc.models import cifar_cnn as M

F64 = torch.float64
NO_GRAD = 255                                   # argmax byte of a window whose pooled value is 0


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _int(t):
    r = t.round()
    assert torch.equal(r, t), "not an integer tensor"
    return r.to(torch.int64)


def pool_first_argmax(y):
    """TF-SAME 3x3 stride-2 max pool of a post-ReLU map ``y`` [B, H, H, C] (H even, y >= 0): pad 0
    before and 1 after, a padded cell never wins, the winner is the FIRST maximum in the order
    d = 3 dy + dx, and the byte is 255 where the pooled value is 0 (no gradient: the ReLU mask).
    Returns (pooled [B, H/2, H/2, C], argmax bytes uint8, tie mask: a positive maximum reached by
    more than one real cell of the window)."""
    B, H, W, C = y.shape
    assert H == W and H % 2 == 0
    assert bool((y >= 0).all()), "pool_first_argmax takes the post-ReLU map"
    HO = H // 2
    ypad = F.pad(y, (0, 0, 0, 1, 0, 1), value=-1)            # the padded row / column: below every y
    taps = torch.stack([ypad[:, dy:dy + 2 * HO:2, dx:dx + 2 * HO:2, :] for dy in range(3) for dx in range(3)])
    pooled = taps.max(0).values
    eq = taps == pooled
    d = torch.arange(9).view(9, 1, 1, 1, 1)
    first = torch.where(eq, d, 9).min(0).values
    am = torch.where(pooled > 0, first, NO_GRAD).to(torch.uint8)
    tie = (eq.sum(0) > 1) & (pooled > 0)
    return pooled, am, tie


def pool_bwd_exact(dp, am, H):
    """Scatter the pooled gradient ``dp`` [B, H/2, H/2, C] through the argmax bytes to [B, H, H, C]
    (overlapping windows add; byte 255 passes nothing)."""
    B, HO, _, C = dp.shape
    assert H == 2 * HO
    out = torch.zeros(B, H + 1, H + 1, C, dtype=dp.dtype)
    for d in range(9):
        dy, dx = divmod(d, 3)
        out[:, dy:dy + H:2, dx:dx + H:2, :] += dp * (am == d)
    assert not bool(out[:, H].any()) and not bool(out[:, :, H].any()), "a padded cell won a window"
    return out[:, :H, :H, :].contiguous()


def _conv5x5(x, w, b):
    """SAME 5x5 convolution, x NHWC, w HWIO, fp64."""
    return _nhwc(F.conv2d(_nchw(x), w.permute(3, 2, 0, 1), b, padding=2)).contiguous()


def _wgrad5x5(x, dy):
    """dW[kh, kw, ci, co] = sum_{b, y, x} xpad[b, y + kh, x + kw, ci] dy[b, y, x, co] (HWIO)."""
    H = x.shape[1]
    xpad = F.pad(x, (0, 0, 2, 2, 2, 2))
    g = torch.zeros(5, 5, x.shape[3], dy.shape[3], dtype=F64)
    for kh in range(5):
        for kw in range(5):
            g[kh, kw] = torch.einsum("byxi,byxo->io", xpad[:, kh:kh + H, kw:kw + H, :], dy)
    return g


def crop(x_u8, cy, cx):
    return x_u8[:, cy:cy + 24, cx:cx + 24, :].to(F64)


def conv_fwd_exact(x_u8, cy, cx, w1, b1, w2, b2, as_int=True):
    """(y1, p1, am1, y2, p2, am2): the pre-ReLU conv outputs, the pooled maps and the argmax bytes of
    images ``x_u8`` [B, 32, 32, 3] cropped at (cy, cx)."""
    w1, b1, w2, b2 = (t.to(F64) for t in (w1, b1, w2, b2))
    y1 = _conv5x5(crop(x_u8, cy, cx), w1, b1)
    p1, am1, _ = pool_first_argmax(y1.clamp(min=0))
    y2 = _conv5x5(p1, w2, b2)
    p2, am2, _ = pool_first_argmax(y2.clamp(min=0))
    if as_int:
        y1, p1, y2, p2 = _int(y1), _int(p1), _int(y2), _int(p2)
    return y1, p1, am1, y2, p2, am2


def conv_bwd_exact(x_u8, cy, cx, w2, p1, am1, am2, dp2, as_int=True):
    """The conv backward for the pool2 gradient ``dp2`` [B, 6, 6, 64]: dy2 (pool2 / ReLU backward),
    dp1 (the conv2 input gradient), dY1 (pool1 / ReLU backward of dp1) and the weight / bias gradients
    gw1 [5,5,3,64], gb1, gw2 [5,5,64,64], gb2 (sums over the batch, TF layout).  ``partial_bound``:
    the largest sum of |x| |dy| over any weight-gradient element -- it bounds every partial sum of
    every summation order."""
    w2, p1, dp2 = w2.to(F64), p1.to(F64), dp2.to(F64)
    x = crop(x_u8, cy, cx)
    dy2 = pool_bwd_exact(dp2, am2, 12)
    # dp1[b, y, x, ci] = sum_{kh, kw, co} dy2[b, y - kh + 2, x - kw + 2, co] w2[kh, kw, ci, co]
    dp1 = _nhwc(F.conv2d(_nchw(dy2), w2.flip(0, 1).permute(2, 3, 0, 1), padding=2)).contiguous()
    dY1 = pool_bwd_exact(dp1, am1, 24)
    r = dict(dy2=dy2, dp1=dp1, dY1=dY1, gw1=_wgrad5x5(x, dY1), gb1=dY1.sum((0, 1, 2)),
             gw2=_wgrad5x5(p1, dy2), gb2=dy2.sum((0, 1, 2)))
    if as_int:
        r = {k: _int(v) for k, v in r.items()}
    r["partial_bound"] = float(max(_wgrad5x5(x.abs(), dY1.abs()).max(), _wgrad5x5(p1.abs(), dy2.abs()).max(),
                                   dY1.abs().sum((0, 1, 2)).max(), dy2.abs().sum((0, 1, 2)).max()))
    return r


# ---------------------------------------------------------------------------------------------------
# (batch, seed, cy, cx) of every case the GPU tests run (tests/test_cnn_exact_gpu.py); the CPU test
# checks the preconditions of each.  The crop offsets are the centre and the two extreme corners the
# bindings accept.
GPU_CASES = ((16, 1, 4, 4), (16, 2, 0, 8), (16, 3, 8, 0), (144, 4, 4, 4))
W2_DENSITY = 0.005        # conv2 taps that are +-1 (at 1 % a y2 of 265 occurred: not a bf16 integer)


def _pool_preconditions(name, y, p, am, tie):
    HO = p.shape[1]
    n = am.numel()
    assert float(tie.float().mean()) >= 0.02, f"{name}: fewer than 2 % tied windows"
    assert int((am == NO_GRAD).sum()) >= 0.05 * n, f"{name}: fewer than 5 % windows with code 255"
    for d in range(9):
        assert bool((am == d).any()), f"{name}: code {d} never wins"
    last_r, last_c = am[:, HO - 1], am[:, :, HO - 1]
    # the last real row / column (dy = 1 / dx = 1 of the last windows) wins somewhere ...
    assert bool(((last_r >= 3) & (last_r <= 5)).any()), f"{name}: no dy = 1 win in the last pooled row"
    assert bool(((last_c % 3 == 1) & (last_c != NO_GRAD)).any()), f"{name}: no dx = 1 win in the last pooled column"
    # ... and the padded row / column behind it never
    assert not bool(((last_r >= 6) & (last_r <= 8)).any()), f"{name}: a padded row won"
    assert not bool(((last_c % 3 == 2) & (last_c != NO_GRAD)).any()), f"{name}: a padded column won"
    assert bool((am[p == 0] == NO_GRAD).all()) and bool((am[p > 0] < 9).all())


@functools.lru_cache(maxsize=None)
def make_exact_case(B, seed, cy=4, cx=4):
    """Integer inputs of ``B`` images at crop (cy, cx), the oracle's forward and backward results for
    them, and the flat fp32 parameter buffer that carries the conv weights (the fc tensors keep the
    reference initialisation: the exact tests never run them).  Asserts, from the oracle alone, that
    the case is exact in bf16 / fp32 and that it exercises ties, the no-gradient code, every window
    position and the bottom / right border.  Cached: one oracle run per case, shared by every test
    (treat the result as read-only)."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
    data = ri(0, 3, B, 32, 32, 3).to(torch.uint8)
    w1 = ri(-1, 1, 5, 5, 3, 64)
    b1 = ri(-8, 2, 64)
    w2 = (torch.rand(5, 5, 64, 64, generator=g) < W2_DENSITY) * (2 * ri(0, 1, 5, 5, 64, 64) - 1)
    b2 = ri(-8, 2, 64)
    dp2 = ri(-3, 3, B, 6, 6, 64)
    y1, p1, am1, y2, p2, am2 = conv_fwd_exact(data, cy, cx, w1, b1, w2, b2)
    bwd = conv_bwd_exact(data, cy, cx, w2, p1, am1, am2, dp2)

    # --- preconditions (conditions on the inputs, from the oracle alone) ---------------------------
    for name, v in (("y1", y1), ("y2", y2), ("dy2", bwd["dy2"]), ("dp1", bwd["dp1"]), ("dY1", bwd["dY1"])):
        assert int(v.abs().max()) <= 256, f"{name} leaves the bf16 integers: {int(v.abs().max())}"
    assert bwd["partial_bound"] < 2 ** 24, f"a weight-gradient partial sum can reach {bwd['partial_bound']}"
    _pool_preconditions("pool1", y1, p1, am1, pool_first_argmax(y1.clamp(min=0))[2])
    _pool_preconditions("pool2", y2, p2, am2, pool_first_argmax(y2.clamp(min=0))[2])

    flat = M.init_flat_params(torch.Generator().manual_seed(seed))
    v = M.views(flat)
    for k, t in (("conv1_kernel", w1), ("conv1_bias", b1), ("conv2_kernel", w2), ("conv2_bias", b2)):
        v[k].copy_(t.to(torch.float32))
    return types.SimpleNamespace(B=B, cy=cy, cx=cx, data=data, labels=torch.zeros(B, dtype=torch.int32), flat=flat,
                                 w1=w1, b1=b1, w2=w2, b2=b2, y1=y1, p1=p1, am1=am1, y2=y2, p2=p2, am2=am2, dp2=dp2,
                                 **{k: bwd[k] for k in ("dy2", "dp1", "dY1", "gw1", "gb1", "gw2", "gb2")})
