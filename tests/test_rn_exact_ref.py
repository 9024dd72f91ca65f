"""The ResNet-20 oracle of tests/rn_exact_ref.py against fp64 autograd through models/resnet.py's own
expressions (CPU only), its shadow layouts against their index formulas, and the construction and the
preconditions of every case the GPU tests (tests/test_rn_exact_gpu.py) feed the kernels."""
import pytest
import torch
import torch.nn.functional as F

import rn_exact_ref as X
from dmlc.engine import fused_resnet as E
from dmlc.models import resnet as R

F64 = torch.float64
ATOL = 1e-10


def _close(a, b):
    return torch.allclose(a, b, rtol=0, atol=ATOL)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _option_a(x_nchw, mode, cin, wdt):
    """The shortcut expression of models/resnet.py resnet20_forward (option A)."""
    if mode == 1:
        return x_nchw
    return F.pad(x_nchw[:, :, ::2, ::2], (0, 0, 0, 0, 0, wdt - cin))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout", [(3, 5), (8, 6)])
def test_conv_and_its_gradients_match_autograd(cin, cout, stride):
    g = torch.Generator().manual_seed(10 * cin + stride)
    B, H = 3, 8
    x = torch.randn(B, H, H, cin, generator=g, dtype=F64, requires_grad=True)
    w = torch.randn(3, 3, cin, cout, generator=g, dtype=F64, requires_grad=True)
    gz = torch.randn(B, H // stride, H // stride, cout, generator=g, dtype=F64)
    z = _nhwc(R._conv3x3(_nchw(x), w, stride))
    z.backward(gz)
    with torch.no_grad():
        assert _close(X.conv3x3(x, w, stride), z)
        assert _close(X.conv3x3_dgrad(gz, w, stride), x.grad)
        per_img = X.conv3x3_wgrad(x, gz, stride)
        assert tuple(per_img.shape) == (B, 9, max(cin, 8), cout)
        assert _close(per_img.sum(0)[:, :cin].reshape(3, 3, cin, cout), w.grad)
        assert not bool(per_img[:, :, cin:].any())
        # the slab row order k = tap * CINP + ci, and grouping by b0 = grp * B / G
        slabs = X.wgrad_exact(x, gz, stride)
        assert torch.equal(slabs[1, 5 * max(cin, 8) + 2], per_img[1, 5, 2])
        assert _close(X.slab_sums(slabs, 2)[1], slabs[1:].sum(0)) and _close(X.slab_sums(slabs, 2)[0], slabs[0])
    assert float(w.grad.abs().max()) > 1 and float(x.grad.abs().max()) > 1


def test_bn_forward_and_backward_formulas_match_autograd():
    g = torch.Generator().manual_seed(3)
    B, H, C = 4, 6, 5
    N = B * H * H
    z = (torch.randn(B, H, H, C, generator=g, dtype=F64) * 2 + 1).requires_grad_(True)
    gamma = (torch.randn(C, generator=g, dtype=F64) + 0.3).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=F64).requires_grad_(True)
    gy = torch.randn(B, H, H, C, generator=g, dtype=F64)
    y = _nhwc(F.batch_norm(_nchw(z), None, None, gamma, beta, training=True, eps=R.BN_EPS))
    y.backward(gy)
    with torch.no_grad():
        stat = (z.sum((0, 1, 2)), (z * z).sum((0, 1, 2)))
        mean, rstd, A, _, _ = X.bn_coeffs(stat, None, gamma, N)
        sc = gamma * rstd
        assert _close(z * sc + (beta - mean * sc), y)
        xhat = (z - mean) * rstd
        red = (gy.sum((0, 1, 2)), (gy * xhat).sum((0, 1, 2)))
        _, _, A, Bc, Cc = X.bn_coeffs(stat, red, gamma, N)
        assert _close(A * gy + Bc * z + Cc, z.grad)
        assert _close(red[1], gamma.grad) and _close(red[0], beta.grad)       # dgamma == R2, dbeta == R1


@pytest.mark.parametrize("mode", [1, 2])
def test_shortcut_and_its_gradient_match_the_option_a_expression(mode):
    g = torch.Generator().manual_seed(mode)
    B, H, cin = 2, 8, 4
    wdt = cin if mode == 1 else 2 * cin
    src = torch.randn(B, H, H, cin, generator=g, dtype=F64, requires_grad=True)
    out = _nhwc(_option_a(_nchw(src), mode, cin, wdt))
    gsc = torch.randn(out.shape, generator=g, dtype=F64)
    out.backward(gsc)
    with torch.no_grad():
        assert torch.equal(X.shortcut(src, mode), out)
        assert torch.equal(X.shortcut_grad(gsc, mode), src.grad)
        if mode == 2:
            assert not bool(X.shortcut(src, mode)[..., cin:].any())
            assert not bool(src.grad[:, 1::2].any()) and not bool(src.grad[:, :, 1::2].any())


@pytest.mark.parametrize("stride,fsc,bsc", [(1, 0, 0), (1, 1, 1), (1, 2, 1), (2, 1, 2)])
def test_one_layer_forward_and_backward_match_autograd(stride, fsc, bsc):
    """fwd_exact, dgrad_exact and wgrad_exact chained as the engine chains the launches, with the
    statistics computed from the data: a = relu(bn(z_prev) + shortcut(src)), z = conv(a), y = bn(z), and
    the block shortcut that leaves ``a`` (backward mode ``bsc``), against autograd."""
    g = torch.Generator().manual_seed(7 + stride + 3 * fsc)
    B, H, cin, cout = 3, 8, 8, 6
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    z_prev = (rn(B, H, H, cin) + 0.5).requires_grad_(True)
    gam_p, bet_p = (rn(cin) + 0.2).requires_grad_(True), rn(cin).requires_grad_(True)
    src = None if fsc == 0 else (rn(B, H, H, cin) if fsc == 1 else rn(B, 2 * H, 2 * H, cin // 2))
    w = rn(3, 3, cin, cout).requires_grad_(True)
    gam = (rn(cout) + 0.2).requires_grad_(True)
    ho = H // stride
    gy = rn(B, ho, ho, cout)
    gy_sc = None if bsc == 0 else (rn(B, H, H, cin) if bsc == 1 else rn(B, H // 2, H // 2, 2 * cin))

    pre = F.batch_norm(_nchw(z_prev), None, None, gam_p, bet_p, training=True, eps=R.BN_EPS)
    if fsc:
        pre = pre + _option_a(_nchw(src), fsc, cin // 2 if fsc == 2 else cin, cin)
    pre.retain_grad()
    a = F.relu(pre)
    z = R._conv3x3(a, w, stride)
    z.retain_grad()
    y = F.batch_norm(z, None, None, gam, torch.zeros(cout, dtype=F64), training=True, eps=R.BN_EPS)
    loss = (_nhwc(y) * gy).sum()
    if bsc:
        loss = loss + (_nhwc(_option_a(a, bsc, cin, cin if bsc == 1 else 2 * cin)) * gy_sc).sum()
    loss.backward()

    with torch.no_grad():
        Np, N = B * H * H, B * ho * ho
        stat_p = (z_prev.sum((0, 1, 2)), (z_prev ** 2).sum((0, 1, 2)))
        mean_p, rstd_p, _, _, _ = X.bn_coeffs(stat_p, None, gam_p, Np)
        a_out, zz, s1, s2 = X.fwd_exact(w, stride, B, z_prev=z_prev, mean=mean_p, rstd=rstd_p, gamma=gam_p, beta=bet_p,
                                        sc_src=src, sc_mode=fsc)
        assert _close(a_out, _nhwc(a)) and _close(zz, _nhwc(z))
        xhat = (zz - s1 / N) * X.bn_coeffs((s1, s2), None, gam, N)[1]
        red = (gy.sum((0, 1, 2)), (gy * xhat).sum((0, 1, 2)))
        _, _, A, Bc, Cc = X.bn_coeffs((s1, s2), red, gam, N)
        g_z, gy_prev, R1, R2 = X.dgrad_exact(gy, zz, A, Bc, Cc, w, stride, a_out, z_prev, mean_p, rstd_p, gy_sc, bsc, B)
        assert _close(g_z, _nhwc(z.grad))
        assert _close(gy_prev, _nhwc(pre.grad))
        assert _close(R2, gam_p.grad) and _close(R1, bet_p.grad)
        slabs = X.wgrad_exact(a_out, g_z, stride)
        assert _close(slabs.sum(0).reshape(3, 3, cin, cout), w.grad)
    assert float(pre.grad.abs().max()) > 0.1 and bool((a_out == 0).any())


def test_padding_images_leave_statistics_and_gradients_alone():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 4, 4, 8, generator=g, dtype=F64)
    w = torch.randn(3, 3, 8, 8, generator=g, dtype=F64)
    _, z, s1, s2 = X.fwd_exact(w, 1, 2, x=x)
    assert _close(s1, z[:2].sum((0, 1, 2))) and _close(s2, (z[:2] ** 2).sum((0, 1, 2))) and bool(z[2:].any())
    gz = X.gz_exact(torch.ones(4, 4, 4, 8), z, torch.ones(8, dtype=F64), torch.ones(8, dtype=F64), torch.ones(8, dtype=F64), 2)
    assert not bool(gz[2:].any()) and bool(gz[:2].any())


@pytest.mark.parametrize("cin,cout", [(3, 16), (16, 32), (64, 64)])
def test_shadow_layouts_follow_their_index_formulas(cin, cout):
    """A weight tensor whose every element is distinct: each shadow element is found by the header's
    formula (fwd k = tap * CINP + ci; dgrad k' = (8 - tap) * COUT + co), every other column is zero."""
    w = torch.arange(1, 9 * cin * cout + 1, dtype=F64).reshape(3, 3, cin, cout)
    wf, wd = X.shadow_fwd(w), X.shadow_dgrad(w)
    cp, KP, KPD = max(cin, 8), (9 * max(cin, 8) + 31) // 32 * 32, (9 * cout + 31) // 32 * 32
    assert tuple(wf.shape) == (cout, KP) and tuple(wd.shape) == (cin, KPD)
    seen_f, seen_d = torch.zeros_like(wf, dtype=torch.bool), torch.zeros_like(wd, dtype=torch.bool)
    for kh in range(3):
        for kw in range(3):
            tap = 3 * kh + kw
            for ci in range(cin):
                k = tap * cp + ci
                assert torch.equal(wf[:, k], w[kh, kw, ci, :])
                seen_f[:, k] = True
                kd = (8 - tap) * cout
                assert torch.equal(wd[ci, kd:kd + cout], w[kh, kw, ci, :])
                seen_d[ci, kd:kd + cout] = True
    assert not bool(wf[~seen_f].any()) and not bool(wd[~seen_d].any())
    assert int(seen_f.sum()) == 9 * cin * cout == int(seen_d.sum())
    assert (KP, KPD) == (E._kp(cin), E._kpd(cout))


def _check_slots(slots, totals, C, N, mean, rstd):
    """The fixed-point encoding decodes to the intended totals, is really spread (slots, fraction
    carry), and both the fp64 and the float emulation of bn_mean_rstd give the intended values."""
    dec = E.fx_decode(slots)
    assert torch.equal(dec, X.fx_total(slots))
    for k in range(2):
        want = totals[k]
        assert torch.allclose(dec[64 * k:64 * k + C], want, rtol=1e-15, atol=0), (dec[64 * k:64 * k + C] - want).abs().max()
    assert not bool(dec[C:64].any()) and not bool(dec[64 + C:].any())
    assert int((slots[:, :C] != 0).sum()) > 4 * C and bool((slots[:, 128:128 + C].sum(0) >= 2 ** 48).any())
    inv_n = 1.0 / N
    assert float(torch.tensor(inv_n, dtype=torch.float32)) == inv_n, "N is not a power of two"
    if mean is None:
        return
    m32, r32 = X.emulate_mean_rstd(slots, C, inv_n)
    assert torch.equal(m32.double(), mean) and torch.equal(r32.double(), rstd)
    m64, r64, _, _, _ = X.bn_coeffs((dec[:C], dec[64:64 + C]), None, torch.ones(C), N)
    assert torch.equal(m64, mean) and float((r64 - rstd).abs().max()) < 1e-11
    for eps in (-1e-9, 1e-9):                    # robust against the rounding of the device's sqrt / divide
        var = (dec[64:64 + C] * inv_n - m64 * m64) * (1 + eps)
        assert torch.equal((1.0 / torch.sqrt(var + X.BN_EPS)).float().double(), rstd)
    assert set(rstd.tolist()) == {1.0, 2.0}


@pytest.mark.parametrize("case", X.GPU_CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1])) if c[1] else 'head'}-nv{c[4]}-sc{c[5]}")
def test_gpu_cases_meet_their_preconditions(case):
    """make_case asserts the value-range preconditions itself; here the construction: the slots decode
    to the intended totals, the emulated bn_mean_rstd gives exactly the intended mean and rstd, the
    coefficients are integers, and every stored tensor survives its bf16 / fp32 round trip."""
    kind, geom, seed, B, nvalid, sc_mode = case
    c = X.make_case(*case)
    assert B == 16 and c.B == 16
    if kind == "head":
        _check_slots(c.stat, c.stat_totals, 64, nvalid * 64, c.mean, c.rstd)
        assert torch.equal(c.labels64[c.idx.long()].long(), c.labels)
        assert c.idx.unique().numel() == B and not torch.equal(c.idx, torch.arange(B, dtype=torch.int32))
        assert torch.equal(c.o.logits * 64, c.logits64.double())
        assert torch.equal(c.o.logits.float().double(), c.o.logits)
        assert not bool(c.o.gy[nvalid:].any()) and not bool(c.o.loss[nvalid:].any()) and not bool(c.o.dW[nvalid:].any())
        return
    cin, cout, hin, stride = geom
    hout = hin // stride
    bf = lambda t: torch.equal(t.to(torch.bfloat16).to(torch.int64), t.to(torch.int64))
    if kind == "fwd":
        if cin > 3:
            _check_slots(c.stat_prev, c.stat_prev_totals, cin, nvalid * hin * hin, c.mean, c.rstd)
            sc = c.gamma.double() * c.rstd
            assert torch.equal(sc, sc.round()) and int(sc.abs().max()) <= 4 and bool((c.gamma < 0).any())
            assert bf(c.a_out) and tuple(c.a_out.shape) == (B, hin, hin, cin)
            assert (c.sc_src is None) == (sc_mode == 0)
        else:
            assert c.idx.unique().numel() == B and c.data.shape[0] == 64
        assert bf(c.z) and tuple(c.z.shape) == (B, hout, hout, cout)
        assert torch.equal(c.s1, c.z[:nvalid].sum((0, 1, 2))) and torch.equal(c.s2, (c.z[:nvalid] ** 2).sum((0, 1, 2)))
        return
    _check_slots(c.stat, c.stat_totals, cout, nvalid * hout * hout, c.mean, c.rstd)
    _check_slots(c.red, c.red_totals, cout, nvalid * hout * hout, None, None)
    assert bf(c.g_z) and bool((c.gamma < 0).any())
    assert not bool(c.gy[nvalid:].any()) and not bool(c.g_z[nvalid:].any())
    assert torch.equal(c.slabs.float().to(torch.int64), c.slabs) and tuple(c.slabs.shape) == (B, 9 * max(cin, 8), cout)
    for G in (16, 8, 3):
        assert torch.equal(X.slab_sums(c.slabs, G).sum(0), c.slabs.sum(0))
    if cin > 3:
        _check_slots(c.stat_prev, c.stat_prev_totals, cin, nvalid * hin * hin, c.mean_prev, c.rstd_prev)
        assert bf(c.gy_prev) and (c.gy_sc is None) == (sc_mode == 0)
        if sc_mode == 2:
            assert tuple(c.gy_sc.shape) == (B, hin // 2, hin // 2, 2 * cin) and bool(c.gy_sc[..., cin:].any())


def test_gpu_pair_tables_equal_the_engines_layers():
    """The (geometry, shortcut mode) pairs of the GPU tests are exactly those the engine launches: the
    wiring its per-layer launchers read from the plan (engine/plan_resnet.py fwd_sc / bwd_sc)."""
    from dmlc.engine.plan_resnet import plan_resnet_step
    plan = plan_resnet_step(batch_size=16)
    fwd = {(tuple(L[1:5]), plan.fwd_sc[l][0]) for l, L in enumerate(E.LAYERS)}
    bwd = {(tuple(L[1:5]), plan.bwd_sc[l]) for l, L in enumerate(E.LAYERS) if l > 0}
    assert fwd == set(X.FWD_PAIRS) and len(X.FWD_PAIRS) == len(fwd) == 11
    assert bwd == set(X.BWD_PAIRS) and len(X.BWD_PAIRS) == len(bwd) == 8
    assert {tuple(L[1:5]) for L in E.LAYERS} == set(X.GEOMS)
    ran = {(c[0], c[1], c[5]) for c in X.GPU_CASES if c[4] == 16}
    assert {("fwd", g, m) for g, m in X.FWD_PAIRS} <= ran and {("bwd", g, m) for g, m in X.BWD_PAIRS} <= ran
    assert all(((g, X.BWD_DEFAULT_MODE[g]) in X.BWD_PAIRS) for g in X.GEOMS[1:])
